"""The sharded degree check with one rank per PROCESS: world 2 at n = 128, two processes on the one test GPU over the
host-exchange communicator (tests/shard_degrees_worker.py; the scaffold of tests/test_sharded_multiprocess.py), the
switch on at rank 1 only.  Both ranks return the same status, message and merged report for the zero-last-row trace and
the same proof bytes for the random-last-row one.  One case: the loopback tests cover the rest."""
import json
import socket
import subprocess
import sys
from pathlib import Path

import pytest

from degrees_ref import ZK_ERR_DEGREES, ZK_OK, expected, make_report, message, pushadd_zero_last_row

WORKER = Path(__file__).resolve().parent / "shard_degrees_worker.py"
WORLD, N = 2, 128


@pytest.mark.gpu
def test_two_processes_agree_on_the_degree_check(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, "-u", str(WORKER), str(r), str(WORLD), port, str(tmp_path)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(WORLD)]
    logs = []
    try:
        for p in procs:  # each child under its own time limit
            logs.append(p.communicate(timeout=120)[0])
    finally:
        for p in procs:  # only the processes started here
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{logs[r] if r < len(logs) else ''}"
    res = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(WORLD)]
    want = make_report(N, pushadd_zero_last_row(N), sum(1 << k for k in (4, 5, 6, 7, 9, 10)))
    for x in res:
        z = x["zero"]
        assert z["rc"] == ZK_ERR_DEGREES and z["msg"] == message(want) and z["proof_len"] == 0
        assert z["degrees"] == want and z["exchanges"] == ["control", "degrees_report", "degrees_slices"]
        assert z["agreement"]["validate_degrees"] == 1 and z["agreement"]["control_calls"] == 2
        g = x["good"]
        assert g["rc"] == ZK_OK and g["proof_len"] > 0 and g["degrees"] == make_report(N, expected(N), 0)
        assert "degrees_slices" in g["exchanges"] and "openings" in g["exchanges"]
    assert res[0]["zero"] == res[1]["zero"]
    assert res[0]["good"]["sha256"] == res[1]["good"]["sha256"]
