"""Two processes, one rank each on the one test GPU, whose sharded proof is given inputs, switches or prover histories
that DIFFER between the ranks (tests/agree_worker.py; zk_comm_create_host over a TCP host group with a 20 s timeout).
Before the agreement such ranks issued collectives of different sizes or counts and waited on each other; now every
rank learns the same outcome from one control exchange: a named field, a named rank, or decisions all ranks follow.
The `lr` golden case (n = 128) throughout; the detection and hint cases add a 2^13-row trace, the shortest kind for
which the library builds a column detector at all (its pin: the single-GPU proof each rank computes first).
Each case starts its two processes once."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

from zkvm_amd import native

pytestmark = pytest.mark.gpu
WORKER = Path(__file__).resolve().parent / "agree_worker.py"
WORLD = 2


def run_case(out, case, env1=None):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    envs = [dict(os.environ), {**os.environ, **(env1 or {})}]
    procs = [subprocess.Popen([sys.executable, "-u", str(WORKER), str(r), str(WORLD), port, str(out), case],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=envs[r])
             for r in range(WORLD)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=120)[0])
    finally:
        for p in procs:  # only the processes started here
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{logs[r] if r < len(logs) else ''}"
    res = [json.loads((out / f"rank{r}.json").read_text()) for r in range(WORLD)]
    steps = [{s["name"]: s for s in x["steps"]} for x in res]
    for r in range(WORLD):
        steps[r]["single"] = res[r].get("single")
    return steps, res[0]["golden"]


def check_disagreement(steps, golden, field):
    a, b = steps[0]["differ"], steps[1]["differ"]
    assert a["rc"] == b["rc"] == native.ZK_ERR_INVALID_ARG
    assert a["msg"] == b["msg"] and field in a["msg"] and "rank 0: " in a["msg"] and "rank 1: " in a["msg"]
    for x in (a, b):
        ag = x["agreement"]
        assert ag["code"] == native.ZK_ERR_INVALID_ARG and (ag["rank_a"], ag["rank_b"]) == (0, 1)
        assert ag["control_calls"] == 1 and ag["control_bytes"] == 256 and ag["field"].startswith(field)
        assert x["exchanges"] == ["control"]  # nothing else ran
    # the same two processes, the same communicator and provers, equal inputs: the proof as always
    for x in (steps[0]["equal"], steps[1]["equal"]):
        assert x["rc"] == 0 and x["sha256"] == golden and x["agreement"]["code"] == 0
        assert "control" in x["exchanges"] and "openings" in x["exchanges"]


def test_ranks_with_different_options(tmp_path):
    steps, golden = run_case(tmp_path, "options")
    check_disagreement(steps, golden, "options.num_queries")
    assert steps[0]["differ"]["msg"].endswith("(rank 0: 32, rank 1: 31)")


def test_ranks_with_different_public_inputs(tmp_path):
    steps, golden = run_case(tmp_path, "pub_inputs")
    check_disagreement(steps, golden, "public inputs")


def test_a_rank_whose_prover_is_too_small(tmp_path):
    steps, _ = run_case(tmp_path, "small_prover")
    a, b = steps[0]["refused"], steps[1]["refused"]
    # rank 1: its own refusal, code and text as a single-process call gives them; rank 0: the peer, named
    assert b["rc"] == native.ZK_ERR_INVALID_ARG and "rank" not in b["msg"] and b["msg"]
    assert a["rc"] == native.ZK_ERR_PEER and a["msg"] == f"rank 1 refused the proof: -1: {b['msg']}"
    for x in (a, b):
        assert x["agreement"]["code"] == native.ZK_ERR_PEER and x["agreement"]["rank_a"] == 1
        assert x["exchanges"] == ["control"]


def test_one_rank_with_column_detection_switched_off(tmp_path):
    steps, golden = run_case(tmp_path, "sparse_off", env1={"ZK_SPARSE": "0"})
    assert steps[0]["single"] and steps[0]["single"] == steps[1]["single"]
    for r in range(WORLD):
        for name, want in (("device", golden), ("big_device", steps[0]["single"])):
            x = steps[r][name]
            assert x["rc"] == 0 and x["sha256"] == want
            assert x["agreement"]["code"] == 0 and x["agreement"]["detect"] == 0
            assert "column_flags" not in x["exchanges"]  # issued by every rank or by none


def test_one_rank_with_a_new_prover(tmp_path):
    steps, golden = run_case(tmp_path, "new_prover")
    assert steps[0]["single"] and steps[0]["single"] == steps[1]["single"]
    for r in range(WORLD):
        s = steps[r]
        want = s.pop("single")
        assert all(s[k]["rc"] == 0 and s[k]["sha256"] == want for k in ("first", "second", "third", "fourth", "fifth"))
        assert s["lr"]["rc"] == 0 and s["lr"]["sha256"] == golden
        assert s["first"]["agreement"]["detect"] == 1 and "column_flags" in s["first"]["exchanges"]
        assert s["first"]["agreement"]["hints"] == 0 and s["first"]["agreement"]["hints_equal"] == 1
        assert s["second"]["agreement"]["hints"] == 1 and s["second"]["info"]["hinted_sparse"] != 0
        # rank 1's prover is new: the sets differ, every rank proves without hints, and nothing is redone
        assert s["third"]["agreement"]["hints"] == 0 and s["third"]["agreement"]["hints_equal"] == 0
        assert s["third"]["info"]["hinted_sparse"] == 0 and s["third"]["info"]["derived"] == 0
        assert s["fourth"]["agreement"]["hints"] == 1
        assert s["fifth"]["agreement"]["hints"] == 1 and s["fifth"]["info"]["hinted_sparse"] != 0
        assert s["fifth"]["info"]["hinted_sparse"] == s["second"]["info"]["hinted_sparse"]
        assert all(s[k]["info"]["hint_redos"] == 0 for k in s)


def test_validate_on_at_one_rank_only(tmp_path):
    steps, golden = run_case(tmp_path, "validate")
    a, b = steps[0]["broken"], steps[1]["broken"]
    n = 128
    want = f"main transition constraint 0 did not evaluate to ZERO at step {n // 2 - 1}; 2 failing steps, 0 failed assertions"
    for x in (a, b):
        assert x["rc"] == native.ZK_ERR_TRACE and x["msg"] == want and x["proof_len"] == 0
        assert x["agreement"]["validate"] == 1 and x["agreement"]["control_calls"] == 2
        assert x["exchanges"] == ["control", "validate_report"]
        v = x["validation"]
        assert v["t_count"][0] == 2 and v["t_first"][0] == n // 2 - 1 and v["failing_steps"] == 2
    assert a["validation"] == b["validation"]
    for r in range(WORLD):
        assert steps[r]["valid"]["rc"] == 0 and steps[r]["valid"]["sha256"] == golden
