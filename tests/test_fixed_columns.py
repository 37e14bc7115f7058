"""Fixed columns of a host-resident trace (trace_commit.hip, zk_prover::FixedSnap).

Trace columns 1 .. 11 (opcode bits, hash flag, sponge, stack depth) depend on the program and lwe_size only, up to the
random last row.  A prover's second proof of a (trace length, program) -- the first one that runs with learned hints --
snapshots their coefficients and LDE; from the third proof on they are neither uploaded nor transformed but formed from
the snapshot and the last-row values, while host threads compare the caller's columns with the snapshot's host copy.  A
mismatch voids the proof (redone from every column) and turns the class off for that program.  Every proof here is
compared with the CPU oracle's bytes; n = 2^13 is the smallest four-step plan (the class needs its Lagrange tables).
"""
import hashlib
import json
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from test_gpu_parity import oracle_pub, workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import ops_for_trace_len

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

FIXED = list(range(1, 12))
QUAD = ProofOptions(43, 8, 0, 2, 8, 127)

_traces, _proofs = {}, {}


def get_trace(log_n, kind, seed, extra=""):
    key = (log_n, kind, seed, extra)
    if key not in _traces:
        _traces[key] = workload_trace(ops_for_trace_len(log_n, kind) + extra, seed=seed)
    return _traces[key]


def oracle_proof(oracle, name, trace, pub, quad=False):
    """The oracle's proof of a trace, computed once per name."""
    key = (name, quad)
    if key not in _proofs:
        opts = oracle.default_options(num_queries=43, field_extension=2) if quad else None
        _proofs[key] = oracle.prove(trace, oracle_pub(oracle, pub), opts)[0]
    return _proofs[key]


def other_last_row(trace):
    """The trace with other last-row values in columns 1 .. 11, one of them zero."""
    t = trace.copy()
    n = t.shape[1]
    for c in FIXED:
        t[c, n - 1] = [0x1234567 * c + 5, 77 * c]
    t[4, n - 1] = [0, 0]
    return t


@pytest.mark.parametrize("schedule", ["throughput", "latency"])
def test_cipher_mix_fixed_from_third_proof(oracle, schedule):
    ta, pa = get_trace(13, "cipher", 41)
    tb, pb = get_trace(13, "cipher", 42)
    assert bytes(pa.program_hash) == bytes(pb.program_hash) and not np.array_equal(ta[12], tb[12])
    n = ta.shape[1]
    tb2 = other_last_row(tb)
    seq = [("c13a", ta, pa), ("c13a", ta, pa), ("c13b", tb, pb), ("c13b2", tb2, pb)]
    g = GpuProver(0, max_trace_len=n)
    g.set_upload_schedule(schedule)
    try:
        ups = []
        for name, t, p in seq:
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == oracle_proof(oracle, name, t, p), name
            assert g.proof_info()["schedule"] == schedule
            ups.append(g.upload_stats())
        assert [u["fixed"] for u in ups] == [[], [], FIXED, FIXED]
        u = ups[2]
        narrow = set(u["narrow8"]) | set(u["narrow32"])
        wide = [c for c in range(28) if c not in narrow and c not in u["sparse"] + u["derived"] + u["fixed"]]
        assert u["bytes"] == 16 * n * len(wide), (u, wide)
        info = g.proof_info()
        assert info["hint_redos"] == 0 and info["fixed_sets"] == 1, info
    finally:
        g.close()


def test_push_add_keeps_its_sparse_columns(oracle):
    t, p = get_trace(13, "pushadd", 43)
    n = t.shape[1]
    sparse = [c for c in range(28) if not t[c, : n - 1].any()]
    assert set(range(1, 4)) <= set(sparse)
    g = GpuProver(0, max_trace_len=n)
    try:
        ups = []
        for _ in range(3):
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == oracle_proof(oracle, "p13", t, p)
            ups.append(g.upload_stats())
        assert ups[2]["fixed"] == list(range(4, 12))
        assert ups[2]["sparse"] == ups[1]["sparse"] == sparse
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_two_programs_alternating_keep_their_own_snapshots(oracle):
    progs = {"a": ("c14", get_trace(14, "cipher", 21)), "b": ("p14", get_trace(14, "pushadd", 22))}
    own = {"a": FIXED, "b": list(range(4, 12))}
    n = progs["a"][1][0].shape[1]
    g = GpuProver(0, max_trace_len=n)
    try:
        seen = {"a": [], "b": []}
        for k in "abababab":
            name, (t, p) = progs[k]
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == oracle_proof(oracle, name, t, p), k
            seen[k].append(g.upload_stats()["fixed"])
        for k in "ab":
            assert seen[k] == [[], [], own[k], own[k]], (k, seen[k])
        info = g.proof_info()
        assert info["hint_redos"] == 0 and info["fixed_sets"] == 2, info
    finally:
        g.close()


def test_snapshots_evict_least_recently_used(oracle):
    """Three programs on a prover that keeps two snapshots: every proof stays the oracle's."""
    progs = [(f"e13_{k}", get_trace(13, "cipher" if k != 1 else "pushadd", 50 + k, f"\npush.{k + 1}\n")) for k in range(3)]
    n = progs[0][1][0].shape[1]
    assert all(t.shape[1] == n for _, (t, _) in progs)
    assert len({bytes(p.program_hash) for _, (_, p) in progs}) == 3
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(4):
            for name, (t, p) in progs:
                proof, _, _, rc = g.prove(t, p, ProofOptions())
                assert rc == 0 and proof == oracle_proof(oracle, name, t, p), name
                assert g.proof_info()["fixed_sets"] <= 2
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_quadratic_extension(oracle):
    ta, pa = get_trace(13, "cipher", 41)
    tb, pb = get_trace(13, "cipher", 42)
    g = GpuProver(0, max_trace_len=ta.shape[1])
    try:
        for name, t, p in (("c13a", ta, pa), ("c13a", ta, pa), ("c13b", tb, pb)):
            proof, _, _, rc = g.prove(t, p, QUAD)
            assert rc == 0 and proof == oracle_proof(oracle, name, t, p, quad=True), name
        assert g.upload_stats()["fixed"] == FIXED and g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_two_provers_on_one_device(oracle):
    ta, pa = get_trace(13, "cipher", 41)
    tb, pb = get_trace(13, "cipher", 42)
    want = {"a": oracle_proof(oracle, "c13a", ta, pa), "b": oracle_proof(oracle, "c13b", tb, pb)}
    inputs = {"a": (ta, pa), "b": (tb, pb)}
    provers = [GpuProver(0, max_trace_len=ta.shape[1]) for _ in range(2)]
    errors = []

    def run(g, order):
        try:
            for k in order:
                t, p = inputs[k]
                proof, _, _, rc = g.prove(t, p, ProofOptions())
                assert rc == 0 and proof == want[k], (order, k)
            assert g.upload_stats()["fixed"] == FIXED and g.proof_info()["hint_redos"] == 0
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    try:
        threads = [threading.Thread(target=run, args=(g, order)) for g, order in zip(provers, ("abab", "bbaa"))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
    finally:
        for g in provers:
            g.close()


CHILD = r'''
import hashlib, json, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
from test_gpu_parity import workload_trace
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import ops_for_trace_len
t, p = workload_trace(ops_for_trace_len(14, "cipher"), seed=21)
g = GpuProver(0, max_trace_len=t.shape[1])
out = []
for _ in range(3):
    proof, _, _, rc = g.prove(t, p, ProofOptions())
    out.append((rc, hashlib.sha256(proof).hexdigest(), g.upload_stats()))
g.close()
print("RESULT " + json.dumps(out), flush=True)
'''


def test_kill_switch_off(oracle, tmp_path):
    """ZK_FIXED=0 (read once per process, so in a child): the third proof takes no fixed column and is the oracle's."""
    t, p = get_trace(14, "cipher", 21)
    want = hashlib.sha256(oracle_proof(oracle, "c14", t, p)).hexdigest()
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=str(ROOT), pkg=str(ROOT / "encrypt-zkvm_amd"), tests=str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-u", str(script)], env=dict(os.environ, ZK_FIXED="0"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert [(rc, sha) for rc, sha, _ in out] == [(0, want)] * 3
    assert out[2][2]["fixed"] == [] and out[2][2]["narrow8"] and out[2][2]["derived"] == [0]


@pytest.mark.parametrize("col,row", [(1, 0), (7, 0), (7, -2), (11, None)], ids=["c1r0", "c7r0", "c7last", "c11mid"])
def test_edited_fixed_column_is_refuted(oracle, col, row):
    """A trace that differs from the snapshot in a fixed column before the last row must not be proved as the
    snapshot's: the host compare voids the proof, the redo from the caller's columns fails the AIR as it would without
    the class, and the class stays off for that program while valid traces keep proving to the oracle's bytes."""
    t, p = get_trace(13, "cipher", 41)
    n = t.shape[1]
    r = n // 2 if row is None else row % n
    assert r <= n - 2
    bad = t.copy()
    bad[col, r, 0] ^= 1
    want = oracle_proof(oracle, "c13a", t, p)
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(3):
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == want
        assert g.upload_stats()["fixed"] == FIXED
        redos = g.proof_info()["hint_redos"]
        _, _, _, rc = g.prove(bad, p, ProofOptions(), allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE
        assert g.proof_info()["hint_redos"] == redos + 1
        for _ in range(3):
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == want
            assert g.upload_stats()["fixed"] == []
        info = g.proof_info()
        assert info["hint_redos"] == redos + 1 and info["fixed_sets"] == 0, info
    finally:
        g.close()
