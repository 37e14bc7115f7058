"""The fixed and clock columns' LDE formed inside the row hash of their blocks (kernels.hip k_fixed_hash).

From a prover's third proof of a (trace length, program) the host-trace path forms columns 0 .. 11 of the LDE -- the
derived clock and the fixed class -- in the kernel that compresses BLAKE3 blocks 0 .. 2 of every row, instead of in a
streaming pass the row hash then reads back; zk_vm_prove's preprocessed columns take the same kernel.  Every proof here
is compared byte for byte with the CPU oracle's (or, for zk_vm_prove, with the proof of the host trace), on the third
and fourth proof of a program on one prover, with upload_stats()["fixed"] non-empty so the fused launch really ran;
the full LDE and the leaves are compared with a fresh prover's, whose first proof has no hints and takes the separate
passes.  n = 2^13 is the smallest length at which the fixed class exists (the smallest four-step plan).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_fixed_columns import FIXED, ROOT, get_trace, oracle_proof, other_last_row
from test_gpu_parity import oracle_pub
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, Program, ProofOptions, make_pub_inputs
from zkvm_amd.workloads import cipher_mix_program, make_workload, ops_for_trace_len

pytestmark = pytest.mark.gpu

B16 = ProofOptions(num_queries=28, blowup_factor=16)
P_LO, P_HI = 0xFFFFD30000000000, 0xFFFFFFFFFFFFFFFF  # p - 1 = 2^128 - 45 2^40


def edge_last_row(trace, shift):
    """Columns 0 .. 11 of the last row from {0, 1, p-1, 2^64, n-1}, cycling per column from `shift`."""
    t = trace.copy()
    n = t.shape[1]
    vals = [(0, 0), (1, 0), (P_LO, P_HI), (0, 1), (n - 1, 0)]
    for c in range(12):
        t[c, n - 1] = vals[(c + shift) % 5]
    return t


def prove_seq(g, oracle, seq):
    """The proofs of seq = [(oracle cache name, trace, pub)] on g, each the oracle's; their upload_stats()."""
    ups = []
    for name, t, p in seq:
        proof, _, _, rc = g.prove(t, p, ProofOptions())
        assert rc == 0 and proof == oracle_proof(oracle, name, t, p), name
        ups.append(g.upload_stats())
    return ups


@pytest.mark.parametrize("schedule", ["throughput", "latency"])
def test_cipher_mix_third_and_fourth_proof(oracle, schedule):
    ta, pa = get_trace(13, "cipher", 41)
    tb, pb = get_trace(13, "cipher", 42)
    tb2 = other_last_row(tb)
    g = GpuProver(0, max_trace_len=ta.shape[1])
    g.set_upload_schedule(schedule)
    try:
        ups = prove_seq(g, oracle, [("c13a", ta, pa), ("c13a", ta, pa), ("c13b", tb, pb), ("c13b2", tb2, pb)])
        assert [u["fixed"] for u in ups] == [[], [], FIXED, FIXED]
        assert ups[2]["derived"] == ups[3]["derived"] == [0]
        assert g.proof_info()["schedule"] == schedule and g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_cipher_mix_blowup_16(oracle):
    """16 cosets: the log_b index math of the fused kernel (r = t & 15, q = t >> 4)."""
    ta, pa = get_trace(13, "cipher", 41)
    tb2 = other_last_row(get_trace(13, "cipher", 42)[0])
    pb = get_trace(13, "cipher", 42)[1]
    oopts = oracle.default_options(num_queries=28, blowup=16)
    g = GpuProver(0, max_trace_len=ta.shape[1], max_blowup=16)
    try:
        # (the oracle's blowup-16 proofs are not shared with another test: two distinct traces keep this to two)
        want_a = oracle.prove(ta, oracle_pub(oracle, pa), oopts)[0]
        want_b = oracle.prove(tb2, oracle_pub(oracle, pb), oopts)[0]
        fixed = []
        for t, p, want in ((ta, pa, want_a), (ta, pa, want_a), (tb2, pb, want_b), (ta, pa, want_a)):
            proof, _, _, rc = g.prove(t, p, B16)
            assert rc == 0 and proof == want
            fixed.append(g.upload_stats()["fixed"])
        assert fixed == [[], [], FIXED, FIXED] and g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_push_add_prefix_holds_loaded_columns(oracle):
    """Opcode bits 1 .. 3 (columns 1 .. 3) stay hinted sparse: blocks 0 .. 2 hold columns the fill wrote (hashed from
    the LDE, not stored) among the formed ones."""
    t, p = get_trace(13, "pushadd", 43)
    g = GpuProver(0, max_trace_len=t.shape[1])
    try:
        ups = prove_seq(g, oracle, [("p13", t, p)] * 4)
        for u in ups[2:]:
            assert u["fixed"] == list(range(4, 12)) and u["derived"] == [0] and set(range(1, 4)) <= set(u["sparse"])
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_edge_last_rows(oracle):
    """Last-row values at the ends of the field's range in columns 0 .. 11, changed between the third and fourth proof.
    shift 4 gives column 0 the value n - 1 (a zero clock correction); p - 1 plus a nonzero snapshot value wraps, the
    case where a sum that is not canonical would change the hashed bytes."""
    t, p = get_trace(13, "cipher", 41)
    e3, e4 = edge_last_row(t, 4), edge_last_row(t, 0)
    n = t.shape[1]
    assert tuple(e3[0, n - 1]) == (n - 1, 0) and tuple(e4[0, n - 1]) == (0, 0)
    g = GpuProver(0, max_trace_len=n)
    try:
        ups = prove_seq(g, oracle, [("c13a", t, p), ("c13a", t, p), ("c13e3", e3, p), ("c13e4", e4, p)])
        assert [u["fixed"] for u in ups] == [[], [], FIXED, FIXED]
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


def test_full_lde_and_leaves_match_the_separate_passes():
    """All 28 columns x N values and all N leaves of the third proof against a fresh prover's dump of the same trace:
    the proof opens 32 rows only and the evaluator never reads coset 7, so this is what catches a wrong store."""
    ta, pa = get_trace(13, "cipher", 41)
    tb2 = other_last_row(get_trace(13, "cipher", 42)[0])
    pb = get_trace(13, "cipher", 42)[1]
    names = ("trace_lde", "trace_leaves")
    n = ta.shape[1]
    g, fresh = GpuProver(0, max_trace_len=n), GpuProver(0, max_trace_len=n)
    try:
        for _ in range(2):
            assert g.prove(ta, pa, ProofOptions())[3] == 0
        proof, _, dumps, rc = g.prove(tb2, pb, ProofOptions(), dump=names)
        assert rc == 0 and g.upload_stats()["fixed"] == FIXED and g.upload_stats()["derived"] == [0]
        want, _, wdumps, rc = fresh.prove(tb2, pb, ProofOptions(), dump=names)
        assert rc == 0 and fresh.upload_stats()["fixed"] == [] and proof == want
        assert dumps["trace_lde"].shape == (8 * n * 28, 2)
        for name in names:
            assert np.array_equal(dumps[name], wdumps[name]), name
    finally:
        g.close()
        fresh.close()


@pytest.mark.parametrize("src,want_n", [(ops_for_trace_len(13, "cipher"), 1 << 13), (cipher_mix_program(200)[0], 1 << 14)],
                         ids=["2p13", "cipher200"])
def test_vm_prove_equals_host_trace_proof(src, want_n):
    """zk_vm_prove (columns 0 .. 11 through the fused launch) gives zk_prove's proof of the host trace of the same
    inputs, call after call with another last row; 2^14 (cipher_mix_program(200)) is the smallest length test_gpu_vm.py
    proves."""
    w = make_workload(src, seed=9)
    prog = Program(src)
    n = prog.trace_len
    assert n == want_n
    g = GpuProver(0, max_trace_len=n)
    try:
        inp = Program.encode_inputs(w.public, w.secret, w.server_key)
        edge = [0, 1, (P_HI << 64) | P_LO, 1 << 64, n - 1]
        for k, last_row in enumerate((w.last_row, [edge[(c + 4) % 5] for c in range(12)] + list(w.last_row[12:]))):
            trace, outs = prog.trace(w.public, w.secret, w.server_key, last_row)
            pub = make_pub_inputs(prog.hash, outs, w.server_key.lwe_size(), w.server_key.parameters.delta)
            ref, _, _, rc = g.prove(trace, pub, ProofOptions())
            assert rc == 0
            h, o, proof = prog.prove_device(g, inp, last_row)
            assert (h, o) == (prog.hash, outs) and proof == ref, k
    finally:
        g.close()
        prog.close()


CHILD = r'''
import hashlib, json, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
from test_gpu_parity import workload_trace
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import ops_for_trace_len
t, p = workload_trace(ops_for_trace_len(13, "cipher"), seed=41)
g = GpuProver(0, max_trace_len=t.shape[1])
out = []
for _ in range(4):
    proof, _, _, rc = g.prove(t, p, ProofOptions())
    out.append((rc, hashlib.sha256(proof).hexdigest(), g.upload_stats()))
g.close()
print("RESULT " + json.dumps(out), flush=True)
'''


def test_kill_switch_off(oracle, tmp_path):
    """ZK_FIXED_FUSE=0 (read once per process, so in a child): the fixed class is still taken, by the separate passes,
    and every proof is the oracle's."""
    t, p = get_trace(13, "cipher", 41)
    want = hashlib.sha256(oracle_proof(oracle, "c13a", t, p)).hexdigest()
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=str(ROOT), pkg=str(ROOT / "encrypt-zkvm_amd"), tests=str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-u", str(script)], env=dict(os.environ, ZK_FIXED_FUSE="0"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert [(rc, sha) for rc, sha, _ in out] == [(0, want)] * 4
    assert out[2][2]["fixed"] == out[3][2]["fixed"] == FIXED and out[3][2]["derived"] == [0]


@pytest.mark.parametrize("col,row", [(1, 0), (11, None)], ids=["c1r0", "c11mid"])
def test_edited_fixed_column_is_still_refuted(oracle, col, row):
    """A fixed column edited before the last row: the host compare voids the fused proof, the redo from the caller's
    columns fails the AIR, and valid traces keep proving to the oracle's bytes."""
    t, p = get_trace(13, "cipher", 41)
    n = t.shape[1]
    r = n // 2 if row is None else row
    bad = t.copy()
    bad[col, r, 0] ^= 1
    want = oracle_proof(oracle, "c13a", t, p)
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(4):
            proof, _, _, rc = g.prove(t, p, ProofOptions())
            assert rc == 0 and proof == want
        assert g.upload_stats()["fixed"] == FIXED
        redos = g.proof_info()["hint_redos"]
        _, _, _, rc = g.prove(bad, p, ProofOptions(), allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE and g.proof_info()["hint_redos"] == redos + 1
        proof, _, _, rc = g.prove(t, p, ProofOptions())
        assert rc == 0 and proof == want and g.upload_stats()["fixed"] == []
    finally:
        g.close()
