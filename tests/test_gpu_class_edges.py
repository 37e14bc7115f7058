"""The three implementations that draw a host trace's column classes -- k_sparse_detect (a prover's first proof of a
program), the detection fused into the interpolation's pass 1 (from the second proof on, over the expanded columns) and
the host checks pack_rows / zero_rows / clock_rows -- held together at the exact class boundaries, through whole proofs
with oracle parity.

The program is the 2^13 cipher mix; its stack registers s10 .. s15 (columns 22 .. 27) are read by no constraint or
assertion, and s11 .. s15 are zero before the last row, so entries written there leave the trace valid:
0xFF / 0x100 split the 8-bit class from the 32-bit one, 2^32 - 1 / 2^32 the 32-bit class from the dense columns, and
2^64 (low limb zero) is dense, not sparse -- at row 0 and at row n - 2, the first and the last row that count."""
import hashlib

import pytest

from test_gpu_parity import oracle_pub, workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import ops_for_trace_len

pytestmark = pytest.mark.gpu
_base, _oracle_proofs = [], {}


def base_trace():
    if not _base:
        t, pub = workload_trace(ops_for_trace_len(13, "cipher"), seed=13)
        n = t.shape[1]
        assert n == 1 << 13 and not t[23:28, :n - 1].any()  # the cipher mix never reaches stack depth 12
        _base.append((t, pub))
    t, pub = _base[0]
    return t.copy(), pub


def prove_like_the_oracle(g, oracle, t, pub):
    """one proof of t on g, equal to the oracle's (computed once per trace); -> its upload statistics"""
    key = hashlib.sha256(t.tobytes()).digest()
    if key not in _oracle_proofs:
        _oracle_proofs[key] = oracle.prove(t, oracle_pub(oracle, pub))[0]
    proof, _, _, rc = g.prove(t, pub, ProofOptions())
    assert rc == 0
    assert proof == _oracle_proofs[key]
    return g.upload_stats()


@pytest.mark.parametrize("schedule", ["throughput", "latency"])
def test_classes_learned_at_the_exact_widths(oracle, schedule):
    """Proof 1 detects with k_sparse_detect, so proof 2's upload classes are its findings; proof 2 detects in pass 1 of
    the interpolation, over the columns it expanded, so proof 3's are those: both must put 0xFF in the 8-bit class,
    0x100 and 2^32 - 1 in the 32-bit class, 2^32 and 2^64 in none."""
    t, pub = base_trace()
    n = t.shape[1]
    t[27, n - 2] = [0xFF, 0]
    t[26, 0] = [0x100, 0]
    t[25, n - 2] = [2**32 - 1, 0]
    t[24, 0] = [2**32, 0]
    t[23, n - 2] = [0, 1]  # 2^64
    g = GpuProver(0, max_trace_len=n)
    g.set_upload_schedule(schedule)
    try:
        stats = [prove_like_the_oracle(g, oracle, t, pub) for _ in range(3)]
        assert g.proof_info()["schedule"] == schedule and g.proof_info()["hint_redos"] == 0
    finally:
        g.close()
    assert stats[0]["bytes"] == 28 * n * 16 and not stats[0]["narrow8"] and not stats[0]["narrow32"]
    for st in stats[1:]:
        assert 27 in st["narrow8"], st
        assert 25 in st["narrow32"] and 26 in st["narrow32"], st
        assert not {23, 24} & set(st["sparse"] + st["narrow8"] + st["narrow32"]), st
        assert not {25, 26, 27} & set(st["sparse"]), st
    st = stats[1]
    wide = 28 - len(st["sparse"]) - len(st["narrow8"]) - len(st["narrow32"]) - len(st["derived"])
    assert st["fixed"] == [] and st["bytes"] == wide * n * 16 + (len(st["narrow8"]) + 4 * len(st["narrow32"])) * n


def test_two_narrow_columns_refuted_at_once(oracle):
    """0x100 in a learned 8-bit column and 2^32 in a learned 32-bit column of one trace: both go up whole (a fallback
    list of two columns that are not adjacent), the proof is the oracle's, and the next proof holds the first under the
    32-bit class and the second under none."""
    t, pub = base_trace()
    n = t.shape[1]
    t[27, n - 2] = [0xFF, 0]
    t[25, 0] = [2**32 - 1, 0]
    bad = t.copy()
    bad[27, 0] = [0x100, 0]
    bad[25, n - 2] = [2**32, 0]
    g = GpuProver(0, max_trace_len=n)
    g.set_upload_schedule("throughput")
    try:
        stats = [prove_like_the_oracle(g, oracle, x, pub) for x in (t, t, bad, bad)]
        assert g.proof_info()["hint_redos"] == 0  # a narrow column that does not fit voids nothing
    finally:
        g.close()
    assert 27 in stats[1]["narrow8"] and 25 in stats[1]["narrow32"]
    assert not {25, 27} & set(stats[2]["narrow8"] + stats[2]["narrow32"] + stats[2]["sparse"]), stats[2]
    assert 27 in stats[3]["narrow32"] and 27 not in stats[3]["narrow8"], stats[3]
    assert 25 not in stats[3]["narrow8"] + stats[3]["narrow32"] + stats[3]["sparse"], stats[3]


@pytest.mark.parametrize("row", [0, -2], ids=["row0", "row_n-2"])
def test_sparse_hint_refuted_in_the_high_limb(oracle, row):
    """2^64 in a hinted sparse column: its low limb is zero, the column is not.  The host check voids the proof and the
    redo from every column gives the oracle's bytes."""
    t, pub = base_trace()
    n = t.shape[1]
    edited = t.copy()
    edited[27, row % n] = [0, 1]
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(2):
            st = prove_like_the_oracle(g, oracle, t, pub)
        assert set(range(23, 28)) <= set(st["sparse"])
        redos = g.proof_info()["hint_redos"]
        prove_like_the_oracle(g, oracle, edited, pub)
        assert g.proof_info()["hint_redos"] == redos + 1
        st = prove_like_the_oracle(g, oracle, edited, pub)
        assert 27 not in st["sparse"] + st["narrow8"] + st["narrow32"] and g.proof_info()["hint_redos"] == redos + 1
    finally:
        g.close()


def test_clock_hint_refuted_in_the_high_limb(oracle):
    """clk[n - 2] = (n - 2) + 2^64: the low limb is the clock's.  The host check refutes the derivation, the redo from
    the caller's column fails the AIR, and the good trace keeps proving to the oracle's bytes with nothing derived."""
    t, pub = base_trace()
    n = t.shape[1]
    bad = t.copy()
    assert bad[0, n - 2].tolist() == [n - 2, 0]
    bad[0, n - 2] = [n - 2, 1]
    g = GpuProver(0, max_trace_len=n)
    try:
        for _ in range(2):
            st = prove_like_the_oracle(g, oracle, t, pub)
        assert st["derived"] == [0]
        redos = g.proof_info()["hint_redos"]
        _, _, _, rc = g.prove(bad, pub, ProofOptions(), allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE and g.proof_info()["hint_redos"] == redos + 1
        for _ in range(2):
            assert prove_like_the_oracle(g, oracle, t, pub)["derived"] == []
    finally:
        g.close()
