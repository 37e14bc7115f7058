"""The full option grid, option switches on one warm prover, and the hint paths at blowup 32 and 64, on the GPU.

check_prove_args accepts blowup 8 .. 64, folding 2 .. 16, either field extension, remainder degrees 2^k - 1 up to 255
and 1 .. 255 queries; the index math of the coset LDE, the FRI layer layout, the fixed-column snapshot, the derived clock
and the fused row hash is written in log_b and per extension.  Every proof here is the CPU oracle's, byte for byte
(tests/option_grid.py holds the cases and the check):

  * one cold proof (fresh prover, no hints) per (blowup, folding, extension), at trace lengths 2^10 .. 2^13;
  * the small extremes: a remainder of one coefficient, one query over E, 255 queries, no FRI layer at blowup 64;
  * option sets whose layer rule folds below the blowup: a degree error, as on the oracle, and the prover proves on;
  * the warm paths (hinted sparse / narrow upload, derived clock, fixed snapshot, fused k_fixed_hash) at blowup 32 and
    64 and over the quadratic extension at blowup 16 -- n = 2^13 is the smallest length at which the fixed class exists;
  * a sequence of option changes on one warm prover, which retakes the fixed snapshot after every change of blowup.
"""
import numpy as np
import pytest

from option_grid import (GRID, OVERFOLDED, SMALL, SMALL_PROGRAMS, case_id, check_against_oracle, grid_trace, options,
                         oracle_options, small_trace)
from test_fixed_columns import FIXED, get_trace, other_last_row
from test_gpu_parity import oracle_pub
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- a. the cold grid
@pytest.mark.parametrize("case", GRID, ids=case_id)
def test_cold_grid(oracle, case):
    blowup, folding, ext, log_n, rem = case
    trace, pub = grid_trace(log_n)
    n = trace.shape[1]
    rec = check_against_oracle(lambda: GpuProver(0, max_trace_len=n, max_blowup=blowup), oracle, trace, pub,
                               options(blowup, folding, ext, rem))
    assert 1 <= rec.num_fri_layers <= 10 and rec.remainder_len >= 1


# ---------------------------------------------------------------- b. small and extreme shapes
@pytest.mark.parametrize("name", list(SMALL_PROGRAMS))
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_small_and_extreme_shapes(oracle, case, name):
    trace, pub = small_trace(name)
    n = trace.shape[1]
    check_against_oracle(lambda: GpuProver(0, max_trace_len=n, max_blowup=case[0]), oracle, trace, pub, options(*case))


# ---------------------------------------------------------------- c. over-folded options
@pytest.mark.parametrize("name", list(SMALL_PROGRAMS))
@pytest.mark.parametrize("case", OVERFOLDED, ids=case_id)
def test_overfolded_options_are_a_degree_error(oracle, case, name):
    """The last layer is shorter than the blowup, so the remainder has no coefficient (remainder_step:
    rl = L / B = 0; every interpolated coefficient counts as beyond the degree bound, nothing is
    written to the record's remainder, the empty remainder is hashed and serialized as zero bytes).  The oracle gives
    its degree error with remainder_len 0; so must the GPU, and its next proof with default options is the oracle's."""
    trace, pub = small_trace(name)
    opub = oracle_pub(oracle, pub)
    orc, _, orec, _ = oracle.prove_rc(trace, opub, oracle_options(oracle, options(*case)))
    assert orc == native.ZK_ERR_DEGREE and orec.remainder_len == 0
    g = GpuProver(0, max_trace_len=trace.shape[1], max_blowup=case[0])
    try:
        _, rec, _, rc = g.prove(trace, pub, options(*case), record=True, allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE
        assert rec.remainder_len == 0 and rec.num_fri_layers == orec.num_fri_layers
        proof, _, _, rc = g.prove(trace, pub, ProofOptions())
        assert rc == 0 and proof == oracle.prove(trace, opub)[0]
    finally:
        g.close()


# ---------------------------------------------------------------- d. warm paths at blowup 32 and 64, and over E
def test_warm_blowup_32(oracle):
    """32 cosets (r = t & 31, q = t >> 5): the third proof forms columns 0 .. 11 of another trace of the program from
    the snapshot, the fourth of the first trace again."""
    ta, pa = get_trace(13, "cipher", 41)
    tb2 = other_last_row(get_trace(13, "cipher", 42)[0])
    pb = get_trace(13, "cipher", 42)[1]
    opts = options(32, 8, 1, 127)
    oopts = oracle_options(oracle, opts)
    want_a = oracle.prove(ta, oracle_pub(oracle, pa), oopts)[0]
    want_b = oracle.prove(tb2, oracle_pub(oracle, pb), oopts)[0]
    g = GpuProver(0, max_trace_len=ta.shape[1], max_blowup=32)
    try:
        ups = []
        for t, p, want in ((ta, pa, want_a), (ta, pa, want_a), (tb2, pb, want_b), (ta, pa, want_a)):
            proof, _, _, rc = g.prove(t, p, opts)
            assert rc == 0 and proof == want
            ups.append(g.upload_stats())
        assert [u["fixed"] for u in ups] == [[], [], FIXED, FIXED]
        assert ups[2]["derived"] == ups[3]["derived"] == [0]
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


_b64 = {}


def b64_oracle_proof(oracle, t, p, opts):
    """The one oracle proof at blowup 64 (about 7 s of CPU), shared by the two tests below."""
    if "want" not in _b64:
        _b64["want"] = oracle.prove(t, oracle_pub(oracle, p), oracle_options(oracle, opts))[0]
    return _b64["want"]


def test_warm_blowup_64(oracle):
    """64 cosets, one trace proved four times (one oracle proof); the proof opens 32 of 2^19 rows, so the fourth
    proof's whole LDE and every leaf are compared with the dumps of a fresh prover's first proof, which has no hints
    and takes the separate passes."""
    t, p = get_trace(13, "cipher", 41)
    n = t.shape[1]
    opts = options(64, 8, 1, 127)
    want = b64_oracle_proof(oracle, t, p, opts)
    names = ("trace_lde", "trace_leaves")
    g = GpuProver(0, max_trace_len=n, max_blowup=64)
    try:
        ups = []
        for k in range(4):
            proof, _, dumps, rc = g.prove(t, p, opts, dump=names if k == 3 else ())
            assert rc == 0 and proof == want, k
            ups.append(g.upload_stats())
        assert [u["fixed"] for u in ups] == [[], [], FIXED, FIXED]
        assert ups[2]["derived"] == ups[3]["derived"] == [0]
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()
    fresh = GpuProver(0, max_trace_len=n, max_blowup=64)
    try:
        proof, _, wdumps, rc = fresh.prove(t, p, opts, dump=names)
        assert rc == 0 and proof == want and fresh.upload_stats()["fixed"] == []
    finally:
        fresh.close()
    assert dumps["trace_lde"].shape == (64 * n * 28, 2) and dumps["trace_leaves"].shape == (64 * n * 2, 2)
    for name in names:
        assert np.array_equal(dumps[name], wdumps[name]), name


def test_warm_blowup_64_other_trace(oracle):
    """The test above proves one trace four times, so columns 0 .. 11 of the LDE and the leaves its second proof left
    in the prover's buffers are already the right ones: a fused launch that stored nothing at some coset would pass.
    Here the third proof is of another trace of the program with another last row (other leaves everywhere, other
    values in columns 0 .. 11).  No second oracle proof at this blowup: the reference is a fresh prover's first proof of
    that trace -- the cold path, which the grid checks against the oracle at blowup 64 -- by proof bytes, the whole LDE
    and every leaf; both verifiers accept the proof."""
    from zkvm_amd.prover import verify
    ta, pa = get_trace(13, "cipher", 41)
    tb2 = other_last_row(get_trace(13, "cipher", 42)[0])
    pb = get_trace(13, "cipher", 42)[1]
    n = ta.shape[1]
    opts = options(64, 8, 1, 127)
    want_a = b64_oracle_proof(oracle, ta, pa, opts)
    names = ("trace_lde", "trace_leaves")
    g, fresh = GpuProver(0, max_trace_len=n, max_blowup=64), GpuProver(0, max_trace_len=n, max_blowup=64)
    try:
        for _ in range(2):
            proof, _, _, rc = g.prove(ta, pa, opts)
            assert rc == 0 and proof == want_a
        proof, _, dumps, rc = g.prove(tb2, pb, opts, dump=names)
        assert rc == 0 and g.upload_stats()["fixed"] == FIXED and g.upload_stats()["derived"] == [0]
        want, _, wdumps, rc = fresh.prove(tb2, pb, opts, dump=names)
        assert rc == 0 and fresh.upload_stats()["fixed"] == [] and proof == want
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()
        fresh.close()
    for name in names:
        assert np.array_equal(dumps[name], wdumps[name]), name
    assert oracle.verify(proof, oracle_pub(oracle, pb), 0) == (0, "")
    assert verify(proof, pb, 0) == (0, "")


def test_warm_quadratic_blowup_16(oracle):
    t, p = get_trace(13, "cipher", 41)
    opts = options(16, 8, 2, 127)
    want = oracle.prove(t, oracle_pub(oracle, p), oracle_options(oracle, opts))[0]
    g = GpuProver(0, max_trace_len=t.shape[1], max_blowup=16)
    try:
        fixed = []
        for _ in range(3):
            proof, _, _, rc = g.prove(t, p, opts)
            assert rc == 0 and proof == want
            fixed.append(g.upload_stats()["fixed"])
        assert fixed == [[], [], FIXED] and g.upload_stats()["derived"] == [0]
        assert g.proof_info()["hint_redos"] == 0
    finally:
        g.close()


# ---------------------------------------------------------------- e. option changes on one warm prover
DEFAULT = ProofOptions()
B16 = options(16, 8, 1, 127)
EXT2 = options(8, 8, 2, 127)
FOLD4 = options(8, 4, 1, 31)
B16_EXT2 = options(16, 8, 2, 127)
SWITCHES = [DEFAULT] * 3 + [B16] * 3 + [DEFAULT] * 2 + [EXT2, FOLD4] + [B16_EXT2] * 2


def test_option_changes_on_one_warm_prover(oracle):
    """One trace under changing options on one prover: every proof is the oracle's, no hint is refuted, and the fixed
    snapshot is retaken exactly after a change of blowup.

    The expected upload_stats()["fixed"] sequence follows from trace_commit.hip and upload_plan.hpp:
      * hints are kept per (trace length, program hash) -- prove_impl (prover.hip) sets src.key = pub->program_hash
        and HostTraceCommit::classify looks the set up with hint_find(p, n, src.key) -- so the options are not part of
        the key, and a completed proof under any options leaves h->have set (trace_hints_learn, hint_slot) for the
        next one;
      * the first proof has no hint set ("fresh" is false): nothing fixed, no snapshot.  The second is fresh with
        H->snap < 0: FS stays null, the plan's fixm = snap ? snap_mask & ~hint : 0 is 0, snap_now = fix_ok && !snap
        takes the snapshot after the LDE is written (fixed_slot(p, owner, n, B, ..) records the plan's B), and
        trace_hints_refuted hands it to the hint set (hint_sets[owner].snap = si) because the proof stood.  The third
        finds FS: FIXED;
      * classify accepts the set's snapshot only `if (s.live && s.n == n && s.B == B && s.lwe == src.lwe)`;
        otherwise `fixed_drop(p, H->snap)` forgets it, FS stays null, this proof forms nothing from it (fixed == [])
        and snap_now retakes it at the new B, so the proof after that is FIXED again.  B is the plan's blowup
        (1 << pl->log_b): only a change of blowup (or lwe_size) takes this branch.  The field extension and the FRI
        folding enter after the trace commitment (SingleProof::constraints onward), so changing them alone keeps FIXED."""
    t, p = get_trace(13, "cipher", 41)
    opub = oracle_pub(oracle, p)
    want = {}
    g = GpuProver(0, max_trace_len=t.shape[1], max_blowup=16)
    try:
        fixed = []
        for k, opts in enumerate(SWITCHES):
            if opts not in want:
                want[opts] = oracle.prove(t, opub, oracle_options(oracle, opts))[0]
            proof, _, _, rc = g.prove(t, p, opts)
            assert rc == 0 and proof == want[opts], (k, opts)
            fixed.append(g.upload_stats()["fixed"])
            assert g.proof_info()["hint_redos"] == 0, k
    finally:
        g.close()
    assert len(want) == 5
    retaken = [k for k in range(1, len(SWITCHES)) if SWITCHES[k].blowup_factor != SWITCHES[k - 1].blowup_factor]
    assert retaken == [3, 6, 10]
    assert fixed == [[] if k < 2 or k in retaken else FIXED for k in range(len(SWITCHES))], fixed
