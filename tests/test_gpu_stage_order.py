"""What the staged provers (SingleProof in prover.hip, ShardedProof in shard.hip, both over ProofRun) must keep and no
pinned-proof test asserts: the order of the stage marks, the branch without FRI layers on both provers, and an early
return through the guards followed by another proof on the same prover."""
import pytest

from option_grid import STAGES, options, small_trace
from test_gpu_eval_frames import random_trace
from test_sharded import CASES, case_inputs
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, verify
from zkvm_amd.sharded import ShardedProver

pytestmark = pytest.mark.gpu

# zk_prover_stage_times of one proof, in order (a stage ends at its mark); taken on the commit before the stages became
# methods, from this helper
SINGLE_STAGES = ["trace_commit", "constraints", "composition", "ood", "deep", "fri", "queries", "serialize"]
SHARDED_STAGES = ["trace_lde"] + SINGLE_STAGES


def golden(name):
    """The smallest golden cases: "lr" (n = 128, base field) and "lr_quad" (the quadratic extension)."""
    return case_inputs(next(c for c in CASES if c["name"] == name))


def proved_stages(prover, trace, pub, opts, want):
    try:
        assert prover.prove(trace, pub, opts)[0] == want
        return list(prover.stage_times())
    finally:
        prover.close()


@pytest.mark.parametrize("name", ["lr", "lr_quad"])
def test_single_gpu_stage_order(name):
    trace, proof, pub, opts = golden(name)
    assert proved_stages(GpuProver(0, max_trace_len=trace.shape[1]), trace, pub, opts, proof) == SINGLE_STAGES


def test_sharded_stage_order():
    trace, proof, pub, opts = golden("lr")
    assert proved_stages(ShardedProver.loopback(2, max_trace_len=trace.shape[1]), trace, pub, opts, proof) == SHARDED_STAGES


@pytest.mark.parametrize("ext", [1, 2])
def test_no_fri_layers_single_and_sharded(ext):
    """fri_num_layers = 0: the DEEP layer is the remainder (natural order, lb0 = 0), no layer-0 tree, so the openings'
    plans never read rows0 or Y.len[0] / fold.  The option grid's no-layer case (option_grid.SMALL: remainder degree 255,
    32 queries, on the 64-row trace) is at blowup 64, which the sharded prover does not take; the same trace and
    remainder degree at blowup 8, the sharded prover's only one, give N = 512 <= 256 * 8, again no layer.  Folding 2, so
    that the 2-rank loopback accepts the length (n / fold >= 16)."""
    trace, pub = small_trace("pushadd64")
    n = trace.shape[1]
    assert n == 64
    opts = options(8, 2, ext, 255, 32)
    g = GpuProver(0, max_trace_len=n)
    try:
        single, rec, _, rc = g.prove(trace, pub, opts, record=True)
    finally:
        g.close()
    assert rc == 0 and rec.num_fri_layers == 0 and rec.remainder_len == n
    sp = ShardedProver.loopback(2, max_trace_len=n)
    try:
        sharded, srec = sp.prove(trace, pub, opts, record=True)
    finally:
        sp.close()
    assert srec.num_fri_layers == 0
    assert sharded == single
    assert verify(single, pub, 0) == (0, "")


def test_rejected_trace_between_good_proofs():
    """A trace the AIR rejects (test_gpu_eval_frames' random trace) with the stage dumps requested ends at the
    out-of-domain identity: ZK_ERR_DEGREE, the front stages dumped, the proof left through its guards.  The same prover
    then gives the valid trace's pinned proof, as it did before."""
    trace, proof, pub, opts = golden("lr")
    n = trace.shape[1]
    g = GpuProver(0, max_trace_len=n)
    try:
        assert g.prove(trace, pub, opts)[0] == proof
        _, _, dumps, rc = g.prove(random_trace(n, 5), pub, opts, dump=STAGES, allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE
        assert dumps["composition"].any() and dumps["comp_lde"].any() and not dumps["deep"].any()
        got, _, _, rc = g.prove(trace, pub, opts)
        assert rc == 0 and got == proof
    finally:
        g.close()
