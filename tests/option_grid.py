"""The proof-option grid shared by tests/test_gpu_option_grid.py (GPU against the oracle) and
tests/test_option_grid_cpu.py (the table itself, and the oracle's side of the small cases).  Not a test module.

check_prove_args accepts blowup 8 .. 64, FRI folding 2 .. 16, field extension 1 or 2, remainder degrees 2^k - 1 up to
255 and 1 .. 255 queries; GRID holds one case per (blowup, folding, extension), at the trace length the oracle proves
in a few seconds, SMALL the extreme shapes (remainder of one coefficient, one query, 255 queries, no FRI layer) and
OVERFOLDED the option sets whose layer rule folds below the blowup, which no prover can satisfy (degree error).
"""
import numpy as np

from test_gpu_parity import compare_records, oracle_pub, workload_trace
from zkvm_amd.prover import ProofOptions, verify
from zkvm_amd.workloads import LR_PROGRAM, ops_for_trace_len

MAX_FRI_LAYERS = 16  # ZK_MAX_FRI_LAYERS (include/zkvm_gpu.h)
BLOWUPS, FOLDINGS, EXTENSIONS = (8, 16, 32, 64), (2, 4, 8, 16), (1, 2)
GRID_QUERIES = 32
# log2 of the trace length per (blowup, extension)
GRID_LOG_N = {(8, 1): 13, (8, 2): 13, (16, 1): 13, (16, 2): 12, (32, 1): 12, (32, 2): 11, (64, 1): 12, (64, 2): 10}
REM_BY_FOLDING = {2: 7, 4: 31, 8: 127, 16: 255}


def grid_remainder_degree(blowup, folding):
    """Remainder degree of a grid case: by folding, but (8, 16) takes 15 so that it has three layers."""
    return 15 if (blowup, folding) == (8, 16) else REM_BY_FOLDING[folding]


# (blowup, folding, extension, log_n, remainder degree)
GRID = [(b, f, e, GRID_LOG_N[(b, e)], grid_remainder_degree(b, f)) for b in BLOWUPS for f in FOLDINGS for e in EXTENSIONS]

SMALL_PROGRAMS = {"pushadd64": "push.5\npush.3\nadd", "lr128": LR_PROGRAM}
# (blowup, folding, extension, remainder degree, queries)
SMALL = [(64, 2, 1, 0, 255),   # 6 / 7 layers, a remainder of one coefficient, the most queries
         (8, 2, 2, 0, 1),      # a single query over E
         (32, 4, 2, 3, 100),
         (64, 16, 1, 255, 32)]  # no FRI layer at blowup 64
OVERFOLDED = [(64, 16, 2, 0, 32), (16, 16, 2, 0, 127)]  # the last layer has 16 or 4 (n = 64), 32 or 8 (n = 128) values

STAGES = ("trace_polys", "trace_lde", "trace_leaves", "composition", "comp_polys", "comp_lde", "deep", "fri_layer1")


def case_id(case):
    return "-".join(str(v) for v in case)


def layer_sizes(N, blowup, folding, rem_max_deg):
    """The FRI layer lengths by prover.hip's fri_num_layers rule (fold while the layer is longer than
    (remainder degree + 1) * blowup): [N, N / folding, ..., last]; the number of layers is len() - 1."""
    sizes = [N]
    while sizes[-1] > (rem_max_deg + 1) * blowup:
        sizes.append(sizes[-1] // folding)
    return sizes


def options(blowup, folding, extension, rem, queries=GRID_QUERIES):
    return ProofOptions(num_queries=queries, blowup_factor=blowup, grinding_factor=0, field_extension=extension,
                        fri_folding_factor=folding, fri_remainder_max_degree=rem)


def oracle_options(oracle, opts):
    return oracle.default_options(num_queries=opts.num_queries, blowup=opts.blowup_factor, grinding=opts.grinding_factor,
                                  field_extension=opts.field_extension, fri_folding=opts.fri_folding_factor,
                                  fri_rem_max_deg=opts.fri_remainder_max_degree)


_traces = {}


def grid_trace(log_n):
    """The cipher-mix trace of 2^log_n rows with workload seed log_n, made once."""
    if log_n not in _traces:
        _traces[log_n] = workload_trace(ops_for_trace_len(log_n, "cipher"), seed=log_n)
        assert _traces[log_n][0].shape[1] == 1 << log_n
    return _traces[log_n]


def small_trace(name):
    if name not in _traces:
        _traces[name] = workload_trace(SMALL_PROGRAMS[name], seed=len(name))
    return _traces[name]


def first_differing_stage(make_prover, oracle, trace, pub, opts):
    """Proves the trace again on a fresh prover with every stage dumped and returns the name of the first stage that
    differs from the oracle's, or None.  E-valued stages are dumped as their a components; the composition columns as
    extension * num_ccols base columns, of which the dumps hold only the first n (polys) / blowup * n (LDE) rows'
    worth."""
    g = make_prover()
    try:
        _, _, dumps, _ = g.prove(trace, pub, opts, dump=STAGES, allow_degree_error=True)
    finally:
        g.close()
    _, _, orec, odumps = oracle.prove_rc(trace, oracle_pub(oracle, pub), oracle_options(oracle, opts), want=STAGES)
    n, B = trace.shape[1], opts.blowup_factor
    ck = opts.field_extension * orec.num_ccols
    trim = {"comp_polys": ck * n, "comp_lde": B * n * ck}
    for name in STAGES:
        if name == "fri_layer1" and orec.num_fri_layers == 0:
            continue
        k = trim.get(name, len(odumps[name]))
        if not np.array_equal(dumps[name][:k], odumps[name][:k]):
            return name
    return None


def check_against_oracle(make_prover, oracle, trace, pub, opts):
    """One proof on a fresh prover (the cold path: no hints): status, record, bytes and both verifiers.  Only when
    the record or the bytes differ is the trace proved again with stage dumps, to name the first stage that differs."""
    g = make_prover()
    try:
        proof, rec, _, rc = g.prove(trace, pub, opts, record=True)
    finally:
        g.close()
    assert rc == 0
    opub = oracle_pub(oracle, pub)
    oproof, orec, _ = oracle.prove(trace, opub, oracle_options(oracle, opts))
    try:
        compare_records(rec, orec)
        assert proof == oproof
    except AssertionError as e:
        stage = first_differing_stage(make_prover, oracle, trace, pub, opts)
        raise AssertionError(f"{e}; first stage that differs from the oracle: {stage}") from e
    assert oracle.verify(proof, opub, 0) == (0, "")
    assert verify(proof, pub, 0) == (0, "")
    return rec
