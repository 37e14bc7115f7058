"""The composition stage (S4, composition_stage in prover.hip) called directly on the GPU at its edges, against the
plain-integer reference of tests/back_half_ref.py (whose parts tests/test_back_half_ref_cpu.py pins on the CPU).

zk_diag_composition runs the stage as a single-GPU proof does: the per-coset inverse NTTs, the cross-coset step
k_comp_cross (with nce = 7 it derives CE coset 7 from the degree bound, CrossMap::derive7), the assertion terms'
quotient in coefficient form (boundary_poly_add: k_bnd_div_g, k_deep_div_scan<2>, k_deep_div_q<1, true>) added into
column 0, the LDE and the commitment.  zk_diag_composition_parts runs the cross step and the quotient by coefficient ranges, as
the ranks of a sharded proof do.

A whole proof of a valid trace gives these kernels one kind of input.  Here: trace lengths 16 and 32 (the smallest),
256 and 512 (one and two phase-1 blocks of 256), 2048 (one phase-3 chunk, the low half of the split power tables) and
4096 (a carry across chunks, the tables' high half); polynomials of all 0, all p - 1, one coefficient at each end of a
column and of the degree bound; a failing assertion at either end alone and in one plane alone; the two degree flags
one coefficient each side of their edge.  Every comparison is exact (integers and bytes).
"""
import ctypes as C
import random

import numpy as np
import pytest

import back_half_ref as ref
from test_gpu_back_half import elems, ref_ints, root_of_unity, unit
from test_gpu_parity import workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver
from zkvm_amd.workloads import LR_PROGRAM

pytestmark = pytest.mark.gpu
P = ref.P
W = 28
SIZES = [16, 32, 256, 512, 2048, 4096]
# blowup 8 everywhere; 16 at two sizes: there the LDE cosets are no longer the CE cosets
SIZES_BLOWUPS = [(n, 8) for n in SIZES] + [(16, 16), (512, 16)]
# ranges of 2048 coefficients (one phase-3 chunk each) for every parts count, and one of two chunks per range
RANGES = [(4096, 2), (8192, 4), (16384, 8), (8192, 2)]


# ---------------------------------------------------------------- calling the two diagnostics
def split_cols(raw, n):
    v = ref_ints(raw)
    return [v[i:i + n] for i in range(0, len(v), n)]


def comp_bytes(comp):
    return b"".join(pl if isinstance(pl, bytes) else elems(pl) for pl in comp)


def run_comp(comp, n, ext, ncols, nce, blowup=8, bnd=None):
    """zk_diag_composition.  comp: ext planes of 8 n coset-major values (integers, or encoded); bnd: (trace bytes,
    coeff_b planes, bnd1 values) or None.  -> (the ext ncols base columns in the order (c ext + j), root, flag)"""
    assert native.device_count() > 0, "no GPU visible"
    polys, root = C.create_string_buffer(16 * ext * ncols * n), C.create_string_buffer(32)
    flag = C.c_uint32(7)
    tpb, cb, b1 = bnd if bnd else (None, None, None)
    native.check(native.lib().zk_diag_composition(
        0, comp_bytes(comp), n, blowup, ext, ncols, nce, tpb, elems(v for pl in cb for v in pl) if bnd else None,
        elems(b1) if bnd else None, polys, root, C.byref(flag)), "zk_diag_composition")
    return split_cols(polys.raw, n), root.raw, flag.value


def run_parts(comp, n, ext, ncols, parts, bnd=None):
    """zk_diag_composition_parts on the same inputs -> (columns, flag)"""
    polys = C.create_string_buffer(16 * ext * ncols * n)
    flag = C.c_uint32(7)
    tpb, cb, b1 = bnd if bnd else (None, None, None)
    native.check(native.lib().zk_diag_composition_parts(
        0, comp_bytes(comp), n, ext, ncols, parts, tpb, elems(v for pl in cb for v in pl) if bnd else None,
        elems(b1) if bnd else None, polys, C.byref(flag)), "zk_diag_composition_parts")
    return split_cols(polys.raw, n), flag.value


# ---------------------------------------------------------------- inputs and expectations, made once per key
_values = {}


def kinds(d):
    """the polynomial classes under a bound of d n coefficients: names only (n-independent, for the test ids)"""
    at = ["0", "n-1"] + (["n"] if d > 1 else []) + (["top-1"] if d > 1 else [])
    return ["random", "all 0", "all p-1", "constant p-1"] + [f"{v} at {k}" for k in at for v in ("one", "p-1")]


def poly(kind, n, d):
    """the coefficients (at most d n) of class `kind`; deterministic per (kind, n, d)"""
    rnd = random.Random(f"poly {kind} {n} {d}")
    top = d * n
    if kind == "random":
        return [rnd.randrange(P) for _ in range(top)]
    if kind == "all 0":
        return [0] * top
    if kind == "all p-1":
        return [P - 1] * top
    if kind == "constant p-1":
        return [P - 1]
    v, _, k = kind.split(" ")
    k = {"0": 0, "n-1": n - 1, "n": n, "top-1": top - 1}[k]
    return unit(top, k, 1 if v == "one" else P - 1)


def values(oracle, coeffs, n, key=None):
    """composition_values of the coefficients (Horner's rule at n = 16, the oracle's transform above), kept per key"""
    if key is not None and key in _values:
        return _values[key]
    v = ref.composition_values(coeffs, n, None if n == 16 else oracle.eval_coset)
    if key is not None:
        _values[key] = v
    return v


def class_values(oracle, kind, n, d):
    coeffs = poly(kind, n, d)
    return coeffs, values(oracle, coeffs, n, (kind, n, d))


def hide_coset7(vals, n):
    """coset 7 all p - 1: a launch with nce = 7 must not read it"""
    return vals[:7 * n] + [P - 1] * n


def columns(plane_coeffs, n, ncols):
    """the expected base columns in the stage's order (c ext + j) from the planes' coefficients"""
    segs = [ref.segment(c, n, ncols) for c in plane_coeffs]
    return [segs[j][c] for c in range(ncols) for j in range(len(segs))]


def root_of(oracle, cols, n, blowup=8):
    return ref.composition_root(oracle.blake3, oracle.merkle_root, oracle.eval_coset, cols, n, blowup)


def first_diff(got, want):
    return [(c, k) for c, (g, w) in enumerate(zip(got, want)) for k in range(len(w)) if g[k] != w[k]][:6]


def check_cols(got, want, what):
    assert len(got) == len(want)
    assert got == want, f"{what}: (column, coefficient) {first_diff(got, want)} differ"


# ---------------------------------------------------------------- the cross step in the production shape
@pytest.mark.parametrize("kind", kinds(7))
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,blowup", SIZES_BLOWUPS)
def test_cross_step_seven_cosets_seven_columns(oracle, n, blowup, ext, kind):
    """ncols = 7, nce = 7 (SingleProof's shape for every n >= 16), no assertion terms: coset 7 is derived, never read.
    Over E the second plane holds another class, so a plane taken for the other cannot pass."""
    names = kinds(7)
    mine = [kind, names[(names.index(kind) + 5) % len(names)]][:ext]
    planes = [class_values(oracle, k, n, 7) for k in mine]
    got, root, flag = run_comp([hide_coset7(v, n) for _, v in planes], n, ext, 7, 7, blowup)
    want = columns([c for c, _ in planes], n, 7)
    check_cols(got, want, f"n={n} ext={ext} {mine}")
    assert flag == 0
    assert root == root_of(oracle, want, n, blowup)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_derived_coset_beyond_its_premise(oracle, n, ext):
    """nce = 7 with a polynomial of degree in [7n, 8n): the seven columns are the polynomial with a zero top block that
    agrees with the input on cosets 0 .. 6, and the flag stays 0 -- the documented contract (the out-of-domain identity
    reports such a trace, not this flag)."""
    rnd = random.Random(f"beyond {n}")
    polys = [unit(8 * n, 7 * n), [rnd.randrange(P) for _ in range(8 * n)], unit(8 * n, 8 * n - 1, P - 1)]
    for i in range(len(polys)):
        idx = [i, (i + 1) % len(polys)][:ext]
        mine = [polys[t] for t in idx]
        comp = [hide_coset7(values(oracle, polys[t], n, ("beyond", n, t)), n) for t in idx]
        got, _, flag = run_comp(comp, n, ext, 7, 7)
        assert flag == 0, f"n={n} ext={ext} polynomial {i}"
        for j in range(ext):
            q = [v for c in range(7) for v in got[c * ext + j]]
            assert q != mine[j][:7 * n]  # (not the truncation: the top block is folded into the columns)
            back = values(oracle, q, n)
            assert back[:7 * n] == comp[j][:7 * n], f"n={n} ext={ext} polynomial {i} plane {j}: cosets 0 .. 6 differ"


# ---------------------------------------------------------------- all eight cosets, every column count, the flag's edge
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("ncols", [1, 2, 7, 8])
@pytest.mark.parametrize("n", SIZES)
def test_cross_step_eight_cosets(oracle, n, ncols, ext):
    """nce = 8: every class under the bound ncols n (flag 0; the root for the random and the all p - 1 class), then
    the flag's edge: one coefficient at ncols n or at 8n - 1 raises it, at ncols n - 1 does not.  Over E the refused
    coefficient is in the second plane alone."""
    names = kinds(ncols)
    for i, kind in enumerate(names):
        mine = [kind, names[(i + 5) % len(names)]][:ext]
        planes = [class_values(oracle, k, n, ncols) for k in mine]
        got, root, flag = run_comp([v for _, v in planes], n, ext, ncols, 8)
        want = columns([c for c, _ in planes], n, ncols)
        check_cols(got, want, f"n={n} ncols={ncols} ext={ext} {mine}")
        assert flag == 0, (kind, flag)
        if kind in ("random", "all p-1"):
            assert root == root_of(oracle, want, n)
    good = class_values(oracle, "random", n, ncols)
    edges = [(ncols * n - 1, 0)] + ([(ncols * n, 1), (8 * n - 1, 1)] if ncols < 8 else [])
    for k, want_flag in edges:
        c = unit(8 * n, k)
        planes = ([good] if ext == 2 else []) + [(c, values(oracle, c, n, ("unit", n, k)))]
        got, _, flag = run_comp([v for _, v in planes], n, ext, ncols, 8)
        assert flag == want_flag, f"n={n} ncols={ncols} ext={ext}: one coefficient at {k}"
        check_cols(got, columns([c for c, _ in planes], n, ncols), f"n={n} ncols={ncols} ext={ext} edge {k}")


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("ncols", [1, 5])
@pytest.mark.parametrize("n", SIZES)
def test_seven_cosets_fewer_columns_flag(oracle, n, ncols, ext):
    """nce = 7 with fewer than seven columns: a coefficient inside columns ncols .. 6 raises the flag, the last one
    of column ncols - 1 does not."""
    good = class_values(oracle, "random", n, ncols)
    for k, want_flag in ((ncols * n - 1, 0), (ncols * n, 1), (7 * n - 1, 1)):
        c = unit(8 * n, k)
        planes = ([good] if ext == 2 else []) + [(c, values(oracle, c, n, ("unit", n, k)))]
        got, _, flag = run_comp([hide_coset7(v, n) for _, v in planes], n, ext, ncols, 7)
        assert flag == want_flag, f"n={n} ncols={ncols} ext={ext}: one coefficient at {k}"
        check_cols(got, columns([c for c, _ in planes], n, ncols), f"n={n} ncols={ncols} ext={ext} edge {k}")


@pytest.mark.parametrize("ncols", [1, 7])
def test_public_commit_refuses_the_first_coefficient_past_the_bound(oracle, ncols):
    """zk_commit_composition (natural CE order in): the coefficient at ncols n is ZK_ERR_DEGREE, the one before it
    commits to the reference's columns and root."""
    trace, _ = workload_trace(LR_PROGRAM, seed=3)
    n = trace.shape[1]
    L = native.lib()
    g = GpuProver(0, max_trace_len=n)
    h = C.c_void_p()
    try:
        tb = np.ascontiguousarray(trace)
        native.check(L.zk_lde_new(g.handle, tb.ctypes.data, W, n, 8, C.byref(h), C.create_string_buffer(32)))
        natural = lambda v: elems(v[(i % 8) * n + i // 8] for i in range(8 * n))  # noqa: E731
        cc, root, polys = C.c_void_p(), C.create_string_buffer(32), C.create_string_buffer(16 * ncols * n)
        bad = values(oracle, unit(8 * n, ncols * n), n)
        assert L.zk_commit_composition(h, natural(bad), ncols, C.byref(cc), root, polys) == native.ZK_ERR_DEGREE
        last = unit(8 * n, ncols * n - 1)
        native.check(L.zk_commit_composition(h, natural(values(oracle, last, n)), ncols, C.byref(cc), root, polys))
        want = ref.segment(last, n, ncols)
        check_cols(split_cols(polys.raw, n), want, f"ncols={ncols}")
        assert root.raw == root_of(oracle, want, n)
        L.zk_comp_free(cc)
    finally:
        if h:
            L.zk_lde_free(h)
        g.close()


# ---------------------------------------------------------------- the assertion quotient
def g_last2(n):
    return pow(root_of_unity(n.bit_length() - 1), n - 2, P)


def make_consistent(tp, cb, n):
    """Changes the constant coefficients of column 12 (and 14 over two planes) so that f0(1) = 0 in every plane, and
    returns the bnd1 of every plane that makes f1(c) = 0: both assertions' remainders vanish."""
    ext = len(cb)
    sums = {k: sum(tp[k]) % P for k in ref.ASSERT_COL0}
    r = [-sum(cb[j][i] * sums[k] for i, k in enumerate(ref.ASSERT_COL0)) % P for j in range(ext)]
    if ext == 1:
        d12, d14 = r[0] * pow(cb[0][4], -1, P) % P, 0
    else:
        (a, b), (cc, d) = (cb[0][4], cb[0][6]), (cb[1][4], cb[1][6])
        det = pow((a * d - b * cc) % P, -1, P)
        d12, d14 = (r[0] * d - b * r[1]) * det % P, (a * r[1] - cc * r[0]) * det % P
    tp[12][0] = (tp[12][0] + d12) % P
    tp[14][0] = (tp[14][0] + d14) % P
    c = g_last2(n)
    at_c = {k: ref.horner(tp[k], c) for k in ref.ASSERT_COL1}
    return [sum(cb[j][12 + i] * at_c[k] for i, k in enumerate(ref.ASSERT_COL1)) % P for j in range(ext)]


_traces = {}


def consistent_trace(n, ext):
    """random trace planes and coefficients with both remainders zero: (columns, their encodings, cb, bnd1), shared"""
    if (n, ext) not in _traces:
        rnd = random.Random(f"trace {n} {ext}")
        tp = [[rnd.randrange(P) for _ in range(n)] for _ in range(W)]
        cb = [[rnd.randrange(1, P) for _ in range(22)] for _ in range(ext)]
        bnd1 = make_consistent(tp, cb, n)
        _traces[n, ext] = (tp, [elems(col) for col in tp], cb, bnd1)
    return _traces[n, ext]


def quotients(tp, cb, bnd1, n):
    """the reference quotient and flag of every plane"""
    c = g_last2(n)
    return [ref.boundary_quotient(tp, cb[j], bnd1[j], c) for j in range(len(cb))]


BND_CASES = ["consistent", "step 0 broken", "last step broken", "both broken", "second plane broken", "all 0",
             "all p-1", "with composition"]
BND_PARAMS = [(ext, case) for ext in (1, 2) for case in BND_CASES if ext == 2 or case != "second plane broken"]


@pytest.mark.parametrize("ext,case", BND_PARAMS)
@pytest.mark.parametrize("n", SIZES)
def test_boundary_quotient(oracle, n, ext, case):
    """ncols = 7, nce = 7 with the assertion terms (the shape every single-GPU proof runs).  comp is all zero, so
    column 0 is the quotient alone and columns 1 .. 6 stay zero -- except in the last case, where column 0 must be the
    cross step's column 0 plus the quotient.  The quotient is defined, and compared, whether or not a remainder is
    left; the flag is 1 exactly when one is, in either divisor and in either plane alone."""
    tp, enc, cb, bnd1 = consistent_trace(n, ext)
    want_flag = 1
    if case in ("step 0 broken", "both broken"):
        # a column asserted at step 0 only (0 or 11): f0(1) moves, f1 does not
        col, k = (0, n // 2) if n.bit_length() % 2 else (11, n - 1)
        tp = list(tp)
        tp[col] = list(tp[col])
        tp[col][k] = (tp[col][k] + 1) % P
        enc = list(enc)
        enc[col] = elems(tp[col])
    if case in ("last step broken", "both broken"):
        bnd1 = [(v + 1) % P for v in bnd1]
    if case == "second plane broken":
        bnd1 = [bnd1[0], (bnd1[1] + 1) % P]
    if case == "all 0":
        tp, bnd1, want_flag = [[0] * n] * W, [0] * ext, 0
        enc = [bytes(16 * n)] * W
    if case == "all p-1":
        # 12 (and 10) maximal products and bnd1 into the lazy accumulator of k_bnd_div_g
        tp, cb, bnd1, want_flag = [[P - 1] * n] * W, [[P - 1] * 22] * ext, [P - 1] * ext, None
        enc = [elems(tp[0])] * W
    if case in ("consistent", "with composition"):
        want_flag = 0
    planes = [([], [0] * (8 * n))] * ext
    if case == "with composition":
        planes = [class_values(oracle, k, n, 7) for k in ("random", "all p-1")[:ext]]
    ref_q = quotients(tp, cb, bnd1, n)
    if want_flag is None:
        want_flag = int(any(f for _, f in ref_q))
    else:
        assert want_flag == int(any(f for _, f in ref_q))
    if case == "second plane broken":
        assert [f for _, f in ref_q] == [0, 1]
    got, root, flag = run_comp([hide_coset7(v, n) for _, v in planes], n, ext, 7, 7, 8, (b"".join(enc), cb, bnd1))
    want = columns([c for c, _ in planes], n, 7)
    for j in range(ext):
        want[j] = [(x + y) % P for x, y in zip(want[j], ref_q[j][0])]
    check_cols(got, want, f"n={n} ext={ext} {case}")
    assert flag == want_flag
    if case == "all 0":
        assert got == [[0] * n] * (7 * ext)
    if n <= 512 or case in ("consistent", "with composition"):
        assert root == root_of(oracle, want, n)


# ---------------------------------------------------------------- by coefficient ranges
RANGE_CLASSES = ["random", "all 0", "all p-1", "before first boundary", "first boundary", "before last boundary",
                 "last boundary", "top", "random at boundary"]


def range_index(kind, n, kg):
    return {"before first boundary": kg - 1, "first boundary": kg, "before last boundary": n - kg - 1,
            "last boundary": n - kg, "top": n - 1, "random at boundary": kg}[kind]


@pytest.mark.parametrize("kind", RANGE_CLASSES)
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,parts", RANGES)
def test_composition_by_coefficient_ranges(oracle, n, parts, ext, kind):
    """The cross step and the quotient range by range (a sharded proof's ranks, in rank order on one device) against
    the whole stage with nce = 8 on the same inputs, and both against the reference.  The classes put one coefficient
    each side of the first and the last range boundary and at the top, in the composition columns (columns 0 and 6)
    and in every trace polynomial the boundary sums carry; the trace is then made consistent, so the flag is 0."""
    rnd = random.Random(f"ranges {n} {parts} {ext} {kind}")
    kg = n // parts
    if kind in ("random", "all 0", "all p-1"):
        coeffs = poly(kind, n, 7)
        fill = {"random": lambda: rnd.randrange(P), "all 0": lambda: 0, "all p-1": lambda: P - 1}[kind]
        tp = [[fill() for _ in range(n)] for _ in range(W)]
    else:
        k = range_index(kind, n, kg)
        v = rnd.randrange(1, P) if kind == "random at boundary" else 1
        coeffs = unit(7 * n, k, v)
        coeffs[6 * n + k] = P - v
        tp = [unit(n, k, rnd.randrange(1, P) if kind == "random at boundary" else 1) for _ in range(W)]
    plane_coeffs = [coeffs, poly("random", n, 7)][:ext]
    comp = [values(oracle, coeffs, n), class_values(oracle, "random", n, 7)[1]][:ext]
    cb = [[rnd.randrange(1, P) for _ in range(22)] for _ in range(ext)]
    bnd1 = make_consistent(tp, cb, n)
    bnd = (b"".join(elems(col) for col in tp), cb, bnd1)
    want = columns(plane_coeffs, n, 7)
    for j, (q, f) in enumerate(quotients(tp, cb, bnd1, n)):
        assert f == 0
        want[j] = [(x + y) % P for x, y in zip(want[j], q)]
    got_p, flag_p = run_parts(comp, n, ext, 7, parts, bnd)
    check_cols(got_p, want, f"n={n} parts={parts} ext={ext} {kind}: ranges against the reference")
    got_w, _, flag_w = run_comp(comp, n, ext, 7, 8, 8, bnd)
    check_cols(got_w, want, f"n={n} parts={parts} ext={ext} {kind}: whole stage against the reference")
    assert got_p == got_w and (flag_p, flag_w) == (0, 0)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,parts", RANGES)
def test_failing_assertion_in_any_range_raises_the_flag(oracle, n, parts, ext):
    """Only the range with k0 = 0 looks at the remainders: a trace coefficient that breaks the step 0 assertion must
    raise the flag from whichever range holds it; so must a wrong last-step value; and a coefficient past the column
    bound seen by one range's cross step alone."""
    tp, enc, cb, bnd1 = consistent_trace(n, ext)
    kg = n // parts
    comp = [bytes(16 * 8 * n)] * ext
    zero_cols = [[0] * n] * (7 * ext)
    for g in range(parts):
        k = g * kg + 5
        t2, e2 = list(tp), list(enc)
        t2[0] = list(tp[0])
        t2[0][k] = (t2[0][k] + 1) % P
        e2[0] = elems(t2[0])
        want = list(zero_cols)
        for j, (q, f) in enumerate(quotients(t2, cb, bnd1, n)):
            assert f == 1
            want[j] = q
        got, flag = run_parts(comp, n, ext, 7, parts, (b"".join(e2), cb, bnd1))
        check_cols(got, want, f"n={n} parts={parts} ext={ext}: offending coefficient in range {g}")
        assert flag == 1, f"offending coefficient {k} in range {g}"
    got_w, _, flag_w = run_comp(comp, n, ext, 7, 8, 8, (b"".join(e2), cb, bnd1))
    assert got_w == got and flag_w == 1
    # the last-step value wrong in the last plane alone
    b2 = bnd1[:-1] + [(bnd1[-1] + 1) % P]
    got, flag = run_parts(comp, n, ext, 7, parts, (b"".join(enc), cb, b2))
    want = list(zero_cols)
    for j, (q, f) in enumerate(quotients(tp, cb, b2, n)):
        assert f == int(j == ext - 1)
        want[j] = q
    check_cols(got, want, f"n={n} parts={parts} ext={ext}: last-step value")
    assert flag == 1
    # the cross step's flag from the last range alone: one coefficient at 7n + (n - 1), its neighbour below allowed
    for k, want_flag in ((7 * n - 1, 0), (8 * n - 1, 1)):
        c = unit(8 * n, k)
        planes = [poly("random", n, 7), c][-ext:]
        vals = [class_values(oracle, "random", n, 7)[1], values(oracle, c, n, ("unit", n, k))][-ext:]
        got, flag = run_parts(vals, n, ext, 7, parts)
        check_cols(got, columns(planes, n, 7), f"n={n} parts={parts} ext={ext}: coefficient {k}")
        assert flag == want_flag, k


# ---------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_and_a_good_call_still_matches(oracle):
    L = native.lib()
    n = 16
    comp, tpb = bytes(16 * 2 * 8 * n), bytes(16 * W * n)
    cbb, b1 = bytes(16 * 44), bytes(32)
    out, root, flag = C.create_string_buffer(16 * 16 * n), C.create_string_buffer(32), C.c_uint32(7)
    big = elems([P]) + bytes(16 * (2 * 8 * n - 1))
    base = dict(comp=comp, n=n, blowup=8, ext=1, ncols=7, nce=7, tp=tpb, cb=cbb, b1=b1, out=out, root=root,
                flag=C.byref(flag))
    bad = [dict(nce=6), dict(nce=9), dict(nce=7, ncols=8), dict(ncols=0), dict(ncols=9, nce=8), dict(ext=0),
           dict(ext=3), dict(n=8), dict(n=24), dict(n=0), dict(blowup=4), dict(blowup=12), dict(blowup=128), dict(comp=None),
           dict(out=None), dict(root=None), dict(flag=None), dict(comp=big), dict(cb=None), dict(b1=None),
           dict(tp=elems([2**128 - 1]) + bytes(16 * (W * n - 1))), dict(cb=elems([P]) + bytes(16 * 43)),
           dict(b1=elems([P, 0])), dict(ext=2, b1=elems([0, P]))]
    for kw in bad:
        a = dict(base, **kw)
        rc = L.zk_diag_composition(0, a["comp"], a["n"], a["blowup"], a["ext"], a["ncols"], a["nce"], a["tp"], a["cb"],
                                   a["b1"], a["out"], a["root"], a["flag"])
        assert rc == native.ZK_ERR_INVALID_ARG and L.zk_last_error(), kw
    n2 = 4096
    comp2, tp2 = bytes(16 * 8 * n2), bytes(16 * W * n2)
    out2 = C.create_string_buffer(16 * 8 * n2)
    pbase = dict(comp=comp2, n=n2, ext=1, ncols=7, parts=2, tp=tp2, cb=cbb, b1=b1, out=out2, flag=C.byref(flag))
    pbad = [dict(parts=1), dict(parts=3), dict(parts=16), dict(parts=4), dict(n=2048), dict(n=16), dict(ncols=0),
            dict(ncols=9), dict(ext=3), dict(comp=None), dict(out=None), dict(flag=None), dict(cb=None),
            dict(comp=elems([P]) + bytes(16 * (8 * n2 - 1)))]
    for kw in pbad:
        a = dict(pbase, **kw)
        rc = L.zk_diag_composition_parts(0, a["comp"], a["n"], a["ext"], a["ncols"], a["parts"], a["tp"], a["cb"],
                                         a["b1"], a["out"], a["flag"])
        assert rc == native.ZK_ERR_INVALID_ARG and L.zk_last_error(), kw
    assert flag.value == 7  # no refused call wrote it
    # good calls afterwards: the all-zero inputs of above, then a random polynomial with a consistent trace
    native.check(L.zk_diag_composition(0, comp, n, 8, 2, 7, 7, tpb, cbb, b1, out, root, C.byref(flag)))
    assert flag.value == 0 and out.raw[:16 * 14 * n] == bytes(16 * 14 * n)
    assert root.raw == root_of(oracle, [[0] * n] * 14, n)
    native.check(L.zk_diag_composition_parts(0, comp2, n2, 1, 7, 2, tp2, cbb, b1, out2, C.byref(flag)))
    assert flag.value == 0 and out2.raw[:16 * 7 * n2] == bytes(16 * 7 * n2)
    tp, enc, cb, bnd1 = consistent_trace(n, 1)
    coeffs, vals = class_values(oracle, "random", n, 7)
    got, r, f = run_comp([hide_coset7(vals, n)], n, 1, 7, 7, 8, (b"".join(enc), cb, bnd1))
    want = columns([coeffs], n, 7)
    want[0] = [(x + y) % P for x, y in zip(want[0], quotients(tp, cb, bnd1, n)[0][0])]
    check_cols(got, want, "after the refusals")
    assert f == 0 and r == root_of(oracle, want, n)
