"""The constant-multiplier forms of the field multiply and the coset-table LDE, each called directly on the GPU.

  * fe_mul_uniform / fe_mul_wsv / fe_mul_uniform2 / fe_mul_wsv2 / fe_mul_w2_2 (zk_diag_field_op 11 .. 15; fe_mul and
    fe_mul_w2, ops 2 and 7, on the same operands) bit for bit against Python integers, on random operands, on edge
    operands, and on operands crafted so that the value before the last conditional subtraction is p + d (the branch
    "bit 128 of U set" of ws_fold, which random operands take about once in 2^47 multiplies) or just below p;
  * the shared final reductions ws_fold / ws_fold2 on raw inputs (ops 16, 17) around every threshold of that branch;
  * ntt_lde through zk_diag_lde, bytes compared with the oracle's coset evaluation, at the smallest size of every
    path (single pass, generic and fused coset pass 1, every tile shape), every launch shape the prover uses, and on
    columns of 0, 1, p - 1 and unit vectors, which an interpolated trace never feeds it.

The constants reach the kernels through the production builders make_fe_ws / make_fe_w2 (run by the diagnostic's host
side), so those are under test as well (their CPU test: test_native_cpu.test_constant_forms_on_host).
"""
import ctypes as C
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from zkvm_amd import native
from zkvm_amd.prover import bytes_elems, elems_bytes

pytestmark = pytest.mark.gpu
P = 2**128 - 45 * 2**40 + 1
C128 = 2**128 - P  # 2^128 mod p
M32 = 2**32 - 1


def run_op(op, a, b):
    assert native.device_count() > 0, "no GPU visible"
    out = C.create_string_buffer(16 * len(a))
    native.check(native.lib().zk_diag_field_op(0, op, elems_bytes(a), elems_bytes(b), out, len(a)))
    return bytes_elems(out.raw)


# ---------------------------------------------------------------- models of the operands' classes (inputs only)
def ws_pre(a, w):
    """The W-set forms' value before the final conditional subtraction: S = L + T C for the column sum
    sum_i a_i W_i = L + T 2^128 (W_i = w 2^(32 i) mod p, a_i the 32-bit words of a)."""
    sigma = sum(((a >> (32 * i)) & M32) * (w * 2**(32 * i) % P) for i in range(4))
    return (sigma % 2**128) + (sigma >> 128) * C128, sigma >> 128


def w2_pre(a, w):
    """The two-part forms': the 193-bit sum a_lo w + a_hi (w 2^64 mod p) folded once (L + H C, at most 129 bits), its
    bit 128 folded again."""
    sigma = (a % 2**64) * w + (a >> 64) * (w * 2**64 % P)
    s1 = (sigma % 2**128) + (sigma >> 128) * C128
    return (s1 % 2**128) + (s1 >> 128) * C128


EDGE_A = [0, 1, 2, P - 1, P - 2, 2**64 - 1, 2**64, 2**127, P - 2**64, 45 * 2**40,  # test_field_ops
          2**128 - 1, 2**128 - 2, P, P + 1, 2**128 - 45 * 2**40]                    # test_lazy_field_forms
EDGE_W = [0, 1, 2, P - 1, P - 2, 2**32, 2**64, 2**96, 2**127, 45 * 2**40, 2**64 - 1]


def crafted(w, r):
    """a < 2^128 with a w = r (mod p); r = 0 as a = p, which the contract (any first operand below 2^128) admits"""
    return r * pow(w, -1, P) % P if r else P


@pytest.fixture(scope="module")
def operands():
    """Blocks of 64 lanes with one constant w each (b constant over the block, as the wave-uniform forms need it): the
    operands under test at the even positions, random partners below 2^128 at the odd ones -- in every two-output
    form exactly the even positions are returned, once from each slot.  kind[t]: the class of position t."""
    rnd = random.Random(2024)
    groups = []  # (w, [(a, kind)])
    for lo, hi, kind, count in ((0, P, "random canonical", 128), (P, 2**128, "random in [p, 2^128)", 32),
                                (0, 2**128, "random below 2^128", 32)):
        for _ in range(count):
            groups.append((rnd.randrange(P), [(rnd.randrange(lo, hi), kind) for _ in range(32)]))
    for w in EDGE_W:
        groups.append((w, [(a, "edge") for a in EDGE_A]))
    n_pd = n_below = 0
    for small in (False, True):
        blocks = 0
        while blocks < 8:  # p + d: a w = d (mod p) with the column sum k p + d, k >= 1 and d < k C
            w = rnd.randrange(2, 2**32) if small else rnd.randrange(2, P)
            ds = [0, 1, 2, C128 - 1, C128] + [rnd.randrange(2**45) for _ in range(27)]
            ops = [(crafted(w, d), "p + d") for d in ds]
            if any(ws_pre(a, w)[0] != P + d for (a, _), d in zip(ops, ds)):
                continue  # (a sum below p + d: possible for the smallest w only)
            groups.append((w, ops))
            n_pd += len(ops)
            blocks += 1
        for _ in range(8):  # just below p: a w = p - 1 - e, no subtraction may fire
            w = rnd.randrange(2, 2**32) if small else rnd.randrange(2, P)
            es = [0, 1, 2, C128] * 8
            ops = [(crafted(w, P - 1 - e), "below p") for e in es]
            assert all(ws_pre(a, w)[0] == P - 1 - e for (a, _), e in zip(ops, es))
            groups.append((w, ops))
            n_below += len(ops)
    for _ in range(8):  # p + d with a top part of more than 32 bits (s5 > 0): w < 2^32 never has one, a random w often
        w, ops = rnd.randrange(2, P), []
        while len(ops) < 32:
            d = rnd.randrange(2**45)
            s, top = ws_pre(crafted(w, d), w)
            if s == P + d and top >= 2**32:
                ops.append((crafted(w, d), "p + d"))
        groups.append((w, ops))
    assert n_pd >= 256 and n_below >= 256
    a, b, kind = [], [], []
    for w, ops in groups:
        ops = ops + [(rnd.randrange(P), "pad") for _ in range(32 - len(ops))]
        for x, k in ops:
            a += [x, rnd.randrange(2**128)]
            kind += [k, "partner"]
        b += [w] * 64
    return a, b, kind


def test_operand_classes_reach_their_branch(operands):
    """(inputs only) what the crafted operands reach in each pipeline, by the integer models above: in the W-set forms
    every p + d operand arrives at exactly p + d -- at least 256 with a top part T = k - 1 below 2^32 (s5 = 0) and 256
    with one above (s5 > 0) -- and every below-p operand at p - 1 - e;
    in the two-part forms (one fold more, then the same final step) the p + d operands with d < C arrive at p + d too."""
    a, b, kind = operands
    pd = [(x, w) for x, w, k in zip(a, b, kind) if k == "p + d"]
    assert all(P <= ws_pre(x, w)[0] < P + 2**47 for x, w in pd)
    assert sum(ws_pre(x, w)[1] >= 2**32 for x, w in pd) >= 256, "p + d with s5 > 0"
    assert sum(ws_pre(x, w)[1] < 2**32 for x, w in pd) >= 256, "p + d with s5 = 0"
    assert sum(w2_pre(x, w) >= P for x, w in pd) >= 256
    below = [(x, w) for x, w, k in zip(a, b, kind) if k == "below p"]
    assert all(ws_pre(x, w)[0] < P for x, w in below) and all(w2_pre(x, w) < P for x, w in below)


def check_products(op, got, want_of, a, b, kind):
    bad = [(t, kind[t], hex(a[t]), hex(b[t]), hex(got[t]), hex(want_of(t))) for t in range(len(got))
           if got[t] != want_of(t) or got[t] >= P]
    assert not bad, f"op {op}: {len(bad)} wrong or non-canonical products (t, class, a[t], b[t], got, want): {bad[:4]}"


@pytest.mark.parametrize("op", [2, 7, 11, 12])
def test_multiply_forms_single(operands, op):
    """fe_mul, fe_mul_w2, fe_mul_uniform (W set from scalar loads, one constant per wave), fe_mul_wsv (per lane): every
    lane returns a[t] b[t] mod p, canonical."""
    a, b, kind = operands
    check_products(op, run_op(op, a, b), lambda t: a[t] * b[t] % P, a, b, kind)


@pytest.mark.parametrize("op", [14, 15])
def test_multiply_forms_paired(operands, op):
    """fe_mul_wsv2 / fe_mul_w2_2: lane t pairs (a, b)[t] with the mirrored lane's (a, b)[count - 1 - t] and returns
    output t & 1, so each even position is returned once from the first slot and once from the second."""
    a, b, kind = operands
    m = len(a)
    assert m % 2 == 0
    check_products(op, run_op(op, a, b), lambda t: (a[m - 1 - t] * b[m - 1 - t] if t & 1 else a[t] * b[t]) % P, a, b, kind)


def test_multiply_uniform2(operands):
    """fe_mul_uniform2: lane t of a wave starting at w0 pairs (a[t], A) with (a[w0 + 63 - l], B), A / B the W sets of
    b[w0] / b[w0 + 63], and returns output t & 1.  First with A = B (the crafted operands meet their own constant in both
    slots), then with B the constant of another block (a swapped or shared constant would show)."""
    a, b, kind = operands
    m = len(a)

    def want(bb):
        return lambda t: (a[(t & ~63) + 63 - (t & 63)] * bb[(t & ~63) + 63] if t & 1 else a[t] * bb[t & ~63]) % P

    check_products(13, run_op(13, a, b), want(b), a, b, kind)
    b2 = list(b)
    for w0 in range(0, m, 64):
        b2[w0 + 63] = b[(w0 + 64 * 7) % m]
    assert sum(b2[w0] != b2[w0 + 63] for w0 in range(0, m, 64)) > m // 64 - 8
    check_products(13, run_op(13, a, b2), want(b2), a, b2, kind)


# ---------------------------------------------------------------- raw final reductions
@pytest.fixture(scope="module")
def fold_inputs():
    """(L, T = s4 + s5 2^32) at the even positions, random partners at the odd ones.  U = L + (T + 1) C reaches 2^128,
    where the branch flips, at L = 2^128 - C (T + 1)."""
    rnd = random.Random(77)
    cases = []
    for s5 in range(8):
        for s4 in [0, 1, 2**31, 2**32 - 1] + [rnd.randrange(2**32) for _ in range(3)]:
            T = s4 + s5 * 2**32
            Ls = [0, 1, 2**128 - 1, 2**128 - C128 * (T + 1) - 1, 2**128 - C128 * (T + 1), 2**128 - C128 * (T + 1) + 1,
                  2**128 - C128 * T] + [rnd.randrange(2**128) for _ in range(3)]
            cases += [(L, T) for L in Ls if 0 <= L < 2**128]
    a, b = [], []
    for L, T in cases:
        a += [L, rnd.randrange(2**128)]
        b += [T, rnd.randrange(2**35)]
    return a, b


def test_ws_fold_raw(fold_inputs):
    a, b = fold_inputs
    got = run_op(16, a, b)
    bad = [(hex(L), hex(T), hex(g)) for L, T, g in zip(a, b, got) if g != (L + T * 2**128) % P]
    assert not bad, f"ws_fold: {len(bad)} wrong (L, T, got): {bad[:4]}"


def test_ws_fold2_raw(fold_inputs):
    """lane t reduces its own input and the mirrored lane's in one paired block and returns output t & 1"""
    a, b = fold_inputs
    m = len(a)
    got = run_op(17, a, b)
    src = [m - 1 - t if t & 1 else t for t in range(m)]
    bad = [(t, hex(a[s]), hex(b[s]), hex(g)) for t, (s, g) in enumerate(zip(src, got)) if g != (a[s] + b[s] * 2**128) % P]
    assert not bad, f"ws_fold2: {len(bad)} wrong (lane, L, T, got): {bad[:4]}"


# ---------------------------------------------------------------- coset LDE
KINDS = ["random", "from {0, 1, 2, p - 2, p - 1}", "all p - 1", "v e_0", "v e_(n-1)"]


def pair(v):
    return [v % 2**64, v >> 64]


def columns(n, seed):
    """one column of each kind, as an (5, n, 2) array of (lo, hi) words"""
    rng = np.random.default_rng(seed)
    cols = np.zeros((len(KINDS), n, 2), dtype=np.uint64)
    cols[0, :, 0] = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    cols[0, :, 1] = rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64)  # hi < 2^64 - 1: below p
    pick = np.array([pair(0), pair(1), pair(2), pair(P - 2), pair(P - 1)], dtype=np.uint64)
    cols[1] = pick[rng.integers(0, 5, size=n)]
    cols[2] = np.array(pair(P - 1), dtype=np.uint64)
    cols[3, 0] = rng.integers(0, 2**64 - 1, size=2, dtype=np.uint64)
    cols[4, n - 1] = rng.integers(0, 2**64 - 1, size=2, dtype=np.uint64)
    return cols


# (log_n, blowup, r0, rstride, ncos, from_evals): ntt_log_n2 splits 13 -> 7/6, 16 -> 8/8, 19 -> 10/9, 20 -> 10/10,
# 21 -> 11/10, 22 -> 12/10; pass-1 lines of 2^10 .. 2^12 are the fused coset pass 1 (Lds::UNI tiles)
LDE_CASES = [
    (3, 8, 0, 1, 8, 0), (10, 8, 0, 1, 8, 0), (11, 8, 0, 1, 8, 0), (12, 8, 0, 1, 8, 0),  # single pass, full tables
    (13, 8, 0, 1, 8, 0),    # first four-step size, generic coset pass 1
    (13, 16, 0, 1, 16, 0),  # 16 cosets: two launches of 8
    (16, 8, 0, 1, 8, 0),
    (19, 8, 0, 1, 8, 0),    # first fused coset pass 1 (lines of 2^10), generic pass 2
    (20, 8, 0, 1, 8, 0), (20, 8, 3, 1, 2, 0), (20, 8, 1, 2, 4, 0),  # both passes wave-uniform tiles; launch shapes
    (21, 8, 4, 1, 4, 0),    # odd tile (lines of 2^11), radix-2 last stage
    (22, 8, 6, 1, 2, 0),    # 4096-point tile, one line per block
    (13, 8, 0, 1, 8, 1), (19, 8, 0, 1, 8, 1), (20, 8, 0, 1, 8, 1),  # from evaluations: the prover's interpolation first
]


@pytest.mark.parametrize("log_n,blowup,r0,rstride,ncos,from_evals", LDE_CASES)
def test_coset_lde(oracle, log_n, blowup, r0, rstride, ncos, from_evals):
    """out[(c ncos + j) n + k] = P_c(s_r w_n^k), s_r = 3 w_N^r, r = r0 + j rstride: every (column, coset) plane byte for
    byte against the oracle's radix-2 or_eval_coset (from_evals: of the oracle's interpolation of the column)."""
    assert native.device_count() > 0, "no GPU visible"
    n = 1 << log_n
    cols = columns(n, 1000 * log_n + 16 * r0 + ncos + from_evals)
    ncols = cols.shape[0]
    out = np.empty((ncols, ncos, n, 2), dtype=np.uint64)
    native.check(native.lib().zk_diag_lde(0, cols.ctypes.data, n, ncols, blowup, r0, rstride, ncos, from_evals,
                                          out.ctypes.data))
    wN = oracle.root_of_unity(log_n + blowup.bit_length() - 1)
    L = oracle.lib()
    one = elems_bytes([1])

    def coeffs_of(c):
        if from_evals:
            assert L.or_interp_coset(cols[c].ctypes.data, n, one) == 0  # in place
        return c

    def plane(cj):
        c, j = cj
        ref = np.empty((n, 2), dtype=np.uint64)
        off = elems_bytes([3 * pow(wN, r0 + j * rstride, P) % P])
        assert L.or_eval_coset(cols[c].ctypes.data, n, n, off, ref.ctypes.data) == 0
        return c, j, np.flatnonzero((ref != out[c, j]).any(axis=1))

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:  # the oracle calls release the GIL
        list(ex.map(coeffs_of, range(ncols)))
        bad = [(KINDS[c], f"coset {r0 + j * rstride}", f"{len(d)} of {n} differ, first at k = {d[0]}")
               for c, j, d in ex.map(plane, [(c, j) for c in range(ncols) for j in range(ncos)]) if len(d)]
    assert not bad, bad


def test_coset_lde_refuses_cosets_outside_the_domain():
    buf = C.create_string_buffer(16 * 8)
    for r0, rstride, ncos in ((8, 1, 1), (0, 1, 9), (1, 2, 5), (7, 1, 2)):
        assert native.lib().zk_diag_lde(0, buf, 8, 1, 8, r0, rstride, ncos, 0, buf) == native.ZK_ERR_INVALID_ARG
