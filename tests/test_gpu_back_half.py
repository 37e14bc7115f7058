"""The back half of a proof, each stage called directly on the GPU at its edges: the out-of-domain frame
(zk_diag_ood: ood_eval), the DEEP quotient (zk_diag_deep: deep_poly), the grinding
search (zk_diag_grind: one grind_launch; and whole proofs whose search crosses the host / GPU threshold and the first
2^22 batch) and the batch openings of the plug points (zk_lde_query, zk_comp_query, zk_lde_read_frame); the DEEP
quotient by coefficient ranges as a sharded proof's ranks compute it (zk_diag_deep_parts) and one FRI layer, committed
and folded (zk_diag_fri_layer).

Whole proofs feed these stages what a valid trace and the coin give, at the trace lengths the VM makes (64 rows and
up).  Here the inputs are chosen: trace lengths 16 and 32, points on the trace domain and of small order, polynomials
of all 0, all p - 1 and one coefficient at each block boundary, coefficient sets of 0, 1 and p - 1, nonce windows
that cross 2^32 and end inside a block, position sets that share every or no Merkle path.  Every comparison is exact
(bytes or integers) against tests/back_half_ref.py, whose parts tests/test_back_half_ref_cpu.py checks on the CPU.

Not here: the path of k_deep_div_scan on which a thread owns several block entries needs n >= 2^19 coefficients, more
than a plain-integer reference does in a test's time; it stays with the full-size proofs (test_gpu_parity
test_bench_size_proof_verifies, test_2_22_proof_verifies, the large goldens).  A BLAKE3 output whose first word is zero
(the head == 0 branch of k_grind) cannot be constructed; bits = 64 runs the comparison it feeds.
"""
import ctypes as C
import random

import numpy as np
import pytest

import back_half_ref as ref
from option_grid import small_trace
from test_gpu_parity import compare_records, oracle_pub, workload_trace
from zkvm_amd import native, wire
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import LR_PROGRAM

pytestmark = pytest.mark.gpu
P = ref.P
TWO_ADIC_ROOT = pow(3, (P - 1) >> 40, P)  # order 2^40 (tests/test_golden.py checks the oracle's roots against it)


def root_of_unity(log_n):
    return pow(TWO_ADIC_ROOT, 1 << (40 - log_n), P)


def elems(values):
    return b"".join(int(v).to_bytes(16, "little") for v in values)


def point_bytes(z, ext):
    return elems([z]) if ext == 1 else elems(z)


class Polys(list):
    """polynomials (lists of n integers) that keep their column-major encoding once made"""
    encoded = None


def cols_bytes(polys):
    if isinstance(polys, Polys):
        if polys.encoded is None:
            polys.encoded = b"".join(elems(p) for p in polys)
        return polys.encoded
    return b"".join(elems(p) for p in polys)


def unit(n, k, v=1):
    c = [0] * n
    c[k] = v
    return c


def ood_e(n):
    """coefficients per lane of k_ood_eval (ood_eval's E)"""
    return 16 if n >= 1024 else max(1, n // 64)


# ---------------------------------------------------------------- OOD
def run_ood(tp, cp, n, ext, z, zg, rank=0, G=1):
    assert native.device_count() > 0, "no GPU visible"
    out = C.create_string_buffer(16 * ext * (56 + len(cp)))
    native.check(native.lib().zk_diag_ood(0, cols_bytes(tp), cols_bytes(cp), len(cp), n, ext, point_bytes(z, ext),
                                          point_bytes(zg, ext), rank, G, out), "zk_diag_ood")
    flat = ref_ints(out.raw)
    if ext == 1:
        return flat
    np_ = 56 + len(cp)
    return list(zip(flat[:np_], flat[np_:]))


def ref_ints(b):
    return [int.from_bytes(b[i:i + 16], "little") for i in range(0, len(b), 16)]


def class_polys(rnd, n, count):
    """`count` polynomials cycling through the classes: random, all 0, all p - 1, and a single one at k = 0, n - 1,
    64 E - 1 and 64 E (the last lane of a wave's first row and the first of the next; dropped where n has no such
    coefficient) -- every class in each group of seven polynomials a block of k_ood_eval owns"""
    e64 = 64 * ood_e(n)
    kinds = [lambda: [rnd.randrange(P) for _ in range(n)], lambda: [0] * n, lambda: [P - 1] * n,
             lambda: unit(n, 0), lambda: unit(n, n - 1)]
    kinds += [lambda k=k: unit(n, k) for k in (e64 - 1, e64, 63, 64) if 0 < k < n - 1]
    return Polys(kinds[(i + i // len(kinds)) % len(kinds)]() for i in range(count))


def ood_points(rnd, n, ext):
    """(name, z, zg): random and independent; 1, p - 1 and an order-64 root with zg = z g_n as the prover pairs them;
    the trace-domain point g_n with g_n^2; over E also points with a zero component"""
    g = root_of_unity(n.bit_length() - 1)
    base = [("one", 1, g), ("minus_one", P - 1, (P - 1) * g % P), ("order64", root_of_unity(6), root_of_unity(6) * g % P),
            ("trace_domain", g, g * g % P)]
    if ext == 1:
        return [("random", rnd.randrange(P), rnd.randrange(P))] + base
    pts = [("random", (rnd.randrange(P), rnd.randrange(P)), (rnd.randrange(P), rnd.randrange(P)))]
    pts += [(name, (z, 0), (zg, 0)) for name, z, zg in base]
    a, b = rnd.randrange(1, P), rnd.randrange(1, P)
    return pts + [("b_zero", (a, 0), (a * g % P, 0)), ("a_zero", (0, b), (0, b * g % P))]


OOD_SIZES = [16, 32, 64, 128, 512, 1024, 2048, 8192]  # E = 1, 1, 1, 2, 8, 16, 16, 16 and nw = 1 ... 1, 2, 8


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", OOD_SIZES)
def test_ood_frame(n, ext):
    """Every point class with the composition column counts in turn, and every count at the random point."""
    rnd = random.Random(1000 * ext + n)
    counts = [1, 7, 8] if ext == 1 else [2, 16]
    tp = class_polys(rnd, n, 28)
    cps = {c: class_polys(rnd, n, c) for c in counts}
    pts = ood_points(rnd, n, ext)
    runs = [(pt, counts[i % len(counts)]) for i, pt in enumerate(pts)] + [(pts[0], c) for c in counts[1:]]
    for (name, z, zg), ccols in runs:
        got = run_ood(tp, cps[ccols], n, ext, z, zg)
        want = ref.ood_frame(tp, cps[ccols], z, zg, ext)
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, f"n={n} ext={ext} point {name} ccols={ccols}: frame entries {bad[:8]} differ"


def test_ood_reference_cross_check():
    """The power-table evaluation the frames are compared with, against Horner's rule at one size."""
    rnd = random.Random(5)
    n = 128
    tp, cp = class_polys(rnd, n, 28), class_polys(rnd, n, 2)
    z, zg = (rnd.randrange(P), rnd.randrange(P)), (0, rnd.randrange(P))
    want = ref.ood_frame(tp, cp, z, zg, 2)
    assert want == ([ref.horner_ext(t, z) for t in tp] + [ref.horner_ext(t, zg) for t in tp] +
                    [ref.horner_ext(c, z) for c in cp])
    assert run_ood(tp, cp, n, 2, z, zg) == want


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,G", [(2048, 2), (2048, 8), (8192, 2), (8192, 8)])
def test_ood_shares_add_up(n, G, ext):
    """The G ranks' frames, added mod p, are the whole frame; a rank that owns no wave returns zeros (n = 2048 has two
    waves: of eight ranks only 3 and 7 own one)."""
    rnd = random.Random(77 * ext + n + G)
    ccols = 4 * ext
    tp, cp = class_polys(rnd, n, 28), class_polys(rnd, n, ccols)
    _, z, zg = ood_points(rnd, n, ext)[0]
    whole = run_ood(tp, cp, n, ext, z, zg)
    assert whole == ref.ood_frame(tp, cp, z, zg, ext)
    shares = [run_ood(tp, cp, n, ext, z, zg, r, G) for r in range(G)]
    zero = 0 if ext == 1 else (0, 0)
    add = (lambda x, y: (x + y) % P) if ext == 1 else ref.e_add
    total = [zero] * len(whole)
    for s in shares:
        total = [add(x, y) for x, y in zip(total, s)]
    assert total == whole
    nw = n // 1024
    owners = [r for r in range(G) if nw * r // G < nw * (r + 1) // G]
    if (n, G) == (2048, 8):
        assert owners == [3, 7]
    for r in range(G):
        if r not in owners:
            assert shares[r] == [zero] * len(whole), f"rank {r} owns no wave"
        else:
            assert shares[r] != [zero] * len(whole)


def test_ood_and_deep_refuse_bad_arguments():
    L = native.lib()
    n = 16
    tp, cp = bytes(16 * 28 * n), bytes(16 * 16 * n)
    one, out = elems([1, 0]), C.create_string_buffer(16 * 2 * 72)
    bad = [dict(n=8), dict(n=24), dict(ccols=0), dict(ccols=9), dict(ext=3), dict(ext=2, ccols=3), dict(ext=2, ccols=18),
           dict(z=elems([P, 0])), dict(zg=elems([2**128 - 1, 0])), dict(ext=2, ccols=2, z=elems([1, P])), dict(G=0),
           dict(rank=2, G=2), dict(rank=-1)]
    for kw in bad:
        a = dict(n=n, ccols=1, ext=1, z=one, zg=one, rank=0, G=1)
        a.update(kw)
        rc = L.zk_diag_ood(0, tp, cp, a["ccols"], a["n"], a["ext"], a["z"], a["zg"], a["rank"], a["G"], out)
        assert rc == native.ZK_ERR_INVALID_ARG and L.zk_last_error(), kw
    assert L.zk_diag_ood(0, None, cp, 1, n, 1, one, one, 0, 1, out) == native.ZK_ERR_INVALID_ARG
    al = elems([1, 0] * 28)
    for kw in (dict(z=elems([0, 0])), dict(zg=elems([0, 0])), dict(ext=2, ccols=2, z=elems([0, 0])), dict(n=8),
               dict(ccols=9), dict(at=elems([P] * 28)), dict(ac=elems([P] * 16)), dict(at=None)):
        a = dict(n=n, ccols=1, ext=1, z=one, zg=one, at=al, ac=al)
        a.update(kw)
        rc = L.zk_diag_deep(0, tp, cp, a["ccols"], a["n"], a["ext"], a["z"], a["zg"], a["at"], a["ac"], out)
        assert rc == native.ZK_ERR_INVALID_ARG and L.zk_last_error(), kw
    # the same buffers with good arguments: all-zero polynomials have an all-zero frame and quotient
    native.check(L.zk_diag_ood(0, tp, cp, 2, n, 2, one, one, 0, 1, out))
    assert out.raw[:16 * 2 * 58] == bytes(16 * 2 * 58)
    native.check(L.zk_diag_deep(0, tp, cp, 2, n, 2, one, one, al, al, out))
    assert out.raw[:32 * n] == bytes(32 * n)


# ---------------------------------------------------------------- DEEP
def run_deep(tp, cp, n, ext, z, zg, at, ac, parts=1):
    """zk_diag_deep, or with parts > 1 zk_diag_deep_parts: the same quotient by coefficient ranges"""
    assert native.device_count() > 0, "no GPU visible"
    out = C.create_string_buffer(16 * ext * n)
    flat = (lambda v: elems(v)) if ext == 1 else (lambda v: elems([c for pair in v for c in pair]))
    args = (0, cols_bytes(tp), cols_bytes(cp), len(cp), n, ext, point_bytes(z, ext), point_bytes(zg, ext), flat(at), flat(ac))
    if parts == 1:
        native.check(native.lib().zk_diag_deep(*args, out), "zk_diag_deep")
    else:
        native.check(native.lib().zk_diag_deep_parts(*args, parts, out), "zk_diag_deep_parts")
    v = ref_ints(out.raw)
    return v if ext == 1 else list(zip(v[:n], v[n:]))


def check_deep(tp, cp, n, ext, z, zg, at, ac, what, combined=None):
    got = run_deep(tp, cp, n, ext, z, zg, at, ac)
    zero = 0 if ext == 1 else (0, 0)
    assert got[n - 1] == zero, f"{what}: D_(n-1) is not zero"
    A, S = combined or ref.deep_combine(tp, cp, at, ac, ext)
    q1, _ = ref.divide_out(S, z, ext)
    q2, _ = ref.divide_out(A, zg, ext)
    want = [(x + y) % P for x, y in zip(q1, q2)] if ext == 1 else [ref.e_add(x, y) for x, y in zip(q1, q2)]
    bad = [k for k in range(n) if got[k] != want[k]]
    assert not bad, f"{what}: {len(bad)} coefficients differ, the first at k = {bad[:6]}"
    return got


def draw_fn(rnd, ext):
    return (lambda: rnd.randrange(P)) if ext == 1 else (lambda: (rnd.randrange(P), rnd.randrange(P)))


def lift(v, ext):
    return v if ext == 1 else (v, 0)


# one partial block, one full block of k_deep_div_g (256), two in one chunk of k_deep_div_q (2048), a full chunk,
# carries across two and four chunks
DEEP_SIZES = [16, 32, 64, 256, 512, 2048, 4096, 8192]


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", DEEP_SIZES)
def test_deep_points_and_coefficient_sets(n, ext):
    """Random polynomials: every point class (the OOD ones and, from n = 4096, a z of order 2048, where the hi half of
    every power table is all ones) with random coefficients, and every coefficient class at the random point."""
    rnd = random.Random(2000 * ext + n)
    ccols = (7 if n % 3 else 8) * ext
    draw = draw_fn(rnd, ext)
    tp = Polys([rnd.randrange(P) for _ in range(n)] for _ in range(28))
    cp = Polys([rnd.randrange(P) for _ in range(n)] for _ in range(ccols))
    at, ac = [draw() for _ in range(28)], [draw() for _ in range(ccols // ext)]
    combined = ref.deep_combine(tp, cp, at, ac, ext)
    pts = ood_points(rnd, n, ext)
    if n >= 4096:
        w, g = root_of_unity(11), root_of_unity(n.bit_length() - 1)
        pts.append(("order2048", lift(w, ext), lift(w * g % P, ext)))
    for name, z, zg in pts:
        check_deep(tp, cp, n, ext, z, zg, at, ac, f"n={n} ext={ext} point {name}", combined)
    _, z, zg = pts[0]
    sets = {"alpha 0": (0, None), "gamma 0": (None, 0), "all 1": (1, 1), "all p-1": (P - 1, P - 1), "both 0": (0, 0),
            "alpha p-1, gamma 1": (P - 1, 1)}
    if ext == 2:
        sets["X and p-1 X"] = ((0, 1), (0, P - 1))
    for name, (a, c) in sets.items():
        at2 = [draw() if a is None else (a if isinstance(a, tuple) else lift(a, ext)) for _ in range(28)]
        ac2 = [draw() if c is None else (c if isinstance(c, tuple) else lift(c, ext)) for _ in range(ccols // ext)]
        got = check_deep(tp, cp, n, ext, z, zg, at2, ac2, f"n={n} ext={ext} coefficients {name}")
        if name == "both 0":
            assert got == [0 if ext == 1 else (0, 0)] * n


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", DEEP_SIZES)
def test_deep_polynomial_classes(n, ext, part):
    """All 0, all p - 1, constants (the quotient is 0) and one coefficient at k = 0, n - 1 and at each side of the
    64 E, 256 and 2048 boundaries, the point classes taken in turn.  (Two halves, to keep each case short: the
    reference is plain Python.)"""
    rnd = random.Random(3000 * ext + n)
    ccols = 8 * ext
    draw = draw_fn(rnd, ext)
    at, ac = [draw() for _ in range(28)], [draw() for _ in range(ccols // ext)]
    pts = ood_points(rnd, n, ext)
    if n >= 4096:
        w, g = root_of_unity(11), root_of_unity(n.bit_length() - 1)
        pts.append(("order2048", lift(w, ext), lift(w * g % P, ext)))
    e64 = 64 * ood_e(n)
    ks = sorted({k for k in (0, n - 1, n - 2, e64 - 1, e64, 255, 256, 2047, 2048) if 0 <= k < n})
    zero = 0 if ext == 1 else (0, 0)
    cases = [("all 0", lambda: [0] * n), ("all p-1", lambda: [P - 1] * n),
             ("constants", lambda: unit(n, 0, rnd.randrange(1, P)))]
    cases += [(f"single at {k}", lambda k=k: unit(n, k)) for k in ks if k]
    cases += [(f"random single at {k}", lambda k=k: unit(n, k, rnd.randrange(1, P))) for k in (ks[-1], ks[len(ks) // 2])]
    for i, (name, make) in list(enumerate(cases))[part::2]:
        tp, cp = [make() for _ in range(28)], [make() for _ in range(ccols)]
        pname, z, zg = pts[i % len(pts)]
        got = check_deep(tp, cp, n, ext, z, zg, at, ac, f"n={n} ext={ext} polynomials {name} at point {pname}")
        if name in ("all 0", "constants"):
            assert got == [zero] * n, f"{name}: the quotient of a constant is 0"
    # the trace polynomials alone carry a coefficient (S = A): at the trace-domain point, where the point-wise
    # quotient has no value, and the composition columns alone (A = 0)
    _, z, zg = pts[4]
    k = ks[-2]
    if part == 0:
        check_deep([unit(n, k)] * 28, [[0] * n] * ccols, n, ext, z, zg, at, ac, f"n={n} ext={ext} trace only, k={k}")
        return
    check_deep([[0] * n] * 28, [unit(n, k)] * ccols, n, ext, z, zg, at, ac, f"n={n} ext={ext} composition only, k={k}")


# ---------------------------------------------------------------- DEEP by coefficient ranges
def same_polys(poly, count):
    """`count` copies of one polynomial, encoded once"""
    ps = Polys([poly] * count)
    ps.encoded = elems(poly) * count
    return ps


RANGE_CLASSES = ["random", "all 0", "all p-1", "before first boundary", "first boundary", "before last boundary",
                 "last boundary", "top", "random at boundary"]


@pytest.mark.parametrize("kind", RANGE_CLASSES)
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,parts", [(4096, 2), (8192, 4), (16384, 8)])
def test_deep_by_coefficient_ranges(n, parts, ext, kind):
    """deep_range_begin for every range, the later ranges' totals summed, deep_range_end for every range (a sharded
    proof's ranks on one device): the coefficients equal deep_poly's and the reference quotient.  A range is a whole
    number of 2048-coefficient chunks, so 4096 / 2 is the smallest split.  The polynomial classes of
    test_deep_polynomial_classes with the single coefficient at each side of a range boundary k0 = n / parts and
    n - n / parts (its suffix sum is carried into every earlier range, or into none) and at n - 1."""
    rnd = random.Random(4000 * ext + n + RANGE_CLASSES.index(kind))
    ccols = 8 * ext
    draw = draw_fn(rnd, ext)
    at, ac = [draw() for _ in range(28)], [draw() for _ in range(ccols // ext)]
    pts = ood_points(rnd, n, ext)
    w, g = root_of_unity(11), root_of_unity(n.bit_length() - 1)
    pts.append(("order2048", lift(w, ext), lift(w * g % P, ext)))
    pname, z, zg = pts[RANGE_CLASSES.index(kind) % len(pts)]
    kn = n // parts
    at_k = {"before first boundary": kn - 1, "first boundary": kn, "before last boundary": n - kn - 1,
            "last boundary": n - kn, "top": n - 1, "random at boundary": n - kn}
    if kind == "random":
        tp = Polys([rnd.randrange(P) for _ in range(n)] for _ in range(28))
        cp = Polys([rnd.randrange(P) for _ in range(n)] for _ in range(ccols))
    else:
        poly = {"all 0": [0] * n, "all p-1": [P - 1] * n}.get(kind) or \
            unit(n, at_k[kind], rnd.randrange(1, P) if kind.startswith("random") else 1)
        tp, cp = same_polys(poly, 28), same_polys(poly, ccols)
    what = f"n={n} parts={parts} ext={ext} polynomials {kind} at point {pname}"
    whole = check_deep(tp, cp, n, ext, z, zg, at, ac, what + " (one range)")
    split = run_deep(tp, cp, n, ext, z, zg, at, ac, parts)
    bad = [k for k in range(n) if split[k] != whole[k]]
    assert not bad, f"{what}: {len(bad)} coefficients differ from the one-range result, the first at k = {bad[:6]}"
    if kind == "all 0":
        assert split == [0 if ext == 1 else (0, 0)] * n


def test_deep_by_ranges_refuses_bad_arguments():
    L = native.lib()
    n = 4096
    tp, cp = bytes(16 * 28 * n), bytes(16 * 2 * n)
    one, al, out = elems([1, 0]), elems([1, 0] * 28), C.create_string_buffer(32 * n)
    for parts in (0, 1, 3, 4, 16):  # (4 ranges of 4096 coefficients would be 1024 each)
        rc = L.zk_diag_deep_parts(0, tp, cp, 2, n, 2, one, one, al, al, parts, out)
        assert rc == native.ZK_ERR_INVALID_ARG and L.zk_last_error(), parts
    native.check(L.zk_diag_deep_parts(0, tp, cp, 2, n, 2, one, one, al, al, 2, out))
    assert out.raw == bytes(32 * n)


# ---------------------------------------------------------------- one FRI layer: commit, then fold
def fri_store(layer, lb):
    """natural order -> the order the kernels read (FriLayout): index i at (i mod 2^lb) L / 2^lb + i / 2^lb"""
    L = len(layer)
    out = [None] * L
    for i, v in enumerate(layer):
        out[(i & ((1 << lb) - 1)) * (L >> lb) + (i >> lb)] = v
    return out


def run_fri_layer(layer, ext, fold, lb, wstride, alpha):
    """(root, next layer) of zk_diag_fri_layer; layer in natural order (ints; over E pairs)"""
    assert native.device_count() > 0, "no GPU visible"
    L = len(layer)
    stored = fri_store(layer, lb)
    data = elems(stored) if ext == 1 else elems([v[0] for v in stored]) + elems([v[1] for v in stored])
    root, nxt = C.create_string_buffer(32), C.create_string_buffer(16 * ext * (L // fold))
    native.check(native.lib().zk_diag_fri_layer(0, data, L, ext, fold, lb, wstride, point_bytes(alpha, ext), root, nxt),
                 "zk_diag_fri_layer")
    v = ref_ints(nxt.raw)
    return root.raw, v if ext == 1 else list(zip(v[:L // fold], v[L // fold:]))


def fri_layers(rnd, L, ext):
    """(name, layer): random, all 0, all p - 1 and a single non-zero entry"""
    draw = draw_fn(rnd, ext)
    zero, top = lift(0, ext), (P - 1 if ext == 1 else (P - 1, P - 1))
    single = [zero] * L
    single[rnd.randrange(L)] = draw()
    return [("random", [draw() for _ in range(L)]), ("all 0", [zero] * L), ("all p-1", [top] * L), ("single", single)]


def fri_alphas(rnd, ext):
    """random, 0 and 1; over E also a = 0 and b = 0"""
    if ext == 1:
        return [rnd.randrange(P), 0, 1]
    return [(rnd.randrange(P), rnd.randrange(P)), (0, 0), (1, 0), (0, rnd.randrange(1, P)), (rnd.randrange(1, P), 0)]


def check_fri_layer(oracle, layer, ext, fold, lb, wstride, alpha, what, want=None):
    root, nxt = run_fri_layer(layer, ext, fold, lb, wstride, alpha)
    want_root, want_next = want or (ref.fri_layer_root(oracle.blake3, layer, fold, ext), ref.fri_fold(layer, fold, alpha, ext))
    assert root == want_root, f"{what}: the layer's root differs"
    bad = [r for r in range(len(want_next)) if nxt[r] != want_next[r]]
    assert not bad, f"{what}: {len(bad)} folded values differ, the first at r = {bad[:6]}"


@pytest.mark.parametrize("lb", [0, 3])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("fold", [2, 4, 8, 16])
def test_fri_layer_smallest_tree(oracle, fold, ext, lb):
    """L = 16 fold: 16 rows, the smallest tree with more than one level; natural order and the coset-major order of a
    layer 0 with B = 8.  Every value class at a random alpha, every alpha class on the
    random layer.  (x_r comes from the tables of a plan of at least 128 points, so wstride = max(1, 128 / L).)"""
    rnd = random.Random(5000 * ext + 10 * fold + lb)
    L = 16 * fold
    wstride = max(1, 128 // L)
    layers, alphas = fri_layers(rnd, L, ext), fri_alphas(rnd, ext)
    for name, layer in layers:
        check_fri_layer(oracle, layer, ext, fold, lb, wstride, alphas[0], f"fold={fold} ext={ext} lb={lb} values {name}")
    root = ref.fri_layer_root(oracle.blake3, layers[0][1], fold, ext)
    for alpha in alphas[1:]:
        want = (root, ref.fri_fold(layers[0][1], fold, alpha, ext))
        check_fri_layer(oracle, layers[0][1], ext, fold, lb, wstride, alpha, f"fold={fold} ext={ext} lb={lb} alpha {alpha}",
                        want)
    if ext == 2:  # a layer of lifted base values folds to the base fold, lifted
        base = [v[0] for v in layers[0][1]]
        a = alphas[4]
        _, nxt = run_fri_layer([(v, 0) for v in base], 2, fold, lb, wstride, a)
        assert nxt == [(v, 0) for v in ref.fri_fold(base, fold, a[0], 1)]


@pytest.mark.parametrize("lb", [0, 3])
@pytest.mark.parametrize("ext", [1, 2])
def test_fri_layer_rows_past_the_split_tables_low_half(oracle, ext, lb):
    """L = 8192, fold 2, wstride 1: the rows 2048 .. 4095 take 1 / x_r from the hi half of pow_split's tables."""
    rnd = random.Random(6000 + 10 * ext + lb)
    name, layer = fri_layers(rnd, 8192, ext)[0]
    check_fri_layer(oracle, layer, ext, 2, lb, 1, fri_alphas(rnd, ext)[0], f"L=8192 ext={ext} lb={lb}")


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("fold", [2, 4, 8, 16])
def test_fri_layer_later_layer(oracle, fold, ext):
    """L = 1024 on a plan of N = 8192 points (wstride 8): a later layer, natural order."""
    rnd = random.Random(7000 + 10 * fold + ext)
    name, layer = fri_layers(rnd, 1024, ext)[0]
    check_fri_layer(oracle, layer, ext, fold, 0, 8, fri_alphas(rnd, ext)[0], f"L=1024 wstride=8 fold={fold} ext={ext}")


def test_fri_layer_refuses_bad_arguments():
    F = native.lib().zk_diag_fri_layer
    layer, one = bytes(32 * 256), elems([1, 0])
    root, nxt = C.create_string_buffer(32), C.create_string_buffer(32 * 128)
    good = dict(L=256, ext=1, fold=4, lb=0, wstride=1, alpha=one)
    for kw in (dict(L=192), dict(L=64, wstride=1), dict(ext=3), dict(fold=3), dict(fold=32), dict(wstride=3), dict(wstride=0),
               dict(lb=-1), dict(lb=7), dict(L=8, fold=4, wstride=16), dict(alpha=elems([P, 0])),
               dict(ext=2, alpha=elems([1, P])), dict(alpha=None)):
        a = dict(good)
        a.update(kw)
        rc = F(0, layer, a["L"], a["ext"], a["fold"], a["lb"], a["wstride"], a["alpha"], root, nxt)
        assert rc == native.ZK_ERR_INVALID_ARG and native.lib().zk_last_error(), kw
    assert F(0, None, 256, 1, 4, 0, 1, one, root, nxt) == native.ZK_ERR_INVALID_ARG


# ---------------------------------------------------------------- grinding, one launch
GRIND_SEED = bytes(range(7, 39))
GRIND_STARTS = [1, 2**32 - 100, 2**40]  # the second window crosses the nonce's 32-bit word boundary


def run_grind(seed, start, count, bits):
    assert native.device_count() > 0, "no GPU visible"
    best = C.c_uint64(0)
    native.check(native.lib().zk_diag_grind(0, seed, start, count, bits, C.byref(best)), "zk_diag_grind")
    return best.value


@pytest.fixture(scope="module")
def zeros(oracle):
    """nonce_zeros of the 65536 nonces from each start, hashed once (the reference's loop, at most 65536 per case)"""
    return {s: ref.zeros_table(oracle.blake3, GRIND_SEED, s, 65536) for s in GRIND_STARTS}


@pytest.mark.parametrize("start", GRIND_STARTS)
@pytest.mark.parametrize("count", [1, 255, 257, 65536])
@pytest.mark.parametrize("bits", [0, 8, 12])
def test_grind_window(zeros, bits, count, start):
    want = ref.grind_in_table(zeros[start], start, count, bits)
    if bits == 0:
        assert want == start
    assert run_grind(GRIND_SEED, start, count, bits) == want


def test_grind_picks_the_smallest_of_several_hits(oracle, zeros):
    for start in GRIND_STARTS:
        hits = [start + t for t, z in enumerate(zeros[start]) if z >= 8]
        assert len(hits) >= 2 and hits == ref.grind_hits(oracle.blake3, GRIND_SEED, start, 4096, 8) + \
            [h for h in hits if h >= start + 4096]
        assert run_grind(GRIND_SEED, start, 65536, 8) == hits[0]
        # windows that begin at the second hit, end at the third, and hold exactly two hits in one or two blocks
        assert run_grind(GRIND_SEED, hits[1], hits[2] - hits[1] + 1, 8) == hits[1]
        assert run_grind(GRIND_SEED, hits[0] + 1, hits[2] - hits[0], 8) == hits[1]
        # every nonce passes bits = 0: 65536 hits
        assert run_grind(GRIND_SEED, hits[1], 65536, 0) == hits[1]


def test_grind_window_without_a_hit(oracle, zeros):
    for start in GRIND_STARTS:
        hits = [t for t, z in enumerate(zeros[start]) if z >= 8]
        # the gap between the first two hits, and the nonces before the first
        lo, hi = hits[0] + 1, hits[1]
        assert hi > lo and ref.grind(oracle.blake3, GRIND_SEED, start + lo, hi - lo, 8) == ref.NO_NONCE
        assert run_grind(GRIND_SEED, start + lo, hi - lo, 8) == ref.NO_NONCE
        if hits[0]:
            assert run_grind(GRIND_SEED, start, hits[0], 8) == ref.NO_NONCE
        assert run_grind(GRIND_SEED, start, hits[0] + 1, 8) == start + hits[0]
        # no BLAKE3 output of these windows starts with 64 zero bits
        assert max(zeros[start]) < 64
        assert run_grind(GRIND_SEED, start, 65536, 64) == ref.NO_NONCE


def test_grind_hit_past_the_word_boundary(zeros):
    """A window that begins below 2^32 and whose only hit lies at or above it: the nonce's high word differs between
    the window's two ends."""
    start = GRIND_STARTS[1]
    hits = [t for t, z in enumerate(zeros[start]) if z >= 8]
    past = [t for t in hits if t >= 100]
    before = [t for t in hits if t < 100]
    first = before[-1] + 1 if before else 0
    assert first < 100 <= past[0]
    assert run_grind(GRIND_SEED, start + first, past[0] - first + 1, 8) == start + past[0] >= 2**32
    assert run_grind(GRIND_SEED, start + first, past[0] - first, 8) == ref.NO_NONCE
    # the largest window that fits below 2^64
    top = 2**64 - 1 - 256
    assert run_grind(GRIND_SEED, top, 256, 0) == top


def test_grind_refuses_bad_arguments():
    L = native.lib()
    best = C.c_uint64(0)
    for start, count, bits in ((1, 0, 8), (1, 16, -1), (1, 16, 65), (2**64 - 10, 16, 8)):
        assert L.zk_diag_grind(0, GRIND_SEED, start, count, bits, C.byref(best)) == native.ZK_ERR_INVALID_ARG
    assert L.zk_diag_grind(0, None, 1, 16, 8, C.byref(best)) == native.ZK_ERR_INVALID_ARG


# ---------------------------------------------------------------- grinding, whole proofs
@pytest.fixture(scope="module")
def gpu():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=1 << 10, max_blowup=32)
    yield g
    g.close()


@pytest.mark.parametrize("grinding", [7, 8, 22])
def test_proof_grinding_threshold_and_second_batch(gpu, oracle, grinding):
    """Grinding 7 is searched on the host and 8 on the GPU (grind_and_positions' threshold); at 22 this trace's nonce
    lies past the first batch of 2^22 nonces, so the batch loop runs a second launch.  Bytes equal the oracle's."""
    trace, pub = workload_trace(LR_PROGRAM, seed=0)
    opts = ProofOptions(num_queries=20, grinding_factor=grinding)
    proof, rec, _, rc = gpu.prove(trace, pub, opts, record=True)
    assert rc == 0
    if grinding == 22:
        assert rec.pow_nonce > 2**22, "the precondition of this case: the nonce is not in the first batch"
    opub = oracle_pub(oracle, pub)
    oproof, orec, _ = oracle.prove(trace, opub, oracle.default_options(num_queries=20, grinding=grinding))
    assert rec.pow_nonce == orec.pow_nonce
    compare_records(rec, orec)
    assert proof == oproof
    assert oracle.verify(proof, opub, 0) == (0, "")


# ---------------------------------------------------------------- openings
class Committed:
    """A trace committed through plug point 1 and its composition through plug point 3, with the oracle's proof of
    the same trace and options (roots, LDEs, positions, proof sections)."""

    def __init__(self, gpu, oracle, name, blowup):
        self.L = native.lib()
        trace, pub = small_trace(name)
        self.n, self.B = trace.shape[1], blowup
        self.N = self.n * blowup
        self.depth = self.N.bit_length() - 1
        self.h, self.cc = C.c_void_p(), C.c_void_p()
        self.root, self.croot = C.create_string_buffer(32), C.create_string_buffer(32)
        tb = np.ascontiguousarray(trace)
        native.check(self.L.zk_lde_new(gpu.handle, tb.ctypes.data, 28, self.n, blowup, C.byref(self.h), self.root))
        self.oproof, self.orec, od = oracle.prove(trace, oracle_pub(oracle, pub), oracle.default_options(blowup=blowup),
                                                  want=("trace_lde", "composition", "comp_lde"))
        self.ncols = self.orec.num_ccols
        comp = np.ascontiguousarray(od["composition"])
        native.check(self.L.zk_commit_composition(self.h, comp.ctypes.data, self.ncols, C.byref(self.cc), self.croot, None))
        self.lde = od["trace_lde"].reshape(self.N, 28, 2)
        self.clde = od["comp_lde"].reshape(-1, 2)[:self.N * self.ncols].reshape(self.N, self.ncols, 2)
        self.blake3 = oracle.blake3

    def close(self):
        self.L.zk_comp_free(self.cc)
        self.L.zk_lde_free(self.h)

    def query(self, which, positions, cap=1 << 16):
        """(rc, rows bytes, proof bytes, proof_len) of zk_lde_query / zk_comp_query"""
        k = len(positions)
        width = 28 if which == "trace" else self.ncols
        rows, pbuf, plen = C.create_string_buffer(max(1, k) * width * 16), C.create_string_buffer(max(1, cap)), C.c_size_t(cap)
        pos = (C.c_uint64 * max(1, k))(*positions)
        fn, handle = (self.L.zk_lde_query, self.h) if which == "trace" else (self.L.zk_comp_query, self.cc)
        rc = fn(handle, pos, k, rows, pbuf, C.byref(plen))
        return rc, rows.raw, pbuf.raw[:plen.value] if rc == 0 else b"", plen.value

    def check(self, which, positions):
        """rows equal the oracle's LDE rows in caller order, and rows + proof rebuild the committed root"""
        rc, rows, proof, _ = self.query(which, positions)
        assert rc == 0, (which, positions)
        table, width, root = (self.lde, 28, self.root) if which == "trace" else (self.clde, self.ncols, self.croot)
        assert rows == b"".join(table[p].tobytes() for p in positions), (which, positions)
        rb = 16 * width
        leaves = [ref.row_digest(self.blake3, rows[rb * q:rb * q + rb]) for q in range(len(positions))]
        assert ref.batch_root(self.blake3, leaves, list(positions), proof, self.depth) == root.raw, (which, positions)
        return rows, proof


@pytest.fixture(scope="module", params=[("pushadd64", 8), ("pushadd64", 32), ("lr128", 8), ("lr128", 32)],
                ids=lambda p: f"{p[0]}-b{p[1]}")
def committed(request, gpu, oracle):
    c = Committed(gpu, oracle, *request.param)
    yield c
    c.close()


def test_commitments_are_the_oracles(committed):
    c = committed
    assert c.n == (64 if c.N // c.B == 64 else 128)
    assert c.root.raw == bytes(c.orec.trace_root) and c.croot.raw == bytes(c.orec.constraint_root)


@pytest.mark.parametrize("which", ["trace", "comp"])
def test_opening_position_sets(committed, which):
    c, N = committed, committed.N
    rnd = random.Random(N)
    k = rnd.randrange(1, N // 2 - 1)
    sub = 8 * rnd.randrange(N // 8)
    sets = [[0], [N - 1], [rnd.randrange(N)], [0, N - 1], [2 * k, 2 * k + 1], [2 * k + 1, 2 * k + 2],
            list(range(sub, sub + 8)), list(range(N - 8, N)), sorted(rnd.sample(range(N), 255)), list(range(255)),
            list(range(0, 510, 2))]
    sizes = set()
    for s in sets:
        _, proof = c.check(which, s)
        sizes.add(len(proof))
    # a sibling pair needs no leaf digest and one path; a subtree of 8 shares all but depth - 3 digests
    _, pair = c.check(which, [2 * k, 2 * k + 1])
    assert len(pair) == 2 + 32 * (c.depth - 1)
    _, tree = c.check(which, list(range(sub, sub + 8)))
    assert len(tree) == 1 + 4 + 32 * (c.depth - 3)
    _, one = c.check(which, [5])
    assert len(one) == 2 + 32 * c.depth


@pytest.mark.parametrize("which", ["trace", "comp"])
def test_opening_unsorted_positions(committed, which):
    """Rows come back in the caller's order; the proof is the one of the sorted set."""
    c = committed
    rnd = random.Random(c.N + 1)
    for count in (2, 9, 40, 255):
        s = sorted(rnd.sample(range(c.N), count))
        rows, proof = c.check(which, s)
        shuffled = list(s)
        while shuffled == s:
            rnd.shuffle(shuffled)
        rows2, proof2 = c.check(which, shuffled)
        assert proof2 == proof
        rb = len(rows) // count
        assert [rows2[rb * i:rb * i + rb] for i in range(count)] == \
               [rows[rb * s.index(p):rb * s.index(p) + rb] for p in shuffled]
    c.check(which, [c.N - 1, 0])
    c.check(which, [7, 6])


def test_openings_of_a_proofs_positions_are_the_proofs_sections(committed):
    c = committed
    view, _ = wire.parse_proof(c.oproof)

    def body(section):
        at, width, ln = view.sections[section]
        return view.raw[at + width:at + width + ln]

    pos = [c.orec.positions[i] for i in range(c.orec.num_positions)]
    assert len(pos) == view.num_unique_queries and pos == sorted(set(pos))
    rows, proof = c.check("trace", pos)
    assert rows == body("trace_values") and proof == body("trace_proof")
    rows, proof = c.check("comp", pos)
    assert rows == body("constraint_values") and proof == body("constraint_proof")


@pytest.mark.parametrize("which", ["trace", "comp"])
def test_opening_proof_buffer_too_small(committed, which):
    c = committed
    pos = [3, 64, 65, c.N - 2]
    _, want = c.check(which, pos)
    for cap in (0, 1, len(want) - 1):
        rc, _, _, need = c.query(which, pos, cap)
        assert rc == native.ZK_ERR_BUFFER_TOO_SMALL and need == len(want), cap
    rc, _, proof, need = c.query(which, pos, len(want))
    assert rc == 0 and proof == want and need == len(want)


@pytest.mark.parametrize("which", ["trace", "comp"])
def test_opening_refuses_duplicate_and_bad_positions(committed, which):
    """MerkleTree::prove_batch refuses a repeated index (DuplicateLeafIndex); so do the plug points."""
    c = committed
    for pos in ([5, 5], [3, 9, 3], [0, 1, 2, 1], [c.N - 1] * 2, [7] * 255):
        rc, _, _, _ = c.query(which, pos)
        assert rc == native.ZK_ERR_INVALID_ARG and b"duplicate" in c.L.zk_last_error(), pos
    for pos in ([c.N], [0, 2**63], []):
        assert c.query(which, pos)[0] == native.ZK_ERR_INVALID_ARG, pos
    assert c.query(which, list(range(256)))[0] == native.ZK_ERR_INVALID_ARG  # more than 255 positions
    c.check(which, [5, 4])  # and the handle still answers


def test_read_frame_wraps(committed):
    """The next row of the steps N - B .. N - 1 is row step + B - N: the frame wraps round the LDE domain."""
    c = committed
    cur, nxt = C.create_string_buffer(28 * 16), C.create_string_buffer(28 * 16)
    for step in (c.N - 1, c.N - c.B, c.N - c.B - 1, 0, c.B - 1):
        native.check(c.L.zk_lde_read_frame(c.h, step, cur, nxt))
        assert cur.raw == c.lde[step].tobytes(), step
        assert nxt.raw == c.lde[(step + c.B) % c.N].tobytes(), step
    assert c.L.zk_lde_read_frame(c.h, c.N, cur, nxt) == native.ZK_ERR_INVALID_ARG
