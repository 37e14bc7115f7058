"""The front of the trace commitment, each piece called directly on the GPU and compared exactly (bytes or integers) with
tests/trace_classes_ref.py: column detection by k_sparse_detect (zk_diag_detect how = 0) and by the interpolation's
pass 1 (how = 1), the device-resident commitment that skips and fills what detection found (zk_diag_trace_commit), the
fills of a host trace's hinted columns (zk_diag_column_fills) and the expansion of packed narrow columns
(zk_diag_expand_narrow).

Detection columns hold exactly one interesting entry each, so nothing masks it: an edge value (0xFF / 0x100,
2^32 - 1 / 2^32, values whose low limb or low word is zero, p - 1) at an edge row (0, n - 2, either side of the 256-row
and 4096-row strides of the kernels), and p - 1 in row n - 1, which must never count.

The commitment's 28 crafted columns (column(), below):

     0        the AIR clock, or one of the near-clocks that must be refused
     2 4 6 8  sparse: last row 0, 1, p - 1, random          15 17 19 21 23 25 27  sparse, random last rows
    10 12 14  near-sparse, transformed densely: a single 1 at row 0, a single 1 at row n - 2, a single 2^64 at row n / 2
    16 18     dense with 8-bit and with 32-bit values (high limbs and words all zero)
    the rest  dense random -- so sparse and dense columns alternate and column 27 is sparse
"""
import ctypes as C

import numpy as np
import pytest

import trace_classes_ref as ref
from zkvm_amd import native

pytestmark = pytest.mark.gpu
P, W = ref.P, ref.W
VALUES = [1, 0xFF, 0x100, 2**32 - 1, 2**32, 2**32 + 0xFF, 2**63, 2**64, 2**96, P - 1]
BAD = native.ZK_ERR_INVALID_ARG


def edge_rows(n):
    return [0, 14] if n == 16 else [0, 1, 255, 256, 4095, 4096, n - 2]


# ---------------------------------------------------------------- the entry points
def detect(cols, c0, how, parts=1):
    """-> (flags[4 W], last[W], coefficients (k, n, 2) or None)"""
    assert native.device_count() > 0, "no GPU visible"
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    k, n = cols.shape[0], cols.shape[1]
    flags = np.full(4 * W, 7, dtype=np.uint32)
    last = np.full((W, 2), 7, dtype=np.uint64)
    polys = np.empty((k, n, 2), dtype=np.uint64) if how else None
    native.check(native.lib().zk_diag_detect(0, cols.ctypes.data, n, k, c0, how, parts, flags.ctypes.data,
                                             last.ctypes.data, polys.ctypes.data if how else None), "zk_diag_detect")
    return [int(f) for f in flags], ref.ints(last), polys


def commit(trace, blowup):
    """-> (flags, polys (W, n, 2), lde (W, blowup, n, 2), root)"""
    assert native.device_count() > 0, "no GPU visible"
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    n = trace.shape[1]
    flags = np.full(4 * W, 7, dtype=np.uint32)
    polys = np.empty((W, n, 2), dtype=np.uint64)
    lde = np.empty((W, blowup, n, 2), dtype=np.uint64)
    root = C.create_string_buffer(32)
    native.check(native.lib().zk_diag_trace_commit(0, trace.ctypes.data, n, blowup, flags.ctypes.data, polys.ctypes.data,
                                                   lde.ctypes.data, root), "zk_diag_trace_commit")
    return [int(f) for f in flags], polys, lde, root.raw


def differing_planes(got, want, names):
    """the planes that are not byte for byte the reference's, reported as test_coset_lde reports them"""
    bad = []
    for idx in np.ndindex(*got.shape[:-2]):
        d = np.flatnonzero((got[idx] != want[idx]).any(axis=1))
        if len(d):
            bad.append((names(idx), f"{len(d)} of {got.shape[-2]} differ, first at k = {d[0]}"))
    return bad


# ---------------------------------------------------------------- detection
_cache = {}


def detection_columns(n):
    """one column per (value, row) and the two extras; the reference's interpolation of each (four-step sizes)"""
    if n not in _cache:
        cols, names = [], []
        for v in VALUES:
            for row in edge_rows(n):
                col = np.zeros((n, 2), dtype=np.uint64)
                ref.put(col, row, v)
                ref.put(col, n - 1, P - 1)
                cols.append(col)
                names.append(f"{v:#x} at row {row}")
        cols.append(np.zeros((n, 2), dtype=np.uint64))
        names.append("all zero")
        only_last = np.zeros((n, 2), dtype=np.uint64)
        ref.put(only_last, n - 1, P - 1)
        cols.append(only_last)
        names.append("only the last row")
        _cache[n] = (np.array(cols), names)
    return _cache[n]


_polys = {}


def detection_polys(oracle, n):
    if n not in _polys:
        _polys[n] = ref.interpolate(oracle, detection_columns(n)[0])
    return _polys[n]


def check_detection(oracle, cols, names, c0, how, parts=1, polys_ref=None):
    flags, last, polys = detect(cols, c0, how, parts)
    want = ref.flag_array(cols, c0, clock_check=how == 0)
    rows = {0: "nonzero", 1: "w8", 2: "w32"}
    wrong = [(names[i - c0] if c0 <= i < c0 + len(cols) else f"untouched column {i}", rows[j], flags[j * W + i])
             for j in range(3) for i in range(W) if flags[j * W + i] != want[j * W + i]]
    assert not wrong, wrong
    assert flags[3 * W:] == want[3 * W:], "the clock flag (and the three entries after it)"
    assert last == (ref.last_array(cols, c0) if how == 0 else [0] * W)
    if how:
        bad = differing_planes(polys, polys_ref, lambda idx: names[idx[0]])
        assert not bad, bad  # fused detection skips no column
    return flags


@pytest.mark.parametrize("log_n,how", [(13, 0), (13, 1), (14, 0), (14, 1), (4, 0)])
def test_detection_at_every_value_and_row_edge(oracle, log_n, how):
    """70 (value, row) columns and 2 extras, 28 at a time (22 in one call at n = 16): flags and last rows are the
    reference's for every column; with fused detection the coefficients are the oracle's interpolation too."""
    n = 1 << log_n
    cols, names = detection_columns(n)
    assert len(cols) == (72 if n > 16 else 22)
    polys_ref = detection_polys(oracle, n) if how else None
    for b in range(0, len(cols), W):
        check_detection(oracle, cols[b:b + W], names[b:b + W], 0, how, polys_ref=polys_ref[b:b + W] if how else None)


@pytest.mark.parametrize("how", [0, 1])
def test_detection_of_a_column_list_that_starts_past_column_zero(oracle, how):
    """c0 = 5, 7 columns: their flags land at [5, 12) and every other entry stays 0"""
    n = 1 << 13
    cols, names = detection_columns(n)
    pick = [names.index(s) for s in ("0x100 at row 0", "0xff at row 8190", "0x100000000 at row 4096", "all zero",
                                     "0x10000000000000000 at row 4095", "only the last row", "0x1 at row 256")]
    polys_ref = detection_polys(oracle, n)[pick] if how else None
    flags = check_detection(oracle, cols[pick], [names[i] for i in pick], 5, how, polys_ref=polys_ref)
    assert flags[5:12] == [1, 1, 1, 0, 1, 0, 1] and flags[W + 5:W + 12] == [1, 0, 1, 0, 1, 0, 0]
    assert flags[2 * W + 5:2 * W + 12] == [0, 0, 1, 0, 1, 0, 0]
    assert not any(flags[j * W + c] for j in range(3) for c in range(W) if not 5 <= c < 12) and not any(flags[3 * W:])


@pytest.mark.parametrize("log_n,parts", [(13, 2), (14, 4)])
def test_detection_by_row_ranges(oracle, log_n, parts):
    """a sharded rank's share: `parts` launches over n / parts rows each into the same flags give the flags of one"""
    n = 1 << log_n
    cols, names = detection_columns(n)
    for b in range(0, len(cols), W):
        whole = check_detection(oracle, cols[b:b + W], names[b:b + W], 0, 0)
        assert check_detection(oracle, cols[b:b + W], names[b:b + W], 0, 0, parts=parts) == whole


def test_detect_refuses_bad_arguments():
    L = native.lib()
    buf = np.zeros((W + 1, 16, 2), dtype=np.uint64)
    flags, last = np.zeros(4 * W, dtype=np.uint32), np.zeros((W, 2), dtype=np.uint64)
    a = (flags.ctypes.data, last.ctypes.data)
    assert L.zk_diag_detect(0, buf.ctypes.data, 16, 28, 1, 0, 1, *a, None) == BAD   # c0 + ncols > 28
    assert L.zk_diag_detect(0, buf.ctypes.data, 12, 1, 0, 0, 1, *a, None) == BAD    # n not a power of two
    assert L.zk_diag_detect(0, buf.ctypes.data, 8, 1, 0, 0, 1, *a, None) == BAD     # n < 16
    assert L.zk_diag_detect(0, buf.ctypes.data, 16, 1, 0, 0, 2, *a, None) == BAD    # ranges of less than 4096 rows
    assert L.zk_diag_detect(0, buf.ctypes.data, 16, 1, 0, 0, 3, *a, None) == BAD    # parts
    assert L.zk_diag_detect(0, buf.ctypes.data, 16, 1, 0, 1, 1, *a, buf.ctypes.data) == BAD  # fused: four-step sizes
    assert L.zk_diag_detect(0, buf.ctypes.data, 16, 1, 0, 2, 1, *a, None) == BAD    # how
    assert L.zk_diag_detect(0, None, 16, 1, 0, 0, 1, *a, None) == BAD


# ---------------------------------------------------------------- the clock
def clock_column(n, variant, rng):
    """column 0: -> (column, is the clock)"""
    col = np.zeros((n, 2), dtype=np.uint64)
    col[:, 0] = np.arange(n, dtype=np.uint64)
    col[n - 1] = rng.integers(0, 2**64 - 1, size=2, dtype=np.uint64)  # the random last row
    if variant == "exact":
        return col, True
    if variant == "d = 0":
        ref.put(col, n - 1, n - 1)
        return col, True
    if variant == "row 0 holds 1":
        ref.put(col, 0, 1)
    elif variant == "row n-2 holds n-1":
        ref.put(col, n - 2, n - 1)
    elif variant == "row 4096 off by one":
        ref.put(col, 4096, 4097)
    elif variant == "row 7 wrong in the high limb":
        ref.put(col, 7, 7 + 2**64)
    elif variant == "every row shifted by one":
        col[:n - 1, 0] += np.uint64(1)
    else:
        raise KeyError(variant)
    return col, False


CLOCKS = ["exact", "d = 0", "row 0 holds 1", "row n-2 holds n-1", "row 4096 off by one", "row 7 wrong in the high limb",
          "every row shifted by one"]


@pytest.mark.parametrize("variant", CLOCKS)
def test_clock_detection(oracle, variant):
    n = 1 << 13
    col, is_clock = clock_column(n, variant, np.random.default_rng(7))
    flags = check_detection(oracle, col[None], [variant], 0, 0)
    assert flags[3 * W] == (0 if is_clock else 1)
    assert check_detection(oracle, col[None], [variant], 0, 0, parts=2) == flags


# ---------------------------------------------------------------- the commitment
SPARSE_LAST = {2: 0, 4: 1, 6: P - 1}  # (the other sparse columns' last rows are random)
SPARSE = [2, 4, 6, 8, 15, 17, 19, 21, 23, 25, 27]
NEAR_SPARSE = {10: lambda n: (0, 1), 12: lambda n: (n - 2, 1), 14: lambda n: (n // 2, 2**64)}


def crafted_trace(n, variant, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 2**64 - 1, size=(W, n, 2), dtype=np.uint64)  # dense random (hi <= 2^64 - 2: below p)
    t[0], is_clock = clock_column(n, variant, rng)
    for c in SPARSE + list(NEAR_SPARSE):
        t[c, :n - 1] = 0
        if c in SPARSE_LAST:
            ref.put(t[c], n - 1, SPARSE_LAST[c])
    for c, where in NEAR_SPARSE.items():
        ref.put(t[c], *where(n))
    t[16, :n - 1, 1] = 0
    t[16, :n - 1, 0] &= np.uint64(0xFF)
    t[18, :n - 1, 1] = 0
    t[18, :n - 1, 0] &= np.uint64(2**32 - 1)
    ref.put(t[16], 3, 0xFF)
    ref.put(t[18], n - 2, 2**32 - 1)
    return t, is_clock


def check_commit(oracle, log_n, blowup, variant):
    n = 1 << log_n
    trace, is_clock = crafted_trace(n, variant, 100 * log_n + blowup)
    flags, polys, lde, root = commit(trace, blowup)
    # (the commitment to a device-resident trace takes no width flags: nothing of it is uploaded)
    want = ref.flag_array(trace, 0, clock_check=True, widths=False)
    assert flags == want, [(i % W, i // W, flags[i], want[i]) for i in range(4 * W) if flags[i] != want[i]]
    assert [c for c in range(W) if not flags[c]] == SPARSE and flags[3 * W] == (0 if is_clock else 1)
    polys_ref = ref.interpolate(oracle, trace)
    bad = differing_planes(polys, polys_ref, lambda idx: f"column {idx[0]} coefficients")
    lde_ref = ref.coset_lde(oracle, polys_ref, blowup)
    bad += differing_planes(lde, lde_ref, lambda idx: f"column {idx[0]} coset {idx[1]}")
    assert not bad, bad
    assert root == ref.trace_root(oracle, lde_ref)


@pytest.mark.parametrize("log_n,blowup", [(13, 8), (13, 16), (14, 8), (16, 8)])
def test_commit_of_crafted_columns(oracle, log_n, blowup):
    """flags, every coefficient plane, every (column, coset) LDE plane and the root against the reference; blowup 16
    takes two launches of 8 cosets, the second starting at coset 8"""
    check_commit(oracle, log_n, blowup, "exact")


@pytest.mark.parametrize("variant", CLOCKS[1:])
def test_commit_with_clock_variants(oracle, variant):
    """column 0 filled from the identity column's tables when it is the clock (d = 0 included), transformed like any
    dense column when it is not"""
    check_commit(oracle, 13, 8, variant)


def test_trace_commit_refuses_bad_arguments():
    L = native.lib()
    buf = np.zeros(64, dtype=np.uint64)
    a = (buf.ctypes.data,) * 4
    assert L.zk_diag_trace_commit(0, buf.ctypes.data, 4096, 8, *a) == BAD   # no four-step size
    assert L.zk_diag_trace_commit(0, buf.ctypes.data, 8192, 4, *a) == BAD
    assert L.zk_diag_trace_commit(0, buf.ctypes.data, 8192, 24, *a) == BAD
    assert L.zk_diag_trace_commit(0, None, 8192, 8, *a) == BAD


# ---------------------------------------------------------------- the fills of hinted columns
def mask_of(cols):
    return sum(1 << c for c in cols)


FILL_CASES = {  # name: (sparse columns, clock: None / "d = 0" / "random", last rows of the sparse columns in order)
    "one column": ([17], None, ["random"]),
    "two adjacent runs, clock with d = 0": ([22, 23, 25, 26, 27], "d = 0", [0, 1, P - 1, "random", "random"]),
    "columns 12 .. 27": (list(range(12, 28)), None, [0, 1, P - 1] + ["random"] * 13),
    "the clock alone, random d": ([], "random", []),
    "a run that starts at column 1, clock with random d": ([1, 2], "random", [P - 1, 1]),
}


@pytest.mark.parametrize("blowup", [8, 16])
@pytest.mark.parametrize("case", list(FILL_CASES))
def test_column_fills(oracle, case, blowup):
    """k_sparse_fill and k_axpy_fill as a host trace's hinted columns get them: the planes are the oracle's transform
    of the column last e_(n-1), or of the clock column, written out in full"""
    assert native.device_count() > 0, "no GPU visible"
    n = 1 << 13
    sparse, clock, lasts = FILL_CASES[case]
    rng = np.random.default_rng(len(case) + blowup)
    rand = lambda: ref.ints(rng.integers(0, 2**64 - 1, size=2, dtype=np.uint64))[0]  # noqa: E731
    last = [rand() for _ in range(W)]  # (the columns not named carry values too: they must not leak)
    for c, v in zip(sparse, lasts):
        last[c] = rand() if v == "random" else v
    if clock == "d = 0":
        last[0] = n - 1
    named = ([0] if clock else []) + sparse
    full = np.zeros((len(named), n, 2), dtype=np.uint64)
    for k, c in enumerate(named):
        if c == 0 and clock:
            full[k, :, 0] = np.arange(n, dtype=np.uint64)
        ref.put(full[k], n - 1, last[c])
    polys = np.empty((len(named), n, 2), dtype=np.uint64)
    lde = np.empty((len(named), blowup, n, 2), dtype=np.uint64)
    last_arr = ref.column(last)
    native.check(native.lib().zk_diag_column_fills(0, last_arr.ctypes.data, mask_of(sparse), int(bool(clock)), n,
                                                   blowup, polys.ctypes.data, lde.ctypes.data), "zk_diag_column_fills")
    polys_ref = ref.interpolate(oracle, full)
    bad = differing_planes(polys, polys_ref, lambda idx: f"column {named[idx[0]]} coefficients")
    bad += differing_planes(lde, ref.coset_lde(oracle, polys_ref, blowup),
                            lambda idx: f"column {named[idx[0]]} coset {idx[1]}")
    assert not bad, bad


def test_column_fills_refuses_bad_arguments():
    L = native.lib()
    buf = np.zeros((W, 2), dtype=np.uint64)
    a = (buf.ctypes.data, buf.ctypes.data)
    assert L.zk_diag_column_fills(0, buf.ctypes.data, 1, 1, 8192, 8, *a) == BAD        # column 0 sparse and the clock
    assert L.zk_diag_column_fills(0, buf.ctypes.data, 0, 0, 8192, 8, *a) == BAD        # nothing named
    assert L.zk_diag_column_fills(0, buf.ctypes.data, 1 << 28, 0, 8192, 8, *a) == BAD  # a 29th column
    assert L.zk_diag_column_fills(0, buf.ctypes.data, 2, 0, 4096, 8, *a) == BAD        # no four-step size
    assert L.zk_diag_column_fills(0, buf.ctypes.data, 2, 0, 8192, 12, *a) == BAD


# ---------------------------------------------------------------- expansion of packed narrow columns
@pytest.mark.parametrize("n", [16, 1024, 4096, 8192])
def test_expand_narrow(n):
    """widths 1 and 4 mixed, columns in neither ascending nor adjacent order, offsets rounded up to 16 bytes as the
    upload plan lays them out, 0xAB in the padding and in each column's last-row slot (where last[k] must win)"""
    assert native.device_count() > 0, "no GPU visible"
    rng = np.random.default_rng(n)
    cols, widths = [20, 3, 27, 9, 14, 0], [1, 4, 1, 4, 4, 1]
    offs, total = ref.packed_layout(widths, n)
    total += 48  # (and a tail of padding)
    packed = bytearray(b"\xab" * total)
    last = [P - 1, 0, 2**64, 0xAB, int(rng.integers(1, 2**63)) << 64, 1]
    want = []
    for k, (w, off) in enumerate(zip(widths, offs)):
        top = 2**(8 * w) - 1
        rows = [int(v) for v in rng.integers(0, top + 1, size=n - 1, dtype=np.uint64)]
        for i, v in zip((0, 1, 2, 3, n - 2, n - 3, n - 5), (top, 0, top, 0xFF, top, 0, 0xFF)):
            rows[i] = v
        body, fits = ref.pack(rows, w)
        assert fits
        packed[off:off + len(body)] = body
        want.append(ref.expand(bytes(packed[off:off + w * n]), w, n, last[k]))
        assert want[-1][:n - 1] == rows and bytes(packed[off + w * (n - 1):off + w * n]) == b"\xab" * w
    out = np.empty((len(cols), n, 2), dtype=np.uint64)
    arr = lambda t, v: (t * len(v))(*v)  # noqa: E731
    last_arr = ref.column(last)
    native.check(native.lib().zk_diag_expand_narrow(0, bytes(packed), total, len(cols), arr(C.c_int32, cols),
                                                    arr(C.c_int32, widths), arr(C.c_uint64, offs),
                                                    last_arr.ctypes.data, n, out.ctypes.data), "zk_diag_expand_narrow")
    for k, c in enumerate(cols):
        got = ref.ints(out[k])
        d = [i for i in range(n) if got[i] != want[k][i]]
        assert not d, (f"column {c} (width {widths[k]})", f"{len(d)} of {n} rows differ, first at {d[0]}",
                       hex(got[d[0]]), hex(want[k][d[0]]))


def test_expand_narrow_refuses_bad_arguments():
    L = native.lib()
    packed = bytes(256)
    last, out = np.zeros((2, 2), dtype=np.uint64), np.zeros((2, 16, 2), dtype=np.uint64)
    arr = lambda t, v: (t * len(v))(*v)  # noqa: E731

    def call(cols, widths, offs, n=16, length=256):
        return L.zk_diag_expand_narrow(0, packed, length, len(cols), arr(C.c_int32, cols), arr(C.c_int32, widths),
                                       arr(C.c_uint64, offs), last.ctypes.data, n, out.ctypes.data)

    assert call([3, 3], [1, 1], [0, 16]) == BAD      # a column twice
    assert call([28], [1], [0]) == BAD               # no such column
    assert call([3], [2], [0]) == BAD                # width
    assert call([3], [4], [8]) == BAD                # offset not a multiple of 16
    assert call([3], [4], [208]) == BAD              # 64 bytes of rows from offset 208 end past the buffer
    assert call([3], [1], [0], n=8) == BAD
    assert call([3], [4], [0], length=63) == BAD
