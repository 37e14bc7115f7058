"""The host checks behind a host trace's column hints -- pack_rows, zero_rows, clock_rows, same_rows (trace_commit.hip,
through zk_diag_host_rows) -- and row_tasks, which splits them into pool tasks (host_pool.hpp, through
zk_diag_row_tasks), against tests/trace_classes_ref.py.  Runs without a GPU.

Every check is a statement about rows [r0, r1) of a column and nothing else: a column that is good for a check gets one
offending entry, in turn just inside the range (its first and its last row), just outside it (the row before and the
row after), with every edge value (0xFF / 0x100, 2^32 - 1 / 2^32, values whose low limb is good and whose high limb is
not); the verdict must be the reference's, which is computed from the definition for that very column and range."""
import ctypes as C

import numpy as np
import pytest

import trace_classes_ref as ref
from zkvm_amd import native

P = ref.P
N = 64
VALUES = [1, 0xFF, 0x100, 2**32 - 1, 2**32, 2**32 + 0xFF, 2**63, 2**64, 2**96, P - 1]
RANGES = [(0, N - 1), (5, 6), (7, 7), (3, 41), (1, N - 2), (17, 18)]  # whole, one row, empty, odd ends
PACK, ZERO, CLOCK, SAME = 0, 1, 2, 3
SENTINEL = 0xCD


def host_rows(op, col, r0, r1, width=0, aux=None, dst=None):
    rc = native.lib().zk_diag_host_rows(op, col.ctypes.data, aux.ctypes.data if aux is not None else None, r0, r1,
                                        width, dst.ctypes.data if dst is not None else None)
    assert rc in (0, 1), native.lib().zk_last_error()
    return bool(rc)


def placements(r0, r1):
    """(row, where) of the offending entry: the range's first and last row, the rows just outside it"""
    spots = [(r0 - 1, "before"), (r1, "after")]
    if r1 > r0:
        spots += [(r0, "first"), (r1 - 1, "last")]
    return [(row, where) for row, where in spots if 0 <= row < N]


def edits(good):
    """the offending values for a row whose good value is `good`: the edge values, and the good low limb under a high
    limb that is not zero (wrong in the high limb only)"""
    return VALUES + [good + 2**64, good + 2**96, good + 2**127]


def small_values(width):
    rnd = np.random.default_rng(width)
    vals = [int(v) for v in rnd.integers(0, 2**(8 * width), size=N, dtype=np.uint64)]
    vals[2], vals[3], vals[4] = 0, 2**(8 * width) - 1, 1
    return vals


def test_reference_flag_forms_agree():
    """flags_of (Python ints) and flags_of_column (limbs) on every edge value at the rows that count and the one that
    does not"""
    for base in ([0] * N, list(range(N))):
        for v in [0] + VALUES + [5 + 2**64]:
            for row in (0, 5, N - 2, N - 1):
                vals = list(base)
                vals[row] = v
                assert ref.flags_of(vals) == ref.flags_of_column(ref.column(vals)), (v, row)
    assert ref.flags_of([0] * (N - 1) + [P - 1]) == {"nonzero": 0, "w8": 0, "w32": 0, "not_clock": 1}
    assert ref.flags_of(list(range(N - 1)) + [P - 1]) == {"nonzero": 1, "w8": 0, "w32": 0, "not_clock": 0}
    assert ref.flags_of([0] * (N - 2) + [0x100, 0]) == {"nonzero": 1, "w8": 1, "w32": 0, "not_clock": 1}


def test_reference_pack_expand_round_trip():
    for width in (1, 4):
        vals = small_values(width)
        packed, fits = ref.pack(vals[:-1], width)
        assert fits and len(packed) == width * (N - 1)
        assert ref.expand(packed + b"\xab" * width, width, N, P - 1) == vals[:-1] + [P - 1]
        assert not ref.pack([2**(8 * width)], width)[1] and ref.pack([2**(8 * width) - 1], width)[1]
    assert ref.packed_layout([1, 4, 1], 24) == ([0, 32, 128], 160)


def test_reference_commitment_is_the_oracle_provers(oracle):
    """interpolate, coset_lde and trace_root put together give the coefficients and the trace root of the oracle's own
    proof of a real trace"""
    from golden_large import oracle_pub
    from zkvm_amd.prover import make_pub_inputs, vm_trace
    from zkvm_amd.workloads import LR_PROGRAM, make_workload
    w = make_workload(LR_PROGRAM, seed=1)
    trace, outputs, h = vm_trace(LR_PROGRAM, w.public, w.secret, w.server_key, w.last_row)
    pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    _, rec, held = oracle.prove(trace, oracle_pub(oracle, pub), want=("trace_polys",))
    polys = ref.interpolate(oracle, trace)
    assert (polys.reshape(-1, 2) == held["trace_polys"]).all()
    assert ref.trace_root(oracle, ref.coset_lde(oracle, polys, 8)) == bytes(rec.trace_root)


@pytest.mark.parametrize("r0,r1", RANGES)
def test_zero_rows(r0, r1):
    seen = set()
    for row, where in placements(r0, r1):
        for v in edits(0):
            vals = [0] * N
            vals[row] = v
            want = all(x == 0 for x in vals[r0:r1])
            assert host_rows(ZERO, ref.column(vals), r0, r1) == want, (row, where, hex(v))
            seen.add((where, want))
    assert host_rows(ZERO, ref.column([0] * N), r0, r1)
    assert {w for w, ok in seen if not ok} == ({"first", "last"} if r1 > r0 else set())


@pytest.mark.parametrize("r0,r1", RANGES)
def test_clock_rows(r0, r1):
    clock = list(range(N))
    seen = set()
    for row, where in placements(r0, r1):
        for v in edits(row) + [row + 1, row - 1 if row else 2]:
            if v == row:
                continue  # (an edge value that happens to be the row's own number)
            vals = list(clock)
            vals[row] = v
            want = all(x == i for i, x in enumerate(vals) if r0 <= i < r1)
            assert host_rows(CLOCK, ref.column(vals), r0, r1) == want, (row, where, hex(v))
            seen.add((where, want))
    assert host_rows(CLOCK, ref.column(clock), r0, r1)
    assert {w for w, ok in seen if not ok} == ({"first", "last"} if r1 > r0 else set())


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("r0,r1", RANGES)
def test_pack_rows(r0, r1, width):
    """the verdict, the bytes of every row of the range that fits (also when another row does not), and nothing
    written outside dst[width r0, width r1)"""
    good = small_values(width)
    verdicts = set()
    for row, where in placements(r0, r1) + [(None, "none")]:
        for v in edits(good[row]) if row is not None else [0]:
            vals = list(good)
            if row is not None:
                vals[row] = v
            dst = np.full(width * N, SENTINEL, dtype=np.uint8)
            got = host_rows(PACK, ref.column(vals), r0, r1, width, dst=dst)
            want_bytes, want = ref.pack(vals[r0:r1], width)
            assert got == want, (row, where, hex(v))
            verdicts.add((where, want))
            out = dst.tobytes()
            for i in range(r0, r1):
                if vals[i] < 2**(8 * width):
                    assert out[width * i:width * (i + 1)] == want_bytes[width * (i - r0):width * (i - r0 + 1)], (row, i)
            assert set(out[:width * r0]) <= {SENTINEL} and set(out[width * r1:]) <= {SENTINEL}, (row, where)
    assert ("none", True) in verdicts
    assert {w for w, ok in verdicts if not ok} == ({"first", "last"} if r1 > r0 else set())


@pytest.mark.parametrize("width", [1, 4, 16])
@pytest.mark.parametrize("r0,r1", RANGES)
def test_same_rows(r0, r1, width):
    """a column against a snapshot's host copy: packed integers (width 1, 4) or the elements themselves (16)"""
    if width == 16:
        rnd = np.random.default_rng(16)
        good = [int(a) | (int(b) << 64) for a, b in rnd.integers(0, 2**64 - 1, size=(N, 2), dtype=np.uint64)]
        snap = np.frombuffer(ref.column(good).tobytes(), dtype=np.uint8).copy()
    else:
        good = small_values(width)
        snap = np.frombuffer(ref.pack(good, width)[0], dtype=np.uint8).copy()
    assert host_rows(SAME, ref.column(good), r0, r1, width, aux=snap)
    seen = set()
    for row, where in placements(r0, r1):
        low = good[row] % 2**64
        for v in VALUES + [low + 2**64, (low + 2**96) % 2**128, good[row] ^ 1, good[row] ^ 2**(8 * min(width, 8) - 1)]:
            if v == good[row]:
                continue
            vals = list(good)
            vals[row] = v
            want = vals[r0:r1] == good[r0:r1]
            assert host_rows(SAME, ref.column(vals), r0, r1, width, aux=snap) == want, (row, where, hex(v))
            seen.add((where, want))
    assert {w for w, ok in seen if not ok} == ({"first", "last"} if r1 > r0 else set())


def test_host_rows_refuses_bad_arguments():
    col = ref.column([0] * N)
    L = native.lib()
    bad = native.ZK_ERR_INVALID_ARG
    dst = np.zeros(4 * N, dtype=np.uint8)
    assert L.zk_diag_host_rows(4, col.ctypes.data, None, 0, 1, 0, None) == bad       # unknown op
    assert L.zk_diag_host_rows(ZERO, None, None, 0, 1, 0, None) == bad               # no column
    assert L.zk_diag_host_rows(ZERO, col.ctypes.data, None, 2, 1, 0, None) == bad    # r0 > r1
    assert L.zk_diag_host_rows(PACK, col.ctypes.data, None, 0, 1, 2, dst.ctypes.data) == bad   # width
    assert L.zk_diag_host_rows(PACK, col.ctypes.data, None, 0, 1, 4, None) == bad    # no dst
    assert L.zk_diag_host_rows(SAME, col.ctypes.data, None, 0, 1, 4, None) == bad    # no snapshot
    assert L.zk_diag_host_rows(SAME, col.ctypes.data, dst.ctypes.data, 0, 1, 8, None) == bad


@pytest.mark.parametrize("r0,r1,R", [(0, 2**18 + 5, 2**18), (0, 2**16 - 1, 2**16), (3, 4, 1), (0, 0, 8),
                                     (5, 5 + 3 * 7, 7), (1, 30, 4)])
def test_row_tasks_cover_the_range_once(r0, r1, R):
    """the tasks' (first, end) pairs: none empty or longer than R, disjoint, and once sorted they tile [r0, r1)"""
    want = -(-(r1 - r0) // R)
    cap = want + 2
    out = (C.c_uint64 * (2 * cap))()
    count = C.c_size_t(99)
    native.check(native.lib().zk_diag_row_tasks(r0, r1, R, out, cap, C.byref(count)), "zk_diag_row_tasks")
    assert count.value == want
    pairs = sorted((out[2 * k], out[2 * k + 1]) for k in range(count.value))
    if r0 == r1:
        assert pairs == []
        return
    assert pairs[0][0] == r0 and pairs[-1][1] == r1
    for (a, b), (a2, _) in zip(pairs, pairs[1:] + [(r1, r1)]):
        assert a < b <= a + R and b == a2, pairs
    assert pairs == [(a, min(a + R, r1)) for a in range(r0, r1, R)]


def test_row_tasks_refuses_bad_arguments():
    out = (C.c_uint64 * 4)()
    count = C.c_size_t(0)
    L = native.lib()
    assert L.zk_diag_row_tasks(0, 8, 0, out, 2, C.byref(count)) == native.ZK_ERR_INVALID_ARG
    assert L.zk_diag_row_tasks(0, 8, 4, None, 2, C.byref(count)) == native.ZK_ERR_INVALID_ARG
    assert L.zk_diag_row_tasks(0, 12, 4, out, 2, C.byref(count)) == native.ZK_ERR_BUFFER_TOO_SMALL and count.value == 3
