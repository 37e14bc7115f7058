"""The sharded degree check, the parts that need no GPU (csrc/shard_agree.hpp through the test entry points bound in
zkvm_amd/shard_diag.py): the fixed layouts of the degree partial and of the control record's new field, the pure merge
of the ranks' partials (merge_degrees), and the agreement on the switch.  Integers and strings: all exact.
"""
import ctypes as C

import pytest

from degrees_ref import ZK_ERR_DEGREES, ZK_OK, expected, make_report, message, pushadd_zero_last_row
from test_shard_agree_cpu import records
from zkvm_amd import native, shard_diag

WORLDS = (2, 4, 8)
N = 128


def partials(world, n=N):
    """All-zero partials of `world` ranks: every quotient zero in every coefficient range."""
    kg = n // world
    P = [native.DegPartial() for _ in range(world)]
    for r, p in enumerate(P):
        p.version, p.rank, p.status, p.first, p.count = native.AGREE_VERSION, r, ZK_OK, r * kg, kg
    return P


def put(p, k, index):
    p.top[k] = index
    p.nonzero |= 1 << k


def split(n, world, actual, zero_mask=0):
    """Partials as `world` ranks report quotients whose ONLY non-zero coefficient is the top one: coefficient
    actual[k] = k1 + n k2 belongs to the rank whose range holds k1."""
    kg = n // world
    P = partials(world, n)
    for k, a in enumerate(actual):
        if not (zero_mask >> k) & 1:
            put(P[(a % n) // kg], k, a)
    return P


def test_symbols_and_layouts():
    L = native.lib()
    for name in ("zk_degrees_sharded",) + shard_diag.DEGREE_SYMBOLS:
        assert hasattr(L, name), name
    assert "zk_degrees_sharded" in native.EXPORTED
    D = native.DegPartial
    assert C.sizeof(D) == 312
    assert (D.version.offset, D.rank.offset, D.status.offset, D.nonzero.offset) == (0, 4, 8, 12)
    assert (D.first.offset, D.count.offset, D.top.offset, D.msg.offset) == (16, 24, 32, 192)
    assert D.top.size == 160 and D.msg.size == native.AGREE_MSG
    R = native.AgreeRecord
    assert C.sizeof(R) == 256 and R.validate_degrees.offset == 240 and R.msg.offset == 120
    assert R.reserved.offset == 244 and R.reserved.size == 12
    A = native.Agreement
    assert A.validate_degrees.offset == A.field.offset + 32 and C.sizeof(A) == A.validate_degrees.offset + 8


@pytest.mark.parametrize("world", WORLDS)
def test_all_zero_partials(world):
    rc, d, msg = shard_diag.merge_degrees(partials(world), N)
    assert d["actual"] == [0] * 20 and d["zero_mask"] == (1 << 20) - 1 and d["max_actual"] == 0
    assert d["expected"] == expected(N) and d["mismatch_mask"] == (1 << 20) - 1 and d["over_mask"] == 0
    assert d["ce_len_needed"] == 2 * N and (d["trace_len"], d["ce_len"]) == (N, 8 * N)
    assert rc == ZK_ERR_DEGREES and msg == message(d)


@pytest.mark.parametrize("world", WORLDS)
def test_the_top_comes_from_the_right_rank(world):
    kg = N // world
    for owner in range(world):
        P = partials(world)
        for r in range(world):  # every rank reports something in its range; `owner` the highest
            put(P[r], 3, r * kg + (5 * N if r == owner else N))
        put(P[owner], 0, owner * kg)  # a constant-block coefficient that only one rank holds
        rc, d, _ = shard_diag.merge_degrees(P, N)
        assert d["actual"][3] == owner * kg + 5 * N and d["actual"][0] == owner * kg
        assert d["zero_mask"] == ((1 << 20) - 1) & ~0b1001


@pytest.mark.parametrize("world", WORLDS)
def test_a_higher_block_beats_a_higher_range(world):
    """Rank 0 reports index 0 + 7n, rank G - 1 reports n - 1 + 6n: the maximum is over the GLOBAL index."""
    P = partials(world)
    put(P[0], 7, 7 * N)
    put(P[world - 1], 7, N - 1 + 6 * N)
    _, d, _ = shard_diag.merge_degrees(P, N)
    assert d["actual"][7] == 7 * N and d["max_actual"] == 7 * N and d["ce_len_needed"] == 8 * N
    assert d["over_mask"] == 1 << 7
    # a top without its non-zero bit is not a coefficient (an all-zero range reports 0 with the bit clear)
    P = partials(world)
    P[0].top[2] = 5
    _, d, _ = shard_diag.merge_degrees(P, N)
    assert d["actual"][2] == 0 and (d["zero_mask"] >> 2) & 1


@pytest.mark.parametrize("world", WORLDS)
def test_an_error_status_names_the_lowest_rank(world):
    P = partials(world)
    P[world - 1].status, P[world - 1].msg = native.ZK_ERR_DEVICE, b"HIP error: unspecified launch failure"
    rc, _, msg = shard_diag.merge_degrees(P, N)
    assert rc == native.ZK_ERR_PEER
    assert msg == (f"rank {world - 1} could not check its coefficients: {native.ZK_ERR_DEVICE}: "
                   "HIP error: unspecified launch failure")
    P[1].status, P[1].msg = native.ZK_ERR_OUT_OF_MEMORY, b"x" * native.AGREE_MSG
    rc, _, msg = shard_diag.merge_degrees(P, N)
    assert rc == native.ZK_ERR_PEER
    assert msg == f"rank 1 could not check its coefficients: {native.ZK_ERR_OUT_OF_MEMORY}: " + "x" * native.AGREE_MSG


@pytest.mark.parametrize("world", WORLDS)
def test_a_wrong_version_and_an_index_outside_the_domain_are_refused(world):
    P = partials(world)
    P[world - 1].version = native.AGREE_VERSION + 1
    rc, _, msg = shard_diag.merge_degrees(P, N)
    assert rc == native.ZK_ERR_PEER and msg == f"rank {world - 1} sent a degree partial of layout version 2"
    P = partials(world)
    put(P[0], 0, 8 * N)
    rc, _, msg = shard_diag.merge_degrees(P, N)
    assert rc == native.ZK_ERR_PEER and msg == "rank 0 reported a coefficient outside the domain"


@pytest.mark.parametrize("n", [128, 512, 8192])
@pytest.mark.parametrize("world", WORLDS)
def test_merged_report_equals_the_single_gpu_report(world, n):
    """Partials built from the closed forms: the merged zk_degrees is the report zk_degrees_device fills (make_report
    is the statement tests/test_gpu_degrees.py pins it with), status and message included."""
    rc, d, msg = shard_diag.merge_degrees(split(n, world, expected(n)), n)
    assert d == make_report(n, expected(n), 0) and rc == ZK_OK
    zero_mask = sum(1 << k for k in (4, 5, 6, 7, 9, 10))
    act = pushadd_zero_last_row(n)
    rc, d, msg = shard_diag.merge_degrees(split(n, world, act, zero_mask), n)
    want = make_report(n, act, zero_mask)
    assert d == want and rc == ZK_ERR_DEGREES and msg == message(want)


@pytest.mark.parametrize("world", WORLDS)
def test_agreement_on_the_switch(world):
    rc, d, msg = shard_diag.agree(records(world))
    assert rc == ZK_OK and d["validate_degrees"] == 0 and d["validate"] == 0
    for rank in (0, world - 1):
        R = records(world)
        R[rank].validate_degrees = 1
        rc, d, _ = shard_diag.agree(R)
        assert rc == ZK_OK and d["validate_degrees"] == 1 and d["validate"] == 0
    # the two switches decide apart
    R = records(world)
    R[0].validate = 1
    assert shard_diag.agree(R)[1]["validate_degrees"] == 0
    # a record of an older build: the once-reserved bytes all zero reads as "off"
    R = records(world)
    raw = bytearray(bytes(R))
    assert all(raw[256 * r + 240:256 * r + 256] == bytes(16) for r in range(world))
    old = (native.AgreeRecord * world).from_buffer_copy(bytes(raw))
    assert shard_diag.agree(old)[1]["validate_degrees"] == 0
