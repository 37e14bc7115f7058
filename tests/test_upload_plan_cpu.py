"""The upload plan of a host-trace commitment (csrc/upload_plan.hpp through zk_diag_upload_plan): which columns a proof
takes as sparse, narrow, clock, fixed and virtual, the upload items and the fused hash prefix, from hand-built hint
sets.  Runs without a GPU.  The expected values are worked out here from the rules, not read from the planner:

  - hints count only with detection, ZK_SPARSE, hint_ok and a completed proof's findings (have);
  - nw8 = hinted nw8 & ~sparse, nw32 = hinted nw32 & ~sparse & ~nw8 (ZK_NARROW); the clock is bit 0 of nw32, taken out
    of it (ZK_CLOCK, clk_off); fixm = snapshot mask & ~sparse with a snapshot, snap_now without (ZK_FIXED, fixed_off);
    virt = sparse columns >= 22 (ZK_VIRTUAL, no_virtual);
  - columns: clock and fixed ones in no list; sparse -> hin (hnv: not virtual); narrow -> nar; the rest dense;
  - dense groups of 4, the last four columns as 2 + 2; narrow parts 1, 2, 2, ... (latency) or ceil(nn / 2) + rest;
  - packed offsets: width * n rounded up to 16 bytes per column;
  - at most ZK_UPLOAD_GROUPS_MAX = 14 items: ngroups + (1 on the latency schedule with narrow columns, else np + 1);
  - fuse_nb: leading blocks of 4 columns each fixed, the derived clock, or sparse and not virtual (fixm != 0,
    ZK_FIXED_FUSE).
"""
from __future__ import annotations

import ctypes as C
import itertools

import pytest

from zkvm_amd import native

W = 28
GROUPS_MAX = 14
SWITCHES = ["sparse", "narrow", "clock", "fixed", "fixed_fuse", "virtual"]


def mask(cols):
    m = 0
    for c in cols:
        m |= 1 << c
    return m


def cols_of(m):
    return [c for c in range(W) if (m >> c) & 1]


def plan(n=1 << 13, have=True, sparse=0, nw8=0, nw32=0, clk_off=False, fixed_off=False, snap=False, snap_mask=0,
         hint_ok=True, no_virtual=False, lat=False, detect=True, off=()):
    sw = sum(1 << i for i, s in enumerate(SWITCHES) if s not in off)
    arr = (C.c_uint32 * 13)(have, sparse, nw8, nw32, clk_off, fixed_off, snap, snap_mask, hint_ok, no_virtual, lat,
                            detect, sw)
    masks, counts = (C.c_uint32 * 8)(), (C.c_int32 * 7)()
    cols, width, offs = (C.c_int32 * (4 * W))(), (C.c_int32 * W)(), (C.c_uint64 * (W + 1))()
    pb, gsz = (C.c_int32 * (W + 1))(), (C.c_int32 * W)()
    rc = native.lib().zk_diag_upload_plan(arr, n, masks, counts, cols, width, offs, pb, gsz)
    nd, nh, nhv, nn, np_, ng, fuse = list(counts)
    return {
        "rc": rc,
        "hint": masks[0], "nw8": masks[1], "nw32": masks[2], "clk": masks[3], "fixm": masks[4], "virt": masks[5],
        "snap_now": masks[6], "lat": masks[7],
        "dense": list(cols[0:nd]), "hin": list(cols[W:W + nh]), "hnv": list(cols[2 * W:2 * W + nhv]),
        "nar": list(cols[3 * W:3 * W + nn]), "width": list(width[:nn]), "off": list(offs[:nn]), "pack_bytes": offs[W],
        "pb": list(pb[:np_ + 1]), "np": np_, "gsz": list(gsz[:ng]), "fuse_nb": fuse,
    }


def groups(nd):
    """Dense groups of 4, the last four columns as 2 + 2."""
    out, left = [], nd
    while left > 0:
        k = 2 if left == 4 else 4 if left > 4 else 2 if left > 2 else left
        out.append(k)
        left -= k
    return out


def parts(nn, lat):
    if nn == 0:
        return []
    if lat:
        out, left = [], nn
        while left > 0:
            k = min(left, 1 if not out else 2)
            out.append(k)
            left -= k
        return out
    return [nn] if nn == 1 else [(nn + 1) // 2, nn // 2]


def part_sizes(p):
    return [b - a for a, b in zip(p["pb"], p["pb"][1:])]


# the benchmark program's classes: stack registers 23 .. 27 sparse, seven 8-bit columns, the clock found 32-bit,
# columns 1 .. 11 held by the snapshot
SPARSE = mask(range(23, 28))
NW8 = mask([1, 2, 3, 4, 5, 6, 11])
FIXED = mask(range(1, 12))
BENCH = dict(sparse=SPARSE, nw8=NW8, nw32=1)


def test_group_rule_examples():
    assert groups(28) == [4, 4, 4, 4, 4, 4, 2, 2] and groups(7) == [4, 2, 1] and groups(5) == [4, 1]
    assert groups(3) == [2, 1] and groups(11) == [4, 4, 2, 1]


@pytest.mark.parametrize("kw", [dict(have=False), dict(have=False, lat=True), dict(hint_ok=False, **BENCH),
                                dict(detect=False, **BENCH), dict(off=("sparse",), snap=True, snap_mask=FIXED, **BENCH)])
def test_no_hints(kw):
    p = plan(**kw)
    assert p["rc"] == 0
    assert p["dense"] == list(range(28)) and p["gsz"] == [4] * 6 + [2, 2]
    assert p["np"] == 0 and p["pb"] == [0] and p["fuse_nb"] == 0 and p["pack_bytes"] == 0
    assert [p[k] for k in ("hint", "nw8", "nw32", "clk", "fixm", "virt", "snap_now", "lat")] == [0] * 8
    assert p["hin"] == p["hnv"] == p["nar"] == []


@pytest.mark.parametrize("lat", [False, True])
def test_benchmark_classes_with_snapshot(lat):
    p = plan(lat=lat, snap=True, snap_mask=FIXED, **BENCH)
    assert p["rc"] == 0
    assert p["hint"] == SPARSE and p["nw8"] == NW8 and p["clk"] == 1 and p["nw32"] == 0  # the clock left nw32
    assert p["fixm"] == FIXED and p["snap_now"] == 0 and p["virt"] == SPARSE
    assert p["nar"] == [] and p["np"] == 0 and p["lat"] == 0  # every narrow column is fixed
    assert p["hin"] == list(range(23, 28)) and p["hnv"] == []
    assert p["fuse_nb"] == 3
    assert p["dense"] == list(range(12, 23)) and p["gsz"] == [4, 4, 2, 1]  # eleven columns: no 2 + 2 tail


@pytest.mark.parametrize("lat", [False, True])
def test_benchmark_classes_without_snapshot(lat):
    n = (1 << 10) + 5  # width * n is no multiple of 16 for either width
    p = plan(n=n, lat=lat, **BENCH)
    assert p["rc"] == 0 and p["snap_now"] == 1 and p["fixm"] == 0 and p["fuse_nb"] == 0 and p["clk"] == 1
    assert p["nar"] == [1, 2, 3, 4, 5, 6, 11] and p["width"] == [1] * 7
    assert part_sizes(p) == ([1, 2, 2, 2] if lat else [4, 3]) == parts(7, lat) and p["lat"] == int(lat)
    step = (n + 15) // 16 * 16
    assert step != n and p["off"] == [i * step for i in range(7)] and p["pack_bytes"] == 7 * step
    assert p["dense"] == [7, 8, 9, 10] + list(range(12, 23)) and p["gsz"] == groups(15) == [4, 4, 4, 2, 1]
    # 32-bit columns: 4 bytes per row
    q = plan(n=n, lat=lat, sparse=SPARSE, nw8=mask([3]), nw32=mask([0, 3, 9, 23]), off=("clock",))
    assert q["nw8"] == mask([3]) and q["nw32"] == mask([0, 9]) and q["nar"] == [0, 3, 9] and q["width"] == [4, 1, 4]
    s4, s1 = (4 * n + 15) // 16 * 16, step
    assert s4 != 4 * n and q["off"] == [0, s4, s4 + s1] and q["pack_bytes"] == 2 * s4 + s1
    assert part_sizes(q) == ([1, 2] if lat else [2, 1])
    assert part_sizes(plan(lat=lat, nw8=mask([5]))) == [1]  # one narrow column: one part on either schedule


def test_each_switch_off():
    base = dict(snap=True, snap_mask=FIXED, **BENCH)
    full = plan(**base)
    p = plan(off=("narrow",), **base)  # no narrow class, so no clock either (it is learned as a 32-bit column)
    assert p["nw8"] == p["nw32"] == p["clk"] == 0 and p["fixm"] == FIXED and p["fuse_nb"] == 0
    assert p["dense"] == [0] + list(range(12, 23))
    p = plan(off=("clock",), **base)  # column 0 stays a 32-bit narrow column; block 0 is not all formed
    assert p["clk"] == 0 and p["nw32"] == 1 and p["nar"] == [0] and p["fuse_nb"] == 0 and p["fixm"] == FIXED
    p = plan(off=("fixed",), **base)
    assert p["fixm"] == 0 and p["snap_now"] == 0 and p["fuse_nb"] == 0 and p["nar"] == [1, 2, 3, 4, 5, 6, 11]
    p = plan(off=("fixed_fuse",), **base)
    assert p["fuse_nb"] == 0 and {k: v for k, v in p.items() if k != "fuse_nb"} == \
        {k: v for k, v in full.items() if k != "fuse_nb"}
    for p in (plan(off=("virtual",), **base), plan(no_virtual=True, **base)):  # virt cleared, nothing else shortened
        assert p["virt"] == 0 and p["hnv"] == p["hin"] == list(range(23, 28))
        assert {k: v for k, v in p.items() if k not in ("virt", "hnv")} == \
            {k: v for k, v in full.items() if k not in ("virt", "hnv")}
    p = plan(clk_off=True, **base)
    assert p["clk"] == 0 and p["nw32"] == 1 and p["nar"] == [0] and p["fuse_nb"] == 0
    p = plan(fixed_off=True, **base)
    assert p["fixm"] == 0 and p["snap_now"] == 0 and p["clk"] == 1 and p["nar"] == [1, 2, 3, 4, 5, 6, 11]
    p = plan(fixed_off=True, **BENCH)
    assert p["snap_now"] == 0


def test_masks_exclude_each_other():
    # a sparse column is in no other class, not even with a snapshot holding it; only sparse columns >= 22 are virtual
    p = plan(sparse=mask([2, 21, 22]), nw8=mask([2, 4]), nw32=mask([4, 21, 0]), snap=True, snap_mask=mask([1, 2, 3]))
    assert p["hint"] == mask([2, 21, 22]) and p["nw8"] == mask([4]) and p["nw32"] == 0 and p["clk"] == 1
    assert p["fixm"] == mask([1, 3]) and p["virt"] == mask([22])
    assert p["hin"] == [2, 21, 22] and p["hnv"] == [2, 21] and p["nar"] == [4]
    assert p["dense"] == [c for c in range(28) if c not in (0, 1, 2, 3, 4, 21, 22)]
    assert p["fuse_nb"] == 1  # block 0: clock, fixed, sparse (written), fixed; block 1 has dense columns


def test_fused_prefix_edges():
    # one non-fixed column in block 1 stops the prefix there
    p = plan(snap=True, snap_mask=FIXED & ~mask([6]), **BENCH)
    assert p["fuse_nb"] == 1 and p["nar"] == [6]
    # the clock not derived: column 0 is not formed, no prefix
    assert plan(snap=True, snap_mask=FIXED, sparse=SPARSE, nw8=NW8, nw32=0)["fuse_nb"] == 0
    # a sparse column inside the prefix counts when its LDE is written ...
    p = plan(snap=True, snap_mask=FIXED, sparse=mask([5]), nw8=NW8, nw32=1)
    assert p["fixm"] == FIXED & ~mask([5]) and p["fuse_nb"] == 3
    # ... and every block can be in it: 12 .. 27 sparse, written (ZK_VIRTUAL=0)
    p = plan(snap=True, snap_mask=FIXED, sparse=mask(range(12, 28)), nw32=1, off=("virtual",))
    assert p["fuse_nb"] == 7 and p["dense"] == [] and p["gsz"] == []
    # ... but a virtual column is never formed: the prefix ends before its block
    p = plan(snap=True, snap_mask=FIXED, sparse=mask(range(12, 28)), nw32=1)
    assert p["virt"] == mask(range(22, 28)) and p["fuse_nb"] == 5


def test_group_limit_cannot_be_exceeded():
    """No class mix within W = 28 exceeds ZK_UPLOAD_GROUPS_MAX = 14: the throughput schedule's worst is one narrow
    column beside 27 dense ones (8 groups, 1 part, the fallback item: 10), the latency schedule's 8 groups + 1 = 9.  So
    no input reaches the error status; every (nd, nn) split is tried and says so."""
    worst = 0
    for nn, lat in itertools.product(range(0, 29), (False, True)):
        for nd in range(0, 29 - nn):
            np_ = len(parts(nn, lat))
            worst = max(worst, len(groups(nd)) + (1 if lat and nn else np_ + 1))
            p = plan(lat=lat, nw8=mask(range(nn)), sparse=mask(range(nn + nd, 28)), off=("clock",))
            assert p["rc"] == 0 and p["gsz"] == groups(nd) and part_sizes(p) == parts(nn, lat)
    assert worst == 10 < GROUPS_MAX
