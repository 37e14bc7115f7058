"""The two decisions of the coset-sharded prover that need no device (csrc/shard_plan.hpp through zk_diag_shard_rounds
and zk_diag_shard_locate).  Runs without a GPU.  The properties are stated here from what the protocol needs, not from
the planner's formulas:

Rounds.  Of the columns U (ascending) the first `rep` are replicated; the others are split round robin over G ranks.
  - every split column appears exactly once, the i-th of them in round i div G at rank i mod G;
  - a round is gathered in place iff its columns are consecutive and the G columns from its first one fit under 32
    (the coefficient buffer holds 8 ceil(28 / 8) columns); an in-place round's rank g lands on column first + g;
  - the padding chunks of an in-place short round land on columns >= 28 or not in U (formed after the rounds), and never
    on a replicated column.

Locate.  A tree of M leaves (leaf 8q + r: row q of coset r) over G ranks of Bl = 8 / G cosets each, heap node idx at
level L covering leaves [i 2^L, (i + 1) 2^L), i = idx - M / 2^L:
  - levels 0 .. Lb = log2 Bl are on the rank that owns all the leaves below the node (leaf 8q + r: rank r div Bl), in its
    block buffer;
  - above them rank d holds the subtree over the level-Lb nodes [d Q, (d + 1) Q), Q = M / 8, as a heap (children of k
    at 2k, 2k + 1); heap nodes below G are the host's;
  - within one rank and buffer the offsets are distinct, 32-byte aligned and inside the buffer.
"""
from __future__ import annotations

import ctypes as C
import random

import pytest

from zkvm_amd import native

W = 28


def rounds(U, G, rep):
    arr = (C.c_int32 * max(len(U), 1))(*U)
    out = (C.c_int32 * (W * (3 + 2 * G)))()
    nr = C.c_int32(-1)
    native.check(native.lib().zk_diag_shard_rounds(arr, len(U), G, rep, out, len(out), C.byref(nr)), "rounds")
    k = 3 + 2 * G
    return [{"i0": out[k * r], "real": out[k * r + 1], "inplace": bool(out[k * r + 2]),
             "cols": list(out[k * r + 3:k * r + 3 + G]), "land": list(out[k * r + 3 + G:k * r + 3 + 2 * G])}
            for r in range(nr.value)]


def column_sets():
    yield list(range(W))
    for md in range(1, 17):
        yield list(range(12, 12 + md))
    for c in range(W):
        yield [x for x in range(W) if x != c]
    rng = random.Random(20240607)
    for _ in range(2000):
        yield sorted(rng.sample(range(W), rng.randint(0, W)))


@pytest.mark.parametrize("G", [2, 4, 8])
def test_round_plan(G):
    for U in column_sets():
        for rep in sorted({min(r, len(U)) for r in (0, 3, 4, len(U))}):
            split, replicated = U[rep:], set(U[:rep])
            plan = rounds(U, G, rep)
            assert len(plan) == -(-len(split) // G), (U, rep)
            seen = []
            for k, r in enumerate(plan):
                mine = split[G * k:G * k + G]
                assert r["i0"] == G * k and r["real"] == len(mine) >= 1
                assert r["cols"] == mine + [-1] * (G - len(mine)), (U, rep, k)  # the i-th split column: rank i mod G
                seen += [c for c in r["cols"] if c >= 0]
                consecutive = all(b == a + 1 for a, b in zip(mine, mine[1:]))
                assert r["inplace"] == (consecutive and mine[0] + G <= 32), (U, rep, k)
                if not r["inplace"]:
                    assert r["land"] == [-1] * G
                    continue
                assert r["land"] == [mine[0] + g for g in range(G)]
                for pad in r["land"][len(mine):]:
                    assert pad >= W or pad not in U, f"padding lands on interpolated column {pad}: U={U} rep={rep} G={G}"
                    assert pad not in replicated
            assert seen == split, (U, rep)  # each exactly once, in order


def locate(M, G, is_node, idx):
    arr = (C.c_uint64 * len(idx))(*idx)
    out = (C.c_int64 * (3 * len(idx)))()
    native.check(native.lib().zk_diag_shard_locate(M, G, is_node, arr, len(idx), out), "locate")
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(len(idx))]


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("M", [64, 256, 1024])
def test_tree_locate(M, G):
    Bl = 8 // G
    Lb, Q = Bl.bit_length() - 1, M // 8
    leaf_owner = lambda x: (x % 8) // Bl  # noqa: E731
    where = {}  # (level, index in level) -> (owner, buffer, offset)
    for x, loc in enumerate(locate(M, G, 0, list(range(M)))):
        where[(0, x)] = loc
    nodes = list(range(1, M))
    for idx, loc in zip(nodes, locate(M, G, 1, nodes)):
        L = next(lv for lv in range(1, 32) if (M >> lv) <= idx < (M >> (lv - 1)))  # level lv: heap [M / 2^lv, 2 M / 2^lv)
        where[(L, idx - (M >> L))] = loc
    assert len(where) == 2 * M - 1
    used = {}
    for (L, i), (owner, buf, off) in where.items():
        heap_idx = (M >> L) + i
        assert (owner == -1) == (L > 0 and heap_idx < G), (L, i)
        if owner < 0:
            continue
        if L <= Lb:  # a block level: on the owner of every leaf below
            owners = {leaf_owner(x) for x in range(i << L, (i + 1) << L)}
            assert owners == {owner} and buf == 2, (L, i)
            assert off < 32 * (2 * Bl - 1) * Q
        else:  # a subtree node: the rank whose range of level-Lb nodes holds the first one below it
            assert owner == (i << (L - Lb)) // Q and buf == 1, (L, i)
            assert off < 32 * Q
            if L > Lb + 1:  # a heap: the children of node k at 2k and 2k + 1
                for side in (0, 1):
                    assert where[(L - 1, 2 * i + side)] == (owner, 1, 2 * off + 32 * side), (L, i)
        assert off % 32 == 0
        assert used.setdefault((owner, buf, off), (L, i)) == (L, i), "two nodes at one offset"
