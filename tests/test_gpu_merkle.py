"""The Merkle tree builder (csrc/kernels.hip merkle_tree: k_merge_level3_pf, k_merge_block and the launcher that chains
them), called directly through zk_diag_merkle and compared node by node with tests/merkle_ref.py, whose merge
tests/test_merkle_ref_cpu.py pins to the oracle.

Why every node and not the root: most stored nodes never feed the root.  The three-level kernel computes a group's two
upper levels from registers and k_merge_block every level above its first from LDS, so a node stored to the wrong slot,
not stored, or stored from a stale prefetch leaves the root as it should be; only an opening whose path crosses the node
sees it.  Here every comparison is exact, heap slot by heap slot, and a mismatch names the first differing heap index
and its level.

The sizes of the default configuration (17, 2048, 512: merkle_tree's own) are the smallest that reach each path of the
launcher.  The forced configurations move its three constants (merkle_tree_cfg) so that trees of 8 to 2^13 leaves reach
what only 2^18 to 2^23 leaves reach by default: the three-level kernel, launches of it chained to each other and to
nothing, several grid-stride rounds per thread, a grid in which only some threads make a second round (the tn < q
prefetch boundary), a partial last block and a partial wave; and many chained passes of small blocks.

Leaves are distinct by construction (word 0 of leaf i is i, the rest random from a fixed seed): identical leaves would
give identical nodes across a level and hide a misplaced one.  Every case also asserts that slot 0 of the heap, the
4 KiB guard on each side of it and the leaf buffer are as they were before the launches.
"""
import ctypes as C
import random

import numpy as np
import pytest

import back_half_ref
import merkle_ref as ref
from test_gpu_back_half import draw_fn, run_fri_layer
from zkvm_amd import native

pytestmark = pytest.mark.gpu

DEFAULT = (17, 2048, 512)  # ZK_MERKLE_L3_MIN, MERKLE_PF_BLOCKS, k_merge_block's block size
GUARD = 4096
FILL = 0xA5


# ---------------------------------------------------------------- leaves and their reference heaps, made once
_trees = {}


def tree(nl, kind="random"):
    """(leaf bytes, reference heap as (nl, 32) uint8) of the nl-leaf tree of `kind`; never modified"""
    if (nl, kind) not in _trees:
        if kind == "random":
            words = np.random.default_rng(0x3E7 + nl).integers(0, 1 << 32, size=(nl, 8), dtype=np.uint32)
            words[:, 0] = np.arange(nl, dtype=np.uint32)  # distinct whatever the draw
        else:
            words = np.full((nl, 8), {"zero": 0, "ones": 0xFFFFFFFF}[kind], dtype=np.uint32)
        heap = np.frombuffer(ref.as_bytes(ref.heap(words)), dtype=np.uint8).reshape(nl, 32)
        heap.flags.writeable = False
        _trees[(nl, kind)] = (ref.as_bytes(words), heap)
    return _trees[(nl, kind)]


# ---------------------------------------------------------------- the entry point
def run_merkle(leaves, cfg=DEFAULT, positions=None, cap=1 << 17):
    """zk_diag_merkle: (heap (nl, 32) uint8, guards bytes, leaf buffer bytes, proof bytes or None)"""
    assert native.device_count() > 0, "no GPU visible"
    nl = len(leaves) // 32
    nodes = np.empty((nl, 32), dtype=np.uint8)
    guard, back = C.create_string_buffer(2 * GUARD), C.create_string_buffer(32 * nl)
    pos, k, proof, plen = None, 0, None, C.c_size_t(0)
    if positions is not None:
        pos, k, proof, plen = (C.c_uint64 * len(positions))(*positions), len(positions), C.create_string_buffer(cap), C.c_size_t(cap)
    native.check(native.lib().zk_diag_merkle(0, leaves, nl, cfg[0], cfg[1], cfg[2], nodes.ctypes.data, guard, back, pos, k,
                                             proof, C.byref(plen)), "zk_diag_merkle")
    return nodes, guard.raw, back.raw, proof.raw[:plen.value] if positions is not None else None


def assert_heap(got, want, what):
    """every node of the heap, exactly.  A wrong node makes its ancestors wrong when they are computed from the stored
    copy, so the report names the first differing heap index and also the widest level with a wrong node, where the
    fault began."""
    nl = len(want)
    diff = np.flatnonzero((got[1:] != want[1:]).any(axis=1)) + 1
    if not diff.size:
        return
    first = int(diff[0])
    levels = sorted({ref.level_of(int(i)) for i in diff})
    widest = levels[-1]
    origin = int(diff[diff >= widest][0])
    unwritten = int((got[diff] == FILL).all(axis=1).sum())
    raise AssertionError(
        f"{what}: {diff.size} of {nl - 1} nodes differ, the first at heap index {first}, node {first - ref.level_of(first)} "
        f"of the level of {ref.level_of(first)} nodes; levels with a wrong node: {levels}; in the widest of them the "
        f"first is heap index {origin}, node {origin - widest} of {widest}; {unwritten} of the wrong nodes still hold "
        f"the {FILL:#x} fill (never stored)")


def check_tree(nl, cfg=DEFAULT, kind="random"):
    leaves, want = tree(nl, kind)
    got, guard, back, _ = run_merkle(leaves, cfg)
    assert_heap(got, want, f"nl={nl} cfg={cfg} {kind}")
    assert got[0].tobytes() == bytes([FILL]) * 32, "slot 0 of the heap was written"
    assert guard[:GUARD] == bytes([FILL]) * GUARD, "a store below the heap"
    assert guard[GUARD:] == bytes([FILL]) * GUARD, "a store above the heap"
    assert back == leaves, "the leaf buffer was written"


# ---------------------------------------------------------------- the default configuration
# 2: P = 1, the level loop of k_merge_block not entered; 4, 8: the smallest block trees; 2^9: cnt = 256 < 512;
# 2^10: P = 512, one block; 2^11: two blocks, then a P = 1 launch; 2^12: four blocks, then P = 2; 2^17: the largest
# block-only tree, 128 blocks then P = 64; 2^18: the smallest three-level launch, then 32 blocks, then P = 16;
# 2^21: two three-level launches chained, then blocks
@pytest.mark.parametrize("log_nl", [1, 2, 3, 9, 10, 11, 12, 17, 18, 21])
def test_default_configuration(log_nl):
    check_tree(1 << log_nl)


@pytest.mark.parametrize("kind", ["zero", "ones"])
def test_constant_leaves(kind):
    """all-zero and all-0xFF digests, at one small size"""
    check_tree(1 << 10, kind=kind)


# ---------------------------------------------------------------- forced configurations: (nl, l3_min_log, pf_blocks, block_p)
FORCED = [
    # the three-level kernel at its smallest: q = 1 and the launch writes the root itself; then cnt = 1 (a one-thread
    # block); then cnt = 2; two three-level launches with nothing after
    (8, 2, 2048, 512), (16, 2, 2048, 512), (32, 2, 2048, 512), (64, 2, 2048, 512),
    # q = 1024 groups in the first launch: one block (four rounds per thread); three blocks (stride 768: threads 0 .. 255
    # make two rounds, the rest one, so tn < q differs inside the launch); a cap of eight blocks, above what any launch
    # asks for: one round, and from the second launch (q = 128) more threads than groups, a partial last block
    (1 << 13, 2, 1, 512), (1 << 13, 2, 3, 512), (1 << 13, 2, 8, 512),
    # q = 32 in a block of 256: one partial wave
    (1 << 8, 2, 1, 512),
    # small blocks: 256 roots and nine chained passes; 8 roots and two passes
    (1 << 10, 17, 2048, 2), (1 << 10, 17, 2048, 64),
    # one thread per block: every level a launch of its own
    (1 << 6, 17, 2048, 1),
    # the wide kernel handing over to chained small blocks
    (1 << 12, 8, 2, 4),
]


@pytest.mark.parametrize("case", FORCED, ids=lambda c: "nl%d-l3min%d-pf%d-p%d" % c)
def test_forced_configuration(case):
    nl, l3_min_log, pf_blocks, block_p = case
    check_tree(nl, (l3_min_log, pf_blocks, block_p))


# ---------------------------------------------------------------- openings
def opening_sets(nl, rnd, groups):
    """position sets over nl leaves; groups: leaf ranges (first leaf, count) a set must cross"""
    edge = sorted({0, nl - 1} | {first for first, _ in groups} | {first + count - 1 for first, count in groups})
    k = rnd.randrange(1, nl // 2 - 1)
    sets = [[p] for p in edge] + [edge, [2 * k, 2 * k + 1], [2 * k + 1, 2 * k + 2], sorted(rnd.sample(range(nl), 255)),
                                  list(range(255))]
    return sets


# (nl, cfg, the leaves of the groups to cross).  2^18, default: every launch's first and last group start at leaf 0
# and end at leaf nl - 1 (group t of the first launch: leaves 8 t .. 8 t + 7; block b of the second: 8192 b ..).
# 2^13, (2, 3, 512): the first launch has q = 1024 groups of 8 leaves on 768 threads: group 767 the last of the first
# round, group 768 the first of the second, groups 255 / 256 the two sides of the tn < q boundary; the second launch
# (q = 128 groups of 64 leaves, one block) and the later ones run a single round.
OPENING_TREES = [
    (1 << 18, DEFAULT, []),
    (1 << 13, (2, 3, 512), [(8 * 767, 8), (8 * 768, 8), (8 * 255, 8), (8 * 256, 8), (64 * 127, 64)]),
]


@pytest.mark.parametrize("case", OPENING_TREES, ids=lambda c: "nl%d-l3min%d-pf%d-p%d" % ((c[0],) + c[1]))
def test_openings_rebuild_the_reference_root(oracle, case):
    """plan_batch and the digest reads at depth 13 and 18, as zk_lde_query runs them: the opened leaves and the proof
    bytes rebuild the reference's root (back_half_ref.batch_root), and the heap that served them is the reference's"""
    nl, cfg, groups = case
    leaves, want = tree(nl)
    depth = nl.bit_length() - 1
    rnd = random.Random(nl)
    for positions in opening_sets(nl, rnd, groups):
        got, _, _, proof = run_merkle(leaves, cfg, positions)
        assert_heap(got, want, f"nl={nl} cfg={cfg} opening {positions[:4]}")
        opened = [leaves[32 * p:32 * p + 32] for p in positions]
        assert back_half_ref.batch_root(oracle.blake3, opened, list(positions), proof, depth) == want[1].tobytes(), positions
    # sizes: a sibling pair needs no leaf digest and one path; one leaf the whole path
    _, _, _, pair = run_merkle(leaves, cfg, [6, 7])
    assert len(pair) == 2 + 32 * (depth - 1)
    _, _, _, one = run_merkle(leaves, cfg, [5])
    assert len(one) == 2 + 32 * depth
    # unsorted positions: the proof of the sorted set
    s = sorted(rnd.sample(range(nl), 40))
    shuffled = list(s)
    rnd.shuffle(shuffled)
    assert run_merkle(leaves, cfg, shuffled)[3] == run_merkle(leaves, cfg, s)[3]


def test_opening_proof_buffer_too_small():
    leaves, _ = tree(1 << 10)
    nl = 1 << 10
    nodes, guard, back = np.empty((nl, 32), dtype=np.uint8), C.create_string_buffer(2 * GUARD), C.create_string_buffer(32 * nl)
    pos, plen, proof = (C.c_uint64 * 1)(5), C.c_size_t(100), C.create_string_buffer(100)
    rc = native.lib().zk_diag_merkle(0, leaves, nl, *DEFAULT, nodes.ctypes.data, guard, back, pos, 1, proof, C.byref(plen))
    assert rc == native.ZK_ERR_BUFFER_TOO_SMALL and plen.value == 2 + 32 * 10


# ---------------------------------------------------------------- a FRI layer of one row
@pytest.mark.parametrize("ext", [1, 2])
def test_fri_layer_of_one_row_has_the_zero_root(ext):
    """fold 16 at blowup 8 with a remainder of one coefficient ends in a layer of L = 16 values, one row (trace lengths
    32, 512, 8192, ...).  merkle_tree launches nothing for one leaf, so commit_fri_layer sets the root: the zero digest
    the oracle's zeroed heap gives, not what the digest buffer held (zk_diag_fri_layer fills it with 0xA5 first).  The
    fold of the one row is the reference's."""
    rnd = random.Random(9100 + ext)
    draw = draw_fn(rnd, ext)
    layer = [draw() for _ in range(16)]
    alpha = draw()
    root, nxt = run_fri_layer(layer, ext, 16, 0, 8, alpha)
    assert root == bytes(32)
    assert nxt == back_half_ref.fri_fold(layer, 16, alpha, ext)
