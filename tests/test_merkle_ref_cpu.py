"""tests/merkle_ref.py against the CPU oracle (no GPU): the heap the GPU tree builder is compared with, node by node,
must not be wrong the way a kernel could be.  Also here, because they need no device: the arguments zk_diag_merkle
refuses before it touches one.
"""
import ctypes as C

import numpy as np
import pytest

import merkle_ref as ref
from zkvm_amd import native


def random_leaves(nl, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(nl, 8), dtype=np.uint32)


def test_merge_is_blake3_of_the_64_bytes(oracle):
    """every first-level node of a sample: the oracle's BLAKE3 over left || right; and the extreme blocks"""
    leaves = random_leaves(512, 1)
    data = ref.as_bytes(leaves)
    parents = ref.merge(leaves.reshape(256, 16))
    assert parents.shape == (256, 8) and parents.dtype == np.uint32
    for j in range(256):
        assert ref.as_bytes(parents[j]) == oracle.blake3(data[64 * j:64 * j + 64]), j
    for fill in (0x00, 0xFF, 0xA5):
        block = bytes([fill]) * 64
        assert ref.as_bytes(ref.merge(ref.as_words(block).reshape(1, 16))[0]) == oracle.blake3(block), fill


@pytest.mark.parametrize("nl", [2, 4, 1 << 10, 1 << 18])
def test_root_is_the_oracles(oracle, nl):
    leaves = random_leaves(nl, 100 + nl)
    nodes = ref.heap(leaves)
    assert nodes.shape == (nl, 8) and not nodes[0].any()
    assert ref.as_bytes(nodes[1]) == oracle.merkle_root(ref.as_bytes(leaves))
    assert ref.root(ref.as_bytes(leaves)) == ref.as_bytes(nodes[1])  # (bytes in, the same tree)


def test_heap_layout(oracle):
    """node i is the merge of nodes 2 i and 2 i + 1, the level of nl / 2 nodes that of the leaf pairs: every node of a
    64-leaf heap against the oracle's BLAKE3 of its children"""
    nl = 64
    leaves = random_leaves(nl, 7)
    nodes = ref.heap(leaves)
    slots = np.concatenate([nodes, leaves])  # children of i at 2 i and 2 i + 1 throughout: the leaves are slots nl ..
    for i in range(1, nl):
        assert ref.as_bytes(nodes[i]) == oracle.blake3(ref.as_bytes(slots[2 * i:2 * i + 2])), i
    assert [ref.level_of(i) for i in (1, 2, 3, 4, 7, 8, 63)] == [1, 2, 2, 4, 4, 8, 32]


def test_heap_refuses_what_is_not_a_tree():
    for nl in (0, 1, 3, 6, 12):
        with pytest.raises(ValueError):
            ref.heap(np.zeros((nl, 8), dtype=np.uint32))


def test_as_words_round_trip():
    leaves = random_leaves(16, 9)
    data = ref.as_bytes(leaves)
    assert np.array_equal(ref.as_words(data), leaves)
    assert np.array_equal(ref.as_words(np.frombuffer(data, dtype=np.uint8)), leaves)
    assert ref.as_words(bytes(range(32)))[0, 0] == 0x03020100  # little-endian words


def test_diag_merkle_refuses_bad_arguments():
    """every refusal comes before the first device call, so it needs no GPU"""
    F = native.lib().zk_diag_merkle
    nl = 16
    leaves = bytes(32 * nl)
    nodes, guard, back = (C.create_string_buffer(32 * nl), C.create_string_buffer(8192), C.create_string_buffer(32 * nl))
    plen = C.c_size_t(4096)
    proof = C.create_string_buffer(4096)
    pos = (C.c_uint64 * 2)(3, 9)
    good = dict(leaves=leaves, nl=nl, l3=17, pf=2048, bp=512, nodes=nodes, guard=guard, back=back, pos=None, k=0)
    bad = [dict(nl=0), dict(nl=1), dict(nl=3), dict(nl=24), dict(nl=1 << 25), dict(leaves=None), dict(nodes=None),
           dict(guard=None), dict(back=None), dict(l3=1), dict(l3=0), dict(l3=-1), dict(l3=63), dict(pf=0),
           dict(pf=(1 << 20) + 1), dict(bp=0), dict(bp=3), dict(bp=48), dict(bp=1024),
           dict(pos=pos, k=0), dict(pos=pos, k=256), dict(pos=(C.c_uint64 * 2)(3, 16), k=2),
           dict(pos=(C.c_uint64 * 2)(5, 5), k=2)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = F(0, a["leaves"], a["nl"], a["l3"], a["pf"], a["bp"], a["nodes"], a["guard"], a["back"], a["pos"], a["k"],
               proof, C.byref(plen))
        assert rc == native.ZK_ERR_INVALID_ARG and native.lib().zk_last_error(), kw
    assert F(0, leaves, nl, 17, 2048, 512, nodes, guard, back, pos, 2, proof, None) == native.ZK_ERR_INVALID_ARG
