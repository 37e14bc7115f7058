"""A plain reference of the Merkle tree the prover commits with (csrc/kernels.hip merkle_tree): the BLAKE3 two-to-one
merge over numpy uint32 arrays, one array operation per step of the compression for all the nodes of a level at once, and
the whole heap built from it.  Written from the BLAKE3 specification (section 2.2, the compression function); it shares
no code with the device's b3::merge or the oracle's C.  tests/test_merkle_ref_cpu.py pins it against the oracle.  Not a
test module.

The merge of two digests is one compression of the 64-byte block left || right: chaining value IV, counter 0, block
length 64, flags CHUNK_START | CHUNK_END | ROOT (a one-block, one-chunk message is its own root), the first eight
output words.  That is winter-crypto's Blake3_256::merge, blake3::hash of the 64 bytes.

Heap layout, as merkle_tree documents it: over nl leaves (a power of two) the heap has nl slots of one digest each,
slot 1 the root, the children of node i at 2 i and 2 i + 1, the level of cnt nodes at [cnt, 2 cnt); the level of nl / 2
nodes merges the leaf pairs, and slot 0 is not a node.
"""
import numpy as np

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
MSG_PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, ROOT = 1, 2, 8
# the columns, then the diagonals, of the 4 x 4 state: (a, b, c, d) of each G
ROUND_GS = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
            (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def as_words(digests):
    """digests as a (count, 8) array of little-endian uint32 words; bytes or an array of either form"""
    if isinstance(digests, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(digests), dtype="<u4").reshape(-1, 8).astype(np.uint32)
    a = np.asarray(digests)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a).reshape(-1).view("<u4").reshape(-1, 8).astype(np.uint32)
    return a.astype(np.uint32, copy=False).reshape(-1, 8)


def as_bytes(words):
    """(count, 8) uint32 words as the digests' bytes"""
    return np.ascontiguousarray(words, dtype="<u4").tobytes()


def merge(blocks):
    """blocks: (m, 16) uint32, row j the words of left_j || right_j.  Returns the (m, 8) words of the parents."""
    blocks = np.asarray(blocks, dtype=np.uint32)
    count = blocks.shape[0]
    m = [np.ascontiguousarray(blocks[:, i]) for i in range(16)]
    const = lambda value: np.full(count, value, dtype=np.uint32)
    # h = IV (no key), then IV[0..4], the counter's two halves (0), the block length, the flags
    v = [const(w) for w in IV] + [const(w) for w in IV[:4]] + [const(0), const(0), const(64),
                                                               const(CHUNK_START | CHUNK_END | ROOT)]
    for rnd in range(7):
        for g, (a, b, c, d) in enumerate(ROUND_GS):
            v[a] = v[a] + v[b] + m[2 * g]
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 12)
            v[a] = v[a] + v[b] + m[2 * g + 1]
            v[d] = _rotr(v[d] ^ v[a], 8)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 7)
        if rnd < 6:
            m = [m[MSG_PERMUTATION[i]] for i in range(16)]
    return np.stack([v[i] ^ v[i + 8] for i in range(8)], axis=1)


def heap(leaves):
    """Every level of the tree over `leaves` (bytes, or (nl, 8) words; nl a power of two >= 2) as one (nl, 8) uint32 array
    in the heap layout above; slot 0 is left zero."""
    level = as_words(leaves)
    nl = level.shape[0]
    if nl < 2 or nl & (nl - 1):
        raise ValueError("the number of leaves must be a power of two, at least 2")
    nodes = np.zeros((nl, 8), dtype=np.uint32)
    cnt = nl
    while cnt > 1:
        cnt //= 2
        level = merge(level.reshape(cnt, 16))
        nodes[cnt:2 * cnt] = level
    return nodes


def root(leaves):
    return as_bytes(heap(leaves)[1])


def level_of(index):
    """the number of nodes cnt of the level heap slot `index` (>= 1) lies in: cnt <= index < 2 cnt"""
    return 1 << (int(index).bit_length() - 1)
