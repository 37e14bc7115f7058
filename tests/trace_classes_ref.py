"""Reference for the front of the trace commitment: the column classes and what consumes them, in plain Python integers
and numpy (tests/test_gpu_trace_classes.py, tests/test_host_rows_cpu.py; the entry points are zk_diag_detect,
zk_diag_trace_commit, zk_diag_column_fills, zk_diag_expand_narrow, zk_diag_host_rows and zk_diag_row_tasks).

A column is n field elements, here an (n, 2) uint64 array (lo, hi: the 16-byte little-endian encoding) or a list of
ints.  Its classes are decided by rows 0 .. n-2 alone (the last row of a trace is random):

    nonzero    some row before the last is not 0            (clear: the column is sparse)
    w8         some row before the last is >= 2^8           (clear: the column packs into 1 byte per row)
    w32        some row before the last is >= 2^32          (clear: into 4 bytes per row)
    not_clock  some row i before the last does not hold i   (clear: the column is the AIR clock)

Coefficients and coset LDE come from the oracle's radix-2 transforms, called as test_coset_lde calls them; the trace
root from the pieces of back_half_ref.composition_root (row digest, Merkle root over the natural-order LDE rows).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

P = 2**128 - 45 * 2**40 + 1
W = 28          # trace width: the flag array is 4 W entries
M64 = 2**64 - 1
OFFSET = 3      # the LDE domain's coset offset


# ---------------------------------------------------------------- columns
def ints(col):
    """an (n, 2) uint64 column as Python ints"""
    return [int(lo) | (int(hi) << 64) for lo, hi in np.asarray(col, dtype=np.uint64).reshape(-1, 2)]


def column(values):
    """ints -> (n, 2) uint64"""
    a = np.empty((len(values), 2), dtype=np.uint64)
    a[:, 0] = [v & M64 for v in values]
    a[:, 1] = [v >> 64 for v in values]
    return a


def put(col, row, value):
    col[row, 0] = value & M64
    col[row, 1] = value >> 64


# ---------------------------------------------------------------- the classes
def flags_of(values):
    """the four flags of a column given as ints, straight from their definitions"""
    body = values[:-1]
    return {"nonzero": int(any(v != 0 for v in body)), "w8": int(any(v >= 2**8 for v in body)),
            "w32": int(any(v >= 2**32 for v in body)), "not_clock": int(any(v != i for i, v in enumerate(body)))}


def flags_of_column(col):
    """flags_of on an (n, 2) uint64 column without the detour through Python ints: lo + 2^64 hi >= 2^k (k <= 64) iff
    hi != 0 or lo >= 2^k (tests/test_host_rows_cpu.py holds the two against each other)"""
    lo, hi = col[:-1, 0], col[:-1, 1]
    high = bool(hi.any())
    rows = np.arange(len(lo), dtype=np.uint64)
    return {"nonzero": int(high or bool(lo.any())), "w8": int(high or bool((lo >= 2**8).any())),
            "w32": int(high or bool((lo >= 2**32).any())), "not_clock": int(high or bool((lo != rows).any()))}


def flag_array(cols, c0, clock_check, widths=True):
    """The flag array after detection of `cols` placed as trace columns c0 .. c0 + len(cols) - 1: [c] nonzero, [W + c]
    w8, [2 W + c] w32, [3 W] trace column 0 is not the clock (when it is among the columns and the check is on);
    every other entry 0.  widths = False: the width flags are not taken (a device-resident trace, which is never
    uploaded, learns no narrow hint: SparseCols::wstride = 0) and stay 0."""
    out = [0] * (4 * W)
    for k, col in enumerate(cols):
        f = flags_of_column(np.asarray(col, dtype=np.uint64))
        c = c0 + k
        out[c] = f["nonzero"]
        if widths:
            out[W + c], out[2 * W + c] = f["w8"], f["w32"]
        if c == 0 and clock_check:
            out[3 * W] = f["not_clock"]
    return out


def last_array(cols, c0):
    """the `last` array: trace column c's last row, 0 for the columns not detected"""
    out = [0] * W
    for k, col in enumerate(cols):
        out[c0 + k] = ints(col[-1:])[0]
    return out


# ---------------------------------------------------------------- packing and expansion
def pack(values, width):
    """rows as `width`-byte little-endian integers (the low bytes of each value), and whether every value fits"""
    mask = (1 << (8 * width)) - 1
    return b"".join((v & mask).to_bytes(width, "little") for v in values), all(v <= mask for v in values)


def expand(packed, width, n, last):
    """a packed column back as n field elements: rows 0 .. n-2 from the packed integers, row n-1 the value `last`
    (whatever the packed buffer holds in that row's slot)"""
    return [int.from_bytes(packed[width * i:width * (i + 1)], "little") for i in range(n - 1)] + [last]


def packed_layout(widths, n):
    """byte offsets of packed columns laid out one after the other, each rounded up to 16 bytes, and the total"""
    offs, total = [], 0
    for w in widths:
        offs.append(total)
        total += (w * n + 15) & ~15
    return offs, total


# ---------------------------------------------------------------- transforms (the oracle's), commitment
def _pool():
    return ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))  # the oracle calls release the GIL


def interpolate(oracle, cols):
    """coefficients of the columns' interpolants over <w_n>: (k, n, 2) uint64"""
    out = np.array(cols, dtype=np.uint64, order="C")  # a copy: or_interp_coset works in place
    n = out.shape[1]
    L, one = oracle.lib(), oracle.to_bytes([1])

    def run(c):
        assert L.or_interp_coset(out[c].ctypes.data, n, one) == 0

    with _pool() as ex:
        list(ex.map(run, range(out.shape[0])))
    return out


def coset_lde(oracle, polys, blowup):
    """out[c, r, q] = P_c(3 w_N^r w_n^q), N = blowup n: the coset-major layout of the prover's LDE"""
    polys = np.ascontiguousarray(polys, dtype=np.uint64)
    k, n = polys.shape[0], polys.shape[1]
    out = np.empty((k, blowup, n, 2), dtype=np.uint64)
    wN = oracle.root_of_unity((blowup * n).bit_length() - 1)
    L = oracle.lib()
    offs = [oracle.to_bytes([OFFSET * pow(wN, r, P) % P]) for r in range(blowup)]

    def run(cr):
        c, r = cr
        assert L.or_eval_coset(polys[c].ctypes.data, n, n, offs[r], out[c, r].ctypes.data) == 0

    with _pool() as ex:
        list(ex.map(run, [(c, r) for c in range(k) for r in range(blowup)]))
    return out


def trace_root(oracle, lde):
    """The root over the LDE rows in natural order: row i = r + blowup q holds every column's value at (coset r,
    position q); each row's digest is BLAKE3 over its elements' 16-byte encodings, the root the oracle's Merkle root."""
    k, B, n, _ = lde.shape
    rows = np.ascontiguousarray(lde.transpose(2, 1, 0, 3))  # [q, r, c, limb]: row i = q B + r, 16 k bytes each
    N, row_bytes = n * B, 16 * k
    leaves = np.empty((N, 32), dtype=np.uint8)
    L = oracle.lib()
    src, dst = rows.ctypes.data, leaves.ctypes.data
    for i in range(N):
        L.or_blake3(src + i * row_bytes, row_bytes, dst + 32 * i)
    return oracle.merkle_root(leaves.tobytes())
