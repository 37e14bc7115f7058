"""winterfell's plug points (Prover::new_trace_lde, new_evaluator, build_constraint_commitment; include/zkvm_gpu.h
"plug point 1 .. 3" and their forms over the challenge field) as two thin wrappers over the library's handles.

Field elements are (…, 2) uint64 arrays, the low and high halves of a canonical f128 value, as everywhere in the
package.  An E value (ext = 2, FieldExtension::Quadratic) is two of them, component a then b, so E arrays end in
(…, 2, 2); with ext = 1 that axis is dropped and the calls are the base-field plug points byte for byte.

    lde, polys = TraceLde.new(gpu, trace, blowup=8, polys=True)   # new_trace_lde -> (TraceLde, TracePolyTable)
    cur, nxt = lde.read_frame(step)                               # TraceLde::read_main_trace_frame_into
    rows, proof = lde.query(positions)                            # TraceLde::query
    matrix = lde.read_rows()                                      # DefaultTraceLde's RowMatrix, (N, 28, 2)
    comp = lde.evaluate(pub, coeff_t, coeff_b, ext=2)             # ConstraintEvaluator::evaluate
    cc, cpolys = ConstraintCommitment.commit(lde, comp, ext=2, num_cols=7, polys=True)
    rows, proof = cc.query(positions)                             # ConstraintCommitment::query
    evaluations = cc.read_rows()                                  # its RowMatrix<E>, (N, num_cols, [2,] 2)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .native import PubInputs, ZkError, check, lib

WIDTH = 28
PROOF_CAP = 1 << 20  # a batch Merkle proof of 255 positions at depth 26 stays below 255 * 26 * 32 + 511 bytes


def _elems(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.shape != shape:
        raise ValueError(f"{what}: expected a uint64 array of shape {shape}, got {a.shape}")
    return a


def _eshape(ext, *lead):
    if ext not in (1, 2):
        raise ZkError(native.ZK_ERR_INVALID_ARG, "ext must be 1 (base field) or 2 (quadratic extension)")
    return (*lead, 2) if ext == 1 else (*lead, 2, 2)


def _query(call, positions, row_shape):
    pos = np.ascontiguousarray(positions, dtype=np.uint64)
    rows = np.empty((len(pos), *row_shape), dtype=np.uint64)
    proof, plen = C.create_string_buffer(PROOF_CAP), C.c_size_t(PROOF_CAP)
    check(call(pos.ctypes.data, len(pos), rows.ctypes.data, proof, C.byref(plen)), "query")
    return rows, proof.raw[:plen.value]


def _read_rows(call, what, N, first, count, out, row_shape):
    count = N if count is None else count
    if out is None:
        out = np.empty((max(count, 0), *row_shape), dtype=np.uint64)
    elif (not isinstance(out, np.ndarray) or out.dtype != np.uint64 or out.shape != (count, *row_shape)
          or not out.flags.c_contiguous or not out.flags.writeable):
        raise ValueError(f"out: expected a writeable C-contiguous uint64 array of shape {(count, *row_shape)}")
    check(call(first, count, out.ctypes.data if out.size else None), what)
    return out


class TraceLde:
    """DefaultTraceLde: the trace's low-degree extension and its row commitment in one prover's device memory."""

    def __init__(self, gpu, handle, n: int, blowup: int, root: bytes):
        self.gpu, self.handle, self.n, self.blowup, self.root = gpu, handle, n, blowup, root

    @classmethod
    def new(cls, gpu, trace: np.ndarray, blowup: int = 8, polys: bool = False):
        """Prover::new_trace_lde of a (28, n, 2) host trace (any strides between columns: one pointer per column goes
        down).  Returns the TraceLde, or with polys=True (TraceLde, trace polynomials (28, n, 2))."""
        trace = np.asarray(trace, dtype=np.uint64)
        if trace.ndim != 3 or trace.shape[0] != WIDTH or trace.shape[2] != 2:
            raise ValueError(f"trace: expected (28, n, 2) uint64, got {trace.shape}")
        if trace.strides[1:] != (16, 8):
            trace = np.ascontiguousarray(trace)
        n = trace.shape[1]
        cols = (C.c_void_p * WIDTH)(*(trace.ctypes.data + c * trace.strides[0] for c in range(WIDTH)))
        h, root = C.c_void_p(), C.create_string_buffer(32)
        table = np.empty((WIDTH, n, 2), dtype=np.uint64) if polys else None
        check(lib().zk_lde_new_columns(gpu.handle, cols, n, blowup, C.byref(h), root,
                                       table.ctypes.data if polys else None), "zk_lde_new_columns")
        lde = cls(gpu, h, n, blowup, root.raw)
        return (lde, table) if polys else lde

    def read_frame(self, lde_step: int):
        """TraceLde::read_main_trace_frame_into: rows lde_step and lde_step + blowup (mod N), (28, 2) each."""
        cur, nxt = np.empty((WIDTH, 2), dtype=np.uint64), np.empty((WIDTH, 2), dtype=np.uint64)
        check(lib().zk_lde_read_frame(self.handle, lde_step, cur.ctypes.data, nxt.ctypes.data), "zk_lde_read_frame")
        return cur, nxt

    def query(self, positions):
        """TraceLde::query: (rows (k, 28, 2), BatchMerkleProof bytes) at k distinct positions."""
        return _query(lambda *a: lib().zk_lde_query(self.handle, *a), positions, (WIDTH, 2))

    def read_rows(self, first: int = 0, count: int | None = None, out: np.ndarray | None = None):
        """A slice of DefaultTraceLde's main segment RowMatrix: rows (first + k) mod N, k < count (all N from `first` on
        when count is None; at most N + blowup, so a window of frames may wrap), (count, 28, 2).  out: the caller's
        array of that shape, for instance one over page-locked memory (zk_host_alloc), which the copies fill at the link
        rate."""
        return _read_rows(lambda *a: lib().zk_lde_read_rows(self.handle, *a), "zk_lde_read_rows", self.n * self.blowup,
                          first, count, out, (WIDTH, 2))

    def evaluate(self, pub: PubInputs, coeff_t, coeff_b, ext: int = 1, keep_on_device: bool = False):
        """ConstraintEvaluator::evaluate: coeff_t (20, [2,] 2) and coeff_b (22, [2,] 2) -> the CompositionPolyTrace,
        (8n, [2,] 2) in natural CE-domain order.  keep_on_device: nothing comes back (None); the values stay on the GPU
        for ConstraintCommitment.commit(lde, None, ...)."""
        ct = _elems(coeff_t, _eshape(ext, 20), "coeff_t")
        cb = _elems(coeff_b, _eshape(ext, 22), "coeff_b")
        out = None if keep_on_device else np.empty(_eshape(ext, 8 * self.n), dtype=np.uint64)
        check(lib().zk_eval_constraints_ext(self.handle, C.byref(pub), ext, ct.ctypes.data, cb.ctypes.data,
                                            None if out is None else out.ctypes.data), "zk_eval_constraints_ext")
        return out

    def close(self):
        if self.handle:
            lib().zk_lde_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ConstraintCommitment:
    """ConstraintCommitment: the composition columns' LDE and its row commitment, valid until the next proof or
    commitment on the prover."""

    def __init__(self, handle, n: int, ext: int, num_cols: int, root: bytes, blowup: int = 8):
        self.handle, self.n, self.ext, self.num_cols, self.root, self.blowup = handle, n, ext, num_cols, root, blowup

    @classmethod
    def commit(cls, lde: TraceLde, composition, ext: int = 1, num_cols: int = 8, polys: bool = False):
        """Prover::build_constraint_commitment: composition (8n, [2,] 2) in natural order, or None for the values
        lde.evaluate(..., keep_on_device=True) left on the GPU.  Returns the commitment, or with polys=True
        (commitment, CompositionPoly columns (num_cols, n, [2,] 2)).  ZkError with code ZK_ERR_DEGREE when the
        polynomial does not fit num_cols columns."""
        comp = None if composition is None else _elems(composition, _eshape(ext, 8 * lde.n), "composition")
        h, root = C.c_void_p(), C.create_string_buffer(32)
        table = np.empty(_eshape(ext, num_cols, lde.n), dtype=np.uint64) if polys else None
        check(lib().zk_commit_composition_ext(lde.handle, None if comp is None else comp.ctypes.data, ext, num_cols,
                                              C.byref(h), root, table.ctypes.data if polys else None),
              "zk_commit_composition_ext")
        cc = cls(h, lde.n, ext, num_cols, root.raw, lde.blowup)
        return (cc, table) if polys else cc

    def query(self, positions):
        """ConstraintCommitment::query: (rows (k, num_cols, [2,] 2), BatchMerkleProof bytes) at k distinct positions."""
        return _query(lambda *a: lib().zk_comp_query(self.handle, *a), positions, _eshape(self.ext, self.num_cols))

    def read_rows(self, first: int = 0, count: int | None = None, out: np.ndarray | None = None):
        """The evaluations ConstraintCommitment keeps as a RowMatrix<E>: rows (first + k) mod N, k < count (N when
        count is None), (count, num_cols, [2,] 2), each as query returns it.  out: as in TraceLde.read_rows."""
        return _read_rows(lambda *a: lib().zk_comp_read_rows(self.handle, *a), "zk_comp_read_rows",
                          self.n * self.blowup, first, count, out, _eshape(self.ext, self.num_cols))

    def close(self):
        if self.handle:
            lib().zk_comp_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the CE layout conversion called directly (csrc/diag.hip), for the tests
CE_GUARD = 4096  # bytes on each side of the destination


def ce_layout_direct(values: np.ndarray, n: int, ext: int, to_natural: bool, max_blocks: int = 0, device: int = 0):
    """The production launcher between two guard regions: values holds 8 ext n elements, (…, 2) uint64 -- ext
    coset-major planes (to_natural) or the natural interleaved order.  Returns (converted (8 ext n, 2), guard bytes:
    the lower region, then the upper, 0xA5 each when untouched)."""
    f = lib().zk_diag_ce_layout
    f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    src = _elems(np.asarray(values).reshape(-1, 2), (8 * ext * n, 2), "values")
    out, guard = np.empty_like(src), C.create_string_buffer(2 * CE_GUARD)
    check(f(device, src.ctypes.data, n, ext, int(to_natural), max_blocks, out.ctypes.data, guard), "ce_layout_direct")
    return out, guard.raw


def ce_natural_order(n: int, ext: int) -> np.ndarray:
    """The permutation the conversion applies: natural[t] = planes.reshape(-1)[perm[t]] for flat element index
    t = (r + 8 q) ext + k, perm[t] = (8 k + r) n + q."""
    t = np.arange(8 * ext * n)
    i, k = t // ext, t % ext
    return (8 * k + i % 8) * n + i // 8


# ---- the bulk row read called directly (csrc/diag.hip), for the tests
ROWS_GUARD = 4096  # bytes on each side of the staging buffer
ROWS_TILE = 64     # rows of one tile of the kernel


def rows_layout_direct(planes: np.ndarray, n: int, blowup: int, ncols: int, first: int = 0, count: int | None = None,
                       max_blocks: int = 0, cap_rows: int = 0, device: int = 0):
    """The production launcher and chunk loop on planes of the caller's choice: planes holds ncols blowup n elements,
    (…, 2) uint64, element (c, i) at (c blowup + i mod blowup) n + i div blowup.  cap_rows: the rows the staging buffer
    holds (0: a prover's own), so that small shapes cross chunk boundaries.  Returns (rows (count, ncols, 2), guard
    bytes around the staging buffer: the lower region, then the upper, 0xA5 each when untouched)."""
    f = lib().zk_diag_rows_layout
    f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, C.c_size_t,
                  C.c_void_p, C.c_void_p]
    src = _elems(np.asarray(planes).reshape(-1, 2), (max(ncols, 0) * blowup * n, 2), "planes")
    count = n * blowup if count is None else count
    out, guard = np.empty((max(count, 0), max(ncols, 0), 2), dtype=np.uint64), C.create_string_buffer(2 * ROWS_GUARD)
    check(f(device, src.ctypes.data, n, blowup, ncols, first, count, max_blocks, cap_rows, out.ctypes.data, guard),
          "rows_layout_direct")
    return out, guard.raw


def rows_natural_order(n: int, blowup: int, ncols: int, first: int = 0, count: int | None = None) -> np.ndarray:
    """The permutation the read applies: rows.reshape(-1)[k ncols + c] = planes.reshape(-1)[perm[k, c]] for row
    i = (first + k) mod N of the window, perm[k, c] = (c blowup + i mod blowup) n + i div blowup; (count, ncols)."""
    N = n * blowup
    i = (first + np.arange(N if count is None else count, dtype=np.int64)) % N
    c = np.arange(ncols, dtype=np.int64)
    return (c[None, :] * blowup + (i % blowup)[:, None]) * n + (i // blowup)[:, None]
