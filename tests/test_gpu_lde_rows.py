"""The committed LDEs read in bulk as row matrices on the GPU (include/zkvm_gpu.h: zk_lde_read_rows,
zk_comp_read_rows) and the layout kernel behind them (kernels.hip k_rows_layout, through the chunk loop of
prover.hip's rows_to_host).

References, every comparison exact.  The kernel: a numpy permutation (plug.rows_natural_order) that
tests/test_lde_rows_cpu.py pins to the index formula of the existing host conversion.  The trace rows: zk_lde_query and
zk_lde_read_frame (gather_rows, another kernel), the CPU oracle's LDE, and the trace_lde dump of a whole proof (permuted
on the host).  The constraint rows: the column polynomials evaluated over the LDE coset by the oracle, the Merkle root
rebuilt from the rows in Python, and zk_comp_query.

Sizes: n = 16 (N = 128: two tiles), 64, 128 (the lr trace), 8192 at blowup 16 (the prover's staging buffer holds half
the rows: two chunks on the production path); the direct calls also blowup 64 (one value of i div B per tile), narrow
rows and n = 100 (a partial last tile).
"""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

import back_half_ref as ref
import merkle_ref
import plug_ext_ref as R
from zkvm_amd import native, plug
from zkvm_amd.plug import ConstraintCommitment, TraceLde
from zkvm_amd.prover import GpuProver, ProofOptions, make_pub_inputs

pytestmark = pytest.mark.gpu
P = R.P
W = 28
TILE = plug.ROWS_TILE
GOLD = Path(__file__).resolve().parent / "golden"
CLEAN = b"\xa5" * (2 * plug.ROWS_GUARD)


# ---------------------------------------------------------------- shared inputs, made once
@pytest.fixture(scope="module")
def gpu():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=8192, max_blowup=16)
    yield g
    g.close()


def golden_case(name):
    c = next(c for c in json.loads((GOLD / "cases.json").read_text())["cases"] if c["name"] == name)
    o = c["options"]
    opts = ProofOptions(o["num_queries"], o["blowup"], o["grinding"], o["field_extension"], o["fri_folding"],
                        o["fri_rem_max_deg"])
    pub = make_pub_inputs([int(h, 16) for h in c["program_hash"]], [int(h, 16) for h in c["stack_outputs"]],
                          c["lwe_size"], c["delta"])
    trace = np.load(GOLD / f"{name}.trace.npy", allow_pickle=False)
    trace.setflags(write=False)
    return trace, pub, opts, (GOLD / f"{name}.proof").read_bytes()


@pytest.fixture(scope="module")
def lr():
    """the lr trace with its public inputs: (trace (28, 128, 2), pub)"""
    trace, pub, _, _ = golden_case("lr")
    assert trace.shape == (W, 128, 2)
    return trace, pub


_traces = {}


def random_trace(n):
    if n not in _traces:
        t = R.rand_elems(np.random.default_rng(2000 + n), W, n)
        t.setflags(write=False)
        _traces[n] = t
    return _traces[n]


def some_pub(lwe_size=5):
    rnd = random.Random(78)
    return make_pub_inputs([rnd.randrange(P) for _ in range(2)], [rnd.randrange(P) for _ in range(16)], lwe_size, 16)


def positions_255(N, seed):
    """255 distinct positions in no order, both ends among them (every position when there are fewer)"""
    return random.Random(seed).sample(range(1, N - 1), 253) + [N - 1, 0] if N > 255 else list(range(N))


# ---------------------------------------------------------------- 1. the layout kernel, called directly
SHAPES = [(16, 8, 28), (16, 64, 28), (64, 16, 1), (64, 8, 7), (128, 8, 14), (8192, 16, 28), (8192, 8, 16), (100, 8, 28)]
_planes = {}


def coded_planes(n, blowup, ncols):
    """every element distinct: (c, r, q) in the low half, a fixed mark in the high half; (ncols blowup n, 2)"""
    key = (n, blowup, ncols)
    if key not in _planes:
        c, r, q = np.meshgrid(np.arange(ncols, dtype=np.uint64), np.arange(blowup, dtype=np.uint64),
                              np.arange(n, dtype=np.uint64), indexing="ij")
        a = np.empty((ncols, blowup, n, 2), dtype=np.uint64)
        a[..., 0] = q | (r << np.uint64(32)) | (c << np.uint64(40))
        a[..., 1] = np.uint64(0x5A5A0000) + (q ^ (r << np.uint64(20)))
        a = a.reshape(-1, 2)
        a.setflags(write=False)
        _planes[key] = a
    return _planes[key]


def windows(N, blowup):
    """(first, count): whole; one row; a window that wraps; one from the row before a tile boundary to two rows past
    the next boundary (it wraps where the domain is two tiles)"""
    return [(0, N), (1, 1), (N - 3, 3 + blowup), (TILE - 1, TILE + 3)]


def check_window(n, blowup, ncols, first, count, max_blocks=0, cap_rows=0):
    planes = coded_planes(n, blowup, ncols)
    want = planes[plug.rows_natural_order(n, blowup, ncols, first, count)]
    got, guard = plug.rows_layout_direct(planes, n, blowup, ncols, first, count, max_blocks, cap_rows)
    what = f"n={n} blowup={blowup} ncols={ncols} first={first} count={count} blocks={max_blocks} cap={cap_rows}"
    assert got.shape == want.shape == (count, ncols, 2)
    assert np.array_equal(got, want), f"{what}: first wrong rows {np.argwhere((got != want).any(axis=(1, 2)))[:4].ravel()}"
    assert guard == CLEAN, what


@pytest.mark.parametrize("max_blocks", [1, 3, 0])
@pytest.mark.parametrize("n,blowup,ncols", SHAPES)
def test_layout_kernel_is_the_permutation(n, blowup, ncols, max_blocks):
    """Every window against the numpy permutation, with both guard regions.  One and three blocks force several
    grid-stride rounds (8192 x 16: 2048 tiles)."""
    assert native.device_count() > 0, "no GPU visible"
    N = n * blowup
    if (n, blowup, ncols) == SHAPES[0]:
        assert len(np.unique(coded_planes(n, blowup, ncols), axis=0)) == ncols * N
    for first, count in windows(N, blowup):
        assert first < N and 1 <= count <= N + blowup
        check_window(n, blowup, ncols, first, count, max_blocks)


def chunks(N, first, count, cap):
    """the launches of the chunk loop: a chunk ends at the staging buffer's capacity or at the domain's end"""
    k, done = 0, 0
    while done < count:
        done += min(count - done, N - (first + done) % N, cap)
        k += 1
    return k


@pytest.mark.parametrize("n,blowup,ncols", SHAPES)
def test_small_staging_buffers_cross_chunk_boundaries(n, blowup, ncols):
    """The longest window (N + blowup rows from N - 3: it wraps) and the whole domain, through staging buffers of one
    tile's rows or N / 256 tiles', and of N / 3 - 5 rows, which is no multiple of a tile"""
    assert native.device_count() > 0, "no GPU visible"
    N = n * blowup
    even, odd = TILE * max(1, N // (4 * TILE)), N // 3 - 5
    assert even % TILE == 0 and odd % TILE
    for first, count, cap in ((N - 3, N + blowup, even), (N - 3, N + blowup, odd), (0, N, odd)):
        assert chunks(N, first, count, cap) >= 3
        check_window(n, blowup, ncols, first, count, 0, cap)


# ---------------------------------------------------------------- 2. the trace rows
def check_against_queries_and_frames(lde, rows, seed):
    N, B = lde.n * lde.blowup, lde.blowup
    assert rows.shape == (N, W, 2) and rows.dtype == np.uint64
    pos = positions_255(N, seed)
    opened, _ = lde.query(pos)
    assert np.array_equal(rows[pos], opened)
    for step in (0, 1, N - B, N - 1):
        cur, nxt = lde.read_frame(step)
        window = lde.read_rows(step, B + 1)  # (past the domain's end for the last two steps: it wraps)
        assert np.array_equal(window[0], cur) and np.array_equal(window[B], nxt), step
        assert np.array_equal(window, rows[(step + np.arange(B + 1)) % N]), step


@pytest.mark.parametrize("n,blowup", [(16, 8), (16, 16), (64, 8), (128, 8), (8192, 16)])
def test_trace_rows_of_random_traces(gpu, oracle, n, blowup):
    trace = random_trace(n)
    with TraceLde.new(gpu, trace, blowup) as lde:
        rows = lde.read_rows()
        check_against_queries_and_frames(lde, rows, n + blowup)
    if n in (16, 64):  # the CPU oracle's LDE (the proof itself ends in OR_ERR_DEGREE: a random trace violates the AIR)
        opub = oracle.make_pub([1, 2], list(range(16)))
        _, _, _, od = oracle.prove_rc(trace, opub, oracle.default_options(blowup=blowup), want=("trace_lde",))
        assert od["trace_lde"].any()
        assert np.array_equal(rows.reshape(-1, 2), od["trace_lde"])


def test_trace_rows_of_the_lr_trace(gpu, oracle, lr):
    """... and the whole proof's trace_lde dump (coset_major_rows_to_host: the host's permutation), taken before the
    handle is built, and the oracle's"""
    trace, pub = lr
    _, _, dumps, rc = gpu.prove(trace, pub, ProofOptions(), dump=("trace_lde",))
    assert rc == 0
    with TraceLde.new(gpu, trace, 8) as lde:
        rows = lde.read_rows()
        check_against_queries_and_frames(lde, rows, 7)
        into = np.full((200, W, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert lde.read_rows(1000, 24 + 8, out=into[100:132]) is not None  # the caller's array, and it wraps
        assert np.array_equal(into[100:132], rows[(1000 + np.arange(32)) % 1024])
        assert (into[:100] == 0xA5A5A5A5A5A5A5A5).all() and (into[132:] == 0xA5A5A5A5A5A5A5A5).all()
    assert np.array_equal(rows.reshape(-1, 2), dumps["trace_lde"])
    opub = oracle.make_pub(R.to_ints(np.frombuffer(bytes(pub.program_hash), dtype=np.uint64)),
                           R.to_ints(np.frombuffer(bytes(pub.stack_outputs), dtype=np.uint64)), pub.lwe_size, pub.delta)
    _, _, od = oracle.prove(trace, opub, want=("trace_lde",))
    assert np.array_equal(rows.reshape(-1, 2), od["trace_lde"])


# ---------------------------------------------------------------- 3. the constraint rows
def plane_values(oracle, coeffs, n):
    return R.to_arr(ref.composition_values(coeffs, n, None if n == 16 else oracle.eval_coset))


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("num_cols", [1, 7, 8])
@pytest.mark.parametrize("n,blowup", [(16, 8), (16, 16), (64, 8)])
def test_constraint_rows_against_the_column_polynomials(gpu, oracle, n, blowup, num_cols, ext):
    """Chosen column polynomials: the rows are polys_out's columns (over E the components a, b of each) evaluated over
    the LDE coset by the oracle, and the tree over the rows' digests (tests/merkle_ref.py) has the returned root."""
    N = n * blowup
    rnd = random.Random(f"rows {n} {blowup} {num_cols} {ext}")
    coeffs = [[rnd.randrange(P) for _ in range(num_cols * n)] for _ in range(ext)]
    comp = R.natural_from_planes(np.stack([plane_values(oracle, c, n) for c in coeffs]), n, ext)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        cc, polys = ConstraintCommitment.commit(lde, comp, ext=ext, num_cols=num_cols, polys=True)
        with cc:
            rows = cc.read_rows()
            wrapped = cc.read_rows(N - 3, 3 + blowup)
    assert rows.shape == ((N, num_cols, 2) if ext == 1 else (N, num_cols, 2, 2))
    polys = polys.reshape(num_cols, n, ext, 2)
    cols = [R.to_ints(polys[c, :, k]) for c in range(num_cols) for k in range(ext)]
    assert cols == [coeffs[k][c * n:(c + 1) * n] for c in range(num_cols) for k in range(ext)]
    ldes = [oracle.eval_coset(col, N, ref.FRI_OFFSET) for col in cols]
    want = R.to_arr([v for row in zip(*ldes) for v in row]).reshape(rows.shape)
    assert np.array_equal(rows, want)
    assert np.array_equal(wrapped, want[(N - 3 + np.arange(3 + blowup)) % N])
    leaves = b"".join(ref.row_digest(oracle.blake3, rows[i].tobytes()) for i in range(N))
    assert merkle_ref.root(leaves) == cc.root


@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_rows_against_openings_at_8192(gpu, ext):
    n, blowup = 8192, 16
    N = n * blowup
    rng = np.random.default_rng(40 + ext)
    lead = () if ext == 1 else (2,)
    ct, cb = R.rand_elems(rng, 20, *lead), R.rand_elems(rng, 22, *lead)
    pos = positions_255(N, ext)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        comp = lde.evaluate(some_pub(), ct, cb, ext=ext)
        with ConstraintCommitment.commit(lde, comp, ext=ext, num_cols=8) as cc:
            rows = cc.read_rows()
            opened, _ = cc.query(pos)
    assert rows.shape == (N, 8, *lead, 2)
    assert np.array_equal(rows[pos], opened)
    assert len(np.unique(rows.reshape(N, -1), axis=0)) == N


# ---------------------------------------------------------------- 4. what the reads leave alone
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,blowup", [(64, 8), (8192, 16)])
def test_reads_keep_the_values_left_on_the_device(gpu, n, blowup, ext):
    """evaluate(keep_on_device), both reads, commit(None): the host round trip's commitment.  The earlier commitment's
    handle reads the same rows before and after the evaluation."""
    pub = some_pub()
    rng = np.random.default_rng(n + ext)
    lead = () if ext == 1 else (2,)
    ct, cb = R.rand_elems(rng, 20, *lead), R.rand_elems(rng, 22, *lead)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        comp = lde.evaluate(pub, ct, cb, ext=ext)
        cc, polys = ConstraintCommitment.commit(lde, comp, ext=ext, num_cols=8, polys=True)
        with cc:
            trace_rows, comp_rows = lde.read_rows(), cc.read_rows()
            assert lde.evaluate(pub, ct, cb, ext=ext, keep_on_device=True) is None
            assert np.array_equal(lde.read_rows(), trace_rows)
            assert np.array_equal(cc.read_rows(), comp_rows)
            assert np.array_equal(cc.read_rows(n * blowup - 1, 9), comp_rows[(n * blowup - 1 + np.arange(9)) % (n * blowup)])
        cc2, polys2 = ConstraintCommitment.commit(lde, None, ext=ext, num_cols=8, polys=True)
        with cc2:
            assert cc2.root == cc.root
            assert np.array_equal(polys2, polys)
            assert np.array_equal(cc2.read_rows(), comp_rows)
            assert np.array_equal(lde.read_rows(), trace_rows)


@pytest.mark.parametrize("name", ["lr", "lr_quad"])
def test_whole_proofs_after_the_reads_are_the_golden_bytes(gpu, name):
    trace, pub, opts, proof = golden_case(name)
    n, ext = trace.shape[1], opts.field_extension
    rng = np.random.default_rng(6)
    lead = () if ext == 1 else (2,)
    ct, cb = R.rand_elems(rng, 20, *lead), R.rand_elems(rng, 22, *lead)
    for _ in range(2):  # (the second proof runs with what the first one learned about the columns)
        with TraceLde.new(gpu, trace, 8) as lde:
            comp = lde.evaluate(pub, ct, cb, ext=ext)
            with ConstraintCommitment.commit(lde, comp, ext=ext, num_cols=8) as cc:
                lde.read_rows()
                cc.read_rows(8 * n - 1, 9)
            lde.read_rows(5, 100)
        got, _, _, rc = gpu.prove(trace, pub, opts)
        assert rc == 0 and got == proof


def test_interleaved_reads_of_two_handles(gpu):
    """Two provers, one trace LDE each: windows read in turn are each handle's own rows"""
    other = GpuProver(0, max_trace_len=64)
    try:
        with TraceLde.new(gpu, random_trace(128), 16) as a, TraceLde.new(other, random_trace(64), 8) as b:
            rows_a, rows_b = a.read_rows(), b.read_rows()
            assert not np.array_equal(rows_a[:512], rows_b)
            for first in (0, 100, 500):
                wa = a.read_rows(first, 300)
                wb = b.read_rows(first, 50)
                assert np.array_equal(wa, rows_a[first:first + 300])
                assert np.array_equal(wb, rows_b[(first + np.arange(50)) % 512])
            pa, pb = positions_255(2048, 1), positions_255(512, 2)
            assert np.array_equal(rows_a[pa], a.query(pa)[0]) and np.array_equal(rows_b[pb], b.query(pb)[0])
    finally:
        other.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_buffer_untouched(gpu):
    L = native.lib()
    n, blowup = 16, 8
    N = n * blowup
    comp = np.zeros((8 * n, 2), dtype=np.uint64)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        with ConstraintCommitment.commit(lde, comp, ext=1, num_cols=1) as cc:
            for call, handle, row in ((L.zk_lde_read_rows, lde.handle, 16 * W), (L.zk_comp_read_rows, cc.handle, 16)):
                fill = b"\x5a" * (row * (N + blowup + 1))
                buf = C.create_string_buffer(fill, len(fill))
                for h, first, count, out in ((None, 0, 1, buf), (handle, 0, 1, None), (handle, N, 1, buf),
                                             (handle, N + 5, 1, buf), (handle, 0, 0, buf), (handle, 3, N + blowup + 1, buf),
                                             (handle, 0, 2**63, buf)):
                    assert call(h, first, count, out) == native.ZK_ERR_INVALID_ARG, (first, count)
                    assert L.zk_last_error()
                    assert buf.raw == fill
                assert call(handle, N - 1, N + blowup, buf) == native.ZK_OK  # the longest window is read
                assert buf.raw[:row * (N + blowup)] != fill[:row * (N + blowup)] and buf.raw[row * (N + blowup):] == fill[:row]
            with pytest.raises(native.ZkError) as e:
                lde.read_rows(N, 1)
            assert e.value.code == native.ZK_ERR_INVALID_ARG
            with pytest.raises(ValueError):
                lde.read_rows(0, 4, out=np.zeros((4, W, 2), dtype=np.int64))
