"""The plug points over the challenge field on the GPU (include/zkvm_gpu.h: zk_lde_new_columns,
zk_eval_constraints_ext, zk_commit_composition_ext) and the layout kernel behind them (kernels.hip k_ce_layout).

References.  The trace and the constraints are base-field, so E enters linearly, component by component:
(a, b) c = (a c, b c) for c in F.  The a-plane of every E result is therefore the base-field result for the
a-components of the inputs, and likewise for b, and each plane is compared with the existing, oracle-pinned base-field
call; the extension's modulus never enters.  The layout kernel is compared with a numpy permutation that
tests/test_plug_ext_cpu.py pins to the scalar loop of the existing host conversion.  Every comparison is exact.

Sizes: n = 16 (the smallest accepted, less than one 64-row tile), 64, 128 (the lr trace) and 8192 (the first four-step
NTT size); blowup 8 and 16 (the CE domain stays 8n).
"""
import ctypes as C
import random

import numpy as np
import pytest

import back_half_ref as ref
import plug_ext_ref as R
from zkvm_amd import native, plug
from zkvm_amd.plug import ConstraintCommitment, TraceLde
from zkvm_amd.prover import GpuProver, ProofOptions, make_pub_inputs, vm_trace
from zkvm_amd.workloads import LR_PROGRAM, make_workload

pytestmark = pytest.mark.gpu
P = R.P
W = 28
SIZES = [16, 64, 128, 8192]


# ---------------------------------------------------------------- shared inputs, made once
@pytest.fixture(scope="module")
def gpu():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=8192, max_blowup=16)
    yield g
    g.close()


@pytest.fixture(scope="module")
def lr():
    w = make_workload(LR_PROGRAM, seed=2)
    trace, outputs, h = vm_trace(LR_PROGRAM, w.public, w.secret, w.server_key, w.last_row)
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    trace.setflags(write=False)
    assert trace.shape[1] == 128
    return trace, make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)


_traces = {}


def random_trace(n):
    """28 random columns, but column 0 a clock (0 .. n - 2, then a random last row) and column 27 zero except its
    last row: the two classes a proof would not interpolate"""
    if n not in _traces:
        rng = np.random.default_rng(1000 + n)
        t = R.rand_elems(rng, W, n)
        t[0, :n - 1, 0] = np.arange(n - 1, dtype=np.uint64)
        t[0, :n - 1, 1] = 0
        t[27, :n - 1] = 0
        t.setflags(write=False)
        _traces[n] = t
    return _traces[n]


def some_pub(lwe_size):
    rnd = random.Random(77)
    return make_pub_inputs([rnd.randrange(P) for _ in range(2)], [rnd.randrange(P) for _ in range(16)], lwe_size, 16)


def old_lde(gpu, trace, blowup):
    """zk_lde_new on the flattened trace -> (handle, root)"""
    tb = np.ascontiguousarray(trace)
    h, root = C.c_void_p(), C.create_string_buffer(32)
    native.check(native.lib().zk_lde_new(gpu.handle, tb.ctypes.data, W, tb.shape[1], blowup, C.byref(h), root))
    return h, root.raw


def old_eval(handle, pub, n, ct, cb):
    """zk_eval_constraints with base-field coefficients ((20, 2), (22, 2)) -> (8n, 2)"""
    out = np.empty((8 * n, 2), dtype=np.uint64)
    ct, cb = np.ascontiguousarray(ct), np.ascontiguousarray(cb)
    native.check(native.lib().zk_eval_constraints(handle, C.byref(pub), ct.ctypes.data, cb.ctypes.data, out.ctypes.data))
    return out


def old_commit(handle, comp, n, num_cols):
    """zk_commit_composition -> (rc, commitment handle, root, polys (num_cols, n, 2))"""
    comp = np.ascontiguousarray(comp)
    cc, root, polys = C.c_void_p(), C.create_string_buffer(32), np.zeros((num_cols, n, 2), dtype=np.uint64)
    rc = native.lib().zk_commit_composition(handle, comp.ctypes.data, num_cols, C.byref(cc), root, polys.ctypes.data)
    return rc, cc, root.raw, polys


def raw_query(fn, handle, positions, row_elems, cap=1 << 20):
    pos = (C.c_uint64 * len(positions))(*positions)
    rows, proof, plen = C.create_string_buffer(16 * row_elems * len(positions)), C.create_string_buffer(cap), C.c_size_t(cap)
    rc = fn(handle, pos, len(positions), rows, proof, C.byref(plen))
    return rc, rows.raw, proof.raw[:min(cap, plen.value)], plen.value


def positions_255(N, seed):
    """255 distinct positions in no order, both ends among them (every position when there are fewer)"""
    return random.Random(seed).sample(range(1, N - 1), 253) + [N - 1, 0] if N > 255 else list(range(N))


# ---------------------------------------------------------------- 1. the layout kernel, called directly
def coded_planes(n, ext):
    """every element distinct: (k, r, q) in the low half, a fixed mark in the high half"""
    k, r, q = np.meshgrid(np.arange(ext, dtype=np.uint64), np.arange(8, dtype=np.uint64),
                          np.arange(n, dtype=np.uint64), indexing="ij")
    a = np.empty((ext, 8, n, 2), dtype=np.uint64)
    a[..., 0] = q | (r << np.uint64(32)) | (k << np.uint64(40))
    a[..., 1] = np.uint64(0x5A5A0000) + (q ^ (r << np.uint64(20)))
    return a.reshape(ext, 8 * n, 2)


@pytest.mark.parametrize("max_blocks", [1, 3, 0])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", SIZES + [100])
def test_layout_kernel_is_the_permutation(n, ext, max_blocks):
    """Both directions against the numpy permutation, the round trip, and both guard regions.  One and three blocks
    force several grid-stride rounds (n = 8192: 128 tiles); n = 16 is a partial tile, n = 100 a whole and a partial
    one (the launcher takes any n, a proof only powers of two)."""
    assert native.device_count() > 0, "no GPU visible"
    planes = coded_planes(n, ext)
    assert len(np.unique(planes.reshape(-1, 2), axis=0)) == 8 * ext * n
    want = R.natural_from_planes(planes, n, ext).reshape(-1, 2)
    clean = b"\xa5" * (2 * plug.CE_GUARD)
    nat, guard = plug.ce_layout_direct(planes, n, ext, True, max_blocks)
    assert np.array_equal(nat, want), f"to natural: first wrong element {np.argwhere((nat != want).any(axis=1))[:4].ravel()}"
    assert guard == clean
    back, guard = plug.ce_layout_direct(nat, n, ext, False, max_blocks)
    assert np.array_equal(back, planes.reshape(-1, 2))
    assert guard == clean
    # the inverse on its own: natural values that no forward launch produced
    nat2 = np.ascontiguousarray(want[::-1])
    back2, guard = plug.ce_layout_direct(nat2, n, ext, False, max_blocks)
    assert np.array_equal(back2, R.planes_from_natural(nat2, n, ext).reshape(-1, 2))
    assert guard == clean


# ---------------------------------------------------------------- 2. zk_lde_new_columns
def frames_and_rows(L, handle, N, blowup, seed):
    cur, nxt = C.create_string_buffer(16 * W), C.create_string_buffer(16 * W)
    frames = []
    for step in (0, 1, blowup, N - blowup, N - 1, random.Random(seed).randrange(N)):
        native.check(L.zk_lde_read_frame(handle, step, cur, nxt))
        frames.append(cur.raw + nxt.raw)
    rc, rows, proof, _ = raw_query(L.zk_lde_query, handle, positions_255(N, seed), W)
    assert rc == 0
    return frames, rows, proof


@pytest.mark.parametrize("n,blowup", [(16, 8), (16, 16), (64, 8), (8192, 8), (8192, 16)])
def test_lde_new_columns_on_random_traces(gpu, oracle, n, blowup):
    """Same root, frames and openings as zk_lde_new; the root is the whole proof's (its leaves' Merkle root: the proof
    itself ends in ZK_ERR_DEGREE, a random trace violates the AIR, after the dumps are written); polys_out is the whole
    proof's trace_polys -- for the clock and the column that is zero but for its last row too."""
    L = native.lib()
    trace = random_trace(n)
    N = n * blowup
    h, root = old_lde(gpu, trace, blowup)
    old = frames_and_rows(L, h, N, blowup, n)
    L.zk_lde_free(h)
    # one pointer per column, the columns not adjacent in memory
    spread = np.zeros((W, n + 3, 2), dtype=np.uint64)
    spread[:, :n] = trace
    lde, polys = TraceLde.new(gpu, spread[:, :n], blowup, polys=True)
    with lde:
        assert lde.root == root
        assert frames_and_rows(L, lde.handle, N, blowup, n) == old
    _, _, dumps, rc = gpu.prove(trace, some_pub(5), ProofOptions(blowup_factor=blowup), dump=("trace_polys", "trace_leaves"),
                                allow_degree_error=True)
    assert rc == native.ZK_ERR_DEGREE
    assert oracle.merkle_root(dumps["trace_leaves"].tobytes()) == root
    assert np.array_equal(polys.reshape(-1, 2), dumps["trace_polys"])
    assert polys[0].any() and polys[27].any()
    # column 27 is last[27] e_(n-1): its interpolant's coefficient k is last w^-(n-1)k / n, none of them zero
    assert all(v != 0 for v in R.to_ints(polys[27]))


@pytest.mark.parametrize("blowup", [8, 16])
def test_lde_new_columns_on_the_lr_trace(gpu, lr, blowup):
    """The valid trace: the root is zk_record::trace_root of the whole proof and zk_lde_new's, the table is the proof's
    trace_polys dump.  Its clock and its unused stack registers are the classes a proof of host columns derives."""
    trace, pub = lr
    n = trace.shape[1]
    h, root = old_lde(gpu, trace, blowup)
    native.lib().zk_lde_free(h)
    lde, polys = TraceLde.new(gpu, trace, blowup, polys=True)
    lde.close()
    _, rec, dumps, rc = gpu.prove(trace, pub, ProofOptions(blowup_factor=blowup), record=True, dump=("trace_polys",))
    assert rc == 0
    assert lde.root == root == bytes(rec.trace_root)
    assert np.array_equal(polys.reshape(-1, 2), dumps["trace_polys"])
    zero_but_last = [c for c in range(W) if not trace[c, :n - 1].any() and trace[c, n - 1].any()]
    assert zero_but_last and all(polys[c].any() for c in zero_but_last)


# ---------------------------------------------------------------- 3. ext = 1 is the old call
@pytest.mark.parametrize("which,blowup", [("lr", 8), ("lr", 16), ("random", 8), ("random", 16)])
def test_ext1_is_the_existing_call_byte_for_byte(gpu, lr, which, blowup):
    L = native.lib()
    trace, pub = lr if which == "lr" else (random_trace(8192), some_pub(5))
    n = trace.shape[1]
    N = n * blowup
    rng = np.random.default_rng(5)
    ct, cb = R.rand_elems(rng, 20), R.rand_elems(rng, 22)
    pos = positions_255(N, 3)
    with TraceLde.new(gpu, trace, blowup) as lde:
        want = old_eval(lde.handle, pub, n, ct, cb)
        got = lde.evaluate(pub, ct, cb, ext=1)
        assert got.tobytes() == want.tobytes()
        rc, occ, oroot, opolys = old_commit(lde.handle, want, n, 8)
        assert rc == 0
        orows = raw_query(L.zk_comp_query, occ, pos, 8)
        L.zk_comp_free(occ)
        cc, polys = ConstraintCommitment.commit(lde, got, ext=1, num_cols=8, polys=True)
        with cc:
            assert cc.root == oroot
            assert polys.tobytes() == opolys.tobytes()
            assert raw_query(L.zk_comp_query, cc.handle, pos, 8) == orows
            rows, proof = cc.query(pos)
            assert rows.tobytes() == orows[1] and proof == orows[2]


# ---------------------------------------------------------------- 4. the evaluator over E
def coefficient_sets(rng):
    """(name, coeff_t (20, 2, 2), coeff_b (22, 2, 2)): random, then the edges"""
    ct, cb = R.rand_elems(rng, 20, 2), R.rand_elems(rng, 22, 2)
    yield "random", ct, cb
    z = ct.copy(), cb.copy()
    z[0][:, 1], z[1][:, 1] = 0, 0
    yield "every b zero", *z
    z = ct.copy(), cb.copy()
    z[0][:, 0], z[1][:, 0] = 0, 0
    yield "every a zero", *z
    top = R.to_arr([P - 1])[0]
    yield "every component p - 1", np.broadcast_to(top, (20, 2, 2)).copy(), np.broadcast_to(top, (22, 2, 2)).copy()
    for k, j in ((13, 0), (3, 1)):
        one = np.zeros((20, 2, 2), dtype=np.uint64)
        one[k, j] = ct[k, j]
        yield f"coeff_t[{k}] component {j} alone", one, np.zeros((22, 2, 2), dtype=np.uint64)
    one = np.zeros((22, 2, 2), dtype=np.uint64)
    one[21, 1] = cb[21, 1]
    yield "coeff_b[21] component b alone", np.zeros((20, 2, 2), dtype=np.uint64), one


def check_planes(lde, pub, n, ct, cb, what):
    got = lde.evaluate(pub, ct, cb, ext=2)
    assert got.shape == (8 * n, 2, 2)
    for j in range(2):
        want = old_eval(lde.handle, pub, n, ct[:, j], cb[:, j])
        assert np.array_equal(got[:, j], want), f"{what}: plane {'ab'[j]} differs from zk_eval_constraints"
    return got


@pytest.mark.parametrize("lwe_size", [1, 5])
@pytest.mark.parametrize("n,blowup", [(16, 8), (64, 16), (8192, 8)])
def test_evaluator_over_e_is_the_base_evaluator_per_plane(gpu, n, blowup, lwe_size):
    pub = some_pub(lwe_size)
    rng = np.random.default_rng(10 * n + lwe_size)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        sets = list(coefficient_sets(rng))
        for name, ct, cb in sets if n < 8192 else sets[:1]:
            got = check_planes(lde, pub, n, ct, cb, f"n={n} lwe={lwe_size} {name}")
            if name == "every b zero":
                assert not got[:, 1].any()
            if name == "every a zero":
                assert not got[:, 0].any()
            if name == "random":
                first = got
        # only the b components change: the a plane stays, the b plane moves
        _, ct, cb = sets[0]
        ct2, cb2 = ct.copy(), cb.copy()
        ct2[:, 1], cb2[:, 1] = R.rand_elems(rng, 20), R.rand_elems(rng, 22)
        again = lde.evaluate(pub, ct2, cb2, ext=2)
        assert np.array_equal(again[:, 0], first[:, 0])
        assert not np.array_equal(again[:, 1], first[:, 1])


def test_evaluator_over_e_on_the_valid_trace_and_the_proofs_own_composition(gpu, lr):
    """The lr trace (its own lwe_size), every coefficient set; then the anchor to the oracle: a FieldExtension::Quadratic
    whole proof's composition dump -- the a component, which the parity tests pin to the oracle -- is the a-plane of the
    plug point fed the record's coefficients as a-components and random b-components."""
    trace, pub = lr
    n = trace.shape[1]
    rng = np.random.default_rng(9)
    _, rec, dumps, rc = gpu.prove(trace, pub, ProofOptions(field_extension=2), record=True, dump=("composition",))
    assert rc == 0
    with TraceLde.new(gpu, trace, 8) as lde:
        for name, ct, cb in coefficient_sets(rng):
            check_planes(lde, pub, n, ct, cb, f"lr {name}")
        ct, cb = R.rand_elems(rng, 20, 2), R.rand_elems(rng, 22, 2)
        ct[:, 0] = np.frombuffer(bytes(rec.coeff_t), dtype=np.uint64).reshape(-1, 2)[:20]
        cb[:, 0] = np.frombuffer(bytes(rec.coeff_b), dtype=np.uint64).reshape(-1, 2)[:22]
        got = lde.evaluate(pub, ct, cb, ext=2)
        assert np.array_equal(got[:, 0], dumps["composition"])


def test_ext_three_is_refused(gpu):
    z20, z22 = np.zeros((20, 2, 2), dtype=np.uint64), np.zeros((22, 2, 2), dtype=np.uint64)
    with TraceLde.new(gpu, random_trace(16), 8) as lde:
        L, h, root = native.lib(), C.c_void_p(), C.create_string_buffer(32)
        pub = some_pub(5)
        for ext in (0, 3):
            assert L.zk_eval_constraints_ext(lde.handle, C.byref(pub), ext, z20.ctypes.data, z22.ctypes.data,
                                             None) == native.ZK_ERR_INVALID_ARG
            assert L.zk_commit_composition_ext(lde.handle, None, ext, 8, C.byref(h), root, None) == native.ZK_ERR_INVALID_ARG
        for num_cols in (0, 9):
            assert L.zk_commit_composition_ext(lde.handle, None, 2, num_cols, C.byref(h), root,
                                               None) == native.ZK_ERR_INVALID_ARG
        assert not h


# ---------------------------------------------------------------- 5. the commitment over E
def plane_values(oracle, coeffs, n):
    """coset-major CE values of one plane's polynomial, as an array"""
    return R.to_arr(ref.composition_values(coeffs, n, None if n == 16 else oracle.eval_coset))


def e_natural(oracle, plane_coeffs, n):
    """the natural interleaved E values of the planes' polynomials, (8n, 2, 2)"""
    return R.natural_from_planes(np.stack([plane_values(oracle, c, n) for c in plane_coeffs]), n, 2)


@pytest.mark.parametrize("num_cols", [1, 7, 8])
@pytest.mark.parametrize("n,blowup", [(16, 8), (16, 16), (64, 8)])
def test_commitment_over_e_against_the_python_root(gpu, oracle, n, blowup, num_cols):
    """Chosen column polynomials per plane: each plane of polys_out is the existing call's polys_out on that plane
    alone, and the root is the one computed in Python from the polynomials (E rows interleaved, row digests, tree)."""
    rnd = random.Random(f"commit {n} {num_cols}")
    coeffs = [[rnd.randrange(P) for _ in range(num_cols * n)] for _ in range(2)]
    coeffs[1][-1] = P - 1
    comp = e_natural(oracle, coeffs, n)
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        per_plane = []
        for j in range(2):
            rc, occ, _, opolys = old_commit(lde.handle, comp[:, j], n, num_cols)
            assert rc == 0
            native.lib().zk_comp_free(occ)
            assert R.to_ints(opolys) == coeffs[j]
            per_plane.append(opolys)
        cc, polys = ConstraintCommitment.commit(lde, comp, ext=2, num_cols=num_cols, polys=True)
        with cc:
            assert polys.shape == (num_cols, n, 2, 2)
            for j in range(2):
                assert np.array_equal(polys[:, :, j], per_plane[j])
            cols = [seg for c in range(num_cols) for seg in (coeffs[0][c * n:(c + 1) * n], coeffs[1][c * n:(c + 1) * n])]
            assert cc.root == ref.composition_root(oracle.blake3, oracle.merkle_root, oracle.eval_coset, cols, n, blowup)


@pytest.mark.parametrize("blowup", [8, 16])
def test_commitment_over_e_openings_at_8192(gpu, oracle, blowup):
    """255 distinct positions: each row's planes are the per-plane base-field commitments' rows, the row bytes are
    num_cols E elements, and the batch proof rebuilds the root from BLAKE3(row bytes)."""
    n, num_cols = 8192, 7
    N = n * blowup
    rnd = random.Random(f"open {blowup}")
    coeffs = [[rnd.randrange(P) for _ in range(num_cols * n)] for _ in range(2)]
    comp = e_natural(oracle, coeffs, n)
    pos = positions_255(N, blowup)
    L = native.lib()
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        base_rows = []
        for j in range(2):
            rc, occ, _, _ = old_commit(lde.handle, comp[:, j], n, num_cols)
            assert rc == 0
            qrc, rows, _, _ = raw_query(L.zk_comp_query, occ, pos, num_cols)
            assert qrc == 0
            L.zk_comp_free(occ)
            base_rows.append(np.frombuffer(rows, dtype=np.uint64).reshape(len(pos), num_cols, 2))
        with ConstraintCommitment.commit(lde, comp, ext=2, num_cols=num_cols) as cc:
            rows, proof = cc.query(pos)
            assert rows.shape == (len(pos), num_cols, 2, 2)
            for j in range(2):
                assert np.array_equal(rows[:, :, j], base_rows[j])
            leaves = [ref.row_digest(oracle.blake3, rows[t].tobytes()) for t in range(len(pos))]
            assert len(rows[0].tobytes()) == 32 * num_cols
            assert ref.batch_root(oracle.blake3, leaves, pos, proof, N.bit_length() - 1) == cc.root
            # the query's own refusals are the existing ones
            rc, _, _, need = raw_query(L.zk_comp_query, cc.handle, pos, 2 * num_cols, cap=len(proof) - 1)
            assert rc == native.ZK_ERR_BUFFER_TOO_SMALL and need == len(proof)
            rc, _, again, _ = raw_query(L.zk_comp_query, cc.handle, pos, 2 * num_cols, cap=need)
            assert rc == 0 and again == proof
            assert raw_query(L.zk_comp_query, cc.handle, [5, 9, 5], 2 * num_cols)[0] == native.ZK_ERR_INVALID_ARG


@pytest.mark.parametrize("plane", [0, 1])
@pytest.mark.parametrize("num_cols", [1, 7, 8])
def test_degree_edge_per_plane(gpu, oracle, num_cols, plane):
    """One coefficient at num_cols n - 1 in one plane alone commits; at num_cols n (there is one below 8n) it is
    ZK_ERR_DEGREE and no handle comes back."""
    n = 16
    rnd = random.Random(f"edge {num_cols} {plane}")
    other = [rnd.randrange(P) for _ in range(num_cols * n)]

    def comp_with(k):
        unit = [0] * (8 * n)
        unit[k] = rnd.randrange(1, P)
        planes = [other, other]
        planes[plane] = unit
        return e_natural(oracle, planes, n), unit

    with TraceLde.new(gpu, random_trace(n), 8) as lde:
        comp, unit = comp_with(num_cols * n - 1)
        cc, polys = ConstraintCommitment.commit(lde, comp, ext=2, num_cols=num_cols, polys=True)
        cc.close()
        assert R.to_ints(polys[:, :, plane]) == unit[:num_cols * n]
        assert R.to_ints(polys[:, :, 1 - plane]) == other
        if num_cols < 8:
            comp, _ = comp_with(num_cols * n)
            h, root = C.c_void_p(), C.create_string_buffer(32)
            rc = native.lib().zk_commit_composition_ext(lde.handle, comp.ctypes.data, 2, num_cols, C.byref(h), root, None)
            assert rc == native.ZK_ERR_DEGREE and not h
            with pytest.raises(native.ZkError) as e:
                ConstraintCommitment.commit(lde, comp, ext=2, num_cols=num_cols)
            assert e.value.code == native.ZK_ERR_DEGREE


# ---------------------------------------------------------------- 6. the device hand-off
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n,blowup", [(64, 8), (8192, 16)])
def test_device_hand_off_is_the_host_round_trip(gpu, n, blowup, ext):
    pub = some_pub(5)
    rng = np.random.default_rng(n + ext)
    shape = (2,) if ext == 1 else (2, 2)
    ct, cb = R.rand_elems(rng, 20, *shape[:-1]), R.rand_elems(rng, 22, *shape[:-1])
    with TraceLde.new(gpu, random_trace(n), blowup) as lde:
        comp = lde.evaluate(pub, ct, cb, ext=ext)
        cc, polys = ConstraintCommitment.commit(lde, comp, ext=ext, num_cols=8, polys=True)
        cc.close()
        assert lde.evaluate(pub, ct, cb, ext=ext, keep_on_device=True) is None
        cc2, polys2 = ConstraintCommitment.commit(lde, None, ext=ext, num_cols=8, polys=True)
        cc2.close()
        assert cc2.root == cc.root
        assert np.array_equal(polys2, polys)


def commit_kept(lde, ext):
    h, root = C.c_void_p(), C.create_string_buffer(32)
    rc = native.lib().zk_commit_composition_ext(lde.handle, None, ext, 8, C.byref(h), root, None)
    if h:
        native.lib().zk_comp_free(h)
    return rc


def test_device_hand_off_refusals(gpu):
    """composition = NULL with nothing kept, with another ext, once consumed, and after a proof on the prover"""
    n = 64
    pub = some_pub(5)
    rng = np.random.default_rng(3)
    ct, cb = R.rand_elems(rng, 20, 2), R.rand_elems(rng, 22, 2)
    trace = random_trace(n)
    with TraceLde.new(gpu, trace, 8) as lde:
        assert commit_kept(lde, 1) == native.ZK_ERR_INVALID_ARG
        assert commit_kept(lde, 2) == native.ZK_ERR_INVALID_ARG
        assert "kept" in native.lib().zk_last_error().decode()
        lde.evaluate(pub, ct, cb, ext=2, keep_on_device=True)
        assert commit_kept(lde, 1) == native.ZK_ERR_INVALID_ARG  # another ext: refused, and the values stay
        assert commit_kept(lde, 2) == native.ZK_OK
        assert commit_kept(lde, 2) == native.ZK_ERR_INVALID_ARG  # consumed
        lde.evaluate(pub, ct[:, 0], cb[:, 0], ext=1, keep_on_device=True)
        assert commit_kept(lde, 2) == native.ZK_ERR_INVALID_ARG
        lde.evaluate(pub, ct, cb, ext=2, keep_on_device=True)
        lde.evaluate(pub, ct, cb, ext=2)  # an evaluation that comes back keeps nothing
        assert commit_kept(lde, 2) == native.ZK_ERR_INVALID_ARG
        lde.evaluate(pub, ct, cb, ext=2, keep_on_device=True)
        d_trace, _ = gpu.upload_trace(trace)
        _, _, _, rc = gpu.prove_device(d_trace, n, pub, ProofOptions(), allow_degree_error=True)
        assert rc == native.ZK_ERR_DEGREE  # (a random trace; the proof ran on the prover's buffers all the same)
        assert commit_kept(lde, 2) == native.ZK_ERR_INVALID_ARG


# ---------------------------------------------------------------- 7. existing behaviour
@pytest.mark.parametrize("field_extension", [1, 2])
def test_whole_proofs_after_the_new_calls_are_unchanged(gpu, lr, field_extension):
    trace, pub = lr
    n = trace.shape[1]
    rng = np.random.default_rng(4)
    ct, cb = R.rand_elems(rng, 20, 2), R.rand_elems(rng, 22, 2)
    with TraceLde.new(gpu, trace, 8, polys=True)[0] as lde:
        comp = lde.evaluate(pub, ct, cb, ext=2)
        ConstraintCommitment.commit(lde, comp, ext=2, num_cols=8).close()
        lde.evaluate(pub, ct, cb, ext=2, keep_on_device=True)
    opts = ProofOptions(field_extension=field_extension)
    proof, _, _, rc = gpu.prove(trace, pub, opts)
    assert rc == 0
    fresh = GpuProver(0, max_trace_len=n)
    try:
        want, _, _, rc = fresh.prove(trace, pub, opts)
    finally:
        fresh.close()
    assert rc == 0 and proof == want
