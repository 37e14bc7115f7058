"""The evaluator's folded Rescue round (kernels.hip k_eval_constraints: u_k, AirConsts::pv, the selector section's
is_push) and the row hash's virtual columns through their W sets, at the shapes where the new indexing can go wrong.

Constraints 12..15 read pv[i & 127], a per-proof table of the CE step i = rc + 8 q.  A 256-thread block holds 256 / n
CE cosets when n < 256, so at n = 16 and n = 64 the index wraps inside a block and changes coset with it; n = 256 is
one coset per block, n = 1024 four blocks per coset.  Every case goes through the zk_eval_constraints plug point (the
<1, true> instantiation) on random traces, which exercise every selector and both Rescue halves at every row, against
the oracle's composition values under the oracle's own coefficients.  Those are drawn from the trace root, so every
call on the module's one prover brings new ones: a pv table left over from the call before would show at once (the
test asserts the coefficients did change).  lwe_size 2 and 4 move the ciphertext loops' bounds.

The quadratic field (KE = 2) takes E-valued coefficients, which the plug point cannot pass: it is reached through whole
proofs with the stages dumped.  With the composition dumped the prover evaluates the boundary terms per row (<2, true>;
the dump holds the a plane, comp_polys both planes).  Random traces go through it at n = 16, 64, 256, 1024 and lwe_size
2 and 4 as well: the AIR rejects them at the out-of-domain identity, after the composition commitment, and the prover
then still fills the dumps of the stages that ran, as the oracle does.  Valid programs (64 rows at the least) also run
without dumps, the <2, false> form, and their proof bytes are compared."""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_eval_frames import random_trace, with_lwe_size
from test_gpu_parity import oracle_pub, workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions
from zkvm_amd.workloads import LR_PROGRAM, cipher_mix_program

pytestmark = pytest.mark.gpu
P = 2**128 - 45 * 2**40 + 1


@pytest.fixture(scope="module")
def gpu():
    g = GpuProver(0, max_trace_len=1 << 10)
    yield g
    g.close()


@pytest.fixture(scope="module")
def lr_pub():
    return workload_trace(LR_PROGRAM, seed=2)[1]


_seen_coeffs = []


@pytest.mark.parametrize("lwe_size", [2, 4])
@pytest.mark.parametrize("n", [16, 64, 256, 1024])
def test_plug_point_against_oracle(gpu, oracle, lr_pub, n, lwe_size):
    pub = with_lwe_size(lr_pub, lwe_size)
    trace = random_trace(n, 31 * n + lwe_size)
    orc, _, orec, od = oracle.prove_rc(trace, oracle_pub(oracle, pub), want=("composition",))
    assert orc == native.ZK_ERR_DEGREE  # the AIR rejects a random trace; every stage ran
    want = od["composition"]
    assert want.shape == (8 * n, 2) and want.any()
    ct = bytes(orec.coeff_t)
    assert ct[16 * 12:16 * 16] not in _seen_coeffs  # coefficients 12..15 (u and pv) differ from every call before
    _seen_coeffs.append(ct[16 * 12:16 * 16])
    L = native.lib()
    hnd = C.c_void_p()
    tb = np.ascontiguousarray(trace)
    native.check(L.zk_lde_new(gpu.handle, tb.ctypes.data, 28, n, 8, C.byref(hnd), C.create_string_buffer(32)))
    try:
        out = C.create_string_buffer(16 * 8 * n)
        native.check(L.zk_eval_constraints(hnd, C.byref(pub), ct, bytes(orec.coeff_b), out))
        got = np.frombuffer(out.raw, dtype=np.uint64).reshape(8 * n, 2)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{bad.size} of {8 * n} composition values differ, first at CE steps {bad[:8].tolist()}"
    finally:
        L.zk_lde_free(hnd)


def test_same_lde_two_coefficient_sets(gpu, oracle, lr_pub):
    """One committed LDE evaluated under two coefficient sets in a row: the second call's values are those of its own
    coefficients (the oracle's), the first call's those of the same vector with coefficients 12..15 negated -- which
    changes the composition by exactly -2 times their share, so the two outputs must differ."""
    n = 64
    pub = with_lwe_size(lr_pub, 4)
    trace = random_trace(n, 977)
    _, _, orec, od = oracle.prove_rc(trace, oracle_pub(oracle, pub), want=("composition",))
    ct = bytearray(bytes(orec.coeff_t))
    other = bytearray(ct)
    for k in range(12, 16):
        v = int.from_bytes(ct[16 * k:16 * k + 16], "little")
        other[16 * k:16 * k + 16] = ((P - v) % P).to_bytes(16, "little")
    L = native.lib()
    hnd = C.c_void_p()
    tb = np.ascontiguousarray(trace)
    native.check(L.zk_lde_new(gpu.handle, tb.ctypes.data, 28, n, 8, C.byref(hnd), C.create_string_buffer(32)))
    try:
        first, second = C.create_string_buffer(16 * 8 * n), C.create_string_buffer(16 * 8 * n)
        native.check(L.zk_eval_constraints(hnd, C.byref(pub), bytes(other), bytes(orec.coeff_b), first))
        native.check(L.zk_eval_constraints(hnd, C.byref(pub), bytes(ct), bytes(orec.coeff_b), second))
        assert second.raw == od["composition"].tobytes()
        assert first.raw != second.raw
    finally:
        L.zk_lde_free(hnd)


@pytest.mark.parametrize("lwe_size", [2, 4])
@pytest.mark.parametrize("n", [16, 64, 256, 1024])
def test_quadratic_field_rejected_trace(gpu, oracle, lr_pub, n, lwe_size):
    """<2, true> on a random trace: 256 / n CE cosets per block, K2->pv[i & 127] and the second plane's cube weights."""
    pub = with_lwe_size(lr_pub, lwe_size)
    trace = random_trace(n, 37 * n + lwe_size)
    names = ("composition", "comp_polys")
    orc, _, orec, od = oracle.prove_rc(trace, oracle_pub(oracle, pub), oracle.default_options(field_extension=2),
                                       want=names)
    assert orc == native.ZK_ERR_DEGREE and od["composition"].any()
    _, _, dumps, rc = gpu.prove(trace, pub, ProofOptions(field_extension=2), dump=names, allow_degree_error=True)
    assert rc == native.ZK_ERR_DEGREE
    bad = np.flatnonzero((dumps["composition"] != od["composition"][:8 * n]).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {8 * n} composition values (a plane) differ, first at CE steps {bad[:8].tolist()}"
    k = 2 * orec.num_ccols * n
    assert od["comp_polys"][:k].any()
    assert np.array_equal(dumps["comp_polys"][:k], od["comp_polys"][:k])  # both planes' column polynomials


QUADRATIC = [("push.5\npush.3\nadd", 64), (cipher_mix_program(4)[0], 256), (cipher_mix_program(12)[0], 1024)]


@pytest.mark.parametrize("src,n", QUADRATIC, ids=[str(n) for _, n in QUADRATIC])
def test_quadratic_field_against_oracle(gpu, oracle, src, n):
    trace, pub = workload_trace(src, seed=n)
    assert trace.shape[1] == n
    names = ("composition", "comp_polys")
    opts = ProofOptions(field_extension=2)
    oproof, orec, odumps = oracle.prove(trace, oracle_pub(oracle, pub), oracle.default_options(field_extension=2),
                                        want=names)
    proof, _, dumps, rc = gpu.prove(trace, pub, opts, dump=names)  # boundary terms per row: <2, true>
    assert rc == 0
    assert np.array_equal(dumps["composition"], odumps["composition"][:8 * n])
    k = 2 * orec.num_ccols * n
    assert np.array_equal(dumps["comp_polys"][:k], odumps["comp_polys"][:k])  # both planes
    assert proof == oproof
    proof, _, _, rc = gpu.prove(trace, pub, opts)  # <2, false>, boundary terms in coefficient form
    assert rc == 0 and proof == oproof


def test_row_hash_virtual_columns(oracle):
    """hash_rows_blocks at n = 64, blowup 8, with virtual columns in BLAKE3 blocks 5 and 6 (columns 20, 21, 23 and
    25, 27), launched as blocks [0, 5) and [5, 7) and as [0, 6) and [6, 7): a virtual column's LDE is never read (the
    buffer holds other values there), its element is last[c] * lagr_lde[r n + q].  Leaves against the oracle's BLAKE3 of
    the rows built with Python integers; the last-row values include 0, 1 and p - 1."""
    n, B, W = 64, 8, 28
    N = n * B
    rnd = random.Random(64)
    lde = [rnd.randrange(P) for _ in range(W * N)]  # coset-major: (c B + r) n + q
    lagr = [rnd.randrange(P) for _ in range(N)]
    lagr[0], lagr[1], lagr[N - 1] = 0, 1, P - 1
    last = [rnd.randrange(P) for _ in range(W)]
    last[20], last[23], last[27] = P - 1, 0, 1
    virt = (20, 21, 23, 25, 27)
    mask = sum(1 << c for c in virt)
    to_b = lambda vals: b"".join(v.to_bytes(16, "little") for v in vals)
    want = []
    for i in range(N):
        r, q = i % B, i // B
        row = [last[c] * lagr[r * n + q] % P if c in virt else lde[(c * B + r) * n + q] for c in range(W)]
        want.append(oracle.blake3(to_b(row)))
    f = native.lib().zk_diag_hash_rows_virtual
    f.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    f.restype = C.c_int
    for split in (5, 6):
        out = C.create_string_buffer(32 * N)
        native.check(f(0, to_b(lde), n, B, mask, to_b(last), to_b(lagr), split, out))
        bad = [i for i in range(N) if out.raw[32 * i:32 * i + 32] != want[i]]
        assert not bad, f"split {split}: {len(bad)} of {N} leaves differ, first rows {bad[:8]}"
