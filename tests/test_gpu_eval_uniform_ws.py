"""The constraint evaluator's products by constants of the proof through W sets (kernels.hip k_eval_constraints:
AirConsts::ws read by scalar loads, fe_mul_uniform, the lazy sums acc192 / acc288_madd_uniform of f128.hpp).

Composition values, all four instances of the kernel, element for element or through the proof bytes:
  <1, true>   the zk_eval_constraints plug point on random traces (they violate the AIR, so every selector and both
              Rescue halves are non-zero at every row) against the oracle's composition under the oracle's coefficients;
  <2, true>   whole proofs in the quadratic field with the composition dumped, on the same kind of trace (both planes
              through comp_polys);
  <1, false>, <2, false>   valid programs without dumps, the proof bytes against the oracle's.
n = 16, 64, 256, 1024 and lwe_size 2, 4, 5 for the first two.  A 256-thread block holds 256 / n CE cosets: at n = 16 the
one block spans all eight, at n = 64 four; n = 256 and n = 1024 wrap i mod 128 (the pv table and the periodic columns)
many times inside a coset.

The lazy sums on their own (zk_diag_field_op 18 .. 20) against Python integers: 16 terms, more than the evaluator's
longest sum (12 W-set terms; 10 on top of a start value), and ACC192_MAX_TERMS = 2^15 terms, each with all-(p - 1)
operands, the largest column sums there are, and with random and edge operands."""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_eval_frames import check_frames, random_trace, with_lwe_size
from test_gpu_parity import oracle_pub, workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions, bytes_elems, elems_bytes
from zkvm_amd.workloads import LR_PROGRAM, cipher_mix_program

pytestmark = pytest.mark.gpu
P = 2**128 - 45 * 2**40 + 1
SIZES = [16, 64, 256, 1024]
LWE_SIZES = [2, 4, 5]
ACC192_MAX_TERMS = 1 << 15  # f128.hpp


@pytest.fixture(scope="module")
def gpu():
    g = GpuProver(0, max_trace_len=1 << 10)
    yield g
    g.close()


@pytest.fixture(scope="module")
def lr_pub():
    return workload_trace(LR_PROGRAM, seed=2)[1]


@pytest.mark.parametrize("lwe_size", LWE_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_base_field_rows_with_boundary(gpu, oracle, lr_pub, n, lwe_size):
    check_frames(gpu, oracle, random_trace(n, 41 * n + lwe_size), with_lwe_size(lr_pub, lwe_size))


@pytest.mark.parametrize("lwe_size", LWE_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_quadratic_field_rows_with_boundary(gpu, oracle, lr_pub, n, lwe_size):
    pub = with_lwe_size(lr_pub, lwe_size)
    trace = random_trace(n, 43 * n + lwe_size)
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


VALID = [("push.5\npush.3\nadd", 64), (cipher_mix_program(4)[0], 256), (cipher_mix_program(12)[0], 1024)]


@pytest.mark.parametrize("field_extension", [1, 2])
@pytest.mark.parametrize("src,n", VALID, ids=[str(n) for _, n in VALID])
def test_rows_without_boundary_through_the_proof(gpu, oracle, src, n, field_extension):
    trace, pub = workload_trace(src, seed=n + field_extension)
    assert trace.shape[1] == n
    oproof, _, _ = oracle.prove(trace, oracle_pub(oracle, pub), oracle.default_options(field_extension=field_extension))
    proof, _, _, rc = gpu.prove(trace, pub, ProofOptions(field_extension=field_extension))
    assert rc == 0 and proof == oproof


# ---------------------------------------------------------------- the lazy sums of W-set products
def run_op(op, a, b):
    out = C.create_string_buffer(16 * len(a))
    native.check(native.lib().zk_diag_field_op(0, op, elems_bytes(a), elems_bytes(b), out, len(a)))
    return bytes_elems(out.raw)


def _operands():
    """192 lanes (three waves): wave 0 all p - 1 under the constant p - 1, wave 1 edge values, wave 2 random."""
    rnd = random.Random(192)
    edges = [0, 1, P - 1, P - 2, 2**32 - 1, 2**64, 2**96 - 1, 2**127, 45 * 2**40, 2**128 - 2**96 - 1]
    a = [P - 1] * 64 + [edges[i % len(edges)] for i in range(64)] + [rnd.randrange(P) for _ in range(64)]
    b = [P - 1] * 64 + [P - 1] + [rnd.randrange(P) for _ in range(63)] + [rnd.randrange(P) for _ in range(64)]
    return a, b


def test_acc192_sixteen_terms():
    a, b = _operands()
    m = len(a)
    got = run_op(18, a, b)
    for t in range(m):
        w = b[t & ~63]
        assert got[t] == (a[t] + sum(a[(t + j) % m] * w for j in range(16))) % P, t


def test_acc288_product_plus_sixteen_uniform_terms():
    a, b = _operands()
    m = len(a)
    got = run_op(19, a, b)
    for t in range(m):
        w = b[t & ~63]
        assert got[t] == (a[t] * b[t] + sum(a[(t + j) % m] * w for j in range(16))) % P, t


def test_acc192_most_terms():
    a, b = _operands()
    got = run_op(20, a, b)
    for t in range(len(a)):
        assert got[t] == (a[t] + ACC192_MAX_TERMS * a[t] * b[t & ~63]) % P, t
