"""The constraint evaluator (kernels.hip k_eval_constraints) on frames no program produces.

Every proof in the suite hands the evaluator the LDE of a valid trace, whose values are generic field elements: its lazy
sums (acc160, acc192 with the "p 2^41 exceeds the negative terms" bound, acc288, reduce_fold) and its regrouped identities
never see 0, 1 or p - 1 in every operand at once.  The zk_lde_new / zk_eval_constraints plug points accept any 28-column
trace, and the oracle fills its stage dumps for traces the AIR rejects (oracle.prove_rc returns its degree error after
every stage ran), so crafted traces go through the kernel and are compared with the oracle's composition values at every
CE step, with the oracle's own composition coefficients:

  * random traces (every cell uniform below p), n = 64 and n = 8192 (the direct and the four-step plan);
  * constant columns from {0, 1, 2, p - 1, p - 2, 2^64 - 1, 2^64, 2^127, 45 2^40}: the column's LDE is that constant at
    every row, in the current and the next row of every frame at once; the assignment cycles per column over nine shifts,
    so every column sees every constant, plus the uniform traces of all 0, all 1 and all p - 1;
  * opcode-bit columns 1 .. 5 of random 0 / 1 values per row, the rest random;
  * sparse-shaped traces (columns 12 .. 27 zero but for a random last row), which at n = 8192 take the sparse fill
    instead of the transforms on the way in;
  * each of these at lwe_size 1 .. 5 (delta 16), which moves the add2 / read2 loops' bounds.

The trace root of zk_lde_new is compared with the oracle's as well.  This reaches only the base-field instantiation with
boundary rows (<1, true>, the one zk_eval_constraints launches); the extension and no-boundary instantiations are covered
through valid traces only, by the proofs and stage dumps of tests/test_gpu_option_grid.py and tests/test_gpu_parity.py.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _random_elems_bytes, oracle_pub, workload_trace
from zkvm_amd import native
from zkvm_amd.prover import GpuProver
from zkvm_amd.workloads import LR_PROGRAM

pytestmark = pytest.mark.gpu
P = 2**128 - 45 * 2**40 + 1
CONSTS = [0, 1, 2, P - 1, P - 2, 2**64 - 1, 2**64, 2**127, 45 * 2**40]
LWE_SIZES = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def gpu():
    g = GpuProver(0, max_trace_len=1 << 13)
    yield g
    g.close()


@pytest.fixture(scope="module")
def lr_pub():
    return workload_trace(LR_PROGRAM, seed=2)[1]


def with_lwe_size(pub, lwe_size):
    q = native.PubInputs()
    C.memmove(C.byref(q), C.byref(pub), C.sizeof(pub))
    q.lwe_size, q.delta = lwe_size, 16
    return q


def random_trace(n, seed):
    return np.frombuffer(_random_elems_bytes(28 * n, seed), dtype=np.uint64).reshape(28, n, 2).copy()


def constant_trace(n, values):
    """Column c holds values[c] in every row (the last included): a constant polynomial."""
    t = np.empty((28, n, 2), dtype=np.uint64)
    for c, v in enumerate(values):
        t[c, :, 0] = v & (2**64 - 1)
        t[c, :, 1] = v >> 64
    return t


def check_frames(gpu, oracle, trace, pub):
    """zk_lde_new's root and zk_eval_constraints' 8n values against the oracle's, with the oracle's coefficients."""
    n = trace.shape[1]
    orc, _, orec, od = oracle.prove_rc(trace, oracle_pub(oracle, pub), want=("composition",))
    assert orc == native.ZK_ERR_DEGREE  # the AIR rejects the trace; every stage ran
    want = od["composition"]
    assert want.shape == (8 * n, 2) and want.any()
    L = native.lib()
    hnd, root = C.c_void_p(), C.create_string_buffer(32)
    tb = np.ascontiguousarray(trace)
    native.check(L.zk_lde_new(gpu.handle, tb.ctypes.data, 28, n, 8, C.byref(hnd), root))
    try:
        assert root.raw == bytes(orec.trace_root)
        out = C.create_string_buffer(16 * 8 * n)
        native.check(L.zk_eval_constraints(hnd, C.byref(pub), bytes(orec.coeff_t), bytes(orec.coeff_b), out))
        got = np.frombuffer(out.raw, dtype=np.uint64).reshape(8 * n, 2)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{bad.size} of {8 * n} composition values differ, first at CE steps {bad[:8].tolist()}"
    finally:
        L.zk_lde_free(hnd)


@pytest.mark.parametrize("n,lwe_size", [(64, k) for k in LWE_SIZES] + [(8192, 5), (8192, 2)])
def test_random_trace(gpu, oracle, lr_pub, n, lwe_size):
    check_frames(gpu, oracle, random_trace(n, 7 * n + lwe_size), with_lwe_size(lr_pub, lwe_size))


@pytest.mark.parametrize("lwe_size", LWE_SIZES)
def test_constant_columns(gpu, oracle, lr_pub, lwe_size):
    pub = with_lwe_size(lr_pub, lwe_size)
    for shift in range(len(CONSTS)):
        check_frames(gpu, oracle, constant_trace(64, [CONSTS[(c + shift) % len(CONSTS)] for c in range(28)]), pub)
    for v in (0, 1, P - 1):
        check_frames(gpu, oracle, constant_trace(64, [v] * 28), pub)


@pytest.mark.parametrize("n,lwe_size", [(64, k) for k in LWE_SIZES] + [(8192, 5)])
def test_opcode_bit_columns(gpu, oracle, lr_pub, n, lwe_size):
    t = random_trace(n, 11 * n + lwe_size)
    bits = np.random.default_rng(n + lwe_size).integers(0, 2, size=(5, n), dtype=np.uint64)
    t[1:6, :, 0] = bits
    t[1:6, :, 1] = 0
    check_frames(gpu, oracle, t, with_lwe_size(lr_pub, lwe_size))


@pytest.mark.parametrize("n,lwe_size", [(64, k) for k in LWE_SIZES] + [(8192, 5)])
def test_sparse_shaped_trace(gpu, oracle, lr_pub, n, lwe_size):
    t = random_trace(n, 13 * n + lwe_size)
    t[12:28, : n - 1] = 0
    assert t[12:28, n - 1].any(axis=-1).all()  # a non-zero last row in every sparse column
    check_frames(gpu, oracle, t, with_lwe_size(lr_pub, lwe_size))
