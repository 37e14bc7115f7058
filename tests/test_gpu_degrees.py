"""Transition constraint degrees on the GPU (zk_degrees_device / zk_degrees_columns; kernels.hip
k_transition_quotients, the composition interpolation, k_poly_degrees) against the reference of tests/degrees_ref.py
(winterfell 0.9's validate_transition_degrees over the CPU oracle).

Where the quotients are compared, every one of the 20 x 8n coefficients must equal the reference exactly; the report
(expected, actual, the three masks, max_actual, ce_len_needed), the status and the text of zk_last_error() are compared
with the reference's as well.

  * crafted traces at n = 16 (one periodic cycle, half a block of CE rows) and 32, the smallest the prover takes:
    random cells at lwe_size 1 .. 5 (every trip count of the LWE loops, every quotient generic), the all-zero trace,
    a trace constant per column;
  * VM traces at n = 64, the shortest the VM writes: a random last row passes; a zero one, or a copy of row n - 2,
    fails with six zero quotients; one changed cell makes constraint 11 alone a non-polynomial;
  * the golden `lr` (n = 128);
  * the two NTT regimes: n = 4096, the largest single-pass size, and n = 8192, the smallest four-step one, push/add
    with a random and a zero last row -- degrees only, against the closed forms (tests/test_degrees_ref_cpu.py checks
    those against the reference at n = 64 and 256);
  * the switch of zk_prover_set_validate_degrees through the three prove entry points, its order after Trace::validate,
    and a blowup-16 proof, whose check borrows the CE cosets from the blowup-16 tables;
  * zk_degrees_columns against zk_degrees_device, and the refusals.

One reference run at n = 8192 (65536 frames through the oracle, 4 s on one CPU core; not repeated here): for
ops_for_trace_len(13, "pushadd") with make_workload(seed=7) the reference gives exactly expected(8192) with the random
last row and pushadd_zero_last_row(8192) with a zero one, as the closed forms say.
"""
import ctypes as C

import numpy as np
import pytest

from degrees_ref import (ZK_ERR_DEGREES, ZK_OK, expected, pushadd_trace, pushadd_zero_last_row, reference,
                         reference_rc)
from test_degrees_ref_cpu import golden
from test_golden import options_of
from test_gpu_eval_frames import CONSTS, constant_trace, random_trace
from test_gpu_parity import oracle_pub
from validate_ref import add_to_cell
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, ProofOptions, Program, elems_bytes, make_pub_inputs, verify, vm_trace
from zkvm_amd.workloads import make_workload, ops_for_trace_len

pytestmark = pytest.mark.gpu
MAX_N = 1 << 13
ZERO_QUOTIENTS = sum(1 << k for k in (4, 5, 6, 7, 9, 10))


@pytest.fixture(scope="module")
def gpu():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=MAX_N)
    yield g
    g.close()


_REF = {}


def ref_of(oracle, key, trace, pub):
    """The reference of one trace, computed once per module."""
    if key not in _REF:
        _REF[key] = reference(oracle, trace, pub.lwe_size, pub.delta)
    return _REF[key]


_TRACES = {}


def pushadd64(last):
    if last not in _TRACES:
        _TRACES[last] = pushadd_trace(1, last)
        assert _TRACES[last][0].shape[1] == 64
    return _TRACES[last]


def last_error():
    return native.lib().zk_last_error().decode()


def check(gpu, oracle, key, trace, pub, via="device"):
    """Check `trace` on the GPU and compare coefficients, report, status and message with the reference."""
    coeffs, want, msg = ref_of(oracle, key, trace, pub)
    if via == "device":
        d, n = gpu.upload_trace(trace)
        rc, got, quot = gpu.degrees_device(d, n, pub, quotients=True)
    else:
        rc, got, quot = gpu.degrees_host(trace, pub, quotients=True)
    err = last_error()
    for k in range(20):
        assert quot[k] == coeffs[k], f"quotient {k}: a coefficient differs from the reference"
    assert got == want
    assert rc == reference_rc(want)
    if rc != ZK_OK:
        assert err == msg
    assert gpu.degrees() == got
    return got


def crafted_pub(lwe_size):
    return make_pub_inputs([0, 0], [0] * 16, lwe_size, 16)


@pytest.mark.parametrize("lwe_size", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [16, 32])
def test_random_cells(gpu, oracle, n, lwe_size):
    rep = check(gpu, oracle, ("random", n, lwe_size), random_trace(n, 31 * n + lwe_size), crafted_pub(lwe_size))
    # random cells satisfy nothing: no quotient is a polynomial, and the twelve without a periodic factor fill the domain
    assert rep["actual"][:12] == [8 * n - 1] * 12 and rep["zero_mask"] == 0 and rep["over_mask"] & 0xFFF == 0xFFF
    assert rep["ce_len_needed"] == 8 * n


@pytest.mark.parametrize("n", [16, 32])
def test_zero_and_constant_traces(gpu, oracle, n):
    zero = np.zeros((28, n, 2), dtype=np.uint64)
    rep = check(gpu, oracle, ("zero", n), zero, crafted_pub(5))
    # only the clock constraint is left: -1 / D, and every other quotient is the zero polynomial
    assert rep["zero_mask"] == ((1 << 20) - 1) & ~1 and rep["actual"][1:] == [0] * 19
    consts = [CONSTS[(c + 3) % len(CONSTS)] for c in range(28)]
    check(gpu, oracle, ("const", n, 5), constant_trace(n, consts), crafted_pub(5))
    check(gpu, oracle, ("const", n, 2), constant_trace(n, consts), crafted_pub(2))


def test_vm_trace_with_random_last_row_passes(gpu, oracle):
    trace, pub, _ = pushadd64("random")
    rep = check(gpu, oracle, "pa64_random", trace, pub)
    assert rep["actual"] == expected(64) and rep["mismatch_mask"] == 0


@pytest.mark.parametrize("last", ["zero", "copy"])
def test_vm_trace_with_a_degenerate_last_row_fails(gpu, oracle, last):
    trace, pub, _ = pushadd64(last)
    d, n = gpu.upload_trace(trace)
    rep = check(gpu, oracle, "pa64_" + last, trace, pub)
    assert gpu.degrees_device(d, n, pub)[0] == ZK_ERR_DEGREES
    assert rep["zero_mask"] == ZERO_QUOTIENTS and rep["actual"] == pushadd_zero_last_row(64)
    assert last_error() == (
        "transition constraint degrees didn't match\n"
        "expected: [  1, 253,  64, 316, 316, 316, 379, 379, 316, 316, 316, 316, 250, 439, 250, 250, 124, 124, 124, 124]\n"
        "actual:   [  1,   1,  64, 127,   0,   0,   0,   0, 127,   0,   0, 127, 250, 250, 250, 250, 124, 124, 124, 124]")


def test_changed_cell_breaks_one_quotient(gpu, oracle):
    trace, pub, _ = pushadd64("random")
    rep = check(gpu, oracle, "pa64_cell", add_to_cell(trace, 12, 5, 1), pub)
    assert rep["over_mask"] == rep["mismatch_mask"] == 1 << 11 and rep["actual"][11] == 511


@pytest.mark.parametrize("via", ["device", "host"])
def test_golden_lr(gpu, oracle, via):
    trace, _, pub, _ = golden("lr")
    rep = check(gpu, oracle, "lr", trace, pub, via=via)
    assert rep["trace_len"] == 128 and rep["actual"] == expected(128) and rep["mismatch_mask"] == 0


@pytest.mark.parametrize("log_n", [12, 13])
def test_size_regimes(gpu, log_n):
    """n = 4096: the last single-pass NTT size; n = 8192: the first four-step one.  Degrees against the closed forms."""
    n = 1 << log_n
    src = ops_for_trace_len(log_n, "pushadd")
    w = make_workload(src, seed=7)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    assert trace.shape[1] == n
    pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    rc, rep = gpu.degrees_device(*gpu.upload_trace(trace), pub)
    assert rc == ZK_OK and rep["actual"] == rep["expected"] == expected(n) and rep["ce_len_needed"] == 8 * n
    trace[:, -1, :] = 0
    rc, rep = gpu.degrees_device(*gpu.upload_trace(trace), pub)
    assert rc == ZK_ERR_DEGREES and rep["actual"] == pushadd_zero_last_row(n) and rep["zero_mask"] == ZERO_QUOTIENTS
    assert rep["over_mask"] == 0 and bin(rep["mismatch_mask"]).count("1") == 11


def vm_prove_raw(gpu, prog, inputs, last_row):
    """zk_vm_prove through ctypes: (rc, proof_len)."""
    buf = C.create_string_buffer(1 << 20)
    plen = C.c_size_t(len(buf))
    opt = ProofOptions().to_c()
    rc = native.lib().zk_vm_prove(gpu.handle, prog.handle, *inputs, elems_bytes(last_row), C.byref(opt), buf,
                                  C.byref(plen), None, None)
    return rc, plen.value, buf.raw[:plen.value]


def test_switch_refuses_a_degenerate_last_row(gpu, oracle):
    good, pub, w = pushadd64("random")
    bad = pushadd64("zero")[0]
    want = ref_of(oracle, "pa64_zero", bad, pub)[1]
    want_msg = ref_of(oracle, "pa64_zero", bad, pub)[2]
    oproof_bad = oracle.prove(bad, oracle_pub(oracle, pub))[0]
    oproof_good = oracle.prove(good, oracle_pub(oracle, pub))[0]
    prog = Program(w.source)
    inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
    try:
        # off (the default): the degenerate trace proves, to the bytes of today, and the proof verifies
        gpu.set_validate_degrees(False)
        assert gpu.prove_device(*gpu.upload_trace(bad), pub)[0] == oproof_bad
        assert gpu.prove_host(bad, pub)[0] == oproof_bad
        assert vm_prove_raw(gpu, prog, inputs, [0] * 28) == (0, len(oproof_bad), oproof_bad)
        assert verify(oproof_bad, pub, 95) == (0, "")
        gpu.set_validate_degrees(True)
        info = gpu.proof_info()
        proof, _, _, rc = gpu.prove_device(*gpu.upload_trace(bad), pub, allow_degrees_error=True)
        assert rc == native.ZK_ERR_DEGREES == ZK_ERR_DEGREES and proof == b""
        assert last_error() == want_msg and gpu.degrees() == want
        gpu.degrees_device(*gpu.upload_trace(good), pub)  # another report in between
        proof, _, _, rc = gpu.prove_host(bad, pub, allow_degrees_error=True)
        assert rc == ZK_ERR_DEGREES and proof == b"" and gpu.degrees() == want and last_error() == want_msg
        gpu.degrees_device(*gpu.upload_trace(good), pub)
        rc, plen, _ = vm_prove_raw(gpu, prog, inputs, [0] * 28)
        assert rc == ZK_ERR_DEGREES and plen == 0 and gpu.degrees() == want
        assert gpu.proof_info() == info  # no hint or snapshot moved
        # a pass goes on to the same proof bytes, through all three
        assert gpu.prove_device(*gpu.upload_trace(good), pub)[0] == oproof_good
        assert gpu.degrees()["mismatch_mask"] == 0
        assert gpu.prove_host(good, pub)[0] == oproof_good
        assert vm_prove_raw(gpu, prog, inputs, w.last_row) == (0, len(oproof_good), oproof_good)
        # both switches: Trace::validate speaks first
        gpu.set_validate(True)
        broken = add_to_cell(bad, 12, 3, 1)
        proof, _, _, rc = gpu.prove_device(*gpu.upload_trace(broken), pub, allow_trace_error=True)
        assert rc == native.ZK_ERR_TRACE and proof == b"" and gpu.degrees()["mismatch_mask"] == 0
        # ... and a trace it accepts goes on to the degree check
        proof, _, _, rc = gpu.prove_device(*gpu.upload_trace(bad), pub, allow_degrees_error=True)
        assert rc == ZK_ERR_DEGREES and proof == b"" and gpu.validation()["first_kind"] == 0
        assert gpu.prove_host(good, pub)[0] == oproof_good
    finally:
        gpu.set_validate(False)
        gpu.set_validate_degrees(False)
        prog.close()
    assert gpu.prove_device(*gpu.upload_trace(bad), pub)[0] == oproof_bad


def test_switch_keeps_the_golden_proof(gpu):
    trace, proof, pub, c = golden("lr")
    try:
        gpu.set_validate_degrees(True)
        assert gpu.prove_host(trace, pub, options_of(c))[0] == proof
        assert gpu.degrees()["actual"] == expected(128)
        assert gpu.prove_device(*gpu.upload_trace(trace), pub, options_of(c))[0] == proof
    finally:
        gpu.set_validate_degrees(False)


def test_switch_at_blowup_16(oracle):
    """The check inside a blowup-16 proof takes the CE cosets 0, 2, 4, ... of the blowup-16 tables: the same report as
    the stand-alone call, which builds the blowup-8 ones."""
    good, pub, _ = pushadd64("random")
    bad = pushadd64("zero")[0]
    opts = ProofOptions(blowup_factor=16)
    g = GpuProver(0, max_trace_len=64, max_blowup=16)
    try:
        g.set_validate_degrees(True)
        proof, _, _, rc = g.prove_device(*g.upload_trace(good), pub, opts)
        assert rc == 0 and proof == oracle.prove(good, oracle_pub(oracle, pub), oracle.default_options(blowup=16))[0]
        inside = g.degrees()
        proof, _, _, rc = g.prove_host(bad, pub, opts, allow_degrees_error=True)
        assert rc == ZK_ERR_DEGREES and proof == b""
        inside_bad = g.degrees()
        assert g.degrees_device(*g.upload_trace(good), pub) == (ZK_OK, inside)
        assert g.degrees_host(bad, pub) == (ZK_ERR_DEGREES, inside_bad)
        assert inside == ref_of(oracle, "pa64_random", good, pub)[1]
        assert inside_bad == ref_of(oracle, "pa64_zero", bad, pub)[1]
    finally:
        g.close()


def test_refusals(gpu):
    """Refused on the host, before any launch: ZK_ERR_INVALID_ARG each."""
    L = native.lib()
    _, pub, _ = pushadd64("random")
    d = gpu.trace_buffer()
    v = native.Degrees()
    cols = (C.c_void_p * 28)(*([d] * 28))
    bad = native.ZK_ERR_INVALID_ARG
    for n in (24, 8, 2 * MAX_N):
        assert L.zk_degrees_device(gpu.handle, d, n, C.byref(pub), C.byref(v), None) == bad
        assert last_error() == "trace length must be a power of two in [16, max_trace_len]"
        assert L.zk_degrees_columns(gpu.handle, cols, n, C.byref(pub), C.byref(v), None) == bad
    for lwe_size in (0, 6):
        q = crafted_pub(lwe_size)
        assert L.zk_degrees_device(gpu.handle, d, 64, C.byref(q), C.byref(v), None) == bad
        assert last_error().startswith("lwe_size must be in [1, 5]")
        assert L.zk_degrees_columns(gpu.handle, cols, 64, C.byref(q), C.byref(v), None) == bad
    assert L.zk_degrees_device(gpu.handle, d, 64, C.byref(pub), None, None) == bad
    assert L.zk_degrees_device(gpu.handle, None, 64, C.byref(pub), C.byref(v), None) == bad
    assert L.zk_degrees_columns(gpu.handle, cols, 64, None, C.byref(v), None) == bad
    holed = (C.c_void_p * 28)(*([d] * 27 + [None]))
    assert L.zk_degrees_columns(gpu.handle, holed, 64, C.byref(pub), C.byref(v), None) == bad
    h = C.c_void_p()
    native.check(L.zk_prover_create(0, 16, 8, C.byref(h)), "zk_prover_create")
    try:
        assert L.zk_prover_degrees(h, C.byref(v)) == bad  # none has run on this prover
    finally:
        L.zk_prover_destroy(h)
    native.check(L.zk_prover_create_shard(0, 64, 2, C.byref(h)), "zk_prover_create_shard")
    try:
        sd = C.c_void_p()
        native.check(L.zk_prover_trace_buffer(h, C.byref(sd)))
        assert L.zk_degrees_device(h, sd, 64, C.byref(pub), C.byref(v), None) == bad
        assert "sharded" in last_error()
        scols = (C.c_void_p * 28)(*([sd.value] * 28))
        assert L.zk_degrees_columns(h, scols, 64, C.byref(pub), C.byref(v), None) == bad
    finally:
        L.zk_prover_destroy(h)
