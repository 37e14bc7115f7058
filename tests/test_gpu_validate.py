"""Trace validation on the GPU (zk_validate_device / zk_validate_columns, kernels.hip k_validate_trace) against the
reference validator of tests/validate_ref.py (winterfell 0.9's Trace::validate over the CPU oracle's ProcessorAir).

Every case compares the whole report -- per-constraint counts, first steps and values, the failing-step total, the
assertion mask and found values, the first failure's kind / index / step -- the status, and the text of
zk_last_error() with the reference's wording of the first failure.

  * valid traces of VM programs, through the device and the host entry point;
  * random traces (every cell uniform below p) at the lengths where the indexing can go wrong -- n = 16 (one hash
    cycle, a partial wave), 64, 256 (the last two threads of a full block stay out), 512 (a frame's next row in the
    next block), 8192 (many blocks adding into one report: every count equals n - 2 only if no step is missed or
    counted twice) -- at lwe_size 1 .. 5;
  * constant-column traces with the edge constants of test_gpu_eval_frames.CONSTS;
  * single-cell corruptions of a valid n = 128 trace (the set tests/test_validate_cpu.py proves to reach every
    constraint and assertion), where a change in row n - 1 alone must stay valid;
  * one changed cell in a valid 2^16 trace at a wave boundary, a block boundary and the ends of the range;
  * the validate switch of zk_prover_set_validate on one warm prover;
  * the argument refusals, all decided on the host before any launch.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_eval_frames import CONSTS, constant_trace, random_trace, with_lwe_size
from test_gpu_parity import oracle_pub, workload_trace
from test_validate_cpu import BIT_COLS, corruption_rows, valid_trace_128
from validate_ref import (ZK_ERR_TRACE, ZK_OK, add_to_cell, neighbour_steps, reference_message, reference_rc,
                          reference_report)
from zkvm_amd import native
from zkvm_amd.prover import GpuProver, Program, make_pub_inputs, vm_trace
from zkvm_amd.workloads import LR_PROGRAM, LweParameters, make_workload, ops_for_trace_len

pytestmark = pytest.mark.gpu
P = 2**128 - 45 * 2**40 + 1
MAX_N = 1 << 16


@pytest.fixture(scope="module")
def gpu():
    assert native.device_count() > 0, "no GPU visible"
    g = GpuProver(0, max_trace_len=MAX_N)
    yield g
    g.close()


@pytest.fixture(scope="module")
def lr_pub():
    return workload_trace(LR_PROGRAM, seed=2)[1]


@pytest.fixture(scope="module")
def valid128():
    return valid_trace_128()


def check(gpu, oracle, trace, pub, via="device", steps=None):
    """Validate `trace` on the GPU and compare status, report and message with the reference; returns the report."""
    want = reference_report(oracle, trace, pub, steps=steps)
    if via == "device":
        d, n = gpu.upload_trace(trace)
        rc, got = gpu.validate_device(d, n, pub)
    else:
        rc, got = gpu.validate_host(trace, pub)
    msg = native.lib().zk_last_error().decode()
    for key in want:
        assert got[key] == want[key], f"report field {key}: got {got[key]}, want {want[key]}"
    assert set(got) == set(want)
    assert rc == reference_rc(want)
    if rc != ZK_OK:
        assert msg == reference_message(want)
    assert gpu.validation() == got
    return got


def vm_workload(src, seed, params=None):
    w = make_workload(src, seed=seed, params=params) if params is not None else make_workload(src, seed=seed)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    return trace, make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta), w


VALID = [("one_op", "push.1\n", 64, None), ("lr", LR_PROGRAM, None, None),
         ("pushadd12", ops_for_trace_len(12, "pushadd"), 1 << 12, None),
         ("cipher13_lwe5", ops_for_trace_len(13), 1 << 13, None),
         ("pushadd12_lwe3", ops_for_trace_len(12, "pushadd"), 1 << 12, LweParameters(k=2))]


@pytest.mark.parametrize("via", ["device", "host"])
@pytest.mark.parametrize("name,src,want_n,params", VALID, ids=[v[0] for v in VALID])
def test_valid_traces(gpu, oracle, name, src, want_n, params, via):
    trace, pub, _ = vm_workload(src, 5, params)
    if want_n is not None:
        assert trace.shape[1] == want_n
    if params is not None:
        assert pub.lwe_size == 3
    rep = check(gpu, oracle, trace, pub, via=via)
    assert rep["first_kind"] == 0 and rep["failing_steps"] == 0 and rep["a_mask"] == 0
    assert rep["t_count"] == [0] * 20 and rep["t_first"] == [2**64 - 1] * 20 and rep["t_value"] == [0] * 20


@pytest.mark.parametrize("via", ["device", "host"])
def test_cipher_trace_at_another_lwe_size(gpu, oracle, via):
    """ops_for_trace_len(13) run by the VM at lwe_size 3.  ProcessorAir fixes the lwe_size-5 geometry in two
    constraints whatever the server key says -- enforce_stack_depth moves the depth by 4 for read2 / add2
    (constrains.rs:103-105) and enforce_read2 reads stack_item_next(5) (constrains.rs:174-175) -- so the VM's trace of a
    read2 program at any other lwe_size breaks exactly those two (1 and 10) at its read2 / add2 steps and nothing else,
    in the reference validator as on the GPU.  (A valid trace at lwe_size 3 is test_valid_traces' push/add one.)"""
    trace, pub, _ = vm_workload(ops_for_trace_len(13), 5, LweParameters(k=2))
    assert trace.shape[1] == 1 << 13 and pub.lwe_size == 3
    rep = check(gpu, oracle, trace, pub, via=via)
    assert rep["first_kind"] == 2 and rep["a_mask"] == 0
    assert [k for k in range(20) if rep["t_count"][k]] == [1, 10]


@pytest.mark.parametrize("lwe_size", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [16, 64, 256, 512, 8192])
def test_random_traces(gpu, oracle, lr_pub, n, lwe_size):
    rep = check(gpu, oracle, random_trace(n, 17 * n + lwe_size), with_lwe_size(lr_pub, lwe_size))
    # a random frame satisfies nothing: every step fails (the constraints with several random factors at every step)
    assert rep["failing_steps"] == n - 2 and rep["t_count"][0] == n - 2 and rep["first_kind"] == 1


@pytest.mark.parametrize("lwe_size", [1, 5])
def test_constant_columns(gpu, oracle, lr_pub, lwe_size):
    pub = with_lwe_size(lr_pub, lwe_size)
    for shift in range(len(CONSTS)):
        check(gpu, oracle, constant_trace(64, [CONSTS[(c + shift) % len(CONSTS)] for c in range(28)]), pub)
    for v in (0, 1, P - 1):
        check(gpu, oracle, constant_trace(64, [v] * 28), pub)


@pytest.mark.parametrize("col", range(28))
def test_single_cell_corruptions(gpu, oracle, valid128, col):
    trace, pub = valid128
    n = trace.shape[1]
    for delta in (1, 2) if col in BIT_COLS else (1,):
        for row in corruption_rows(n):
            rep = check(gpu, oracle, add_to_cell(trace, col, row, delta), pub)  # the reference over the whole trace
            if row == n - 1:
                assert rep["first_kind"] == 0  # the last row is never constrained


def test_localisation_at_size(gpu, oracle):
    trace, pub, _ = vm_workload(ops_for_trace_len(16), 8)
    n = trace.shape[1]
    assert n == MAX_N
    # the unchanged trace holds at every step (the reference over the whole trace, once: 11 s less than the oracle's
    # proof of it), so the reports of the changed traces need the steps next to the changed cell only
    assert reference_report(oracle, trace, pub)["first_kind"] == 0
    # (column, row): the clock breaks constraint 0 in both frames that hold the cell; row n - 2 in an asserted column
    cells = [(0, 1), (0, 64 * 331), (12, 64 * 331 + 63), (0, 256 * 77), (12, 256 * 77 - 1), (0, n - 3), (12, n - 2)]
    for col, row in cells:
        rep = check(gpu, oracle, add_to_cell(trace, col, row, 1), pub, steps=neighbour_steps([row]))
        assert rep["first_kind"] != 0
        if rep["first_kind"] == 2:
            assert rep["first_step"] in (row - 1, row)
    rep = check(gpu, oracle, add_to_cell(trace, 12, n - 2, 1), pub, steps=neighbour_steps([n - 2]))
    assert rep["first_kind"] == 1 and rep["a_step"][rep["first_index"]] == n - 2 and rep["a_col"][rep["first_index"]] == 12
    check(gpu, oracle, add_to_cell(trace, 12, n - 1, 1), pub, steps=neighbour_steps([n - 1]))  # still valid


def test_validate_switch(gpu, oracle):
    src = ops_for_trace_len(8)
    trace, pub, w = vm_workload(src, 9)
    n = trace.shape[1]
    opub = oracle_pub(oracle, pub)
    oproof = oracle.prove(trace, opub)[0]
    prog = Program(src)
    inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
    bad = add_to_cell(trace, 12, 3, 1)
    want_bad = reference_report(oracle, bad, pub)
    assert want_bad["first_kind"] == 2
    try:
        gpu.set_validate(False)
        for _ in range(3):  # warm: the host-trace hints of this program are learned
            assert gpu.prove_host(trace, pub)[0] == oproof
        off = {"device": gpu.prove_device(*gpu.upload_trace(trace), pub)[0], "host": gpu.prove_host(trace, pub)[0],
               "vm": prog.prove_device(gpu, inputs, last_row=w.last_row)[2]}
        gpu.set_validate(True)
        on = {"device": gpu.prove_device(*gpu.upload_trace(trace), pub)[0], "host": gpu.prove_host(trace, pub)[0],
              "vm": prog.prove_device(gpu, inputs, last_row=w.last_row)[2]}
        for k in off:
            assert on[k] == off[k] == oproof, k
        assert gpu.validation()["first_kind"] == 0
        # a corrupted trace is refused before the proof: no bytes, the report kept, no hint or snapshot state moved
        info = gpu.proof_info()
        proof, _, _, rc = gpu.prove_host(bad, pub, allow_trace_error=True)
        assert rc == native.ZK_ERR_TRACE == ZK_ERR_TRACE and proof == b""
        assert native.lib().zk_last_error().decode() == reference_message(want_bad)
        assert gpu.validation() == want_bad
        proof, _, _, rc = gpu.prove_device(*gpu.upload_trace(bad), pub, allow_trace_error=True)
        assert rc == native.ZK_ERR_TRACE and proof == b"" and gpu.validation() == want_bad
        assert gpu.proof_info() == info
        # off again: the same trace runs the whole proof and ends in the degree check, as before
        gpu.set_validate(False)
        assert gpu.prove_device(*gpu.upload_trace(bad), pub, allow_degree_error=True)[3] == native.ZK_ERR_DEGREE
        assert gpu.prove_host(bad, pub, allow_degree_error=True)[3] == native.ZK_ERR_DEGREE
        assert gpu.prove_host(trace, pub)[0] == oproof
    finally:
        gpu.set_validate(False)
        prog.close()


def test_refusals(gpu, lr_pub):
    """Refused on the host, before any launch: ZK_ERR_INVALID_ARG each."""
    L = native.lib()
    d = gpu.trace_buffer()
    v = native.Validation()
    cols = (C.c_void_p * 28)(*([d] * 28))
    bad = native.ZK_ERR_INVALID_ARG
    pub = lr_pub
    for n in (24, 2 * MAX_N):
        assert L.zk_validate_device(gpu.handle, d, n, C.byref(pub), C.byref(v)) == bad
        assert L.zk_last_error().decode() == "trace length must be a power of two in [16, max_trace_len]"
        assert L.zk_validate_columns(gpu.handle, cols, n, C.byref(pub), C.byref(v)) == bad
    for lwe_size in (0, 6):
        q = with_lwe_size(pub, lwe_size)
        assert L.zk_validate_device(gpu.handle, d, 64, C.byref(q), C.byref(v)) == bad
        assert L.zk_last_error().decode().startswith("lwe_size must be in [1, 5]")
        assert L.zk_validate_columns(gpu.handle, cols, 64, C.byref(q), C.byref(v)) == bad
    assert L.zk_validate_device(gpu.handle, d, 64, C.byref(pub), None) == bad
    assert L.zk_validate_columns(gpu.handle, cols, 64, C.byref(pub), None) == bad
    h = C.c_void_p()
    native.check(L.zk_prover_create_shard(0, 64, 2, C.byref(h)), "zk_prover_create_shard")
    try:
        sd = C.c_void_p()
        native.check(L.zk_prover_trace_buffer(h, C.byref(sd)))
        assert L.zk_validate_device(h, sd, 64, C.byref(pub), C.byref(v)) == bad
        assert "sharded" in L.zk_last_error().decode()
        scols = (C.c_void_p * 28)(*([sd.value] * 28))
        assert L.zk_validate_columns(h, scols, 64, C.byref(pub), C.byref(v)) == bad
    finally:
        L.zk_prover_destroy(h)
