"""Trace validation, the parts that need no GPU.

  * the reference validator (tests/validate_ref.py, over the CPU oracle) on a valid trace: clean over the steps
    0 .. n - 3, and step n - 2 alone -- the frame that reaches into the random last row -- fails, so a validator whose
    range is one step too long is caught even on valid traces;
  * the single-cell corruption set tests/test_gpu_validate.py runs on the GPU reaches every one of the 20 transition
    constraints and every one of the 22 assertions, so that set cannot silently stop covering one;
  * the ctypes binding: native.Validation has the size and field offsets of include/zkvm_gpu.h's zk_validation, and
    the built library exports the four new entry points.
"""
import ctypes as C
import re
from pathlib import Path

import pytest

from validate_ref import NUM_ASSERTS, NUM_TCONS, StepEvaluator, add_to_cell, neighbour_steps, reference_report
from zkvm_amd import native
from zkvm_amd.prover import make_pub_inputs, vm_trace
from zkvm_amd.workloads import cipher_mix_program, make_workload

ROOT = Path(__file__).resolve().parent.parent
BIT_COLS = (1, 2, 3, 4, 5)


def corruption_rows(n):
    """Rows 0, 1, 14, 15, 16, 17, n - 3, n - 2, n - 1 (the first rows, the hash cycle's boundary, the last steps and
    the unconstrained last row) hold read2, read, push and noop steps only on this trace, and no single-cell change
    there makes is_sadd, is_add2, is_mul or is_smul non-zero (each needs two non-zero opcode bits with b0 != 1): they
    reach 16 of the 20 constraints.  Rows 2 (smul), 6 (add2), 8 (sadd) and 25 (mul) are added for constraints 7, 5,
    4 and 6."""
    return (0, 1, 14, 15, 16, 17, n - 3, n - 2, n - 1, 2, 6, 8, 25)


def corruption_set(n):
    """(column, row, delta): every column at the rows above with + 1, the opcode-bit columns with + 2 as well."""
    cases = [(c, r, 1) for c in range(28) for r in corruption_rows(n)]
    cases += [(c, r, 2) for c in BIT_COLS for r in corruption_rows(n)]
    return cases


def valid_trace_128():
    src = cipher_mix_program(1)[0]
    w = make_workload(src, seed=3)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    assert trace.shape == (28, 128, 2) and w.server_key.lwe_size() == 5
    return trace, make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)


@pytest.fixture(scope="module")
def valid():
    return valid_trace_128()


def test_valid_trace_is_clean_and_the_step_past_the_range_fails(oracle, valid):
    trace, pub = valid
    n = trace.shape[1]
    rep = reference_report(oracle, trace, pub)
    assert rep["first_kind"] == 0 and rep["first_index"] == -1 and rep["failing_steps"] == 0
    assert rep["a_mask"] == 0 and rep["a_failed"] == 0 and rep["a_found"] == rep["a_expected"]
    assert rep["t_count"] == [0] * NUM_TCONS and rep["steps_checked"] == n - 2
    # the frame (n - 2, n - 1) reads the random last row
    vals = StepEvaluator(oracle, trace, pub)(n - 2)
    assert sum(1 for v in vals if v) == 3, [k for k, v in enumerate(vals) if v]


def test_corruption_set_reaches_every_constraint_and_assertion(oracle, valid):
    trace, pub = valid
    n = trace.shape[1]
    tcons, asserts = set(), set()
    for col, row, delta in corruption_set(n):
        rep = reference_report(oracle, add_to_cell(trace, col, row, delta), pub, steps=neighbour_steps([row]))
        tcons |= {k for k in range(NUM_TCONS) if rep["t_count"][k]}
        asserts |= {k for k in range(NUM_ASSERTS) if (rep["a_mask"] >> k) & 1}
        if row == n - 1:
            assert rep["first_kind"] == 0, (col, row, delta)  # the last row is never constrained
    assert tcons == set(range(NUM_TCONS)), sorted(set(range(NUM_TCONS)) - tcons)
    assert asserts == set(range(NUM_ASSERTS)), sorted(set(range(NUM_ASSERTS)) - asserts)


def header_constant(name):
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    return int(re.search(rf"#define\s+{name}\s+(-?\d+)", text).group(1))


def test_validation_binding_layout():
    """zk_validation as the C compiler lays it out (natural alignment, the header's field order and array bounds)."""
    T, A = header_constant("ZK_MAX_TCONS"), header_constant("ZK_MAX_ASSERTS")
    assert header_constant("ZK_ERR_TRACE") == native.ZK_ERR_TRACE == -21
    fields = [("trace_len", 8, 1), ("steps_checked", 8, 1), ("failing_steps", 8, 1), ("t_count", 8, T),
              ("t_first", 8, T), ("t_value", 1, 16 * T), ("a_failed", 4, 1), ("a_mask", 4, 1), ("a_col", 4, A),
              ("a_step", 8, A), ("a_expected", 1, 16 * A), ("a_found", 1, 16 * A), ("first_kind", 4, 1),
              ("first_index", 4, 1), ("first_step", 8, 1)]
    assert [f[0] for f in native.Validation._fields_] == [f[0] for f in fields]
    off = 0
    for name, size, count in fields:
        off = (off + size - 1) // size * size
        assert getattr(native.Validation, name).offset == off, name
        assert getattr(native.Validation, name).size == size * count, name
        off += size * count
    assert C.sizeof(native.Validation) == (off + 7) // 8 * 8
    assert native.Validation.NUM_TCONS == NUM_TCONS <= T and native.Validation.NUM_ASSERTS == NUM_ASSERTS <= A


def test_library_exports_the_validation_entry_points():
    L = native.lib()
    for name in ("zk_validate_device", "zk_validate_columns", "zk_prover_set_validate", "zk_prover_validation"):
        assert hasattr(L, name), name
        assert name in native.EXPORTED
    # null arguments are refused before any device is touched
    v = native.Validation()
    assert L.zk_validate_device(None, None, 16, None, C.byref(v)) == native.ZK_ERR_INVALID_ARG
    assert L.zk_validate_columns(None, None, 16, None, C.byref(v)) == native.ZK_ERR_INVALID_ARG
    assert L.zk_prover_set_validate(None, 1) == native.ZK_ERR_INVALID_ARG
    assert L.zk_prover_validation(None, C.byref(v)) == native.ZK_ERR_INVALID_ARG
