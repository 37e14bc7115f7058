"""Transition constraint degrees, the parts that need no GPU.

  * the reference of tests/degrees_ref.py (winterfell 0.9's validate_transition_degrees over the CPU oracle) on the
    committed goldens `lr` (n = 128) and `pushadd12` (n = 256): the actual degrees equal the declared ones exactly --
    the anchor of the recollected semantics, the reference's own example meets its own declaration;
  * the closed form of a push/add trace whose last row is zero, or a copy of row n - 2, at n = 64 and 256 (the GPU
    tests of the two NTT regimes compare with it where the reference would take too long);
  * one changed cell of a valid trace makes one quotient a non-polynomial: constraint 11 alone, at 8n - 1;
  * the ctypes binding: native.Degrees has the size and field offsets a C compiler gives include/zkvm_gpu.h's struct
    (a tiny host program compiled from the header), and the entry points refuse NULL arguments without a GPU.
"""
import ctypes as C
import json
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from degrees_ref import (NUM_TCONS, ZK_ERR_DEGREES, ZK_OK, expected, message, pushadd_trace, pushadd_zero_last_row,
                         reference, reference_rc)
from test_golden import CASES, load_case
from validate_ref import add_to_cell
from zkvm_amd import native

ROOT = Path(__file__).resolve().parent.parent
E128 = [1, 509, 128, 636, 636, 636, 763, 763, 636, 636, 636, 636, 502, 883, 502, 502, 248, 248, 248, 248]


def golden(name):
    c = next(c for c in CASES if c["name"] == name)
    trace, proof, pub = load_case(c)
    return trace, proof, pub, c


def test_expected_degrees():
    assert expected(128) == E128
    assert len(expected(64)) == NUM_TCONS and max(expected(64)) < 7 * 64


@pytest.mark.parametrize("name,n", [("lr", 128), ("pushadd12", 256)])
def test_goldens_meet_the_declared_degrees(oracle, name, n):
    trace, _, pub, _ = golden(name)
    assert trace.shape[1] == n
    coeffs, rep, _ = reference(oracle, trace, pub.lwe_size, pub.delta)
    assert rep["actual"] == rep["expected"] == expected(n)
    assert rep["mismatch_mask"] == rep["zero_mask"] == rep["over_mask"] == 0
    assert rep["max_actual"] == max(expected(n)) and rep["ce_len_needed"] == 8 * n == rep["ce_len"]
    assert reference_rc(rep) == ZK_OK
    assert all(len(c) == 8 * n for c in coeffs)


@pytest.mark.parametrize("k,n", [(1, 64), (6, 256)])
@pytest.mark.parametrize("last", ["zero", "copy"])
def test_zero_last_row_pattern(oracle, k, n, last):
    trace, pub, _ = pushadd_trace(k, last)
    assert trace.shape[1] == n
    _, rep, msg = reference(oracle, trace, pub.lwe_size, pub.delta)
    assert rep["actual"] == pushadd_zero_last_row(n)
    assert rep["zero_mask"] == sum(1 << k for k in (4, 5, 6, 7, 9, 10)) and rep["over_mask"] == 0
    assert bin(rep["mismatch_mask"]).count("1") == 11
    assert reference_rc(rep) == ZK_ERR_DEGREES
    assert msg == message(rep) and msg.startswith("transition constraint degrees didn't match\nexpected: [  1, ")


def test_random_last_row_passes_and_a_changed_cell_breaks_one_quotient(oracle):
    trace, pub, _ = pushadd_trace(1, "random")
    n = trace.shape[1]
    assert n == 64
    _, rep, _ = reference(oracle, trace, pub.lwe_size, pub.delta)
    assert rep["actual"] == expected(n) and rep["mismatch_mask"] == 0
    _, rep, _ = reference(oracle, add_to_cell(trace, 12, 5, 1), pub.lwe_size, pub.delta)
    assert rep["mismatch_mask"] == rep["over_mask"] == 1 << 11 and rep["zero_mask"] == 0
    assert rep["actual"][11] == 8 * n - 1 == 511
    assert rep["ce_len_needed"] == 8 * n  # the second assertion of winterfell would still hold


def test_message_format():
    rep = {"expected": [1, 509, 128], "actual": [1, 1, 1006]}
    assert message(rep) == ("transition constraint degrees didn't match\nexpected: [  1, 509, 128]\n"
                            "actual:   [  1,   1, 1006]")


FIELDS = ["trace_len", "ce_len", "expected", "actual", "mismatch_mask", "zero_mask", "over_mask", "_pad", "max_actual",
          "ce_len_needed"]


def test_degrees_binding_layout(tmp_path):
    """zk_degrees as a C compiler lays it out: a host program compiled from the header prints sizeof and offsetof."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf(", \\"{f}\\": [%zu, %zu]", offsetof(zk_degrees, {f}), sizeof(((zk_degrees *)0)->{f}));\n'
                    for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zkvm_gpu.h"\nint main(void) {\n'
                   '    printf("{\\"sizeof\\": %zu, \\"err\\": %d", sizeof(zk_degrees), ZK_ERR_DEGREES);\n' + lines +
                   '    printf("}\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert got["err"] == native.ZK_ERR_DEGREES == ZK_ERR_DEGREES == -22
    assert [f[0] for f in native.Degrees._fields_] == FIELDS
    assert C.sizeof(native.Degrees) == got["sizeof"]
    for f in FIELDS:
        assert [getattr(native.Degrees, f).offset, getattr(native.Degrees, f).size] == got[f], f
    assert native.Degrees.NUM_TCONS == NUM_TCONS
    assert set(native.Degrees().to_dict()) == set(FIELDS) - {"_pad"}
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    assert int(re.search(r"#define\s+ZK_ERR_DEGREES\s+(-?\d+)", text).group(1)) == -22


def test_entry_points_refuse_null_arguments():
    import zkvm_amd
    assert zkvm_amd.ZK_ERR_DEGREES == -22 and zkvm_amd.Degrees is native.Degrees
    L = native.lib()
    names = ("zk_degrees_device", "zk_degrees_columns", "zk_prover_set_validate_degrees", "zk_prover_degrees")
    for name in names:
        assert hasattr(L, name), name
        assert name in native.EXPORTED
    d = native.Degrees()
    bad = native.ZK_ERR_INVALID_ARG
    assert L.zk_degrees_device(None, None, 16, None, C.byref(d), None) == bad
    assert L.zk_degrees_columns(None, None, 16, None, C.byref(d), None) == bad
    assert L.zk_prover_set_validate_degrees(None, 1) == bad
    assert L.zk_prover_degrees(None, C.byref(d)) == bad
    for m in ("degrees_device", "degrees_host", "set_validate_degrees", "degrees"):
        assert hasattr(zkvm_amd.GpuProver, m), m
