"""The bulk row reads, as far as no GPU is needed: the two entry points are declared, exported and bound with the
argument counts of their prototypes; each refuses a NULL handle before it touches a device; and the numpy permutation
that tests/test_gpu_lde_rows.py uses as the layout reference is a bijection onto its window, is the index formula of the
existing host conversion (prover.hip's coset_major_rows_to_host), and wraps at the domain's end."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from zkvm_amd import native, plug

ROOT = Path(__file__).resolve().parent.parent
NEW = ("zk_lde_read_rows", "zk_comp_read_rows")


def prototype_args(name):
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/zkvm_gpu.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound(name):
    L = native.lib()
    assert name in native.EXPORTED
    assert hasattr(L, name), f"{name} is not exported"
    args = prototype_args(name)
    assert len(args) == 4, args
    assert len(getattr(L, name).argtypes) == 4


def test_header_states_what_the_reads_leave_alone():
    text = (ROOT / "include" / "zkvm_gpu.h").read_text()
    block = text[text.index("A slice of DefaultTraceLde"):text.index("int zk_lde_read_rows")]
    for needle in ("prover/src/lib.rs:55-62", "read_main_trace_frame_into", "N + blowup", "ZK_ERR_INVALID_ARG",
                   "stay valid", "zk_commit_composition_ext(NULL)", "hint, snapshot or proof state"):
        assert needle in block, needle


def test_null_handles_are_refused_without_a_device():
    L = native.lib()
    fill = b"\x5a" * 64
    buf = C.create_string_buffer(fill, len(fill))
    for name in NEW:
        assert getattr(L, name)(None, 0, 1, buf) == native.ZK_ERR_INVALID_ARG
        assert (L.zk_last_error() or b"").decode()
    assert buf.raw == fill


def test_the_direct_call_checks_its_arguments():
    """shapes, windows and a grid cap out of range are refused before any device is opened"""
    def call(n, blowup, ncols, first, count, max_blocks=0):
        return plug.rows_layout_direct(np.zeros((max(ncols, 0) * blowup * n, 2), dtype=np.uint64), n, blowup, ncols, first,
                                       count, max_blocks)

    for args in ((0, 8, 1, 0, 1), (16, 4, 1, 0, 1), (16, 12, 1, 0, 1), (16, 128, 1, 0, 1), (16, 8, 0, 0, 1),
                 (16, 8, 29, 0, 1), (16, 8, 1, 128, 1), (16, 8, 1, 0, 0), (16, 8, 1, 0, 137), (16, 8, 1, 0, 1, (1 << 20) + 1)):
        with pytest.raises(native.ZkError) as e:
            call(*args)
        assert e.value.code == native.ZK_ERR_INVALID_ARG, args
    with pytest.raises(ValueError):
        plug.rows_layout_direct(np.zeros((8, 2), dtype=np.uint64), 16, 8, 1)  # 8 elements are not ncols blowup n


def host_conversion(h, ncols, n, B):
    """coset_major_rows_to_host's loop: o[i * ncols + c] = h[(c * B + i % B) * n + i / B]"""
    N = n * B
    o = [None] * (ncols * N)
    for c in range(ncols):
        for i in range(N):
            o[i * ncols + c] = h[(c * B + (i % B)) * n + i // B]
    return o


@pytest.mark.parametrize("n,B,ncols", [(16, 8, 28), (64, 16, 7)])
def test_permutation_is_the_host_conversions_formula(n, B, ncols):
    N = n * B
    perm = plug.rows_natural_order(n, B, ncols)
    assert perm.shape == (N, ncols)
    assert perm.reshape(-1).tolist() == host_conversion(list(range(ncols * N)), ncols, n, B)
    assert sorted(perm.reshape(-1).tolist()) == list(range(ncols * N))
    # a window is those rows of it, and a bijection onto their elements
    for first, count in ((0, N), (1, 1), (37, 200), (N - 3, 3 + B), (N - 1, N + B)):
        win = plug.rows_natural_order(n, B, ncols, first, count)
        rows = (first + np.arange(count)) % N
        assert np.array_equal(win, perm[rows])
        inside = win[:min(count, N)].reshape(-1).tolist()
        assert len(set(inside)) == len(inside)
        want = {(c * B + i % B) * n + i // B for i in rows[:N].tolist() for c in range(ncols)}
        assert set(inside) == want


def test_permutation_wraps_at_the_last_row():
    n, B, ncols = 16, 8, 3
    N = n * B
    win = plug.rows_natural_order(n, B, ncols, N - 1, 3)
    # row N - 1 is coset B - 1, i div B = n - 1; then rows 0 and 1: cosets 0 and 1 at i div B = 0
    assert win.tolist() == [[(c * B + B - 1) * n + n - 1 for c in range(ncols)], [c * B * n for c in range(ncols)],
                            [(c * B + 1) * n for c in range(ncols)]]
