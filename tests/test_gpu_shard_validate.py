"""Trace::validate for sharded proofs (zk_prover_set_validate on the ranks' provers; kernels.hip k_validate_window).

  * The window kernel alone (zkvm_amd.shard_diag.validate_window): one changed cell in a valid VM trace at every place where a
    window's indexing can go wrong, each window's partial report compared with tests/validate_ref.py restricted to the
    steps next to the change that lie in the window; both ways the rows reach the kernel (in place with ld = n, as a
    device trace; only the window's rows with ld = count + 1, as a host trace's upload).
  * The union of G windows, merged by the pure rule (shard_diag.merge_validation), against the whole-trace launch
    (zk_validate_columns on a full prover, itself pinned against validate_ref.py by tests/test_gpu_validate.py).
  * The whole path through the loopback communicator: with the switch on a valid trace gives the golden / single-GPU
    proof bytes and a broken one ZK_ERR_TRACE with the single-GPU text and report on every rank's prover, no proof
    bytes and no data collective; with it off the same trace ends in ZK_ERR_DEGREE.
Integers, bytes and strings throughout: every comparison is exact.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from test_gpu_eval_frames import random_trace
from test_sharded import CASES, case_inputs
from test_validate_cpu import valid_trace_128
from validate_ref import ZK_ERR_TRACE, ZK_OK, add_to_cell, neighbour_steps, reference_report
from zkvm_amd import native, shard_diag
from zkvm_amd.prover import GpuProver, ProofOptions, make_pub_inputs, vm_trace
from zkvm_amd.sharded import ShardedProver
from zkvm_amd.workloads import make_workload, ops_for_trace_len

pytestmark = pytest.mark.gpu
ROW0, LAST = native.ASSERT_ROW0, native.ASSERT_LAST


def vm_case(log_n):
    src = ops_for_trace_len(log_n, "pushadd")
    w = make_workload(src, seed=40 + log_n)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    assert trace.shape[1] == 1 << log_n
    return trace, make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)


@pytest.fixture(scope="module")
def traces():
    assert native.device_count() > 0, "no GPU visible"
    t = {128: valid_trace_128()}
    for log_n in (9, 10, 11, 12):
        t[1 << log_n] = vm_case(log_n)
    return t


@pytest.fixture(scope="module")
def full():
    g = GpuProver(0, max_trace_len=1 << 12)
    yield g
    g.close()


def amask_of(n, first, count):
    return (ROW0 if first == 0 else 0) | (LAST if first + count == n - 2 else 0)


def tile(n, w, j):
    """Window j of a trace split into windows of w steps (the last one ends at step n - 3)."""
    first = j * w
    return first, min(first + w, n - 2) - first


def run_window(trace, pub, first, count, amask, packed):
    rc, p = shard_diag.validate_window(trace, pub, first, count, amask, packed)
    assert rc == ZK_OK, native.lib().zk_last_error().decode()
    return p


def check_window(oracle, trace, pub, rows, first, count, amask=None, packed=(0, 1)):
    """The window's partial against the reference restricted to the steps next to the changed `rows` in the window."""
    n = trace.shape[1]
    amask = amask_of(n, first, count) if amask is None else amask
    steps = [s for s in neighbour_steps(rows) if first <= s < first + count]
    want = reference_report(oracle, trace, pub, steps=steps)
    el = lambda b, k: int.from_bytes(bytes(b[16 * k:16 * k + 16]), "little")  # noqa: E731
    for pk in packed:
        p = run_window(trace, pub, first, count, amask, pk)
        assert (p.version, p.status, p.first, p.count, p.amask) == (native.AGREE_VERSION, ZK_OK, first, count, amask)
        assert p.failing_steps == want["failing_steps"], (first, count, pk)
        assert list(p.t_count) == want["t_count"] and list(p.t_first) == want["t_first"], (first, count, pk)
        assert [el(p.t_value, k) for k in range(20)] == want["t_value"]
        assert p.a_mask == want["a_mask"] & amask
        for k in range(22):
            if (amask >> k) & 1:
                assert el(p.a_found, k) == want["a_found"][k]
    return want


SIZES = [(n, w) for n in (128, 1024, 4096) for w in (8, 64, 256, 1024) if 2 * w <= n]


@pytest.mark.parametrize("n,w", SIZES, ids=[f"n{n}-w{w}" for n, w in SIZES])
def test_window_edges(oracle, traces, n, w):
    trace, pub = traces[n]
    nw = n // w
    # a valid trace: nothing is reported, by the first, a middle and the last window
    for j in (0, nw // 2, nw - 1):
        rep = check_window(oracle, trace, pub, (), *tile(n, w, j))
        assert rep["failing_steps"] == 0 and rep["a_mask"] == 0
    # step 0: the clock cell of row 0 is an asserted cell and the frame of step 0
    t = add_to_cell(trace, 0, 0, 1)
    rep = check_window(oracle, t, pub, (0,), *tile(n, w, 0))
    assert rep["a_mask"] == 1 and rep["t_count"][0] == 1 and rep["t_first"][0] == 0
    # ... with the assertion mask off the broken row-0 cell is not reported, the step is
    p = run_window(t, pub, *tile(n, w, 0), 0, 0)
    assert p.a_mask == 0 and p.failing_steps == 1 and p.t_first[0] == 0
    check_window(oracle, t, pub, (0,), *tile(n, w, 0), amask=0)
    # the first row of a window: the last step of the window before it (its frame reads that row) and the first step
    # of this one; j = 1 and a j whose first step is no multiple of 256 (w < 256)
    for j in sorted({1, min(3, nw - 1), nw - 1}):
        r = j * w
        t = add_to_cell(trace, 0, r, 1)
        before = check_window(oracle, t, pub, (r,), *tile(n, w, j - 1))
        after = check_window(oracle, t, pub, (r,), *tile(n, w, j))
        assert before["t_first"][0] == r - 1 and before["t_count"][0] == 1
        if r < n - 2:
            assert after["t_first"][0] == r and after["t_count"][0] == 1
        # a window further on sees nothing of it
        if j + 1 < nw:
            assert check_window(oracle, t, pub, (r,), *tile(n, w, j + 1))["failing_steps"] == 0
    # the end of the range, in the last window: step n - 3, row n - 2 (the `next` of step n - 3, and an asserted cell),
    # row n - 1 (never read)
    last = tile(n, w, nw - 1)
    assert last[0] + last[1] == n - 2
    rep = check_window(oracle, add_to_cell(trace, 0, n - 3, 1), pub, (n - 3,), *last)
    assert rep["t_count"][0] == 2 and rep["t_first"][0] == n - 4
    rep = check_window(oracle, add_to_cell(trace, 0, n - 2, 1), pub, (n - 2,), *last)
    assert rep["t_count"][0] == 1 and rep["t_first"][0] == n - 3 and rep["a_mask"] == 0
    rep = check_window(oracle, add_to_cell(trace, 12, n - 2, 1), pub, (n - 2,), *last)
    assert rep["a_mask"] == 1 << 7
    p = run_window(add_to_cell(trace, 12, n - 2, 1), pub, *last, 0, 1)
    assert p.a_mask == 0
    rep = check_window(oracle, add_to_cell(trace, 0, n - 1, 1), pub, (n - 1,), *last)
    assert rep["failing_steps"] == 0 and rep["a_mask"] == 0


@pytest.mark.parametrize("n,first,count", [(1024, 100, 600), (4096, 100, 600), (4096, 1000, 3094), (128, 9, 117)])
def test_lane_and_block_boundaries_in_an_unaligned_window(oracle, traces, n, first, count):
    """A window whose first step is no multiple of 64 or 256: the wave and block boundaries of the launch fall at
    local steps 64 k, not at global ones, and the reported steps must be global all the same."""
    trace, pub = traces[n]
    for local in (64, 256, 512):
        if local >= count:
            continue
        r = first + local  # breaks local steps local - 1 (the last lane of a wave / thread of a block) and local
        rep = check_window(oracle, add_to_cell(trace, 0, r, 1), pub, (r,), first, count)
        assert rep["t_count"][0] == 2 and rep["t_first"][0] == r - 1
    # several at once: the lowest wins across waves and blocks, the counts add
    rows = [first + k for k in (3, 64, 256) if k < count]
    t = trace
    for r in rows:
        t = add_to_cell(t, 0, r, 1)
    rep = check_window(oracle, t, pub, rows, first, count)
    assert rep["t_count"][0] == 2 * len(rows) and rep["t_first"][0] == first + 2


def merged(trace, pub, G, packed):
    n = trace.shape[1]
    parts = []
    for g in range(G):
        parts.append(run_window(trace, pub, *shard_diag.val_window(n, g, G), packed))
    return shard_diag.merge_validation(parts, n, pub)


@pytest.mark.parametrize("G", [2, 4, 8])
def test_union_of_windows_equals_the_whole_trace_launch(traces, full, G):
    trace, pub = traces[1024]
    n = 1024
    broken = trace
    for col, row in ((0, 7), (0, n // G), (13, n // 2 - 1), (5, n // 2), (7, 700), (0, n - 3), (14, n - 2)):
        broken = add_to_cell(broken, col, row, 1)
    for t in (trace, broken, add_to_cell(trace, 0, 0, 1), random_trace(64, 5), random_trace(4096, 6)):
        rc0, want = full.validate_host(t, pub)
        msg0 = native.lib().zk_last_error().decode()
        for packed in (0, 1):
            rc, got, msg = merged(t, pub, G, packed)
            assert got == want and rc == rc0
            if rc != ZK_OK:
                assert msg == msg0


# ---------------------------------------------------------------- the whole path, loopback
def lr_case():
    c = next(c for c in CASES if c["name"] == "lr")
    return case_inputs(c)


def prove_raw(sp, trace, pub, opts, n=0):
    """zk_prove_sharded -> (rc, proof bytes, proof_len, zk_last_error)."""
    L = native.lib()
    if trace is not None:
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        n = trace.shape[1]
    opt = opts.to_c()
    buf = C.create_string_buffer(1 << 20)
    plen = C.c_size_t(len(buf))
    arr = (C.c_void_p * len(sp.provers))(*[p.value for p in sp.provers])
    rc = L.zk_prove_sharded(sp.comm, arr, len(sp.provers), trace.ctypes.data if trace is not None else None, n,
                            C.byref(opt), C.byref(pub), buf, C.byref(plen), None)
    return rc, buf.raw[:plen.value], plen.value, L.zk_last_error().decode()


DATA = ("trace_coeffs", "column_flags", "trace_digests", "trace_roots", "comp_slices", "comp_columns", "degree_flags",
        "comp_digests", "comp_roots", "ood_parts", "deep_totals", "deep_slices", "fri0_digests", "fri0_roots",
        "fri_layer1", "openings")
WHOLE = [("lr", 2), (512, 8), (2048, 4)]


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("which,G", WHOLE, ids=[f"{w}-G{g}" for w, g in WHOLE])
def test_sharded_proof_validates_first(traces, full, which, G, source):
    if which == "lr":
        trace, want_proof, pub, opts = lr_case()
    else:
        trace, pub = traces[which]
        opts = ProofOptions()
        want_proof, _, _, rc = full.prove(trace, pub, opts)
        assert rc == ZK_OK
    n = trace.shape[1]
    w = n // G  # rank g's window starts at row g w
    sp = ShardedProver.loopback(G, max_trace_len=n)
    try:
        def run(t):
            if source == "host":
                return prove_raw(sp, t, pub, opts)
            return prove_raw(sp, None, pub, opts, n=sp.upload_trace(t))

        # switch off: a broken trace costs a whole proof and ends in ZK_ERR_DEGREE, as before
        bad = add_to_cell(trace, 0, w, 1)
        rc, _, _, _ = run(bad)
        assert rc == native.ZK_ERR_DEGREE
        a = sp.agreement()
        assert a["code"] == ZK_OK and a["validate"] == 0 and a["control_calls"] == 1 and a["control_bytes"] == 256 * (G - 1)
        # on at ONE rank's prover: the ranks agree to validate (OR)
        native.check(native.lib().zk_prover_set_validate(sp.provers[G - 1], 1))
        rc, proof, _, msg = run(trace)
        assert rc == ZK_OK, msg
        assert proof == want_proof
        a = sp.agreement()
        assert a["validate"] == 1 and a["control_calls"] == 2
        stats = sp.exchange_stats()
        assert stats["control"][2] == 1 and stats["validate_report"][2] == 1 and stats["openings"][2] >= 1
        assert all(sp.validation(l)["first_kind"] == 0 for l in range(G))
        cells = [(0, 0), (0, w - 1), (0, w), (0, n - 3), (12, n - 2), (0, n // 2 + 3)]
        for col, row in cells:
            t = add_to_cell(trace, col, row, 1)
            rc0, want = full.validate_host(t, pub)
            msg0 = native.lib().zk_last_error().decode()
            assert rc0 == ZK_ERR_TRACE
            rc, proof, plen, msg = run(t)
            assert rc == ZK_ERR_TRACE and msg == msg0 and plen == 0 and proof == b""
            for l in range(G):
                assert sp.validation(l) == want
            stats = sp.exchange_stats()
            assert set(stats) == {"control", "validate_report"} and not set(stats) & set(DATA)
            assert stats["control"][2] == 1 and stats["validate_report"][2] == 1
        # row n - 1 is never constrained: the trace is valid and proves
        t = add_to_cell(trace, 0, n - 1, 1)
        single, _, _, rc = full.prove(t, pub, opts)
        assert rc == ZK_OK
        rc, proof, _, msg = run(t)
        assert rc == ZK_OK and proof == single
        # the provers stay usable: the valid trace again
        rc, proof, _, _ = run(trace)
        assert rc == ZK_OK and hashlib.sha256(proof).digest() == hashlib.sha256(want_proof).digest()
    finally:
        sp.close()


def test_vm_prove_sharded_validates_the_written_trace():
    """zk_vm_prove_sharded with the switch on takes the all-columns trace source on every rank and validates it."""
    from zkvm_amd.prover import Program
    src = ops_for_trace_len(10, "pushadd")
    w = make_workload(src, seed=50)
    prog = Program(src)
    sp = ShardedProver.loopback(4, max_trace_len=1 << 10)
    try:
        inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
        _, _, plain = sp.prove_program(prog, inputs, w.last_row, ProofOptions())
        assert sp.agreement()["validate"] == 0
        sp.set_validate(True)
        _, _, proof = sp.prove_program(prog, inputs, w.last_row, ProofOptions())
        a = sp.agreement()
        assert proof == plain and a["validate"] == 1 and a["control_calls"] == 2
        assert sp.validation(3)["first_kind"] == 0 and sp.validation(0)["trace_len"] == 1 << 10
    finally:
        sp.close()
        prog.close()
