"""What the plug points cost at the benchmark size: the existing base-field calls (zk_eval_constraints,
zk_commit_composition: layout change on the host, one element at a time) against the calls over the challenge field
(zk_eval_constraints_ext, zk_commit_composition_ext: layout change by k_ce_layout, one contiguous copy per direction),
on one warm prover in one process, old and new alternating.

  * host clock around each call (every call ends in a stream synchronise); the median of `reps` calls each, with min and
    max; the output and input buffers are allocated and touched once, outside the clock;
  * ext = 1 old against new, then ext = 2;
  * the device hand-off pair (evaluate with out = NULL, commit with composition = NULL) against the stages
    "constraints" and "composition" of whole proofs of the same trace (zk_prover_stage_times; the proof evaluates 7 of
    the 8 CE cosets and adds the assertion terms in coefficient form, the plug point evaluates all 8 with them);
  * from profiled calls (zk_prover_kernel_stats): the layout kernel's device time between HIP events and the bytes it
    moves (each element read once and written once) over that time.

Usage (GPU box): python3 tools/plug_time.py [log_n] [reps]    (profiles/plug_ext_time.txt keeps one run's output)

`python3 tools/plug_time.py rows [log_n] [reps]` measures the bulk row reads instead (zk_lde_read_rows,
zk_comp_read_rows; profiles/lde_rows_time.txt), on a random trace -- an LDE costs the same whatever it extends:

  * the whole trace LDE (N x 28 x 16 B) into a page-locked buffer against a plain hipMemcpy of as many bytes from a
    device buffer of that size into the same host buffer, alternating.  The library has no call that hands out the
    address of its LDE, so the yardstick copies from an allocation of its own.  In order on one stream the read should
    cost the copy plus the layout kernel: it passes if median(read) <= median(copy) (1 + s) + kernel time, s the copy's
    own (max - min) / median, the kernel time from zk_prover_kernel_stats of profiled calls;
  * the same read into a pageable buffer;
  * 4096 consecutive frames through zk_lde_read_frame, scaled to the 8n calls an evaluator makes (extrapolated);
  * zk_comp_read_rows of an ext = 2, 8-column commitment in the same manner;
  * the layout kernel's rate (each element read once and written once, over the device time between HIP events), at
    blowup 8 and, on a prover of the same size (half the trace length), at blowup 16.
"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "encrypt-zkvm_amd"))

from zkvm_amd import native  # noqa: E402
from zkvm_amd.plug import TraceLde  # noqa: E402
from zkvm_amd.prover import GpuProver, Program, ProofOptions, make_pub_inputs  # noqa: E402
from zkvm_amd.workloads import make_workload, ops_for_trace_len  # noqa: E402

HBM_COPY_TBS = 6.29  # the measured float4 copy rate of the part (of 8.0 TB/s spec)


def clock(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def alternate(reps, calls):
    """`reps` rounds over the calls in order -> one list of times per call"""
    ts = [[] for _ in calls]
    for _ in range(reps):
        for k, call in enumerate(calls):
            ts[k].append(clock(call))
    return ts


def line(what, ts):
    print(f"{what:58s} median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  ({len(ts)} calls)")
    return statistics.median(ts)


def rand_elems(rng, *shape):
    a = rng.integers(0, 2**64, size=(*shape, 2), dtype=np.uint64)
    a[..., 1] = rng.integers(0, 2**64 - 1, size=shape, dtype=np.uint64)
    return a


def rows_main(log_n, reps):
    from zkvm_amd.plug import ConstraintCommitment

    L = native.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    D2H = 2
    n = 1 << log_n
    rng = np.random.default_rng(1)
    pub = make_pub_inputs([1, 2], list(range(16)), 5, 16)
    print(f"n = 2^{log_n}, blowup 8, {reps} calls each, read and plain copy alternating")

    def pinned(nbytes):
        p = C.c_void_p()
        native.check(L.zk_host_alloc(nbytes, C.byref(p)))
        C.memset(p, 0, nbytes)
        return p

    def measure(what, g, read, nbytes, kernel_calls=5):
        """read(pointer) fills nbytes of host memory; -> median of the page-locked read"""
        host, dev = pinned(nbytes), C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), nbytes) == 0
        pageable = np.zeros(nbytes, dtype=np.uint8)

        def copy():
            assert hip.hipMemcpy(host, dev, nbytes, D2H) == 0

        copy(), read(host.value), read(pageable.ctypes.data)  # warm
        assert C.string_at(host.value + nbytes - 4096, 4096) == pageable[-4096:].tobytes()
        tr, tc = alternate(reps, [lambda: read(host.value), copy])
        a = line(f"{what} -> page-locked, {nbytes / 1e9:.3f} GB", tr)
        b = line("plain hipMemcpy of as many bytes -> the same buffer", tc)
        g.profile(True)
        for _ in range(kernel_calls):
            read(host.value)
        ms, launches, moved = g.kernel_stats()["rows_to_natural"]
        g.profile(False)
        k = ms / kernel_calls
        s = (max(tc) - min(tc)) / b
        bound = b * (1 + s) + k
        print(f"    read {nbytes / a / 1e6:.2f} GB/s, copy {nbytes / b / 1e6:.2f} GB/s; rows_to_natural {k:.4f} ms a call "
              f"({launches // kernel_calls} launch(es)), {moved / ms / 1e9:.3f} TB/s (HBM copy rate {HBM_COPY_TBS} TB/s)")
        print(f"    median(read) {a:.3f} ms {'<=' if a <= bound else '>'} median(copy) (1 + s) + kernel = "
              f"{b:.3f} x (1 + {s:.4f}) + {k:.4f} = {bound:.3f} ms: {'passes' if a <= bound else 'DOES NOT PASS'}")
        line(f"{what} -> pageable", alternate(reps, [lambda: read(pageable.ctypes.data)])[0])
        hip.hipFree(dev)
        L.zk_host_free(host)
        return a

    g = GpuProver(0, max_trace_len=n)
    trace = rand_elems(rng, 28, n)
    with TraceLde.new(g, trace, 8) as lde:
        N = 8 * n
        bulk = measure("zk_lde_read_rows, whole trace LDE", g,
                       lambda p: native.check(L.zk_lde_read_rows(lde.handle, 0, N, p)), N * 28 * 16)
        cur, nxt = C.create_string_buffer(28 * 16), C.create_string_buffer(28 * 16)
        lde.read_frame(0)

        def frames():
            for step in range(4096):
                native.check(L.zk_lde_read_frame(lde.handle, step, cur, nxt))

        f = line("zk_lde_read_frame, 4096 consecutive frames", alternate(reps, [frames])[0])
        print(f"    {f / 4096 * 1e3:.2f} us a frame; extrapolated to the 8n = {N} frames of an evaluator: {f / 4096 * N / 1e3:.1f} s, "
              f"{f / 4096 * N / bulk:.0f} times the bulk read")
        ct, cb = rand_elems(rng, 20, 2), rand_elems(rng, 22, 2)
        lde.evaluate(pub, ct, cb, ext=2, keep_on_device=True)
        with ConstraintCommitment.commit(lde, None, ext=2, num_cols=8) as cc:
            measure("zk_comp_read_rows, ext = 2, 8 columns", g,
                    lambda p: native.check(L.zk_comp_read_rows(cc.handle, 0, N, p)), N * 16 * 16)
    g.close()

    # blowup 16 at half the trace length: the same N, the plane-side runs half as long, two chunks through the staging
    g = GpuProver(0, max_trace_len=n // 2, max_blowup=16)
    with TraceLde.new(g, np.ascontiguousarray(trace[:, :n // 2]), 16) as lde:
        host = pinned(N * 28 * 16)
        g.profile(True)
        for _ in range(5):
            native.check(L.zk_lde_read_rows(lde.handle, 0, N, host))
        ms, launches, moved = g.kernel_stats()["rows_to_natural"]
        g.profile(False)
        print(f"n = 2^{log_n - 1}, blowup 16: rows_to_natural {ms / 5:.4f} ms a call ({launches // 5} launches), "
              f"{moved / ms / 1e9:.3f} TB/s")
        L.zk_host_free(host)
    g.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rows":
        return rows_main(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 11)
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    L = native.lib()
    src = ops_for_trace_len(log_n, "cipher")
    w = make_workload(src, seed=1000)
    prog = Program(src)
    trace, outputs = prog.trace(w.public, w.secret, w.server_key, w.last_row)[:2]
    n = trace.shape[1]
    pub = make_pub_inputs(prog.hash, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    g = GpuProver(0, max_trace_len=n)
    print(f"n = 2^{log_n}, blowup 8, {reps} calls each, old and new alternating")

    stages = {}
    for ext in (1, 2):
        opts = ProofOptions(field_extension=ext)
        for _ in range(3):  # (the third proof runs with the learned column classes, like the benchmark's)
            assert g.prove(trace, pub, opts)[3] == 0
        stages[ext] = g.stage_times()

    rng = np.random.default_rng(1)
    ct, cb = rand_elems(rng, 20, 2), rand_elems(rng, 22, 2)
    ct1, cb1 = np.ascontiguousarray(ct[:, 0]), np.ascontiguousarray(cb[:, 0])
    out1, new1 = np.zeros((8 * n, 2), dtype=np.uint64), np.zeros((8 * n, 2), dtype=np.uint64)
    out2 = np.zeros((8 * n, 2, 2), dtype=np.uint64)
    root, cc = C.create_string_buffer(32), C.c_void_p()
    lde = TraceLde.new(g, trace, 8)
    h = lde.handle
    p = C.byref(pub)

    def free():
        if cc:
            L.zk_comp_free(cc)
            cc.value = None

    def eval_old():
        native.check(L.zk_eval_constraints(h, p, ct1.ctypes.data, cb1.ctypes.data, out1.ctypes.data))

    def eval_new(ext, out):
        a, b = (ct1, cb1) if ext == 1 else (ct, cb)
        native.check(L.zk_eval_constraints_ext(h, p, ext, a.ctypes.data, b.ctypes.data, None if out is None else out.ctypes.data))

    def commit_old():
        native.check(L.zk_commit_composition(h, out1.ctypes.data, 8, C.byref(cc), root, None))
        free()

    def commit_new(ext, comp):
        native.check(L.zk_commit_composition_ext(h, None if comp is None else comp.ctypes.data, ext, 8, C.byref(cc), root, None))
        free()

    def hand_off(ext):
        eval_new(ext, None)
        commit_new(ext, None)

    # warm: the divisor table, the E working set, the pages of the host buffers
    eval_old(), eval_new(1, new1), eval_new(2, out2), commit_old(), commit_new(1, new1), commit_new(2, out2)
    assert out1.tobytes() == new1.tobytes() and np.array_equal(out2[:, 0], out1)

    old_e, new_e = alternate(reps, [eval_old, lambda: eval_new(1, new1)])
    a = line("zk_eval_constraints", old_e)
    b = line("zk_eval_constraints_ext(ext = 1)", new_e)
    print(f"    old / new {a / b:.2f}; spread of the old call {max(old_e) - min(old_e):.3f} ms")
    old_c, new_c = alternate(reps, [commit_old, lambda: commit_new(1, new1)])
    a = line("zk_commit_composition(8 columns)", old_c)
    b = line("zk_commit_composition_ext(ext = 1, 8 columns)", new_c)
    print(f"    old / new {a / b:.2f}; spread of the old call {max(old_c) - min(old_c):.3f} ms")
    e2, c2 = alternate(reps, [lambda: eval_new(2, out2), lambda: commit_new(2, out2)])
    line("zk_eval_constraints_ext(ext = 2)", e2)
    line("zk_commit_composition_ext(ext = 2, 8 columns)", c2)
    for ext in (1, 2):
        hs = alternate(reps, [lambda: hand_off(ext)])[0]
        st = stages[ext]
        line(f"device hand-off, ext = {ext}: evaluate(NULL) + commit(NULL)", hs)
        print(f"    whole proof, field_extension = {ext}: constraints {st.get('constraints', float('nan')):.3f} ms + "
              f"composition {st.get('composition', float('nan')):.3f} ms (stage times of the last proof)")

    g.profile(True)
    for ext, buf in ((1, new1), (2, out2)):
        for _ in range(5):
            eval_new(ext, buf)
            commit_new(ext, buf)
    ks = g.kernel_stats()
    g.profile(False)
    for name in ("ce_to_natural", "ce_from_natural"):
        ms, launches, nbytes = ks[name]
        print(f"{name:16s} {launches} launches (5 at ext = 1, 5 at ext = 2): {ms / launches:.4f} ms each on average, "
              f"{nbytes / 1e6:.1f} MB moved in {ms:.4f} ms = {nbytes / ms / 1e9:.3f} TB/s "
              f"(HBM copy rate {HBM_COPY_TBS} TB/s)")
    lde.close()
    prog.close()
    g.close()


if __name__ == "__main__":
    main()
