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


def main():
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
