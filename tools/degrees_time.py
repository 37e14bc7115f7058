"""What the transition-constraint degree check costs (zk_degrees_device) on a device-resident valid 2^20 trace, against
a whole proof and its constraint evaluator on the same GPU in the same process.

  * the median wall time of `reps` zk_degrees_device calls (the call ends in a stream sync) and of `reps`
    zk_prove_device calls of the same trace with the switch off;
  * from one profiled check (zk_prover_kernel_stats): k_transition_quotients, the NTT passes, comp_cross and
    k_poly_degrees.  The NTT passes of the front (28 interpolations, 224 coset transforms) and of the quotients'
    interpolation (160 inverse transforms) run under the same kernel names, so the 160 transforms' time is given as
    their share of the transformed elements (160 of 412 n), an estimate and labelled so;
  * from one profiled proof: eval_constraints, the production evaluator over 7 of the same 8 CE cosets.

Usage (GPU box): python3 tools/degrees_time.py [log_n] [reps]    (profiles/degrees_time.txt keeps one run's output)
"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "encrypt-zkvm_amd"))

from zkvm_amd import native  # noqa: E402
from zkvm_amd.prover import GpuProver, Program, ProofOptions, make_pub_inputs  # noqa: E402
from zkvm_amd.workloads import make_workload, ops_for_trace_len  # noqa: E402


def timed(reps, call):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def line(what, reps, ts):
    print(f"{what}, {reps} calls: median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}")


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 31
    src = ops_for_trace_len(log_n, "cipher")
    w = make_workload(src, seed=1000)
    prog = Program(src)
    g = GpuProver(0, max_trace_len=1 << log_n)
    inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
    d, n, outputs = prog.trace_device(g, inputs, last_row=w.last_row)
    pub = make_pub_inputs(prog.hash, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)

    def degrees():
        rc, rep = g.degrees_device(d, n, pub)
        assert rc == native.ZK_OK and rep["actual"] == rep["expected"], (rc, rep)

    def proof():
        assert g.prove_device(d, n, pub, ProofOptions())[3] == 0

    degrees()  # warm: the plan's tables, the divisor table
    proof()
    print(f"n = 2^{log_n}")
    line("zk_degrees_device", reps, timed(reps, degrees))
    line("zk_prove_device (switch off)", reps, timed(reps, proof))
    g.profile(True)
    degrees()
    check = g.kernel_stats()
    g.profile(True)  # (resets the totals)
    proof()
    prove = g.kernel_stats()
    g.profile(False)
    for name in ("transition_quotients", "ntt_single", "ntt_pass1", "ntt_pass2", "comp_cross", "poly_degrees"):
        if name in check:
            ms, launches, nbytes = check[name]
            print(f"check  {name:22s} {ms:9.4f} ms, {launches:3d} launches, {nbytes / ms / 1e6:8.1f} GB/s algorithmic")
    ntt_ms = sum(check[k][0] for k in ("ntt_single", "ntt_pass1", "ntt_pass2") if k in check)
    print(f"check  NTT passes together {ntt_ms:.4f} ms over 412 n elements; the 160 size-n inverse transforms by their "
          f"share of the elements (160 / 412, an estimate): {ntt_ms * 160 / 412:.4f} ms")
    print(f"check  all kernels {sum(v[0] for v in check.values()):.4f} ms")
    e_ms, e_launches, _ = prove["eval_constraints"]
    print(f"proof  eval_constraints       {e_ms:9.4f} ms, {e_launches:3d} launch (7 CE cosets, coefficients folded)")
    print(f"proof  all kernels {sum(v[0] for v in prove.values()):.4f} ms")
    q_ms = check["transition_quotients"][0]
    print(f"transition_quotients / eval_constraints per CE row: {(q_ms / 8) / (e_ms / 7):.3f}")
    prog.close()
    g.close()


if __name__ == "__main__":
    main()
