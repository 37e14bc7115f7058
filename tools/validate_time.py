"""What trace validation costs (zk_validate_device) on a device-resident valid 2^20 trace, against the constraint
evaluator of the same proof on the same GPU in the same process.

  * the median wall time of `reps` zk_validate_device calls (one launch, one small read-back, one stream sync);
  * from one profiled proof with the validate switch on (zk_prover_kernel_stats): the device time per row of
    validate_trace (n rows) and of eval_constraints (its CE rows: algorithmic bytes / 480 B at blowup 8), and their
    ratio -- the yardstick is the evaluator's per-row time, 1.5 x it the bound.

Usage (GPU box): python3 tools/validate_time.py [log_n] [reps]    (profiles/validate_time.txt keeps one run's output)
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
    rc, rep = g.validate_device(d, n, pub)
    assert rc == native.ZK_OK and rep["first_kind"] == 0 and rep["steps_checked"] == n - 2, (rc, rep)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rc, _ = g.validate_device(d, n, pub)
        ts.append(1e3 * (time.perf_counter() - t0))
        assert rc == native.ZK_OK
    print(f"n = 2^{log_n}: zk_validate_device, {reps} calls: median {statistics.median(ts):.4f} ms  "
          f"min {min(ts):.4f}  max {max(ts):.4f}")
    # one profiled proof of the same trace with the switch on: both kernels' device time
    g.prove_device(d, n, pub, ProofOptions())  # warm: the plan's tables
    g.set_validate(True)
    g.profile(True)
    _, _, _, rc = g.prove_device(d, n, pub, ProofOptions())
    stats = g.kernel_stats()
    g.profile(False)
    g.set_validate(False)
    assert rc == 0
    v_ms, v_launches, v_bytes = stats["validate_trace"]
    e_ms, e_launches, e_bytes = stats["eval_constraints"]
    v_rows, e_rows = v_bytes / 448.0, e_bytes / 480.0
    v_ns, e_ns = 1e6 * v_ms / v_rows, 1e6 * e_ms / e_rows
    print(f"validate_trace:   {v_ms:.4f} ms, {v_launches} launch, {v_rows:.0f} rows ({v_rows / n:.2f} n), "
          f"{v_ns:.4f} ns/row, {v_bytes / v_ms / 1e6:.1f} GB/s algorithmic")
    print(f"eval_constraints: {e_ms:.4f} ms, {e_launches} launch, {e_rows:.0f} rows ({e_rows / n:.2f} n), "
          f"{e_ns:.4f} ns/row")
    print(f"validate_trace / eval_constraints per row: {v_ns / e_ns:.3f} (bound 1.5)")
    prog.close()
    g.close()


if __name__ == "__main__":
    main()
