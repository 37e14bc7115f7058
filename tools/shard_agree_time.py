"""Loopback sharded proofs of configs[2] (the c2_cipher_2p20 pin) timed call by call, for the A/B of the control
exchange (run once per library, ZKVM_GPU_LIB, alternating) and for the cost of sharded trace validation.
    python3 tools/shard_agree_time.py ab [calls]        -> one JSON line: median / p10 / p90 ms at G = 2 and G = 8,
                                                           host trace, validate off
    python3 tools/shard_agree_time.py validate [calls]  -> one JSON line per (G, source): the proof with the switch
                                                           off and on, and the call a broken trace ends in
"""
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "encrypt-zkvm_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


def timed(f, calls, warm=3, prep=None):
    for _ in range(warm):
        if prep:
            prep()
        f()
    ts = []
    for _ in range(calls):
        time.sleep(0.01)
        if prep:
            prep()  # (untimed)
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 3), "p10_ms": round(ts[len(ts) // 10], 3),
            "p90_ms": round(ts[(9 * len(ts)) // 10], 3), "min_ms": round(ts[0], 3)}


def main():
    from golden_large import LARGE_CASES, large_inputs
    from zkvm_amd import native
    from zkvm_amd.sharded import ShardedProver
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 31
    c = next(c for c in LARGE_CASES if c["name"] == "c2_cipher_2p20")
    ht, trace, pub, opts = large_inputs(c)
    n = trace.shape[1]
    lib = os.environ.get("ZKVM_GPU_LIB", "default")
    if mode == "ab":
        out = {"lib": lib, "calls": calls}
        for G in (2, 8):
            sp = ShardedProver.loopback(G, max_trace_len=n)
            out[f"G{G}"] = timed(lambda: sp.prove(trace, pub, opts), calls)
            sp.close()
        print(json.dumps(out), flush=True)
    else:
        from validate_ref import add_to_cell
        bad = add_to_cell(trace, 0, n // 2, 1)
        for G in (2, 4, 8):
            for source in ("host", "device"):
                sp = ShardedProver.loopback(G, max_trace_len=n)

                def run(t, want):
                    def f():
                        try:
                            sp.prove(None, pub, opts, n=n) if source == "device" else sp.prove(t, pub, opts)
                            rc = 0
                        except native.ZkError as e:
                            rc = e.code
                        assert rc == want, rc
                    return f

                def up(t):  # device source: the trace goes into every rank's buffer before each call, untimed
                    return (lambda: sp.upload_trace(t)) if source == "device" else None
                off = timed(run(trace, 0), calls, prep=up(trace))
                sp.set_validate(True)
                on = timed(run(trace, 0), calls, prep=up(trace))
                broken = timed(run(bad, native.ZK_ERR_TRACE), calls, prep=up(bad))
                sp.close()
                print(json.dumps({"G": G, "source": source, "calls": calls, "proof_validate_off": off,
                                  "proof_validate_on": on, "broken_trace_call": broken}), flush=True)
    ht.close()


if __name__ == "__main__":
    main()
