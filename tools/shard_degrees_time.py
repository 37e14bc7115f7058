"""What the sharded transition-constraint degree check costs at 2^20 (configs[2], the c2_cipher_2p20 pin), through the
LOOPBACK communicator on ONE GPU: every rank's kernels and the exchange's copies share that GPU, so a call's time is
roughly the sum over the ranks, not what one rank of a multi-GPU job would see.  No multi-GPU hardware has run this.

Each call is synchronous (it ends in stream syncs), and is timed by two HIP events recorded on the null stream around
it, as the GPU's clock sees it.

    python3 tools/shard_degrees_time.py time [calls]  -> per world 2, 4, 8 one JSON line: the sharded check
                                                        (zk_degrees_sharded, trace in every rank's buffer), and a
                                                        sharded proof with both switches off; and one line for
                                                        zk_degrees_device on a full prover in the same run
    python3 tools/shard_degrees_time.py ab [calls]    -> one JSON line: the sharded proof with both switches off at
                                                        world 2 and 8, for the A/B against the parent commit's
                                                        library (run once per library, ZKVM_GPU_LIB, alternating)
profiles/shard_degrees_time.txt and profiles/shard_degrees_ab.txt keep one session's output.
"""
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "encrypt-zkvm_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


class EventTimer:
    def __init__(self, hip):
        self.hip, self.a, self.b = hip, C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

    def ms(self, call):
        hip = self.hip
        assert hip.hipEventRecord(self.a, None) == 0
        call()
        assert hip.hipEventRecord(self.b, None) == 0 and hip.hipEventSynchronize(self.b) == 0
        out = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(out), self.a, self.b) == 0
        return out.value


def timed(timer, call, calls, warm=3, prep=None):
    """prep (untimed) before every call: the trace goes into every rank's buffer again."""
    ts = []
    for i in range(warm + calls):
        if prep:
            prep()
        t = timer.ms(call)
        if i >= warm:
            ts.append(t)
    ts.sort()
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def main():
    from golden_large import LARGE_CASES, large_inputs
    from zkvm_amd import native
    from zkvm_amd.prover import GpuProver
    from zkvm_amd.sharded import ShardedProver
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    c = next(c for c in LARGE_CASES if c["name"] == "c2_cipher_2p20")
    ht, trace, pub, opts = large_inputs(c)
    n = trace.shape[1]
    hip = native.hip_runtime()
    for f in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize, hip.hipEventElapsedTime):
        f.restype = C.c_int
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    timer = EventTimer(hip)
    label = "loopback on one GPU"
    if mode == "ab":
        out = {"lib": os.environ.get("ZKVM_GPU_LIB", "default"), "what": f"sharded proof, switches off, {label}",
               "calls": calls}
        for G in (2, 8):
            sp = ShardedProver.loopback(G, max_trace_len=n)
            out[f"G{G}"] = timed(timer, lambda: sp.prove(trace, pub, opts), calls)
            sp.close()
        print(json.dumps(out), flush=True)
        ht.close()
        return
    g = GpuProver(0, max_trace_len=n)
    d, _ = g.upload_trace(trace)

    def single():
        rc, rep = g.degrees_device(d, n, pub)
        assert rc == native.ZK_OK and rep["mismatch_mask"] == 0

    print(json.dumps({"n": n, "what": "zk_degrees_device, full prover", "calls": calls, **timed(timer, single, calls)}),
          flush=True)
    g.close()
    for G in (2, 4, 8):
        sp = ShardedProver.loopback(G, max_trace_len=n)

        def up():
            sp.upload_trace(trace)

        def check():
            rc, rep = sp.degrees_device(n, pub)
            assert rc == native.ZK_OK and rep["mismatch_mask"] == 0

        def proof():
            sp.prove(None, pub, opts, n=n)

        line = {"n": n, "world": G, "what": label, "calls": calls,
                "degrees_sharded": timed(timer, check, calls, prep=up)}
        stats = sp.exchange_stats()
        line["degrees_slices_ms_bytes"] = [round(stats["degrees_slices"][0], 3), stats["degrees_slices"][1]]
        line["proof_switches_off"] = timed(timer, proof, calls, prep=up)
        sp.set_validate_degrees(True)
        line["proof_degrees_on"] = timed(timer, proof, calls, prep=up)
        sp.close()
        print(json.dumps(line), flush=True)
    ht.close()


if __name__ == "__main__":
    main()
