"""One rank of a two-process sharded proof whose ranks are given DIFFERENT inputs, switches or prover histories
(tests/test_gpu_shard_agree.py): what zk_prove_sharded returns on each rank once the ranks have exchanged their control
records (include/zkvm_gpu.h, "what the ranks agree on").  The `lr` golden case (n = 128) over zk_comm_create_host and
a TCP host group with a 20 s timeout: a rank left waiting is a failed test in bounded time.  The two cases about
column detection and column hints also prove a 2^13-row trace: the library builds a detector only above 2^12 rows, so
at n = 128 no rank detects or holds hints whatever its switches say.  Every step's status, message, proof sha256,
agreement and exchange names go to <out>/rank<r>.json.

usage: python tests/agree_worker.py RANK WORLD PORT OUTDIR CASE
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "encrypt-zkvm_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402


def main():
    rank, world, port, out, case = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), Path(sys.argv[4]), sys.argv[5]
    from zkvm_amd import native
    res = {"case": case, "steps": []}
    L = native.lib()
    # first of all: without the agreement this worker must not start a proof whose ranks differ
    if not hasattr(L, "zk_comm_agreement"):
        res["missing"] = "zk_comm_agreement"
        (out / f"rank{rank}.json").write_text(json.dumps(res))
        sys.exit(3)
    from test_sharded import CASES, case_inputs
    from validate_ref import add_to_cell
    from zkvm_amd.hostgroup import HostGroup
    from zkvm_amd.prover import ProofOptions
    from zkvm_amd.sharded import ShardedProver
    trace, golden, pub, opts = case_inputs(next(c for c in CASES if c["name"] == "lr"))
    n = trace.shape[1]
    res["golden"] = hashlib.sha256(golden).hexdigest()
    big = None
    if case in ("sparse_off", "new_prover"):  # a trace long enough for a detector; the single-GPU proof is the pin
        from zkvm_amd.prover import GpuProver, make_pub_inputs, vm_trace
        from zkvm_amd.workloads import make_workload, ops_for_trace_len
        src = ops_for_trace_len(13, "pushadd")
        w = make_workload(src, seed=61)
        bt, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
        bpub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
        g = GpuProver(0, max_trace_len=bt.shape[1])
        try:
            single, _, _, rc = g.prove(bt, bpub, ProofOptions())
            assert rc == 0
        finally:
            g.close()
        big = (bt, bpub, ProofOptions())
        res["single"] = hashlib.sha256(single).hexdigest()
    max_n = big[0].shape[1] if big else n
    dist = HostGroup(rank, world, port=port, timeout=20)
    fn = dist.exchange_fn()
    sp = ShardedProver.host(rank, world, fn, 0, 64 if (case == "small_prover" and rank == 1) else max_n)

    def info(s):
        pi = native.ProofInfo()
        native.check(L.zk_prover_proof_info(s.provers[0], C.byref(pi)))
        return {"hint_redos": pi.hint_redos, "hinted_sparse": pi.hinted_sparse, "derived": pi.derived}

    def step(name, s, t, pub_, opts_, device=False):
        t = np.ascontiguousarray(t, dtype=np.uint64)
        nn = s.upload_trace(t) if device else t.shape[1]
        opt = opts_.to_c()
        buf = C.create_string_buffer(1 << 20)
        plen = C.c_size_t(len(buf))
        arr = (C.c_void_p * 1)(s.provers[0].value)
        rc = L.zk_prove_sharded(s.comm, arr, 1, None if device else t.ctypes.data, nn, C.byref(opt), C.byref(pub_), buf,
                                C.byref(plen), None)
        rec = {"name": name, "rc": rc, "msg": L.zk_last_error().decode() if rc != 0 else "",
               "proof_len": plen.value, "sha256": hashlib.sha256(buf.raw[:plen.value]).hexdigest() if rc == 0 else None,
               "agreement": s.agreement(), "exchanges": sorted(s.exchange_stats()), "info": info(s)}
        res["steps"].append(rec)
        print(f"rank {rank} {case}/{name}: rc {rc}", flush=True)
        return rec

    try:
        if case == "options":
            mine = ProofOptions(31, opts.blowup_factor, opts.grinding_factor, opts.field_extension,
                                opts.fri_folding_factor, opts.fri_remainder_max_degree) if rank == 1 else opts
            step("differ", sp, trace, pub, mine)
            step("equal", sp, trace, pub, opts)
        elif case == "pub_inputs":
            mine = type(pub).from_buffer_copy(bytes(pub))
            if rank == 1:
                mine.stack_outputs[16 * 3] ^= 1
            step("differ", sp, trace, mine, opts)
            step("equal", sp, trace, pub, opts)
        elif case == "small_prover":
            step("refused", sp, trace, pub, opts)
        elif case == "sparse_off":  # (ZK_SPARSE=0 is in rank 1's environment: the test sets it)
            step("device", sp, trace, pub, opts, device=True)
            step("big_device", sp, *big, device=True)
        elif case == "new_prover":
            step("first", sp, *big)
            step("second", sp, *big)
            if rank == 1:  # a new prover on the same exchange callback: it holds no hints
                sp.close()
                sp = ShardedProver.host(rank, world, fn, 0, max_n)
            step("third", sp, *big)
            step("fourth", sp, *big)
            step("fifth", sp, *big)
            step("lr", sp, trace, pub, opts)
        elif case == "validate":
            if rank == 0:
                sp.set_validate(True)
            bad = add_to_cell(trace, 0, n // 2, 1)  # the first row of rank 1's window
            r = step("broken", sp, bad, pub, opts)
            r["validation"] = sp.validation()
            step("valid", sp, trace, pub, opts)
        else:
            raise SystemExit(f"unknown case {case}")
    finally:
        sp.close()
    (out / f"rank{rank}.json").write_text(json.dumps(res))
    dist.close()


if __name__ == "__main__":
    main()
