"""One rank of a two-process sharded degree check (zk_prover_set_validate_degrees through zk_prove_sharded over
zk_comm_create_host + a TCP host group), started by tests/test_shard_degrees_multiprocess.py: a push/add VM trace of
128 rows with a zero last row (the switch on: ZK_ERR_DEGREES and the merged report) and with its random one (the
proof bytes).  The rank's results go to <out>/rank<r>.json.

usage: python tests/shard_degrees_worker.py RANK WORLD PORT OUTDIR
"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "encrypt-zkvm_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], Path(sys.argv[4])
    from zkvm_amd import native
    from zkvm_amd.hostgroup import HostGroup
    from zkvm_amd.prover import ProofOptions, make_pub_inputs, vm_trace
    from zkvm_amd.sharded import ShardedProver
    from zkvm_amd.workloads import make_workload, push_add_program
    src = push_add_program(3)  # (128 rows)
    w = make_workload(src, seed=7)
    good, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    zero = good.copy()
    zero[:, -1, :] = 0
    dist = HostGroup(rank, world, port=int(port), timeout=20)
    sp = ShardedProver.host(rank, world, dist.exchange_fn(), 0, good.shape[1])
    res = {}
    try:
        sp.set_validate_degrees(rank == world - 1)  # on at the last rank only: the ranks agree to check (OR)
        L = native.lib()
        opt = ProofOptions().to_c()
        arr = (C.c_void_p * 1)(sp.provers[0].value)
        for name, trace in (("zero", zero), ("good", good)):
            t = np.ascontiguousarray(trace, dtype=np.uint64)
            buf = C.create_string_buffer(1 << 20)
            plen = C.c_size_t(len(buf))
            rc = L.zk_prove_sharded(sp.comm, arr, 1, t.ctypes.data, t.shape[1], C.byref(opt), C.byref(pub), buf,
                                    C.byref(plen), None)
            res[name] = {"rc": rc, "msg": L.zk_last_error().decode() if rc else "", "proof_len": plen.value,
                         "sha256": hashlib.sha256(buf.raw[:plen.value]).hexdigest(), "degrees": sp.degrees(),
                         "agreement": sp.agreement(), "exchanges": sorted(sp.exchange_stats())}
    finally:
        sp.close()
    (out / f"rank{rank}.json").write_text(json.dumps(res))
    dist.close()


if __name__ == "__main__":
    main()
