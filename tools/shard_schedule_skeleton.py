"""The coset-sharded prover's schedule reduced to its shape, for comparing two builds of the library.

For every proof of the grid -- a 2^log_n cipher trace; world 2, 4, 8; field extension 1, 2; host trace (first proof, and
third proof: column hints active), device trace with 0, 3, 28 or the default number of replicated columns, and
prove_program; measurement mode on and off -- the schedule log (zk_prover_shard_schedule) without its times, and the
kernel names with their launch counts (zk_prover_kernel_stats on local rank 0, which collects every loopback rank's
launches).  A schedule is one token per entry, in order: `name/op/bytes` an exchange started (they are numbered in this
order, from 0), `Wn` the compute stream waiting for exchange n, `K` a segment boundary; `!` in front: the segment that
ends at this entry ran on the lead rank only.  Each distinct schedule and each distinct set of launch counts is printed
once; the last section names, for every proof of the grid, the two it produced.  Two libraries that enqueue the same
work in the same order print the same text.
    python3 tools/shard_schedule_skeleton.py [log_n] > skeleton.txt      (GPU box; ZKVM_GPU_LIB selects the library)
"""
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "encrypt-zkvm_amd"))


def kernel_counts(handle):
    from zkvm_amd.native import check, lib
    names, nl, cnt = (C.c_char_p * 64)(), (C.c_int * 64)(), C.c_int(0)
    check(lib().zk_prover_kernel_stats(handle, names, None, nl, None, 64, C.byref(cnt)))
    return sorted((names[i].decode(), nl[i]) for i in range(min(cnt.value, 64)))


def skeleton(sp, label, out):
    """out: {"sched": {text: id}, "kern": {text: id}, "proofs": [line]} (ids in order of first appearance)."""
    from zkvm_amd.native import check, lib
    toks, lead, ent = [], False, sp.schedule()["entries"]
    for i, e in enumerate(ent):
        if "seg_ms" in e:
            lead = e["lead"]
            if i + 1 == len(ent) or "seg_ms" in ent[i + 1]:
                toks.append("!K" if lead else "K")
        elif "start" in e:
            toks.append(f"{'!' if lead else ''}{e['name']}/{e['op']}/{e['bytes']:.0f}")
        else:
            toks.append(f"{'!' if lead else ''}W{e['wait']}")
    kern = ", ".join(f"{name} x{n}" for name, n in kernel_counts(sp.provers[0]))
    s = out["sched"].setdefault(" ".join(toks), len(out["sched"]) + 1)
    k = out["kern"].setdefault(kern, len(out["kern"]) + 1)
    out["proofs"].append(f"{label}: schedule {s}, launches {k}")
    check(lib().zk_prover_kernel_stats(sp.provers[0], None, None, None, None, 0, None))  # reset


def render(out):
    import textwrap
    lines = []
    for what, key in (("schedule", "sched"), ("launches", "kern")):
        for text, i in out[key].items():
            lines.append(f"== {what} {i}")
            lines += textwrap.wrap(text, 118, break_long_words=False, break_on_hyphens=False)
    return "\n".join(lines + ["== proofs"] + out["proofs"])


def main():
    from zkvm_amd.native import check, lib
    from zkvm_amd.prover import HostTrace, Program, ProofOptions, make_pub_inputs, vm_trace
    from zkvm_amd.sharded import ShardedProver
    from zkvm_amd.workloads import make_workload, ops_for_trace_len
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    src = ops_for_trace_len(log_n, "cipher")
    w = make_workload(src, seed=1000)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    n = trace.shape[1]
    pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    host = HostTrace(n)
    host.array[...] = trace
    prog = Program(src)
    inp = Program.encode_inputs(w.public, w.secret, w.server_key)
    out = {"sched": {}, "kern": {}, "proofs": []}
    for G in (2, 4, 8):
        for ext in (1, 2):
            opt = ProofOptions(field_extension=ext)
            proofs = set()
            for measure in (True, False):
                sp = ShardedProver.loopback(G, max_trace_len=n)  # (a new prover: no column hints yet)
                tag = f"G={G} ext={ext} measure={int(measure)}"
                try:
                    sp.set_measure(measure)
                    check(lib().zk_prover_profile(sp.provers[0], 1))
                    check(lib().zk_prover_kernel_stats(sp.provers[0], None, None, None, None, 0, None))
                    for k in (1, 2, 3):
                        proofs.add(sp.prove(host.array, pub, opt)[0])
                        if k != 2:
                            skeleton(sp, f"{tag} host proof {k}", out)
                    check(lib().zk_prover_kernel_stats(sp.provers[0], None, None, None, None, 0, None))
                    sp.upload_trace(trace)
                    for rep in (-1, 0, 3, 28):
                        sp.set_trace_split(rep)
                        proofs.add(sp.prove(None, pub, opt, n=n)[0])
                        skeleton(sp, f"{tag} device split {rep}", out)
                    sp.set_trace_split(-1)
                    proofs.add(sp.prove_program(prog, inp, w.last_row, opt)[2])
                    skeleton(sp, f"{tag} prove_program", out)
                    check(lib().zk_prover_profile(sp.provers[0], 0))
                finally:
                    sp.close()
                print(tag, file=sys.stderr, flush=True)
            assert len(proofs) == 1, "trace sources / modes disagree on the proof bytes"
    host.close()
    prog.close()
    print(render(out))


if __name__ == "__main__":
    main()
