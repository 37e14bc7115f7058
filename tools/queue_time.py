#!/usr/bin/env python3
"""What the proof queue (zk_queue, zkvm_amd/queue.py) costs and gains, on one GPU.

Leg A, the bench's workload: the 2^20 cipher-mix program from page-locked host columns, rotating four input sets,
  one      one thread calling prove_host (zk_prove_columns) on one prover;
  threads  three threads, each on a prover of its own (the recommendation so far);
  queue    one thread submitting to a 3-prover queue, keeping three jobs outstanding.
Leg B, short traces (n = 128, the reference's example program; 2^10; 2^16): proofs per second of a plain blocking loop
and of a queue of 1, 3 and 6 provers fed by one thread that keeps 2 P jobs outstanding.

Every leg of a size runs in every round, one after the other in one process, on the same pooled provers (a leg hands
them back and the next takes them), after an untimed warm-up round; a figure is the median over the rounds with the
spread beside it.  A leg's time is host wall time around proofs that have been delivered (zk_prove* returns, and a job
is done, only after the proof bytes are written).  Every proof is compared with the first proof of its input set.

    python tools/queue_time.py [--log-n 20] [--steps 30] [--rounds 5] [--out profiles/queue_time.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "encrypt-zkvm_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from zkvm_amd import native  # noqa: E402
from zkvm_amd.prover import GpuProver, HostTrace, Program, ProofOptions, make_pub_inputs  # noqa: E402
from zkvm_amd.queue import ProofQueue  # noqa: E402
from zkvm_amd.workloads import LR_PROGRAM, make_workload, ops_for_trace_len  # noqa: E402

OPTS = ProofOptions()
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def input_sets(src: str, count: int = 4):
    """`count` input sets of one program, each trace in page-locked memory: [(trace, pub)], and the trace length."""
    prog = Program(src)
    sets = []
    for k in range(count):
        w = make_workload(src, seed=7000 + k)
        host = HostTrace(prog.trace_len)
        trace, outputs = prog.trace(w.public, w.secret, w.server_key, w.last_row, out=host)
        sets.append((trace, make_pub_inputs(prog.hash, outputs, w.server_key.lwe_size(),
                                            w.server_key.parameters.delta)))
    n = prog.trace_len
    prog.close()
    return sets, n


class Checker:
    """Every proof of an input set must be the same bytes, whichever leg and prover made it."""

    def __init__(self, count):
        self.first = [None] * count
        self.lock = threading.Lock()

    def __call__(self, i, proof):
        with self.lock:
            if self.first[i] is None:
                self.first[i] = proof
            elif self.first[i] != proof:
                raise AssertionError(f"input set {i}: two proofs of the same trace differ")


def blocking_leg(sets, n, threads: int, steps: int, check) -> float:
    """`steps` proofs by `threads` host threads, each on a pooled prover of its own -> seconds."""
    provers = [GpuProver(0, max_trace_len=n, pooled=True) for _ in range(threads)]
    nxt, lock, errs = [0], threading.Lock(), []

    def run(g):
        try:
            while True:
                with lock:
                    j = nxt[0]
                    if j >= steps:
                        return
                    nxt[0] += 1
                i = j % len(sets)
                check(i, g.prove_host(sets[i][0], sets[i][1], OPTS)[0])
        except BaseException as e:  # noqa: BLE001  (re-raised below)
            errs.append(e)

    try:
        native.synchronize(0)
        t0 = time.perf_counter()
        if threads == 1:
            run(provers[0])
        else:
            ths = [threading.Thread(target=run, args=(g,)) for g in provers]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
        dt = time.perf_counter() - t0
    finally:
        for g in provers:
            g.close()
    if errs:
        raise errs[0]
    return dt


def queue_leg(sets, n, provers: int, outstanding: int, steps: int, check):
    """`steps` jobs through a queue of `provers`, one submitting thread keeping `outstanding` jobs in the queue ->
    (seconds, [queued_ms], [run_ms], peak_running)."""
    q = ProofQueue(0, max_trace_len=n, provers=provers)
    bufs = [(C.c_uint8 * (4 << 20))() for _ in range(outstanding)]
    queued, ran = [], []
    try:
        native.synchronize(0)
        t0 = time.perf_counter()
        slot_of, free, sent, got = {}, list(range(outstanding)), 0, 0
        while got < steps:
            while sent < steps and free:
                s = free.pop()
                i = sent % len(sets)
                job = q.submit_host(sets[i][0], sets[i][1], OPTS, proof_buf=bufs[s])
                slot_of[job.id] = (s, i)
                sent += 1
            job, status, proof, res = q.wait_any()
            if status != native.ZK_OK:
                raise AssertionError(f"job {job.id}: status {status}: {res['message']}")
            s, i = slot_of.pop(job.id)
            check(i, proof)
            free.append(s)
            queued.append(res["queued_ms"])
            ran.append(res["run_ms"])
            got += 1
        dt = time.perf_counter() - t0
        peak = q.stats()["peak_running"]
    finally:
        q.close()
    return dt, queued, ran, peak


def spread(values, fmt="{:.2f}"):
    return f"{fmt.format(statistics.median(values))} ({fmt.format(min(values))} .. {fmt.format(max(values))})"


def leg_a(log_n: int, steps: int, rounds: int):
    sets, n = input_sets(ops_for_trace_len(log_n, "cipher"))
    check = Checker(len(sets))
    say(f"Leg A: 2^{log_n} cipher-mix trace from page-locked host columns, {len(sets)} input sets, {steps} proofs per "
        f"leg and round, {rounds} timed rounds after one warm-up round; ms per proof, median (min .. max)")
    ms = {"one": [], "threads": [], "queue": []}
    q_ms, r_ms = [], []
    for r in range(rounds + 1):
        one = blocking_leg(sets, n, 1, steps, check)
        thr = blocking_leg(sets, n, 3, steps, check)
        que, queued, ran, peak = queue_leg(sets, n, 3, 3, steps, check)
        row = {"one": 1e3 * one / steps, "threads": 1e3 * thr / steps, "queue": 1e3 * que / steps}
        say(f"  round {r}{' (warm-up, not counted)' if r == 0 else ''}: one {row['one']:.2f}  threads {row['threads']:.2f}"
            f"  queue {row['queue']:.2f}  (queue: peak_running {peak}, queued_ms median {statistics.median(queued):.2f}, "
            f"run_ms median {statistics.median(ran):.2f})")
        if r:
            for k in ms:
                ms[k].append(row[k])
            q_ms += queued
            r_ms += ran
    say(f"  one thread, one prover (zk_prove_columns):      {spread(ms['one'])} ms per proof")
    say(f"  three threads, three provers:                   {spread(ms['threads'])} ms per proof")
    say(f"  one thread, 3-prover queue, 3 jobs outstanding: {spread(ms['queue'])} ms per proof")
    say(f"  queue jobs: queued_ms {spread(q_ms)}, run_ms {spread(r_ms)} (host wall time per job: waiting for a prover / "
        f"inside the blocking call; three run at once, so run_ms / 3 bounds the ms per proof)")
    lo, hi = min(ms["threads"]), max(ms["threads"])
    med = statistics.median(ms["queue"])
    inside = lo <= med <= hi
    say(f"  the queue's median {med:.2f} is {'inside' if inside else 'OUTSIDE'} the three-thread spread "
        f"{lo:.2f} .. {hi:.2f}" + ("" if inside else f" (gap to its median: {med - statistics.median(ms['threads']):+.2f} ms)"))
    say()


def leg_b(steps_of: dict, rounds: int):
    say(f"Leg B: short traces, proofs per second, median (min .. max) over {rounds} timed rounds after one warm-up "
        f"round; the queue is fed by one thread keeping 2 P jobs outstanding")
    for label, src in (("n = 128 (lr)", LR_PROGRAM), ("n = 2^10", ops_for_trace_len(10)),
                       ("n = 2^16", ops_for_trace_len(16))):
        sets, n = input_sets(src)
        steps = steps_of[n]
        check = Checker(len(sets))
        rate = {"blocking": [], 1: [], 3: [], 6: []}
        for r in range(rounds + 1):
            row = {"blocking": steps / blocking_leg(sets, n, 1, steps, check)}
            for P in (1, 3, 6):
                row[P] = steps / queue_leg(sets, n, P, 2 * P, steps, check)[0]
            if r:
                for k in rate:
                    rate[k].append(row[k])
        say(f"  {label}, {steps} proofs per leg and round")
        say(f"    blocking loop, one prover: {spread(rate['blocking'], '{:.0f}')} proofs/s")
        for P in (1, 3, 6):
            say(f"    queue of {P}:                {spread(rate[P], '{:.0f}')} proofs/s "
                f"({statistics.median(rate[P]) / statistics.median(rate['blocking']):.2f}x the blocking loop)")
    say()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-n", type=int, default=20, help="leg A's trace length (default 2^20)")
    ap.add_argument("--steps", type=int, default=30, help="leg A: proofs per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--short-steps", type=int, default=200, help="leg B: proofs per leg and round at n <= 2^10")
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if native.device_count() < 1:
        raise SystemExit("queue_time.py needs a GPU")
    rt = native.runtime_info()
    say(f"tools/queue_time.py --log-n {args.log_n} --steps {args.steps} --rounds {args.rounds} --short-steps "
        f"{args.short_steps}; hip runtime {rt['hip_runtime_version']}")
    say()
    if "a" in args.legs:
        leg_a(args.log_n, args.steps, args.rounds)
        native.lib().zk_prover_pool_trim(0)
    if "b" in args.legs:
        leg_b({128: args.short_steps, 1 << 10: args.short_steps, 1 << 16: max(20, args.short_steps // 4)}, args.rounds)
        native.lib().zk_prover_pool_trim(0)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
