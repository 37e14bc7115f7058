"""The proof queue on the GPU (zk_queue, zkvm_amd/queue.py): the jobs return the blocking calls' bytes, three jobs of a
resumed queue run at once, results and errors arrive where the header's contract says, and the pool is left intact.
Nothing here depends on timing: concurrency is read from what the queue decided under its lock (peak_running,
running_at_start, the provers), and every wait is on a job that was submitted."""
import ctypes as C
import threading

import pytest

from test_sharded import CASES, case_inputs
from validate_ref import add_to_cell
from zkvm_amd import native
from zkvm_amd.prover import (FIELD_EXTENSION_QUADRATIC, REFERENCE_OPTIONS, GpuProver, Program, ProofOptions,
                             make_pub_inputs, verify, vm_trace)
from zkvm_amd.queue import ProofQueue
from zkvm_amd.workloads import make_workload, ops_for_trace_len

pytestmark = pytest.mark.gpu
OK = native.ZK_OK
MAX_N = 1 << 10
QUAD = ProofOptions(num_queries=27, field_extension=FIELD_EXTENSION_QUADRATIC, fri_folding_factor=4,
                    fri_remainder_max_degree=31)
SOURCES = {64: "push.1\n", 256: ops_for_trace_len(8), 1024: ops_for_trace_len(10)}


def workload(n, seed=3):
    src = SOURCES[n]
    w = make_workload(src, seed=seed)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    assert trace.shape[1] == n
    return trace, make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta), w


@pytest.fixture(scope="module")
def traces():
    return {n: workload(n) for n in SOURCES}


@pytest.fixture(scope="module")
def lr():
    return case_inputs(next(c for c in CASES if c["name"] == "lr"))


@pytest.fixture(scope="module")
def want(traces):
    """The bytes GpuProver.prove_host returns on a fresh prover, per (n, options): computed once."""
    out = {}
    for n, (trace, pub, _) in traces.items():
        for name, opts in (("ref", REFERENCE_OPTIONS), ("quad", QUAD)):
            g = GpuProver(0, max_trace_len=MAX_N)
            try:
                out[n, name] = g.prove_host(trace, pub, opts)[0]
            finally:
                g.close()
    return out


@pytest.fixture(scope="module")
def queue():
    assert native.device_count() > 0, "no GPU visible"
    q = ProofQueue(0, max_trace_len=MAX_N, provers=3)
    yield q
    q.close()
    native.lib().zk_prover_pool_trim(0)


def test_same_bytes_as_the_blocking_call(queue, traces, want, lr):
    jobs = [(n, name, queue.submit_host(traces[n][0], traces[n][1], opts))
            for n in SOURCES for name, opts in (("ref", REFERENCE_OPTIONS), ("quad", QUAD))]
    lr_trace, lr_proof, lr_pub, lr_opts = lr
    assert lr_trace.shape[1] == 128
    lr_job = queue.submit_host(lr_trace, lr_pub, lr_opts)
    assert len(jobs) == 6 and len({j.id for _, _, j in jobs} | {lr_job.id}) == 7
    for n, name, job in jobs:
        status, proof, res = job.wait()
        assert status == OK and res["message"] == "" and 0 <= res["prover"] < 3, (n, name, res)
        assert res["proof_len"] == len(proof) and res["queued_ms"] >= 0 and res["run_ms"] > 0
        assert proof == want[n, name], (n, name)
        assert verify(proof, traces[n][1], 80 if name == "quad" else 95) == (0, ""), (n, name)
    status, proof, _ = lr_job.wait()
    assert status == OK and proof == lr_proof  # the committed golden
    assert verify(proof, lr_pub, 95) == (0, "")


def test_three_jobs_run_at_once(traces):
    q = ProofQueue(0, max_trace_len=MAX_N, provers=3)
    try:
        q.pause()
        jobs = [q.submit_host(traces[n][0], traces[n][1]) for n in (64, 256, 1024)]
        s = q.stats()
        assert (s["submitted"], s["queued"], s["running"], s["peak_running"]) == (3, 3, 0, 0)
        q.resume()
        got = [j.wait() for j in jobs]
        assert [st for st, _, _ in got] == [OK] * 3
        s = q.stats()
        assert s["peak_running"] == 3 and s["completed"] == 3 and s["queued"] == s["running"] == 0
        assert sorted(r["prover"] for _, _, r in got) == [0, 1, 2]
        assert sorted(r["running_at_start"] for _, _, r in got) == [0, 1, 2]
    finally:
        q.close()


def test_a_job_alone_takes_the_latency_schedule():
    n = 1 << 16
    src = ops_for_trace_len(16)
    w = make_workload(src, seed=4)
    trace, outputs, h = vm_trace(src, w.public, w.secret, w.server_key, w.last_row)
    pub = make_pub_inputs(h, outputs, w.server_key.lwe_size(), w.server_key.parameters.delta)
    q = ProofQueue(0, max_trace_len=n, provers=1)
    try:
        status, proof, res = q.submit_host(trace, pub).wait()
        assert status == OK and res["running_at_start"] == 0
        assert res["info"]["schedule"] == 2  # ZK_SCHED_LATENCY: the AUTO contract for a proof alone on its device
        assert verify(proof, pub, 95) == (0, "")
    finally:
        q.close()
        native.lib().zk_prover_pool_trim(0)


def test_delivery(queue, traces, want):
    trace, pub, _ = traces[64]
    jobs = [queue.submit_host(trace, pub) for _ in range(5)]
    for job in reversed(jobs):
        status, proof, _ = job.wait()
        assert status == OK and proof == want[64, "ref"]
    with pytest.raises(native.ZkError) as e:
        jobs[0].wait()  # delivered once: the id is unknown now
    assert e.value.code == native.ZK_ERR_INVALID_ARG
    more = {queue.submit_host(trace, pub).id for _ in range(5)}
    assert not more & {j.id for j in jobs}
    seen = []
    for _ in range(5):
        job, status, proof, res = queue.wait_any()
        assert status == OK and proof == want[64, "ref"] and res["id"] == job.id
        seen.append(job.id)
    assert sorted(seen) == sorted(more)  # each id once
    with pytest.raises(native.ZkError) as e:
        queue.wait_any()
    assert e.value.code == native.ZK_ERR_INVALID_ARG
    queue.pause()
    try:
        job = queue.submit_host(trace, pub)
        assert job.poll() is None  # ZK_ERR_PENDING
        res = native.JobResult()
        assert native.lib().zk_queue_poll(queue.handle, job.id, C.byref(res)) == native.ZK_ERR_PENDING
    finally:
        queue.resume()
    assert job.wait()[0] == OK


def test_errors_arrive_where_the_contract_says(queue, traces, want):
    trace, pub, _ = traces[256]
    # refused at submit, with the blocking call's text, and no job created
    before = queue.stats()["submitted"]
    g = GpuProver(0, max_trace_len=MAX_N)
    try:
        with pytest.raises(native.ZkError) as blocking:
            g.prove_host(trace, pub, ProofOptions(blowup_factor=4))
        with pytest.raises(native.ZkError) as queued:
            queue.submit_host(trace, pub, ProofOptions(blowup_factor=4))
        assert queued.value.code == blocking.value.code == native.ZK_ERR_INVALID_ARG
        assert str(queued.value).split(": ", 1)[1] == str(blocking.value).split(": ", 1)[1] != ""
        assert queue.stats()["submitted"] == before
        # a proof buffer that is too small: the job reports the size, and a job with that size succeeds
        status, proof, res = queue.submit_host(trace, pub, proof_cap=16).wait()
        assert status == native.ZK_ERR_BUFFER_TOO_SMALL and proof == b"" and res["message"] != ""
        assert res["proof_len"] == len(want[256, "ref"])
        status, proof, _ = queue.submit_host(trace, pub, proof_cap=res["proof_len"]).wait()
        assert status == OK and proof == want[256, "ref"]
        # one cell changed
        bad = add_to_cell(trace, 14, 100, 1)
        rc, report = g.validate_host(bad, pub)
        message = native.lib().zk_last_error().decode()
        assert rc == native.ZK_ERR_TRACE and message
    finally:
        g.close()
    queue.set_validate(True)
    try:
        job = queue.submit_host(bad, pub)
        got = job.validation()  # blocks until the job has finished; the report stays with the job until it is consumed
        status, proof, res = job.wait()
        assert status == native.ZK_ERR_TRACE and proof == b"" and res["proof_len"] == 0
        assert res["message"] == message and got == report
        assert native.lib().zk_last_error().decode() == message  # the caller's zk_last_error() is the job's message
        with pytest.raises(native.ZkError):
            job.validation()  # consumed
        with pytest.raises(native.ZkError):
            job.degrees()
    finally:
        queue.set_validate(False)
    status, proof, _ = queue.submit_host(bad, pub).wait()
    assert status == native.ZK_ERR_DEGREE
    # the queue proves normally after the failed jobs
    status, proof, _ = queue.submit_host(trace, pub).wait()
    assert status == OK and proof == want[256, "ref"]


def patterned(size=4 << 20):
    buf = (C.c_uint8 * size)()
    C.memset(buf, 0xA5, size)
    return buf


def untouched(buf):
    return bytes(buf) == b"\xa5" * len(buf)


def test_cancel_and_destroy(traces, want):
    trace, pub, _ = traces[64]
    q = ProofQueue(0, max_trace_len=MAX_N, provers=3)
    try:
        q.pause()
        bufs = [patterned() for _ in range(3)]
        jobs = [q.submit_host(trace, pub, proof_buf=b) for b in bufs]
        assert jobs[1].cancel() and not jobs[1].cancel()
        status, proof, res = jobs[1].wait()  # delivered while the queue is still paused
        assert status == native.ZK_ERR_CANCELLED and proof == b"" and res["prover"] == -1 and res["proof_len"] == 0
        assert untouched(bufs[1])
        q.resume()
        for k in (0, 2):
            status, proof, _ = jobs[k].wait()
            assert status == OK and proof == want[64, "ref"] and not untouched(bufs[k])
        assert not jobs[0].cancel()  # consumed
        assert q.stats()["completed"] == 2
    finally:
        q.close()
    q = ProofQueue(0, max_trace_len=MAX_N, provers=3)
    q.pause()
    bufs = [patterned() for _ in range(2)]
    jobs = [q.submit_host(trace, pub, proof_buf=b) for b in bufs]
    assert q.stats()["queued"] == 2
    q.close()  # returns: the queued jobs are cancelled, nothing ran
    assert all(untouched(b) for b in bufs)
    with pytest.raises(native.ZkError):
        jobs[0].wait()


def test_vm_and_device_jobs(queue, traces, want):
    trace, pub, w = traces[256]
    prog = Program(SOURCES[256])
    g = GpuProver(0, max_trace_len=MAX_N)
    try:
        inputs = Program.encode_inputs(w.public, w.secret, w.server_key)
        h, outputs, proof = prog.prove_device(g, inputs, w.last_row)
        assert proof == want[256, "ref"]
        status, got, res = queue.submit_program(prog, inputs, w.last_row).wait()
        assert status == OK and got == proof and res["outputs"] == outputs and res["program_hash"] == h
        # a device job on a trace that lives in ANOTHER prover's trace buffer
        d, n = g.upload_trace(trace)
        blocking = g.prove_device(d, n, pub)[0]
        assert blocking == want[256, "ref"]
        d, n = g.upload_trace(trace)
        status, got, res = queue.submit_device(d, n, pub, keep=g).wait()
        assert status == OK and got == blocking and res["info"]["schedule"] == 0
        # null pointers are refused at submit
        with pytest.raises(native.ZkError) as e:
            queue.submit_device(0, n, pub)
        assert e.value.code == native.ZK_ERR_INVALID_ARG
    finally:
        g.close()
        prog.close()


def test_several_submitters(queue, traces, want):
    results, errors = {}, []

    def submitter(t):
        try:
            jobs = [(n, queue.submit_host(traces[n][0], traces[n][1])) for n in (64, 256, 1024)]
            for n, job in jobs:
                status, proof, _ = job.wait()
                results[t, n] = (job.id, status, proof == want[n, "ref"])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=submitter, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 12 and len({r[0] for r in results.values()}) == 12
    assert all(status == OK and same for _, status, same in results.values()), results


def test_the_pool_is_intact_after_close(traces, lr):
    trace, pub, _ = traces[64]
    q = ProofQueue(0, max_trace_len=MAX_N, provers=2)
    q.set_validate(True)  # a switch of the queue's must not follow the prover back into the pool
    assert q.submit_host(trace, pub).wait()[0] == OK
    q.close()
    lr_trace, lr_proof, lr_pub, lr_opts = lr
    g = GpuProver(0, max_trace_len=MAX_N, pooled=True)
    try:
        assert g.prove_host(lr_trace, lr_pub, lr_opts)[0] == lr_proof
        # the trace test_errors_arrive_where_the_contract_says uses: ZK_ERR_TRACE on a prover that validates first
        bad = add_to_cell(traces[256][0], 14, 100, 1)
        assert g.prove_host(bad, traces[256][1], allow_degree_error=True)[3] == native.ZK_ERR_DEGREE
    finally:
        g.close()
        native.lib().zk_prover_pool_trim(0)
