"""The proof queue (zk_queue, include/zkvm_gpu.h "proof queue"): one host thread keeps several proofs in flight.

    q = ProofQueue(device=0, max_trace_len=1 << 20, provers=3)
    jobs = [q.submit_host(trace, pub) for trace, pub in requests]     # returns at once
    for job in jobs:
        status, proof, result = job.wait()                            # blocks on a condition variable
    q.close()

A job is one blocking call (zk_prove_columns, zk_prove_device, zk_vm_prove) run by a worker thread on one of the queue's
pooled provers: the same proof bytes.  Jobs start in submission order; a job prefers the idle prover that last proved
the same (trace length, program hash).
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import native
from .native import JobResult, PubInputs, ZkError, check, lib
from .prover import REFERENCE_OPTIONS, ProofOptions, bytes_elems, elems_bytes

PROOF_CAP = 4 << 20  # the proof buffer a job gets unless the caller passes one (GpuProver's size)


class ProofJob:
    """A job of a ProofQueue.  It keeps the arrays and buffers the library reads or writes alive until it is
    consumed (wait, a poll that delivers, or the queue's wait_any)."""

    def __init__(self, queue: "ProofQueue", job_id: int, buf, keep):
        self.queue = queue
        self.id = job_id
        self.buf = buf
        self._keep = keep
        self.outputs_buf = self.hash_buf = None
        self.consumed = False

    def _deliver(self, res: JobResult):
        self.consumed = True
        self.queue._jobs.pop(self.id, None)
        n = res.proof_len if res.status in (native.ZK_OK, native.ZK_ERR_DEGREE) else 0
        proof = C.string_at(C.addressof(self.buf), min(n, len(self.buf))) if n else b""
        d = res.to_dict()
        d["id"] = self.id
        if self.outputs_buf is not None and res.status in (native.ZK_OK, native.ZK_ERR_DEGREE):
            d["outputs"] = bytes_elems(bytes(self.outputs_buf))
            d["program_hash"] = bytes_elems(bytes(self.hash_buf))
        self._keep = None
        return res.status, proof, d

    def wait(self):
        """zk_queue_wait -> (status, proof bytes, result dict).  status is what the blocking call would have returned
        (ZK_ERR_CANCELLED for a cancelled job); the proof is empty unless one was written; the dict is zk_job_result
        (and, for a VM job, `outputs` and `program_hash`).  Raises ZkError for a job already consumed."""
        res = JobResult()
        check(lib().zk_queue_wait(self.queue._handle(), self.id, C.byref(res)), "zk_queue_wait")
        return self._deliver(res)

    def poll(self):
        """zk_queue_poll: None while the job is queued or running, else what wait() returns."""
        res = JobResult()
        rc = lib().zk_queue_poll(self.queue._handle(), self.id, C.byref(res))
        if rc == native.ZK_ERR_PENDING:
            return None
        check(rc, "zk_queue_poll")
        return self._deliver(res)

    def cancel(self) -> bool:
        """zk_queue_cancel: True if the job had not started (it is then delivered as ZK_ERR_CANCELLED)."""
        return lib().zk_queue_cancel(self.queue._handle(), self.id) == native.ZK_OK

    def validation(self) -> dict:
        """zk_queue_job_validation: the trace validation report of a finished job, before it is consumed."""
        v = native.Validation()
        check(lib().zk_queue_job_validation(self.queue._handle(), self.id, C.byref(v)), "zk_queue_job_validation")
        return v.to_dict()

    def degrees(self) -> dict:
        """zk_queue_job_degrees: the degree check's report of a finished job, before it is consumed."""
        d = native.Degrees()
        check(lib().zk_queue_job_degrees(self.queue._handle(), self.id, C.byref(d)), "zk_queue_job_degrees")
        return d.to_dict()


class ProofQueue:
    """zk_queue: `provers` pooled provers of one device, each with a worker thread."""

    def __init__(self, device: int = 0, max_trace_len: int = 1 << 16, max_blowup: int = 8, provers: int = 3):
        h = C.c_void_p()
        check(lib().zk_queue_create(device, max_trace_len, max_blowup, provers, C.byref(h)), "zk_queue_create")
        self.handle = h
        self.device, self.max_trace_len, self.provers = device, max_trace_len, provers
        self._jobs = {}  # id -> ProofJob, until consumed: keeps the jobs' buffers alive, and serves wait_any
        self._lock = threading.Lock()  # a job is registered before any thread can look its id up

    def _handle(self):
        if not self.handle:
            raise ZkError(native.ZK_ERR_INVALID_ARG, "the queue is closed")
        return self.handle

    def _submitted(self, rc, what, jid, buf, keep) -> ProofJob:
        check(rc, what)
        job = ProofJob(self, jid.value, buf, keep)
        self._jobs[job.id] = job
        return job

    @staticmethod
    def _buffer(proof_cap, proof_buf):
        if proof_buf is not None:
            return proof_buf, len(proof_buf) if proof_cap is None else proof_cap
        cap = PROOF_CAP if proof_cap is None else proof_cap
        return (C.c_uint8 * max(cap, 1))(), cap

    def submit_host(self, trace: np.ndarray, pub: PubInputs, options: ProofOptions = REFERENCE_OPTIONS,
                    proof_cap: int | None = None, proof_buf=None) -> ProofJob:
        """zk_queue_submit_columns: a (28, n, 2) uint64 host trace (pinned -- HostTrace -- or pageable).  proof_buf: a
        ctypes uint8 array of the caller's to receive the proof (default: one of 4 MiB per job); proof_cap: the capacity
        to declare (default: the buffer's size)."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        assert trace.ndim == 3 and trace.shape[0] == 28 and trace.shape[2] == 2
        cols = (C.c_void_p * 28)(*[trace.ctypes.data + c * trace.strides[0] for c in range(28)])
        buf, cap = self._buffer(proof_cap, proof_buf)
        opt, jid = options.to_c(), C.c_uint64(0)
        with self._lock:
            rc = lib().zk_queue_submit_columns(self._handle(), cols, trace.shape[1], C.byref(opt), C.byref(pub), buf,
                                               cap, C.byref(jid))
            return self._submitted(rc, "zk_queue_submit_columns", jid, buf, (trace,))

    def submit_device(self, d_trace: int, n: int, pub: PubInputs, options: ProofOptions = REFERENCE_OPTIONS,
                      proof_cap: int | None = None, proof_buf=None, keep=None) -> ProofJob:
        """zk_queue_submit_device: a trace in the device's HBM (e.g. GpuProver.upload_trace's pointer); keep: whatever
        owns that memory, held until the job is consumed."""
        buf, cap = self._buffer(proof_cap, proof_buf)
        opt, jid = options.to_c(), C.c_uint64(0)
        with self._lock:
            rc = lib().zk_queue_submit_device(self._handle(), d_trace, n, C.byref(opt), C.byref(pub), buf, cap,
                                              C.byref(jid))
            return self._submitted(rc, "zk_queue_submit_device", jid, buf, (keep,))

    def submit_program(self, program, inputs, last_row=None, options: ProofOptions = REFERENCE_OPTIONS,
                       proof_cap: int | None = None, proof_buf=None) -> ProofJob:
        """zk_queue_submit_vm: vm::prove of a compiled Program on inputs from Program.encode_inputs; last_row None:
        drawn by the library.  The result dict carries `outputs` and `program_hash`."""
        buf, cap = self._buffer(proof_cap, proof_buf)
        outputs, h = (C.c_uint8 * 256)(), (C.c_uint8 * 32)()
        opt, jid = options.to_c(), C.c_uint64(0)
        with self._lock:
            rc = lib().zk_queue_submit_vm(self._handle(), program.handle, *inputs,
                                          elems_bytes(last_row) if last_row is not None else None, C.byref(opt), buf,
                                          cap, outputs, h, C.byref(jid))
            job = self._submitted(rc, "zk_queue_submit_vm", jid, buf, (program,))
            job.outputs_buf, job.hash_buf = outputs, h
            return job

    def wait_any(self):
        """zk_queue_wait_any -> (job, status, proof bytes, result dict) of the first undelivered job to finish;
        raises ZkError (ZK_ERR_INVALID_ARG) when nothing is pending."""
        res, jid = JobResult(), C.c_uint64(0)
        check(lib().zk_queue_wait_any(self._handle(), C.byref(jid), C.byref(res)), "zk_queue_wait_any")
        with self._lock:
            job = self._jobs[jid.value]
        return (job,) + job._deliver(res)

    def pause(self):
        check(lib().zk_queue_pause(self._handle()), "zk_queue_pause")

    def resume(self):
        check(lib().zk_queue_resume(self._handle()), "zk_queue_resume")

    def set_validate(self, on: bool):
        """zk_queue_set_validate: Trace::validate before every proof, on every prover; refused while jobs are pending."""
        check(lib().zk_queue_set_validate(self._handle(), 1 if on else 0), "zk_queue_set_validate")

    def set_validate_degrees(self, on: bool):
        check(lib().zk_queue_set_validate_degrees(self._handle(), 1 if on else 0), "zk_queue_set_validate_degrees")

    def stats(self) -> dict:
        s, c = C.c_uint64(0), C.c_uint64(0)
        q, r, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().zk_queue_stats(self._handle(), C.byref(s), C.byref(c), C.byref(q), C.byref(r), C.byref(p)),
              "zk_queue_stats")
        return {"submitted": s.value, "completed": c.value, "queued": q.value, "running": r.value,
                "peak_running": p.value}

    def close(self):
        """zk_queue_destroy: cancels the queued jobs, waits for the running ones, returns the provers to the pool.  The
        jobs' buffers are kept until then."""
        if self.handle:
            lib().zk_queue_destroy(self.handle)
            self.handle = None
            self._jobs.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
