"""The test entry point of the proof queue's scheduling core (csrc/job_queue.hpp, driven by csrc/queue.cpp's scripted
executor: no GPU, no HIP call): its ctypes binding and one Python call per operation.  A job is a (key length, key tag)
pair; the executor logs (id, prover), holds the job until release(id), and returns tag + 1000.
"""
from __future__ import annotations

import ctypes as C

from . import native

SYMBOL = "zk_diag_" + "job_queue"
(CREATE, SUBMIT, RELEASE, WAIT, POLL, WAIT_ANY, CANCEL, PAUSE, RESUME, STATS, STATE, LOG, CLOSE, JOIN, DESTROY, LAYOUT,
 CHOOSE) = range(17)
QUEUED, RUNNING, DONE, CANCELLED = range(4)  # job_queue.hpp JobState
_bound = False


def _fn():
    global _bound
    f = getattr(native.lib(), SYMBOL)
    if not _bound:
        # (handle, op, a, b, out, cap)
        f.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_size_t]
        _bound = True
    return f


def _signed(v: int) -> int:
    return v - (1 << 64) if v >> 63 else v


def job_result_layout() -> dict:
    """sizeof(zk_job_result) and its field offsets as the library was compiled."""
    out = (C.c_uint64 * 10)()
    native.check(_fn()(C.byref(C.c_void_p()), LAYOUT, 0, 0, out, 10), SYMBOL)
    names = ("sizeof", "status", "prover", "proof_len", "queued_ms", "run_ms", "running_at_start", "info", "message",
             "message_size")
    return dict(zip(names, out))


def choose_prover(slots, tag: int) -> int:
    """choose_prover on a list of (idle, has_key, key tag, used) per prover, for a job with key tag `tag`."""
    out = (C.c_uint64 * (4 * len(slots)))(*[int(v) for s in slots for v in s])
    native.check(_fn()(C.byref(C.c_void_p()), CHOOSE, len(slots), tag, out, len(out)), SYMBOL)
    return _signed(out[0])


class CoreQueue:
    """One JobQueue with the scripted executor."""

    def __init__(self, provers: int):
        self.h = C.c_void_p()
        native.check(_fn()(C.byref(self.h), CREATE, provers, 0, None, 0), SYMBOL)

    def _op(self, op, a=0, b=0, n=0):
        out = (C.c_uint64 * max(n, 1))()
        rc = _fn()(C.byref(self.h), op, a, b, out, n)
        return rc, list(out)

    def submit(self, tag: int, n: int = 16) -> int:
        rc, out = self._op(SUBMIT, n, tag, 1)
        if rc != native.ZK_OK:
            raise native.ZkError(rc, "submit")
        return out[0]

    def release(self, job: int = 0):
        """Open job's gate (before or after it starts); 0: every gate, now and later."""
        self._op(RELEASE, job)

    @staticmethod
    def _delivery(rc, out):
        if rc != native.ZK_OK:
            return rc, None
        return rc, {"state": out[0], "prover": _signed(out[1]), "running_at_start": out[2], "start_seq": out[3],
                    "result": out[4], "times_ok": out[5] == 1 and out[6] == 1, "id": out[7]}

    def wait(self, job: int):
        return self._delivery(*self._op(WAIT, job, 0, 8))

    def poll(self, job: int):
        return self._delivery(*self._op(POLL, job, 0, 8))

    def wait_any(self):
        return self._delivery(*self._op(WAIT_ANY, 0, 0, 8))

    def cancel(self, job: int) -> int:
        return self._op(CANCEL, job)[0]

    def pause(self):
        self._op(PAUSE)

    def resume(self):
        self._op(RESUME)

    def stats(self) -> dict:
        _, out = self._op(STATS, 0, 0, 6)
        return dict(zip(("submitted", "completed", "cancelled", "queued", "running", "peak_running"), out))

    def state(self, job: int) -> int:
        return _signed(self._op(STATE, job, 0, 1)[1][0])

    def log(self) -> list:
        """(id, prover) in the order the executor saw the jobs."""
        _, out = self._op(LOG, 0, 0, 4096)
        return [(out[1 + 2 * i], _signed(out[2 + 2 * i])) for i in range(out[0])]

    def close(self):
        self._op(CLOSE)

    def join(self):
        self._op(JOIN)

    def destroy(self):
        if self.h:
            self._op(DESTROY)
            self.h = C.c_void_p()
