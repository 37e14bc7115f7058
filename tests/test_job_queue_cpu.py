"""The proof queue's scheduling core (csrc/job_queue.hpp) driven through the library's test entry point with a scripted
executor (zkvm_amd/queue_diag.py): a job is a key tag, the executor logs (id, prover), holds the job until the test
opens its gate, and returns tag + 1000.  No GPU and no HIP call, and nothing here depends on timing: a job is matched
with its prover under the core's lock at submit / completion / resume, so what a call returns is already decided when it
returns, and every wait is on a job whose gate is open."""
import ctypes as C
import re
from pathlib import Path

import pytest

from zkvm_amd import native, queue_diag
from zkvm_amd.queue_diag import CANCELLED, DONE, QUEUED, RUNNING, CoreQueue, choose_prover

ROOT = Path(__file__).resolve().parent.parent
OK, INVALID, PENDING = native.ZK_OK, native.ZK_ERR_INVALID_ARG, native.ZK_ERR_PENDING


@pytest.fixture
def make():
    made = []

    def _make(provers):
        q = CoreQueue(provers)
        made.append(q)
        return q

    yield _make
    for q in made:
        q.release()  # nothing may stay behind a gate when the workers are joined
        q.destroy()


def finish(q, job):
    """Open the job's gate and consume it."""
    q.release(job)
    rc, d = q.wait(job)
    assert rc == OK and d["state"] == DONE and d["id"] == job and d["times_ok"]
    return d


def test_status_codes_and_symbol():
    assert (native.ZK_ERR_PENDING, native.ZK_ERR_CANCELLED) == (-6, -7)
    header = (ROOT / "include" / "zkvm_gpu.h").read_text()
    assert re.search(r"#define ZK_ERR_PENDING\s+-6\b", header) and re.search(r"#define ZK_ERR_CANCELLED\s+-7\b", header)
    assert hasattr(native.lib(), queue_diag.SYMBOL)
    for name in native.EXPORTED:
        if name.startswith("zk_queue_"):
            assert hasattr(native.lib(), name), name
    assert sum(name.startswith("zk_queue_") for name in native.EXPORTED) == 16


def test_job_result_layout_matches_ctypes():
    lay = queue_diag.job_result_layout()
    R = native.JobResult
    assert lay["sizeof"] == C.sizeof(R) == 568
    for f in ("status", "prover", "proof_len", "queued_ms", "run_ms", "running_at_start", "info", "message"):
        assert lay[f] == getattr(R, f).offset, f
    assert lay["message_size"] == R.message.size == 512
    assert R.info.size == C.sizeof(native.ProofInfo) == 24


def test_fifo_start_order_one_prover(make):
    q = make(1)
    ids = [q.submit(tag) for tag in (7, 3, 9, 3)]
    assert ids == [1, 2, 3, 4]
    assert [q.state(i) for i in ids] == [RUNNING, QUEUED, QUEUED, QUEUED]
    got = [finish(q, i) for i in ids]
    assert [d["start_seq"] for d in got] == [1, 2, 3, 4]
    assert [d["result"] for d in got] == [1007, 1003, 1009, 1003]
    assert q.log() == [(i, 0) for i in ids]


def test_fifo_start_order_two_provers(make):
    q = make(2)
    ids = [q.submit(10 + k) for k in range(5)]
    assert [q.state(i) for i in ids] == [RUNNING, RUNNING, QUEUED, QUEUED, QUEUED]
    d2 = finish(q, ids[1])  # the SECOND job finishes first: the third starts, on its prover
    assert (d2["prover"], d2["start_seq"], d2["running_at_start"]) == (1, 2, 1)
    assert [q.state(i) for i in ids[2:]] == [RUNNING, QUEUED, QUEUED]
    d1 = finish(q, ids[0])
    assert (d1["prover"], d1["start_seq"], d1["running_at_start"]) == (0, 1, 0)
    assert [q.state(i) for i in ids[3:]] == [RUNNING, QUEUED]
    rest = [finish(q, i) for i in ids[2:]]
    assert [d["start_seq"] for d in rest] == [3, 4, 5]
    assert [d["prover"] for d in rest[:2]] == [1, 0]
    assert all(d["running_at_start"] == 1 for d in rest)  # each started while exactly one other job ran
    assert [i for i, _ in q.log()] == ids
    assert q.stats() == {"submitted": 5, "completed": 5, "cancelled": 0, "queued": 0, "running": 0, "peak_running": 2}


def warmed(make, order):
    """Three provers whose last keys are tags 1, 2, 3 (prover w: tag w + 1), finished in `order` (job ids)."""
    q = make(3)
    ids = [q.submit(tag) for tag in (1, 2, 3)]
    assert ids == [1, 2, 3]
    for i in order:
        assert finish(q, i)["prover"] == i - 1  # a fresh queue fills its provers in index order
    return q


def test_matching_key_beats_least_recently_used(make):
    q = warmed(make, [1, 2, 3])  # prover 0 is the least recently used, prover 2 the most
    a = q.submit(3)
    b = q.submit(9)  # no prover has seen tag 9: the least recently used of the idle ones (0, 1)
    c = q.submit(2)  # prover 1 is the only idle one, and it matches
    assert [q.state(j) for j in (a, b, c)] == [RUNNING] * 3
    assert [finish(q, j)["prover"] for j in (a, b, c)] == [2, 0, 1]


def test_same_tag_other_length_is_another_key(make):
    q = warmed(make, [1, 2, 3])
    a = q.submit(3, n=32)  # the warm-up jobs had length 16
    assert finish(q, a)["prover"] == 0


def test_no_match_takes_least_recently_used(make):
    q = warmed(make, [3, 1, 2])  # finished in this order: prover 2 is now the least recently used, then 0, then 1
    a, b, c = q.submit(7), q.submit(8), q.submit(9)
    got = {j: finish(q, j)["prover"] for j in (a, b, c)}
    assert got == {a: 2, b: 0, c: 1}


def test_choose_prover_pure():
    idle = lambda tag, used, has=1: (1, has, tag, used)  # noqa: E731
    busy = lambda tag, used: (0, 1, tag, used)  # noqa: E731
    assert choose_prover([idle(0, 0, 0), idle(0, 0, 0), idle(0, 0, 0)], 5) == 0  # fresh: the lowest index
    assert choose_prover([idle(1, 3), idle(2, 1), idle(5, 2)], 5) == 2  # the match, though 1 is older
    assert choose_prover([idle(1, 3), idle(2, 1), idle(5, 2)], 6) == 1  # no match: the least recently used
    assert choose_prover([idle(1, 3), idle(2, 1), busy(5, 2)], 5) == 1  # the match is busy
    assert choose_prover([busy(1, 3), busy(2, 1), busy(5, 2)], 5) == -1  # none idle
    assert choose_prover([idle(5, 1), idle(5, 4), idle(2, 0, 0)], 5) == 1  # two matches: the warmer one
    assert choose_prover([idle(5, 7, 0), idle(6, 1)], 5) == 1  # a tag without has_key is no match
    assert choose_prover([busy(1, 0), idle(9, 9)], 1) == 1


@pytest.mark.parametrize("k", [1, 2, 3])
def test_resume_matches_k_jobs_in_one_step(make, k):
    q = make(3)
    q.pause()
    ids = [q.submit(20 + j) for j in range(k)]
    assert [q.state(i) for i in ids] == [QUEUED] * k
    s = q.stats()
    assert (s["queued"], s["running"], s["peak_running"]) == (k, 0, 0)
    q.resume()
    # no gate is open yet: nothing can have completed, and all k are running
    s = q.stats()
    assert (s["queued"], s["running"], s["peak_running"], s["completed"]) == (0, k, k, 0)
    assert [q.state(i) for i in ids] == [RUNNING] * k
    got = [finish(q, i) for i in ids]
    assert sorted(d["running_at_start"] for d in got) == list(range(k))
    assert sorted(d["prover"] for d in got) == list(range(k))
    assert q.stats()["peak_running"] == k


def test_resume_with_more_jobs_than_provers(make):
    q = make(3)
    q.pause()
    ids = [q.submit(j) for j in range(5)]
    q.resume()
    assert [q.state(i) for i in ids] == [RUNNING] * 3 + [QUEUED] * 2
    assert q.stats()["peak_running"] == 3
    for i in ids:
        finish(q, i)
    assert q.stats()["peak_running"] == 3


def test_paused_queue_starts_nothing_and_running_jobs_finish(make):
    q = make(2)
    a = q.submit(1)
    q.pause()
    b = q.submit(2)
    assert (q.state(a), q.state(b)) == (RUNNING, QUEUED)
    finish(q, a)  # a running job finishes under pause ...
    assert q.state(b) == QUEUED  # ... and nothing starts, with both provers idle
    q.resume()
    assert q.state(b) == RUNNING
    finish(q, b)


def test_wait_and_poll_deliver_once(make):
    q = make(1)
    a, b = q.submit(1), q.submit(2)
    assert q.poll(a) == (PENDING, None) and q.poll(b) == (PENDING, None)  # running / queued
    assert q.wait(99) == (INVALID, None) and q.poll(99) == (INVALID, None)  # never submitted
    finish(q, a)
    assert q.wait(a) == (INVALID, None) and q.poll(a) == (INVALID, None) and q.state(a) == -1
    q.release(b)
    rc, d = q.wait(b)
    assert rc == OK and d["result"] == 1002
    assert q.poll(b) == (INVALID, None) and q.wait(b) == (INVALID, None)


def test_wait_any_delivers_each_job_once_in_finish_order(make):
    q = make(1)  # one prover: the jobs finish in submission order
    ids = [q.submit(30 + k) for k in range(5)]
    q.release()
    got = [q.wait_any() for _ in ids]
    assert [rc for rc, _ in got] == [OK] * 5
    assert [d["id"] for _, d in got] == ids
    assert [d["result"] for _, d in got] == [1030 + k for k in range(5)]
    assert q.wait_any() == (INVALID, None)  # nothing pending
    assert all(q.wait(i) == (INVALID, None) for i in ids)


def test_wait_any_on_an_empty_queue(make):
    assert make(2).wait_any() == (INVALID, None)


def test_poll_delivers_a_finished_job(make):
    q = make(1)
    a, b = q.submit(1), q.submit(2)
    q.release(a)
    q.release(b)
    assert q.wait(b)[0] == OK  # b ran after a: a has finished
    rc, d = q.poll(a)
    assert rc == OK and d["id"] == a and d["state"] == DONE and d["result"] == 1001
    assert q.poll(a) == (INVALID, None)


def test_cancel_a_queued_job(make):
    q = make(1)
    a, b, c = q.submit(1), q.submit(2), q.submit(3)
    assert q.cancel(b) == OK
    assert q.state(b) == CANCELLED
    assert q.cancel(b) == INVALID  # not queued any more
    s = q.stats()
    assert (s["queued"], s["running"], s["cancelled"]) == (1, 1, 1)
    rc, d = q.wait(b)  # delivered without any gate opened
    assert rc == OK and (d["state"], d["prover"], d["start_seq"], d["result"]) == (CANCELLED, -1, 0, 0)
    assert q.wait(b) == (INVALID, None)
    finish(q, a)
    assert finish(q, c)["start_seq"] == 2
    assert [i for i, _ in q.log()] == [a, c]  # the executor never saw b
    s = q.stats()
    assert (s["submitted"], s["completed"], s["cancelled"]) == (3, 2, 1)


def test_cancelled_job_comes_out_of_wait_any(make):
    q = make(1)
    a, b = q.submit(1), q.submit(2)
    assert q.cancel(b) == OK
    rc, d = q.wait_any()  # b finished (as cancelled) first; a is still behind its gate
    assert rc == OK and d["id"] == b and d["state"] == CANCELLED
    finish(q, a)


def test_cancel_of_a_running_or_consumed_job_is_refused(make):
    q = make(1)
    a = q.submit(1)
    assert q.state(a) == RUNNING and q.cancel(a) == INVALID
    assert q.state(a) == RUNNING
    finish(q, a)
    assert q.cancel(a) == INVALID  # consumed
    assert q.cancel(12345) == INVALID  # never submitted
    b, c = q.submit(2), q.submit(3)
    q.release(b)
    q.release(c)
    assert q.wait(c)[0] == OK
    assert q.state(b) == DONE and q.cancel(b) == INVALID  # finished, not yet consumed
    assert q.wait(b)[0] == OK


def test_drain_cancels_queued_and_completes_running(make):
    q = make(2)
    ids = [q.submit(k) for k in range(4)]
    q.close()  # the first half of a destroy: returns at once
    assert [q.state(i) for i in ids] == [RUNNING, RUNNING, CANCELLED, CANCELLED]
    with pytest.raises(native.ZkError):
        q.submit(9)
    q.release(ids[0])
    q.release(ids[1])
    q.join()  # the second half: the running jobs complete, the workers end
    got = [q.wait(i) for i in ids]  # finished jobs can still be collected
    assert [d["state"] for _, d in got] == [DONE, DONE, CANCELLED, CANCELLED]
    assert sorted(i for i, _ in q.log()) == ids[:2]
    s = q.stats()
    assert (s["completed"], s["cancelled"], s["queued"], s["running"]) == (2, 2, 0, 0)


def test_destroy_of_a_paused_queue_returns():
    q = CoreQueue(3)
    q.pause()
    for k in range(4):
        q.submit(k)
    q.destroy()  # close + join + free: nothing ran, nothing to wait for


def test_ids_are_never_reused(make):
    q = make(2)
    seen = []
    for _ in range(6):
        a, b, c = q.submit(1), q.submit(2), q.submit(3)
        seen += [a, b, c]
        assert q.cancel(c) == OK
        finish(q, a)
        finish(q, b)
        assert q.wait(c)[1]["state"] == CANCELLED
    assert seen == list(range(1, 19))


def test_queue_entry_points_refuse_null_arguments_without_a_gpu():
    L = native.lib()
    bad = native.ZK_ERR_INVALID_ARG
    res, job = native.JobResult(), C.c_uint64(0)
    assert L.zk_queue_create(0, 1 << 10, 8, 3, None) == bad
    h = C.c_void_p()
    assert L.zk_queue_create(0, 1 << 10, 8, 0, C.byref(h)) == bad and not h  # 1 to 8 provers
    assert L.zk_queue_create(0, 1 << 10, 8, 9, C.byref(h)) == bad and not h
    assert b"1 to 8" in L.zk_last_error()
    L.zk_queue_destroy(None)
    for fn in (L.zk_queue_pause, L.zk_queue_resume):
        assert fn(None) == bad
    assert L.zk_queue_set_validate(None, 1) == bad and L.zk_queue_set_validate_degrees(None, 1) == bad
    assert L.zk_queue_submit_columns(None, None, 16, None, None, None, 0, C.byref(job)) == bad
    assert L.zk_queue_submit_device(None, None, 16, None, None, None, 0, C.byref(job)) == bad
    assert L.zk_queue_submit_vm(None, None, None, 0, None, 0, 5, 16, None, None, None, 0, None, None, C.byref(job)) == bad
    assert L.zk_queue_wait(None, 1, C.byref(res)) == bad and L.zk_queue_poll(None, 1, C.byref(res)) == bad
    assert L.zk_queue_wait_any(None, C.byref(job), C.byref(res)) == bad and L.zk_queue_cancel(None, 1) == bad
    assert L.zk_queue_job_validation(None, 1, None) == bad and L.zk_queue_job_degrees(None, 1, None) == bad
    assert L.zk_queue_stats(None, None, None, None, None, None) == bad
    assert job.value == 0
