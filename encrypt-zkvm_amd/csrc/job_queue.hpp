// job_queue.hpp -- the scheduling core of zk_queue (queue.cpp): job ids and states, FIFO start order, which prover a job
// takes, pause / resume, wait / poll / wait-any, cancel and drain.  No HIP and no prover: the core is a template over
// the job payload, its result and an executor callable, and owns one worker thread per prover slot.  queue.cpp
// instantiates it with an executor that calls the blocking entry points on the worker's prover; the test entry point
// (the end of queue.cpp, zkvm_amd/queue_diag.py, tests/test_job_queue_cpu.py) and tools/tsan/job_queue_main.cpp drive it with
// executors of their own.
//
// States.  A job is QUEUED from submit until it is matched with a prover, RUNNING while the executor has it, then DONE;
// a QUEUED job that is cancelled (cancel, or close with the job still waiting) becomes CANCELLED without ever reaching
// the executor.  DONE and CANCELLED jobs wait to be delivered: wait, poll or wait_any hand each job out exactly once
// and forget its id.  Ids count up from 1 and are never reused.
//
// Matching.  Jobs start in submission order.  Whenever something changes (submit, a job finishing, resume) one step
// under the lock matches queued jobs with idle provers until either runs out, so a resume with k <= P jobs waiting
// marks k jobs RUNNING before any of them can complete.  The prover is chosen by choose_prover below.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/zkvm_gpu.h"

namespace zk {

// What a prover's per-key state (column hints, fixed-column snapshots) is keyed by: trace length and program hash.
struct JobKey {
    uint64_t n = 0;
    uint8_t hash[32] = {};
    bool operator==(const JobKey &o) const { return n == o.n && !memcmp(hash, o.hash, sizeof hash); }
};

enum JobState : int { JOB_QUEUED = 0, JOB_RUNNING = 1, JOB_DONE = 2, JOB_CANCELLED = 3 };

// One prover as the choice sees it.  used: a tick that grows with every job the queue finishes (0: never used).
struct ProverSlot {
    bool idle = true;
    bool has_key = false;
    JobKey last;
    uint64_t used = 0;
};

// The prover for a job with this key, or -1 when none is idle: among the idle provers the one whose last job had the
// same key (the most recently used of several), else the one used least recently (the lowest index among equals, so a
// fresh queue fills its provers in order).
inline int choose_prover(const ProverSlot *slots, int count, const JobKey &key) {
    int same = -1, lru = -1;
    for (int w = 0; w < count; w++) {
        if (!slots[w].idle) continue;
        if (slots[w].has_key && slots[w].last == key && (same < 0 || slots[w].used > slots[same].used)) same = w;
        if (lru < 0 || slots[w].used < slots[lru].used) lru = w;
    }
    return same >= 0 ? same : lru;
}

// What the core knows about a delivered job beside the executor's result.
struct JobInfo {
    int state = JOB_QUEUED;         // JOB_DONE or JOB_CANCELLED once delivered
    int prover = -1;                // the slot that ran it, -1 if none
    uint32_t running_at_start = 0;  // jobs already RUNNING when this one was matched
    uint64_t start_seq = 0;         // 1, 2, ... in the order jobs were matched (0: never started)
    float queued_ms = 0, run_ms = 0;  // submit -> matched (or cancelled); matched -> the executor returned
};

struct JobQueueStats {
    uint64_t submitted = 0, completed = 0, cancelled = 0;  // completed: jobs the executor has returned from
    uint32_t queued = 0, running = 0, peak_running = 0;
};

// Exec: void(int prover, Job &job, Result &result), called on prover's worker thread with no lock held.
template <class Job, class Result, class Exec>
class JobQueue {
  public:
    JobQueue(int provers, Exec exec) : exec_(std::move(exec)), slots_((size_t)provers), assigned_((size_t)provers, 0) {
        for (int w = 0; w < provers; w++) threads_.emplace_back([this, w] { worker(w); });
    }
    ~JobQueue() {
        close();
        join();
    }
    JobQueue(const JobQueue &) = delete;
    JobQueue &operator=(const JobQueue &) = delete;

    int provers() const { return (int)slots_.size(); }

    // ZK_OK and the job's id, or ZK_ERR_INVALID_ARG once the queue is closed.  Thread-safe, like every call here.
    int submit(const JobKey &key, Job job, uint64_t *id) {
        std::unique_lock<std::mutex> lk(mu_);
        if (closed_) return ZK_ERR_INVALID_ARG;
        const uint64_t i = next_id_++;
        Entry &e = jobs_[i];
        e.key = key;
        e.job = std::move(job);
        e.t_submit = Clock::now();
        fifo_.push_back(i);
        stats_.submitted++;
        stats_.queued++;
        *id = i;
        match();
        return ZK_OK;
    }

    void pause() {
        std::lock_guard<std::mutex> lk(mu_);
        paused_ = true;
    }
    void resume() {
        std::lock_guard<std::mutex> lk(mu_);
        paused_ = false;
        match();
    }

    // Blocks until job id is DONE or CANCELLED and hands it out.  ZK_ERR_INVALID_ARG: no such job (never submitted, or
    // delivered already -- also when another waiter took it first).
    int wait(uint64_t id, Result *res, JobInfo *info) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            auto it = jobs_.find(id);
            if (it == jobs_.end()) return ZK_ERR_INVALID_ARG;
            if (finished(it->second)) return deliver(it, res, info);
            done_cv_.wait(lk);
        }
    }
    // The same without blocking: ZK_ERR_PENDING while the job is QUEUED or RUNNING.
    int poll(uint64_t id, Result *res, JobInfo *info) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = jobs_.find(id);
        if (it == jobs_.end()) return ZK_ERR_INVALID_ARG;
        if (!finished(it->second)) return ZK_ERR_PENDING;
        return deliver(it, res, info);
    }
    // The first undelivered job to finish, in the order they finished.  ZK_ERR_INVALID_ARG when no job is pending or
    // undelivered (also when other waiters take the last one while this call waits).
    int wait_any(uint64_t *id, Result *res, JobInfo *info) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            if (jobs_.empty()) return ZK_ERR_INVALID_ARG;
            if (!finished_.empty()) {
                *id = finished_.front();
                return deliver(jobs_.find(*id), res, info);
            }
            done_cv_.wait(lk);
        }
    }
    // Only a QUEUED job can be cancelled; it is then delivered as JOB_CANCELLED.
    int cancel(uint64_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = jobs_.find(id);
        if (it == jobs_.end() || it->second.info.state != JOB_QUEUED) return ZK_ERR_INVALID_ARG;
        for (auto f = fifo_.begin(); f != fifo_.end(); ++f)
            if (*f == id) {
                fifo_.erase(f);
                break;
            }
        cancel_entry(id, it->second);
        done_cv_.notify_all();
        return ZK_OK;
    }
    // f(result, info) on an undelivered job once it has finished, under the lock: blocks like wait, delivers nothing.
    template <class F>
    int inspect(uint64_t id, F f) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            auto it = jobs_.find(id);
            if (it == jobs_.end()) return ZK_ERR_INVALID_ARG;
            if (finished(it->second)) return f(it->second.res, it->second.info);
            done_cv_.wait(lk);
        }
    }
    // The state of an undelivered job, or -1.
    int state(uint64_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = jobs_.find(id);
        return it == jobs_.end() ? -1 : it->second.info.state;
    }
    // f() under the lock if no job is QUEUED or RUNNING (settings that must not change under a job), else
    // ZK_ERR_INVALID_ARG.
    template <class F>
    int when_idle(F f) {
        std::lock_guard<std::mutex> lk(mu_);
        if (stats_.queued || stats_.running) return ZK_ERR_INVALID_ARG;
        return f();
    }
    JobQueueStats stats() const {
        std::lock_guard<std::mutex> lk(mu_);
        return stats_;
    }

    // Drain, in two steps so that a caller can act between them (the destructor runs both).  close: no job starts any
    // more, every QUEUED job becomes CANCELLED, submit is refused; returns at once.  join: waits for the RUNNING jobs
    // and ends the workers.  Finished jobs can still be delivered after either.
    void close() {
        std::lock_guard<std::mutex> lk(mu_);
        if (closed_) return;
        closed_ = true;
        while (!fifo_.empty()) {
            const uint64_t id = fifo_.front();
            fifo_.pop_front();
            cancel_entry(id, jobs_[id]);
        }
        work_cv_.notify_all();
        done_cv_.notify_all();
    }
    void join() {
        for (auto &t : threads_)
            if (t.joinable()) t.join();
    }

  private:
    typedef std::chrono::steady_clock Clock;
    struct Entry {
        JobKey key;
        Job job;
        Result res;
        JobInfo info;
        Clock::time_point t_submit, t_start;
    };
    typedef typename std::map<uint64_t, Entry>::iterator Iter;

    static float ms(Clock::time_point a, Clock::time_point b) {
        return std::chrono::duration<float, std::milli>(b - a).count();
    }
    static bool finished(const Entry &e) { return e.info.state == JOB_DONE || e.info.state == JOB_CANCELLED; }

    // (lock held) queued jobs meet idle provers, in submission order, until either runs out
    void match() {
        bool any = false;
        while (!paused_ && !closed_ && !fifo_.empty()) {
            const uint64_t id = fifo_.front();
            Entry &e = jobs_[id];
            const int w = choose_prover(slots_.data(), (int)slots_.size(), e.key);
            if (w < 0) break;
            fifo_.pop_front();
            slots_[(size_t)w].idle = false;
            assigned_[(size_t)w] = id;
            e.t_start = Clock::now();
            e.info.state = JOB_RUNNING;
            e.info.prover = w;
            e.info.running_at_start = stats_.running;
            e.info.start_seq = ++start_seq_;
            e.info.queued_ms = ms(e.t_submit, e.t_start);
            stats_.queued--;
            stats_.running++;
            if (stats_.running > stats_.peak_running) stats_.peak_running = stats_.running;
            any = true;
        }
        if (any) work_cv_.notify_all();
    }
    void cancel_entry(uint64_t id, Entry &e) {
        e.info.state = JOB_CANCELLED;
        e.info.queued_ms = ms(e.t_submit, Clock::now());
        stats_.queued--;
        stats_.cancelled++;
        finished_.push_back(id);
    }
    int deliver(Iter it, Result *res, JobInfo *info) {
        if (res) *res = std::move(it->second.res);
        if (info) *info = it->second.info;
        for (auto f = finished_.begin(); f != finished_.end(); ++f)
            if (*f == it->first) {
                finished_.erase(f);
                break;
            }
        jobs_.erase(it);
        // a wait_any left with nothing to wait for must see that
        if (jobs_.empty()) done_cv_.notify_all();
        return ZK_OK;
    }
    void worker(int w) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            work_cv_.wait(lk, [&] { return assigned_[(size_t)w] != 0 || closed_; });
            const uint64_t id = assigned_[(size_t)w];
            if (!id) return;  // closed, and nothing was matched with this prover
            Entry &e = jobs_.find(id)->second;  // (a RUNNING job is never delivered: the entry stays put)
            lk.unlock();
            exec_(w, e.job, e.res);
            lk.lock();
            e.info.state = JOB_DONE;
            e.info.run_ms = ms(e.t_start, Clock::now());
            ProverSlot &s = slots_[(size_t)w];
            s.idle = true;
            s.has_key = true;
            s.last = e.key;
            s.used = ++tick_;
            assigned_[(size_t)w] = 0;
            stats_.running--;
            stats_.completed++;
            finished_.push_back(id);
            match();
            done_cv_.notify_all();
        }
    }

    Exec exec_;
    mutable std::mutex mu_;
    std::condition_variable work_cv_, done_cv_;
    std::map<uint64_t, Entry> jobs_;  // every undelivered job (node addresses are stable)
    std::deque<uint64_t> fifo_;       // the QUEUED ones, in submission order
    std::deque<uint64_t> finished_;   // DONE and CANCELLED ones, in the order they finished
    std::vector<ProverSlot> slots_;
    std::vector<uint64_t> assigned_;  // per prover: the job matched with it (0: none)
    std::vector<std::thread> threads_;
    JobQueueStats stats_;
    uint64_t next_id_ = 1, start_seq_ = 0, tick_ = 0;
    bool paused_ = false, closed_ = false;
};

}  // namespace zk
