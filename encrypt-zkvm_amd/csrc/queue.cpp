// queue.cpp -- zk_queue (include/zkvm_gpu.h "proof queue"): P pooled provers of one device, one worker thread bound to
// each, and the scheduling core of job_queue.hpp instantiated with an executor that runs the blocking entry points
// (zk_prove_columns, zk_prove_device, zk_vm_prove) on the worker's prover.  Host code only: no kernel, no stream and
// no device memory of its own; the proof path is the blocking calls', unchanged.  The core's test entry point
// (zk_diag_job_queue, a scripted executor and no HIP call) is at the end of the file.
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "job_queue.hpp"
#include "prover_internal.hpp"
#include "vm_internal.hpp"

using namespace zk;

namespace {

// One job: the arguments of its blocking call, with what the header says is copied at submit held by value.
struct QueueJob {
    enum Kind { COLUMNS, DEVICE, VM } kind = COLUMNS;
    const uint8_t *cols[W] = {};
    const void *d_trace = nullptr;
    size_t n = 0;
    zk_options opt = {};
    zk_pub_inputs pub = {};
    uint8_t *proof_out = nullptr;
    size_t proof_cap = 0;
    // VM jobs
    zk_program *prog = nullptr;
    std::vector<uint8_t> public_in, secret;
    size_t num_secret = 0;
    uint32_t lwe_size = 0, delta = 0;
    bool has_last = false;
    uint8_t last_row[W * 16] = {};
    uint8_t *outputs = nullptr, *program_hash = nullptr;
};

struct QueueResult {
    int status = ZK_ERR_CANCELLED;
    size_t proof_len = 0;
    zk_proof_info info = {};
    std::string message;
    std::unique_ptr<zk_validation> val;  // the reports of the checks that ran during the job
    std::unique_ptr<zk_degrees> deg;
};

struct QueueExec {
    zk_queue *q;
    void operator()(int w, QueueJob &job, QueueResult &res) const;
};

}  // namespace

struct zk_queue {
    int device = 0;
    size_t max_n = 0;
    uint32_t max_b = 0;
    bool validate = false, validate_degrees = false;
    std::vector<zk_prover *> provers;
    std::unique_ptr<JobQueue<QueueJob, QueueResult, QueueExec>> core;
};

void QueueExec::operator()(int w, QueueJob &job, QueueResult &res) const {
    zk_prover *p = q->provers[(size_t)w];
    size_t len = job.proof_cap;
    g_err.clear();
    int rc;
    switch (job.kind) {
    case QueueJob::COLUMNS:
        rc = zk_prove_columns(p, job.cols, job.n, &job.opt, &job.pub, job.proof_out, &len);
        break;
    case QueueJob::DEVICE:
        rc = zk_prove_device(p, job.d_trace, job.n, &job.opt, &job.pub, job.proof_out, &len, nullptr, nullptr);
        break;
    default:
        rc = zk_vm_prove(p, job.prog, job.public_in.data(), job.public_in.size(), job.secret.data(), job.num_secret,
                         job.lwe_size, job.delta, job.has_last ? job.last_row : nullptr, &job.opt, job.proof_out, &len,
                         job.outputs, job.program_hash);
        break;
    }
    res.status = rc;
    res.proof_len = len;
    if (rc != ZK_OK) res.message = g_err;
    (void)zk_prover_proof_info(p, &res.info);
    // The prover keeps the report of the last check that ran on it; with the switch on, that is this job's unless the
    // call ended before the check (an argument error; the degree check does not run after a failed validation)
    const bool ran = rc != ZK_ERR_INVALID_ARG;
    if (q->validate && ran) {
        res.val.reset(new zk_validation);
        if (zk_prover_validation(p, res.val.get()) != ZK_OK) res.val.reset();
    }
    if (q->validate_degrees && ran && rc != ZK_ERR_TRACE) {
        res.deg.reset(new zk_degrees);
        if (zk_prover_degrees(p, res.deg.get()) != ZK_OK) res.deg.reset();
    }
}

int zk_queue_create(int device, size_t max_trace_len, uint32_t max_blowup, int provers, zk_queue **out) {
    if (!out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (provers < 1 || provers > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "a queue has 1 to 8 provers");
    std::unique_ptr<zk_queue> q(new zk_queue);
    q->device = device;
    q->max_n = max_trace_len;
    q->max_b = max_blowup;
    for (int w = 0; w < provers; w++) {
        zk_prover *p = nullptr;
        const int rc = zk_prover_acquire(device, max_trace_len, max_blowup, &p);
        if (rc != ZK_OK) {  // (the message is zk_prover_acquire's)
            for (zk_prover *r : q->provers) zk_prover_release(r);
            return rc;
        }
        q->provers.push_back(p);
    }
    // a pooled prover may come with another owner's settings: a queue starts with both checks off, as a new prover does
    for (zk_prover *p : q->provers) {
        (void)zk_prover_set_validate(p, 0);
        (void)zk_prover_set_validate_degrees(p, 0);
    }
    q->core.reset(new JobQueue<QueueJob, QueueResult, QueueExec>(provers, QueueExec{q.get()}));
    *out = q.release();
    return ZK_OK;
}

void zk_queue_destroy(zk_queue *q) {
    if (!q) return;
    q->core.reset();  // cancels the queued jobs, waits for the running ones, ends the workers
    for (zk_prover *p : q->provers) {
        (void)zk_prover_set_validate(p, 0);
        (void)zk_prover_set_validate_degrees(p, 0);
        zk_prover_release(p);
    }
    delete q;
}

static int set_switch(zk_queue *q, bool zk_queue::*member, int (*set)(zk_prover *, int), int on) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    const int rc = q->core->when_idle([&] {
        for (zk_prover *p : q->provers) ZK_TRY(set(p, on));
        q->*member = on != 0;
        return (int)ZK_OK;
    });
    if (rc == ZK_ERR_INVALID_ARG && g_err.empty()) g_err = "the queue has pending jobs";
    return rc;
}

int zk_queue_set_validate(zk_queue *q, int on) {
    g_err.clear();
    return set_switch(q, &zk_queue::validate, zk_prover_set_validate, on);
}

int zk_queue_set_validate_degrees(zk_queue *q, int on) {
    g_err.clear();
    return set_switch(q, &zk_queue::validate_degrees, zk_prover_set_validate_degrees, on);
}

int zk_queue_pause(zk_queue *q) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    q->core->pause();
    return ZK_OK;
}

int zk_queue_resume(zk_queue *q) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    q->core->resume();
    return ZK_OK;
}

static int submit(zk_queue *q, const uint8_t *hash32, uint64_t n, QueueJob &&job, uint64_t *id) {
    JobKey key;
    key.n = n;
    memcpy(key.hash, hash32, sizeof key.hash);
    if (q->core->submit(key, std::move(job), id) != ZK_OK) ZK_FAIL(ZK_ERR_INVALID_ARG, "the queue is closed");
    return ZK_OK;
}

int zk_queue_submit_columns(zk_queue *q, const uint8_t *const *columns, size_t n, const zk_options *opt,
                            const zk_pub_inputs *pub, uint8_t *proof_out, size_t proof_cap, uint64_t *job) {
    if (!q || !job || !columns || !proof_out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < W; c++)
        if (!columns[c]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null trace column");
    ZK_TRY(check_prove_args(n, q->max_n, q->max_b, opt, pub));
    QueueJob j;
    j.kind = QueueJob::COLUMNS;
    memcpy(j.cols, columns, sizeof j.cols);
    j.n = n, j.opt = *opt, j.pub = *pub, j.proof_out = proof_out, j.proof_cap = proof_cap;
    return submit(q, &pub->program_hash[0][0], n, std::move(j), job);
}

int zk_queue_submit_device(zk_queue *q, const void *d_trace, size_t n, const zk_options *opt,
                           const zk_pub_inputs *pub, uint8_t *proof_out, size_t proof_cap, uint64_t *job) {
    if (!q || !job || !d_trace || !proof_out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_TRY(check_prove_args(n, q->max_n, q->max_b, opt, pub));
    QueueJob j;
    j.kind = QueueJob::DEVICE;
    j.d_trace = d_trace;
    j.n = n, j.opt = *opt, j.pub = *pub, j.proof_out = proof_out, j.proof_cap = proof_cap;
    return submit(q, &pub->program_hash[0][0], n, std::move(j), job);
}

int zk_queue_submit_vm(zk_queue *q, zk_program *prog, const uint8_t *public_in, size_t num_public,
                       const uint8_t *secret, size_t num_secret, uint32_t lwe_size, uint32_t delta,
                       const uint8_t *last_row, const zk_options *opt, uint8_t *proof_out, size_t proof_cap,
                       uint8_t *outputs, uint8_t *program_hash, uint64_t *job) {
    if (!q || !job || !prog || !opt || !proof_out || (num_secret && !secret) || (num_public && !public_in))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    QueueJob j;
    j.kind = QueueJob::VM;
    j.prog = prog;
    j.public_in.assign(public_in, public_in + num_public);
    // the blocking call reads lwe_size elements per ciphertext; a width it would refuse copies nothing (and is refused
    // by the job's own call)
    const size_t width = lwe_size >= 1 && lwe_size <= 5 ? lwe_size : 0;
    if (width) j.secret.assign(secret, secret + num_secret * width * 16);
    j.num_secret = num_secret, j.lwe_size = lwe_size, j.delta = delta;
    if (last_row) {
        j.has_last = true;
        memcpy(j.last_row, last_row, sizeof j.last_row);
    }
    j.opt = *opt, j.proof_out = proof_out, j.proof_cap = proof_cap, j.outputs = outputs, j.program_hash = program_hash;
    uint8_t hash[32];
    fe_to_bytes(prog->P.hash[0], hash);
    fe_to_bytes(prog->P.hash[1], hash + 16);
    return submit(q, hash, prog->P.trace_len, std::move(j), job);
}

static void fill_result(const QueueResult &r, const JobInfo &info, zk_job_result *out) {
    memset(out, 0, sizeof *out);
    out->status = info.state == JOB_CANCELLED ? ZK_ERR_CANCELLED : r.status;
    out->prover = info.prover;
    out->proof_len = info.state == JOB_CANCELLED ? 0 : r.proof_len;
    out->queued_ms = info.queued_ms;
    out->run_ms = info.run_ms;
    out->running_at_start = info.running_at_start;
    out->info = r.info;
    const std::string &m = info.state == JOB_CANCELLED ? std::string("the job was cancelled before it started") : r.message;
    strncpy(out->message, m.c_str(), sizeof out->message - 1);
}

// the tail of the three delivering calls: the caller's zk_last_error() is the job's message
static int delivered(int rc, const QueueResult &r, const JobInfo &info, zk_job_result *res) {
    if (rc == ZK_ERR_PENDING) ZK_FAIL(rc, "the job has not finished");
    if (rc != ZK_OK) ZK_FAIL(rc, "no such job (never submitted, or delivered already)");
    zk_job_result tmp;
    fill_result(r, info, &tmp);
    g_err = tmp.message;
    if (res) *res = tmp;
    return ZK_OK;
}

int zk_queue_wait(zk_queue *q, uint64_t job, zk_job_result *res) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    QueueResult r;
    JobInfo info;
    return delivered(q->core->wait(job, &r, &info), r, info, res);
}

int zk_queue_poll(zk_queue *q, uint64_t job, zk_job_result *res) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    QueueResult r;
    JobInfo info;
    return delivered(q->core->poll(job, &r, &info), r, info, res);
}

int zk_queue_wait_any(zk_queue *q, uint64_t *job, zk_job_result *res) {
    if (!q || !job) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    QueueResult r;
    JobInfo info;
    const int rc = q->core->wait_any(job, &r, &info);
    if (rc != ZK_OK) ZK_FAIL(rc, "no job is pending or undelivered");
    return delivered(rc, r, info, res);
}

int zk_queue_cancel(zk_queue *q, uint64_t job) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (q->core->cancel(job) != ZK_OK) ZK_FAIL(ZK_ERR_INVALID_ARG, "only a job that has not started can be cancelled");
    return ZK_OK;
}

int zk_queue_job_validation(zk_queue *q, uint64_t job, zk_validation *out) {
    if (!q || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    const int rc = q->core->inspect(job, [&](const QueueResult &r, const JobInfo &) {
        if (!r.val) return (int)ZK_ERR_INVALID_ARG;
        *out = *r.val;
        return (int)ZK_OK;
    });
    if (rc != ZK_OK) ZK_FAIL(rc, "no such undelivered job, or no validation ran during it");
    return ZK_OK;
}

int zk_queue_job_degrees(zk_queue *q, uint64_t job, zk_degrees *out) {
    if (!q || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    const int rc = q->core->inspect(job, [&](const QueueResult &r, const JobInfo &) {
        if (!r.deg) return (int)ZK_ERR_INVALID_ARG;
        *out = *r.deg;
        return (int)ZK_OK;
    });
    if (rc != ZK_OK) ZK_FAIL(rc, "no such undelivered job, or no degree check ran during it");
    return ZK_OK;
}

int zk_queue_stats(const zk_queue *q, uint64_t *submitted, uint64_t *completed, uint32_t *queued, uint32_t *running,
                   uint32_t *peak_running) {
    if (!q) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    const JobQueueStats s = q->core->stats();
    if (submitted) *submitted = s.submitted;
    if (completed) *completed = s.completed;
    if (queued) *queued = s.queued;
    if (running) *running = s.running;
    if (peak_running) *peak_running = s.peak_running;
    return ZK_OK;
}

// ---------------------------------------------------------------- the core's test entry point
// zk_diag_job_queue drives job_queue.hpp with a scripted executor: a job is a tag, and the executor appends (id, prover)
// to a log, then holds the job until the test releases it (a gate per job, which may be opened before the job starts),
// and returns tag + 1000 as its result.  No GPU and no HIP call.  One multiplexed entry: (handle, op, a, b, out, cap).
//   0 CREATE   a = provers                      -> *handle
//   1 SUBMIT   a = key length, b = key hash tag -> out[0] = id; the job's tag is b
//   2 RELEASE  a = id (0: every job, now and later)
//   3 WAIT     a = id    -> out[0..7] = state, prover, running_at_start, start_seq, result, queued_ms >= 0, run_ms >= 0,
//   4 POLL     a = id       the id delivered (all three calls; the call's status is the core's)
//   5 WAIT_ANY
//   6 CANCEL   a = id
//   7 PAUSE    8 RESUME
//   9 STATS    -> out[0..5] = submitted, completed, cancelled, queued, running, peak_running
//  10 STATE    a = id -> out[0] = state (-1: unknown)
//  11 LOG      -> out[0] = entries, then (id, prover) pairs in the order the executor saw them
//  12 CLOSE    13 JOIN    14 DESTROY (close + join + free)
//  15 LAYOUT   -> out[0..9] = sizeof(zk_job_result), offsets of status, prover, proof_len, queued_ms, run_ms,
//                 running_at_start, info, message, sizeof(message)
//  16 CHOOSE   a = count, b = key tag, out (in/out): per prover (idle, has_key, key tag, used) -> out[0] = the choice
namespace {
struct DiagJob {
    uint64_t tag = 0;
};
struct DiagShared {
    std::mutex mu;
    std::condition_variable cv;
    std::map<uint64_t, bool> open;  // the released gates, by job id
    bool open_all = false;
    std::vector<std::pair<uint64_t, int>> log;
};
struct DiagExec {
    DiagShared *S;
    void operator()(int w, std::pair<uint64_t, DiagJob> &job, uint64_t &res) const {
        std::unique_lock<std::mutex> lk(S->mu);
        S->log.emplace_back(job.first, w);
        S->cv.wait(lk, [&] { return S->open_all || S->open.count(job.first); });
        res = job.second.tag + 1000;
    }
};
struct DiagQueue {
    DiagShared S;
    // the job carries its own id for the log: ids are handed out in submit order, which the one submitting test
    // thread knows before the call (next)
    std::unique_ptr<JobQueue<std::pair<uint64_t, DiagJob>, uint64_t, DiagExec>> core;
    uint64_t next = 1;
    std::mutex submit_mu;
};
static JobKey diag_key(uint64_t n, uint64_t tag) {
    JobKey k;
    k.n = n;
    memcpy(k.hash, &tag, sizeof tag);
    return k;
}
}  // namespace

extern "C" int zk_diag_job_queue(void **handle, int op, uint64_t a, uint64_t b, uint64_t *out, size_t cap) {
    if (!handle) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_job_queue: null handle");
    if (op == 15) {
        if (!out || cap < 10) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        out[0] = sizeof(zk_job_result);
        out[1] = offsetof(zk_job_result, status), out[2] = offsetof(zk_job_result, prover);
        out[3] = offsetof(zk_job_result, proof_len), out[4] = offsetof(zk_job_result, queued_ms);
        out[5] = offsetof(zk_job_result, run_ms), out[6] = offsetof(zk_job_result, running_at_start);
        out[7] = offsetof(zk_job_result, info), out[8] = offsetof(zk_job_result, message);
        out[9] = sizeof(((zk_job_result *)nullptr)->message);
        return ZK_OK;
    }
    if (op == 16) {
        if (!out || a < 1 || a > 8 || cap < 4 * a) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_job_queue: 1 to 8 provers, 4 values each");
        ProverSlot slots[8];
        for (uint64_t w = 0; w < a; w++) {
            slots[w].idle = out[4 * w] != 0, slots[w].has_key = out[4 * w + 1] != 0;
            slots[w].last = diag_key(16, out[4 * w + 2]), slots[w].used = out[4 * w + 3];
        }
        out[0] = (uint64_t)(int64_t)choose_prover(slots, (int)a, diag_key(16, b));
        return ZK_OK;
    }
    if (op == 0) {
        if (a < 1 || a > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_job_queue: 1 to 8 provers");
        DiagQueue *D = new DiagQueue;
        D->core.reset(new JobQueue<std::pair<uint64_t, DiagJob>, uint64_t, DiagExec>((int)a, DiagExec{&D->S}));
        *handle = D;
        return ZK_OK;
    }
    DiagQueue *D = (DiagQueue *)*handle;
    if (!D) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_job_queue: no queue");
    auto need = [&](size_t k) { return out && cap >= k; };
    switch (op) {
    case 1: {
        if (!need(1)) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        std::lock_guard<std::mutex> lk(D->submit_mu);
        uint64_t id = 0;
        const int rc = D->core->submit(diag_key(a, b), std::make_pair(D->next, DiagJob{b}), &id);
        if (rc != ZK_OK) ZK_FAIL(rc, "zk_diag_job_queue: the queue is closed");
        D->next = id + 1;
        out[0] = id;
        return ZK_OK;
    }
    case 2: {
        std::lock_guard<std::mutex> lk(D->S.mu);
        if (a)
            D->S.open[a] = true;
        else
            D->S.open_all = true;
        D->S.cv.notify_all();
        return ZK_OK;
    }
    case 3:
    case 4:
    case 5: {
        if (!need(8)) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        uint64_t id = a, r = 0;
        JobInfo info;
        const int rc = op == 3 ? D->core->wait(id, &r, &info) : op == 4 ? D->core->poll(id, &r, &info)
                                                                        : D->core->wait_any(&id, &r, &info);
        if (rc != ZK_OK) return rc;
        out[0] = (uint64_t)info.state, out[1] = (uint64_t)(int64_t)info.prover, out[2] = info.running_at_start;
        out[3] = info.start_seq, out[4] = r, out[5] = info.queued_ms >= 0, out[6] = info.run_ms >= 0, out[7] = id;
        return ZK_OK;
    }
    case 6: return D->core->cancel(a);
    case 7: D->core->pause(); return ZK_OK;
    case 8: D->core->resume(); return ZK_OK;
    case 9: {
        if (!need(6)) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        const JobQueueStats s = D->core->stats();
        out[0] = s.submitted, out[1] = s.completed, out[2] = s.cancelled, out[3] = s.queued, out[4] = s.running;
        out[5] = s.peak_running;
        return ZK_OK;
    }
    case 10:
        if (!need(1)) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        out[0] = (uint64_t)(int64_t)D->core->state(a);
        return ZK_OK;
    case 11: {
        std::lock_guard<std::mutex> lk(D->S.mu);
        if (!need(1 + 2 * D->S.log.size())) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_job_queue: out too small");
        out[0] = D->S.log.size();
        for (size_t i = 0; i < D->S.log.size(); i++)
            out[1 + 2 * i] = D->S.log[i].first, out[2 + 2 * i] = (uint64_t)(int64_t)D->S.log[i].second;
        return ZK_OK;
    }
    case 12: D->core->close(); return ZK_OK;
    case 13: D->core->join(); return ZK_OK;
    case 14:
        D->core.reset();
        delete D;
        *handle = nullptr;
        return ZK_OK;
    default: ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_job_queue: unknown op");
    }
}
