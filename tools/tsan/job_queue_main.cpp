// job_queue_main.cpp -- csrc/job_queue.hpp under ThreadSanitizer, as a host program of its own: four threads submit to
// one core with three executor threads (a no-op executor) and collect their jobs through wait, poll, wait_any and
// cancel, while a fifth pauses and resumes the queue; then a queue is destroyed with jobs still waiting.  Every job must
// be delivered exactly once, and the counters must add up.
//   c++ -std=c++17 -O1 -g -fsanitize=thread -I include -o job_queue_main tools/tsan/job_queue_main.cpp -lpthread &&
//   ./job_queue_main [jobs per submitter]
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../encrypt-zkvm_amd/csrc/job_queue.hpp"

using namespace zk;

struct NoOp {
    std::atomic<uint64_t> *ran;
    void operator()(int, uint64_t &job, uint64_t &res) const {
        res = job + 1;
        ran->fetch_add(1, std::memory_order_relaxed);
    }
};
typedef JobQueue<uint64_t, uint64_t, NoOp> Queue;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "job_queue_main: line %d: %s\n", __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static JobKey key_of(uint64_t k) {
    JobKey key;
    key.n = 16 << (k % 3);
    key.hash[0] = (uint8_t)(k % 5);
    return key;
}

int main(int argc, char **argv) {
    const uint64_t per = argc > 1 ? strtoull(argv[1], nullptr, 10) : 5000;
    constexpr int SUBMITTERS = 4, EXECUTORS = 3;
    std::atomic<uint64_t> ran{0}, delivered{0}, done{0}, cancelled{0};
    {
        Queue q(EXECUTORS, NoOp{&ran});
        std::atomic<bool> stop{false};
        std::thread toggler([&] {
            while (!stop.load()) {
                q.pause();
                std::this_thread::yield();
                q.resume();
                std::this_thread::yield();
            }
        });
        std::vector<std::thread> subs;
        for (int t = 0; t < SUBMITTERS; t++)
            subs.emplace_back([&, t] {
                std::vector<uint64_t> mine;
                auto take = [&](int rc, uint64_t job, uint64_t res, const JobInfo &info) {
                    REQUIRE(rc == ZK_OK);
                    REQUIRE(info.state == JOB_DONE || info.state == JOB_CANCELLED);
                    if (info.state == JOB_DONE) {
                        REQUIRE(res == job + 1 && info.prover >= 0 && info.prover < EXECUTORS);
                        REQUIRE(info.running_at_start < (uint32_t)EXECUTORS && info.start_seq > 0);
                        done++;
                    } else {
                        REQUIRE(info.prover == -1 && info.start_seq == 0);
                        cancelled++;
                    }
                    delivered++;
                };
                for (uint64_t k = 0; k < per; k++) {
                    const uint64_t job = (uint64_t)t * per + k;
                    uint64_t id = 0;
                    REQUIRE(q.submit(key_of(job), job, &id) == ZK_OK && id != 0);
                    mine.push_back(id);
                    if (k % 7 == 3) (void)q.cancel(id);  // succeeds only while the job is still queued
                    if (mine.size() < 8) continue;
                    // collect this thread's own jobs: half by poll-then-wait, half by wait
                    for (size_t i = 0; i < mine.size(); i++) {
                        uint64_t res = 0;
                        JobInfo info;
                        int rc = i % 2 ? q.poll(mine[i], &res, &info) : ZK_ERR_PENDING;
                        if (rc == ZK_ERR_PENDING) rc = q.wait(mine[i], &res, &info);
                        take(rc, (uint64_t)t * per + (k + 1 - mine.size()) + i, res, info);
                        REQUIRE(q.poll(mine[i], &res, &info) == ZK_ERR_INVALID_ARG);  // delivered once
                    }
                    mine.clear();
                }
                for (uint64_t id : mine) {
                    uint64_t res = 0;
                    JobInfo info;
                    REQUIRE(q.wait(id, &res, &info) == ZK_OK);
                    delivered++;
                    (info.state == JOB_DONE ? done : cancelled)++;
                }
            });
        for (auto &s : subs) s.join();
        stop = true;
        toggler.join();
        q.resume();
        const JobQueueStats s = q.stats();
        REQUIRE(s.submitted == SUBMITTERS * per && delivered.load() == s.submitted);
        REQUIRE(s.completed == done.load() && s.cancelled == cancelled.load() && s.completed == ran.load());
        REQUIRE(s.completed + s.cancelled == s.submitted && s.queued == 0 && s.running == 0);
        REQUIRE(s.peak_running >= 1 && s.peak_running <= (uint32_t)EXECUTORS);
        uint64_t id = 0, res = 0;
        JobInfo info;
        REQUIRE(q.wait_any(&id, &res, &info) == ZK_ERR_INVALID_ARG);  // nothing pending

        // wait_any from two threads while two submit: each job comes out once
        std::atomic<uint64_t> got{0};
        const uint64_t more = per / 2 + 1;
        std::vector<std::thread> th;
        for (int t = 0; t < 2; t++)
            th.emplace_back([&] {
                for (uint64_t k = 0; k < more; k++) {
                    uint64_t i2 = 0;
                    REQUIRE(q.submit(key_of(k), k, &i2) == ZK_OK);
                }
            });
        for (auto &t : th) t.join();
        th.clear();
        for (int t = 0; t < 2; t++)
            th.emplace_back([&] {
                uint64_t i2 = 0, r2 = 0;
                JobInfo in2;
                while (q.wait_any(&i2, &r2, &in2) == ZK_OK) got++;
            });
        for (auto &t : th) t.join();
        REQUIRE(got.load() == 2 * more);
    }
    {
        // destroy with work waiting: a paused queue's jobs are cancelled, none runs
        const uint64_t before = ran.load();
        Queue q(EXECUTORS, NoOp{&ran});
        q.pause();
        for (uint64_t k = 0; k < 100; k++) {
            uint64_t id = 0;
            REQUIRE(q.submit(key_of(k), k, &id) == ZK_OK && id == k + 1);
        }
        q.close();
        uint64_t id = 0, res = 0;
        JobInfo info;
        REQUIRE(q.submit(key_of(0), 0, &id) == ZK_ERR_INVALID_ARG);
        REQUIRE(q.wait(1, &res, &info) == ZK_OK && info.state == JOB_CANCELLED);
        REQUIRE(q.stats().cancelled == 100 && ran.load() == before);
    }
    printf("job_queue_main ok: %llu jobs from %d submitters on %d executors, %llu ran, %llu cancelled\n",
           (unsigned long long)(SUBMITTERS * per), SUBMITTERS, EXECUTORS, (unsigned long long)done.load(),
           (unsigned long long)cancelled.load());
    return 0;
}
