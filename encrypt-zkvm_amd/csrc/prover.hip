// prover.hip -- host orchestration of the gfx950 prove path and the C ABI (include/zkvm_gpu.h).
//
// zk_prove_device() runs winterfell 0.9's generate_proof stages for ProcessorAir
// (prover/src/lib.rs:40-77) on one GPU:
//   S0 coin seed                       host (Context::to_elements || PublicInputs::to_elements)
//   S2 trace iNTT + coset LDE + commit  ntt / hash_rows / merkle           (new_trace_lde)
//   S3 constraint evaluation           batch_inv + eval_constraints       (new_evaluator + evaluate)
//   S4 composition poly + commit       ntt(inverse) + comp_cross + ntt + hash_rows + merkle
//   S5 OOD frame, DEEP                 poly_eval + batch_inv + deep
//   S6 FRI layers + remainder          commit_fri_layer + fri_fold; remainder on host
//   S7 grinding + query positions      host
//   S8 openings                        gather kernels + host batch-proof assembly
//   S9 proof bytes                     host
// The public coin runs on the host and sees only 32-byte roots, so each commitment costs one
// small device->host copy.  Protocol choices are the ones of DESIGN.md "Protocol profile".
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "host_pool.hpp"
#include "prover_internal.hpp"
#include "rescue_consts.hpp"

namespace zk {
thread_local std::string g_err;
// ZK_HOST_TIMING=1: per proof, the host-only critical-path segments (the GPU idles during these) to stderr
struct HostTimer {
    bool on = getenv("ZK_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    std::string log;
    void start() { t = std::chrono::steady_clock::now(); }
    void lap(const char *what) { stop(what), start(); }
    void stop(const char *what) {
        if (!on) return;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t).count();
        char b[96];
        snprintf(b, sizeof b, " %s=%.1f", what, us);
        log += b;
    }
    ~HostTimer() {
        if (on && !log.empty()) fprintf(stderr, "[zk host us]%s\n", log.c_str());
    }
};
}
using namespace zk;

const char *zk_last_error(void) { return g_err.c_str(); }

struct zk_trace_lde {
    zk_prover *p;
    size_t n;
    uint32_t B;
    int width;
};

// ---------------------------------------------------------------- table construction
template <typename T>
static hipError_t upload(zk_prover *p, T **dst, const std::vector<T> &v) {
    hipError_t e = p->arena.alloc(dst, v.size());
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
static std::vector<fe_ws> ws_of(const std::vector<fe> &v) {
    std::vector<fe_ws> w(v.size());
    for (size_t i = 0; i < v.size(); i++) w[i] = make_fe_ws(v[i]);
    return w;
}
static std::vector<fe_w2> w2_of(const std::vector<fe> &v) {
    std::vector<fe_w2> w(v.size());
    for (size_t i = 0; i < v.size(); i++) w[i] = make_fe_w2(v[i]);
    return w;
}

static hipError_t make_pow_table(zk_prover *p, fe s, size_t n, PowTable *out) {
    std::vector<fe> lo(2048), hi(n / 2048 + 1);
    lo[0] = fe_one();
    for (int t = 1; t < 2048; t++) lo[t] = fe_mul(lo[t - 1], s);
    fe s2048 = fe_mul(lo[2047], s);
    hi[0] = fe_one();
    for (size_t u = 1; u < hi.size(); u++) hi[u] = fe_mul(hi[u - 1], s2048);
    hipError_t e = upload(p, &out->lo, lo);
    if (e != hipSuccess) return e;
    return upload(p, &out->hi, hi);
}

static hipError_t make_ntt_tables(zk_prover *p, int log_n, NttTables *T) {
    T->log_n = log_n;
    // w_4096 powers, forward and inverse: built once per process (a function-local static is
    // initialised exactly once even when provers on several threads reach it together)
    struct Dft4096 {
        std::vector<fe> f, i;
        std::vector<fe_ws> fw, iw;
        std::vector<fe_w2> f2, i2;
        Dft4096() : f(2048), i(2048) {
            const fe w = h_root_of_unity(12), wi = h_inv(w);
            f[0] = i[0] = fe_one();
            for (int t = 1; t < 2048; t++) {
                f[t] = fe_mul(f[t - 1], w);
                i[t] = fe_mul(i[t - 1], wi);
            }
            fw = ws_of(f);
            iw = ws_of(i);
            f2 = w2_of(f);
            i2 = w2_of(i);
        }
    };
    static const Dft4096 d4096;
    hipError_t e = upload(p, &T->dft_fwd, d4096.f);
    if (e == hipSuccess) e = upload(p, &T->dft_inv, d4096.i);
    if (e == hipSuccess) e = upload(p, &T->dft_fwd_ws, d4096.fw);
    if (e == hipSuccess) e = upload(p, &T->dft_inv_ws, d4096.iw);
    if (e == hipSuccess) e = upload(p, &T->dft_fwd_w2, d4096.f2);
    if (e == hipSuccess) e = upload(p, &T->dft_inv_w2, d4096.i2);
    size_t n = (size_t)1 << log_n;
    fe w = h_root_of_unity(log_n);
    PowTable f, i;
    if (e == hipSuccess) e = make_pow_table(p, w, n, &f);
    if (e == hipSuccess) e = make_pow_table(p, h_inv(w), n, &i);
    T->fwd_lo = f.lo;
    T->fwd_hi = f.hi;
    T->inv_lo = i.lo;
    T->inv_hi = i.hi;
    return e;
}

// Periodic columns (air/src/lib.rs:201-225): CYCLE_MASK and the 8 ARK columns, interpolated over
// <w_16> and evaluated at (3 * w_CE^i)^(n/16) for the 128 distinct CE steps i mod 128.
static std::vector<fe> periodic_table(size_t n) {
    std::vector<std::vector<fe>> cols(9, std::vector<fe>(16));
    for (int r = 0; r < 16; r++) {
        cols[0][r] = fe_make(r < 14 ? 1 : 0);
        for (int c = 0; c < 8; c++) cols[1 + c][r] = fe_make(ZK_ARK[8 * r + c][0], ZK_ARK[8 * r + c][1]);
    }
    for (auto &c : cols) h_interp_coset(c, fe_one());
    const int log_ce = ilog2(8 * n);
    fe w = h_root_of_unity(log_ce), x = fe_make(3);
    std::vector<fe> out(128 * 9);
    for (int i = 0; i < 128; i++) {
        fe y = h_pow(x, n / 16);
        for (int j = 0; j < 9; j++) out[i * 9 + j] = h_poly_eval(cols[j].data(), 16, y);
        x = fe_mul(x, w);
    }
    return out;
}

int zk::get_plan(zk_prover *p, size_t n, uint32_t B, Plan **out) {
    auto key = std::make_pair(ilog2(n), ilog2(B));
    auto it = p->plans.find(key);
    if (it != p->plans.end()) {
        *out = it->second.get();
        return ZK_OK;
    }
    auto pl = std::make_unique<Plan>();
    pl->log_n = key.first;
    pl->log_b = key.second;
    ZK_CHECK_HIP(make_ntt_tables(p, pl->log_n, &pl->Tn));
    if (pl->log_n > 12) {  // four-step NTTs: inter-pass twiddle tables (2n elements)
        ZK_CHECK_HIP(p->arena.alloc(&pl->Tn.fwd_pass, n));
        ZK_CHECK_HIP(p->arena.alloc(&pl->Tn.inv_pass, n));
        ZK_CHECK_HIP(p->arena.alloc(&pl->Tn.inv_pass_n, n));
        pl->Tn.inv_n = h_inv(fe_make(n));
        make_pass_twiddles(p->st, pl->Tn);
    }
    ZK_CHECK_HIP(make_ntt_tables(p, pl->log_n + 3, &pl->Tce));
    ZK_CHECK_HIP(make_ntt_tables(p, pl->log_n + pl->log_b, &pl->TN));
    fe wN = h_root_of_unity(pl->log_n + pl->log_b), wce = h_root_of_unity(pl->log_n + 3);
    std::vector<fe> xrN(B), xrce(8), xnN(B);
    fe s = fe_make(3);
    // coset-LDE tables (CosetTables, B * n elements: 128 MiB at n = 2^20, B = 8)
    if (pl->log_n <= 12) {
        ZK_CHECK_HIP(p->arena.alloc(&pl->ct.full, (size_t)B * n));
    } else {
        ZK_CHECK_HIP(p->arena.alloc(&pl->ct.pass, (size_t)B * n));
        ZK_CHECK_HIP(p->arena.alloc(&pl->ct.stage, (size_t)B * 4096));
    }
    const int log_n2 = ntt_log_n2(pl->log_n);  // pass-1 line length of the four-step split (as in ntt_run())
    const size_t n2 = (size_t)1 << log_n2, n1 = n >> log_n2;
    std::vector<fe> stage(pl->log_n > 12 ? (size_t)B * 4096 : 0);
    for (uint32_t r = 0; r < B; r++) {
        xrN[r] = s;
        xnN[r] = h_pow(s, n);
        PowTable t;
        ZK_CHECK_HIP(make_pow_table(p, s, n, &t));
        if (pl->log_n <= 12) {
            pow_expand(p->st, t.lo, t.hi, n, pl->ct.full + (size_t)r * n);
        } else {
            // pass[r][k1 n2 + j2] = s^k1 w_n^(j2 k1); stage[r][h + j] = c^(n2/2h) w_2h^j with c = s^n1
            coset_pass_tables(p->st, t.lo, t.hi, pl->Tn.fwd_pass, pl->log_n, log_n2, pl->ct.pass + (size_t)r * n);
            const fe c = h_pow(s, n1);
            for (size_t h = 1; h < n2; h *= 2) {
                const fe w = h_root_of_unity(ilog2(2 * h));
                fe v = h_pow(c, n2 / (2 * h));
                for (size_t j = 0; j < h; j++) {
                    stage[(size_t)r * 4096 + h + j] = v;
                    v = fe_mul(v, w);
                }
            }
        }
        pl->coset.push_back(t);
        s = fe_mul(s, wN);
    }
    if (pl->log_n > 12) {
        ZK_CHECK_HIP(hipMemcpy(pl->ct.stage, stage.data(), stage.size() * sizeof(fe), hipMemcpyHostToDevice));
        ZK_CHECK_HIP(upload(p, &pl->ct.stage_ws, ws_of(stage)));
        ZK_CHECK_HIP(upload(p, &pl->ct.stage_w2, w2_of(stage)));
    }
    s = fe_make(3);
    for (int r = 0; r < 8; r++) {
        xrce[r] = s;
        s = fe_mul(s, wce);
    }
    ZK_CHECK_HIP(upload(p, &pl->xr_N, xrN));
    ZK_CHECK_HIP(upload(p, &pl->xn_N, xnN));
    ZK_CHECK_HIP(upload(p, &pl->xr_ce, xrce));
    ZK_CHECK_HIP(make_pow_table(p, h_inv(fe_make(3)), n, &pl->inv3));
    ZK_CHECK_HIP(upload(p, &pl->periodic, periodic_table(n)));
    if (pl->log_n > 12) {
        // e_(n-1)'s interpolant and coset LDE (the sparse trace columns': SparseCols).  A rank-sized prover holds the
        // LDE of its own cosets only (plan_rank_tables, once its rank is known)
        ZK_CHECK_HIP(p->arena.alloc(&pl->lagr, n));
        const bool full = p->shard_world <= 1;
        if (full) {
            ZK_CHECK_HIP(p->arena.alloc(&pl->lagr_lde, (size_t)B * n));
            pl->lde_cos = (int)B;
        }
        std::vector<fe> e(n, fe_zero());
        e[n - 1] = fe_one();
        fe *de = nullptr;
        ZK_CHECK_HIP(hipMalloc(&de, n * sizeof(fe)));
        hipError_t err = hipMemcpy(de, e.data(), n * sizeof(fe), hipMemcpyHostToDevice);
        if (err == hipSuccess) {
            const fe inv_n = h_inv(fe_make(n));
            ntt(p->st, pl->Tn, de, n, pl->lagr, n, 1, true, nullptr, &inv_n, p->tmp);
            if (full) ntt_lde(p->st, pl->Tn, pl->ct, pl->lagr, n, 1, 0, 1, (int)B, pl->lagr_lde, (size_t)B * n, n, p->tmp);
            err = hipStreamSynchronize(p->st);
        }
        (void)hipFree(de);
        ZK_CHECK_HIP(err);
    }
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    *out = pl.get();
    p->plans[key] = std::move(pl);
    return ZK_OK;
}

Fe8 zk::ce_inv_zn(int log_n) {
    const size_t n = (size_t)1 << log_n;
    const fe wce = h_root_of_unity(log_n + 3);
    Fe8 z;
    fe x = fe_make(3);
    for (int r = 0; r < 8; r++, x = fe_mul(x, wce)) z.v[r] = h_inv(fe_sub(h_pow(x, n), fe_one()));
    return z;
}

const fe *zk::boundary_inverses(zk_prover *p, Plan *pl) {
    if (!pl->bnd_inv) {
        const size_t CE = (size_t)8 << pl->log_n, n = (size_t)1 << pl->log_n;
        if (p->arena.alloc(&pl->bnd_inv, 3 * CE) != hipSuccess) return nullptr;
        const fe g = h_root_of_unity(pl->log_n);
        divisor_tables(p->st, pl->Tn, pl->xr_ce, 3, pl->log_n, h_pow(g, n - 1), h_pow(g, n - 2), ce_inv_zn(pl->log_n),
                       pl->bnd_inv);
    }
    return pl->bnd_inv;
}

// ---------------------------------------------------------------- prover object
int zk_device_count(int *count) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    if (count) *count = c;
    return ZK_OK;
}

// One upload stream per device for the process (created on first use, kept for the process's lifetime), shared by
// every prover on that device, with the mutex that keeps one prover's copy and its event record adjacent.
static int shared_upload_stream(int device, hipStream_t *st, std::mutex **mu, std::atomic<int> **busy) {
    struct Up {
        hipStream_t st = nullptr;
        std::mutex mu;
        std::atomic<int> busy{0};
    };
    static std::mutex reg_mu;
    static std::map<int, Up *> reg;  // process lifetime: never freed
    std::lock_guard<std::mutex> lk(reg_mu);
    Up *&u = reg[device];
    if (!u) {
        auto fresh = std::make_unique<Up>();
        ZK_CHECK_HIP(hipStreamCreateWithFlags(&fresh->st, hipStreamNonBlocking));
        u = fresh.release();
    }
    *st = u->st;
    *mu = &u->mu;
    *busy = &u->busy;
    return ZK_OK;
}

int zk::upload_gate(zk_prover *p, hipEvent_t ev) {
    (void)p;
    ZK_CHECK_HIP(hipEventSynchronize(ev));
    return ZK_OK;
}

void zk::upload_drain(zk_prover *p) {
    for (auto &e : p->ev_up)
        if (e) (void)hipEventSynchronize(e);
}

// world = 0: a full prover; world = G: one rank of a G-way coset-sharded proof (blowup 8), whose LDE-domain
// buffers (trace / composition LDE, DEEP, NTT scratch, Merkle subtrees) hold N / G points instead of N
static int create_prover(int device, size_t max_n, uint32_t max_b, int world, zk_prover **out) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) ZK_FAIL(ZK_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= cnt) ZK_FAIL(ZK_ERR_INVALID_ARG, "device index out of range");
    ZK_CHECK_HIP(hipSetDevice(device));
    // The host waits on the prover stream a few times per proof (transcript round trips): spin instead
    // of yielding (A/B: -0.05 ms per 2^20 proof).  PROCESS-WIDE side effect (documented at zk_prover_create
    // in zkvm_gpu.h): hipDeviceScheduleSpin applies to every stream sync of the process on this device, so
    // each waiting host thread busy-spins.  Only takes effect if this is the first use of the device in the
    // process; ZK_SPIN_WAIT=0 keeps the runtime's default (yield).
    {
        const char *e = getenv("ZK_SPIN_WAIT");
        if (!e || atoi(e)) {
            (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
            (void)hipGetLastError();  // refused once the context exists: leave no sticky error behind
        }
    }
    auto p = std::make_unique<zk_prover>();
    p->device = device;
    p->max_n = max_n;
    p->max_b = max_b;
    ZK_CHECK_HIP(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
    ZK_TRY(shared_upload_stream(device, &p->up, &p->up_mu, &p->dev_busy));
    for (auto &e : p->ev_up) ZK_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ZK_CHECK_HIP(upload_rescue_consts(p->st));
    const size_t n = max_n, N = max_n * max_b, CE = 8 * max_n;
    // Nl: LDE-domain points this prover holds (all N, or the N / G of one sharded rank)
    if (world == 1) world = 0;  // one rank holds the whole domain: a full prover
    p->shard_world = world;
    const size_t Nl = world ? N / (size_t)world : N;
    DeviceArena &A = p->arena;
    ZK_CHECK_HIP(A.alloc(&p->d_trace, (size_t)W * n));
    // trace polynomials; as a rank of a sharded proof, G slices of ceil(W / G) columns (the in-place all-gather of
    // shard.hip): 8 ceil(W / 8) columns cover G = 1, 2, 4, 8
    ZK_CHECK_HIP(A.alloc(&p->polys, (size_t)8 * ((W + 7) / 8) * n));
    // NTT scratch: the four-step intermediate of a whole 8-coset LDE of the trace (28 x 8 x n; a sharded rank's
    // cosets: 28 x 8/G x n, at least the 28 x n of the interpolation)
    ZK_CHECK_HIP(A.alloc(&p->tmp, (size_t)W * (world ? std::max<size_t>(n, Nl) : 8 * n)));
    ZK_CHECK_HIP(A.alloc(&p->lde, (size_t)W * Nl));
    ZK_CHECK_HIP(A.alloc(&p->comp, CE));
    ZK_CHECK_HIP(A.alloc(&p->ctmp, CE));
    ZK_CHECK_HIP(A.alloc(&p->cpolys, (size_t)ZK_MAX_CCOLS * n));
    ZK_CHECK_HIP(A.alloc(&p->clde, (size_t)8 * Nl));
    ZK_CHECK_HIP(A.alloc(&p->deep, Nl));
    if (!world) ZK_CHECK_HIP(A.alloc(&p->ulde, N));  // the single path's DEEP LDE
    ZK_CHECK_HIP(A.alloc(&p->dscratch, DeepScratch::size(n, 1)));
    // FRI layers: sum over layers of L/fold values and 2*L/fold digests; worst case fold = 2
    ZK_CHECK_HIP(A.alloc(&p->fri, N + 16));
    ZK_CHECK_HIP(A.alloc(&p->leaves, 32 * Nl));
    ZK_CHECK_HIP(A.alloc(&p->nodes, 32 * Nl));
    ZK_CHECK_HIP(A.alloc(&p->cleaves, 32 * Nl));
    ZK_CHECK_HIP(A.alloc(&p->cnodes, 32 * Nl));
    // digest scratch: a sharded rank's all-to-all send + receive areas (64 B per local point), and the digests of
    // the FRI layers >= 1 (at most 32 B per point of the whole domain, fold 2)
    ZK_CHECK_HIP(A.alloc(&p->fri_dig, (world ? std::max<size_t>(64 * Nl, 32 * N) : 64 * N) + 64));
    ZK_CHECK_HIP(A.alloc(&p->partials, (size_t)(2 * ZK_MAX_COLS + ZK_MAX_CCOLS) * ood_waves(max_n)));
    ZK_CHECK_HIP(A.alloc(&p->ood_tab, (size_t)128 + 2 * ood_waves(max_n)));
    ZK_CHECK_HIP(A.alloc(&p->ood, 256));
    ZK_CHECK_HIP(A.alloc(&p->gather_out, ZK_GATHER_CAP));
    ZK_CHECK_HIP(A.alloc(&p->gather_idx, ZK_GATHER_CAP));
    // the largest read is the last FRI layer: up to ZK_MAX_REMAINDER * blowup values, two planes over E
    p->io_cap = ((size_t)64 << 10) + (size_t)2 * ZK_MAX_REMAINDER * p->max_b * sizeof(fe);
    ZK_CHECK_HIP(hipHostMalloc((void **)&p->h_io, p->io_cap, hipHostMallocDefault));
    p->io_pending.reserve(64);
    ZK_CHECK_HIP(hipHostMalloc((void **)&p->h_gather_idx, ZK_GATHER_CAP * sizeof(uint64_t), hipHostMallocDefault));
    ZK_CHECK_HIP(hipHostMalloc((void **)&p->h_gather_out, ZK_GATHER_CAP * sizeof(fe), hipHostMallocDefault));
    ZK_CHECK_HIP(A.alloc(&p->flag, 4));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->air_consts, sizeof(AirConsts)));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->deep_consts, sizeof(DeepConsts<1>)));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->fold_consts, sizeof(FoldConsts<1>)));
    ZK_CHECK_HIP(A.alloc(&p->fri_seed, 32));
    ZK_CHECK_HIP(A.alloc(&p->fri_alphas, 2 * ZK_MAX_FRI_LAYERS));
    // trace validation: the report and the raw periodic table (the Rescue constants, as the AIR lists them)
    ZK_CHECK_HIP(A.alloc(&p->val_rep, 1));
    ZK_CHECK_HIP(A.alloc(&p->val_per, 16 * 9));
    {
        fe per[16 * 9];
        for (int r = 0; r < 16; r++) air_periodic_row((size_t)r, per + 9 * r);
        ZK_CHECK_HIP(hipMemcpyAsync(p->val_per, per, sizeof per, hipMemcpyHostToDevice, p->st));
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    }
    *out = p.release();
    return ZK_OK;
}

int zk_prover_create(int device, size_t max_n, uint32_t max_b, zk_prover **out) {
    if (!out || max_n < 16 || (max_n & (max_n - 1)) || max_b < 8 || (max_b & (max_b - 1)) || max_b > 64)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_prover_create: max_trace_len must be a power of two >= 16, blowup in [8, 64]");
    return create_prover(device, max_n, max_b, 0, out);
}

int zk_prover_create_shard(int device, size_t max_n, int world, zk_prover **out) {
    if (!out || max_n < 16 || (max_n & (max_n - 1)) || (world != 1 && world != 2 && world != 4 && world != 8))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_prover_create_shard: max_trace_len a power of two >= 16, world 1, 2, 4 or 8");
    return create_prover(device, max_n, 8, world, out);
}

void zk_prover_destroy(zk_prover *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->st);
    upload_drain(p);
    for (auto &e : p->stage_pool) (void)hipEventDestroy(e);
    for (auto &e : p->xchg_pool) (void)hipEventDestroy(e);
    if (p->cst) {
        (void)hipStreamSynchronize(p->cst);
        (void)hipStreamDestroy(p->cst);
    }
    if (p->ev_ready) (void)hipEventDestroy(p->ev_ready);
    for (auto &e : p->ev_up)
        if (e) (void)hipEventDestroy(e);
    if (p->ev_vm) (void)hipEventDestroy(p->ev_vm);
    (void)hipStreamDestroy(p->st);
    if (p->h_io) (void)hipHostFree(p->h_io);
    if (p->h_gather_idx) (void)hipHostFree(p->h_gather_idx);
    if (p->h_gather_out) (void)hipHostFree(p->h_gather_out);
    if (p->h_vm) (void)hipHostFree(p->h_vm);
    if (p->sp_h) (void)hipHostFree(p->sp_h);
    if (p->h_pack) (void)hipHostFree(p->h_pack);
    for (auto &s : p->fix_snaps) {
        (void)hipFree(s.fpolys);
        (void)hipFree(s.flde);
    }
    delete p->open;
    delete p;
}

// ---------------------------------------------------------------- process-wide prover pool
// The reference builds its prover per call (ExecutionProver::new in vm::prove, vm/src/lib.rs:24).  A zk_prover is
// ~12.5 GB of HBM at 2^20 plus per-size tables built by its first proof, so the drop-in keeps released provers for
// the next acquire on the same device instead (zk_prover_acquire / zk_prover_release).
namespace {
struct Pool {
    std::mutex mu;
    std::vector<zk_prover *> idle;
};
Pool &pool() {
    static Pool *P = new Pool();  // process lifetime (provers released at exit are reclaimed with the process)
    return *P;
}
}  // namespace

int zk_prover_acquire(int device, size_t max_n, uint32_t max_b, zk_prover **out) {
    if (!out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    {
        Pool &P = pool();
        std::lock_guard<std::mutex> lk(P.mu);
        // the smallest idle full prover of this device that fits
        size_t best = P.idle.size();
        for (size_t i = 0; i < P.idle.size(); i++) {
            const zk_prover *q = P.idle[i];
            if (q->device != device || q->shard_world || q->max_n < max_n || q->max_b < max_b) continue;
            if (best == P.idle.size() || q->max_n * q->max_b < P.idle[best]->max_n * P.idle[best]->max_b) best = i;
        }
        if (best < P.idle.size()) {
            *out = P.idle[best];
            P.idle.erase(P.idle.begin() + (long)best);
            return ZK_OK;
        }
    }
    return zk_prover_create(device, max_n, max_b, out);
}

void zk_prover_release(zk_prover *p) {
    if (!p) return;
    if (p->shard_world) {  // rank-sized provers are not pooled
        zk_prover_destroy(p);
        return;
    }
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->st);
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    P.idle.push_back(p);
}

int zk_prover_pool_trim(int device) {
    std::vector<zk_prover *> drop;
    {
        Pool &P = pool();
        std::lock_guard<std::mutex> lk(P.mu);
        for (size_t i = 0; i < P.idle.size();)
            if (device < 0 || P.idle[i]->device == device) {
                drop.push_back(P.idle[i]);
                P.idle.erase(P.idle.begin() + (long)i);
            } else {
                i++;
            }
    }
    for (zk_prover *p : drop) zk_prover_destroy(p);
    return (int)drop.size();
}

int zk_prover_trace_buffer(zk_prover *p, void **d_trace) {
    if (!p || !d_trace) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *d_trace = p->d_trace;
    return ZK_OK;
}

// ---------------------------------------------------------------- stage timing
void zk::stage_begin(zk_prover *p) {
    p->stage_names.clear();
    p->stage_done = false;
    p->xchg.clear();
    p->xchg_next = 0;
    p->sched.clear();
}
void zk::stage_mark(zk_prover *p, const char *name) {
    const size_t i = p->stage_names.size();
    if (i == p->stage_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;  // timing only: a missing mark is not an error
        p->stage_pool.push_back(e);
    }
    (void)hipEventRecord(p->stage_pool[i], p->st);
    p->stage_names.push_back(name);
}
// the proof is complete (its stream synchronized): its stage events may be read until the next proof
void zk::stage_collect(zk_prover *p) { p->stage_done = true; }

int zk_prover_stage_times(zk_prover *p, const char **names, float *ms, int cap, int *count) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    p->stage_ms.clear();
    if (p->stage_done)
        for (size_t i = 1; i < p->stage_names.size(); i++) {
            float t = 0;
            (void)hipEventElapsedTime(&t, p->stage_pool[i - 1], p->stage_pool[i]);
            p->stage_ms.push_back({p->stage_names[i], t});
        }
    int k = (int)p->stage_ms.size();
    for (int i = 0; i < k && i < cap; i++) {
        if (names) names[i] = p->stage_ms[i].first;
        if (ms) ms[i] = p->stage_ms[i].second;
    }
    if (count) *count = k;
    return ZK_OK;
}

int zk_prover_proof_info(const zk_prover *p, zk_proof_info *out) {
    if (!p || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    memset(out, 0, sizeof *out);
    out->schedule = p->last_sched;
    out->hint_redos = p->hint_redos;
    for (const auto &h : p->hint_sets) out->hint_sets += h.n != 0 && h.have ? 1u : 0u;
    out->hinted_sparse = p->tc.sp_hinted;
    out->derived = p->tc.clk_used ? 1u : 0u;
    for (int i = 0; i < zk_prover::ZK_FIXED_SNAPS; i++) {
        const auto &s = p->fix_snaps[i];
        out->fixed_sets += s.live && s.owner >= 0 && p->hint_sets[s.owner].snap == i ? 1u : 0u;
    }
    return ZK_OK;
}

int zk_prover_upload_stats(zk_prover *p, uint64_t *bytes, uint32_t *sparse_cols, uint32_t *narrow8_cols,
                           uint32_t *narrow32_cols) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    if (bytes) *bytes = p->tc.up_bytes;
    if (sparse_cols) *sparse_cols = p->tc.up_sparse;
    if (narrow8_cols) *narrow8_cols = p->tc.up_nw8;
    if (narrow32_cols) *narrow32_cols = p->tc.up_nw32;
    return ZK_OK;
}

int zk_prover_upload_derived(zk_prover *p, uint32_t *derived_cols) {
    if (!p || !derived_cols) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *derived_cols = p->tc.clk_used ? 1u : 0u;
    return ZK_OK;
}

int zk_prover_upload_fixed(zk_prover *p, uint32_t *fixed_cols) {
    if (!p || !fixed_cols) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *fixed_cols = p->tc.fix_used;
    return ZK_OK;
}

int zk_prover_coeff_sources(zk_prover *p, uint32_t *cols) {
    if (!p || !cols) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *cols = p->tc.coeff_src;
    return ZK_OK;
}

int zk_prover_exchange_stats_ex(zk_prover *p, const char **names, float *ms, float *exposed_ms, double *bytes,
                                int *calls, int cap, int *count) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    std::vector<const char *> nm;
    std::vector<float> t, w;
    std::vector<double> b;
    std::vector<int> c;
    if (p->stage_done)
        for (const auto &r : p->xchg) {
            float x = 0, y = 0;
            (void)hipEventElapsedTime(&x, p->xchg_pool[r.ev], p->xchg_pool[r.ev + 1]);
            if (r.waited) (void)hipEventElapsedTime(&y, p->xchg_pool[r.ev + 2], p->xchg_pool[r.ev + 3]);
            size_t i = 0;
            while (i < nm.size() && strcmp(nm[i], r.name)) i++;
            if (i == nm.size()) {
                nm.push_back(r.name);
                t.push_back(0);
                w.push_back(0);
                b.push_back(0);
                c.push_back(0);
            }
            t[i] += x;
            w[i] += y;
            b[i] += r.bytes;
            c[i] += 1;
        }
    const int k = (int)nm.size();
    for (int i = 0; i < k && i < cap; i++) {
        if (names) names[i] = nm[i];
        if (ms) ms[i] = t[i];
        if (exposed_ms) exposed_ms[i] = w[i];
        if (bytes) bytes[i] = b[i];
        if (calls) calls[i] = c[i];
    }
    if (count) *count = k;
    return ZK_OK;
}

int zk_prover_exchange_stats(zk_prover *p, const char **names, float *ms, double *bytes, int *calls, int cap,
                             int *count) {
    return zk_prover_exchange_stats_ex(p, names, ms, nullptr, bytes, calls, cap, count);
}

int zk_prover_shard_schedule(zk_prover *p, char *buf, size_t cap, size_t *len) {
    if (!p || !len) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    std::string js = "{\"world\": " + std::to_string(p->sched_world) +
                     ", \"measure\": " + (p->sched_measure ? "true" : "false") + ", \"entries\": [";
    char tmp[256];
    auto el = [&](size_t a, size_t b) {
        float x = 0;
        (void)hipEventElapsedTime(&x, p->xchg_pool[a], p->xchg_pool[b]);
        return x;
    };
    if (p->stage_done)
        for (size_t i = 0; i < p->sched.size(); i++) {
            const auto &e = p->sched[i];
            // the compute segment before this entry
            const float seg = i ? el(p->sched[i - 1].post, e.pre) : 0.f;
            snprintf(tmp, sizeof tmp, "%s{\"seg_ms\": %.5f, \"lead\": %s}", i ? ", " : "", seg,
                     e.lead ? "true" : "false");
            js += tmp;
            if (e.kind == 'S' || e.kind == 'W') {
                const auto &r = p->xchg[e.x];
                if (e.kind == 'S')
                    snprintf(tmp, sizeof tmp, ", {\"start\": %d, \"name\": \"%s\", \"op\": \"%s\", \"bytes\": %.0f, "
                             "\"ms\": %.5f}", e.x, r.name, r.op ? "ag" : "a2a", r.bytes, el(r.ev, r.ev + 1));
                else
                    snprintf(tmp, sizeof tmp, ", {\"wait\": %d, \"exposed_ms\": %.5f}", e.x, el(e.pre, e.post));
                js += tmp;
            }
        }
    js += "]}";
    *len = js.size() + 1;
    if (!buf || cap < js.size() + 1) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "schedule buffer too small");
    memcpy(buf, js.c_str(), js.size() + 1);
    return ZK_OK;
}

int zk_prover_set_upload_schedule(zk_prover *p, int schedule) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    if (schedule < ZK_SCHED_AUTO || schedule > ZK_SCHED_LATENCY) ZK_FAIL(ZK_ERR_INVALID_ARG, "unknown upload schedule");
    p->upload_sched = schedule;
    return ZK_OK;
}

int zk_prover_profile(zk_prover *p, int enable) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    profiler().on = enable != 0;
    profiler().reset();
    return ZK_OK;
}

void zk::collect_kernel_stats(zk_prover *p) {
    KernelProfiler &P = profiler();
    if (!P.on) return;
    (void)hipStreamSynchronize(p->st);
    for (auto &r : P.recs) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        size_t i = 0;
        for (; i < p->kstat_names.size(); i++)
            if (p->kstat_names[i] == r.name) break;
        if (i == p->kstat_names.size()) {
            p->kstat_names.push_back(r.name);
            p->kstat_ms.push_back(0);
            p->kstat_n.push_back(0);
            p->kstat_bytes.push_back(0);
            p->kstat_muls.push_back(0);
            p->kstat_addsubs.push_back(0);
        }
        p->kstat_ms[i] += ms;
        p->kstat_n[i] += 1;
        p->kstat_bytes[i] += r.bytes;
        p->kstat_muls[i] += r.muls;
        p->kstat_addsubs[i] += r.addsubs;
    }
    P.reset();
}

int zk_prover_kernel_stats(zk_prover *p, const char **names, float *total_ms, int *launches, double *total_bytes,
                           int cap, int *count) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    int k = (int)p->kstat_names.size();
    for (int i = 0; i < k && i < cap; i++) {
        if (names) names[i] = p->kstat_names[i].c_str();
        if (total_ms) total_ms[i] = p->kstat_ms[i];
        if (launches) launches[i] = p->kstat_n[i];
        if (total_bytes) total_bytes[i] = p->kstat_bytes[i];
    }
    if (count) *count = k;
    if (!names && !total_ms && !launches && !total_bytes) {  // reset request
        p->kstat_names.clear();
        p->kstat_ms.clear();
        p->kstat_n.clear();
        p->kstat_bytes.clear();
        p->kstat_muls.clear();
        p->kstat_addsubs.clear();
    }
    return ZK_OK;
}

int zk_prover_kernel_ops(zk_prover *p, double *total_muls, double *total_addsubs, int cap, int *count) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    const int k = (int)p->kstat_names.size();
    for (int i = 0; i < k && i < cap; i++) {
        if (total_muls) total_muls[i] = p->kstat_muls[i];
        if (total_addsubs) total_addsubs[i] = p->kstat_addsubs[i];
    }
    if (count) *count = k;
    return ZK_OK;
}

// ---------------------------------------------------------------- Merkle batch openings
void zk::plan_batch(size_t nl, const std::vector<uint64_t> &idx, BatchPlan &bp) {
    int depth = ilog2(nl);
    bp.norm.clear();
    for (uint64_t i : idx) bp.norm.push_back(i & ~1ULL);
    std::sort(bp.norm.begin(), bp.norm.end());
    bp.norm.erase(std::unique(bp.norm.begin(), bp.norm.end()), bp.norm.end());
    bp.paths.resize(bp.norm.size());
    for (auto &path : bp.paths) path.clear();  // keep their capacity across proofs
    std::vector<uint64_t> &next = bp.next, &cur = bp.cur;
    next.clear();
    for (size_t i = 0; i < bp.norm.size(); i++) {
        for (uint64_t l = bp.norm[i]; l < bp.norm[i] + 2; l++)
            if (std::find(idx.begin(), idx.end(), l) == idx.end()) bp.paths[i].push_back({0, l});
        next.push_back((bp.norm[i] + nl) >> 1);
    }
    for (int lvl = 1; lvl < depth; lvl++) {
        std::swap(cur, next);
        next.clear();
        for (size_t i = 0; i < cur.size(); i++) {
            uint64_t sib = cur[i] ^ 1;
            if (i + 1 < cur.size() && cur[i + 1] == sib)
                i++;
            else
                bp.paths[i].push_back({1, sib});
            next.push_back(sib >> 1);
        }
    }
}

// ---------------------------------------------------------------- protocol steps (host side)
// the two checks of a trace alone, shared with the validation entry points (same bounds, same messages)
static int check_trace_len(size_t n, size_t max_n) {
    if (n < 16 || (n & (n - 1)) || n > max_n) ZK_FAIL(ZK_ERR_INVALID_ARG, "trace length must be a power of two in [16, max_trace_len]");
    return ZK_OK;
}
static int check_lwe_size(const zk_pub_inputs *pub) {
    if (pub->lwe_size == 0 || pub->lwe_size > 5)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "lwe_size must be in [1, 5] (enforce_add2 reads 2*lwe_size stack items, constrains.rs:129)");
    return ZK_OK;
}

int zk::check_prove_args(size_t n, size_t max_n, uint32_t max_b, const zk_options *o, const zk_pub_inputs *pub) {
    if (!o || !pub) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if ((o->field_extension != 1 && o->field_extension != 2) || o->blowup < 8 || (o->blowup & (o->blowup - 1)) ||
        (o->fri_folding != 2 && o->fri_folding != 4 && o->fri_folding != 8 && o->fri_folding != 16) ||
        ((o->fri_rem_max_deg + 1) & o->fri_rem_max_deg) || o->fri_rem_max_deg + 1 > ZK_MAX_REMAINDER ||
        o->num_queries == 0 || o->num_queries > ZK_MAX_QUERIES)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "unsupported proof options");
    // winter-air ProofOptions::new asserts grinding_factor <= 32 (and the proof stores it as one byte)
    if (o->grinding > 32) ZK_FAIL(ZK_ERR_INVALID_ARG, "grinding factor must be at most 32");
    ZK_TRY(check_trace_len(n, max_n));
    if (o->blowup > max_b) ZK_FAIL(ZK_ERR_INVALID_ARG, "blowup exceeds the prover's max_blowup");
    ZK_TRY(check_lwe_size(pub));
    if (o->num_queries >= n * o->blowup) ZK_FAIL(ZK_ERR_INVALID_ARG, "num_queries must be smaller than the LDE domain");
    return ZK_OK;
}

Coin zk::seed_coin(size_t n, const zk_options *opt, const zk_pub_inputs *pub) {
    std::vector<fe> e;
    e.push_back(fe_make((uint64_t)W << 16));
    e.push_back(fe_make(n));
    e.push_back(fe_make(ZK_P_LO));
    e.push_back(fe_make(ZK_P_HI));
    e.push_back(fe_make(((uint64_t)opt->field_extension << 16) | ((uint64_t)opt->fri_folding << 8) | opt->fri_rem_max_deg));
    e.push_back(fe_make(opt->grinding));
    e.push_back(fe_make(opt->blowup));
    e.push_back(fe_make(opt->num_queries));
    for (int i = 0; i < 2; i++) e.push_back(fe_from_bytes(pub->program_hash[i]));
    for (int i = 0; i < 16; i++) e.push_back(fe_from_bytes(pub->stack_outputs[i]));
    Coin coin;
    coin.init(e);
    return coin;
}

// what a plane's constants derive from its own coefficients (and delta): bnd1, the folded round constants pv
// (per: the periodic columns over the CE steps, periodic_table(n)) and the evaluator's W sets
static void set_coeff_derived(AirConsts &K, const fe *per) {
    K.bnd1 = fe_zero();
    for (int k = 12; k < NUM_ASSERTS; k++) K.bnd1 = fe_add(K.bnd1, fe_mul(K.coeff_b[k], K.assert_val[k]));
    air_fold_periodic(K.coeff_t + 12, per, K.pv);
    air_build_ws(K);
}

// assertions (air/src/lib.rs:170-195) sorted by (stride, first_step, column) [P3]; CE-coset constants
// returns the host copy of the periodic table of n (valid for the thread's lifetime)
static const fe *air_static_consts(const zk_pub_inputs *pub, size_t n, AirConsts &K) {
    const int log_n = ilog2(n);
    const int first_cols[12] = {0, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19};
    int k = 0;
    for (int i = 0; i < 12; i++, k++) {
        K.assert_col[k] = first_cols[i];
        K.assert_grp[k] = 0;
        K.assert_val[k] = fe_zero();
    }
    for (int i = 0; i < 2; i++, k++) {
        K.assert_col[k] = 7 + i;
        K.assert_grp[k] = 1;
        K.assert_val[k] = fe_from_bytes(pub->program_hash[i]);
    }
    for (int i = 0; i < 8; i++, k++) {
        K.assert_col[k] = 12 + i;
        K.assert_grp[k] = 1;
        K.assert_val[k] = fe_from_bytes(pub->stack_outputs[i]);
    }
    // the divisor constants depend only on n: computed once per n and thread (8 inversions and
    // 10 exponentiations, host time the GPU would otherwise wait for on every proof)
    struct DivConsts {
        fe xr[8], inv_zn[8], g_last2, g_last1;
        std::vector<fe> per;  // periodic_table(n)
    };
    static thread_local std::map<size_t, DivConsts> cache;
    auto it = cache.find(n);
    if (it == cache.end()) {
        DivConsts d;
        const fe g = h_root_of_unity(log_n);
        fe wce = h_root_of_unity(log_n + 3), x = fe_make(3);
        for (int r = 0; r < 8; r++) {
            d.xr[r] = x;
            d.inv_zn[r] = h_inv(fe_sub(h_pow(x, n), fe_one()));  // x^n constant on CE coset r
            x = fe_mul(x, wce);
        }
        d.g_last2 = h_pow(g, n - 2);
        d.g_last1 = h_pow(g, n - 1);
        d.per = periodic_table(n);
        it = cache.emplace(n, std::move(d)).first;
    }
    memcpy(K.xr, it->second.xr, sizeof K.xr);
    memcpy(K.inv_zn, it->second.inv_zn, sizeof K.inv_zn);
    K.g_last2 = it->second.g_last2;
    K.g_last1 = it->second.g_last1;
    K.delta = fe_make(pub->delta);
    K.lwe_size = (int)pub->lwe_size;
    set_coeff_derived(K, it->second.per.data());
    return it->second.per.data();
}

// K[j]: the constants with component j of every coefficient (KX planes; the record keeps the a components)
void zk::draw_air_consts(Coin &coin, const zk_pub_inputs *pub, size_t n, int KX, AirConsts *K, zk_record &R) {
    memset(K, 0, KX * sizeof K[0]);
    for (int k = 0; k < NUM_TCONS; k++) {
        const fe2 v = coin.draw_ext(KX);
        for (int j = 0; j < KX; j++) K[j].coeff_t[k] = j ? v.b : v.a;
        fe_to_bytes(v.a, R.coeff_t[k]);
    }
    for (int k = 0; k < NUM_ASSERTS; k++) {
        const fe2 v = coin.draw_ext(KX);
        for (int j = 0; j < KX; j++) K[j].coeff_b[k] = j ? v.b : v.a;
        fe_to_bytes(v.a, R.coeff_b[k]);
    }
    const fe *per = air_static_consts(pub, n, K[0]);
    if (KX == 2) {  // the b plane: the same constants around its own coefficients
        const AirConsts b = K[1];
        K[1] = K[0];
        memcpy(K[1].coeff_t, b.coeff_t, sizeof b.coeff_t);
        memcpy(K[1].coeff_b, b.coeff_b, sizeof b.coeff_b);
        set_coeff_derived(K[1], per);
    }
}

// hv = ood_eval's output (KX planes of np = 2W + C KX values): T(z), T(zg) and the C KX base composition columns at z.
// Builds the frame e = T(z) ++ T(zg) ++ H(z) (over E: H_c = P_2c + X P_2c+1), its flattened form h (the
// serialization order, KX elements per value), records the a components, reseeds the coin [P7, P15].
void zk::ood_reseed(Coin &coin, int KX, const std::vector<fe> &hv, int C, zk_record &R, std::vector<fe2> &e,
                    std::vector<fe> &h) {
    const int np = 2 * W + C * KX;
    auto val = [&](int s) { return fe2{hv[s], KX == 2 ? hv[np + s] : fe_zero()}; };
    e.assign(2 * W + C, fe2_zero());
    for (int c = 0; c < 2 * W; c++) e[c] = val(c);
    for (int c = 0; c < C; c++)
        e[2 * W + c] = KX == 1 ? val(2 * W + c) : fe2_add(val(2 * W + 2 * c), fe2_mulX(val(2 * W + 2 * c + 1)));
    h.assign(KX * e.size(), fe_zero());
    for (size_t i = 0; i < e.size(); i++) {
        h[KX * i] = e[i].a;
        if (KX == 2) h[2 * i + 1] = e[i].b;
    }
    for (int c = 0; c < W; c++) {
        fe_to_bytes(e[c].a, R.ood_trace_z[c]);
        fe_to_bytes(e[W + c].a, R.ood_trace_zg[c]);
    }
    for (int j = 0; j < C; j++) fe_to_bytes(e[2 * W + j].a, R.ood_constraints[j]);
    uint8_t d[32];
    hash_elems(h.data(), 2 * W * KX, d);  // T(z) || T(zg)
    coin.reseed(d);
    hash_elems(h.data() + 2 * W * KX, C * KX, d);
    coin.reseed(d);
}

template <int KX>
DeepConsts<KX> zk::draw_deep_consts(Coin &coin, const std::vector<fe2> &e, int C, typename Chal<KX>::T z,
                                    typename Chal<KX>::T zg, zk_record &R) {
    typedef Chal<KX> X;
    DeepConsts<KX> D;
    memset(&D, 0, sizeof D);
    typename X::T k1 = X::zero(), k2 = X::zero();
    for (int c = 0; c < W; c++) {
        D.alpha_t[c] = X::make(coin.draw_ext(KX));
        fe_to_bytes(X::comp(D.alpha_t[c], 0), R.deep_t[c]);
        k1 = X::add(k1, X::mul(D.alpha_t[c], X::make(e[c])));
        k2 = X::add(k2, X::mul(D.alpha_t[c], X::make(e[W + c])));
    }
    for (int j = 0; j < C; j++) {
        D.alpha_c[j] = X::make(coin.draw_ext(KX));
        fe_to_bytes(X::comp(D.alpha_c[j], 0), R.deep_c[j]);
        k1 = X::add(k1, X::mul(D.alpha_c[j], X::make(e[2 * W + j])));
    }
    D.k1 = k1;
    D.k2 = k2;
    D.z = z;
    D.zg = zg;
    return D;
}
template DeepConsts<1> zk::draw_deep_consts<1>(Coin &, const std::vector<fe2> &, int, fe, fe, zk_record &);
template DeepConsts<2> zk::draw_deep_consts<2>(Coin &, const std::vector<fe2> &, int, fe2, fe2, zk_record &);

int zk::fri_num_layers(size_t N, const zk_options *opt) {
    const size_t max_rem = (size_t)(opt->fri_rem_max_deg + 1) * opt->blowup;
    int nl = 0;
    for (size_t s = N; s > max_rem; s /= opt->fri_folding) nl++;
    return nl;
}

template <int KX>
FoldConsts<KX> zk::fold_consts(fe2 alpha, uint32_t fold) {
    FoldConsts<KX> F;
    memset(&F, 0, sizeof F);
    const fe zeta_inv = h_inv(h_root_of_unity(ilog2(fold)));
    F.zinv[0] = fe_one();
    for (uint32_t t = 1; t < 16; t++) F.zinv[t] = t < fold ? fe_mul(F.zinv[t - 1], zeta_inv) : fe_zero();
    F.alpha = Chal<KX>::make(alpha);
    F.inv_offset = h_inv(fe_make(3));
    F.inv_fold = h_inv(fe_make(fold));
    return F;
}
template FoldConsts<1> zk::fold_consts<1>(fe2, uint32_t);
template FoldConsts<2> zk::fold_consts<2>(fe2, uint32_t);

// rv: the last layer, KX planes of L values each, natural order over 3 * <w_L>
int zk::remainder_step(int KX, const std::vector<fe> &rv, uint32_t B, Coin &coin, zk_record &R, unsigned &degree_flag,
                       std::vector<fe> &rem_flat) {
    const size_t L = rv.size() / KX, rl = L / B;
    std::vector<fe> v[2];
    for (int j = 0; j < KX; j++) {
        v[j].assign(rv.begin() + j * L, rv.begin() + (j + 1) * L);
        h_interp_coset3_cached(v[j]);
        for (size_t k = rl; k < L; k++)
            if (!fe_is_zero(v[j][k])) degree_flag = 1;
    }
    if (rl > ZK_MAX_REMAINDER) ZK_FAIL(ZK_ERR_INVALID_ARG, "remainder too large");
    R.remainder_len = (uint32_t)rl;
    rem_flat.clear();
    for (size_t k = 0; k < rl; k++) {
        fe_to_bytes(v[0][k], R.remainder[k]);
        for (int j = 0; j < KX; j++) rem_flat.push_back(v[j][k]);
    }
    hash_elems(rem_flat.data(), rem_flat.size(), R.remainder_commitment);
    coin.reseed(R.remainder_commitment);
    return ZK_OK;
}

static bool nonce_ok(const uint8_t seed[32], uint64_t nonce, uint32_t bits) {
    uint8_t d[32];
    Coin::merge_with_int(seed, nonce, d);
    uint64_t head;
    memcpy(&head, d, 8);
    const unsigned tz = head ? (unsigned)__builtin_ctzll(head) : 64;
    return tz >= bits;
}

int zk::grind_and_positions(zk_prover *p, Coin &coin, const zk_options *opt, size_t N, zk_record &R,
                            std::vector<uint64_t> &pos) {
    uint64_t nonce = 1;
    if (p && opt->grinding >= 8) {
        // ~2^grinding BLAKE3 calls: search batches of 2^22 nonces on the GPU, smallest hit wins
        if (!p->pow_seed) {
            ZK_CHECK_HIP(p->arena.alloc(&p->pow_seed, 8));
            ZK_CHECK_HIP(p->arena.alloc(&p->pow_best, 1));
        }
        ZK_TRY(h2d_small(p, p->pow_seed, coin.seed, 32));
        const unsigned long long none = ~0ULL;
        unsigned long long best = none;
        ZK_TRY(h2d_small(p, p->pow_best, &none, 8));
        const uint32_t batch = 1u << 22;
        for (uint64_t start = 1; best == none; start += batch) {
            grind_launch(p->st, p->pow_seed, start, batch, (int)opt->grinding, p->pow_best);
            ZK_TRY(d2h_small(p, &best, p->pow_best, 8));
            ZK_TRY(d2h_flush(p));
        }
        nonce = best;
        if (!nonce_ok(coin.seed, nonce, opt->grinding)) ZK_FAIL(ZK_ERR_DEVICE, "GPU grinding returned an invalid nonce");
    } else {
        while (!nonce_ok(coin.seed, nonce, opt->grinding)) nonce++;
    }
    R.pow_nonce = nonce;
    Coin::merge_with_int(coin.seed, nonce, coin.seed);
    coin.counter = 0;
    pos.clear();
    for (uint32_t q = 0; q < opt->num_queries; q++) {
        uint8_t d[32];
        coin.next(d);
        uint64_t v;
        memcpy(&v, d, 8);
        pos.push_back(v & (N - 1));
    }
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    R.num_positions = (uint32_t)pos.size();
    memcpy(R.positions, pos.data(), pos.size() * 8);
    return ZK_OK;
}

std::vector<std::vector<uint64_t>> zk::fri_fold_positions(const std::vector<uint64_t> &pos, size_t N, uint32_t fold,
                                                          int nl) {
    std::vector<std::vector<uint64_t>> out(nl);
    std::vector<uint64_t> fp = pos;
    size_t dsz = N;
    for (int l = 0; l < nl; l++) {
        const size_t target = dsz / fold;
        std::vector<uint64_t> f;
        for (uint64_t x : fp) {
            const uint64_t q = x % target;
            if (std::find(f.begin(), f.end(), q) == f.end()) f.push_back(q);
        }
        out[l] = f;
        fp = f;
        dsz = target;
    }
    return out;
}

void zk::serialize_proof(size_t n, const zk_options *opt, int C, const zk_record &R, const fe *ood, const Openings &O,
                         const std::vector<fe> *rem_flat, std::vector<uint8_t> &out) {
    const int nl = (int)R.num_fri_layers;
    const int K = (int)opt->field_extension, ES = 16 * K;
    const size_t nu = R.num_positions;
    Bytes pf;
    pf.v.swap(out);  // write into the caller's storage (capacity kept across proofs: no page faults)
    pf.v.clear();
    static thread_local Bytes paths;
    pf.u8(W);
    pf.u8(0);
    pf.u8(0);
    pf.u8((uint8_t)ilog2(n));
    pf.u16(0);
    pf.u8(16);
    pf.u64(ZK_P_LO);
    pf.u64(ZK_P_HI);
    pf.u8((uint8_t)opt->num_queries);
    pf.u8((uint8_t)opt->blowup);
    pf.u8((uint8_t)opt->grinding);
    pf.u8((uint8_t)opt->field_extension);
    pf.u8((uint8_t)opt->fri_folding);
    pf.u8((uint8_t)opt->fri_rem_max_deg);
    pf.u8((uint8_t)nu);
    pf.u16((uint16_t)(32 * (2 + nl + 1)));
    pf.put(R.trace_root, 32);
    pf.put(R.constraint_root, 32);
    for (int l = 0; l < nl; l++) pf.put(R.fri_roots[l], 32);
    pf.put(R.remainder_commitment, 32);
    auto write_queries = [&](const void *vals, size_t vlen, int b) {
        paths.v.clear();
        const BatchPlan &plan = O.plans[b];
        paths.u8((uint8_t)plan.paths.size());
        size_t k = 0;
        for (auto &path : plan.paths) {
            paths.u8((uint8_t)path.size());
            for (size_t t = 0; t < path.size(); t++, k++) paths.put(&O.digests[b][32 * k], 32);
        }
        pf.u32((uint32_t)vlen);
        pf.put(vals, vlen);
        pf.u32((uint32_t)paths.v.size());
        pf.put(paths.v.data(), paths.v.size());
    };
    pf.u8(1);
    write_queries(O.trace_rows.data(), nu * W * 16, 0);
    write_queries(O.comp_rows.data(), nu * C * ES, 1);
    pf.u16((uint16_t)(1 + 2 * W * ES));
    pf.u8(2);
    for (int c = 0; c < W; c++) {
        pf.put(&ood[c * K], ES);
        pf.put(&ood[(W + c) * K], ES);
    }
    pf.u16((uint16_t)(C * ES));
    pf.put(ood + 2 * W * K, C * ES);
    pf.u8((uint8_t)nl);
    for (int l = 0; l < nl; l++) write_queries(O.fri_rows[l].data(), O.fri_rows[l].size() * 16, 2 + l);
    pf.u16((uint16_t)(R.remainder_len * ES));
    if (rem_flat) pf.put(rem_flat->data(), R.remainder_len * ES);
    else pf.put(R.remainder, R.remainder_len * 16);
    pf.u8(0);
    pf.u64(R.pow_nonce);
    pf.u8(0);
    out.swap(pf.v);
}

int zk::deliver_proof(const std::vector<uint8_t> &bytes, unsigned degree_flag, uint8_t *proof_out, size_t *proof_len) {
    int status = degree_flag ? ZK_ERR_DEGREE : ZK_OK;
    if (degree_flag) g_err = "the trace does not satisfy ProcessorAir (composition degree check failed)";
    if (proof_out && *proof_len >= bytes.size())
        memcpy(proof_out, bytes.data(), bytes.size());
    else if (status == ZK_OK) {
        status = ZK_ERR_BUFFER_TOO_SMALL;
        g_err = "proof buffer too small";
    }
    *proof_len = bytes.size();
    return status;
}

// ---------------------------------------------------------------- the single-GPU prove path
// Coset LDE of the ncols column polynomials at `polys` into the coset-major `lde` and the commitment to
// its rows (leaves, nodes; the root is read back with the caller's next d2h_flush).
static int lde_commit(zk_prover *p, Plan *pl, const fe *polys, int ncols, fe *lde, uint8_t *leaves, uint8_t *nodes,
                      uint8_t root[32]) {
    const int log_n = pl->log_n, log_b = pl->log_b;
    const size_t n = (size_t)1 << log_n, B = (size_t)1 << log_b;
    ntt_lde(p->st, pl->Tn, pl->ct, polys, n, ncols, 0, 1, (int)B, lde, B * n, n, p->tmp);
    hash_rows_cosets(p->st, lde, ncols, log_n, log_b, 0, log_b, leaves);
    merkle_tree(p->st, leaves, n * B, nodes);
    return d2h_small(p, root, nodes + 32, 32);
}

static void coset_major_rows_to_host(zk_prover *p, const fe *base, int ncols, size_t n, uint32_t B, uint8_t *dst) {
    // dst: N x ncols row-major (natural index)
    size_t N = n * B;
    std::vector<fe> h((size_t)ncols * N);
    (void)hipMemcpy(h.data(), base, h.size() * sizeof(fe), hipMemcpyDeviceToHost);
    fe *o = reinterpret_cast<fe *>(dst);
    for (int c = 0; c < ncols; c++)
        for (size_t i = 0; i < N; i++) o[i * ncols + c] = h[((size_t)c * B + (i % B)) * n + i / B];
}

// FieldExtension::Quadratic buffers (planar E): composition 2 x 8n, its inverse NTT, the composition LDE
// (up to 2 x 8 base columns), DEEP 2N, FRI layers 2(N + 16), OOD tables and partial sums.
int zk::ensure_ext(zk_prover *p) {
    if (p->x_comp) return ZK_OK;
    const size_t n = p->max_n, N = n * p->max_b, CE = 8 * n;
    const size_t Nl = p->shard_world ? N / (size_t)p->shard_world : N;  // LDE points held (see create_prover)
    DeviceArena &A = p->arena;
    ZK_CHECK_HIP(A.alloc(&p->x_comp, 2 * CE));
    ZK_CHECK_HIP(A.alloc(&p->x_ctmp, 2 * CE));
    ZK_CHECK_HIP(A.alloc(&p->x_clde, (size_t)2 * 8 * Nl));  // C <= 8 E columns
    ZK_CHECK_HIP(A.alloc(&p->x_deep, 2 * Nl));
    ZK_CHECK_HIP(A.alloc(&p->x_fri, 2 * (N + 16)));
    ZK_CHECK_HIP(A.alloc(&p->x_partials, (size_t)2 * (2 * ZK_MAX_COLS + ZK_MAX_CCOLS) * ood_waves(n)));
    ZK_CHECK_HIP(A.alloc(&p->x_tab, (size_t)2 * (128 + 2 * ood_waves(n))));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->x_air, 2 * sizeof(AirConsts)));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->x_deep_consts, sizeof(DeepConsts<2>)));
    ZK_CHECK_HIP(A.alloc((uint8_t **)&p->x_fold_consts, sizeof(FoldConsts<2>)));
    if (!p->shard_world) ZK_CHECK_HIP(A.alloc(&p->x_ulde, 2 * N));
    ZK_CHECK_HIP(A.alloc(&p->x_dscratch, DeepScratch::size(n, 2)));
    return ZK_OK;
}

// S4, shared by zk_prove_device and plug point 3 (build_constraint_commitment): interpolate the 8n
// composition values (coset-major in comp, KX planes) over the CE coset, split the polynomial into C
// column polynomials of n coefficients (p->cpolys; base column (c, j) of E column c at (c*KX + j)*n),
// extend them over the B LDE cosets into clde and commit to its rows (a leaf is C E values).
// p->flag is set when the interpolant has a coefficient at or beyond C*n (the degree check).
// bnd (KX coefficient planes, or nullptr when comp already holds the assertion terms): add the assertion
// terms' quotient polynomial to column 0 of each plane (boundary_poly_add) before the LDE.
// nce = 7 (C <= 7): only CE cosets 0..6 were evaluated; the cross-coset step derives coset 7 from the degree
// bound (CrossMap::derive7).  Same polynomial for a trace that satisfies the AIR; for one that does not, the
// out-of-domain identity check (check_ood_identity) reports it instead of the top-block flag.
// TS, w (with bnd): where the boundary quotient reads the trace coefficients (CoeffSrc and its scalars; null: p->polys).
static int composition_stage(zk_prover *p, Plan *pl, int KX, int C, fe *comp, fe *ctmp, fe *clde, uint8_t root[32],
                             const AirConsts *bnd = nullptr, int nce = 8, const CoeffSrc *TS = nullptr,
                             const fe *w = nullptr) {
    const size_t n = (size_t)1 << pl->log_n, CE = 8 * n;
    const int CK = C * KX;
    if (nce != 8 && (nce != 7 || C > 7)) ZK_FAIL(ZK_ERR_INVALID_ARG, "composition: unsupported CE coset count");
    if (nce == 8) ntt(p->st, pl->Tn, comp, n, ctmp, n, 8 * KX, true, nullptr, nullptr, p->tmp);
    else
        for (int j = 0; j < KX; j++) ntt(p->st, pl->Tn, comp + j * CE, n, ctmp + j * CE, n, nce, true, nullptr, nullptr, p->tmp);
    ZK_CHECK_HIP(hipMemsetAsync(p->flag, 0, 4, p->st));
    const fe w8 = h_root_of_unity(3);
    for (int j = 0; j < KX; j++) {
        CrossMap m;
        for (int r = 0; r < 8; r++) m.c[r] = ctmp + (size_t)(8 * j + r) * n;
        m.k0 = 0;
        m.kcount = n;
        m.pstride = (size_t)KX * n;
        if (nce == 7) {
            m.derive7 = 1;
            fe w = w8;
            for (int r = 0; r < 7; r++, w = fe_mul(w, w8)) m.k7[r] = fe_sub(fe_zero(), w);  // -w_8^(r+1)
        }
        comp_cross_mapped(p->st, m, pl->Tce, pl->inv3, h_inv(fe_make(CE)), h_inv(w8), h_inv(h_pow(fe_make(3), n)), C,
                          p->cpolys + (size_t)j * n, p->flag);
    }
    if (bnd) {
        const CoeffSrc plain = coeff_plain(p->polys, n);
        for (int j = 0; j < KX; j++)
            boundary_poly_add(p->st, TS ? *TS : plain, w, pl->log_n, bnd[j], bnd[0].g_last2, p->dscratch,
                              p->cpolys + (size_t)j * n, p->flag);
    }
    return lde_commit(p, pl, p->cpolys, CK, clde, p->cleaves, p->cnodes, root);
}

// Degree check of the composition: the verifier's out-of-domain identity (zk::ood_identity) on the
// frame the proof will carry.  For a trace that satisfies ProcessorAir the composition columns are
// exactly C(x)/Z(x) + boundary quotients, so the identity holds; for any other trace the committed
// columns interpolate a function that is not a polynomial of degree < C*n and the identity fails at the
// transcript-derived z except with probability ~ (degree / p) ~ 2^-100 (Schwartz-Zippel).
// K: the composition coefficients (planes a, b for FieldExtension::Quadratic).
static int check_ood_identity(const std::vector<fe2> &e, int C, const AirConsts *K, int KX, fe2 z, size_t n,
                              const zk_pub_inputs *pub) {
    fe2 ct[NUM_TCONS], cb[NUM_ASSERTS];
    for (int k = 0; k < NUM_TCONS; k++) ct[k] = fe2{K[0].coeff_t[k], KX == 2 ? K[1].coeff_t[k] : fe_zero()};
    for (int k = 0; k < NUM_ASSERTS; k++) cb[k] = fe2{K[0].coeff_b[k], KX == 2 ? K[1].coeff_b[k] : fe_zero()};
    if (!ood_identity(e.data(), C, ct, cb, z, n, pub))
        ZK_FAIL(ZK_ERR_DEGREE, "the trace does not satisfy ProcessorAir (out-of-domain constraint identity failed)");
    return ZK_OK;
}

static int prove_once(zk_prover *p, const TraceSrc &src, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                      uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump);

// One proof, plus the hints' bookkeeping for host-resident traces (trace_commit.hip): a hinted column that the host
// check refutes voids the proof, which is redone without hints; a completed proof leaves the columns it found sparse
// and narrow (8- or 32-bit before the last row) as the next proof's hints.
static int prove_impl(zk_prover *p, TraceSrc src, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                      uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump) {
    if (dump) src.no_virtual = true;  // the stage dumps read every trace LDE column
    if (src.cols && pub) {
        src.key = &pub->program_hash[0][0];  // hints are per (n, program)
        src.lwe = pub->lwe_size;
    }
    p->tc = {};
    const size_t cap = proof_len ? *proof_len : 0;  // (in/out: a voided attempt has overwritten it with its length)
    int rc = prove_once(p, src, n, opt, pub, proof_out, proof_len, rec, dump);
    if (trace_hints_refuted(p, src, n, rc)) {  // prove again from every column
        src.hint_ok = false;
        *proof_len = cap;
        rc = prove_once(p, src, n, opt, pub, proof_out, proof_len, rec, dump);
    }
    trace_hints_learn(p, src, n, rc);
    return rc;
}

zk_record zk::record_init(size_t n, size_t N, int C) {
    zk_record R;
    memset(&R, 0, sizeof R);
    R.trace_len = (uint32_t)n;
    R.lde_len = (uint32_t)N;
    R.width = W;
    R.num_ccols = (uint32_t)C;
    return R;
}

int zk::fri_lead_layers(zk_prover *p, const Plan *pl, int KX, uint32_t fold, uint32_t B, size_t N, int l0, int lb0,
                        fe *next, uint8_t *dig, FriLayers &Y, Coin &coin, zk_record &R, unsigned &degree_flag,
                        HostTimer *ht) {
    const int nl = (int)R.num_fri_layers;
    // the constant part of the fold constants is uploaded once; each layer's coin writes alpha into it
    void *fc = planes(p, KX).fold_consts;
    fe *alpha_dev = nullptr;
    ZK_TRY(with_kx(KX, [&](auto kx) {
        const auto F = fold_consts<decltype(kx)::value>(fe2_zero(), fold);
        alpha_dev = (fe *)&((decltype(F) *)fc)->alpha;
        return h2d_small(p, fc, &F, sizeof F);
    }));
    ZK_TRY(h2d_small(p, p->fri_seed, coin.seed, 32));  // (the next reseed restarts the counter)
    for (int l = l0; l < nl; l++) {
        const size_t L = Y.len[l], rows = L / fold;
        Y.leaves[l] = dig;
        Y.nodes[l] = dig + 32 * rows;
        dig += 64 * rows;
        const int lb = l == l0 ? lb0 : 0;
        commit_fri_layer(p->st, KX, Y.vals[l], L, (int)fold, Y.leaves[l], Y.nodes[l], lb);
        fri_coin_launch(p->st, (uint32_t *)p->fri_seed, Y.nodes[l] + 32, KX, alpha_dev, p->fri_alphas + 2 * l);
        fri_fold_launch(p->st, KX, Y.vals[l], L, (int)fold, fc, pl->TN, N / L, next, lb);
        Y.vals[l + 1] = next;
        Y.len[l + 1] = rows;
        next += KX * rows;
    }
    // one round trip for the whole commit phase: roots, device alphas, the last layer
    std::vector<fe> rv(KX * Y.len[nl]), dalpha(2 * nl);
    for (int l = l0; l < nl; l++) ZK_TRY(d2h_small(p, R.fri_roots[l], Y.nodes[l] + 32, 32));
    if (nl > l0) ZK_TRY(d2h_small(p, dalpha.data() + 2 * l0, p->fri_alphas + 2 * l0, 2 * (nl - l0) * sizeof(fe)));
    ZK_TRY(d2h_small(p, rv.data(), Y.vals[nl], rv.size() * sizeof(fe)));
    ZK_TRY(d2h_flush(p));
    if (ht) ht->start();
    // host replay of the same transcript (it continues into the remainder, grinding and queries)
    for (int l = l0; l < nl; l++) {
        coin.reseed(R.fri_roots[l]);
        const fe2 alpha = coin.draw_ext(KX);
        fe_to_bytes(alpha.a, R.fri_alphas[l]);
        if (!fe_eq(alpha.a, dalpha[2 * l]) || (KX == 2 && !fe_eq(alpha.b, dalpha[2 * l + 1])))
            ZK_FAIL(ZK_ERR_DEVICE, "device FRI transcript diverged from the host transcript");
    }
    if (ht) ht->lap("fri_replay");
    return remainder_step(KX, rv, B, coin, R, degree_flag, Y.rem_flat);
}

void Openings::unpack(const fe *got, size_t nu, int CK, const std::vector<std::vector<uint64_t>> &fri_pos,
                      uint32_t fold, int KX, size_t off_dig) {
    trace_rows.assign(got, got + nu * W);
    size_t off = nu * W;
    comp_rows.assign(got + off, got + off + nu * CK);
    off += nu * CK;
    for (size_t l = 0; l < fri_rows.size(); l++) {
        fri_rows[l].assign(got + off, got + off + fri_pos[l].size() * fold * KX);
        off += fri_pos[l].size() * fold * KX;
    }
    const uint8_t *dg = (const uint8_t *)(got + off_dig);
    for (size_t b = 0; b < plans.size(); b++) {
        const size_t bytes = 32 * plans[b].count();
        digests[b].assign(dg, dg + bytes);
        dg += bytes;
    }
}

// S5 on one GPU: z from the coin, the OOD frame (its flattened form into h), the DEEP constants and the DEEP LDE into
// the plane set's ulde (coset-major) and, deep_out != nullptr, in natural order into deep_out.
template <int KX>
static int ood_deep_stage(zk_prover *p, Plan *pl, Coin &coin, zk_record &R, HostTimer &HT, int C, const AirConsts *Kp,
                          const zk_pub_inputs *pub, fe *deep_out, std::vector<fe> &h) {
    typedef Chal<KX> X;
    const Planes b = planes(p, KX);
    const int log_n = pl->log_n;
    const typename X::T z = X::make(coin.draw_ext(KX)), zg = X::mulb(z, h_root_of_unity(log_n));
    fe_to_bytes(X::comp(z, 0), R.z);
    // the trace coefficients where this proof's commitment left them (p->csrc: p->polys, or the derived columns' sources)
    const CoeffSrc &TS = p->csrc;
    ood_eval(p->st, TS, W, p->cpolys, C * KX, log_n, z, zg, b.ood_tab, b.partials, p->ood);
    HT.stop("z");
    std::vector<fe> raw((size_t)KX * ood_out_values(TS, W, C * KX)), hv((size_t)KX * (2 * W + C * KX));
    ZK_TRY(d2h_small(p, raw.data(), p->ood, raw.size() * sizeof(fe)));
    ZK_TRY(d2h_flush(p));
    HT.start();
    ood_fold_sources(KX, W, C * KX, TS, p->csrc_w, raw.data(), hv.data());
    std::vector<fe2> e;
    ood_reseed(coin, KX, hv, C, R, e, h);
    stage_mark(p, "ood");
    DeepConsts<KX> D = draw_deep_consts<KX>(coin, e, C, z, zg, R);
    deep_source_weight(D, TS, p->csrc_w);
    ZK_TRY(h2d_small(p, b.deep_consts, &D, sizeof D));
    deep_coeff_launch(p->st, pl->Tn, TS, p->cpolys, C, log_n, pl->log_b, b.deep_consts, z, zg, pl->ct, b.dscratch,
                      b.ulde, p->tmp, deep_out);
    HT.stop("deep_consts");
    // while the GPU runs DEEP: the verifier's out-of-domain identity on the frame just read
    return check_ood_identity(e, C, Kp, KX, X::wide(z), (size_t)1 << log_n, pub);
}

// ---- the stages both provers run the same way (ProofRun, prover_internal.hpp)
int ProofRun::fri_shape() {
    nl = fri_num_layers(N, opt);
    if (nl > ZK_MAX_FRI_LAYERS) ZK_FAIL(ZK_ERR_INVALID_ARG, "too many FRI layers");
    R.num_fri_layers = (uint32_t)nl;
    Y = FriLayers(nl);
    Y.len[0] = N;
    return ZK_OK;
}

int ProofRun::open_plans(zk_prover *lead, size_t rows0) {
    ZK_TRY(grind_and_positions(lead, coin, opt, N, R, pos));
    fri_pos = fri_fold_positions(pos, N, fold, nl);
    if (ht) ht->lap("positions");
    if (!lead->open) lead->open = new Openings();
    O = lead->open;
    O->reset(2 + nl);
    plan_batch(N, pos, O->plans[0]);
    O->plans[1] = O->plans[0];  // the composition tree opens the same positions
    for (int l = 0; l < nl; l++) plan_batch(l == 0 ? rows0 : Y.len[l] / fold, fri_pos[l], O->plans[2 + l]);
    return ZK_OK;
}

int ProofRun::finish(zk_prover *lead, uint8_t *proof_out, size_t *proof_len, zk_record *rec) {
    if (ht) ht->start();
    serialize_proof(n, opt, C, R, h.data(), *O, KX == 2 ? &Y.rem_flat : nullptr, lead->proof_bytes);
    if (ht) ht->stop("serialize");
    stage_mark(lead, "serialize");
    ZK_CHECK_HIP(hipStreamSynchronize(lead->st));
    stage_collect(lead);
    collect_kernel_stats(lead);
    if (rec) *rec = R;
    return deliver_proof(lead->proof_bytes, degree_flag, proof_out, proof_len);
}

// One single-GPU proof: the per-proof state and the protocol's stages S0 .. S9 (the list at the top of this file) as
// methods that prove_once calls in order.  A stage queues its GPU work before its host segment (HT) starts.
struct SingleProof : ProofRun {
    zk_prover *const p;
    const TraceSrc &src;
    const zk_dump *const dump;
    const uint32_t B = opt->blowup;
    Plan *pl = nullptr;
    int log_n = 0, log_b = 0;
    Planes pb = {};
    HostTimer HT;
    // The assertion terms are not evaluated per row: S4 adds them in coefficient form (unless the caller dumps the
    // composition values, which must then include them).
    const bool bnd_rows = dump && dump->composition;
    // CE cosets evaluated: 7 when the composition has at most 7 columns (the composition stage derives the 8th)
    const int nce = (!bnd_rows && C <= 7) ? 7 : 8;
    AirConsts Kp[2];
    // FRI layer 0 is the DEEP LDE, coset-major as the coset NTT wrote it (FriLayout lb0 = log_b), unless it is
    // already the remainder (no fold layers), which the host reads in natural order
    int lb0 = 0;
    size_t na = 0;  // chunks the proof opens (open_addresses)
    SingleProof(zk_prover *p_, const TraceSrc &src_, size_t n_, const zk_options *opt_, const zk_pub_inputs *pub_,
                const zk_dump *dump_)
        : ProofRun(opt_, pub_, n_, num_comp_cols(n_)), p(p_), src(src_), dump(dump_) {
        ht = &HT;
    }
    int start(int others) {
        // the AUTO rule (include/zkvm_gpu.h, zk_proof_info): the latency schedule iff no other proof is in flight on the
        // device (others = 0)
        const int sched = p->upload_sched;
        p->lat_sched = sched == ZK_SCHED_LATENCY || (sched == ZK_SCHED_AUTO && others == 0);
        p->last_sched = src.cols ? (p->lat_sched ? ZK_SCHED_LATENCY : ZK_SCHED_THROUGHPUT) : 0;
        ZK_TRY(get_plan(p, n, B, &pl));
        log_n = pl->log_n, log_b = pl->log_b;
        if (C > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "composition column count exceeds 8");
        if (KX == 2) ZK_TRY(ensure_ext(p));
        pb = planes(p, KX);
        lb0 = fri_num_layers(N, opt) > 0 ? log_b : 0;
        stage_begin(p);
        stage_mark(p, "start");
        coin = seed_coin(n, opt, pub);  // S0 [P1]
        return ZK_OK;
    }
    // S2: trace LDE + commitment
    int commit_trace() {
        ZK_TRY(trace_lde_commit(p, pl, src, n, R.trace_root));
        ZK_TRY(d2h_flush(p));
        stage_mark(p, "trace_commit");
        HT.start();
        coin.reseed(R.trace_root);
        return ZK_OK;
    }
    // S3: constraint composition coefficients [P4] and evaluation over the CE domain.  With FieldExtension::Quadratic
    // the coefficients are E values and the composition has two planes (a, b): the evaluator folds every constraint
    // value into both, each with that component of every coefficient.
    int constraints() {
        draw_air_consts(coin, pub, n, KX, Kp, R);
        ZK_TRY(h2d_small(p, pb.air_consts, Kp, KX * sizeof Kp[0]));
        const fe *binv = boundary_inverses(p, pl);
        if (!binv) ZK_FAIL(ZK_ERR_OUT_OF_MEMORY, "boundary divisor table");
        ZK_CHECK_HIP(eval_constraints(p->st, KX, p->lde, log_n, eval_map_whole(log_b, nce, bnd_rows), pl->periodic, binv,
                                      (const AirConsts *)pb.air_consts, (size_t)8 << log_n, pb.comp, bnd_rows));
        HT.stop("air_consts");
        stage_mark(p, "constraints");
        return ZK_OK;
    }
    // S4: composition polynomial (interpolate over the CE coset, segment into C columns) + commit
    int composition() {
        ZK_TRY(composition_stage(p, pl, KX, C, pb.comp, pb.ctmp, pb.clde, R.constraint_root, bnd_rows ? nullptr : Kp, nce,
                                 &p->csrc, p->csrc_w));
        ZK_TRY(d2h_small(p, &degree_flag, p->flag, 4));
        ZK_TRY(d2h_flush(p));
        stage_mark(p, "composition");
        HT.start();
        coin.reseed(R.constraint_root);
        return ZK_OK;
    }
    // S5: OOD frame [P7], DEEP coefficients [P8] and evaluations (ood_deep_stage)
    int ood_deep() {
        const int rc = with_kx(KX, [&](auto kx) {
            return ood_deep_stage<decltype(kx)::value>(p, pl, coin, R, HT, C, Kp, pub, lb0 ? nullptr : pb.deep, h);
        });
        // a trace the AIR rejects ends here (the out-of-domain identity): the stages that ran are still dumped, as the
        // oracle dumps them, so the evaluator can be compared on traces no program produces
        if (rc == ZK_ERR_DEGREE && dump) {
            ZK_CHECK_HIP(hipStreamSynchronize(p->st));
            ZK_TRY(dump_front());
        }
        if (rc == ZK_OK) stage_mark(p, "deep");
        return rc;
    }
    // S6: FRI [P9, P10]; E layers are planar (KX planes of L values)
    int fri() {
        ZK_TRY(fri_shape());
        size_t tot = 0, s = N;
        for (int l = 0; l < nl; l++) tot += (s /= fold);
        if (tot > p->max_n * p->max_b) ZK_FAIL(ZK_ERR_INVALID_ARG, "FRI layers exceed the prover's buffers");
        Y.vals[0] = lb0 ? pb.ulde : pb.deep;
        ZK_TRY(fri_lead_layers(p, pl, KX, fold, B, N, 0, lb0, pb.fri, p->fri_dig, Y, coin, R, degree_flag, &HT));
        stage_mark(p, "fri");
        HT.lap("remainder");
        return ZK_OK;
    }
    // S7, S8: positions, then every value and digest the proof opens as a list of 16-byte device chunks: one address
    // upload, one gather kernel, one download
    int openings() {
        ZK_TRY(open_plans(p, N / fold));
        ZK_TRY(open_addresses());
        HT.stop("plans_addresses");
        ZK_TRY(gather());
        scale_virtual();
        stage_mark(p, "queries");
        return ZK_OK;
    }
    // the chunks' addresses into the prover's pinned list (na of them): the trace rows, the composition rows, every
    // layer's fold rows, then from off_dig every plan's digests.  A virtual column's chunk is e_(n-1)'s LDE instead.
    int open_addresses() {
        uint64_t *addr = p->h_gather_idx;
        na = 0;
        auto fe_at = [&](const fe *base, size_t idx) { addr[na++] = (uint64_t)(uintptr_t)(base + idx); };
        auto row_at = [&](const fe *base, int ncols, uint64_t i) {  // coset-major LDE row i
            for (int c = 0; c < ncols; c++) {
                if (base == p->lde && ((p->tc.virt >> c) & 1u)) fe_at(p->tc.virt_lagr, (i & (B - 1)) * n + (i >> log_b));
                else fe_at(base, ((size_t)c * B + (i & (B - 1))) * n + (i >> log_b));
            }
        };
        size_t need = pos.size() * (W + CK);
        for (int l = 0; l < nl; l++) need += fri_pos[l].size() * fold * KX;
        for (int b = 0; b < 2 + nl; b++) need += 2 * O->plans[b].count();
        if (need > ZK_GATHER_CAP) ZK_FAIL(ZK_ERR_INVALID_ARG, "too many opened values for the gather buffer");
        for (uint64_t q : pos) row_at(p->lde, W, q);
        for (uint64_t q : pos) row_at(pb.clde, CK, q);
        for (int l = 0; l < nl; l++) {
            const size_t rows = Y.len[l] / fold;
            for (uint64_t r : fri_pos[l])
                for (uint32_t k = 0; k < fold; k++)
                    for (int j = 0; j < KX; j++) {
                        const uint64_t i = r + k * rows;  // natural index in layer l
                        fe_at(Y.vals[l], j * Y.len[l] + ((l || !lb0) ? i : ((i & (B - 1)) << log_n) + (i >> log_b)));
                    }
        }
        off_dig = na;
        for (int b = 0; b < 2 + nl; b++) {
            const uint8_t *lv = b == 0 ? p->leaves : b == 1 ? p->cleaves : Y.leaves[b - 2];
            const uint8_t *nd = b == 0 ? p->nodes : b == 1 ? p->cnodes : Y.nodes[b - 2];
            for (auto &path : O->plans[b].paths)
                for (auto &e : path) {
                    const uint8_t *d = (e.first ? nd : lv) + 32 * e.second;
                    addr[na++] = (uint64_t)(uintptr_t)d;
                    addr[na++] = (uint64_t)(uintptr_t)(d + 16);
                }
        }
        return ZK_OK;
    }
    int gather() {
        ZK_CHECK_HIP(hipMemcpyAsync(p->gather_idx, p->h_gather_idx, na * 8, hipMemcpyHostToDevice, p->st));
        gather_chunks(p->st, p->gather_idx, na, p->gather_out);
        ZK_CHECK_HIP(hipMemcpyAsync(p->h_gather_out, p->gather_out, na * sizeof(fe), hipMemcpyDeviceToHost, p->st));
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        O->unpack(p->h_gather_out, pos.size(), CK, fri_pos, fold, KX, off_dig);
        return ZK_OK;
    }
    void scale_virtual() {  // virtual columns: the gather read e_(n-1)'s LDE there; times the column's last row
        if (!p->tc.virt) return;
        for (size_t q = 0; q < pos.size(); q++)
            for (int c = 0; c < W; c++)
                if ((p->tc.virt >> c) & 1u) O->trace_rows[q * W + c] = fe_mul(O->trace_rows[q * W + c], p->tc.virt_last[c]);
    }

    // the stage dumps up to the composition commitment (E-valued stages dump their a component, as the oracle does)
    int dump_front() {
        if (dump->trace_polys) ZK_CHECK_HIP(hipMemcpy(dump->trace_polys, p->polys, (size_t)W * n * 16, hipMemcpyDeviceToHost));
        if (dump->trace_lde) coset_major_rows_to_host(p, p->lde, W, n, B, dump->trace_lde);
        if (dump->trace_leaves) ZK_CHECK_HIP(hipMemcpy(dump->trace_leaves, p->leaves, 32 * N, hipMemcpyDeviceToHost));
        if (dump->composition) coset_major_rows_to_host(p, pb.comp, 1, n, 8, dump->composition);
        if (dump->comp_polys) ZK_CHECK_HIP(hipMemcpy(dump->comp_polys, p->cpolys, (size_t)CK * n * 16, hipMemcpyDeviceToHost));
        if (dump->comp_lde) coset_major_rows_to_host(p, pb.clde, CK, n, B, dump->comp_lde);
        return ZK_OK;
    }
    // ... and after it: DEEP in natural order, FRI layer 1
    int dump_back() {
        if (dump->deep) {
            if (lb0) coset_major_to_natural(p->st, Y.vals[0], log_n, log_b, pb.deep);
            ZK_CHECK_HIP(hipStreamSynchronize(p->st));
            ZK_CHECK_HIP(hipMemcpy(dump->deep, pb.deep, N * 16, hipMemcpyDeviceToHost));
        }
        if (dump->fri_layer1 && nl > 0)
            ZK_CHECK_HIP(hipMemcpy(dump->fri_layer1, Y.vals[1], Y.len[1] * 16, hipMemcpyDeviceToHost));
        return ZK_OK;
    }
    // S9: proof bytes, then the dumps of a completed proof (the stream is idle)
    int finish(uint8_t *proof_out, size_t *proof_len, zk_record *rec) {
        const int rc = ProofRun::finish(p, proof_out, proof_len, rec);
        if (!p->stage_done) return rc;  // (the stream did not drain)
        if (dump) {
            ZK_TRY(dump_front());
            ZK_TRY(dump_back());
        }
        p->last_n = n;
        p->last_b = B;
        return rc;
    }
};

// Copies from the caller's host columns may still be in flight on an early error return: the caller may free those
// columns as soon as the proof returns (a completed proof has long finished them).  Kernels of a failed proof may also
// still be queued on st: the next proof's uploads into d_trace (on the upload stream, ordered only by the previous proof
// having drained st) must not race them, so both drain on every way out.
struct CopyGuard {
    zk_prover *p;
    ~CopyGuard() {
        upload_drain(p);
        (void)hipStreamSynchronize(p->st);
    }
};

static int prove_once(zk_prover *p, const TraceSrc &src, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                      uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump) {
    if (!p || !proof_len) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    ZK_TRY(check_prove_args(n, p->max_n, p->max_b, opt, pub));
    // proofs in flight on the device: alone, the trace goes up on the latency schedule (trace_commit.hip).  Declared
    // before the copy guard, so this proof counts as in flight until its uploads and kernels have drained; a stage
    // that ends the proof early returns through all three guards.
    DeviceBusy busy{p->dev_busy};
    CopyGuard copy_guard{p};
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    SingleProof S(p, src, n, opt, pub, dump);
    ZK_TRY(S.start(busy.others));
    ZK_TRY(S.commit_trace());
    ZK_TRY(S.constraints());
    ZK_TRY(S.composition());
    ZK_TRY(S.ood_deep());
    ZK_TRY(S.fri());
    ZK_TRY(S.openings());
    return S.finish(proof_out, proof_len, rec);
}

// ---------------------------------------------------------------- trace validation
// Trace::validate (winterfell 0.9, the debug-build step of Prover::prove) on the GPU: include/zkvm_gpu.h
// "trace validation" fixes the semantics; kernels.hip k_validate_trace is the device side.
static std::string u128_dec(fe v) {
    unsigned __int128 x = ((unsigned __int128)v.hi << 64) | v.lo;
    if (!x) return "0";
    std::string s;
    while (x) {
        s.insert(s.begin(), (char)('0' + (int)(x % 10)));
        x /= 10;
    }
    return s;
}

// the trace is on p's device at d_trace; arguments are checked
static int validate_on_device(zk_prover *p, const fe *d_trace, size_t n, const zk_pub_inputs *pub, zk_validation *out) {
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    zk_validation V;
    memset(&V, 0, sizeof V);
    V.trace_len = n;
    V.steps_checked = n - 2;
    V.first_index = -1;
    // get_assertions (air/src/lib.rs:170-195), in its own order
    fe expect[NUM_ASSERTS];
    {
        int k = 0;
        auto put = [&](int col, size_t step, fe v) {
            V.a_col[k] = (uint32_t)col;
            V.a_step[k] = step;
            expect[k] = v;
            fe_to_bytes(v, V.a_expected[k]);
            k++;
        };
        put(0, 0, fe_zero());
        put(11, 0, fe_zero());
        for (int i = 0; i < 2; i++) {
            put(7 + i, 0, fe_zero());
            put(7 + i, n - 2, fe_from_bytes(pub->program_hash[i]));
        }
        for (int i = 0; i < 8; i++) {
            put(12 + i, 0, fe_zero());
            put(12 + i, n - 2, fe_from_bytes(pub->stack_outputs[i]));
        }
    }
    ValReport R;
    memset(&R, 0, sizeof R);
    for (int k = 0; k < NUM_TCONS; k++) R.t_first[k] = ~0ull;
    for (int k = 0; k < NUM_ASSERTS; k++) R.a_found[k] = expect[k];
    ZK_TRY(h2d_small(p, p->val_rep, &R, sizeof R));
    ZK_CHECK_HIP(validate_trace(p->st, d_trace, n, p->val_per, fe_make(pub->delta), (int)pub->lwe_size, p->val_rep));
    ZK_TRY(d2h_small(p, &R, p->val_rep, sizeof R));
    ZK_TRY(d2h_flush(p));
    V.failing_steps = R.failing_steps;
    V.a_mask = R.a_mask;
    V.a_failed = (uint32_t)__builtin_popcount(R.a_mask);
    for (int k = 0; k < NUM_ASSERTS; k++) fe_to_bytes(R.a_found[k], V.a_found[k]);
    for (int k = 0; k < ZK_MAX_TCONS; k++) V.t_first[k] = UINT64_MAX;
    // the slow path: per failing constraint, rows t_first and t_first + 1 come back (28 pairs of neighbouring cells,
    // one strided copy) and the host evaluator fills the value -- and must agree that it is not zero
    for (int k = 0; k < NUM_TCONS; k++) {
        V.t_count[k] = R.t_count[k];
        if (!R.t_count[k]) continue;
        const uint64_t s = R.t_first[k];
        if (s >= n - 2) ZK_FAIL(ZK_ERR_DEVICE, "trace validation: the device reported a step outside the trace");
        V.t_first[k] = s;
        fe rows[W][2], cur[W], nxt[W], per[9], ev[NUM_TCONS];
        ZK_CHECK_HIP(hipMemcpy2DAsync(rows, 2 * sizeof(fe), d_trace + s, n * sizeof(fe), 2 * sizeof(fe), W,
                                      hipMemcpyDeviceToHost, p->st));
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        for (int c = 0; c < W; c++) {
            cur[c] = rows[c][0];
            nxt[c] = rows[c][1];
        }
        air_periodic_row((size_t)s, per);
        air_eval_base(cur, nxt, per, pub->lwe_size, pub->delta, ev);
        if (fe_is_zero(ev[k]))
            ZK_FAIL(ZK_ERR_DEVICE, "trace validation: device and host evaluators disagree at step " + std::to_string(s) +
                                       " (transition constraint " + std::to_string(k) + ")");
        fe_to_bytes(ev[k], V.t_value[k]);
    }
    // the first failure as winterfell's Trace::validate meets it: assertions first, then steps in order
    std::string msg;
    if (V.a_mask) {
        const int k = __builtin_ctz(V.a_mask);
        V.first_kind = 1;
        V.first_index = k;
        V.first_step = V.a_step[k];
        msg = "trace does not satisfy assertion main_trace(" + std::to_string(V.a_col[k]) + ", " +
              std::to_string(V.a_step[k]) + ") == " + u128_dec(expect[k]);
    } else if (V.failing_steps) {
        int best = -1;
        for (int k = 0; k < NUM_TCONS; k++)
            if (V.t_count[k] && (best < 0 || V.t_first[k] < V.t_first[best])) best = k;
        if (best < 0) ZK_FAIL(ZK_ERR_DEVICE, "trace validation: failing steps without a failing constraint");
        V.first_kind = 2;
        V.first_index = best;
        V.first_step = V.t_first[best];
        msg = "main transition constraint " + std::to_string(best) + " did not evaluate to ZERO at step " +
              std::to_string(V.first_step);
    }
    p->val_last = V;
    p->val_have = true;
    *out = V;
    if (V.first_kind == 0) return ZK_OK;
    ZK_FAIL(ZK_ERR_TRACE, msg + "; " + std::to_string(V.failing_steps) + " failing steps, " + std::to_string(V.a_failed) +
                              " failed assertions");
}

static int check_validate_args(zk_prover *p, const void *trace, size_t n, const zk_pub_inputs *pub, zk_validation *out) {
    if (!p || !trace || !pub || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    ZK_TRY(check_trace_len(n, p->max_n));
    return check_lwe_size(pub);
}

int zk_validate_device(zk_prover *p, const void *d_trace, size_t n, const zk_pub_inputs *pub, zk_validation *out) {
    ZK_TRY(check_validate_args(p, d_trace, n, pub, out));
    return validate_on_device(p, (const fe *)d_trace, n, pub, out);
}

int zk_validate_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub,
                        zk_validation *out) {
    ZK_TRY(check_validate_args(p, columns, n, pub, out));
    for (int c = 0; c < W; c++)
        if (!columns[c]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null trace column");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    // one full upload, every column whole (a debugging aid: none of the prove path's column classes)
    for (int c = 0; c < W; c++)
        ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace + (size_t)c * n, columns[c], n * sizeof(fe), hipMemcpyHostToDevice, p->st));
    const int rc = validate_on_device(p, p->d_trace, n, pub, out);
    (void)hipStreamSynchronize(p->st);  // the caller's columns are free again on every way out
    return rc;
}

int zk_prover_set_validate(zk_prover *p, int on) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    p->validate = on != 0;
    return ZK_OK;
}

int zk_prover_validation(const zk_prover *p, zk_validation *out) {
    if (!p || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (!p->val_have) ZK_FAIL(ZK_ERR_INVALID_ARG, "no validation has run on this prover");
    *out = p->val_last;
    return ZK_OK;
}

// zk_prover_set_validate(p, 1): Trace::validate before the proof.  Arguments the prove path would refuse are left
// for it to report; a failing trace ends the call with ZK_ERR_TRACE and an empty proof before prove_impl is entered,
// so no hint or snapshot state moves.
static int validate_first(zk_prover *p, const void *d_trace, const uint8_t *const *cols, size_t n, const zk_options *opt,
                          const zk_pub_inputs *pub, size_t *proof_len) {
    if (!p || !p->validate || !proof_len || p->shard_world > 1) return ZK_OK;
    if (check_prove_args(n, p->max_n, p->max_b, opt, pub) != ZK_OK) return ZK_OK;
    zk_validation v;
    const int rc = cols ? zk_validate_columns(p, cols, n, pub, &v) : zk_validate_device(p, d_trace, n, pub, &v);
    if (rc != ZK_OK) *proof_len = 0;
    return rc;
}

int zk_prove_device(zk_prover *p, const void *d_trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                    uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump) {
    if (!d_trace) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_TRY(validate_first(p, d_trace, nullptr, n, opt, pub, proof_len));
    TraceSrc src;
    src.dev = (const fe *)d_trace;
    return prove_impl(p, src, n, opt, pub, proof_out, proof_len, rec, dump);
}

int zk::fixed_prefix(zk_prover *p, size_t n, uint32_t B, const FixedCols &fx) {
    p->fix_prefix_blocks = 0;
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, B, &pl));
    if (!p->fix_ws) ZK_CHECK_HIP(p->arena.alloc(&p->fix_ws, W));
    fe_ws ws[W];
    for (int c = 0; c < W; c++) ws[c] = make_fe_ws(fx.last[c]);
    ZK_TRY(h2d_small(p, p->fix_ws, ws, sizeof ws));
    constexpr int nb = 12 / 4;  // columns 0 .. 11 are preprocessed whatever the program's stack depth
    const size_t Bn = n << pl->log_b;
    if (fixed_fuse_on()) {
        // their LDE inside the row hash of their blocks; the streaming pass extends the zero registers only
        fixed_axpy(p->st, fx, p->fix_ws, n, (size_t)1 << pl->log_b, p->polys, p->lde, 4 * nb, !coeff_src_on());
        FixedHashCols A{};
        for (int c = 0; c < 4 * nb; c++) {
            A.mode[c] = FixedHashCols::FORM;
            A.src[c] = fx.flde + (size_t)c * Bn;
            A.wsi[c] = (uint8_t)c;
        }
        fixed_hash(p->st, A, fx.lagr_lde, p->fix_ws, p->lde, W, pl->log_n, pl->log_b, nb, p->leaves);
    } else {
        fixed_axpy(p->st, fx, p->fix_ws, n, (size_t)1 << pl->log_b, p->polys, p->lde, 0, !coeff_src_on());
        hash_rows_blocks(p->st, p->lde, W, pl->log_n, pl->log_b, 0, nb, p->leaves);
    }
    p->fix_prefix_blocks = nb;
    return ZK_OK;
}

int zk::prove_fixed(zk_prover *p, size_t n, const zk_options *opt, const zk_pub_inputs *pub, const FixedCols *fx,
                    uint8_t *proof_out, size_t *proof_len) {
    TraceSrc src;
    src.dev = p->d_trace;
    src.fixed = fx;
    return prove_impl(p, src, n, opt, pub, proof_out, proof_len, nullptr, nullptr);
}

int zk::prove_single(zk_prover *p, const uint8_t *trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                     uint8_t *proof_out, size_t *proof_len, zk_record *rec) {
    const uint8_t *cols[W];
    TraceSrc src;
    if (trace) {
        for (int c = 0; c < W; c++) cols[c] = trace + (size_t)c * n * sizeof(fe);
        src.cols = cols;
    } else {
        src.dev = p->d_trace;
    }
    return prove_impl(p, src, n, opt, pub, proof_out, proof_len, rec, nullptr);
}

int zk_prove_columns_ex(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_options *opt,
                        const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len, zk_record *rec,
                        const zk_dump *dump) {
    if (!columns) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < W; c++)
        if (!columns[c]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null trace column");
    ZK_TRY(validate_first(p, nullptr, columns, n, opt, pub, proof_len));
    TraceSrc src;
    src.cols = columns;
    return prove_impl(p, src, n, opt, pub, proof_out, proof_len, rec, dump);
}

int zk_prove_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_options *opt,
                     const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len) {
    return zk_prove_columns_ex(p, columns, n, opt, pub, proof_out, proof_len, nullptr, nullptr);
}

int zk_prove(zk_prover *p, const uint8_t *trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
             uint8_t *proof_out, size_t *proof_len) {
    if (!trace) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    const uint8_t *cols[W];
    for (int c = 0; c < W; c++) cols[c] = trace + (size_t)c * n * sizeof(fe);
    return zk_prove_columns(p, cols, n, opt, pub, proof_out, proof_len);
}

// ---------------------------------------------------------------- page-locked host memory for traces
int zk_host_alloc(size_t bytes, void **ptr) {
    if (!ptr || !bytes) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    *ptr = nullptr;
    const hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        *ptr = nullptr;
        ZK_CHECK_HIP(e);
    }
    return ZK_OK;
}

void zk_host_free(void *ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

int zk_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_CHECK_HIP(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
    return ZK_OK;
}

int zk_host_unregister(void *ptr) {
    if (!ptr) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_CHECK_HIP(hipHostUnregister(ptr));
    return ZK_OK;
}

// ---------------------------------------------------------------- plug point 1: trace LDE
int zk_lde_new(zk_prover *p, const uint8_t *trace, size_t width, size_t n, uint32_t blowup, zk_trace_lde **out,
               uint8_t root[32]) {
    if (!p || !trace || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    if (width != (size_t)W) ZK_FAIL(ZK_ERR_INVALID_ARG, "ProcessorAir traces have 28 columns");
    if (n < 16 || (n & (n - 1)) || n > p->max_n || blowup < 8 || (blowup & (blowup - 1)) || blowup > p->max_b)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid trace length or blowup");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    Plan *pl;
    int rc = get_plan(p, n, blowup, &pl);
    if (rc) return rc;
    const uint8_t *cols[W];
    for (int c = 0; c < W; c++) cols[c] = trace + (size_t)c * n * sizeof(fe);
    TraceSrc src;
    src.cols = cols;
    src.hint_ok = false;  // no proof follows to verify a hint
    uint8_t r[32];
    rc = trace_lde_commit(p, pl, src, n, r);
    if (!rc) rc = d2h_flush(p);
    upload_drain(p);  // the caller's trace is no longer read once this returns
    if (rc) return rc;
    if (root) memcpy(root, r, 32);
    *out = new zk_trace_lde{p, n, blowup, W};
    return ZK_OK;
}

int zk_lde_read_frame(zk_trace_lde *h, size_t step, uint8_t *cur, uint8_t *next) {
    if (!h || !cur || !next) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    zk_prover *p = h->p;
    const size_t N = h->n * h->B;
    if (step >= N) ZK_FAIL(ZK_ERR_INVALID_ARG, "lde_step out of range");
    uint64_t idx[2] = {step, (step + h->B) % N};
    ZK_CHECK_HIP(hipMemcpyAsync(p->gather_idx, idx, 16, hipMemcpyHostToDevice, p->st));
    gather_rows(p->st, p->lde, W, ilog2(h->n), ilog2(h->B), p->gather_idx, 2, p->gather_out);
    fe rows[2 * W];
    ZK_CHECK_HIP(hipMemcpyAsync(rows, p->gather_out, sizeof rows, hipMemcpyDeviceToHost, p->st));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    memcpy(cur, rows, W * 16);
    memcpy(next, rows + W, W * 16);
    return ZK_OK;
}

// rows at `positions` of a committed coset-major LDE (ncols columns) + the batch Merkle proof bytes
static int query_committed_rows(zk_prover *p, const fe *base, int ncols, size_t n, uint32_t B, const uint8_t *leaves,
                                const uint8_t *nodes, const uint64_t *positions, size_t k, uint8_t *rows_out,
                                uint8_t *proof_out, size_t *proof_len) {
    if (!positions || !rows_out || !proof_len || k == 0 || k > ZK_MAX_QUERIES)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid query arguments");
    const size_t N = n * B;
    std::vector<uint64_t> pos(positions, positions + k);
    for (uint64_t x : pos)
        if (x >= N) ZK_FAIL(ZK_ERR_INVALID_ARG, "query position out of range");
    {
        // MerkleTree::prove_batch refuses a repeated index (MerkleTreeError::DuplicateLeafIndex): the batch proof
        // holds one path per distinct leaf pair, and a verifier rebuilds the root from distinct positions
        std::vector<uint64_t> sorted(pos);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            ZK_FAIL(ZK_ERR_INVALID_ARG, "duplicate query position");
    }
    ZK_CHECK_HIP(hipMemcpyAsync(p->gather_idx, pos.data(), k * 8, hipMemcpyHostToDevice, p->st));
    gather_rows(p->st, base, ncols, ilog2(n), ilog2(B), p->gather_idx, k, p->gather_out);
    ZK_CHECK_HIP(hipMemcpyAsync(rows_out, p->gather_out, k * ncols * 16, hipMemcpyDeviceToHost, p->st));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    BatchPlan bp;
    plan_batch(N, pos, bp);
    Bytes out;
    out.u8((uint8_t)bp.paths.size());
    for (auto &path : bp.paths) {
        out.u8((uint8_t)path.size());
        for (auto &e : path) {
            uint8_t d[32];
            ZK_CHECK_HIP(hipMemcpy(d, (e.first ? nodes : leaves) + 32 * e.second, 32, hipMemcpyDeviceToHost));
            out.put(d, 32);
        }
    }
    size_t cap = *proof_len;
    *proof_len = out.v.size();
    if (!proof_out || cap < out.v.size()) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "proof buffer too small");
    memcpy(proof_out, out.v.data(), out.v.size());
    return ZK_OK;
}

int zk_lde_query(zk_trace_lde *h, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                 size_t *proof_len) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    zk_prover *p = h->p;
    return query_committed_rows(p, p->lde, W, h->n, h->B, p->leaves, p->nodes, positions, k, rows_out, proof_out,
                                proof_len);
}

void zk_lde_free(zk_trace_lde *h) { delete h; }

// ---------------------------------------------------------------- plug point 2: constraint evaluation
int zk_eval_constraints(zk_trace_lde *h, const zk_pub_inputs *pub, const uint8_t *coeff_t, const uint8_t *coeff_b,
                        uint8_t *out) {
    if (!h || !pub || !coeff_t || !coeff_b || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (pub->lwe_size == 0 || pub->lwe_size > 5) ZK_FAIL(ZK_ERR_INVALID_ARG, "lwe_size must be in [1, 5]");
    zk_prover *p = h->p;
    const size_t n = h->n;
    Plan *pl;
    int rc = get_plan(p, n, h->B, &pl);
    if (rc) return rc;
    AirConsts K;
    memset(&K, 0, sizeof K);
    for (int k = 0; k < NUM_TCONS; k++) K.coeff_t[k] = fe_from_bytes(coeff_t + 16 * k);
    for (int k = 0; k < NUM_ASSERTS; k++) K.coeff_b[k] = fe_from_bytes(coeff_b + 16 * k);
    air_static_consts(pub, n, K);
    ZK_CHECK_HIP(hipMemcpyAsync(p->air_consts, &K, sizeof K, hipMemcpyHostToDevice, p->st));
    const fe *binv = boundary_inverses(p, pl);
    if (!binv) ZK_FAIL(ZK_ERR_OUT_OF_MEMORY, "boundary divisor table");
    ZK_CHECK_HIP(eval_constraints(p->st, 1, p->lde, pl->log_n, eval_map_whole(pl->log_b, 8, true), pl->periodic, binv,
                                  (const AirConsts *)p->air_consts, 0, p->comp, true));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    coset_major_rows_to_host(p, p->comp, 1, n, 8, out);
    return ZK_OK;
}

// ---------------------------------------------------------------- plug point 3: constraint commitment
struct zk_comp_commit {
    zk_prover *p;
    size_t n;
    uint32_t B;
    int ncols;
};

int zk_commit_composition(zk_trace_lde *h, const uint8_t *composition, uint32_t num_cols, zk_comp_commit **out,
                          uint8_t root[32], uint8_t *polys_out) {
    if (!h || !composition || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (num_cols < 1 || num_cols > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "num_cols must be in [1, 8]");
    zk_prover *p = h->p;
    const size_t n = h->n, CE = 8 * n;
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    Plan *pl;
    int rc = get_plan(p, n, h->B, &pl);
    if (rc) return rc;
    // natural CE order (step i = r + 8q) -> coset-major comp[r*n + q], the evaluator's layout
    std::vector<fe> cm(CE);
    const fe *in = reinterpret_cast<const fe *>(composition);
    for (size_t i = 0; i < CE; i++) memcpy(&cm[(i & 7) * n + (i >> 3)], in + i, sizeof(fe));
    ZK_CHECK_HIP(hipMemcpyAsync(p->comp, cm.data(), CE * sizeof(fe), hipMemcpyHostToDevice, p->st));
    uint8_t r[32];
    if ((rc = composition_stage(p, pl, 1, (int)num_cols, p->comp, p->ctmp, p->clde, r))) return rc;
    unsigned degree_flag = 0;
    if ((rc = d2h_small(p, &degree_flag, p->flag, 4)) || (rc = d2h_flush(p))) return rc;  // root and flag
    if (degree_flag) ZK_FAIL(ZK_ERR_DEGREE, "composition polynomial degree exceeds num_cols * trace_len");
    if (polys_out)
        ZK_CHECK_HIP(hipMemcpy(polys_out, p->cpolys, (size_t)num_cols * n * sizeof(fe), hipMemcpyDeviceToHost));
    if (root) memcpy(root, r, 32);
    *out = new zk_comp_commit{p, n, h->B, (int)num_cols};
    return ZK_OK;
}

int zk_comp_query(zk_comp_commit *h, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                  size_t *proof_len) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    zk_prover *p = h->p;
    return query_committed_rows(p, p->clde, h->ncols, h->n, h->B, p->cleaves, p->cnodes, positions, k, rows_out,
                                proof_out, proof_len);
}

void zk_comp_free(zk_comp_commit *h) { delete h; }

// ---------------------------------------------------------------- diagnostics
// Host execution of the lazy dot product (acc288: unreduced 256-bit products, one reduction)
extern "C" void zk_diag_dot_host(const uint8_t *a, const uint8_t *b, size_t count, uint8_t *out) {
    acc288 acc = acc288_zero();
    for (size_t i = 0; i < count; i++) acc288_madd(acc, fe_from_bytes(a + 16 * i), fe_from_bytes(b + 16 * i));
    fe_to_bytes(acc288_reduce(acc), out);
}

// Host execution of the exact device multiply (fe_mul_limbs) -- lets CPU tests check the GPU
// reduction algorithm without a GPU.
extern "C" void zk_diag_mul_limbs_host(const uint8_t *a, const uint8_t *b, uint8_t *out, size_t count) {
    for (size_t i = 0; i < count; i++) fe_to_bytes(fe_mul_limbs(fe_from_bytes(a + 16 * i), fe_from_bytes(b + 16 * i)), out + 16 * i);
}
// Host: the constants the evaluator folds from the coefficients of constraints 12..15 (ct: 4 elements) at trace
// length n: u[4] as the kernel's prologue forms them (air_fold_mds) and the pv[128] table of AirConsts
extern "C" void zk_diag_air_fold_host(const uint8_t *ct, size_t n, uint8_t *u_out, uint8_t *pv_out) {
    fe c[4], pv[128];
    for (int r = 0; r < 4; r++) c[r] = fe_from_bytes(ct + 16 * r);
    for (int k = 0; k < 4; k++) fe_to_bytes(air_fold_mds(c, k), u_out + 16 * k);
    const std::vector<fe> per = periodic_table(n);
    air_fold_periodic(c, per.data(), pv);
    for (int j = 0; j < 128; j++) fe_to_bytes(pv[j], pv_out + 16 * j);
}
// Host: the evaluator's W sets (AirConsts::ws, air_build_ws) of the coefficients ct[20], cb[22] and delta (16 bytes
// each): out = EW_COUNT sets of 64 bytes in EvalWs order
extern "C" void zk_diag_air_ws_host(const uint8_t *ct, const uint8_t *cb, const uint8_t *delta, uint8_t *out) {
    AirConsts K;
    memset(&K, 0, sizeof K);
    for (int k = 0; k < NUM_TCONS; k++) K.coeff_t[k] = fe_from_bytes(ct + 16 * k);
    for (int k = 0; k < NUM_ASSERTS; k++) K.coeff_b[k] = fe_from_bytes(cb + 16 * k);
    K.delta = fe_from_bytes(delta);
    air_build_ws(K);
    memcpy(out, K.ws, sizeof K.ws);
}
extern "C" void zk_diag_blake3_host(const uint8_t *in, size_t len, uint8_t out[32]) { b3::hash_bytes(in, len, out); }

// Host: the upload plan of a host-trace commitment (upload_plan.hpp).  in[13] = have, sparse, nw8, nw32, clk_off,
// fixed_off, snap, snap_mask, hint_ok, no_virtual, lat_sched, detect, switches (bit 0 ZK_SPARSE, 1 ZK_NARROW, 2 ZK_CLOCK,
// 3 ZK_FIXED, 4 ZK_FIXED_FUSE, 5 ZK_VIRTUAL, 6 ZK_COEFF_SRC); n the trace length.
static UploadPlanIn diag_upload_plan_in(const uint32_t *in, size_t n) {
    UploadPlanIn q;
    q.have = in[0], q.sparse = in[1], q.nw8 = in[2], q.nw32 = in[3], q.clk_off = in[4], q.fixed_off = in[5];
    q.snap = in[6], q.snap_mask = in[7], q.hint_ok = in[8], q.no_virtual = in[9], q.lat_sched = in[10], q.detect = in[11];
    q.sparse_on = in[12] & 1u, q.narrow_on = in[12] & 2u, q.clock_on = in[12] & 4u, q.fixed_on = in[12] & 8u;
    q.fixed_fuse_on = in[12] & 16u, q.virtual_on = in[12] & 32u, q.coeff_src_on = in[12] & 64u;
    q.n = n;
    return q;
}
// the plan's coeff_src (the derived columns' coefficients read at their source, not written): 1 or 0
extern "C" int zk_diag_upload_plan_coeff_src(const uint32_t *in, size_t n) {
    return upload_plan(diag_upload_plan_in(in, n)).coeff_src ? 1 : 0;
}
// masks[8] = hint, nw8, nw32, clk, fixm, virt, snap_now, lat; counts[7] = nd, nh, nhv, nn, np, ngroups, fuse_nb;
// cols[4 W] = dense, hin, hnv, nar (W each); width[W]; off[W + 1] (off[W] = pack_bytes); pb[W + 1]; gsz[W].  Returns the
// plan's status.
extern "C" int zk_diag_upload_plan(const uint32_t *in, size_t n, uint32_t *masks, int32_t *counts, int32_t *cols,
                                   int32_t *width, uint64_t *off, int32_t *pb, int32_t *gsz) {
    const UploadPlan u = upload_plan(diag_upload_plan_in(in, n));
    const uint32_t m[8] = {u.hint, u.nw8, u.nw32, u.clk, u.fixm, u.virt, u.snap_now, u.lat};
    const int32_t k[7] = {u.nd, u.nh, u.nhv, u.nn, u.np, u.ngroups, u.fuse_nb};
    memcpy(masks, m, sizeof m);
    memcpy(counts, k, sizeof k);
    for (int i = 0; i < W; i++) {
        cols[i] = i < u.nd ? u.dense[i] : -1;
        cols[W + i] = i < u.nh ? u.hin[i] : -1;
        cols[2 * W + i] = i < u.nhv ? u.hnv[i] : -1;
        cols[3 * W + i] = i < u.nn ? u.nar[i] : -1;
        width[i] = i < u.nn ? u.width[i] : 0;
        off[i] = i < u.nn ? u.off[i] : 0;
        gsz[i] = i < u.ngroups ? u.gsz[i] : 0;
    }
    off[W] = u.pack_bytes;
    for (int i = 0; i <= W; i++) pb[i] = i <= u.np ? u.pb[i] : -1;
    if (u.status != ZK_OK) ZK_FAIL(u.status, "too many upload groups");
    return ZK_OK;
}

// Host: the rounds of the sharded trace split (shard_plan.hpp shard_round_plan) over the columns U[nU] (ascending), G ranks,
// the first `rep` columns replicated.  out[(3 + 2 G) k ..] for round k: first split index, real, inplace, then per rank
// g its column (-1: none) and the column its chunk of an in-place all-gather lands on (-1: a staged round); *rounds.
extern "C" int zk_diag_shard_rounds(const int32_t *U, int nU, int G, int rep, int32_t *out, size_t cap, int32_t *rounds) {
    if (!U || !out || !rounds || nU < 0 || nU > W || rep < 0 || rep > nU || (G != 2 && G != 4 && G != 8))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_shard_rounds: up to 28 columns, 0 <= rep <= nU, G = 2, 4 or 8");
    const ShardRounds r = shard_round_plan(U, nU, G, rep);
    if (cap < (size_t)r.rounds * (3 + 2 * G)) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_shard_rounds: out too small");
    for (int k = 0; k < r.rounds; k++) {
        int32_t *o = out + (size_t)k * (3 + 2 * G);
        o[0] = G * k, o[1] = r.real(k), o[2] = r.inplace(k);
        for (int g = 0; g < G; g++) {
            o[3 + g] = r.column(k, g);
            o[3 + G + g] = r.inplace(k) ? r.first(k) + g : -1;
        }
    }
    *rounds = r.rounds;
    return ZK_OK;
}

// Host: where a Merkle tree of M leaves split over G ranks keeps leaf (is_node 0) or heap node idx[i] (shard_plan.hpp
// TreeGeom::locate): out[3 i ..] = owner rank (-1: the host's top), buffer (1 subtree heap, 2 block buffer), byte offset.
extern "C" int zk_diag_shard_locate(uint64_t M, int G, int is_node, const uint64_t *idx, size_t count, int64_t *out) {
    if (!idx || !out || (G != 2 && G != 4 && G != 8) || M < 8 * (uint64_t)G || (M & (M - 1)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_shard_locate: G = 2, 4 or 8, M a power of two >= 8 G");
    TreeGeom T;
    T.shape(M, G);
    for (size_t i = 0; i < count; i++) {
        if (is_node ? (idx[i] < 1 || idx[i] >= M) : idx[i] >= M)
            ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_shard_locate: leaf index below M, heap node index in 1 .. M - 1");
        const TreeGeom::Loc L = T.locate(is_node, idx[i]);
        out[3 * i] = L.owner, out[3 * i + 1] = L.which, out[3 * i + 2] = (int64_t)L.off;
    }
    return ZK_OK;
}

// GPU elementwise field op: 0 add, 1 sub, 2 mul, 3 inv(a), 4 a^b (b as a 128-bit exponent), 5 lazy add,
// 6 canonical form of a, 7 multiply by b in two-part form, 8 .. 10 the butterflies' addsub2 forms.
// 11 .. 15: a times the constant b through the production constant forms, the constants built here by make_fe_ws /
// make_fe_w2 and uploaded as a table: 11 fe_mul_uniform (the constant of the first element of each 64-element wave),
// 12 fe_mul_wsv, 13 fe_mul_uniform2 (count a multiple of 64), 14 fe_mul_wsv2, 15 fe_mul_w2_2; 16 / 17 the raw final
// reductions ws_fold / ws_fold2 of a + (b mod 2^35) 2^128.  The pairing of the two-output forms: kernels.hip k_field_op.
// 18 .. 20: the lazy sums of W-set products (acc192_madd_uniform, acc288_madd_uniform), the constant as in 11; their
// terms: kernels.hip k_field_op.
extern "C" int zk_diag_field_op(int device, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t count) {
    if (!a || !b || !out || count == 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (op < 0 || op > 20 || count > ((size_t)1 << 30) || (op == 13 && count % 64 != 0))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_field_op: unknown op, or a count the op does not take");
    ZK_CHECK_HIP(hipSetDevice(device));
    std::vector<fe_ws> ws;
    std::vector<fe_w2> w2;
    if ((op >= 11 && op <= 14) || op >= 18) {
        ws.resize(count);
        for (size_t i = 0; i < count; i++) ws[i] = make_fe_ws(fe_from_bytes(b + 16 * i));
    } else if (op == 15) {
        w2.resize(count);
        for (size_t i = 0; i < count; i++) w2[i] = make_fe_w2(fe_from_bytes(b + 16 * i));
    }
    fe *d = nullptr;
    void *tab = nullptr;
    const size_t tab_bytes = ws.size() * sizeof(fe_ws) + w2.size() * sizeof(fe_w2);
    ZK_CHECK_HIP(hipMalloc(&d, 3 * count * sizeof(fe)));
    hipError_t e = tab_bytes ? hipMalloc(&tab, tab_bytes) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(d, a, count * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + count, b, count * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess && tab_bytes)
        e = hipMemcpy(tab, ws.empty() ? (const void *)w2.data() : (const void *)ws.data(), tab_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        diag_field_op(nullptr, op, d, d + count, d + 2 * count, count, ws.empty() ? nullptr : (const fe_ws *)tab,
                      w2.empty() ? nullptr : (const fe_w2 *)tab);
        e = hipMemcpy(out, d + 2 * count, count * 16, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (tab) (void)hipFree(tab);
    ZK_CHECK_HIP(e);
    return ZK_OK;
}

// Host: the constant forms of w as the kernels read them -- out[0, 64) = make_fe_ws(w) (word 4 j + i = 32-bit word j
// of w 2^(32 i) mod p), out[64, 96) = make_fe_w2(w) (w, w 2^64 mod p)
extern "C" void zk_diag_make_ws_host(const uint8_t *w, uint8_t *out) {
    const fe v = fe_from_bytes(w);
    const fe_ws W = make_fe_ws(v);
    const fe_w2 W2 = make_fe_w2(v);
    memcpy(out, W.w, 64);
    fe_to_bytes(W2.w, out + 64);
    fe_to_bytes(W2.w64, out + 80);
}

// GPU BLAKE3 of `count` rows of k field elements (k <= 64)
extern "C" int zk_diag_blake3_rows(int device, const uint8_t *rows, int k, size_t count, uint8_t *out) {
    if (!rows || !out || k <= 0 || k > 64 || count == 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid argument");
    ZK_CHECK_HIP(hipSetDevice(device));
    fe *d = nullptr;
    ZK_CHECK_HIP(hipMalloc(&d, count * k * sizeof(fe) + 32 * count));
    ZK_CHECK_HIP(hipMemcpy(d, rows, count * k * 16, hipMemcpyHostToDevice));
    uint8_t *dout = (uint8_t *)(d + count * k);
    diag_blake3_elems(nullptr, d, k, count, dout);
    hipError_t e = hipMemcpy(out, dout, 32 * count, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    ZK_CHECK_HIP(e);
    return ZK_OK;
}

// GPU leaf hashes of the 28-column rows of a coset-major LDE (lde[(c blowup + r) n + q]) whose columns in `mask` are
// virtual: never read, formed as last[c] * lagr_lde[r n + q] (hash_rows_blocks with VirtCols, as the host-trace
// commitment launches it).  Two launches, blocks [0, split) and [split, 7); leaves in natural order (32 B each).
extern "C" int zk_diag_hash_rows_virtual(int device, const uint8_t *lde, size_t n, uint32_t blowup, uint32_t mask,
                                         const uint8_t *last, const uint8_t *lagr_lde, int split, uint8_t *leaves) {
    if (!lde || !last || !lagr_lde || !leaves || n < 2 || (n & (n - 1)) || blowup < 2 || (blowup & (blowup - 1)) ||
        blowup > 64 || split < 1 || split > W / 4 || (mask >> W))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid argument");
    ZK_CHECK_HIP(hipSetDevice(device));
    const size_t N = n * blowup;
    fe_ws ws[W];
    for (int c = 0; c < W; c++) ws[c] = make_fe_ws(fe_from_bytes(last + 16 * c));
    uint8_t *d = nullptr;
    const size_t o_lagr = (size_t)W * N * sizeof(fe), o_ws = o_lagr + N * sizeof(fe), o_leaves = o_ws + sizeof ws;
    ZK_CHECK_HIP(hipMalloc(&d, o_leaves + 32 * N));
    hipError_t e = hipMemcpy(d, lde, o_lagr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_lagr, lagr_lde, N * sizeof(fe), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_ws, ws, sizeof ws, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const VirtCols v{mask, (const fe_ws *)(d + o_ws), (const fe *)(d + o_lagr)};
        hash_rows_blocks(nullptr, (const fe *)d, W, ilog2(n), ilog2(blowup), 0, split, d + o_leaves, v);
        if (split < W / 4) hash_rows_blocks(nullptr, (const fe *)d, W, ilog2(n), ilog2(blowup), split, W / 4, d + o_leaves, v);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(leaves, d + o_leaves, 32 * N, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    ZK_CHECK_HIP(e);
    return ZK_OK;
}

// GPU NTT of `batch` polys of size n: inverse != 0 -> interpolation (with 1/n), else evaluation
// over offset * <w_n> (offset given as 16 bytes; pass 1 for the plain subgroup)
extern "C" int zk_diag_ntt(int device, const uint8_t *in, size_t n, int batch, int inverse, const uint8_t *offset,
                           uint8_t *out) {
    if (!in || !out || n < 2 || (n & (n - 1)) || batch <= 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid argument");
    zk_prover *p = nullptr;
    int rc = zk_prover_create(device, std::max<size_t>(n, 16), 8, &p);
    if (rc) return rc;
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    NttTables T;
    ZK_CHECK_HIP(make_ntt_tables(p, ilog2(n), &T));
    if (T.log_n > 12) {
        ZK_CHECK_HIP(p->arena.alloc(&T.fwd_pass, n));
        ZK_CHECK_HIP(p->arena.alloc(&T.inv_pass, n));
        make_pass_twiddles(p->st, T);
    }
    PowTable pre;
    fe off = offset ? fe_from_bytes(offset) : fe_one();
    bool use_pre = !inverse && !fe_eq(off, fe_one());
    if (use_pre) ZK_CHECK_HIP(make_pow_table(p, off, n, &pre));
    fe *d_in = nullptr, *d_out = nullptr, *d_tmp = nullptr;
    ZK_CHECK_HIP(p->arena.alloc(&d_in, n * batch));
    ZK_CHECK_HIP(p->arena.alloc(&d_out, n * batch));
    ZK_CHECK_HIP(p->arena.alloc(&d_tmp, n * batch));
    ZK_CHECK_HIP(hipMemcpy(d_in, in, n * batch * 16, hipMemcpyHostToDevice));
    fe inv_n = h_inv(fe_make(n));
    ntt(p->st, T, d_in, n, d_out, n, batch, inverse != 0, use_pre ? &pre : nullptr, inverse ? &inv_n : nullptr, d_tmp);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(out, d_out, n * batch * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// GPU coset LDE as the prover runs it (ntt_lde over the plan's CosetTables): ncols (<= the trace width) columns of n
// coefficients -- or, from_evals != 0, of n evaluations over <w_n>, interpolated first exactly as the prover does
// (ntt with post_scale n^-1: four-step sizes take the pass-1 twiddles with n^-1 folded in) -- extended over the ncos
// cosets r = r0 + j rstride of the blowup * n domain:  out[(c ncos + j) n + k] = P_c(3 w_N^r w_n^k).
extern "C" int zk_diag_lde(int device, const uint8_t *in, size_t n, int ncols, uint32_t blowup, int r0, int rstride,
                           int ncos, int from_evals, uint8_t *out) {
    if (!in || !out || n < 8 || (n & (n - 1)) || ncols <= 0 || ncols > W || blowup < 8 || blowup > 64 ||
        (blowup & (blowup - 1)) || r0 < 0 || rstride < 1 || ncos < 1 ||
        (uint64_t)r0 + (uint64_t)(ncos - 1) * (uint64_t)rstride >= blowup)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_lde: n a power of two >= 8, 1 .. 28 columns, cosets r0 + j rstride < blowup");
    zk_prover *p = nullptr;
    int rc = zk_prover_create(device, std::max<size_t>(n, 16), blowup, &p);
    if (rc) return rc;
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, blowup, &pl));
    ZK_CHECK_HIP(hipMemcpy(p->d_trace, in, (size_t)ncols * n * 16, hipMemcpyHostToDevice));
    const fe *coeffs = p->d_trace;
    if (from_evals) {
        const fe inv_n = h_inv(fe_make(n));
        ntt(p->st, pl->Tn, p->d_trace, n, p->polys, n, ncols, true, nullptr, &inv_n, p->tmp);
        coeffs = p->polys;
    }
    // p->lde holds 28 * blowup * n elements, p->tmp 28 * 8 * n (a launch covers at most 8 cosets)
    ntt_lde(p->st, pl->Tn, pl->ct, coeffs, n, ncols, r0, rstride, ncos, p->lde, (size_t)ncos * n, n, p->tmp);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(out, p->lde, (size_t)ncols * ncos * n * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// ---- the front of the trace commitment: the column classes (sparse, the AIR clock, narrow) and what consumes them, each
// through its production launcher on columns of the caller's choice (tests/test_gpu_trace_classes.py; the reference is
// tests/trace_classes_ref.py).  Like zk_diag_lde: a prover of its own on `device`, the inputs uploaded into its
// buffers, the launcher on its stream, the result read back.
static int diag_class_flags(zk_prover *p) {  // the flag array and the last row, as sparse_begin allocates them; zeroed
    if (!p->sp_nz) {
        ZK_CHECK_HIP(p->arena.alloc(&p->sp_nz, 4 * W));
        ZK_CHECK_HIP(p->arena.alloc(&p->sp_last, W));
    }
    ZK_CHECK_HIP(hipMemsetAsync(p->sp_nz, 0, 4 * W * sizeof(unsigned), p->st));
    ZK_CHECK_HIP(hipMemsetAsync(p->sp_last, 0, W * sizeof(fe), p->st));
    return ZK_OK;
}

// Column detection.  ncols columns of n elements are placed as trace columns c0 .. c0 + ncols - 1 (the others zero), the
// flags zeroed.  how = 0: sparse_detect_rows with wstride = 28 and the clock check on (idoff = 3 * 28), in `parts`
// launches over the row ranges [k n / parts, (k + 1) n / parts) into the same flags (a sharded rank's share each; parts
// in {1, 2, 4, 8}, n / parts a multiple of 4096 when parts > 1); n >= 16.  how = 1: the interpolation with
// SparseCols{fused, col0 = c0, wstride = 28} (four-step sizes: n >= 2^13), its coefficients to polys_out (ncols n).
// flags_out[4 * 28]: [c] a row before the last is nonzero, [28 + c] a value >= 2^8, [56 + c] a value >= 2^32, [84]
// column 0 is not the clock (how = 0 only); last_out[28]: the `last` array (how = 0 only writes it).
extern "C" int zk_diag_detect(int device, const uint8_t *cols, size_t n, int ncols, int c0, int how, int parts,
                              uint32_t *flags_out, uint8_t *last_out, uint8_t *polys_out) {
    const bool ok = cols && flags_out && last_out && n >= 16 && !(n & (n - 1)) && n <= ((size_t)1 << 22) && ncols >= 1 &&
                    c0 >= 0 && c0 + ncols <= W && (how == 0 || (how == 1 && n >= 8192 && polys_out && parts == 1)) &&
                    (parts == 1 || ((parts == 2 || parts == 4 || parts == 8) && n / parts >= 4096 && n / parts % 4096 == 0));
    if (!ok)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_detect: n a power of two in [16, 2^22] (how = 1: from 2^13), columns c0 .. c0 + "
                                    "ncols - 1 within 28, parts 1, 2, 4 or 8 ranges of a multiple of 4096 rows");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, 8, &pl));
    ZK_CHECK_HIP(hipMemsetAsync(p->d_trace, 0, (size_t)W * n * sizeof(fe), p->st));
    ZK_TRY(diag_class_flags(p));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(p->d_trace + (size_t)c0 * n, cols, (size_t)ncols * n * 16, hipMemcpyHostToDevice));
    SparseCols sp{p->sp_nz, p->sp_last, pl->lagr, pl->lagr_lde, c0};
    sp.wstride = W;
    if (how == 0) {
        sp.id_poly = p->polys;  // (never read by the detection: non-null turns the clock check on)
        sp.idoff = 3 * W;
        for (int k = 0; k < parts; k++)
            sparse_detect_rows(p->st, p->d_trace, n, c0, ncols, sp, (size_t)k * (n / parts), (size_t)(k + 1) * (n / parts));
    } else {
        sp.fused = true;
        const fe inv_n = h_inv(fe_make(n));
        ntt(p->st, pl->Tn, p->d_trace + (size_t)c0 * n, n, p->polys + (size_t)c0 * n, n, ncols, true, nullptr, &inv_n,
            p->tmp, &sp);
    }
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(flags_out, p->sp_nz, 4 * W * sizeof(unsigned), hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(last_out, p->sp_last, W * 16, hipMemcpyDeviceToHost));
    if (how == 1)
        ZK_CHECK_HIP(hipMemcpy(polys_out, p->polys + (size_t)c0 * n, (size_t)ncols * n * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// The commitment to a device-resident trace of 28 arbitrary columns (no AIR validity needed): copied into the prover's
// trace buffer and committed through trace_lde_commit with a device TraceSrc (commit_device: detection, interpolation
// and coset LDE with the sparse and clock columns skipped in pass 1 and filled in pass 2, row hash, Merkle tree).
// flags_out[4 * 28] as zk_diag_detect's (this path takes no width flags: they stay 0; all 0 with ZK_SPARSE=0);
// polys_out: 28 n coefficients; lde_out: 28 blowup n, coset-major
// (lde[(c blowup + r) n + q]); root_out: the trace root.  n >= 2^13, blowup in {8, 16, 32, 64}.
extern "C" int zk_diag_trace_commit(int device, const uint8_t *trace, size_t n, uint32_t blowup, uint32_t *flags_out,
                                    uint8_t *polys_out, uint8_t *lde_out, uint8_t *root_out) {
    if (!trace || !flags_out || !polys_out || !lde_out || !root_out || n < 8192 || (n & (n - 1)) ||
        n > ((size_t)1 << 22) || blowup < 8 || blowup > 64 || (blowup & (blowup - 1)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_trace_commit: n a power of two in [2^13, 2^22], blowup 8, 16, 32 or 64");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, blowup, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    IoScope io_scope(p);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, blowup, &pl));
    ZK_CHECK_HIP(hipMemcpy(p->d_trace, trace, (size_t)W * n * 16, hipMemcpyHostToDevice));
    TraceSrc src;
    src.dev = p->d_trace;
    uint8_t root[32];
    ZK_TRY(trace_lde_commit(p, pl, src, n, root));
    ZK_TRY(d2h_flush(p));  // the root
    memset(flags_out, 0, 4 * W * sizeof(unsigned));
    if (p->tc.sp_used) ZK_CHECK_HIP(hipMemcpy(flags_out, p->sp_nz, 4 * W * sizeof(unsigned), hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(polys_out, p->polys, (size_t)W * n * 16, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(lde_out, p->lde, (size_t)W * blowup * n * 16, hipMemcpyDeviceToHost));
    memcpy(root_out, root, 32);
    return ZK_OK;
}

// The fills a host trace's hinted columns get, by the calls HostTraceCommit::fill_sparse and derive_clock make: for
// each run of consecutive columns in sparse_mask, ntt and ntt_lde with SparseCols{all, col0 = run start} (k_sparse_fill);
// with `clock`, column 0 by axpy_fill from id_poly and lagr, and from id_lde and lagr_lde, d = last[0] - (n - 1).
// last[28]: the last rows.  Only the named columns are read back, in ascending order: polys_out n, lde_out blowup n
// (coset-major) elements each.
extern "C" int zk_diag_column_fills(int device, const uint8_t *last, uint32_t sparse_mask, int clock, size_t n,
                                    uint32_t blowup, uint8_t *polys_out, uint8_t *lde_out) {
    if (!last || !polys_out || !lde_out || n < 8192 || (n & (n - 1)) || n > ((size_t)1 << 22) || blowup < 8 ||
        blowup > 64 || (blowup & (blowup - 1)) || (sparse_mask >> W) || (clock && (sparse_mask & 1u)) ||
        (!clock && !sparse_mask))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_column_fills: n a power of two in [2^13, 2^22], blowup 8, 16, 32 or 64, a mask "
                                    "of the 28 columns, column 0 sparse or the clock but not both");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, blowup, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    IoScope io_scope(p);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, blowup, &pl));
    SparseCols spc{};
    const SparseCols *sp = nullptr;
    ZK_TRY(sparse_begin(p, pl, &spc, &sp));
    if (!sp) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_column_fills: the sparse class is switched off (ZK_SPARSE=0)");
    const size_t B = blowup;
    fe lastv[W];
    int named[W], nn = 0, hin[W], nh = 0;
    for (int c = 0; c < W; c++) {
        lastv[c] = fe_from_bytes(last + 16 * c);
        if ((sparse_mask >> c) & 1u) hin[nh++] = c;
        if (((sparse_mask >> c) & 1u) || (clock && c == 0)) named[nn++] = c;
    }
    ZK_TRY(h2d_small(p, p->sp_last, lastv, sizeof lastv));
    const fe inv_n = h_inv(fe_make(n));
    ZK_TRY(for_runs(hin, nh, [&](int c0, int nc) {
        SparseCols g = spc;
        g.col0 = c0, g.fused = false, g.all = true;
        const size_t o = (size_t)c0 * n;
        ntt(p->st, pl->Tn, p->d_trace + o, n, p->polys + o, n, nc, true, nullptr, &inv_n, p->tmp, &g);
        ntt_lde(p->st, pl->Tn, pl->ct, p->polys + o, n, nc, 0, 1, (int)B, p->lde + o * B, B * n, n, p->tmp, &g);
        return ZK_OK;
    }));
    if (clock) {
        ZK_TRY(clock_tables(p, pl));
        const fe_ws d = make_fe_ws(fe_sub(lastv[0], fe_make(n - 1)));
        axpy_fill(p->st, pl->id_poly, pl->lagr, d, n, p->polys);
        axpy_fill(p->st, pl->id_lde, pl->lagr_lde, d, B * n, p->lde);
    }
    ZK_TRY(d2h_flush(p));
    for (int k = 0; k < nn; k++) {
        const size_t c = (size_t)named[k];
        ZK_CHECK_HIP(hipMemcpy(polys_out + (size_t)k * n * 16, p->polys + c * n, n * 16, hipMemcpyDeviceToHost));
        ZK_CHECK_HIP(hipMemcpy(lde_out + (size_t)k * B * n * 16, p->lde + c * B * n, B * n * 16, hipMemcpyDeviceToHost));
    }
    return ZK_OK;
}

// expand_narrow on a packed buffer of packed_len bytes: `count` columns, column col[k]'s rows as width[k]-byte integers
// (1 or 4) at packed + off[k] (off a multiple of 16, off[k] + width[k] n <= packed_len), its last row last[k].
// out: the count columns of n elements, in col[] order.
extern "C" int zk_diag_expand_narrow(int device, const uint8_t *packed, size_t packed_len, int count, const int32_t *col,
                                     const int32_t *width, const uint64_t *off, const uint8_t *last, size_t n,
                                     uint8_t *out) {
    bool ok = packed && col && width && off && last && out && count >= 1 && count <= W && n >= 16 && !(n & (n - 1)) &&
              n <= ((size_t)1 << 22);
    uint32_t seen = 0;
    for (int k = 0; ok && k < count; k++) {
        ok = col[k] >= 0 && col[k] < W && !((seen >> col[k]) & 1u) && (width[k] == 1 || width[k] == 4) &&
             off[k] % 16 == 0 && off[k] <= packed_len && (size_t)width[k] * n <= packed_len - off[k];
        if (ok) seen |= 1u << col[k];
    }
    if (!ok)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_expand_narrow: n a power of two in [16, 2^22], 1 .. 28 distinct columns of "
                                    "width 1 or 4 at 16-byte offsets, each with n rows inside the packed buffer");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    uint8_t *d = nullptr;
    ZK_CHECK_HIP(p->arena.alloc(&d, packed_len));
    ZK_CHECK_HIP(hipMemcpy(d, packed, packed_len, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemsetAsync(p->d_trace, 0, (size_t)W * n * sizeof(fe), p->st));  // (p->st does not wait for stream 0)
    NarrowCols nc{};
    nc.count = count;
    for (int k = 0; k < count; k++) {
        nc.col[k] = col[k];
        nc.width[k] = width[k];
        nc.off[k] = (size_t)off[k];
        nc.last[k] = fe_from_bytes(last + 16 * k);
    }
    expand_narrow(p->st, d, nc, n, p->d_trace);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    for (int k = 0; k < count; k++)
        ZK_CHECK_HIP(hipMemcpy(out + (size_t)k * n * 16, p->d_trace + (size_t)col[k] * n, n * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// The host checks of a host column's rows [r0, r1) (no GPU): op 0 pack_rows (width 1 or 4, into dst), 1 zero_rows,
// 2 clock_rows, 3 same_rows against aux (width 1, 4 or 16).  Returns the check's verdict, 0 or 1.
extern "C" int zk_diag_host_rows(int op, const uint8_t *col, const uint8_t *aux, size_t r0, size_t r1, int width,
                                 uint8_t *dst) {
    const bool ok = col && r0 <= r1 && op >= 0 && op <= 3 && (op != 0 || (dst && (width == 1 || width == 4))) &&
                    (op != 3 || (aux && (width == 1 || width == 4 || width == 16)));
    if (!ok) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_host_rows: op 0 .. 3, r0 <= r1, pack: dst and width 1 or 4, same: aux and width 1, 4 or 16");
    switch (op) {
    case 0: return pack_rows(col, r0, r1, width, dst);
    case 1: return zero_rows(col, r0, r1);
    case 2: return clock_rows(col, r0, r1);
    default: return same_rows(col, aux, r0, r1, width);
    }
}

// row_tasks on the process pool (no GPU): the closure records its (first, end) pair; once the latch opens the pairs go to
// ranges_out (2 per task, in the order the tasks finished), their number to *count_out.
extern "C" int zk_diag_row_tasks(size_t r0, size_t r1, size_t R, uint64_t *ranges_out, size_t cap, size_t *count_out) {
    if (!ranges_out || !count_out || R == 0 || (r1 > r0 && (r1 - r0 + R - 1) / R > ((size_t)1 << 20)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_row_tasks: R >= 1, at most 2^20 tasks");
    std::mutex mu;
    std::vector<uint64_t> got;
    Latch done;
    row_tasks(done, 0, r0, r1, R, [&mu, &got](int, size_t a, size_t b) {
        std::lock_guard<std::mutex> lk(mu);
        got.push_back(a);
        got.push_back(b);
    });
    done.wait();
    *count_out = got.size() / 2;
    if (got.size() / 2 > cap) ZK_FAIL(ZK_ERR_BUFFER_TOO_SMALL, "zk_diag_row_tasks: ranges_out too small");
    if (!got.empty()) memcpy(ranges_out, got.data(), got.size() * sizeof(uint64_t));
    return ZK_OK;
}

// ---- the back half of a proof, each stage through its production launcher on inputs of the caller's choice
// (tests/test_gpu_back_half.py; the reference is tests/back_half_ref.py).  Like zk_diag_lde: a prover of its own on
// `device`, the inputs uploaded into its buffers, the launcher on its stream, the result read back.
static bool diag_read_fe(const uint8_t *b, int ext, fe2 *out) {
    out->a = fe_from_bytes(b);
    out->b = ext == 2 ? fe_from_bytes(b + 16) : fe_zero();
    return fe_canonical(out->a) && fe_canonical(out->b);
}
static int diag_back_half_args(const char *who, const void *tpolys, const void *cpolys, int ccols, size_t n, int ext,
                               const uint8_t *z, const uint8_t *zg, const void *out, fe2 *zv, fe2 *zgv) {
    const bool ok = tpolys && cpolys && z && zg && out && n >= 16 && !(n & (n - 1)) && n <= ((size_t)1 << 22) &&
                    (ext == 1 ? ccols >= 1 && ccols <= 8 : ext == 2 && ccols >= 2 && ccols <= 16 && ccols % 2 == 0);
    if (!ok || !diag_read_fe(z, ext, zv) || !diag_read_fe(zg, ext, zgv))
        ZK_FAIL(ZK_ERR_INVALID_ARG, std::string(who) + ": n a power of two in [16, 2^22]; ext 1 with 1 .. 8 composition "
                                    "columns or ext 2 with 2, 4 .. 16 base columns; z and zg canonical");
    return ZK_OK;
}
static int diag_back_half_upload(zk_prover *p, const uint8_t *tpolys, const uint8_t *cpolys, int ccols, size_t n, int ext) {
    if (ext == 2) ZK_TRY(ensure_ext(p));
    ZK_CHECK_HIP(hipMemcpy(p->polys, tpolys, (size_t)W * n * 16, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemcpy(p->cpolys, cpolys, (size_t)ccols * n * 16, hipMemcpyHostToDevice));
    return ZK_OK;
}

// The OOD frame of 28 trace polynomials and ccols composition polynomials (n coefficients each, column-major; over E,
// ext = 2, ccols counts the base columns) at the points z and zg, given independently (16 bytes each, 32 over E):
// ood_eval with the (rank, G) share of the coefficient range.  out: (56 + ccols) elements
// [T(z)]_28 ++ [T(zg)]_28 ++ [H(z)]_ccols; over E the a components of all, then the b components.
extern "C" int zk_diag_ood(int device, const uint8_t *tpolys, const uint8_t *cpolys, int ccols, size_t n, int ext,
                           const uint8_t *z, const uint8_t *zg, int rank, int G, uint8_t *out) {
    fe2 zv, zgv;
    ZK_TRY(diag_back_half_args("zk_diag_ood", tpolys, cpolys, ccols, n, ext, z, zg, out, &zv, &zgv));
    if (G < 1 || G > 64 || rank < 0 || rank >= G) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_ood: 0 <= rank < G <= 64");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    ZK_TRY(diag_back_half_upload(p, tpolys, cpolys, ccols, n, ext));
    const Planes b = planes(p, ext);
    with_kx(ext, [&](auto kx) {
        typedef Chal<decltype(kx)::value> X;
        ood_eval(p->st, coeff_plain(p->polys, n), W, p->cpolys, ccols, ilog2(n), X::make(zv), X::make(zgv), b.ood_tab,
                 b.partials, p->ood, rank, G);
        return 0;
    });
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(out, p->ood, (size_t)ext * (2 * W + ccols) * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// The DEEP polynomial's coefficients through deep_poly: alpha_t (28) weigh the trace polynomials,
// alpha_c the composition columns (ccols of them; over E ccols / 2 E columns H_j = P_2j + X P_2j+1, and every
// coefficient and point is 32 bytes).  out: n coefficients; over E the a plane, then the b plane.  z = 0 or zg = 0 is
// refused: the kernels scale by powers of their inverses.
static int diag_deep(int device, const uint8_t *tpolys, const uint8_t *cpolys, int ccols, size_t n, int ext,
                     const uint8_t *z, const uint8_t *zg, const uint8_t *alpha_t, const uint8_t *alpha_c, int parts,
                     uint8_t *out) {
    fe2 zv, zgv;
    ZK_TRY(diag_back_half_args("zk_diag_deep", tpolys, cpolys, ccols, n, ext, z, zg, out, &zv, &zgv));
    if (!alpha_t || !alpha_c) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_deep: null argument");
    if ((fe_is_zero(zv.a) && fe_is_zero(zv.b)) || (fe_is_zero(zgv.a) && fe_is_zero(zgv.b)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_deep: z and zg must be non-zero (their inverses are taken)");
    const int C = ccols / ext, log_n = ilog2(n);
    fe2 at[W], ac[8];
    for (int c = 0; c < W + C; c++)
        if (!diag_read_fe((c < W ? alpha_t + 16 * ext * c : alpha_c + 16 * ext * (c - W)), ext, c < W ? &at[c] : &ac[c - W]))
            ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_deep: non-canonical coefficient");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    ZK_TRY(diag_back_half_upload(p, tpolys, cpolys, ccols, n, ext));
    const Planes b = planes(p, ext);
    return with_kx(ext, [&](auto kx) -> int {
        constexpr int KX = decltype(kx)::value;
        typedef Chal<KX> X;
        const typename X::T z = X::make(zv), zg = X::make(zgv);
        DeepConsts<KX> D;
        memset(&D, 0, sizeof D);
        for (int c = 0; c < W; c++) D.alpha_t[c] = X::make(at[c]);
        for (int c = 0; c < C; c++) D.alpha_c[c] = X::make(ac[c]);
        D.z = z, D.zg = zg;
        ZK_CHECK_HIP(hipMemcpy(b.deep_consts, &D, sizeof D, hipMemcpyHostToDevice));
        const fe *Dk = nullptr;
        const CoeffSrc TS = coeff_plain(p->polys, n);
        if (parts == 1) {
            Dk = deep_poly(p->st, TS, p->cpolys, C, log_n, b.deep_consts, z, zg, b.dscratch);
        } else {
            // The ranks of a sharded proof on one device, in rank order: every range's begin, the later ranges' totals
            // summed here as the all-gather and k_sh_suffix_carry do, every range's end.  Each rank has a scratch of
            // its own; here the ranges share one, so a range's block carries (begin leaves them at the head of the
            // block-sum area, which the next range's begin overwrites) are kept in p->comp and put back before its end.
            const DeepScratch S(b.dscratch, n, KX);
            const size_t kn = n / parts, nc = 2 * KX, ncarry = nc * (kn / ZK_DEEP_BLOCK);
            std::vector<fe> tot((size_t)parts * nc);
            for (int g = 0; g < parts; g++) {
                const fe *t = deep_range_begin(p->st, TS, p->cpolys, C, log_n, b.deep_consts, z, zg, b.dscratch, g * kn, kn);
                ZK_CHECK_HIP(hipMemcpyAsync(p->comp + g * ncarry, S.bs, ncarry * sizeof(fe), hipMemcpyDeviceToDevice, p->st));
                ZK_CHECK_HIP(hipMemcpyAsync(&tot[g * nc], t, nc * sizeof(fe), hipMemcpyDeviceToHost, p->st));
            }
            ZK_CHECK_HIP(hipStreamSynchronize(p->st));
            std::vector<fe> later((size_t)parts * nc, fe_zero());
            for (int g = parts - 2; g >= 0; g--)
                for (size_t c = 0; c < nc; c++) later[g * nc + c] = fe_add(later[(g + 1) * nc + c], tot[(g + 1) * nc + c]);
            ZK_CHECK_HIP(hipMemcpy(p->ood, later.data(), later.size() * sizeof(fe), hipMemcpyHostToDevice));
            for (int g = 0; g < parts; g++) {
                ZK_CHECK_HIP(hipMemcpyAsync(S.bs, p->comp + g * ncarry, ncarry * sizeof(fe), hipMemcpyDeviceToDevice, p->st));
                Dk = deep_range_end(p->st, log_n, z, zg, b.dscratch, g * kn, kn, p->ood + g * nc);
            }
        }
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        ZK_CHECK_HIP(hipMemcpy(out, Dk, (size_t)KX * n * 16, hipMemcpyDeviceToHost));
        return ZK_OK;
    });
}
extern "C" int zk_diag_deep(int device, const uint8_t *tpolys, const uint8_t *cpolys, int ccols, size_t n, int ext,
                            const uint8_t *z, const uint8_t *zg, const uint8_t *alpha_t, const uint8_t *alpha_c,
                            uint8_t *out) {
    return diag_deep(device, tpolys, cpolys, ccols, n, ext, z, zg, alpha_t, alpha_c, 1, out);
}
// zk_diag_deep by coefficient ranges, as the ranks of a sharded proof compute it: `parts` ranges of n / parts
// coefficients (a whole number of ZK_DEEP_RANGE_QUANTUM each), deep_range_begin / deep_range_end per range.  The same
// output.
extern "C" int zk_diag_deep_parts(int device, const uint8_t *tpolys, const uint8_t *cpolys, int ccols, size_t n, int ext,
                                  const uint8_t *z, const uint8_t *zg, const uint8_t *alpha_t, const uint8_t *alpha_c,
                                  int parts, uint8_t *out) {
    if (parts < 2 || parts > 8 || (parts & (parts - 1)) || n < (size_t)parts * ZK_DEEP_RANGE_QUANTUM)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_deep_parts: 2, 4 or 8 ranges of at least 2048 coefficients");
    return diag_deep(device, tpolys, cpolys, ccols, n, ext, z, zg, alpha_t, alpha_c, parts, out);
}

// ---- the composition stage (S4) on inputs of the caller's choice (tests/test_gpu_composition.py; the reference is
// tests/back_half_ref.py).  comp: ext planes of 8 cosets x n values in the evaluator's coset-major layout,
// comp[(8 j + r) n + q] = plane j at 3 w_8n^r w_n^q.  tpolys (optional): 28 planes of n trace coefficients, with
// coeff_b (ext x 22) and bnd1 (ext values) the assertion terms' constants of each plane; the second divisor point is
// g^(n-2), as draw_air_consts sets it.  Every value canonical.
static int diag_comp_args(const char *who, const uint8_t *comp, size_t n, int ext, int ncols, const uint8_t *tpolys,
                          const uint8_t *coeff_b, const uint8_t *bnd1, const void *polys_out, const void *flag_out,
                          AirConsts *K) {
    bool ok = comp && polys_out && flag_out && n >= 16 && !(n & (n - 1)) && n <= ((size_t)1 << 22) &&
              (ext == 1 || ext == 2) && ncols >= 1 && ncols <= 8 && (!tpolys || (coeff_b && bnd1));
    memset(K, 0, 2 * sizeof K[0]);
    for (size_t i = 0; ok && i < (size_t)ext * 8 * n; i++) ok = fe_canonical(fe_from_bytes(comp + 16 * i));
    for (size_t i = 0; ok && tpolys && i < (size_t)W * n; i++) ok = fe_canonical(fe_from_bytes(tpolys + 16 * i));
    for (int j = 0; ok && tpolys && j < ext; j++) {
        for (int k = 0; k < NUM_ASSERTS; k++) {
            K[j].coeff_b[k] = fe_from_bytes(coeff_b + 16 * (NUM_ASSERTS * j + k));
            ok = ok && fe_canonical(K[j].coeff_b[k]);
        }
        K[j].bnd1 = fe_from_bytes(bnd1 + 16 * j);
        ok = ok && fe_canonical(K[j].bnd1);
    }
    if (!ok)
        ZK_FAIL(ZK_ERR_INVALID_ARG, std::string(who) + ": n a power of two in [16, 2^22], ext 1 or 2, 1 .. 8 columns, "
                                    "canonical values, coeff_b and bnd1 with tpolys");
    for (int j = 0; j < ext; j++) K[j].g_last2 = h_pow(h_root_of_unity(ilog2(n)), n - 2);
    return ZK_OK;
}

// composition_stage as SingleProof::composition calls it, with the all-PLAIN coefficient table: the per-coset inverse
// NTTs of nce cosets (7: coset 7 of comp is not read, the cross step derives it), comp_cross_mapped per plane,
// boundary_poly_add per plane when tpolys is given, lde_commit over `blowup`.  polys_out: the ext ncols column
// polynomials (base column (c, j) at (c ext + j) n); root_out: the constraint root; *flag_out: the degree flag as the
// kernels left it (0 or 1) -- a set flag is the caller's to judge, not an error here.
extern "C" int zk_diag_composition(int device, const uint8_t *comp, size_t n, uint32_t blowup, int ext, int ncols,
                                   int nce, const uint8_t *tpolys, const uint8_t *coeff_b, const uint8_t *bnd1,
                                   uint8_t *polys_out, uint8_t *root_out, uint32_t *flag_out) {
    AirConsts K[2];
    ZK_TRY(diag_comp_args("zk_diag_composition", comp, n, ext, ncols, tpolys, coeff_b, bnd1, polys_out, flag_out, K));
    if (!root_out || (nce != 7 && nce != 8) || (nce == 7 && ncols > 7) || blowup < 8 || blowup > 64 ||
        (blowup & (blowup - 1)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_composition: nce 8, or 7 with at most 7 columns; blowup a power of two in [8, 64]");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, blowup, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    IoScope io_scope(p);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, blowup, &pl));
    if (ext == 2) ZK_TRY(ensure_ext(p));
    const Planes b = planes(p, ext);
    ZK_CHECK_HIP(hipMemcpy(b.comp, comp, (size_t)ext * 8 * n * 16, hipMemcpyHostToDevice));
    if (tpolys) ZK_CHECK_HIP(hipMemcpy(p->polys, tpolys, (size_t)W * n * 16, hipMemcpyHostToDevice));
    uint8_t root[32];
    unsigned degree_flag = 0;
    ZK_TRY(composition_stage(p, pl, ext, ncols, b.comp, b.ctmp, b.clde, root, tpolys ? K : nullptr, nce));
    ZK_TRY(d2h_small(p, &degree_flag, p->flag, 4));
    ZK_TRY(d2h_flush(p));  // root and flag
    ZK_CHECK_HIP(hipMemcpy(polys_out, p->cpolys, (size_t)ext * ncols * n * 16, hipMemcpyDeviceToHost));
    memcpy(root_out, root, 32);
    *flag_out = degree_flag;
    return ZK_OK;
}

// The cross step and the assertion quotient by coefficient ranges, as the ranks of a sharded proof compute them
// (ShardedProof::cross_step, boundary_begin, boundary_quotient), on one device in rank order: `parts` ranges of
// kg = n / parts coefficients (a whole number of ZK_DEEP_RANGE_QUANTUM each).  It takes comp, as zk_diag_composition
// does, and runs the per-coset inverse NTTs once for all ranges (the call composition_stage makes for nce = 8): a
// rank's share of their output is what the all-to-all hands it, and the ranges never transform again.  Per range g and
// plane: comp_cross_mapped with k0 = g kg, kcount = kg, pstride = ext kg, no derived coset and the sources offset to
// the range, into the range's slices [(c ext + plane) kg]; then per plane boundary_range_begin for every range, the
// later ranges' sums added here as the all-gather and k_sh_suffix_carry do, boundary_range_end into the range's slice
// of column 0.  The ranges share one division scratch, so each range's block carries are kept aside between its begin
// and its end (as in zk_diag_deep_parts).  polys_out: the slices assembled in zk_diag_composition's layout;
// *flag_out: the degree flag.  No LDE, no commitment.
extern "C" int zk_diag_composition_parts(int device, const uint8_t *comp, size_t n, int ext, int ncols, int parts,
                                         const uint8_t *tpolys, const uint8_t *coeff_b, const uint8_t *bnd1,
                                         uint8_t *polys_out, uint32_t *flag_out) {
    AirConsts K[2];
    ZK_TRY(diag_comp_args("zk_diag_composition_parts", comp, n, ext, ncols, tpolys, coeff_b, bnd1, polys_out, flag_out, K));
    if (parts < 2 || parts > 8 || (parts & (parts - 1)) || n < (size_t)parts * ZK_DEEP_RANGE_QUANTUM)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_composition_parts: 2, 4 or 8 ranges of a multiple of 2048 coefficients");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, 8, &pl));
    if (ext == 2) ZK_TRY(ensure_ext(p));
    const Planes b = planes(p, ext);
    const int log_n = pl->log_n;
    const size_t kg = n / parts, slice = (size_t)ncols * ext * kg;
    ZK_CHECK_HIP(hipMemcpy(b.comp, comp, (size_t)ext * 8 * n * 16, hipMemcpyHostToDevice));
    if (tpolys) ZK_CHECK_HIP(hipMemcpy(p->polys, tpolys, (size_t)W * n * 16, hipMemcpyHostToDevice));
    ntt(p->st, pl->Tn, b.comp, n, b.ctmp, n, 8 * ext, true, nullptr, nullptr, p->tmp);
    ZK_CHECK_HIP(hipMemsetAsync(p->flag, 0, 4, p->st));
    fe *out = b.comp;  // the ranges' slices, range after range (the transform has consumed the values)
    const fe scale = h_inv(fe_make(8 * n)), w8inv = h_inv(h_root_of_unity(3)), inv3n = h_inv(h_pow(fe_make(3), n));
    for (int g = 0; g < parts; g++)
        for (int pln = 0; pln < ext; pln++) {
            CrossMap cm;
            for (int r = 0; r < 8; r++) cm.c[r] = b.ctmp + (size_t)(8 * pln + r) * n + g * kg;
            cm.k0 = g * kg;
            cm.kcount = kg;
            cm.pstride = (size_t)ext * kg;
            comp_cross_mapped(p->st, cm, pl->Tce, pl->inv3, scale, w8inv, inv3n, ncols, out + g * slice + pln * kg, p->flag);
        }
    const DeepScratch S(p->dscratch, n, 1);
    const size_t ncarry = 2 * (kg / ZK_DEEP_BLOCK);
    for (int pln = 0; tpolys && pln < ext; pln++) {
        std::vector<fe> tot((size_t)parts * 2);
        for (int g = 0; g < parts; g++) {
            const fe *t = boundary_range_begin(p->st, coeff_plain(p->polys, n), nullptr, log_n, K[pln], K[0].g_last2,
                                               p->dscratch, g * kg, kg);
            ZK_CHECK_HIP(hipMemcpyAsync(p->clde + g * ncarry, S.bs, ncarry * sizeof(fe), hipMemcpyDeviceToDevice, p->st));
            ZK_CHECK_HIP(hipMemcpyAsync(&tot[g * 2], t, 2 * sizeof(fe), hipMemcpyDeviceToHost, p->st));
        }
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        std::vector<fe> later((size_t)parts * 2, fe_zero());
        for (int g = parts - 2; g >= 0; g--)
            for (int c = 0; c < 2; c++) later[g * 2 + c] = fe_add(later[(g + 1) * 2 + c], tot[(g + 1) * 2 + c]);
        fe *ext_sums = p->ood + (size_t)pln * parts * 2;
        ZK_CHECK_HIP(hipMemcpy(ext_sums, later.data(), later.size() * sizeof(fe), hipMemcpyHostToDevice));
        for (int g = 0; g < parts; g++) {
            ZK_CHECK_HIP(hipMemcpyAsync(S.bs, p->clde + g * ncarry, ncarry * sizeof(fe), hipMemcpyDeviceToDevice, p->st));
            boundary_range_end(p->st, log_n, K[0].g_last2, p->dscratch, g * kg, kg, ext_sums + g * 2,
                               out + g * slice + pln * kg - g * kg, p->flag);
        }
    }
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    std::vector<fe> h((size_t)parts * slice);
    ZK_CHECK_HIP(hipMemcpy(h.data(), out, h.size() * sizeof(fe), hipMemcpyDeviceToHost));
    for (int g = 0; g < parts; g++)
        for (int c = 0; c < ncols * ext; c++)
            memcpy(polys_out + 16 * ((size_t)c * n + g * kg), &h[g * slice + (size_t)c * kg], kg * sizeof(fe));
    ZK_CHECK_HIP(hipMemcpy(flag_out, p->flag, 4, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// The three consumers of the trace coefficients through a CoeffSrc (tests/test_coeff_sources.py): tplanes = 29 planes of
// n coefficients, plane c < 28 column c's (mode PLAIN: the column; BASE: its base; ZERO: not read) and plane 28 standing
// for e_(n-1) (any polynomial: the consumers are linear in it); modes[28]; w[28] the columns' scalars (canonical).
// ood_eval + ood_fold_sources -> ood_out as zk_diag_ood's; deep_poly (with deep_source_weight) -> deep_out as
// zk_diag_deep's; boundary_poly_add per coefficient plane (coeff_b: ext x 22, bnd1: ext values, c = the second divisor
// point, non-zero) into zeroed columns -> col0_out (ext planes of n) and the degree flag -> *flag_out.  With every mode
// PLAIN this is the table coeff_plain gives, so a caller compares sources against the materialised base + w e planes.
extern "C" int zk_diag_coeff_sources(int device, const uint8_t *tplanes, const uint8_t *modes, const uint8_t *w,
                                     const uint8_t *cpolys, int ccols, size_t n, int ext, const uint8_t *z,
                                     const uint8_t *zg, const uint8_t *alpha_t, const uint8_t *alpha_c,
                                     const uint8_t *coeff_b, const uint8_t *bnd1, const uint8_t *c, uint8_t *ood_out,
                                     uint8_t *deep_out, uint8_t *col0_out, uint32_t *flag_out) {
    fe2 zv, zgv;
    ZK_TRY(diag_back_half_args("zk_diag_coeff_sources", tplanes, cpolys, ccols, n, ext, z, zg, ood_out, &zv, &zgv));
    if (!modes || !w || !alpha_t || !alpha_c || !coeff_b || !bnd1 || !c || !deep_out || !col0_out || !flag_out)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_coeff_sources: null argument");
    if ((fe_is_zero(zv.a) && fe_is_zero(zv.b)) || (fe_is_zero(zgv.a) && fe_is_zero(zgv.b)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_coeff_sources: z and zg must be non-zero (their inverses are taken)");
    const int C = ccols / ext, log_n = ilog2(n);
    fe2 at[W], ac[8];
    for (int k = 0; k < W + C; k++)
        if (!diag_read_fe((k < W ? alpha_t + 16 * ext * k : alpha_c + 16 * ext * (k - W)), ext, k < W ? &at[k] : &ac[k - W]))
            ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_coeff_sources: non-canonical coefficient");
    fe wv[W];
    AirConsts K[2];
    memset(K, 0, sizeof K);
    const fe cv = fe_from_bytes(c);
    bool ok = fe_canonical(cv) && !fe_is_zero(cv);
    for (int k = 0; k < W; k++) {
        wv[k] = fe_from_bytes(w + 16 * k);
        ok = ok && fe_canonical(wv[k]) && modes[k] <= CoeffSrc::ZERO;
    }
    for (int j = 0; j < ext; j++) {
        for (int k = 0; k < NUM_ASSERTS; k++) {
            K[j].coeff_b[k] = fe_from_bytes(coeff_b + 16 * (NUM_ASSERTS * j + k));
            ok = ok && fe_canonical(K[j].coeff_b[k]);
        }
        K[j].bnd1 = fe_from_bytes(bnd1 + 16 * j);
        ok = ok && fe_canonical(K[j].bnd1);
    }
    if (!ok) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_coeff_sources: canonical values, modes 0 .. 2, c non-zero");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, n, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    if (ext == 2) ZK_TRY(ensure_ext(p));
    ZK_CHECK_HIP(hipMemcpy(p->polys, tplanes, (size_t)(W + 1) * n * 16, hipMemcpyHostToDevice));  // (polys holds 32 planes)
    ZK_CHECK_HIP(hipMemcpy(p->cpolys, cpolys, (size_t)ccols * n * 16, hipMemcpyHostToDevice));
    CoeffSrc TS = coeff_plain(p->polys, n);
    for (int k = 0; k < W; k++) {
        TS.mode[k] = modes[k];
        if (modes[k] == CoeffSrc::ZERO) TS.plane[k] = nullptr;
        if (modes[k] != CoeffSrc::PLAIN) TS.lagr = p->polys + (size_t)W * n;
    }
    const Planes b = planes(p, ext);
    return with_kx(ext, [&](auto kx) -> int {
        constexpr int KX = decltype(kx)::value;
        typedef Chal<KX> X;
        const typename X::T zz = X::make(zv), zzg = X::make(zgv);
        ood_eval(p->st, TS, W, p->cpolys, ccols, log_n, zz, zzg, b.ood_tab, b.partials, p->ood);
        std::vector<fe> raw((size_t)KX * ood_out_values(TS, W, ccols)), hv((size_t)KX * (2 * W + ccols));
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        ZK_CHECK_HIP(hipMemcpy(raw.data(), p->ood, raw.size() * sizeof(fe), hipMemcpyDeviceToHost));
        ood_fold_sources(KX, W, ccols, TS, wv, raw.data(), hv.data());
        memcpy(ood_out, hv.data(), hv.size() * sizeof(fe));
        DeepConsts<KX> D;
        memset(&D, 0, sizeof D);
        for (int k = 0; k < W; k++) D.alpha_t[k] = X::make(at[k]);
        for (int k = 0; k < C; k++) D.alpha_c[k] = X::make(ac[k]);
        D.z = zz, D.zg = zzg;
        deep_source_weight(D, TS, wv);
        ZK_CHECK_HIP(hipMemcpy(b.deep_consts, &D, sizeof D, hipMemcpyHostToDevice));
        const fe *Dk = deep_poly(p->st, TS, p->cpolys, C, log_n, b.deep_consts, zz, zzg, b.dscratch);
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        ZK_CHECK_HIP(hipMemcpy(deep_out, Dk, (size_t)KX * n * 16, hipMemcpyDeviceToHost));
        ZK_CHECK_HIP(hipMemsetAsync(p->flag, 0, 4, p->st));
        ZK_CHECK_HIP(hipMemsetAsync(p->ctmp, 0, (size_t)KX * n * 16, p->st));
        for (int j = 0; j < KX; j++)
            boundary_poly_add(p->st, TS, wv, log_n, K[j], cv, p->dscratch, p->ctmp + (size_t)j * n, p->flag);
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
        ZK_CHECK_HIP(hipMemcpy(col0_out, p->ctmp, (size_t)KX * n * 16, hipMemcpyDeviceToHost));
        ZK_CHECK_HIP(hipMemcpy(flag_out, p->flag, 4, hipMemcpyDeviceToHost));
        return ZK_OK;
    });
}

// One FRI layer through commit_fri_layer and fri_fold_launch: `layer` holds L values as the
// kernels read them (over E planar: L a components, then L b components; lb > 0: coset-major over 2^lb cosets,
// FriLayout), folded by `fold` at `alpha` (16 bytes, 32 over E) with x_r = 3 w_L^r taken from the tables of a plan of
// N = L wstride points.  root_out: the layer's Merkle root (32 bytes); next_out: the L / fold folded values (planar).
extern "C" int zk_diag_fri_layer(int device, const uint8_t *layer, size_t L, int ext, int fold, int lb, size_t wstride,
                                 const uint8_t *alpha, uint8_t *root_out, uint8_t *next_out) {
    fe2 av;
    const size_t N = L * wstride;
    const bool ok = layer && alpha && root_out && next_out && (ext == 1 || ext == 2) &&
                    (fold == 2 || fold == 4 || fold == 8 || fold == 16) && L && !(L & (L - 1)) && wstride &&
                    !(wstride & (wstride - 1)) && L >= 4 * (size_t)fold && N >= 128 && N <= ((size_t)1 << 22) && lb >= 0 &&
                    ((size_t)1 << lb) <= L / fold;
    if (!ok || !diag_read_fe(alpha, ext, &av))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_fri_layer: L and wstride powers of two, 128 <= L wstride <= 2^22, fold 2 .. 16, "
                                    "at least 4 rows, 2^lb <= L / fold, alpha canonical");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, N / 8, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, N / 8, 8, &pl));
    if (ext == 2) ZK_TRY(ensure_ext(p));
    const Planes b = planes(p, ext);
    const size_t rows = L / fold;
    uint8_t *leaves = p->fri_dig, *nodes = leaves + 32 * rows;
    ZK_CHECK_HIP(hipMemcpy(b.deep, layer, (size_t)ext * L * 16, hipMemcpyHostToDevice));
    ZK_TRY(with_kx(ext, [&](auto kx) -> int {
        const auto F = fold_consts<decltype(kx)::value>(av, (uint32_t)fold);
        ZK_CHECK_HIP(hipMemcpy(b.fold_consts, &F, sizeof F, hipMemcpyHostToDevice));
        return ZK_OK;
    }));
    commit_fri_layer(p->st, ext, b.deep, L, fold, leaves, nodes, lb);
    fri_fold_launch(p->st, ext, b.deep, L, fold, b.fold_consts, pl->TN, wstride, b.fri, lb);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(root_out, nodes + 32, 32, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(next_out, b.fri, (size_t)ext * rows * 16, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// One grind_launch over the nonces [start, start + count) with the result preset to ~0: *best_out = the smallest
// nonce whose BLAKE3(seed32 || nonce_le64) starts with >= bits trailing zero bits, ~0 when the window holds none.
extern "C" int zk_diag_grind(int device, const uint8_t *seed32, uint64_t start, uint32_t count, int bits,
                             uint64_t *best_out) {
    if (!seed32 || !best_out || count == 0 || bits < 0 || bits > 64 || start > UINT64_MAX - count)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_grind: count >= 1, 0 <= bits <= 64, start + count below 2^64");
    zk_prover *p = nullptr;
    ZK_TRY(zk_prover_create(device, 16, 8, &p));
    std::unique_ptr<zk_prover, void (*)(zk_prover *)> guard(p, zk_prover_destroy);
    ZK_CHECK_HIP(p->arena.alloc(&p->pow_seed, 8));
    ZK_CHECK_HIP(p->arena.alloc(&p->pow_best, 1));
    unsigned long long best = ~0ULL;
    ZK_CHECK_HIP(hipMemcpy(p->pow_seed, seed32, 32, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemcpy(p->pow_best, &best, 8, hipMemcpyHostToDevice));
    grind_launch(p->st, p->pow_seed, start, count, bits, p->pow_best);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_CHECK_HIP(hipMemcpy(&best, p->pow_best, 8, hipMemcpyDeviceToHost));
    *best_out = best;
    return ZK_OK;
}
