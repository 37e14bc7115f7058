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

hipError_t zk::make_pow_table(zk_prover *p, fe s, size_t n, PowTable *out) {
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

hipError_t zk::make_ntt_tables(zk_prover *p, int log_n, NttTables *T) {
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
std::vector<fe> zk::periodic_table(size_t n) {
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
    p->kept_comp_ext = 0;  // whatever follows may overwrite composition values kept for the plug points
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
    ZK_CHECK_HIP(A.alloc(&p->deg_rep, 1));  // transition constraint degrees: the device report
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
            if (r.host_ms >= 0) {  // a control exchange: host wall time, all of it exposed
                x = y = r.host_ms;
            } else {
                (void)hipEventElapsedTime(&x, p->xchg_pool[r.ev], p->xchg_pool[r.ev + 1]);
                if (r.waited) (void)hipEventElapsedTime(&y, p->xchg_pool[r.ev + 2], p->xchg_pool[r.ev + 3]);
            }
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
int zk::composition_stage(zk_prover *p, Plan *pl, int KX, int C, fe *comp, fe *ctmp, fe *clde, uint8_t root[32],
                          const AirConsts *bnd, int nce, const CoeffSrc *TS, const fe *w) {
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

// an empty report of a trace of n rows with get_assertions (air/src/lib.rs:170-195) in its own order
static void validation_begin(size_t n, const zk_pub_inputs *pub, zk_validation &V, fe expect[NUM_ASSERTS]) {
    memset(&V, 0, sizeof V);
    V.trace_len = n;
    V.steps_checked = n - 2;
    V.first_index = -1;
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

// the value of constraint k at global step s from the host evaluator, which must agree that it is not zero: the frame
// (s, s + 1) is rows[c ld .. + 1] of the 28 columns on the device (one strided copy)
static int validation_value(zk_prover *p, const fe *rows_dev, size_t ld, uint64_t s, int k, const zk_pub_inputs *pub,
                            uint8_t out[16]) {
    fe rows[W][2], cur[W], nxt[W], per[9], ev[NUM_TCONS];
    ZK_CHECK_HIP(hipMemcpy2DAsync(rows, 2 * sizeof(fe), rows_dev, ld * sizeof(fe), 2 * sizeof(fe), W,
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
    fe_to_bytes(ev[k], out);
    return ZK_OK;
}

// the first failure as winterfell's Trace::validate meets it (assertions first, then steps in order) into V, and the
// status with its message: ZK_OK, or ZK_ERR_TRACE
static int validation_verdict(zk_validation &V) {
    std::string msg;
    if (V.a_mask) {
        const int k = __builtin_ctz(V.a_mask);
        V.first_kind = 1;
        V.first_index = k;
        V.first_step = V.a_step[k];
        msg = "trace does not satisfy assertion main_trace(" + std::to_string(V.a_col[k]) + ", " +
              std::to_string(V.a_step[k]) + ") == " + u128_dec(fe_from_bytes(V.a_expected[k]));
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
    if (V.first_kind == 0) return ZK_OK;
    ZK_FAIL(ZK_ERR_TRACE, msg + "; " + std::to_string(V.failing_steps) + " failing steps, " + std::to_string(V.a_failed) +
                              " failed assertions");
}

// the trace is on p's device at d_trace; arguments are checked
static int validate_on_device(zk_prover *p, const fe *d_trace, size_t n, const zk_pub_inputs *pub, zk_validation *out) {
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    zk_validation V;
    fe expect[NUM_ASSERTS];
    validation_begin(n, pub, V, expect);
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
        ZK_TRY(validation_value(p, d_trace + s, n, s, k, pub, V.t_value[k]));
    }
    const int rc = validation_verdict(V);
    if (rc != ZK_OK && rc != ZK_ERR_TRACE) return rc;
    p->val_last = V;
    p->val_have = true;
    *out = V;
    return rc;
}

// ---- a sharded proof's validation (shard.hip): one rank's window, and the merged report
// Steps first .. first + count - 1 of a trace of n rows, whose rows first .. first + count are win[c ld + i] on p's
// device; arguments are checked by the caller.  Fills *out (shard_agree.hpp) whatever happens: an error of this rank
// (not a failing trace) goes into out->status / msg and is returned.
int zk::validate_window_partial(zk_prover *p, const fe *win, size_t ld, size_t n, const ValWindow &w,
                                const zk_pub_inputs *pub, int rank, ValPartial *out) {
    memset(out, 0, sizeof *out);
    out->version = ZK_AGREE_VERSION;
    out->rank = (uint32_t)rank;
    out->first = w.first;
    out->count = w.count;
    out->amask = w.amask;
    for (int k = 0; k < NUM_TCONS; k++) out->t_first[k] = UINT64_MAX;
    auto run = [&]() -> int {
        if (!w.count || ld < w.count + 1 || w.first + w.count > n - 2)
            ZK_FAIL(ZK_ERR_INVALID_ARG, "trace validation: a window outside the trace's steps");
        ZK_CHECK_HIP(hipSetDevice(p->device));
        IoScope io_scope(p);
        zk_validation V;
        fe expect[NUM_ASSERTS];
        validation_begin(n, pub, V, expect);
        ValReport R;
        memset(&R, 0, sizeof R);
        for (int k = 0; k < NUM_TCONS; k++) R.t_first[k] = ~0ull;
        for (int k = 0; k < NUM_ASSERTS; k++) R.a_found[k] = expect[k];
        ZK_TRY(h2d_small(p, p->val_rep, &R, sizeof R));
        ZK_CHECK_HIP(validate_window(p->st, win, ld, w.first, w.count, w.amask, p->val_per, fe_make(pub->delta),
                                     (int)pub->lwe_size, p->val_rep));
        ZK_TRY(d2h_small(p, &R, p->val_rep, sizeof R));
        ZK_TRY(d2h_flush(p));
        out->failing_steps = R.failing_steps;
        out->a_mask = R.a_mask & w.amask;
        for (int k = 0; k < NUM_ASSERTS; k++) fe_to_bytes(R.a_found[k], out->a_found[k]);
        for (int k = 0; k < NUM_TCONS; k++) {
            out->t_count[k] = R.t_count[k];
            if (!R.t_count[k]) continue;
            const uint64_t s = R.t_first[k];
            if (s < w.first || s >= w.first + w.count)
                ZK_FAIL(ZK_ERR_DEVICE, "trace validation: the device reported a step outside the window");
            out->t_first[k] = s;
            ZK_TRY(validation_value(p, win + (s - w.first), ld, s, k, pub, out->t_value[k]));
        }
        return ZK_OK;
    };
    const int rc = run();
    if (rc != ZK_OK) {
        out->status = rc;
        snprintf(out->msg, sizeof out->msg, "%s", g_err.c_str());
    }
    return rc;
}

// The merged report of `world` partials (merge_validation) of a trace of n rows, stored in each of the provers P
// (zk_prover_validation).  ZK_OK, ZK_ERR_TRACE with zk_validate_device's message, or -- a rank's partial carries an
// error -- ZK_ERR_PEER naming the lowest such rank (a local rank's own error: shard.hip returns it as it was met).
int zk::validation_from_partials(const ValPartial *parts, int world, size_t n, const zk_pub_inputs *pub,
                                 zk_prover *const *P, int np, zk_validation *out) {
    zk_validation V;
    fe expect[NUM_ASSERTS];
    validation_begin(n, pub, V, expect);
    int bad = -1;
    if (merge_validation(parts, world, &V, &bad) != ZK_OK) {
        char m[ZK_AGREE_MSG + 1];
        memcpy(m, parts[bad].msg, ZK_AGREE_MSG);
        m[ZK_AGREE_MSG] = 0;
        ZK_FAIL(ZK_ERR_PEER, "rank " + std::to_string(bad) + " could not validate its rows: " +
                                 std::to_string(parts[bad].status) + ": " + m);
    }
    const int rc = validation_verdict(V);
    if (rc != ZK_OK && rc != ZK_ERR_TRACE) return rc;
    for (int l = 0; l < np; l++) {
        P[l]->val_last = V;
        P[l]->val_have = true;
    }
    if (out) *out = V;
    return rc;
}

// ---- the scaffold of the two stand-alone checks (trace validation above, constraint degrees below)
// the arguments of their four entry points; trace: the device pointer or the column table, out: the report
static int check_standalone_args(zk_prover *p, const void *trace, size_t n, const zk_pub_inputs *pub, const void *out) {
    if (!p || !trace || !pub || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    ZK_TRY(check_trace_len(n, p->max_n));
    return check_lwe_size(pub);
}

// check(p->d_trace) on the 28 host columns: one full upload, every column whole (a debugging aid: none of the prove
// path's column classes).  The caller's columns are free again on every way out, a failed copy included.
template <class Check>
static int with_uploaded_columns(zk_prover *p, const uint8_t *const *columns, size_t n, Check check) {
    for (int c = 0; c < W; c++)
        if (!columns[c]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null trace column");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    const int rc = [&]() -> int {
        for (int c = 0; c < W; c++)
            ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace + (size_t)c * n, columns[c], n * sizeof(fe), hipMemcpyHostToDevice, p->st));
        return check(p->d_trace);
    }();
    (void)hipStreamSynchronize(p->st);
    return rc;
}

// The gate of a check the prove entry points run first (zk_prover_set_validate / _validate_degrees): its switch is on,
// and the call is one prove_impl would enter on a full prover.  Arguments the prove path would refuse are left for it
// to report.
static bool check_runs_first(const zk_prover *p, bool zk_prover::*on, size_t n, const zk_options *opt,
                             const zk_pub_inputs *pub, const size_t *proof_len) {
    if (!p || !(p->*on) || !proof_len || p->shard_world > 1) return false;
    return check_prove_args(n, p->max_n, p->max_b, opt, pub) == ZK_OK;
}

int zk_validate_device(zk_prover *p, const void *d_trace, size_t n, const zk_pub_inputs *pub, zk_validation *out) {
    ZK_TRY(check_standalone_args(p, d_trace, n, pub, out));
    return validate_on_device(p, (const fe *)d_trace, n, pub, out);
}

int zk_validate_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub,
                        zk_validation *out) {
    ZK_TRY(check_standalone_args(p, columns, n, pub, out));
    return with_uploaded_columns(p, columns, n, [&](const fe *t) { return validate_on_device(p, t, n, pub, out); });
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

// zk_prover_set_validate(p, 1): Trace::validate before the proof (check_runs_first).  A failing trace ends the call
// with ZK_ERR_TRACE and an empty proof before prove_impl is entered, so no hint or snapshot state moves.
static int validate_first(zk_prover *p, const void *d_trace, const uint8_t *const *cols, size_t n, const zk_options *opt,
                          const zk_pub_inputs *pub, size_t *proof_len) {
    if (!check_runs_first(p, &zk_prover::validate, n, opt, pub, proof_len)) return ZK_OK;
    zk_validation v;
    const int rc = cols ? zk_validate_columns(p, cols, n, pub, &v) : zk_validate_device(p, d_trace, n, pub, &v);
    if (rc != ZK_OK) *proof_len = 0;
    return rc;
}

// ---------------------------------------------------------------- transition constraint degrees
// validate_transition_degrees (winterfell 0.9, the debug-build step of DefaultConstraintEvaluator::evaluate) on the
// GPU: include/zkvm_gpu.h "transition constraint degrees" fixes the semantics; kernels.hip k_transition_quotients and
// k_poly_degrees are the device side.  No allocation of its own beyond the small report: the check runs in the
// buffers of a proof, which none of its stages needs at the same time --
//   p->polys  the 28 trace polynomials (dense interpolation of d_trace: ntt inverse, scale 1/n);
//   p->lde    first the trace LDE over the 8 CE cosets (28 x 8 x n, the cosets 0, B/8, 2B/8, ... of the plan's blowup
//             B), then, once the quotients are written, the 160 per-coset inverse transforms (20 x 8 x n);
//   p->tmp    (28 x 8n) the four-step scratch of the front, then the 20 x 8n quotient values with the 8 x 8n behind them
//             as the four-step scratch of their inverse transforms (groups of 8 constraints), and last, the values
//             consumed, the 20 x 8n coefficients the cross-coset step writes (read by k_poly_degrees and quotients_out).
// (the report and winterfell's message from the tops: shard_agree.hpp degrees_report / degrees_message, shared with
// a sharded proof's merge)
// the trace is on p's device at d_trace; arguments are checked.  B: the blowup whose plan lends its tables
static int degrees_on_device(zk_prover *p, const fe *d_trace, size_t n, const zk_pub_inputs *pub, uint32_t B,
                             zk_degrees *out, uint8_t *quotients_out) {
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, B, &pl));
    const int log_n = pl->log_n;
    const size_t CE = 8 * n;
    // the front: dense interpolation of all 28 columns, then their LDE over the 8 CE cosets
    const fe inv_n = h_inv(fe_make(n));
    ntt(p->st, pl->Tn, d_trace, n, p->polys, n, W, true, nullptr, &inv_n, p->tmp);
    ntt_lde(p->st, pl->Tn, pl->ct, p->polys, n, W, 0, (int)(B / 8), 8, p->lde, CE, n, p->tmp);
    const fe *binv = boundary_inverses(p, pl);
    if (!binv) ZK_FAIL(ZK_ERR_OUT_OF_MEMORY, "transition divisor table");
    const EvalMap map{8, 0, 1, 0, 8};
    fe *quot = p->tmp, *scratch = p->tmp + NUM_TCONS * CE, *per_coset = p->lde;
    ZK_CHECK_HIP(transition_quotients(p->st, p->lde, log_n, map, pl->periodic, binv, fe_make(pub->delta),
                                      (int)pub->lwe_size, quot));
    // the composition's interpolation per constraint: 8 per-coset inverse transforms (no scale), then the radix-8
    // cross-coset step with scale 1/(8n), all 8 blocks of n coefficients kept
    for (int k0 = 0; k0 < NUM_TCONS; k0 += 8) {
        const int cnt = std::min(8, NUM_TCONS - k0);
        ntt(p->st, pl->Tn, quot + k0 * CE, n, per_coset + k0 * CE, n, 8 * cnt, true, nullptr, nullptr, scratch);
    }
    const fe w8 = h_root_of_unity(3);
    for (int k = 0; k < NUM_TCONS; k++) {
        CrossMap m;
        for (int r = 0; r < 8; r++) m.c[r] = per_coset + (size_t)(8 * k + r) * n;
        m.k0 = 0;
        m.kcount = n;
        m.pstride = n;
        comp_cross_mapped(p->st, m, pl->Tce, pl->inv3, h_inv(fe_make(CE)), h_inv(w8), h_inv(h_pow(fe_make(3), n)), 8,
                          quot + k * CE, p->flag);
    }
    ZK_CHECK_HIP(hipMemsetAsync(p->deg_rep, 0, sizeof(DegReport), p->st));
    poly_degrees(p->st, quot, CE, NUM_TCONS, p->deg_rep);
    ZK_CHECK_HIP(hipGetLastError());
    DegReport R;
    ZK_TRY(d2h_small(p, &R, p->deg_rep, sizeof R));
    ZK_TRY(d2h_flush(p));
    if (quotients_out) {
        ZK_CHECK_HIP(hipMemcpyAsync(quotients_out, quot, NUM_TCONS * CE * sizeof(fe), hipMemcpyDeviceToHost, p->st));
        ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    }
    collect_kernel_stats(p);  // (zk_prover_profile: a stand-alone check's kernels are counted like a proof's)
    for (int k = 0; k < NUM_TCONS; k++)
        if (R.top[k] >= CE) ZK_FAIL(ZK_ERR_DEVICE, "constraint degrees: the device reported a coefficient outside the domain");
    zk_degrees D;
    uint64_t top[NUM_TCONS];
    for (int k = 0; k < NUM_TCONS; k++) top[k] = R.top[k];
    degrees_report(n, top, R.nonzero, &D);
    p->deg_last = D;
    p->deg_have = true;
    *out = D;
    if (!D.mismatch_mask) return ZK_OK;
    ZK_FAIL(ZK_ERR_DEGREES, degrees_message(D));
}

// The merged report of `world` partials (merge_degrees) of a sharded degree check of a trace of n rows, stored in each
// of the provers P (zk_prover_degrees).  ZK_OK, ZK_ERR_DEGREES with zk_degrees_device's message, or -- a rank's partial
// carries an error -- ZK_ERR_PEER naming the lowest such rank.
int zk::degrees_from_partials(const DegPartial *parts, int world, size_t n, zk_prover *const *P, int np,
                              zk_degrees *out) {
    zk_degrees D;
    int bad = -1;
    if (merge_degrees(parts, world, n, &D, &bad) != ZK_OK) {
        if (parts[bad].version != ZK_AGREE_VERSION)
            ZK_FAIL(ZK_ERR_PEER, "rank " + std::to_string(bad) + " sent a degree partial of layout version " +
                                     std::to_string(parts[bad].version));
        if (parts[bad].status == ZK_OK)
            ZK_FAIL(ZK_ERR_PEER, "rank " + std::to_string(bad) + " reported a coefficient outside the domain");
        char m[ZK_AGREE_MSG + 1];
        memcpy(m, parts[bad].msg, ZK_AGREE_MSG);
        m[ZK_AGREE_MSG] = 0;
        ZK_FAIL(ZK_ERR_PEER, "rank " + std::to_string(bad) + " could not check its coefficients: " +
                                 std::to_string(parts[bad].status) + ": " + m);
    }
    for (int l = 0; l < np; l++) {
        P[l]->deg_last = D;
        P[l]->deg_have = true;
    }
    if (out) *out = D;
    if (!D.mismatch_mask) return ZK_OK;
    ZK_FAIL(ZK_ERR_DEGREES, degrees_message(D));
}

static int degrees_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub, uint32_t B,
                           zk_degrees *out, uint8_t *quotients_out) {
    return with_uploaded_columns(p, columns, n,
                                 [&](const fe *t) { return degrees_on_device(p, t, n, pub, B, out, quotients_out); });
}

int zk_degrees_device(zk_prover *p, const void *d_trace, size_t n, const zk_pub_inputs *pub, zk_degrees *out,
                      uint8_t *quotients_out) {
    ZK_TRY(check_standalone_args(p, d_trace, n, pub, out));
    return degrees_on_device(p, (const fe *)d_trace, n, pub, 8, out, quotients_out);
}

int zk_degrees_columns(zk_prover *p, const uint8_t *const *columns, size_t n, const zk_pub_inputs *pub,
                       zk_degrees *out, uint8_t *quotients_out) {
    ZK_TRY(check_standalone_args(p, columns, n, pub, out));
    return degrees_columns(p, columns, n, pub, 8, out, quotients_out);
}

int zk_prover_set_validate_degrees(zk_prover *p, int on) {
    if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    p->validate_degrees = on != 0;
    return ZK_OK;
}

int zk_prover_degrees(const zk_prover *p, zk_degrees *out) {
    if (!p || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (!p->deg_have) ZK_FAIL(ZK_ERR_INVALID_ARG, "no degree check has run on this prover");
    *out = p->deg_last;
    return ZK_OK;
}

// zk_prover_set_validate_degrees(p, 1): validate_transition_degrees before the proof, after validate_first (the order
// of a debug build; check_runs_first).  As there, a mismatch ends the call before prove_impl is entered.  The CE cosets
// come from the tables of the proof's own blowup (cosets 0, B/8, ... of its LDE domain are the CE domain), so no plan
// is built that the proof does not need.
static int degrees_first(zk_prover *p, const void *d_trace, const uint8_t *const *cols, size_t n, const zk_options *opt,
                         const zk_pub_inputs *pub, size_t *proof_len) {
    if (!check_runs_first(p, &zk_prover::validate_degrees, n, opt, pub, proof_len)) return ZK_OK;
    zk_degrees d;
    const int rc = cols ? degrees_columns(p, cols, n, pub, opt->blowup, &d, nullptr)
                        : degrees_on_device(p, (const fe *)d_trace, n, pub, opt->blowup, &d, nullptr);
    if (rc != ZK_OK) *proof_len = 0;
    return rc;
}

int zk_prove_device(zk_prover *p, const void *d_trace, size_t n, const zk_options *opt, const zk_pub_inputs *pub,
                    uint8_t *proof_out, size_t *proof_len, zk_record *rec, const zk_dump *dump) {
    if (!d_trace) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_TRY(validate_first(p, d_trace, nullptr, n, opt, pub, proof_len));
    ZK_TRY(degrees_first(p, d_trace, nullptr, n, opt, pub, proof_len));
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
    ZK_TRY(degrees_first(p, nullptr, columns, n, opt, pub, proof_len));
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
// interpolate, extend and commit the 28 host columns; polys_out (optional): the 28 x n coefficients (TracePolyTable)
static int lde_new_columns(zk_prover *p, const uint8_t *const *cols, size_t n, uint32_t blowup, zk_trace_lde **out,
                           uint8_t root[32], uint8_t *polys_out) {
    if (n < 16 || (n & (n - 1)) || n > p->max_n || blowup < 8 || (blowup & (blowup - 1)) || blowup > p->max_b)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid trace length or blowup");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    Plan *pl;
    int rc = get_plan(p, n, blowup, &pl);
    if (rc) return rc;
    TraceSrc src;
    src.cols = cols;
    src.hint_ok = false;  // no proof follows to verify a hint
    uint8_t r[32];
    rc = trace_lde_commit(p, pl, src, n, r);
    if (!rc) rc = d2h_flush(p);
    upload_drain(p);  // the caller's trace is no longer read once this returns
    if (rc) return rc;
    if (polys_out) {
        // without hints no column is read at its source: every coefficient is in polys (the stream is idle: d2h_flush)
        if (p->tc.coeff_src) ZK_FAIL(ZK_ERR_DEVICE, "trace coefficients were not written");
        ZK_CHECK_HIP(hipMemcpy(polys_out, p->polys, (size_t)W * n * sizeof(fe), hipMemcpyDeviceToHost));
    }
    if (root) memcpy(root, r, 32);
    *out = new zk_trace_lde{p, n, blowup, W};
    return ZK_OK;
}

int zk_lde_new(zk_prover *p, const uint8_t *trace, size_t width, size_t n, uint32_t blowup, zk_trace_lde **out,
               uint8_t root[32]) {
    if (!p || !trace || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    if (width != (size_t)W) ZK_FAIL(ZK_ERR_INVALID_ARG, "ProcessorAir traces have 28 columns");
    const uint8_t *cols[W];
    for (int c = 0; c < W; c++) cols[c] = trace + (size_t)c * n * sizeof(fe);
    return lde_new_columns(p, cols, n, blowup, out, root, nullptr);
}

int zk_lde_new_columns(zk_prover *p, const uint8_t *const *columns, size_t n, uint32_t blowup, zk_trace_lde **out,
                       uint8_t root[32], uint8_t *polys_out) {
    if (!p || !columns || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    ZK_REQUIRE_FULL_PROVER(p);
    for (int c = 0; c < W; c++)
        if (!columns[c]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null trace column");
    return lde_new_columns(p, columns, n, blowup, out, root, polys_out);
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

// The two halves of a direct batch opening, shared by the plug points' queries below and zk_diag_merkle (diag.hip).
// query_positions: the k positions of a query over N leaves into pos, refused unless 1 <= k <= ZK_MAX_QUERIES, each
// below N and all distinct.
int zk::query_positions(const uint64_t *positions, size_t k, size_t N, std::vector<uint64_t> &pos) {
    if (!positions || k == 0 || k > ZK_MAX_QUERIES) ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid query arguments");
    pos.assign(positions, positions + k);
    for (uint64_t x : pos)
        if (x >= N) ZK_FAIL(ZK_ERR_INVALID_ARG, "query position out of range");
    // MerkleTree::prove_batch refuses a repeated index (MerkleTreeError::DuplicateLeafIndex): the batch proof
    // holds one path per distinct leaf pair, and a verifier rebuilds the root from distinct positions
    std::vector<uint64_t> sorted(pos);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        ZK_FAIL(ZK_ERR_INVALID_ARG, "duplicate query position");
    return ZK_OK;
}
// batch_proof_bytes: the serialized batch Merkle proof of pos over the N device leaves and their heap `nodes` (idle
// stream: plain copies), plan_batch's digests in its order.  *proof_len: in the capacity of proof_out, out the length.
int zk::batch_proof_bytes(size_t N, const std::vector<uint64_t> &pos, const uint8_t *leaves, const uint8_t *nodes,
                          uint8_t *proof_out, size_t *proof_len) {
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

// rows at `positions` of a committed coset-major LDE (ncols columns) + the batch Merkle proof bytes
static int query_committed_rows(zk_prover *p, const fe *base, int ncols, size_t n, uint32_t B, const uint8_t *leaves,
                                const uint8_t *nodes, const uint64_t *positions, size_t k, uint8_t *rows_out,
                                uint8_t *proof_out, size_t *proof_len) {
    if (!rows_out || !proof_len) ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid query arguments");
    const size_t N = n * B;
    std::vector<uint64_t> pos;
    ZK_TRY(query_positions(positions, k, N, pos));
    ZK_CHECK_HIP(hipMemcpyAsync(p->gather_idx, pos.data(), k * 8, hipMemcpyHostToDevice, p->st));
    gather_rows(p->st, base, ncols, ilog2(n), ilog2(B), p->gather_idx, k, p->gather_out);
    ZK_CHECK_HIP(hipMemcpyAsync(rows_out, p->gather_out, k * ncols * 16, hipMemcpyDeviceToHost, p->st));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    return batch_proof_bytes(N, pos, leaves, nodes, proof_out, proof_len);
}

int zk_lde_query(zk_trace_lde *h, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                 size_t *proof_len) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    zk_prover *p = h->p;
    return query_committed_rows(p, p->lde, W, h->n, h->B, p->leaves, p->nodes, positions, k, rows_out, proof_out,
                                proof_len);
}

// The plug points' bulk reads: rows (first + k) mod N, k < count, of a committed coset-major LDE as a row matrix in
// `out`.  rows_layout forms up to cap_rows rows at a time in `stage` and a contiguous copy takes them to the host,
// kernel and copy in order on st (the kernel is a few per cent of the copy), one synchronisation at the end.  A chunk
// ends at the domain's end, where a window that wraps starts again at row 0, so no launch wraps.
int zk::rows_to_host(hipStream_t st, const fe *base, int ncols, size_t n, uint32_t B, size_t first, size_t count,
                     fe *stage, size_t cap_rows, uint8_t *out, unsigned max_blocks) {
    const size_t N = n * B, row = (size_t)ncols * sizeof(fe);
    const int log_b = ilog2(B);
    for (size_t done = 0; done < count;) {
        const size_t f = (first + done) % N, c = std::min({count - done, N - f, cap_rows});
        rows_layout(st, base, ncols, n, log_b, f, c, stage, max_blocks);
        ZK_CHECK_HIP(hipMemcpyAsync(out + done * row, stage, c * row, hipMemcpyDeviceToHost, st));
        done += c;
    }
    ZK_CHECK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
}

// Both read calls stage in p->tmp (28 x 8 max_n elements: 8 max_n rows of 28, more of a narrower row).  It is the
// scratch of the NTTs, the degree check and the VM's trace generation, written and read within one call each on p->st;
// nothing a handle, the kept composition values, the hints or a snapshot hold lives there (the LDEs are in lde / clde
// / x_clde, the kept values in comp / x_comp, the snapshots in buffers of their own), and no plan is fetched, so the
// kept values stay valid.
static int read_committed_rows(zk_prover *p, const fe *base, int ncols, size_t n, uint32_t B, size_t first,
                               size_t count, uint8_t *rows_out) {
    if (!rows_out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (first >= n * B || count == 0 || count > n * B + B)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "first below N and 1 <= count <= N + blowup");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    const size_t cap_rows = (size_t)W * 8 * p->max_n / ncols;
    ZK_TRY(rows_to_host(p->st, base, ncols, n, B, first, count, p->tmp, cap_rows, rows_out, 0));
    collect_kernel_stats(p);
    return ZK_OK;
}

int zk_lde_read_rows(zk_trace_lde *h, size_t first, size_t count, uint8_t *rows_out) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    return read_committed_rows(h->p, h->p->lde, W, h->n, h->B, first, count, rows_out);
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

// The same over the challenge field: ext = 1 (the call above, byte for byte) or 2 (E coefficients and values as
// (a, b) pairs of 16 bytes).  The evaluator leaves `ext` coset-major planes; ce_layout puts them in winterfell's order
// on the device, so the host side is one contiguous copy.  out = NULL keeps the planes for zk_commit_composition_ext.
int zk_eval_constraints_ext(zk_trace_lde *h, const zk_pub_inputs *pub, uint32_t ext, const uint8_t *coeff_t,
                            const uint8_t *coeff_b, uint8_t *out) {
    if (!h || !pub || !coeff_t || !coeff_b) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (ext != 1 && ext != 2) ZK_FAIL(ZK_ERR_INVALID_ARG, "ext must be 1 (base field) or 2 (quadratic extension)");
    if (pub->lwe_size == 0 || pub->lwe_size > 5) ZK_FAIL(ZK_ERR_INVALID_ARG, "lwe_size must be in [1, 5]");
    zk_prover *p = h->p;
    const size_t n = h->n, CE = 8 * n;
    const int KX = (int)ext;
    ZK_CHECK_HIP(hipSetDevice(p->device));
    if (KX == 2) ZK_TRY(ensure_ext(p));
    Plan *pl;
    ZK_TRY(get_plan(p, n, h->B, &pl));
    const Planes b = planes(p, KX);
    AirConsts K[2];
    memset(K, 0, sizeof K);
    for (int j = 0; j < KX; j++) {
        for (int k = 0; k < NUM_TCONS; k++) K[j].coeff_t[k] = fe_from_bytes(coeff_t + 16 * (KX * k + j));
        for (int k = 0; k < NUM_ASSERTS; k++) K[j].coeff_b[k] = fe_from_bytes(coeff_b + 16 * (KX * k + j));
    }
    const fe *per = air_static_consts(pub, n, K[0]);
    if (KX == 2) {  // the b plane: the same constants around its own coefficients (draw_air_consts)
        const AirConsts kb = K[1];
        K[1] = K[0];
        memcpy(K[1].coeff_t, kb.coeff_t, sizeof kb.coeff_t);
        memcpy(K[1].coeff_b, kb.coeff_b, sizeof kb.coeff_b);
        set_coeff_derived(K[1], per);
    }
    ZK_CHECK_HIP(hipMemcpyAsync(b.air_consts, K, KX * sizeof K[0], hipMemcpyHostToDevice, p->st));
    const fe *binv = boundary_inverses(p, pl);
    if (!binv) ZK_FAIL(ZK_ERR_OUT_OF_MEMORY, "boundary divisor table");
    ZK_CHECK_HIP(eval_constraints(p->st, KX, p->lde, pl->log_n, eval_map_whole(pl->log_b, 8, true), pl->periodic, binv,
                                  (const AirConsts *)b.air_consts, KX == 2 ? CE : 0, b.comp, true));
    if (out) ce_layout(p->st, b.comp, n, KX, true, b.ctmp);
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));  // (K is read by the copy above until here)
    collect_kernel_stats(p);  // (zk_prover_profile: a plug point's kernels are counted like a proof's)
    if (out) {
        ZK_CHECK_HIP(hipMemcpy(out, b.ctmp, (size_t)KX * CE * sizeof(fe), hipMemcpyDeviceToHost));
    } else {
        p->kept_comp_ext = KX;
        p->kept_comp_lde = h;
    }
    return ZK_OK;
}

// ---------------------------------------------------------------- plug point 3: constraint commitment
struct zk_comp_commit {
    zk_prover *p;
    size_t n;
    uint32_t B;
    int ncols;
    int ext = 1;  // base elements per value: rows are ncols * ext elements of the plane set's composition LDE
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

// The same over the challenge field.  composition: 8n values in winterfell's order, copied up whole and put into the
// stage's coset-major planes by ce_layout; NULL: the planes zk_eval_constraints_ext(out = NULL) kept on this handle.
int zk_commit_composition_ext(zk_trace_lde *h, const uint8_t *composition, uint32_t ext, uint32_t num_cols,
                              zk_comp_commit **out, uint8_t root[32], uint8_t *polys_out) {
    if (!h || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (ext != 1 && ext != 2) ZK_FAIL(ZK_ERR_INVALID_ARG, "ext must be 1 (base field) or 2 (quadratic extension)");
    if (num_cols < 1 || num_cols > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "num_cols must be in [1, 8]");
    zk_prover *p = h->p;
    const size_t n = h->n, CE = 8 * n;
    const int KX = (int)ext, C = (int)num_cols;
    if (!composition && (p->kept_comp_ext != KX || p->kept_comp_lde != h))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "no composition values of this ext are kept on the device for this trace LDE");
    ZK_CHECK_HIP(hipSetDevice(p->device));
    IoScope io_scope(p);
    if (KX == 2) ZK_TRY(ensure_ext(p));
    Plan *pl;
    ZK_TRY(get_plan(p, n, h->B, &pl));  // (the kept values end here: the stage consumes them)
    const Planes b = planes(p, KX);
    if (composition) {
        ZK_CHECK_HIP(hipMemcpyAsync(b.ctmp, composition, (size_t)KX * CE * sizeof(fe), hipMemcpyHostToDevice, p->st));
        ce_layout(p->st, b.ctmp, n, KX, false, b.comp);
    }
    uint8_t r[32];
    ZK_TRY(composition_stage(p, pl, KX, C, b.comp, b.ctmp, b.clde, r));
    unsigned degree_flag = 0;
    ZK_TRY(d2h_small(p, &degree_flag, p->flag, 4));
    ZK_TRY(d2h_flush(p));  // root and flag
    if (degree_flag) ZK_FAIL(ZK_ERR_DEGREE, "composition polynomial degree exceeds num_cols * trace_len");
    if (polys_out) {
        const fe *src = p->cpolys;
        if (KX == 2) {  // the stage is done with the value planes: they stage the interleaved columns
            interleave_columns(p->st, p->cpolys, n, C, b.comp);
            ZK_CHECK_HIP(hipStreamSynchronize(p->st));
            src = b.comp;
        }
        ZK_CHECK_HIP(hipMemcpy(polys_out, src, (size_t)KX * C * n * sizeof(fe), hipMemcpyDeviceToHost));
    }
    collect_kernel_stats(p);
    if (root) memcpy(root, r, 32);
    *out = new zk_comp_commit{p, n, h->B, C, KX};
    return ZK_OK;
}

int zk_comp_query(zk_comp_commit *h, const uint64_t *positions, size_t k, uint8_t *rows_out, uint8_t *proof_out,
                  size_t *proof_len) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    zk_prover *p = h->p;
    return query_committed_rows(p, planes(p, h->ext).clde, h->ncols * h->ext, h->n, h->B, p->cleaves, p->cnodes,
                                positions, k, rows_out, proof_out, proof_len);
}

int zk_comp_read_rows(zk_comp_commit *h, size_t first, size_t count, uint8_t *rows_out) {
    if (!h) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    return read_committed_rows(h->p, planes(h->p, h->ext).clde, h->ncols * h->ext, h->n, h->B, first, count, rows_out);
}

void zk_comp_free(zk_comp_commit *h) { delete h; }
