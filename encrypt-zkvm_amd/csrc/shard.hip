// shard.hip -- one proof with the LDE domain sharded by coset over `world` GPUs.
//
// Rank g of G owns the LDE cosets r = g*Bl + j, j < Bl = 8/G (blowup 8; round 6: a block, so that the Merkle leaves
// 8q + r of a group q that one rank holds are siblings).  Per stage:
//   trace interpolation          host trace: split by column (a rank uploads and interpolates W/G columns,
//                                round robin), in-place all-gathers of the coefficients; device trace: replicated
//   trace LDE, constraint eval,  local: a coset's LDE is an independent size-n NTT, and constraint
//   DEEP LDE, first FRI fold     row i+8 / a fold row {e[r' + k N/fold]} stay inside one coset
//   OOD values, DEEP coefficients  split by coefficient range; all-gathers of partial sums / range totals and of
//                                the quotient slices
//   Merkle trees                 each rank hashes its leaves and their subtree up to its block of Bl siblings,
//   (trace, composition, FRI 0)  all-to-all of the block nodes into contiguous ranges, a local subtree per rank,
//                                all-gather of the G subtree roots
//   composition interpolation    per-coset inverse NTT local; all-to-all of coefficient slices for the
//                                cross-coset radix-8 step; all-gather of the 7 column polynomials
//   FRI layers 1, >= 2           layer 1 as layer 0 (block trees, local fold), all-gather of layer 2, then the
//                                rest on the lead rank (small)
//   openings                     every rank gathers what it owns, all-gather, the host combines
// The Fiat-Shamir transcript runs on every process's host over identical (all-gathered) roots, so no
// challenge is ever broadcast.  The proof bytes equal the single-GPU prover's (tests/test_sharded.py).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "blake3.hpp"
#include "comm.hpp"
#include "fri_small.hpp"
#include "host_pool.hpp"
#include "prover_internal.hpp"
#include "shard_agree.hpp"

using namespace zk;

namespace {

// ---------------------------------------------------------------- loopback communicator
// Every rank in this process: the collective is device-to-device copies, all of them on the issue stream (ordered
// after every rank's compute stream by xchg_start), so its completion covers every rank's reads and writes.
struct LoopbackComm : zk_comm {
    bool loopback() const override { return true; }
    int all_to_all(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        if ((int)P.size() != world) ZK_FAIL(ZK_ERR_INVALID_ARG, "a loopback communicator drives every rank");
        for (int d = 0; d < world; d++)
            for (int s = 0; s < world; s++)
                ZK_CHECK_HIP(hipMemcpyAsync((uint8_t *)recv[d] + s * bytes, (const uint8_t *)send[s] + d * bytes, bytes,
                                            hipMemcpyDeviceToDevice, is));
        return ZK_OK;
    }
    int all_gather(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        if ((int)P.size() != world) ZK_FAIL(ZK_ERR_INVALID_ARG, "a loopback communicator drives every rank");
        for (int d = 0; d < world; d++)
            for (int s = 0; s < world; s++)
                if ((uint8_t *)recv[d] + s * bytes != send[s])  // in place: a rank's own chunk is already there
                    ZK_CHECK_HIP(hipMemcpyAsync((uint8_t *)recv[d] + s * bytes, send[s], bytes, hipMemcpyDeviceToDevice, is));
        return ZK_OK;
    }
    int control_gather(const void *send, void *recv, size_t bytes) override {
        memcpy(recv, send, bytes * (size_t)world);
        return ZK_OK;
    }
};

// ---------------------------------------------------------------- caller-transport communicator
// One rank per process, exchanges through a caller callback over host memory (MPI, gloo, TCP across nodes).  The
// staging is synchronous on the host: device chunk -> host on the issue stream, callback, host -> device.
struct HostComm : zk_comm {
    zk_exchange_fn fn = nullptr;
    void *ctx = nullptr;
    std::vector<uint8_t> sbuf, rbuf;
    bool loopback() const override { return false; }
    int run(const std::vector<zk_prover *> &P, int op, const void *send, size_t sbytes, void *recv, size_t bytes,
            hipStream_t is) {
        if (P.size() != 1) ZK_FAIL(ZK_ERR_INVALID_ARG, "a host-exchange communicator drives exactly one local rank");
        const size_t rbytes = bytes * (size_t)world;
        sbuf.resize(std::max<size_t>(sbytes, 1));
        rbuf.resize(std::max<size_t>(rbytes, 1));
        if (sbytes) ZK_CHECK_HIP(hipMemcpyAsync(sbuf.data(), send, sbytes, hipMemcpyDeviceToHost, is));
        ZK_CHECK_HIP(hipStreamSynchronize(is));
        const int rc = fn(ctx, op, sbuf.data(), rbuf.data(), bytes);
        if (rc != 0) ZK_FAIL(ZK_ERR_DEVICE, "exchange callback failed (" + std::to_string(rc) + ")");
        if (rbytes) ZK_CHECK_HIP(hipMemcpyAsync(recv, rbuf.data(), rbytes, hipMemcpyHostToDevice, is));
        ZK_CHECK_HIP(hipStreamSynchronize(is));  // rbuf is reused by the next exchange
        return ZK_OK;
    }
    int all_to_all(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        return run(P, ZK_XCHG_ALL_TO_ALL, send.at(0), bytes * (size_t)world, recv.at(0), bytes, is);
    }
    int all_gather(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        return run(P, ZK_XCHG_ALL_GATHER, send.at(0), bytes, recv.at(0), bytes, is);
    }
    int control_gather(const void *send, void *recv, size_t bytes) override {  // host buffers: no device round trip
        const int rc = fn(ctx, ZK_XCHG_ALL_GATHER, send, recv, bytes);
        if (rc != 0) ZK_FAIL(ZK_ERR_DEVICE, "exchange callback failed (" + std::to_string(rc) + ")");
        return ZK_OK;
    }
};

// ---------------------------------------------------------------- local-coset kernels
// Block ownership (round 6): rank g owns the cosets g Bl .. g Bl + Bl - 1, so in every group q of 8 consecutive leaves
// 8q .. 8q + 7 (leaf 8q + r: row q of coset r) its Bl leaves are siblings: it hashes them and their subtree up to level
// Lb = log2 Bl itself, and only that block node -- 1/Bl of the leaf digests -- crosses the link.  Each tree keeps the
// levels 0 .. Lb of its own leaves in a block buffer (level l: node (q, i) at lvl_off(l) + q (Bl >> l) + i, for the
// openings) and sends the block nodes out in K pieces: piece k holds, for every destination d, the groups
// q = d QG + k QGK + q'' (QG = Q / G groups per destination, QGK = QG / K), in send order [d][q''].
__device__ __forceinline__ size_t blk_group(size_t t, int log_QG, int log_K, int k) {
    const int log_QGK = log_QG - log_K;
    const size_t qq = t & (((size_t)1 << log_QGK) - 1), d = t >> log_QGK;
    return (d << log_QG) + ((size_t)k << log_QGK) + qq;
}
// the Bl leaves of group q (leaf(j, h): local coset slot j), their subtree into blk, the block node into send_slot
template <int BL, typename Leaf>
__device__ __forceinline__ void blk_levels(size_t Q, size_t q, uint8_t *blk, uint8_t *send_slot, Leaf leaf) {
    static_assert(BL == 1 || BL == 2 || BL == 4, "a sharded rank holds 1, 2 or 4 cosets");
    uint32_t a[8];
    leaf(0, a);
    b3::store_digest(blk + 32 * (q * BL), a);
    if constexpr (BL >= 2) {
        uint32_t b[8];
        leaf(1, b);
        b3::store_digest(blk + 32 * (q * BL + 1), b);
        b3::merge(a, b, a);
        b3::store_digest(blk + 32 * (Q * BL + q * (BL / 2)), a);
        if constexpr (BL == 4) {
            uint32_t c[8], d[8];
            leaf(2, c);
            b3::store_digest(blk + 32 * (q * 4 + 2), c);
            leaf(3, d);
            b3::store_digest(blk + 32 * (q * 4 + 3), d);
            b3::merge(c, d, c);
            b3::store_digest(blk + 32 * (Q * 4 + q * 2 + 1), c);
            b3::merge(a, c, a);
            b3::store_digest(blk + 32 * (Q * 6 + q), a);
        }
    }
    b3::store_digest(send_slot, a);
}

// LDE rows (column c, local coset j at base[(c*Bl + j)*n + q]; Q = n groups): piece k of K
template <int BL>
__global__ void __launch_bounds__(256) k_sh_hash_rows_blk(const fe *base, int ncols, int log_n, int log_QG, int log_K,
                                                          int k, uint8_t *blk, uint8_t *send) {
    const size_t n = (size_t)1 << log_n;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (n >> log_K)) return;
    const size_t q = blk_group(t, log_QG, log_K, k), cs = (size_t)BL * n;
    blk_levels<BL>(n, q, blk, send + 32 * t, [&](int j, uint32_t h[8]) {
        const fe *p = base + (size_t)j * n + q;
        b3::hash_elements(ncols, [&](int c) { return p[(size_t)c * cs]; }, h);
    });
}

// FRI layer-0 leaves (Q = m groups): leaf (j, q0) holds deep[j][q0 + k m], k < fold (KX planes at stride Bl n)
template <int BL, int KX>
__global__ void __launch_bounds__(256) k_sh_hash_fri0_blk(const fe *deep, int log_n, int fold, int log_m, int log_QG,
                                                          int log_K, int kp, uint8_t *blk, uint8_t *send) {
    const size_t n = (size_t)1 << log_n, m = (size_t)1 << log_m, cs = (size_t)BL * n;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (m >> log_K)) return;
    const size_t q = blk_group(t, log_QG, log_K, kp);
    blk_levels<BL>(m, q, blk, send + 32 * t, [&](int j, uint32_t h[8]) {
        const fe *p = deep + (size_t)j * n + q;
        if constexpr (KX == 1)
            b3::hash_elements(fold, [&](int e) { return p[(size_t)e << log_m]; }, h);
        else
            b3::hash_elements(2 * fold, [&](int e) { return p[(size_t)(e & 1) * cs + ((size_t)(e >> 1) << log_m)]; }, h);
    });
}

template <int BL>
static void launch_fri0_blk(hipStream_t st, int KX, const fe *deep, int log_n, int fold, int log_m, int log_QG,
                            int log_K, int k, uint8_t *blk, uint8_t *send) {
    const dim3 grid(cdiv(((size_t)1 << log_m) >> log_K, 256));
    if (KX == 1)
        hipLaunchKernelGGL((k_sh_hash_fri0_blk<BL, 1>), grid, dim3(256), 0, st, deep, log_n, fold, log_m, log_QG, log_K, k,
                           blk, send);
    else
        hipLaunchKernelGGL((k_sh_hash_fri0_blk<BL, 2>), grid, dim3(256), 0, st, deep, log_n, fold, log_m, log_QG, log_K, k,
                           blk, send);
}

// piece k's received block nodes [s][q''] (group q' = k QGK + q'' of source s is level-Lb node q' G + s of this rank's
// subtree) merged straight into their parents: level Lb + 1 node q' G/2 + j = merge(node q' G + 2j, node q' G + 2j + 1),
// into lvl1 (j fastest: the stores are contiguous, the loads 32-B runs of G/2 chunks)
__global__ void k_sh_blk_merge(const uint8_t *recv, int G, int log_QGK, int k, uint8_t *lvl1) {
    const int hg = G / 2, log_hg = G >= 4 ? (G >= 8 ? 2 : 1) : 0;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= ((size_t)hg << log_QGK)) return;
    const size_t j = t & (size_t)(hg - 1), qq = t >> log_hg;
    uint32_t l[8], r[8], h[8];
    const uint4 *a = reinterpret_cast<const uint4 *>(recv + 32 * (((2 * j) << log_QGK) + qq));
    const uint4 *c = reinterpret_cast<const uint4 *>(recv + 32 * (((2 * j + 1) << log_QGK) + qq));
    const uint4 a0 = a[0], a1 = a[1], c0 = c[0], c1 = c[1];
    l[0] = a0.x; l[1] = a0.y; l[2] = a0.z; l[3] = a0.w; l[4] = a1.x; l[5] = a1.y; l[6] = a1.z; l[7] = a1.w;
    r[0] = c0.x; r[1] = c0.y; r[2] = c0.z; r[3] = c0.w; r[4] = c1.x; r[5] = c1.y; r[6] = c1.z; r[7] = c1.w;
    b3::merge(l, r, h);
    b3::store_digest(lvl1 + 32 * ((((size_t)k << log_QGK) + qq) * hg + j), h);
}

// all-gathered chunks [s][j][q'] (source chunk s at item s * src_stride) -> natural order: item (s Bl + j) + 8 q' (local
// coset j of rank s is coset s Bl + j).  src_stride > Bl << log_mg when each source sent several planes.
__global__ void k_sh_permute(const uint8_t *recv, int G, int Bl, int log_mg, int esize, size_t src_stride,
                             uint8_t *out) {
    const size_t per = (size_t)Bl << log_mg;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= per * G) return;
    const size_t s = t / per, rem = t % per, j = rem >> log_mg, qp = rem & (((size_t)1 << log_mg) - 1);
    const size_t idx = (s * Bl + j) + 8 * qp;
    const uint4 *src = reinterpret_cast<const uint4 *>(recv + (s * src_stride + rem) * esize);
    uint4 *dst = reinterpret_cast<uint4 *>(out + idx * esize);
    for (int w = 0; w < esize / 16; w++) dst[w] = src[w];
}

// one coset's coefficient slices (KX planes at plane_stride) for its all-to-all: send[d][plane][k'] = c[plane][d*kg + k']
__global__ void k_sh_pack_coset(const fe *c, size_t plane_stride, int log_n, int KX, int log_kg, fe *send) {
    const size_t n = (size_t)1 << log_n;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)KX * n) return;
    const size_t pln = t >> log_n, k = t & (n - 1);
    send[((((k >> log_kg) * KX) + pln) << log_kg) + (k & (((size_t)1 << log_kg) - 1))] = c[pln * plane_stride + k];
}

// first FRI fold over the local cosets: row r' = r + 8*q0 (values deep[j][q0 + k*m]) -> out[j*m + q0], as the
// single-GPU fold (kernels.hip k_fri_fold: idft_small per component plane, then Horner at beta = alpha / x_r').
// E buffers are planar with plane stride Bl*n (DEEP) / Bl*m (fold).
template <int KX, int F>
__global__ void __launch_bounds__(256) k_sh_fri_fold0(const fe *deep, int log_n, int Bl, int g, int log_m,
                                                      const FoldConsts<KX> *Fc, const fe *wi_lo, const fe *wi_hi,
                                                      size_t wstride, fe *out) {
    typedef Chal<KX> X;
    typedef typename X::T T;
    const size_t n = (size_t)1 << log_n, m = (size_t)1 << log_m, cs = (size_t)Bl * n, om = (size_t)Bl * m;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= om) return;
    const size_t j = t >> log_m, q0 = t & (m - 1);
    const size_t rp = (size_t)(g * Bl + (int)j) + 8 * q0;  // row index in the layer (1/x_r: w_N^-(rp wstride))
    const size_t wi = rp * wstride;
    fe va[F], vb[KX == 2 ? F : 1];  // the component planes
#pragma unroll
    for (int k = 0; k < F; k++) {
        va[k] = deep[j * n + q0 + ((size_t)k << log_m)];
        if constexpr (KX == 2) vb[k] = deep[cs + j * n + q0 + ((size_t)k << log_m)];
    }
    const T beta = X::mulb(Fc->alpha, fe_mul(Fc->inv_offset, fe_mul(wi_lo[wi & 2047], wi_hi[wi >> 11])));
    idft_small<F>(va, Fc->zinv);
    if constexpr (KX == 2) idft_small<F>(vb, Fc->zinv);
    auto V = [&](int mm) -> T {
        if constexpr (KX == 2) return fe2{va[mm], vb[mm]};
        else return va[mm];
    };
    T acc = V(F - 1);
#pragma unroll
    for (int mm = F - 2; mm >= 0; mm--) acc = X::add(X::mul(acc, beta), V(mm));
    X::st(out + t, om, X::mulb(acc, Fc->inv_fold));
}

// a fold over the local cosets (layer 0, or layer 1 with wstride = fold) for fold 2 / 4 / 8 / 16 (KX planes)
static void sh_fri_fold0(hipStream_t st, int KX, int fold, const fe *deep, int log_n, int Bl, int g, int log_m,
                         const void *consts, const fe *wi_lo, const fe *wi_hi, size_t wstride, fe *out) {
    const dim3 grid(cdiv((size_t)Bl << log_m, 256));
    with_kx(KX, [&](auto kx) {
        constexpr int K = decltype(kx)::value;
#define ZK_SH_FOLD(FF)                                                                               \
    hipLaunchKernelGGL((k_sh_fri_fold0<K, FF>), grid, dim3(256), 0, st, deep, log_n, Bl, g, log_m, \
                       (const FoldConsts<K> *)consts, wi_lo, wi_hi, wstride, out)
        switch (fold) {
            case 2: ZK_SH_FOLD(2); break;
            case 4: ZK_SH_FOLD(4); break;
            case 8: ZK_SH_FOLD(8); break;
            default: ZK_SH_FOLD(16); break;
        }
#undef ZK_SH_FOLD
        return 0;
    });
}

// the suffix carried into rank `rank`'s DEEP range: out[c] = sum over later ranks h of all[h * nc + c]
__global__ void k_sh_suffix_carry(const fe *all, int G, int rank, int nc, fe *out) {
    const int c = threadIdx.x;
    if (c >= nc) return;
    fe s = fe_zero();
    for (int h = rank + 1; h < G; h++) s = fe_add(s, all[(size_t)h * nc + c]);
    out[c] = s;
}

// ---------------------------------------------------------------- a Merkle tree split over G ranks
// the geometry (which rank and buffer holds a node) is shard_plan.hpp's TreeGeom; here the buffers themselves
struct DistTree : TreeGeom {
    std::vector<uint8_t *> blk, nodes;               // per local rank: block levels, subtree heap
    explicit DistTree(int nlocal) : blk(nlocal), nodes(nlocal) {}
    std::vector<std::array<uint8_t, 32>> top;        // heap nodes 1 .. 2G-1
    uint8_t root[32];
};

struct Ctx {
    zk_comm *comm;
    std::vector<zk_prover *> P;
    std::vector<int> rank;  // rank of each local prover
    std::vector<Plan *> pl;
    int G, Bl, log_n, C;
    size_t n;
    // zk_vm_prove_sharded: the preprocessed columns of each local rank (its own cosets), or null: the device trace
    // then holds only the dynamic stack columns 12 .. 12 + md - 1
    const FixedCols *fixed = nullptr;
    // host traces: the previous proof's column hints may be used (hint_ok); whether this proof derives the clock
    // (sh_clock), and the hinted columns the ranks' checks refuted (sh_refuted, bit c: prove_sharded returned
    // ZK_SH_REDO, and prove_sharded_entry proves again without hints)
    bool hint_ok = true, sh_clock = false;
    uint32_t sh_refuted = 0;
    // what the ranks agreed on before the proof (shard_agree.hpp; prove_sharded_entry): every rank detects the sparse
    // columns / may derive the clock, and the hint set every rank uses for a host trace (none unless all sets were equal)
    bool detect = false, clock = false;
    HintSet hints;
    bool lead_seg = false;  // the schedule segment being enqueued runs on the lead rank only (lead_segment)
};
constexpr int ZK_SH_REDO = 1000;  // (internal) a refuted column hint voided the proof on every rank

// every local rank in turn, its device current: f(l, p, pl) -> status
template <typename F>
int each_rank(Ctx &X, F f) {
    for (int l = 0; l < (int)X.P.size(); l++) {
        ZK_CHECK_HIP(hipSetDevice(X.P[l]->device));
        ZK_TRY(f(l, X.P[l], X.pl[l]));
    }
    return ZK_OK;
}
// the send and receive pointers of one exchange, per local rank
struct Bufs {
    std::vector<const void *> snd;
    std::vector<void *> rcv;
    explicit Bufs(const Ctx &X) : snd(X.P.size()), rcv(X.P.size()) {}
    void set(int l, const void *s, void *r) { snd[l] = s, rcv[l] = r; }
};
// f(integral_constant<int, Bl>): the template instance of a rank's Bl = 4, 2 or 1 cosets
template <typename F>
void with_bl(int Bl, F f) {
    if (Bl == 4) f(std::integral_constant<int, 4>{});
    else if (Bl == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}


// ---------------------------------------------------------------- exchanges, overlapped with compute (round 6)
// xchg_start issues a collective on the exchange stream of local rank 0 (its own stream per process: RCCL, host
// transport; every rank's copies for the loopback), ordered after everything already enqueued on every local rank's
// compute stream (an event per rank), and records its completion; xchg_wait makes every local compute stream wait
// for that completion -- a device-side wait, enqueued after the completion was recorded, so it never parks a
// queue on an event not yet recorded.  Between the two the compute streams run whatever does not read the received
// data or write the sent data (the callers keep to that).  xchg = start + wait.  Timing: events around the collective
// on its stream (total) and around the wait on rank 0's compute stream (exposed), and the schedule log
// (zk_prover_shard_schedule) of every start, wait and segment boundary.
// Measurement mode (zk_comm_set_measure, loopback): every rank's compute and the copies share rank 0's stream.
enum XOp { A2A, AG };
struct XH {
    int idx = -1;
};
static int pool_events(zk_prover *p, size_t k, size_t *first) {
    while (p->xchg_pool.size() < p->xchg_next + k) {
        hipEvent_t ev;
        ZK_CHECK_HIP(hipEventCreate(&ev));
        p->xchg_pool.push_back(ev);
    }
    *first = p->xchg_next;
    p->xchg_next += k;
    return ZK_OK;
}
static int exchange_stream(zk_prover *p, hipStream_t *out) {
    if (!p->cst) {
        // the highest priority the device offers: an RCCL collective's workgroups are dispatched ahead of the queued
        // workgroups of the compute stream's long launches instead of behind them
        int least = 0, greatest = 0;
        ZK_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        ZK_CHECK_HIP(hipStreamCreateWithPriority(&p->cst, hipStreamNonBlocking, greatest));
    }
    if (!p->ev_ready) ZK_CHECK_HIP(hipEventCreateWithFlags(&p->ev_ready, hipEventDisableTiming));
    *out = p->cst;
    return ZK_OK;
}
// a schedule entry on local rank 0's compute stream: kind 'S' / 'W' (exchange x) or 'K' (segment boundary);
// `lead`: the segment ending here ran on the lead rank only
static int sched_entry(Ctx &X, char kind, int x, bool post_now = true) {
    zk_prover *p = X.P[0];
    size_t e;
    ZK_TRY(pool_events(p, 2, &e));
    ZK_CHECK_HIP(hipEventRecord(p->xchg_pool[e], p->st));
    if (post_now) ZK_CHECK_HIP(hipEventRecord(p->xchg_pool[e + 1], p->st));
    p->sched.push_back({kind, x, e, e + 1, X.lead_seg});
    X.lead_seg = false;
    return ZK_OK;
}
// the segment starting here runs on the lead rank only (until the next entry)
static int lead_segment(Ctx &X) {
    ZK_TRY(sched_entry(X, 'K', -1));
    X.lead_seg = true;
    return ZK_OK;
}
int xchg_start(Ctx &X, const char *name, XOp op, const Bufs &b, size_t bytes, XH *h) {
    zk_prover *p0 = X.P[0];
    ZK_CHECK_HIP(hipSetDevice(p0->device));
    size_t e;
    ZK_TRY(pool_events(p0, 4, &e));
    const int x = (int)p0->xchg.size();
    p0->xchg.push_back({name, (double)bytes * (X.G - 1), e, op == A2A ? 0 : 1, false});
    hipStream_t is;
    if (X.comm->measure) {
        is = p0->st;  // every rank's stream is this one (prove_sharded_entry): program order, no overlap
        ZK_TRY(sched_entry(X, 'S', x, false));
    } else {
        ZK_TRY(exchange_stream(p0, &is));
        ZK_TRY(sched_entry(X, 'S', x));
        for (zk_prover *p : X.P) {
            ZK_CHECK_HIP(hipSetDevice(p->device));
            if (!p->ev_ready) ZK_CHECK_HIP(hipEventCreateWithFlags(&p->ev_ready, hipEventDisableTiming));
            ZK_CHECK_HIP(hipEventRecord(p->ev_ready, p->st));
            ZK_CHECK_HIP(hipStreamWaitEvent(is, p->ev_ready, 0));  // (captured now: the event may be recorded again)
        }
        ZK_CHECK_HIP(hipSetDevice(p0->device));
    }
    ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[e], is));
    ZK_TRY(op == A2A ? X.comm->all_to_all(X.P, b.snd, b.rcv, bytes, is) : X.comm->all_gather(X.P, b.snd, b.rcv, bytes, is));
    ZK_CHECK_HIP(hipSetDevice(p0->device));
    ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[e + 1], is));
    if (X.comm->measure) ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[p0->sched.back().post], p0->st));
    h->idx = x;
    return ZK_OK;
}
int xchg_wait(Ctx &X, XH &h) {
    if (h.idx < 0) return ZK_OK;
    zk_prover *p0 = X.P[0];
    auto &r = p0->xchg[h.idx];
    const int x = h.idx;
    h.idx = -1;
    if (r.waited) return ZK_OK;
    r.waited = true;
    ZK_CHECK_HIP(hipSetDevice(p0->device));
    ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[r.ev + 2], p0->st));
    ZK_TRY(sched_entry(X, 'W', x, false));
    if (!X.comm->measure)
        for (zk_prover *p : X.P) {
            ZK_CHECK_HIP(hipSetDevice(p->device));
            ZK_CHECK_HIP(hipStreamWaitEvent(p->st, p0->xchg_pool[r.ev + 1], 0));
        }
    ZK_CHECK_HIP(hipSetDevice(p0->device));
    ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[r.ev + 3], p0->st));
    ZK_CHECK_HIP(hipEventRecord(p0->xchg_pool[p0->sched.back().post], p0->st));
    return ZK_OK;
}
int xchg(Ctx &X, const char *name, XOp op, const Bufs &b, size_t bytes) {
    XH h;
    ZK_TRY(xchg_start(X, name, op, b, bytes, &h));
    return xchg_wait(X, h);
}

// the block levels (the hash kernel: leaves, their subtree up to Lb into T.blk, block nodes into the send scratch in
// piece order), all-to-all of the block nodes, merged on arrival into level Lb + 1 of the subtree T.nodes, the subtree,
// roots.  The block nodes go out in K pieces: piece k's all-to-all runs on the exchange stream while piece k + 1 is
// hashed.  hash(l, send, log_QG, log_K, k) launches piece k of local rank l.  `rows`: the leaves are LDE rows (7 or 2
// BLAKE3 blocks each), whose hashing the pieces hide; the FRI trees' leaves hash in a fraction of that and go in one
// piece.  The scratch is fri_dig: the send pieces, and from 32 Q the receive pieces.
template <typename HashFn>
int dist_commit(Ctx &X, DistTree &T, size_t M, HashFn hash, const char *digests_name, const char *roots_name,
                bool rows = true) {
    const int nl = (int)X.P.size();
    T.shape(M, X.G);
    const size_t Q = T.Q, QG = Q / X.G;  // groups per destination rank
    const int log_QG = ilog2(QG);
    // pieces only where the transfer outweighs the latency of three more collectives: >= 1 MiB per destination and
    // piece (the trace and composition trees at 2^20 and up; small FRI trees go in one piece)
    const int log_K = rows && QG >= ((size_t)1 << 17) ? 2 : 0, K = 1 << log_K;
    const int log_QGK = log_QG - log_K;
    const size_t piece = 32 * (size_t)X.G << log_QGK;  // bytes of one piece (all destinations)
    std::vector<XH> h(K);
    Bufs b(X);
    for (int k = 0; k < K; k++) {
        for (int l = 0; l < nl; l++) {
            ZK_CHECK_HIP(hipSetDevice(X.P[l]->device));
            uint8_t *scratch = X.P[l]->fri_dig;
            hash(l, scratch + k * piece, log_QG, log_K, k);
            b.set(l, scratch + k * piece, scratch + 32 * Q + k * piece);
        }
        ZK_TRY(xchg_start(X, digests_name, A2A, b, (size_t)32 << log_QGK, &h[k]));
    }
    for (int k = 0; k < K; k++) {
        ZK_TRY(xchg_wait(X, h[k]));
        for (int l = 0; l < nl; l++) {
            zk_prover *p = X.P[l];
            ZK_CHECK_HIP(hipSetDevice(p->device));
            hipLaunchKernelGGL(k_sh_blk_merge, dim3(cdiv(Q / K / 2, 256)), dim3(256), 0, p->st,
                               (const uint8_t *)p->fri_dig + 32 * Q + k * piece, X.G, log_QGK, k, T.nodes[l] + 32 * (Q / 2));
        }
    }
    for (int l = 0; l < nl; l++) {
        zk_prover *p = X.P[l];
        ZK_CHECK_HIP(hipSetDevice(p->device));
        merkle_tree(p->st, T.nodes[l] + 32 * (Q / 2), Q / 2, T.nodes[l]);  // (Q >= G >= 2; Q = 2: the one leaf is nodes[1])
        b.set(l, T.nodes[l] + 32, p->sh_roots);
    }
    ZK_TRY(xchg(X, roots_name, AG, b, 32));
    std::vector<uint8_t> roots(32 * X.G);
    ZK_TRY(d2h_small(X.P[0], roots.data(), X.P[0]->sh_roots, roots.size()));
    ZK_TRY(d2h_flush(X.P[0]));
    T.top.assign(2 * X.G, {});
    for (int d = 0; d < X.G; d++) memcpy(T.top[X.G + d].data(), &roots[32 * d], 32);
    for (int k = X.G - 1; k >= 1; k--) {
        uint8_t buf[64];
        memcpy(buf, T.top[2 * k].data(), 32);
        memcpy(buf + 32, T.top[2 * k + 1].data(), 32);
        b3::hash_bytes(buf, 64, T.top[k].data());
    }
    memcpy(T.root, T.top[1].data(), 32);
    return ZK_OK;
}

// ---------------------------------------------------------------- one sharded proof
// The per-proof state, and the protocol's stages as methods that prove_sharded calls in order.  The stages read a
// rank's stream (p->st) where they use it: the measurement mode swaps the ranks' streams around the proof.
// Buffers borrowed along the way (COMP .. FRI: the base-field buffer, or its two-plane E counterpart: planes()):
//   comp, ctmp   alternate as the staging of the trace rounds that are not gathered in place (stage_of), until S3
//   clde         holds a host trace's packed narrow columns during S2 (expanded into d_trace before they are read)
//   fri_dig      the all-to-all scratch of all four commitments (dist_commit), then the lead's FRI layer digests
//   tmp          the NTT scratch; in S3 / S4 also the slice send areas (coset j at KX n (1 + j)); from S6 to the
//                openings the FRI-0 subtree heap at tmp and the FRI-1 one 32 m bytes after it
//   COMP         beyond its KX Bl n evaluations: the receive area of the coefficient slices (S3, S4); S6: layer 2 of a
//                sharded layer 1, or the staging of a gathered layer 1 / remainder layer
//   CTMP         S6: layer 1 over this rank's cosets, which the openings read
//   sh_buf       the receive area of every small all-gather (flags, totals, OOD parts) and of the openings
struct ShardedProof : ProofRun {  // (ProofRun: the state and stages shared with the single-GPU proof; N = 8 n)
    Ctx &X;
    const uint8_t *const trace;  // the caller's host trace, or null: the trace is in every rank's HBM
    // (FieldExtension::Quadratic: every E-valued buffer planar, plane stride Bl*n per rank)
    const int G = X.G, Bl = X.Bl, log_n = X.log_n, nlp = (int)X.P.size();
    const size_t col = n * sizeof(fe), kg = n / G;  // kg: a rank's coefficient range
    const size_t m = n / fold, m1 = m / fold, rows0 = N / fold;  // layer-0 / -1 positions per coset, layer-0 leaves
    const int log_m = ilog2(m);
    const fe g = h_root_of_unity(log_n), inv_n = h_inv(fe_make(n));
    // OOD sums, assertion quotient and DEEP are split by coefficient range (n / G per rank, whole phase-3 chunks);
    // traces too short for whole ranges keep the per-row assertion terms and the replicated DEEP
    const bool range_split = kg % ZK_DEEP_RANGE_QUANTUM == 0;
    zk_prover *const P0 = X.P[0];

    Latch checked, packed;  // host checks of the hinted columns, packing of the narrow ones
    std::vector<std::atomic<uint32_t>> bad = std::vector<std::atomic<uint32_t>>(nlp);  // (value-initialised: zero)
    std::vector<std::atomic<uint32_t>> pack_bad = std::vector<std::atomic<uint32_t>>(nlp);

    Bufs xb{X};  // the send / receive pointers of the exchange being issued
    // column classes
    int U[W], nU = 0;   // the columns interpolated, ascending
    uint32_t S = 0;     // sparse columns (zero but the last row): coefficients and LDE from the last row
    bool clk = false;   // the AIR clock (column 0 = 0 .. n-2 but the last row): from the identity column's tables
    fe lastv[W];        // the last row (host trace, device trace: read back with the flags)
    std::vector<SparseCols> spc = std::vector<SparseCols>(nlp);
    std::vector<const SparseCols *> spp = std::vector<const SparseCols *>(nlp, nullptr);
    std::vector<NarrowCols> nar = std::vector<NarrowCols>(nlp);
    std::vector<uint32_t> went_packed = std::vector<uint32_t>(nlp, 0u);
    // the trace rounds
    int rep = 0;  // U[0 .. rep) are interpolated by every rank itself
    ShardRounds rp;
    std::vector<XH> hr;
    // commitments, constraint and composition state
    DistTree Ttrace{nlp}, Tcomp{nlp}, Tfri0{nlp}, Tfri1{nlp};
    AirConsts K, Kp[2];
    std::vector<XH> hs, hc;  // the coefficient slices' all-to-alls (per local coset), the columns' all-gathers
    XH hdeg;                 // the degree flags' all-gather (read once the composition is committed)
    std::vector<const fe *> Dk = std::vector<const fe *>(nlp);  // each rank's DEEP coefficients
    // FRI: layer 1 committed and folded on every rank (sh1) and then layer lg = 2 all-gathered, else layer lg = 1; the
    // gathered layer's storage: natural (lbg 0) or coset-major over 8 cosets (3; FriLayout)
    int lg = 1, lbg = 0;
    bool sh1 = false;
    // openings: chunk requests -- owner rank (-1: host top node), local buffer id, byte offset
    enum { B_LDE, B_CLDE, B_DEEP, B_TN, B_CN, B_F0N, B_FRI, B_FRI_DIG, B_TB, B_CB, B_F0B, B_CT, B_F1N, B_F1B };
    struct Req {
        int owner, buf;
        size_t off;
        const uint8_t *host;
    };
    // (the request list, like the openings and their plans, keeps its storage across proofs: this host work sits on
    // every rank's critical path, in the lead rank's segment, where fresh allocations cost page faults)
    inline static thread_local std::vector<Req> req;
    ShardedProof(Ctx &X_, const uint8_t *trace_, const zk_options *opt_, const zk_pub_inputs *pub_)
        : ProofRun(opt_, pub_, X_.n, X_.C), X(X_), trace(trace_) {}
    using ProofRun::finish;  // (S9, beside a trace round's finish(k))
    // Every way out: first the host tasks are waited for (they read the caller's trace and write bad / pack_bad); then,
    // only when a host trace was given, the upload, compute and exchange streams are drained: on an early error return
    // copies from the trace may still be in flight, and the caller may free it as soon as prove_sharded returns.  The
    // body runs before any member is destroyed, so the order does not hang on how the members are declared.
    ~ShardedProof() {
        checked.wait();
        packed.wait();
        for (zk_prover *p : X.P) {
            if (!trace) break;
            (void)hipSetDevice(p->device);
            upload_drain(p);
            // (and the kernels of a failed proof: the next proof's uploads into d_trace must not overtake them)
            (void)hipStreamSynchronize(p->st);
            if (p->cst) (void)hipStreamSynchronize(p->cst);
        }
    }
    Planes pb(const zk_prover *p) const { return planes(p, KX); }
    using SR = std::pair<const void *, void *>;
    template <typename F>
    const Bufs &bufs(F f) {  // xb filled with f(l, p) -> SR per local rank
        for (int l = 0; l < nlp; l++) {
            const SR x = f(l, X.P[l]);
            xb.set(l, x.first, x.second);
        }
        return xb;
    }

    int start() {
        for (zk_prover *p : X.P) ZK_TRY(io_rewind(p));  // the pinned staging areas start over
        stage_mark(P0, "start");  // (stage_begin: prove_sharded_entry, before the control exchange it lists)
        coin = seed_coin(n, opt, pub);
        return ZK_OK;
    }

    // ---- S2: the trace polynomials on every rank, then the local coset LDE and the distributed commitment.  Every
    // trace source splits the interpolation by column, round robin: in round k rank g interpolates column U[g + G k] and
    // an all-gather (in place when the round's columns are consecutive) fills the round's G columns on every rank, after
    // which every rank extends them over its cosets.  Round k's all-gather runs on the exchange stream while the
    // compute stream interpolates round k + 1 and extends round k - 1 (xchg_start / xchg_wait), so each rank computes
    // 1/G of the coefficients and the exchange hides under the coset LDEs.  U (the columns transformed) leaves out
    // what every rank forms from the last row alone (sparse columns, the AIR clock) or from per-program tables:
    //  * host trace: rank g uploads (copy stream) only its own columns, so each rank moves 1/G of the trace over PCIe;
    //    the previous sharded proof's column hints (sparse, clock, narrow) as the single-GPU host path (section 6c);
    //  * trace already in every rank's HBM (trace = NULL): each rank detects the sparse columns and the clock over its
    //    1/G of the rows, the flags are all-gathered (round 6: the interpolation was replicated before, 4.0 ms of
    //    every rank's time at 2^22);
    //  * zk_vm_prove_sharded: only the dynamic stack columns; the program-only columns from the preprocessed tables.
    void columns_left() {  // U: every column but the sparse ones and the derived clock
        for (int c = 0; c < W; c++)
            if (!((S >> c) & 1u) && !(clk && c == 0)) U[nU++] = c;
    }
    // Host trace.  Column classes (round 4, as the single-GPU host path): the sparse columns (zero but the last row) and
    // the AIR clock (rows 0 .. n-2 = 0 .. n-2) that the previous sharded proof of this length, world and program found
    // -- the same hints on every rank, learned from all-gathered flags -- are neither uploaded, interpolated nor
    // all-gathered: every rank forms their coefficients and local LDE from the last row (fills).  Each rank's host
    // threads check its 1/G row range of them; the flags are all-gathered with the hints of the next proof, and a
    // refuted hint voids the proof on every rank (prove_sharded_entry redoes it without hints).
    int classify_host() {
        // the hint set the ranks agreed on (local_hints on every rank, equal on all of them, else none), unless this is
        // the pass that redoes a proof whose hints were refuted
        const HintSet hs = X.hint_ok && X.detect ? X.hints : HintSet{};
        S = hs.S;
        clk = hs.clk != 0;
        X.sh_clock = clk;
        const uint32_t N8 = hs.N8, N32 = hs.N32;
        for (zk_prover *p : X.P) {  // (zk_prover_proof_info: what this proof took from its hints)
            p->tc.sp_hinted = S;
            p->tc.clk_used = clk;
        }
        columns_left();
        static_assert((W + 1) / 2 <= ZK_UPLOAD_GROUPS_MAX, "one upload event per round at G = 2");
        for (int c = 0; c < W; c++) memcpy(&lastv[c], trace + (size_t)c * col + (n - 1) * sizeof(fe), sizeof(fe));
        ZK_TRY(each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
            ZK_TRY(sparse_begin(p, pl, &spc[l], &spp[l]));  // the flags the interpolation's pass 1 sets
            if (!X.detect) spp[l] = nullptr;                // (agreed: a rank that cannot detect turns it off for all)
            if (spp[l]) spc[l].wstride = W;
            if (clk) ZK_TRY(clock_tables(p, pl));
            return ZK_OK;
        }));
        check_derived();
        return pack_narrow(N8, N32);
    }
    static constexpr size_t TASK_ROWS = (size_t)1 << 18;  // rows per host task
    void check_derived() {  // each local rank's row range of the hinted sparse columns and the clock
        for (int c = 0; c < W; c++) {
            const bool sparse = (S >> c) & 1u, clock = clk && c == 0;
            if (!sparse && !clock) continue;
            const uint8_t *cp = trace + (size_t)c * col;
            for (int l = 0; l < nlp; l++) {
                const size_t r0 = n * (size_t)X.rank[l] / (size_t)G, r1 = std::min(n - 1, n * (size_t)(X.rank[l] + 1) / G);
                std::atomic<uint32_t> *b = &bad[l];
                row_tasks(checked, c, r0, r1, TASK_ROWS, [=](int cc, size_t a, size_t e) {
                    if (!(clock ? clock_rows(cp, a, e) : zero_rows(cp, a, e))) b->fetch_or(1u << cc);
                });
            }
        }
    }
    // narrow columns (8- or 32-bit before the last row): their owner's host threads pack rows 0 .. n-2 into its pinned
    // staging while the other columns go up; a column goes up packed (expanded on the device), or whole if a value does
    // not fit
    int pack_narrow(uint32_t N8, uint32_t N32) {
        for (int l = 0; l < nlp; l++) {
            NarrowCols &nc = nar[l];
            nc.count = 0;
            size_t bytes = 0;
            for (int i = X.rank[l]; i < nU; i += G) {
                const int c = U[i];
                if (!(((N8 | N32) >> c) & 1u)) continue;
                nc.col[nc.count] = c;
                nc.width[nc.count] = ((N8 >> c) & 1u) ? 1 : 4;
                nc.off[nc.count] = bytes;
                nc.last[nc.count] = lastv[c];
                bytes += ((size_t)nc.width[nc.count] * n + 15) & ~(size_t)15;
                nc.count++;
            }
            ZK_TRY(ensure_pack(X.P[l], bytes));
        }
        for (int l = 0; l < nlp; l++)
            for (int k = 0; k < nar[l].count; k++) {
                const uint8_t *cp = trace + (size_t)nar[l].col[k] * col;
                uint8_t *dst = X.P[l]->h_pack + nar[l].off[k];
                const int width = nar[l].width[k];
                const size_t rows = n;
                std::atomic<uint32_t> *b = &pack_bad[l];
                row_tasks(packed, nar[l].col[k], 0, n - 1, TASK_ROWS, [=](int c, size_t r0, size_t r1) {
                    if (!pack_rows(cp, r0, r1, width, dst)) b->fetch_or(1u << c);
                    if (r1 == rows - 1) memset(dst + (size_t)width * (rows - 1), 0, width);  // (the last row's slot)
                });
            }
        return ZK_OK;
    }
    // vm::prove: the dynamic stack columns only (12 .. 12 + md - 1); the program-only columns and the zero registers
    // from the per-program preprocessed columns of this rank's cosets (one streaming pass, after the rounds)
    void classify_fixed() {
        for (int c = 12; c < 12 + X.fixed[0].md; c++) U[nU++] = c;
    }
    // every rank's column flags (sp_nz: 4 W words each) all-gathered, read back (with the last row if asked) and OR-ed
    int gather_flags(unsigned (&nz)[4 * W], bool with_last) {
        ZK_TRY(xchg(X, "column_flags", AG, bufs([](int, zk_prover *p) { return SR{p->sp_nz, p->sh_buf}; }),
                    4 * W * sizeof(unsigned)));
        std::vector<unsigned> f((size_t)G * 4 * W);
        ZK_CHECK_HIP(hipSetDevice(P0->device));
        ZK_TRY(d2h_small(P0, f.data(), P0->sh_buf, f.size() * sizeof(unsigned)));
        if (with_last) ZK_TRY(d2h_small(P0, lastv, P0->sp_last, sizeof lastv));
        ZK_TRY(d2h_flush(P0));
        memset(nz, 0, sizeof nz);
        for (int r = 0; r < G; r++)
            for (int c = 0; c < 4 * W; c++) nz[c] |= f[(size_t)r * 4 * W + c];
        return ZK_OK;
    }
    // every rank holds the whole trace: each detects the sparse columns and the clock over its 1/G of the rows (whole
    // 4096-row blocks; shorter traces: every row), the flags are all-gathered and OR-ed, and every rank reads them back
    // with the last row (one host round trip) to plan the rounds
    int classify_device() {
        ZK_TRY(each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
            ZK_TRY(sparse_begin(p, pl, &spc[l], &spp[l]));
            if (!X.detect) spp[l] = nullptr;
            if (!spp[l]) return ZK_OK;
            const size_t rr = n / (size_t)G;
            const bool row_split = rr % 4096 == 0;
            const size_t r0 = row_split ? rr * (size_t)X.rank[l] : 0, r1 = row_split ? r0 + rr : n;
            sparse_detect_rows(p->st, p->d_trace, n, 0, W, spc[l], r0, r1);
            return ZK_OK;
        }));
        if (X.detect) {  // every rank of the proof detects (agreed: the all-gather is issued by all ranks or by none)
            unsigned nz[4 * W];
            ZK_TRY(gather_flags(nz, true));
            for (int c = 0; c < W; c++)
                if (nz[c] == 0) S |= 1u << c;
            clk = X.clock && !(S & 1u) && nz[3 * W] == 0 && spc[0].id_poly;
        }
        columns_left();
        if (clk)
            for (int l = 0; l < nlp; l++) ZK_TRY(clock_tables(X.P[l], X.pl[l]));
        return ZK_OK;
    }

    int narrow_of(int l, int c) const {  // the narrow column k of local rank l, or -1
        for (int k = 0; k < nar[l].count; k++)
            if (nar[l].col[k] == c) return k;
        return -1;
    }
    int upload(int k) {  // host trace: round k's column of every local rank onto its copy stream
        return each_rank(X, [this, k](int l, zk_prover *p, Plan *) -> int {
            const int c = rp.column(k, X.rank[l]), q = c >= 0 ? narrow_of(l, c) : -1;
            if (q >= 0) packed.wait();  // (before the lock: the packing does not need it)
            std::lock_guard<std::mutex> lk(*p->up_mu);
            UploadEvent rec{p->ev_up[k], p->up};  // recorded on the error path too (the destructor drains it)
            if (q >= 0 && !((pack_bad[l].load() >> c) & 1u)) {
                const size_t w = (size_t)nar[l].width[q] * n;
                ZK_CHECK_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(pb(p).clde) + nar[l].off[q],
                                            p->h_pack + nar[l].off[q], w, hipMemcpyHostToDevice, p->up));
                went_packed[l] |= 1u << c;
            } else if (c >= 0) {
                ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace + (size_t)c * n, trace + (size_t)c * col, col,
                                            hipMemcpyHostToDevice, p->up));
            }
            return rec.record();
        });
    }
    // a round whose columns are not consecutive is gathered into a staging area, alternating between two buffers
    // free until S3 / S4, so round k + 1's all-gather never overwrites what round k's copy-out still reads
    static fe *stage_of(zk_prover *p, int k) { return (k & 1) ? p->comp : p->ctmp; }
    void expand_packed(int l, zk_prover *p, int c) {  // rank l's narrow column c, which went up packed
        const int q = narrow_of(l, c);
        NarrowCols one{};
        one.count = 1;
        one.col[0] = c;
        one.width[0] = nar[l].width[q];
        one.off[0] = nar[l].off[q];
        one.last[0] = nar[l].last[q];
        expand_narrow(p->st, reinterpret_cast<const uint8_t *>(pb(p).clde), one, n, p->d_trace);
    }
    int issue(int k) {  // interpolate this rank's column of round k, start the round's all-gather
        if (trace && k + 1 < rp.rounds) ZK_TRY(upload(k + 1));
        ZK_TRY(each_rank(X, [this, k](int l, zk_prover *p, Plan *pl) -> int {
            const int c = rp.column(k, X.rank[l]), first = rp.first(k);
            if (trace) {
                // (a device-side wait: a sharded rank's process holds one prover, so its compute, exchange and upload
                // streams have hardware queues of their own and the host never blocks on the link)
                ZK_CHECK_HIP(hipStreamWaitEvent(p->st, p->ev_up[k], 0));
                if (c >= 0 && ((went_packed[l] >> c) & 1u)) expand_packed(l, p, c);
            }
            if (c >= 0) {
                SparseCols sc = spc[l];
                sc.col0 = c;
                sc.fused = true;
                ntt(p->st, pl->Tn, p->d_trace + (size_t)c * n, n, p->polys + (size_t)c * n, n, 1, true, nullptr, &inv_n,
                    p->tmp, trace && spp[l] ? &sc : nullptr);
            }
            // in place: the padding chunks of a short last round land on columns nobody interpolates -- filled after
            // the rounds -- or past W (shard_plan.hpp)
            const bool inplace = rp.inplace(k);
            xb.set(l, p->polys + (size_t)(inplace ? first + X.rank[l] : c >= 0 ? c : 0) * n,
                   inplace ? p->polys + (size_t)first * n : stage_of(p, k));
            return ZK_OK;
        }));
        return xchg_start(X, "trace_coeffs", AG, xb, col, &hr[k]);
    }
    int finish(int k) {  // wait for round k's coefficients, extend them over the local cosets
        ZK_TRY(xchg_wait(X, hr[k]));
        return each_rank(X, [this, k](int l, zk_prover *p, Plan *pl) -> int {
            const int real = rp.real(k), *cols = rp.US + G * k;
            if (!rp.inplace(k))
                for (int r = 0; r < real; r++)
                    if (r != X.rank[l])
                        ZK_CHECK_HIP(hipMemcpyAsync(p->polys + (size_t)cols[r] * n, stage_of(p, k) + (size_t)r * n, col,
                                                    hipMemcpyDeviceToDevice, p->st));
            return for_runs(cols, real, [this, l, p, pl](int c0, int k2) {
                ntt_lde(p->st, pl->Tn, pl->ct, p->polys + (size_t)c0 * n, n, k2, X.rank[l] * Bl, 1, Bl,
                        p->lde + (size_t)c0 * Bl * n, (size_t)Bl * n, n, p->tmp);
                return ZK_OK;
            });
        });
    }
    int trace_rounds() {
        // device-resident traces: the first `rep` columns of U are interpolated by every rank itself (no exchange),
        // right after rounds 0 and 1's all-gathers start, so they fill the time those take; the rest go round robin.  A
        // host trace splits every column: replicating one would make every rank upload it.
        // From the replayed schedules of 2^22 proofs (profiles/r06zc_split_sweep_2p22.json): with
        // two rounds in flight four columns hide rounds 0 and 1 at every world size (at G = 2 replicating every column,
        // the one-round-in-flight optimum, is 1.1 ms slower)
        if (!trace) rep = std::min(nU, X.comm->split_rep >= 0 ? X.comm->split_rep : 4);
        rp = shard_round_plan(U, nU, G, rep);
        const int rounds = rp.rounds;
        hr.assign(std::max(rounds, 1), XH{});
        if (trace && rounds) ZK_TRY(upload(0));
        // two rounds in flight: rounds 0 and 1 go out before the replicated columns, and round k + 2 before round k's
        // extension when it is gathered in place (after it when staged: it reuses round k's staging buffer), so the link
        // always has the next round queued
        for (int k = 0; k < std::min(rounds, 2); k++) ZK_TRY(issue(k));
        if (rep) {
            ZK_TRY(sched_entry(X, 'K', -1));
            ZK_TRY(each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
                return for_runs(U, rep, [this, l, p, pl](int c0, int k) {
                    ntt(p->st, pl->Tn, p->d_trace + (size_t)c0 * n, n, p->polys + (size_t)c0 * n, n, k, true, nullptr,
                        &inv_n, p->tmp);
                    ntt_lde(p->st, pl->Tn, pl->ct, p->polys + (size_t)c0 * n, n, k, X.rank[l] * Bl, 1, Bl,
                            p->lde + (size_t)c0 * Bl * n, (size_t)Bl * n, n, p->tmp);
                    return ZK_OK;
                });
            }));
        }
        for (int k = 0; k < rounds; k++) {
            const bool next = k + 2 < rounds, ahead = next && rp.inplace(k + 2);
            if (ahead) ZK_TRY(issue(k + 2));
            ZK_TRY(finish(k));
            if (next && !ahead) ZK_TRY(issue(k + 2));
        }
        return ZK_OK;
    }
    // the columns formed from the last row (after the last round: a short round's padding may have landed there)
    int trace_fills() {
        if (!X.fixed && !(S | (clk ? 1u : 0u))) return ZK_OK;
        return each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
            if (X.fixed) return fill_fixed(p, X.fixed[l]);
            if (S) ZK_TRY(fill_sparse(l, p, pl));
            if (clk) fill_clock(l, p, pl);
            return ZK_OK;
        });
    }
    int fill_fixed(zk_prover *p, const FixedCols &fx) {
        if (!p->fix_ws) ZK_CHECK_HIP(p->arena.alloc(&p->fix_ws, W));
        fe_ws ws[W];
        for (int c = 0; c < W; c++) ws[c] = make_fe_ws(fx.last[c]);
        ZK_TRY(h2d_small(p, p->fix_ws, ws, sizeof ws));
        fixed_axpy(p->st, fx, p->fix_ws, n, (size_t)Bl, p->polys, p->lde);
        return ZK_OK;
    }
    int fill_sparse(int l, zk_prover *p, Plan *pl) {
        if (trace) ZK_TRY(h2d_small(p, p->sp_last, lastv, sizeof lastv));  // (device traces: the detection's)
        int cols[W], k = 0;
        for (int c = 0; c < W; c++)
            if ((S >> c) & 1u) cols[k++] = c;
        return for_runs(cols, k, [this, l, p, pl](int c, int cnt) {
            SparseCols sc = spc[l];
            sc.col0 = c;
            sc.fused = false;
            sc.all = true;  // fills only
            ntt(p->st, pl->Tn, p->polys + (size_t)c * n, n, p->polys + (size_t)c * n, n, cnt, true, nullptr, &inv_n,
                p->tmp, &sc);
            ntt_lde(p->st, pl->Tn, pl->ct, p->polys + (size_t)c * n, n, cnt, X.rank[l] * Bl, 1, Bl,
                    p->lde + (size_t)c * Bl * n, (size_t)Bl * n, n, p->tmp, &sc);
            return ZK_OK;
        });
    }
    void fill_clock(int l, zk_prover *p, const Plan *pl) {
        const fe_ws d = make_fe_ws(fe_sub(lastv[0], fe_make(n - 1)));
        axpy_fill(p->st, pl->id_poly, pl->lagr, d, n, p->polys);
        for (int j = 0; j < Bl; j++) {
            const size_t r = (size_t)X.rank[l] * Bl + j;
            axpy_fill(p->st, pl->id_lde + pl->lde_slot((int)r) * n, pl->lagr_lde + pl->lde_slot((int)r) * n, d, n,
                      p->lde + (size_t)j * n);
        }
    }
    // host traces: the flags of the columns each rank interpolated (for the next proof's hints) and each rank's check
    // of the hinted ones, all-gathered: every rank then holds the same view.  ZK_SH_REDO: a hint was refuted.
    int learn_hints() {
        if (!trace || !X.detect) return ZK_OK;
        checked.wait();
        ZK_TRY(each_rank(X, [this](int l, zk_prover *p, Plan *) -> int {
            const uint32_t b = bad[l].load();
            return h2d_small(p, p->sp_nz + 3 * W + 1, &b, sizeof b);
        }));
        unsigned nz[4 * W];
        ZK_TRY(gather_flags(nz, false));
        if ((X.sh_refuted = nz[3 * W + 1]) != 0) return ZK_SH_REDO;  // (bit c: column c's hint was refuted)
        // next proof: the columns found sparse (uploaded ones with no nonzero entry before the last row, and the
        // hinted ones, which the checks confirmed), narrow (8- / 32-bit before the last row), and the clock when
        // column 0 was found 32-bit (or was derived)
        uint32_t sp_next = S, w8 = 0, w32 = 0;
        for (int i = 0; i < nU; i++) {
            const int c = U[i];
            if (nz[c] == 0) sp_next |= 1u << c;
            else if (nz[W + c] == 0) w8 |= 1u << c;
            else if (nz[2 * W + c] == 0) w32 |= 1u << c;
        }
        const bool clk_next = clk || (!(sp_next & 1u) && (w32 & 1u));
        if (clk_next) w32 &= ~1u;
        for (zk_prover *p : X.P) {
            p->sh_sparse = sp_next;
            p->sh_nw8 = w8;
            p->sh_nw32 = w32;
            p->sh_clock = clk_next;
            p->sh_hint_n = n;
            p->sh_hint_g = G;
            memcpy(p->sh_hint_key, pub->program_hash, 32);
        }
        return ZK_OK;
    }
    // the row hashes of local rank l's cosets, piece k (Bl = 1, 2, 4 -> its template instance)
    void hash_rows(int l, const fe *base, int ncols, uint8_t *blk, uint8_t *send, int log_QG, int log_K, int k) {
        with_bl(Bl, [=](auto bl) {
            hipLaunchKernelGGL((k_sh_hash_rows_blk<decltype(bl)::value>), dim3(cdiv(X.n >> log_K, 256)), dim3(256), 0,
                               X.P[l]->st, base, ncols, X.log_n, log_QG, log_K, k, blk, send);
        });
    }
    int commit_trace() {
        stage_mark(P0, "trace_lde");
        for (int l = 0; l < nlp; l++) Ttrace.blk[l] = X.P[l]->sh_blk, Ttrace.nodes[l] = X.P[l]->nodes;
        ZK_TRY(dist_commit(X, Ttrace, N, [this](int l, uint8_t *send, int log_QG, int log_K, int k) {
            hash_rows(l, X.P[l]->lde, W, Ttrace.blk[l], send, log_QG, log_K, k);
        }, "trace_digests", "trace_roots"));
        memcpy(R.trace_root, Ttrace.root, 32);
        stage_mark(P0, "trace_commit");
        coin.reseed(R.trace_root);
        return ZK_OK;
    }

    // ---- S3: constraint evaluation over the local CE cosets (CE domain = LDE domain at blowup 8).  The assertion terms
    // are not evaluated per row: S4 adds their quotient in coefficient form, each rank over its n / G coefficient
    // slice (boundary_range_*; traces too short for whole ranges keep the per-row form).
    int air_tables() {
        draw_air_consts(coin, pub, n, KX, Kp, R);
        K = Kp[0];
        return each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
            // divisor tables of the local CE cosets (3 planes of Bl*n): they depend on n and the cosets only, so the
            // plan keeps them for the rank's next proofs (round 6: 0.26 ms per rank and proof at G = 8, 2^22)
            const int r0 = X.rank[l] * Bl;
            if (!pl->sh_divs || pl->sh_divs_r0 != r0 || pl->sh_divs_cos != Bl) {
                if (pl->sh_divs && pl->sh_divs_cos < Bl) pl->sh_divs = nullptr;  // (a full prover serving a smaller world)
                if (!pl->sh_divs) ZK_CHECK_HIP(p->arena.alloc(&pl->sh_divs, (size_t)3 * Bl * n));
                fe xr[8];
                for (int j = 0; j < Bl; j++) xr[j] = K.xr[r0 + j];
                ZK_TRY(h2d_small(p, p->sh_xr, xr, Bl * sizeof(fe)));
                Fe8 zloc{};
                for (int j = 0; j < Bl; j++) zloc.v[j] = K.inv_zn[r0 + j];
                divisor_tables(p->st, pl->Tn, p->sh_xr, ilog2(Bl), log_n, K.g_last1, K.g_last2, zloc, pl->sh_divs);
                pl->sh_divs_r0 = r0;
                pl->sh_divs_cos = Bl;
            }
            return h2d_small(p, pb(p).air_consts, Kp, KX * sizeof K);
        });
    }
    // S3 + S4's first step, coset by coset (round 6): evaluate local coset j, inverse-transform it (KX planes), pack
    // its coefficient slices [d][plane][k'] and start its all-to-all, which then runs under coset j + 1's evaluation
    // instead of after the last one.  Piece j lands in the receive area [j][s][plane][k'] (after the KX*Bl*n
    // evaluations in COMP); the NTT scratch and the send areas are in p->tmp.
    size_t recv0() const { return (size_t)KX * Bl * n; }  // the receive area's offset in COMP
    int constraints() {
        ZK_TRY(air_tables());
        hs.assign(Bl, XH{});
        for (int j = 0; j < Bl; j++) {
            ZK_TRY(each_rank(X, [this, j](int l, zk_prover *p, Plan *pl) -> int {
                const EvalMap em{1, X.rank[l] * Bl + j, 1, 0, Bl, (size_t)Bl * n};
                const Planes b = pb(p);
                ZK_CHECK_HIP(eval_constraints(p->st, KX, p->lde + (size_t)j * n, log_n, em, pl->periodic,
                                              pl->sh_divs + (size_t)j * n, (const AirConsts *)b.air_consts, (size_t)Bl * n,
                                              b.comp + (size_t)j * n, !range_split));
                fe *scr = p->tmp, *send = scr + (size_t)KX * n * (1 + j);
                ntt(p->st, pl->Tn, b.comp + (size_t)j * n, (size_t)Bl * n, b.ctmp + (size_t)j * n, (size_t)Bl * n, KX, true,
                    nullptr, nullptr, scr);
                hipLaunchKernelGGL(k_sh_pack_coset, dim3(cdiv((size_t)KX * n, 256)), dim3(256), 0, p->st,
                                   (const fe *)b.ctmp + (size_t)j * n, (size_t)Bl * n, log_n, KX, ilog2(kg), send);
                xb.set(l, send, b.comp + recv0() + (size_t)j * KX * n);
                return ZK_OK;
            }));
            ZK_TRY(xchg_start(X, "comp_slices", A2A, xb, (size_t)KX * kg * sizeof(fe), &hs[j]));
        }
        stage_mark(P0, "constraints");
        return ZK_OK;
    }

    // ---- S4: composition polynomial: the cross-coset step on this rank's slice, all-gather of the C columns; then
    // local coset LDE + commitment
    // this rank's range sums of plane pln's assertion quotient (they read only the trace coefficients), into xb
    int boundary_begin(int pln) {
        return each_rank(X, [this, pln](int l, zk_prover *p, Plan *) -> int {
            // (a sharded rank writes every column's coefficients: the all-PLAIN table)
            const void *sums = boundary_range_begin(p->st, coeff_plain(p->polys, n), nullptr, log_n, Kp[pln], K.g_last2,
                                                    p->dscratch, (size_t)X.rank[l] * kg, kg);
            xb.set(l, sums, p->sh_buf);
            return ZK_OK;
        });
    }
    int cross_step() {
        const fe scale = h_inv(fe_make(8 * n)), w8inv = h_inv(h_root_of_unity(3)), inv3n = h_inv(h_pow(fe_make(3), n));
        return each_rank(X, [=](int l, zk_prover *p, Plan *pl) -> int {
            const Planes b = pb(p);
            ZK_CHECK_HIP(hipMemsetAsync(p->flag, 0, 4, p->st));
            for (int pln = 0; pln < KX; pln++) {  // base column (c, pln) of E column c -> CTMP slice c*KX + pln
                CrossMap cm;
                for (int r = 0; r < 8; r++)  // global coset r = s Bl + j: piece j, source s
                    cm.c[r] = b.comp + recv0() + ((size_t)(r % Bl) * G * KX + (size_t)(r / Bl) * KX + pln) * kg;
                cm.k0 = (size_t)X.rank[l] * kg;
                cm.kcount = kg;
                cm.pstride = (size_t)KX * kg;
                comp_cross_mapped(p->st, cm, pl->Tce, pl->inv3, scale, w8inv, inv3n, C, b.ctmp + pln * kg, p->flag);
            }
            return ZK_OK;
        });
    }
    // the column polynomials: one all-gather per column, started in order on the exchange stream (they run back to
    // back); the coset LDE of a group of columns starts as soon as the group has arrived, so the later columns'
    // all-gathers run under the earlier columns' LDEs.  Over F the columns after column 0 go out before its
    // assertion quotient is added (over E the second plane's range sums would queue behind them).
    int start_columns(int c0, int c1) {
        for (int c = c0; c < c1; c++)
            ZK_TRY(xchg_start(X, "comp_columns", AG, bufs([this, c](int, zk_prover *p) {
                return SR{pb(p).ctmp + c * kg, p->cpolys + (size_t)c * n};
            }), kg * sizeof(fe), &hc[c]));
        return ZK_OK;
    }
    // assertion quotient over this rank's slice of composition column 0 (plane by plane: the division scratch is
    // shared); the range sums are all-gathered and each rank adds the later ranks' as its carry
    int boundary_quotient(XH &hb0) {
        for (int pln = 0; range_split && pln < KX; pln++) {
            if (pln == 0) {
                ZK_TRY(xchg_wait(X, hb0));
            } else {
                ZK_TRY(boundary_begin(pln));
                ZK_TRY(xchg(X, "bnd_totals", AG, xb, 2 * sizeof(fe)));
            }
            ZK_TRY(each_rank(X, [this, pln](int l, zk_prover *p, Plan *) -> int {
                hipLaunchKernelGGL(k_sh_suffix_carry, dim3(1), dim3(64), 0, p->st, p->sh_buf, G, X.rank[l], 2, p->ood);
                const size_t k0 = (size_t)X.rank[l] * kg;
                boundary_range_end(p->st, log_n, K.g_last2, p->dscratch, k0, kg, p->ood, pb(p).ctmp + pln * kg - k0, p->flag);
                return ZK_OK;
            }));
        }
        return ZK_OK;
    }
    int extend(int a, int b) {  // columns [a, b) over the local cosets, as they arrive
        // groups hold >= 2^22 LDE points per launch, in the order the columns went out
        const int grp = (int)std::max<size_t>(1, ((size_t)1 << 22) / ((size_t)Bl * n));
        for (int c0 = a; c0 < b; c0 += grp) {
            const int c1 = std::min(b, c0 + grp);
            for (int c = c0; c < c1; c++) ZK_TRY(xchg_wait(X, hc[c]));
            ZK_TRY(each_rank(X, [this, c0, c1](int l, zk_prover *p, Plan *pl) -> int {
                ntt_lde(p->st, pl->Tn, pl->ct, p->cpolys + (size_t)c0 * n, n, c1 - c0, X.rank[l] * Bl, 1, Bl,
                        pb(p).clde + (size_t)c0 * Bl * n, (size_t)Bl * n, n, p->tmp);
                return ZK_OK;
            }));
        }
        return ZK_OK;
    }
    int composition() {
        // (the first plane's assertion quotient reads only the trace coefficients: it runs under the all-to-all, and
        // its range sums' all-gather follows the all-to-all's pieces on the exchange stream)
        XH hb0;
        if (range_split) {
            ZK_TRY(boundary_begin(0));
            ZK_TRY(xchg_start(X, "bnd_totals", AG, xb, 2 * sizeof(fe), &hb0));
        }
        for (XH &x : hs) ZK_TRY(xchg_wait(X, x));
        ZK_TRY(cross_step());
        hc.assign(CK, XH{});
        const int early = KX == 1 ? 1 : CK;  // columns [early, CK) start before the quotient
        if (early < CK) ZK_TRY(start_columns(early, CK));
        ZK_TRY(boundary_quotient(hb0));
        ZK_TRY(start_columns(0, early));
        ZK_TRY(xchg_start(X, "degree_flags", AG, bufs([](int, zk_prover *p) { return SR{p->flag, p->sh_flags}; }),
                          sizeof(unsigned), &hdeg));
        ZK_TRY(extend(early, CK));
        ZK_TRY(extend(0, early));
        return commit_composition();
    }
    int commit_composition() {
        for (int l = 0; l < nlp; l++) Tcomp.blk[l] = X.P[l]->sh_cblk, Tcomp.nodes[l] = X.P[l]->cnodes;
        ZK_TRY(dist_commit(X, Tcomp, N, [this](int l, uint8_t *send, int log_QG, int log_K, int k) {
            hash_rows(l, pb(X.P[l]).clde, CK, Tcomp.blk[l], send, log_QG, log_K, k);
        }, "comp_digests", "comp_roots"));
        memcpy(R.constraint_root, Tcomp.root, 32);
        stage_mark(P0, "composition");
        ZK_TRY(xchg_wait(X, hdeg));
        std::vector<unsigned> f(G);
        ZK_TRY(d2h_small(P0, f.data(), P0->sh_flags, G * sizeof(unsigned)));
        ZK_TRY(d2h_flush(P0));
        for (unsigned v : f) degree_flag |= v;
        coin.reseed(R.constraint_root);
        return ZK_OK;
    }

    // ---- S5: OOD frame -- every rank evaluates its 1/G of the coefficient range of the (replicated) polynomials, the
    // partial sums are all-gathered and added on the host -- then DEEP over the local cosets
    // nv values per rank (ood_eval output); the frame value v is sum over ranks of part[rank][v]
    template <typename Launch>
    int ood_parts(int nv, Launch launch, std::vector<fe> &sum) {
        ZK_TRY(each_rank(X, [this, launch](int l, zk_prover *p, Plan *) -> int {
            launch(p, X.rank[l]);
            xb.set(l, p->ood, p->sh_buf);
            return ZK_OK;
        }));
        ZK_TRY(xchg(X, "ood_parts", AG, xb, (size_t)nv * sizeof(fe)));
        std::vector<fe> parts((size_t)G * nv);
        ZK_CHECK_HIP(hipSetDevice(P0->device));
        ZK_TRY(d2h_small(P0, parts.data(), P0->sh_buf, parts.size() * sizeof(fe)));
        ZK_TRY(d2h_flush(P0));
        sum.assign(nv, fe_zero());
        for (int d = 0; d < G; d++)
            for (int v = 0; v < nv; v++) sum[v] = fe_add(sum[v], parts[(size_t)d * nv + v]);
        return ZK_OK;
    }
    // DEEP as an exact polynomial (kernels.hip), split by coefficient range: each rank combines and divides its n / G
    // coefficients, the ranges' totals are all-gathered for the suffix carries, and the quotient slices are all-gathered
    // (in place) before every rank extends it over its cosets.  begin(p, k0) -> device totals (2 kx elements),
    // end(p, k0, ext) -> the coefficient buffer (kx planes of n); `upload` stages the DEEP constants
    template <typename Begin, typename End, typename Upload>
    int deep_split_ranges(int kx, Begin begin, End end, Upload upload) {
        const int nc = 2 * kx;
        ZK_TRY(each_rank(X, [this, begin, upload](int l, zk_prover *p, Plan *) -> int {
            ZK_TRY(upload(p));
            xb.set(l, begin(p, (size_t)X.rank[l] * kg), p->sh_buf);
            return ZK_OK;
        }));
        ZK_TRY(xchg(X, "deep_totals", AG, xb, (size_t)nc * sizeof(fe)));
        ZK_TRY(each_rank(X, [this, end, nc](int l, zk_prover *p, Plan *) -> int {
            hipLaunchKernelGGL(k_sh_suffix_carry, dim3(1), dim3(64), 0, p->st, p->sh_buf, G, X.rank[l], nc, p->ood);
            Dk[l] = end(p, (size_t)X.rank[l] * kg, p->ood);
            return ZK_OK;
        }));
        XH hp[2];  // (both planes' all-gathers go out before either is waited for)
        for (int plane = 0; plane < kx; plane++)
            ZK_TRY(xchg_start(X, "deep_slices", AG, bufs([this, plane](int l, zk_prover *) {
                fe *d = const_cast<fe *>(Dk[l]) + (size_t)plane * n;  // (in place: this rank's slice is already there)
                return SR{d + (size_t)X.rank[l] * kg, d};
            }), kg * sizeof(fe), &hp[plane]));
        for (int plane = 0; plane < kx; plane++) ZK_TRY(xchg_wait(X, hp[plane]));
        return ZK_OK;
    }
    int lde_deep() {  // the DEEP coefficients over the local cosets g Bl + j (planar per rank: plane stride Bl * n)
        ZK_TRY(each_rank(X, [this](int l, zk_prover *p, Plan *pl) -> int {
            for (int plane = 0; plane < KX; plane++)
                lde_cosets(p->st, pl->Tn, pl->ct, Dk[l] + plane * n, n, X.rank[l] * Bl, 1, Bl,
                           pb(p).deep + (size_t)plane * Bl * n, p->tmp);
            return ZK_OK;
        }));
        stage_mark(P0, "deep");
        return ZK_OK;
    }
    template <int KX_>
    int ood_deep_kx() {
        typedef Chal<KX_> XF;
        typedef typename XF::T T;
        const T z = XF::make(coin.draw_ext(KX_)), zg = XF::mulb(z, g);
        fe_to_bytes(XF::comp(z, 0), R.z);
        std::vector<fe> hv;
        ZK_TRY(ood_parts(KX_ * (2 * W + CK), [this, z, zg](zk_prover *p, int rank) {
            ood_eval(p->st, coeff_plain(p->polys, n), W, p->cpolys, CK, log_n, z, zg, pb(p).ood_tab, pb(p).partials, p->ood,
                     rank, G);
        }, hv));
        std::vector<fe2> e;
        ood_reseed(coin, KX_, hv, C, R, e, h);
        stage_mark(P0, "ood");
        const DeepConsts<KX_> D = draw_deep_consts<KX_>(coin, e, C, z, zg, R);
        auto upload = [this, D](zk_prover *p) { return h2d_small(p, pb(p).deep_consts, &D, sizeof D); };
        if (range_split) {
            ZK_TRY(deep_split_ranges(KX_, [this, z, zg](zk_prover *p, size_t k0) {
                return deep_range_begin(p->st, coeff_plain(p->polys, n), p->cpolys, C, log_n, pb(p).deep_consts, z, zg,
                                        pb(p).dscratch, k0, kg);
            }, [this, z, zg](zk_prover *p, size_t k0, const fe *ext) {
                return deep_range_end(p->st, log_n, z, zg, pb(p).dscratch, k0, kg, ext);
            }, upload));
        } else {
            ZK_TRY(each_rank(X, [this, z, zg, upload](int l, zk_prover *p, Plan *) -> int {
                ZK_TRY(upload(p));
                Dk[l] = deep_poly(p->st, coeff_plain(p->polys, n), p->cpolys, C, log_n, pb(p).deep_consts, z, zg,
                                  pb(p).dscratch);
                return ZK_OK;
            }));
        }
        return lde_deep();
    }
    int ood_deep() {
        return with_kx(KX, [this](auto kx) { return ood_deep_kx<decltype(kx)::value>(); });
    }

    // ---- S6: FRI.  Layer 0 is sharded (its fold rows stay in one coset), and so is layer 1 when a layer follows it and
    // every rank holds enough of its rows; the next layer is all-gathered and the remaining layers run on local rank 0
    // of every process.
    // a layer all-gathered into `stage` ([s][plane][j][q']: mg positions per coset) -> natural order per plane in FRI
    void permute_gathered(const fe *stage, size_t mg) {
        for (int pln = 0; pln < KX; pln++)
            hipLaunchKernelGGL(k_sh_permute, dim3(cdiv(8 * mg, 256)), dim3(256), 0, P0->st,
                               (const uint8_t *)(stage + (size_t)pln * Bl * mg), G, Bl, ilog2(mg), 16, (size_t)KX * Bl * mg,
                               (uint8_t *)(pb(P0).fri + pln * 8 * mg));
    }
    int fri_none() {  // no folding: the remainder is the whole DEEP layer, all-gathered into natural order per plane
        ZK_TRY(xchg(X, "remainder_layer", AG, bufs([this](int, zk_prover *p) { return SR{pb(p).deep, pb(p).comp}; }),
                    (size_t)KX * Bl * n * sizeof(fe)));
        ZK_TRY(lead_segment(X));
        ZK_CHECK_HIP(hipSetDevice(P0->device));
        permute_gathered(pb(P0).comp, n);
        std::vector<fe> rv(KX * N);
        ZK_TRY(d2h_small(P0, rv.data(), pb(P0).fri, rv.size() * sizeof(fe)));
        ZK_TRY(d2h_flush(P0));
        return remainder_step(KX, rv, 8, coin, R, degree_flag, Y.rem_flat);
    }
    // layer `layer`'s leaves (vals: this rank's cosets, log_len positions each) into tree T, the root into the coin
    int commit_sharded_layer(int layer, DistTree &T, bool ctmp, int log_len, int log_rows, const char *digests,
                             const char *roots) {
        ZK_TRY(dist_commit(X, T, rows0 >> (layer * ilog2(fold)), [=, &T](int l, uint8_t *send, int log_QG, int log_K, int k) {
            zk_prover *p = X.P[l];
            const fe *vals = ctmp ? pb(p).ctmp : pb(p).deep;
            with_bl(Bl, [=, &T](auto bl) {
                launch_fri0_blk<decltype(bl)::value>(p->st, KX, vals, log_len, (int)fold, log_rows, log_QG, log_K, k,
                                                     T.blk[l], send);
            });
        }, digests, roots, false));
        memcpy(R.fri_roots[layer], T.root, 32);
        coin.reseed(R.fri_roots[layer]);
        return ZK_OK;
    }
    // alpha of `layer` from the host coin into every local rank's fold constants, then the fold over the local cosets
    int fold_sharded_layer(int layer, bool from_ctmp, int log_len, int log_rows, size_t wstride) {
        const fe2 alpha = coin.draw_ext(KX);
        fe_to_bytes(alpha.a, R.fri_alphas[layer]);
        ZK_TRY(with_kx(KX, [&](auto kx) {
            const auto F = fold_consts<decltype(kx)::value>(alpha, fold);
            return each_rank(X, [&](int, zk_prover *p, Plan *) -> int { return h2d_small(p, pb(p).fold_consts, &F, sizeof F); });
        }));
        return each_rank(X, [=](int l, zk_prover *p, Plan *pl) -> int {
            const Planes b = pb(p);  // layer 0 (DEEP) -> layer 1 in CTMP -> layer 2 in COMP, each [plane][j][q0]
            sh_fri_fold0(p->st, KX, (int)fold, from_ctmp ? b.ctmp : b.deep, log_len, Bl, X.rank[l], log_rows, b.fold_consts,
                         pl->TN.inv_lo, pl->TN.inv_hi, wstride, from_ctmp ? b.comp : b.ctmp);
            return ZK_OK;
        });
    }
    int fri_sharded() {
        for (int l = 0; l < nlp; l++) {  // the layer-0 tree's subtree heap (m nodes) in the NTT scratch
            Tfri0.blk[l] = X.P[l]->sh_fblk, Tfri0.nodes[l] = (uint8_t *)X.P[l]->tmp;
            Tfri1.blk[l] = X.P[l]->sh_f1blk, Tfri1.nodes[l] = Tfri0.nodes[l] + 32 * m;  // (after its m nodes)
        }
        ZK_TRY(commit_sharded_layer(0, Tfri0, false, log_n, log_m, "fri0_digests", "fri0_roots"));
        ZK_TRY(fold_sharded_layer(0, false, log_n, log_m, 1));
        // Layer 1 (round 6): with a layer after it and enough rows per rank it is committed and folded on every rank
        // over its own cosets, as layer 0 (block ownership keeps its leaves and fold rows local), and layer 2 is
        // all-gathered instead of layer 1; the lead rank runs the layers after the gathered one.
        sh1 = nl >= 2 && m1 >= 8 * (size_t)G;
        lg = sh1 ? 2 : 1;
        const size_t mg = sh1 ? m1 : m, Lg = 8 * mg;  // the gathered layer: positions per coset, length
        if (sh1) {
            ZK_TRY(commit_sharded_layer(1, Tfri1, true, log_m, ilog2(m1), "fri1_digests", "fri1_roots"));
            ZK_TRY(fold_sharded_layer(1, true, log_m, ilog2(m1), fold));  // (a layer of N / fold rows: wstride fold)
        }
        // the gathered layer into the lead's FRI buffer: base field with layers after it, in place (chunk [s][j] is
        // coset s Bl + j: the layer arrives coset-major, which the layer kernels read through FriLayout); else through
        // a staging area, permuted into natural order per plane (over E each source's chunk holds both planes, and a
        // last layer goes to the host in natural order)
        const bool inplace = KX == 1 && nl > lg;
        const size_t stage_off = (size_t)KX * Lg;
        ZK_TRY(xchg(X, sh1 ? "fri_layer2" : "fri_layer1", AG, bufs([=](int, zk_prover *p) {
            const Planes b = pb(p);
            return SR{sh1 ? b.comp : b.ctmp, inplace ? b.fri : sh1 ? b.fri + stage_off : b.comp};
        }), (size_t)KX * Bl * mg * sizeof(fe)));
        ZK_TRY(lead_segment(X));  // from here the FRI layers after it and the queries run on the lead rank alone
        ZK_CHECK_HIP(hipSetDevice(P0->device));
        if (!inplace) permute_gathered(sh1 ? pb(P0).fri + stage_off : pb(P0).comp, mg);
        lbg = inplace ? 3 : 0;
        Y.len[1] = rows0;
        Y.vals[lg] = pb(P0).fri;
        Y.len[lg] = Lg;
        return ZK_OK;
    }
    // the lead's layers, as the single-GPU path's (fri_lead_layers); their digests go into fri_dig: the all-to-all
    // scratch is free once layers 0 (and 1) are committed
    int fri_lead() {
        return fri_lead_layers(P0, X.pl[0], KX, fold, 8, N, lg, lbg, pb(P0).fri + KX * Y.len[lg], P0->fri_dig, Y, coin, R,
                               degree_flag);
    }
    int fri() {
        ZK_TRY(fri_shape());
        ZK_TRY(nl == 0 ? fri_none() : fri_sharded());
        if (nl > 0) ZK_TRY(fri_lead());
        stage_mark(P0, "fri");
        return ZK_OK;
    }

    // ---- S7 / S8: positions, then every rank gathers the chunks it owns; all-gather; the host combines
    void request_row(int buf, int ncols, uint64_t i) {  // row i of the trace or composition LDE
        const int r = (int)(i & 7), own = r / Bl, j = r % Bl;
        const size_t q = i >> 3;
        for (int c = 0; c < ncols; c++) req.push_back({own, buf, 16 * (((size_t)c * Bl + j) * n + q), nullptr});
    }
    // fold row r of a sharded layer (len positions per coset in buffer buf, planes at stride Bl len): value
    // i = r + k rows at [plane][i & 7's slot][i >> 3]
    void request_sharded_fold(int buf, size_t len, size_t rows, uint64_t r) {
        for (uint32_t k = 0; k < fold; k++)
            for (int pln = 0; pln < KX; pln++) {
                const size_t i = r + k * rows;
                const int c = (int)(i & 7), own = c / Bl, j = c % Bl;
                req.push_back({own, buf, 16 * ((size_t)pln * Bl * len + (size_t)j * len + (i >> 3)), nullptr});
            }
    }
    void request_values() {
        req.clear();
        for (uint64_t q : pos) request_row(B_LDE, W, q);
        for (uint64_t q : pos) request_row(B_CLDE, CK, q);
        if (nl > 0)
            for (uint64_t r : fri_pos[0]) request_sharded_fold(B_DEEP, n, rows0, r);
        for (int l = 1; l < nl; l++) {
            const size_t L = Y.len[l], rows = L / fold;
            if (l == 1 && sh1) {  // layer 1 on the owners of its cosets, in CTMP
                for (uint64_t r : fri_pos[1]) request_sharded_fold(B_CT, m, rows, r);
                continue;
            }
            const int lb = l == lg ? lbg : 0, lcn = ilog2(L) - lb;
            for (uint64_t r : fri_pos[l])
                for (uint32_t k = 0; k < fold; k++)
                    for (int pln = 0; pln < KX; pln++) {
                        const size_t i = r + k * rows, at = ((i & (((size_t)1 << lb) - 1)) << lcn) + (i >> lb);
                        req.push_back({0, B_FRI,
                                       (size_t)((const uint8_t *)(Y.vals[l] + pln * L + at) - (const uint8_t *)pb(P0).fri),
                                       nullptr});
                    }
        }
        off_dig = req.size();
    }
    void request_digests() {
        const DistTree *trees[4] = {&Ttrace, &Tcomp, &Tfri0, &Tfri1};
        const int tbuf[4][3] = {{-1, B_TN, B_TB}, {-1, B_CN, B_CB}, {-1, B_F0N, B_F0B}, {-1, B_F1N, B_F1B}};  // (Loc::which)
        const int ndist = sh1 ? 4 : 3;  // distributed trees: trace, composition, FRI layer 0 (and 1)
        for (int b = 0; b < 2 + nl; b++)
            for (auto &path : O->plans[b].paths)
                for (auto &e : path) {
                    Req q{-1, 0, 0, nullptr};  // (a digest is two chunks)
                    if (b < ndist) {
                        const DistTree::Loc L = trees[b]->locate(e.first, e.second);
                        if (L.owner < 0) q.host = trees[b]->top[e.second].data();
                        else q = {L.owner, tbuf[b][L.which], L.off, nullptr};
                    } else {  // the lead's FRI layers (local rank 0 of every process, i.e. rank 0 serves)
                        const uint8_t *base = e.first ? Y.nodes[b - 2] : Y.leaves[b - 2];
                        q = {0, B_FRI_DIG, (size_t)(base + 32 * e.second - P0->fri_dig), nullptr};
                    }
                    req.push_back(q);
                    req.push_back({q.owner, q.buf, q.owner < 0 ? 0 : q.off + 16, q.host ? q.host + 16 : nullptr});
                }
    }
    int gather_openings() {  // every rank gathers the chunks it owns (the others: zero), all-gather
        const size_t NK = req.size();
        for (int l = 0; l < nlp; l++) {
            zk_prover *p = X.P[l];
            const Planes b = pb(p);
            const uint8_t *bases[14] = {(const uint8_t *)p->lde, (const uint8_t *)b.clde, (const uint8_t *)b.deep,
                                        p->nodes, p->cnodes, Tfri0.nodes[l],
                                        (const uint8_t *)b.fri, p->fri_dig, p->sh_blk, p->sh_cblk, p->sh_fblk,
                                        (const uint8_t *)b.ctmp, Tfri1.nodes[l], p->sh_f1blk};
            // (the prover's pinned staging: an asynchronous copy, no wait -- the next proof on this prover writes it again
            // only after this one has drained)
            uint64_t *addr = p->h_gather_idx;
            for (size_t t = 0; t < NK; t++) {
                const Req &q = req[t];
                addr[t] = (q.owner == X.rank[l]) ? (uint64_t)(uintptr_t)(bases[q.buf] + q.off)
                                                 : (uint64_t)(uintptr_t)p->sh_zero;
            }
            ZK_CHECK_HIP(hipSetDevice(p->device));
            ZK_CHECK_HIP(hipMemcpyAsync(p->gather_idx, addr, NK * 8, hipMemcpyHostToDevice, p->st));
            gather_chunks(p->st, p->gather_idx, NK, p->gather_out);
            xb.set(l, p->gather_out, p->sh_buf);
        }
        return xchg(X, "openings", AG, xb, NK * sizeof(fe));
    }
    int openings() {
        ZK_TRY(open_plans(P0, rows0));
        request_values();
        request_digests();
        const size_t NK = req.size();
        if (NK > ZK_GATHER_CAP) ZK_FAIL(ZK_ERR_INVALID_ARG, "too many opened values for the gather buffer");
        ZK_TRY(sched_entry(X, 'K', -1));  // (the lead-only segment ends: every rank gathers its openings)
        ZK_TRY(gather_openings());
        std::vector<fe> all((size_t)G * NK), got(NK);
        ZK_CHECK_HIP(hipMemcpyAsync(all.data(), P0->sh_buf, all.size() * sizeof(fe), hipMemcpyDeviceToHost, P0->st));
        ZK_CHECK_HIP(hipStreamSynchronize(P0->st));
        for (size_t t = 0; t < NK; t++) {
            if (req[t].owner < 0)
                memcpy(&got[t], req[t].host, 16);
            else
                got[t] = all[(size_t)req[t].owner * NK + t];
        }
        O->unpack(got.data(), pos.size(), CK, fri_pos, fold, KX, off_dig);
        stage_mark(P0, "queries");
        return ZK_OK;
    }
};

// One proof over the ranks of X, stage by stage.  ZK_SH_REDO: a column hint was refuted (prove_sharded_entry redoes it).
int prove_sharded(Ctx &X, const uint8_t *trace, const zk_options *opt, const zk_pub_inputs *pub, uint8_t *proof_out,
                  size_t *proof_len, zk_record *rec) {
    ShardedProof S(X, trace, opt, pub);
    ZK_TRY(S.start());
    if (trace) ZK_TRY(S.classify_host());
    else if (X.fixed) S.classify_fixed();
    else ZK_TRY(S.classify_device());
    ZK_TRY(S.trace_rounds());
    ZK_TRY(S.trace_fills());
    ZK_TRY(S.learn_hints());
    ZK_TRY(S.commit_trace());
    ZK_TRY(S.constraints());
    ZK_TRY(S.composition());
    ZK_TRY(S.ood_deep());
    ZK_TRY(S.fri());
    ZK_TRY(S.openings());
    return S.finish(X.P[0], proof_out, proof_len, rec);
}

}  // namespace

// ---------------------------------------------------------------- C ABI
int zk_comm_create_loopback(int world, zk_comm **out) {
    if (!out || (world != 1 && world != 2 && world != 4 && world != 8))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "world must be 1, 2, 4 or 8 (ranks own 8/world cosets)");
    auto *c = new LoopbackComm();
    c->world = world;
    c->rank = 0;
    *out = c;
    return ZK_OK;
}

int zk_comm_unique_id(uint8_t id[128]) {
    if (!id) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    return zk_rccl_unique_id(id);
}

int zk_comm_create_rccl(const uint8_t id[128], int rank, int world, int device, zk_comm **out) {
    if (!id || !out || rank < 0 || rank >= world || (world != 1 && world != 2 && world != 4 && world != 8))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid rank / world (world must be 1, 2, 4 or 8)");
    return zk_make_rccl_comm(id, rank, world, device, out);
}

int zk_comm_create_host(int rank, int world, zk_exchange_fn fn, void *ctx, zk_comm **out) {
    if (!fn || !out || rank < 0 || rank >= world || (world != 1 && world != 2 && world != 4 && world != 8))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid rank / world (world must be 1, 2, 4 or 8) or null callback");
    auto *c = new HostComm();
    c->world = world;
    c->rank = rank;
    c->fn = fn;
    c->ctx = ctx;
    *out = c;
    return ZK_OK;
}

void zk_comm_destroy(zk_comm *c) { delete c; }

int zk_comm_set_trace_split(zk_comm *c, int replicated) {
    if (!c) ZK_FAIL(ZK_ERR_INVALID_ARG, "null communicator");
    if (replicated < -1) ZK_FAIL(ZK_ERR_INVALID_ARG, "replicated columns: -1 (default) or a count");
    c->split_rep = replicated;
    return ZK_OK;
}

int zk_comm_agreement(const zk_comm *c, zk_agreement *out) {
    if (!c || !out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (!c->have_last) ZK_FAIL(ZK_ERR_INVALID_ARG, "no sharded call has exchanged control records on this communicator");
    *out = c->last;
    return ZK_OK;
}

int zk_comm_set_measure(zk_comm *c, int on) {
    if (!c) ZK_FAIL(ZK_ERR_INVALID_ARG, "null communicator");
    if (!c->loopback()) ZK_FAIL(ZK_ERR_INVALID_ARG, "the measurement mode needs a loopback communicator");
    c->measure = on != 0;
    return ZK_OK;
}

int zk_prove_sharded(zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                     const zk_options *opt, const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len,
                     zk_record *rec) {
    return zk::prove_sharded_entry(comm, provers, nlocal, trace, n, opt, pub, proof_out, proof_len, rec, nullptr);
}

int zk::shard_rank_of(const zk_comm *comm, int l) { return comm->loopback() ? l : comm->rank; }

// the exchange-side buffers of a prover, on its first sharded proof
static int shard_buffers(zk_prover *p) {
    if (p->sh_buf) return ZK_OK;
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_buf, (size_t)8 * ZK_GATHER_CAP));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_xr, 8));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_zero, 1));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_roots, 32 * 8));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_flags, 8));
    ZK_CHECK_HIP(hipMemset(p->sh_zero, 0, sizeof(fe)));
    // a rank-sized prover's Bl cosets; a full prover may serve any G >= 2 (Bl <= 4)
    const size_t bl = p->shard_world ? (size_t)8 / p->shard_world : 4, mn = p->max_n;
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_blk, 32 * (2 * bl - 1) * mn));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_cblk, 32 * (2 * bl - 1) * mn));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_fblk, 32 * (2 * bl - 1) * (mn / 2)));
    ZK_CHECK_HIP(p->arena.alloc(&p->sh_f1blk, 32 * (2 * bl - 1) * (mn / 4)));
    return ZK_OK;
}

// a hinted column was not what the previous proof found (every rank saw the same all-gathered checks): forget the
// hints (and stop speculating the clock at this length if it was refuted); the proof is redone from every column
static void forget_hints(Ctx &X) {
    for (zk_prover *p : X.P) {
        p->sh_hint_n = 0;
        p->sh_sparse = p->sh_nw8 = p->sh_nw32 = 0;
        p->sh_clock = false;
        if (X.sh_clock && (X.sh_refuted & 1u)) p->sh_clock_off_n = X.n;
    }
    X.hint_ok = false;
    X.sh_refuted = 0;
}

// the arguments checked, and the proof's context: the local ranks, their plans and buffers
static int shard_context(Ctx &X, zk_comm *comm, zk_prover **provers, int nlocal, size_t n, const zk_options *opt,
                         const zk_pub_inputs *pub) {
    if (comm->loopback() ? nlocal != comm->world : nlocal != 1)
        ZK_FAIL(ZK_ERR_INVALID_ARG,
                "a loopback communicator needs one prover per rank, an RCCL or host-exchange one exactly one");
    X.comm = comm;
    X.G = comm->world;
    X.Bl = 8 / X.G;
    X.n = n;
    for (int l = 0; l < nlocal; l++) {
        zk_prover *p = provers[l];
        if (!p) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
        if (p->shard_world && p->shard_world != X.G)
            ZK_FAIL(ZK_ERR_INVALID_ARG, "prover was created for a sharded proof over a different number of ranks");
        ZK_TRY(check_prove_args(n, p->max_n, p->max_b, opt, pub));
        X.P.push_back(p);
        X.rank.push_back(shard_rank_of(comm, l));
    }
    if (opt->blowup != 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "the sharded prover needs blowup 8 (LDE cosets = CE cosets)");
    const size_t m = n / opt->fri_folding;
    if (m < 8 * (size_t)X.G || n / X.G < 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "trace too short to shard over this many ranks");
    X.log_n = ilog2(n);
    X.C = num_comp_cols(n);
    if (X.C > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "composition column count exceeds 8");
    for (auto *p : X.P) {
        ZK_CHECK_HIP(hipSetDevice(p->device));
        Plan *pl = nullptr;
        ZK_TRY(get_plan(p, n, 8, &pl));
        ZK_TRY(plan_rank_tables(p, pl, X.rank[X.pl.size()] * X.Bl, X.G));  // its fill tables over this rank's cosets
        X.pl.push_back(pl);
        if (opt->field_extension == 2) ZK_TRY(ensure_ext(p));
        ZK_TRY(shard_buffers(p));
    }
    return ZK_OK;
}

// The hint set a rank would use for a host trace of this length, world and program (column classes are a property of
// the program): what its last sharded proof learned, under this process's switches.  ZK_SHARD_HINTS=0: none.
static HintSet local_hints(const zk_prover *H, const Plan *pl, size_t n, int G, const zk_pub_inputs *pub) {
    static const bool hints_on = env_switch("ZK_SHARD_HINTS");
    HintSet h;
    const bool fresh = hints_on && sparse_on() && pl->lagr && H->sh_hint_n == n && H->sh_hint_g == G &&
                       !memcmp(H->sh_hint_key, pub->program_hash, 32);
    if (!fresh) return h;
    h.fresh = 1;
    h.S = H->sh_sparse;
    h.clk = H->sh_clock && clock_on() && H->sh_clock_off_n != n && !(h.S & 1u) ? 1u : 0u;
    const uint32_t derived = h.S | h.clk;
    h.N8 = narrow_on() ? H->sh_nw8 & ~derived : 0u;
    h.N32 = narrow_on() ? H->sh_nw32 & ~derived & ~h.N8 : 0u;
    return h;
}

// one control exchange (comm.hpp control_gather), listed with the proof's collectives on local rank 0's prover
static int control_exchange(zk_comm *comm, zk_prover *p0, const char *name, const void *send, void *recv, size_t bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    ZK_TRY(comm->control_gather(send, recv, bytes));
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    zk_prover::XchgRec r{name, (double)bytes * (comm->world - 1), 0, 1, true};
    r.host_ms = ms;
    p0->xchg.push_back(r);
    comm->last.control_calls += 1;
    comm->last.control_bytes += bytes * (size_t)(comm->world - 1);
    return ZK_OK;
}
static bool rank_is_local(const zk_comm *comm, int r) { return comm->loopback() || r == comm->rank; }

// Trace::validate of a sharded proof, split by rows (shard_agree.hpp val_window): each local rank checks its window
// -- a device trace in place, a host trace from an upload of only its count + 1 rows of the 28 columns into its trace
// buffer, which no stage has written yet (the proof's own uploads follow, after this has drained) -- the partial
// reports are all-gathered over the control channel and every rank merges them.  No data collective, no hint state.
static int validate_sharded(Ctx &X, const uint8_t *trace, const zk_pub_inputs *pub) {
    const int nl = (int)X.P.size();
    const size_t n = X.n;
    std::vector<ValPartial> mine(nl), all(X.G);
    for (int l = 0; l < nl; l++) {
        zk_prover *p = X.P[l];
        const ValWindow w = val_window(n, X.rank[l], X.G);
        const fe *win = p->d_trace + w.first;
        size_t ld = n;
        auto upload = [&]() -> int {
            ZK_CHECK_HIP(hipSetDevice(p->device));
            ld = w.count + 1;
            win = p->d_trace;
            for (int c = 0; c < W; c++)
                ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace + (size_t)c * ld, trace + ((size_t)c * n + w.first) * sizeof(fe),
                                            ld * sizeof(fe), hipMemcpyHostToDevice, p->st));
            return ZK_OK;
        };
        const int rc = trace ? upload() : ZK_OK;
        if (rc == ZK_OK) {
            (void)validate_window_partial(p, win, ld, n, w, pub, X.rank[l], &mine[l]);  // (its status travels)
        } else {
            memset(&mine[l], 0, sizeof mine[l]);
            mine[l].version = ZK_AGREE_VERSION;
            mine[l].rank = (uint32_t)X.rank[l];
            mine[l].status = rc;
            snprintf(mine[l].msg, sizeof mine[l].msg, "%s", g_err.c_str());
        }
        if (trace) (void)hipStreamSynchronize(p->st);  // the caller's trace is free again on every way out
    }
    ZK_TRY(control_exchange(X.comm, X.P[0], "validate_report", mine.data(), all.data(), sizeof(ValPartial)));
    for (int r = 0; r < X.G; r++)
        if (all[r].status != ZK_OK && rank_is_local(X.comm, r)) {  // this rank's own error, as it met it
            char m[ZK_AGREE_MSG + 1];
            memcpy(m, all[r].msg, ZK_AGREE_MSG);
            m[ZK_AGREE_MSG] = 0;
            ZK_FAIL(all[r].status, std::string(m));
        } else if (all[r].status != ZK_OK) {
            break;  // (validation_from_partials names the lowest such rank)
        }
    return validation_from_partials(all.data(), X.G, n, pub, X.P.data(), nl, nullptr);
}

// validate_transition_degrees of a sharded proof (include/zkvm_gpu.h "transition constraint degrees": nothing in the
// definitions changes), the work split by CE coset and then by coefficient range.  Every rank holds the whole trace in
// its trace buffer (a host trace: the 28 columns copied whole, as zk_degrees_columns does), interpolates all 28 columns
// and extends them over its own Bl = 8 / G CE cosets; it forms the 20 quotients there, inverse-transforms them per
// coset and sends each rank its kg = n / G coefficients of every one (all-to-all "degrees_slices"); k_cross_degrees
// then forms coefficients k1 + n k2 of the rank's k1 range and keeps each quotient's highest non-zero global index.
// The partials travel over the control channel ("degrees_report") and every rank runs merge_degrees.  No allocation:
// the check runs in a rank-sized prover's buffers (polys; lde and tmp of 28 Bl n each), which no stage of the proof
// has written yet --
//   p->polys  the 28 trace polynomials (dense interpolation of the trace buffer, scale 1/n);
//   p->lde    first the trace LDE over the Bl local cosets (28 x Bl x n), then, once the quotients are written, the
//             20 Bl per-coset inverse transforms (plane k Bl + j), and last, once those are packed, the receive area
//             [source s][plane k Bl + j][kl] of 20 x 8 x kg coefficients: coset s Bl + j of quotient k;
//   p->tmp    the four-step scratch of the front; then the 20 x Bl n quotient values with the 8 Bl n behind them first
//             as the divisor table (3 Bl n, unless the plan's sh_divs already holds this rank's cosets) and then as the
//             scratch of the inverse transforms (groups of 8 constraints); then the send area [destination d][plane][kl];
//             and last, the exchange over, the 20 x 8 x kg coefficients when the caller asked for them.
// A rank's own error goes into its partial's status and it still issues every collective, so no peer is stranded.
struct DegreesSharded {
    Ctx &X;
    const uint8_t *const trace;  // the caller's host trace, or null: the trace is in every rank's trace buffer
    const zk_pub_inputs *const pub;
    uint8_t *const *const quotients_out;  // per local rank (null entries skipped), or null
    const int G = X.G, Bl = X.Bl, nl = (int)X.P.size(), log_n = X.log_n;
    const size_t n = X.n, kg = n / (size_t)G, CEl = (size_t)Bl * n, slice = (size_t)NUM_TCONS * 8 * kg;
    std::vector<DegPartial> mine = std::vector<DegPartial>(nl), all = std::vector<DegPartial>(G);
    std::vector<DegReport> rep = std::vector<DegReport>(nl);

    bool wants(int l) const { return quotients_out && quotients_out[l]; }
    void fail(int l, int rc) {  // (the first error of a rank is the one it reports)
        if (mine[l].status != ZK_OK) return;
        mine[l].status = rc;
        snprintf(mine[l].msg, sizeof mine[l].msg, "%s", g_err.c_str());
    }
    // steps 1 to 3 and the packing on local rank l
    int front(int l) {
        zk_prover *p = X.P[l];
        Plan *pl = X.pl[l];
        ZK_CHECK_HIP(hipSetDevice(p->device));
        if (trace) ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace, trace, (size_t)W * n * sizeof(fe), hipMemcpyHostToDevice, p->st));
        const int r0 = X.rank[l] * Bl;
        const fe inv_n = h_inv(fe_make(n));
        ntt(p->st, pl->Tn, p->d_trace, n, p->polys, n, W, true, nullptr, &inv_n, p->tmp);
        ntt_lde(p->st, pl->Tn, pl->ct, p->polys, n, W, r0, 1, Bl, p->lde, CEl, n, p->tmp);
        fe *quot = p->tmp, *scratch = p->tmp + NUM_TCONS * CEl, *per_coset = p->lde, *send = p->tmp;
        // plane 0 of the divisor tables of the local cosets: they depend on n and the cosets only
        const fe *divs = pl->sh_divs;
        if (!divs || pl->sh_divs_r0 != r0 || pl->sh_divs_cos != Bl) {
            const fe g = h_root_of_unity(log_n);
            const Fe8 zall = ce_inv_zn(log_n);
            Fe8 zloc{};
            for (int j = 0; j < Bl; j++) zloc.v[j] = zall.v[r0 + j];
            divisor_tables(p->st, pl->Tn, pl->xr_ce + r0, ilog2(Bl), log_n, h_pow(g, n - 1), h_pow(g, n - 2), zloc, scratch);
            divs = scratch;
        }
        const EvalMap em{Bl, r0, 1, 0, Bl};
        ZK_CHECK_HIP(transition_quotients(p->st, p->lde, log_n, em, pl->periodic, divs, fe_make(pub->delta),
                                          (int)pub->lwe_size, quot));
        for (int k0 = 0; k0 < NUM_TCONS; k0 += 8) {
            const int cnt = std::min(8, NUM_TCONS - k0);
            ntt(p->st, pl->Tn, quot + k0 * CEl, n, per_coset + k0 * CEl, n, Bl * cnt, true, nullptr, nullptr, scratch);
        }
        const int planes = NUM_TCONS * Bl;
        hipLaunchKernelGGL(k_sh_pack_coset, dim3(cdiv((size_t)planes * n, 256)), dim3(256), 0, p->st,
                           (const fe *)per_coset, n, log_n, planes, ilog2(kg), send);
        ZK_CHECK_HIP(hipGetLastError());
        return ZK_OK;
    }
    // steps 5 and 6's first half on local rank l: the fused kernel over the received slices, the report read back
    int scan_launch(int l) {
        zk_prover *p = X.P[l];
        Plan *pl = X.pl[l];
        ZK_CHECK_HIP(hipSetDevice(p->device));
        DegCrossMap m;
        m.c = p->lde;
        for (int r = 0; r < 8; r++) m.off[r] = ((size_t)(r / Bl) * NUM_TCONS * Bl + (size_t)(r % Bl)) * kg;
        m.cstride = (size_t)Bl * kg;
        m.k0 = (size_t)X.rank[l] * kg;
        m.kcount = kg;
        m.log_n = log_n;
        m.first = 0;
        m.count = NUM_TCONS;
        m.coeffs = wants(l) ? p->tmp : nullptr;
        ZK_CHECK_HIP(hipMemsetAsync(p->deg_rep, 0, sizeof(DegReport), p->st));
        cross_degrees(p->st, m, pl->Tce, pl->inv3, h_inv(fe_make(8 * n)), h_inv(h_root_of_unity(3)),
                      h_inv(h_pow(fe_make(3), n)), p->deg_rep);
        ZK_CHECK_HIP(hipGetLastError());
        ZK_TRY(d2h_small(p, &rep[l], p->deg_rep, sizeof(DegReport)));
        if (wants(l))
            ZK_CHECK_HIP(hipMemcpyAsync(quotients_out[l], p->tmp, slice * sizeof(fe), hipMemcpyDeviceToHost, p->st));
        return ZK_OK;
    }
    int scan_read(int l) {
        zk_prover *p = X.P[l];
        ZK_CHECK_HIP(hipSetDevice(p->device));
        ZK_TRY(d2h_flush(p));  // (a stream sync: the caller's trace and quotients_out are free again)
        collect_kernel_stats(p);
        mine[l].nonzero = rep[l].nonzero;
        for (int k = 0; k < NUM_TCONS; k++) mine[l].top[k] = rep[l].top[k];
        return ZK_OK;
    }
    // in the measurement mode a collective's copies run on local rank 0's stream, which the ranks do not share yet
    // (prove_sharded_entry swaps the streams after the checks): the ranks' streams are drained around it instead
    void drain() {
        for (zk_prover *p : X.P) {
            (void)hipSetDevice(p->device);
            (void)hipStreamSynchronize(p->st);
        }
    }
    int run(zk_degrees *out) {
        std::vector<std::unique_ptr<IoScope>> io_scopes;
        for (int l = 0; l < nl; l++) {
            ZK_CHECK_HIP(hipSetDevice(X.P[l]->device));
            io_scopes.push_back(std::make_unique<IoScope>(X.P[l]));
            memset(&mine[l], 0, sizeof mine[l]);
            mine[l].version = ZK_AGREE_VERSION;
            mine[l].rank = (uint32_t)X.rank[l];
            mine[l].first = (uint64_t)X.rank[l] * kg;
            mine[l].count = kg;
        }
        Bufs b(X);
        for (int l = 0; l < nl; l++) {
            const int rc = front(l);
            if (rc != ZK_OK) fail(l, rc);
            b.set(l, X.P[l]->tmp, X.P[l]->lde);
        }
        if (X.comm->measure) drain();
        const int xrc = xchg(X, "degrees_slices", A2A, b, (size_t)NUM_TCONS * Bl * kg * sizeof(fe));
        if (X.comm->measure) drain();
        if (xrc != ZK_OK) {  // (a transport error: the peers meet it too)
            drain();
            return xrc;
        }
        for (int l = 0; l < nl; l++) {
            const int rc = mine[l].status == ZK_OK ? scan_launch(l) : ZK_OK;
            if (rc != ZK_OK) fail(l, rc);
        }
        for (int l = 0; l < nl; l++) {
            const int rc = scan_read(l);
            if (rc != ZK_OK) fail(l, rc);
        }
        drain();  // on every way: the caller's trace and quotients_out are free again, the buffers the proof's again
        ZK_TRY(control_exchange(X.comm, X.P[0], "degrees_report", mine.data(), all.data(), sizeof(DegPartial)));
        for (int r = 0; r < G; r++)
            if (all[r].status != ZK_OK && rank_is_local(X.comm, r)) {  // this rank's own error, as it met it
                char m[ZK_AGREE_MSG + 1];
                memcpy(m, all[r].msg, ZK_AGREE_MSG);
                m[ZK_AGREE_MSG] = 0;
                ZK_FAIL(all[r].status, std::string(m));
            } else if (all[r].status != ZK_OK) {
                break;  // (degrees_from_partials names the lowest such rank)
            }
        return degrees_from_partials(all.data(), G, n, X.P.data(), nl, out);
    }
};
static int degrees_sharded(Ctx &X, const uint8_t *trace, const zk_pub_inputs *pub, zk_degrees *out,
                           uint8_t *const *quotients_out) {
    DegreesSharded D{X, trace, pub, quotients_out};
    return D.run(out);
}

// The front of every sharded entry point (world > 1): this rank's own checks into a status -- a rank that returned
// here would strand the peers whose arguments passed in their first collective -- then the control exchange, from which
// every rank learns the same outcome.  opt: the proof's options, or null for the stand-alone degree check (the record's
// options are all zero, and the context is checked under the smallest options a sharded proof accepts: n / world >= 8
// and n >= 16 world).  On a non-OK outcome nothing else has run.
static int agree_first(Ctx &X, Agreed *out, zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                       const zk_options *opt, bool proof, const zk_pub_inputs *pub, const FixedCols *fixed) {
    const int G = comm->world;
    int status = ZK_OK;
    zk_options shortest;
    memset(&shortest, 0, sizeof shortest);
    shortest.num_queries = 1, shortest.blowup = 8, shortest.field_extension = 1, shortest.fri_folding = 2;
    if ((proof && !opt) || !pub) {
        g_err = "null argument";
        status = ZK_ERR_INVALID_ARG;
    } else if (fixed && trace) {
        g_err = "preprocessed columns go with a device trace";
        status = ZK_ERR_INVALID_ARG;
    } else {
        status = shard_context(X, comm, provers, nlocal, n, proof ? opt : &shortest, pub);
    }
    const std::string status_msg = status != ZK_OK ? g_err : std::string();
    std::vector<AgreeRecord> mine(nlocal), all(G);
    for (int l = 0; l < nlocal; l++) {
        AgreeRecord &r = mine[l];
        memset(&r, 0, sizeof r);
        r.version = ZK_AGREE_VERSION;
        r.world = (uint32_t)G;
        r.rank = (uint32_t)shard_rank_of(comm, l);
        r.status = status;
        snprintf(r.msg, sizeof r.msg, "%s", status_msg.c_str());
        r.n = n;
        if (proof && opt) {
            const uint32_t o[6] = {opt->num_queries,     opt->blowup,      opt->grinding,
                                   opt->field_extension, opt->fri_folding, opt->fri_rem_max_deg};
            memcpy(r.opt, o, sizeof o);
        }
        if (pub) b3::hash_bytes(reinterpret_cast<const uint8_t *>(pub), sizeof *pub, r.pub_hash);
        r.source = fixed ? ZK_SRC_FIXED : trace ? ZK_SRC_HOST : ZK_SRC_DEVICE;
        r.split_rep = comm->split_rep;
        r.measure = comm->measure ? 1u : 0u;
        r.validate = provers[l]->validate ? 1u : 0u;
        r.validate_degrees = provers[l]->validate_degrees ? 1u : 0u;
        if (status != ZK_OK) continue;
        const Plan *pl = X.pl[l];
        r.detect = (sparse_on() && pl->lagr && pl->lagr_lde ? 1u : 0u) | (clock_on() ? 2u : 0u);
        if (trace && proof) {
            const HintSet h = local_hints(provers[l], pl, n, G, pub);
            r.hint_fresh = h.fresh, r.hint_S = h.S, r.hint_clk = h.clk, r.hint_N8 = h.N8, r.hint_N32 = h.N32;
        }
    }
    zk_prover *const p0 = provers[0];
    stage_begin(p0);  // the record of this call's exchanges starts with the control exchange
    comm->last = zk_agreement{};
    comm->have_last = false;
    ZK_TRY(control_exchange(comm, p0, "control", mine.data(), all.data(), sizeof(AgreeRecord)));
    const Agreed A = agree(all.data(), G);
    {
        const uint64_t calls = comm->last.control_calls, bytes = comm->last.control_bytes;
        comm->last = A.a;
        comm->last.control_calls = calls;
        comm->last.control_bytes = bytes;
        comm->have_last = true;
    }
    *out = A;
    if (A.a.code != ZK_OK) {
        p0->stage_done = true;  // (zk_prover_exchange_stats: the control exchange is all that ran)
        if (A.a.code == ZK_ERR_PEER && rank_is_local(comm, A.a.rank_a)) ZK_FAIL(status, status_msg);
        ZK_FAIL(A.a.code, A.msg);
    }
    return ZK_OK;
}

int zk::prove_sharded_entry(zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                            const zk_options *opt, const zk_pub_inputs *pub, uint8_t *proof_out, size_t *proof_len,
                            zk_record *rec, const FixedCols *fixed) {
    // a null or wrong-shaped communicator or prover list: no exchange is possible, so these alone return at once
    if (!comm || !provers || !proof_len || nlocal <= 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (comm->loopback() ? nlocal != comm->world : nlocal != 1)
        ZK_FAIL(ZK_ERR_INVALID_ARG,
                "a loopback communicator needs one prover per rank, an RCCL or host-exchange one exactly one");
    for (int l = 0; l < nlocal; l++)
        if (!provers[l]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    Ctx X;
    // one rank: nothing to shard or exchange, so the single-GPU path proves it (the same proof bytes; its
    // seven-coset evaluation only pays off without ranks to balance: DESIGN.md section 7, round 4)
    if (comm->world == 1) {
        if (fixed && trace) ZK_FAIL(ZK_ERR_INVALID_ARG, "preprocessed columns go with a device trace");
        ZK_TRY(shard_context(X, comm, provers, nlocal, n, opt, pub));
        return fixed ? prove_fixed(X.P[0], n, opt, pub, fixed, proof_out, proof_len)
                     : prove_single(X.P[0], trace, n, opt, pub, proof_out, proof_len, rec);
    }
    Agreed A;
    ZK_TRY(agree_first(X, &A, comm, provers, nlocal, trace, n, opt, true, pub, fixed));
    zk_prover *const p0 = provers[0];
    X.detect = A.a.detect != 0;
    X.clock = A.a.clock != 0;
    X.hints = A.hints;
    if (!A.a.hints_equal)  // stale on some rank: every rank proves from every column and learns the set anew
        for (zk_prover *p : X.P) {
            p->sh_hint_n = 0;
            p->sh_sparse = p->sh_nw8 = p->sh_nw32 = 0;
            p->sh_clock = false;
        }
    if (A.a.validate) {
        int rc = ZK_OK;
        if (fixed) {
            g_err = "sharded validation needs every trace column in HBM, not the preprocessed ones";
            rc = ZK_ERR_INVALID_ARG;
        } else {
            rc = validate_sharded(X, trace, pub);
        }
        if (rc != ZK_OK) {
            *proof_len = 0;
            p0->stage_done = true;
            return rc;
        }
    }
    if (A.a.validate_degrees) {  // the order of a debug build: Trace::validate, then the evaluator's degree check
        int rc = ZK_OK;
        if (fixed) {
            g_err = "the sharded degree check needs every trace column in HBM, not the preprocessed ones";
            rc = ZK_ERR_INVALID_ARG;
        } else {
            rc = degrees_sharded(X, trace, pub, nullptr, nullptr);
        }
        if (rc != ZK_OK) {
            *proof_len = 0;
            p0->stage_done = true;
            return rc;
        }
    }
    X.fixed = fixed;
    // measurement mode (loopback): every rank's kernels on rank 0's stream, in program order (restored on the way out)
    struct SharedStream {
        std::vector<zk_prover *> P;
        std::vector<hipStream_t> own;
        ~SharedStream() {
            for (size_t l = 1; l < P.size(); l++) {
                (void)hipStreamSynchronize(P[l]->st);
                P[l]->st = own[l];
            }
        }
    } shared;
    if (comm->measure) {
        for (auto *p : X.P) {
            // (work the caller queued on a rank's own stream -- zk_vm_prove_sharded's trace rows -- completes first)
            ZK_CHECK_HIP(hipSetDevice(p->device));
            ZK_CHECK_HIP(hipStreamSynchronize(p->st));
            shared.P.push_back(p);
            shared.own.push_back(p->st);
        }
        for (size_t l = 1; l < X.P.size(); l++) X.P[l]->st = X.P[0]->st;
    }
    X.P[0]->sched_world = X.G;
    X.P[0]->sched_measure = comm->measure;
    // every local rank's proof counts as in flight on its device (the single-GPU AUTO upload schedule reads it)
    std::vector<std::unique_ptr<DeviceBusy>> busy;
    for (auto *p : X.P) busy.push_back(std::make_unique<DeviceBusy>(p->dev_busy));
    // drop any staged reads an earlier failed proof left behind, and again on every way out of this one
    std::vector<std::unique_ptr<IoScope>> io_scopes;
    for (auto *p : X.P) {
        ZK_CHECK_HIP(hipSetDevice(p->device));
        io_scopes.push_back(std::make_unique<IoScope>(p));
    }
    const size_t cap = *proof_len;  // (in/out)
    int rc = prove_sharded(X, trace, opt, pub, proof_out, proof_len, rec);
    if (rc != ZK_SH_REDO) return rc;
    *proof_len = cap;
    forget_hints(X);
    for (zk_prover *p : X.P) p->hint_redos++;
    {  // the redone proof's record starts over, the control exchanges kept at its head
        // (host-timed records only: a degree check's "degrees_slices" sits among them, and its events start over too)
        std::vector<zk_prover::XchgRec> ctl;
        for (const auto &r : p0->xchg)
            if (r.host_ms >= 0.f && ctl.size() < comm->last.control_calls) ctl.push_back(r);
        stage_begin(p0);
        p0->xchg = ctl;
    }
    return prove_sharded(X, trace, opt, pub, proof_out, proof_len, rec);
}

int zk_degrees_sharded(zk_comm *comm, zk_prover **provers, int nlocal, const uint8_t *trace, size_t n,
                       const zk_pub_inputs *pub, zk_degrees *out, uint8_t *const *quotients_out) {
    if (!comm || !provers || nlocal <= 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (comm->loopback() ? nlocal != comm->world : nlocal != 1)
        ZK_FAIL(ZK_ERR_INVALID_ARG,
                "a loopback communicator needs one prover per rank, an RCCL or host-exchange one exactly one");
    for (int l = 0; l < nlocal; l++)
        if (!provers[l]) ZK_FAIL(ZK_ERR_INVALID_ARG, "null prover");
    if (comm->world == 1) {  // one rank: the single-GPU check (its quotients_out is the one slice, k1 = 0 .. n - 1)
        zk_degrees d;
        uint8_t *q = quotients_out ? quotients_out[0] : nullptr;
        if (!trace) {
            void *dt = nullptr;
            ZK_TRY(zk_prover_trace_buffer(provers[0], &dt));
            const int rc = zk_degrees_device(provers[0], dt, n, pub, &d, q);
            if (out && (rc == ZK_OK || rc == ZK_ERR_DEGREES)) *out = d;
            return rc;
        }
        const uint8_t *cols[W];
        for (int c = 0; c < W; c++) cols[c] = trace + (size_t)c * n * sizeof(fe);
        const int rc = zk_degrees_columns(provers[0], cols, n, pub, &d, q);
        if (out && (rc == ZK_OK || rc == ZK_ERR_DEGREES)) *out = d;
        return rc;
    }
    Ctx X;
    Agreed A;
    ZK_TRY(agree_first(X, &A, comm, provers, nlocal, trace, n, nullptr, false, pub, nullptr));
    const int rc = degrees_sharded(X, trace, pub, out, quotients_out);
    provers[0]->stage_done = true;
    return rc;
}

// (diag.hip zk_diag_degrees_parts: the production pack kernel on planes of the caller's choice)
void zk::diag_pack_coset(hipStream_t st, const fe *c, size_t plane_stride, int log_n, int planes, int log_kg, fe *send) {
    hipLaunchKernelGGL(k_sh_pack_coset, dim3(cdiv((size_t)planes << log_n, 256)), dim3(256), 0, st, c, plane_stride, log_n,
                       planes, log_kg, send);
}
