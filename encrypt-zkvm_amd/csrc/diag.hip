// diag.hip -- the test entry points (C ABI: zk_diag_*), each a direct call into one piece of the prover on inputs of the
// caller's choice.  Nothing on the prove path calls into this file.  (zk_diag_vm_states, one more, reads vm_gpu.hip's
// file-local VM state and lives there.)
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "blake3.hpp"
#include "host_pool.hpp"
#include "prover_internal.hpp"

using namespace zk;

// ---------------------------------------------------------------- the kernels only the tests launch
namespace zk {
__global__ void k_field_op(int op, const fe *a, const fe *b, fe *out, size_t count, const fe_ws *ws, const fe_w2 *w2) {
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    fe x = a[t], y = b[t];
    fe r;
    const size_t w0 = t & ~(size_t)63, mir = count - 1 - t;  // the first element of lane t's wave; the mirrored lane
    switch (op) {
    // ---- the constant-multiplier forms: ws[i] = make_fe_ws(b[i]), w2[i] = make_fe_w2(b[i]), built by the host
    case 11: r = fe_mul_uniform(x, load_fe_ws(ws, (int)w0)); break;  // wave-uniform: the W set of b[w0], scalar loads
    case 12: r = fe_mul_wsv(x, ws[t]); break;                        // per lane: the W set of b[t], vector loads
    case 13: {
        // pair (a[t], A) with (a[w0 + 63 - l], B), l = t - w0: A the W set of b[w0], B that of b[w0 + 63] (the wave's
        // first and last element; count a multiple of 64); lane t returns output t & 1 of (a[t] A, a[w0 + 63 - l] B)
        const fe_ws WA = load_fe_ws(ws, (int)w0), WB = load_fe_ws(ws, (int)w0 + 63);
        fe o[2];
        fe_mul_uniform2(x, WA, a[w0 + 63 - (t - w0)], WB, o[0], o[1]);
        r = o[t & 1];
        break;
    }
    case 14:
    case 15: {
        // pair (a[t], b[t]) with the mirrored lane's (a, b)[count - 1 - t]; lane t returns output t & 1
        fe o[2];
        if (op == 14) fe_mul_wsv2(x, ws[t], a[mir], ws[mir], o[0], o[1]);
        else fe_mul_w2_2(x, w2[t], a[mir], w2[mir], o[0], o[1]);
        r = o[t & 1];
        break;
    }
    // ---- the raw final reductions: L = a[t] (128 bits), s4 = bits 0 .. 31 of b[t], s5 = bits 32 .. 34;
    // (L + (s4 + s5 2^32) 2^128) mod p
    case 16: r = ws_fold(lo32(x.lo), hi32(x.lo), lo32(x.hi), hi32(x.hi), lo32(y.lo), hi32(y.lo) & 7u); break;
    case 17: {
        // lane t's input and the mirrored lane's (count - 1 - t) in one paired block; lane t returns output t & 1
        const fe x2 = a[mir], y2 = b[mir];
        uint32_t A[4] = {lo32(x.lo), hi32(x.lo), lo32(x.hi), hi32(x.hi)};
        uint32_t B[4] = {lo32(x2.lo), hi32(x2.lo), lo32(x2.hi), hi32(x2.hi)};
        fe o[2];
        ws_fold2(A, lo32(y.lo), hi32(y.lo) & 7u, B, lo32(y2.lo), hi32(y2.lo) & 7u, o[0], o[1]);
        r = o[t & 1];
        break;
    }
    // ---- the lazy sums of W-set products (f128.hpp acc192 / acc288_madd_uniform), W the W set of b[w0]:
    // 18: a[t] + sum_(j < 16) a[(t + j) mod count] b[w0] in 192 bits; 19: a[t] b[t] (a 256-bit product) + the same 16
    // terms in 288 bits; 20: a[t] + ACC192_MAX_TERMS times a[t] b[w0], the most terms acc192 takes
    case 18:
    case 19: {
        const fe_ws Wc = load_fe_ws(ws, (int)w0);
        acc192 s = acc192_from(x);
        acc288 s2 = acc288_zero();
        if (op == 19) acc288_madd(s2, x, y);
#pragma unroll 1
        for (int j = 0; j < 16; j++) {
            const fe v = a[(t + j) % count];
            if (op == 18) acc192_madd_uniform(s, v, Wc);
            else acc288_madd_uniform(s2, v, Wc);
        }
        r = op == 18 ? acc192_reduce(s) : acc288_reduce(s2);
        break;
    }
    case 20: {
        const fe_ws Wc = load_fe_ws(ws, (int)w0);
        acc192 s = acc192_from(x);
#pragma unroll 1
        for (int j = 0; j < ACC192_MAX_TERMS; j++) acc192_madd_uniform(s, x, Wc);
        r = acc192_reduce(s);
        break;
    }
    case 0: r = fe_add(x, y); break;
    case 1: r = fe_sub(x, y); break;
    case 2: r = fe_mul(x, y); break;
    case 3: r = fe_inv(x); break;
    case 5: r = fe_add_lazy(x, y); break;  // the NTT's lazy forms: x any value < 2^128, y canonical
    case 6: r = fe_canon(x); break;
    case 7: r = fe_mul_w2(x, fe_w2{y, fe_mul(y, fe{0, 1})}); break;  // two-part constant (w, w 2^64)
    case 8:
    case 9:
    case 10: {
        // the NTT butterflies' addsub2 forms (V = op - 8: both sums canonical, both lazy, first lazy): inputs (x, y) and
        // (a, b)[count - 1 - t]; lane t returns output t & 3 of (x + y, x - y, x2 + y2, x2 - y2)
        const fe x2 = a[count - 1 - t], y2 = b[count - 1 - t];
        fe o[4];
        if (op == 8) addsub2_v<0>(x, y, x2, y2, o[0], o[1], o[2], o[3]);
        else if (op == 9) addsub2_v<1>(x, y, x2, y2, o[0], o[1], o[2], o[3]);
        else addsub2_v<2>(x, y, x2, y2, o[0], o[1], o[2], o[3]);
        r = o[t & 3];
        break;
    }
    default: r = fe_exp(x, y.lo, y.hi); break;
    }
    out[t] = r;
}

__global__ void k_blake3_elems(const fe *in, int k, size_t count, uint8_t *out) {
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    uint32_t h[8];
    b3::hash_elements(k, [&](int i) { return in[t * k + i]; }, h);
    b3::store_digest(out + 32 * t, h);
}

// ws / w2: the W sets / two-part forms of b[0 .. count) (ops 11 .. 14 and 18 .. 20 / op 15; else null)
void diag_field_op(hipStream_t st, int op, const fe *a, const fe *b, fe *out, size_t count, const fe_ws *ws,
                   const fe_w2 *w2) {
    hipLaunchKernelGGL(k_field_op, dim3(cdiv(count, 256)), dim3(256), 0, st, op, a, b, out, count, ws, w2);
}
void diag_blake3_elems(hipStream_t st, const fe *in, int k, size_t count, uint8_t *out) {
    hipLaunchKernelGGL(k_blake3_elems, dim3(cdiv(count, 256)), dim3(256), 0, st, in, k, count, out);
}
}  // namespace zk

// ---------------------------------------------------------------- the scaffold of the GPU entry points
namespace {
// A prover of its own for one call: open() creates it on `device` for (n, blowup), with the plan on request and the E
// working set for ext = 2; up() copies caller bytes into one of its buffers, down() reads back once its stream is
// idle.  Whatever way the call is left, transfers still staged are dropped (IoScope) and then the prover is destroyed.
// It stands in for the zk_prover pointer, so an entry point names it p and reads like the code it calls.
struct DiagProver {
    zk_prover *pr = nullptr;
    Plan *pl = nullptr;
    ~DiagProver() {
        if (!pr) return;
        { IoScope drop(pr); }
        zk_prover_destroy(pr);
    }
    operator zk_prover *() const { return pr; }
    zk_prover *operator->() const { return pr; }
    int open(int device, size_t n, uint32_t blowup, bool plan = false, int ext = 1) {
        ZK_TRY(zk_prover_create(device, n, blowup, &pr));
        if (plan) ZK_TRY(get_plan(pr, n, blowup, &pl));
        if (ext == 2) ZK_TRY(ensure_ext(pr));
        return ZK_OK;
    }
    template <class T>
    int up(T *dst, const void *src, size_t count) {
        ZK_CHECK_HIP(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
        return ZK_OK;
    }
    template <class T>
    int down(void *dst, const T *src, size_t count) {
        ZK_CHECK_HIP(hipStreamSynchronize(pr->st));
        ZK_CHECK_HIP(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost));
        return ZK_OK;
    }
};
// Device memory for the entry points that need no prover: freed on every way out
struct DiagBuf {
    uint8_t *d = nullptr;
    ~DiagBuf() {
        if (d) (void)hipFree(d);
    }
    int alloc(int device, size_t bytes) {
        ZK_CHECK_HIP(hipSetDevice(device));
        ZK_CHECK_HIP(hipMalloc(&d, bytes));
        return ZK_OK;
    }
};
}  // namespace

// ---------------------------------------------------------------- the entry points
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
// reductions ws_fold / ws_fold2 of a + (b mod 2^35) 2^128.  The pairing of the two-output forms: k_field_op above.
// 18 .. 20: the lazy sums of W-set products (acc192_madd_uniform, acc288_madd_uniform), the constant as in 11; their
// terms: k_field_op above.
extern "C" int zk_diag_field_op(int device, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t count) {
    if (!a || !b || !out || count == 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (op < 0 || op > 20 || count > ((size_t)1 << 30) || (op == 13 && count % 64 != 0))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_field_op: unknown op, or a count the op does not take");
    std::vector<fe_ws> ws;
    std::vector<fe_w2> w2;
    if ((op >= 11 && op <= 14) || op >= 18) {
        ws.resize(count);
        for (size_t i = 0; i < count; i++) ws[i] = make_fe_ws(fe_from_bytes(b + 16 * i));
    } else if (op == 15) {
        w2.resize(count);
        for (size_t i = 0; i < count; i++) w2[i] = make_fe_w2(fe_from_bytes(b + 16 * i));
    }
    DiagBuf abo, tab;  // a, b and out; the constants' table
    const size_t tab_bytes = ws.size() * sizeof(fe_ws) + w2.size() * sizeof(fe_w2);
    ZK_TRY(abo.alloc(device, 3 * count * sizeof(fe)));
    if (tab_bytes) ZK_TRY(tab.alloc(device, tab_bytes));
    fe *d = (fe *)abo.d;
    ZK_CHECK_HIP(hipMemcpy(d, a, count * 16, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemcpy(d + count, b, count * 16, hipMemcpyHostToDevice));
    if (tab_bytes)
        ZK_CHECK_HIP(hipMemcpy(tab.d, ws.empty() ? (const void *)w2.data() : (const void *)ws.data(), tab_bytes,
                               hipMemcpyHostToDevice));
    diag_field_op(nullptr, op, d, d + count, d + 2 * count, count, ws.empty() ? nullptr : (const fe_ws *)tab.d,
                  w2.empty() ? nullptr : (const fe_w2 *)tab.d);
    ZK_CHECK_HIP(hipMemcpy(out, d + 2 * count, count * 16, hipMemcpyDeviceToHost));
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
    DiagBuf buf;
    ZK_TRY(buf.alloc(device, count * k * sizeof(fe) + 32 * count));
    ZK_CHECK_HIP(hipMemcpy(buf.d, rows, count * k * 16, hipMemcpyHostToDevice));
    uint8_t *dout = buf.d + count * k * sizeof(fe);
    diag_blake3_elems(nullptr, (const fe *)buf.d, k, count, dout);
    ZK_CHECK_HIP(hipMemcpy(out, dout, 32 * count, hipMemcpyDeviceToHost));
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
    const size_t N = n * blowup;
    fe_ws ws[W];
    for (int c = 0; c < W; c++) ws[c] = make_fe_ws(fe_from_bytes(last + 16 * c));
    DiagBuf buf;
    const size_t o_lagr = (size_t)W * N * sizeof(fe), o_ws = o_lagr + N * sizeof(fe), o_leaves = o_ws + sizeof ws;
    ZK_TRY(buf.alloc(device, o_leaves + 32 * N));
    uint8_t *d = buf.d;
    ZK_CHECK_HIP(hipMemcpy(d, lde, o_lagr, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemcpy(d + o_lagr, lagr_lde, N * sizeof(fe), hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemcpy(d + o_ws, ws, sizeof ws, hipMemcpyHostToDevice));
    const VirtCols v{mask, (const fe_ws *)(d + o_ws), (const fe *)(d + o_lagr)};
    hash_rows_blocks(nullptr, (const fe *)d, W, ilog2(n), ilog2(blowup), 0, split, d + o_leaves, v);
    if (split < W / 4) hash_rows_blocks(nullptr, (const fe *)d, W, ilog2(n), ilog2(blowup), split, W / 4, d + o_leaves, v);
    ZK_CHECK_HIP(hipGetLastError());
    ZK_CHECK_HIP(hipMemcpy(leaves, d + o_leaves, 32 * N, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// GPU NTT of `batch` polys of size n: inverse != 0 -> interpolation (with 1/n), else evaluation
// over offset * <w_n> (offset given as 16 bytes; pass 1 for the plain subgroup)
extern "C" int zk_diag_ntt(int device, const uint8_t *in, size_t n, int batch, int inverse, const uint8_t *offset,
                           uint8_t *out) {
    if (!in || !out || n < 2 || (n & (n - 1)) || batch <= 0) ZK_FAIL(ZK_ERR_INVALID_ARG, "invalid argument");
    DiagProver p;
    ZK_TRY(p.open(device, std::max<size_t>(n, 16), 8));
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
    ZK_TRY(p.up(d_in, in, n * batch));
    fe inv_n = h_inv(fe_make(n));
    ntt(p->st, T, d_in, n, d_out, n, batch, inverse != 0, use_pre ? &pre : nullptr, inverse ? &inv_n : nullptr, d_tmp);
    return p.down(out, d_out, n * batch);
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
    DiagProver p;  // (sized for max(n, 16), the plan for n itself)
    ZK_TRY(p.open(device, std::max<size_t>(n, 16), blowup));
    Plan *pl = nullptr;
    ZK_TRY(get_plan(p, n, blowup, &pl));
    ZK_TRY(p.up(p->d_trace, in, (size_t)ncols * n));
    const fe *coeffs = p->d_trace;
    if (from_evals) {
        const fe inv_n = h_inv(fe_make(n));
        ntt(p->st, pl->Tn, p->d_trace, n, p->polys, n, ncols, true, nullptr, &inv_n, p->tmp);
        coeffs = p->polys;
    }
    // p->lde holds 28 * blowup * n elements, p->tmp 28 * 8 * n (a launch covers at most 8 cosets)
    ntt_lde(p->st, pl->Tn, pl->ct, coeffs, n, ncols, r0, rstride, ncos, p->lde, (size_t)ncos * n, n, p->tmp);
    return p.down(out, p->lde, (size_t)ncols * ncos * n);
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
    DiagProver p;
    ZK_TRY(p.open(device, n, 8, true));
    Plan *pl = p.pl;
    ZK_CHECK_HIP(hipMemsetAsync(p->d_trace, 0, (size_t)W * n * sizeof(fe), p->st));
    ZK_TRY(diag_class_flags(p));
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    ZK_TRY(p.up(p->d_trace + (size_t)c0 * n, cols, (size_t)ncols * n));
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
    ZK_TRY(p.down(flags_out, p->sp_nz, 4 * W));
    ZK_TRY(p.down(last_out, p->sp_last, W));
    if (how == 1) ZK_TRY(p.down(polys_out, p->polys + (size_t)c0 * n, (size_t)ncols * n));
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
    DiagProver p;
    ZK_TRY(p.open(device, n, blowup, true));
    ZK_TRY(p.up(p->d_trace, trace, (size_t)W * n));
    TraceSrc src;
    src.dev = p->d_trace;
    uint8_t root[32];
    ZK_TRY(trace_lde_commit(p, p.pl, src, n, root));
    ZK_TRY(d2h_flush(p));  // the root
    memset(flags_out, 0, 4 * W * sizeof(unsigned));
    if (p->tc.sp_used) ZK_TRY(p.down(flags_out, p->sp_nz, 4 * W));
    ZK_TRY(p.down(polys_out, p->polys, (size_t)W * n));
    ZK_TRY(p.down(lde_out, p->lde, (size_t)W * blowup * n));
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
    DiagProver p;
    ZK_TRY(p.open(device, n, blowup, true));
    Plan *pl = p.pl;
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
        ZK_TRY(p.down(polys_out + (size_t)k * n * 16, p->polys + c * n, n));
        ZK_TRY(p.down(lde_out + (size_t)k * B * n * 16, p->lde + c * B * n, B * n));
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
    DiagProver p;
    ZK_TRY(p.open(device, n, 8));
    uint8_t *d = nullptr;
    ZK_CHECK_HIP(p->arena.alloc(&d, packed_len));
    ZK_TRY(p.up(d, packed, packed_len));
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
    for (int k = 0; k < count; k++) ZK_TRY(p.down(out + (size_t)k * n * 16, p->d_trace + (size_t)col[k] * n, n));
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
// the assertion terms' constants of ext planes (coeff_b: ext x 22, bnd1: ext values) into K; false: one is not canonical
static bool diag_read_bnd(const uint8_t *coeff_b, const uint8_t *bnd1, int ext, AirConsts *K) {
    bool ok = true;
    for (int j = 0; j < ext; j++) {
        for (int k = 0; k < NUM_ASSERTS; k++) {
            K[j].coeff_b[k] = fe_from_bytes(coeff_b + 16 * (NUM_ASSERTS * j + k));
            ok = ok && fe_canonical(K[j].coeff_b[k]);
        }
        K[j].bnd1 = fe_from_bytes(bnd1 + 16 * j);
        ok = ok && fe_canonical(K[j].bnd1);
    }
    return ok;
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
static int diag_back_half_upload(DiagProver &p, int device, const uint8_t *tpolys, const uint8_t *cpolys, int ccols,
                                 size_t n, int ext) {
    ZK_TRY(p.open(device, n, 8, false, ext));
    ZK_TRY(p.up(p->polys, tpolys, (size_t)W * n));
    return p.up(p->cpolys, cpolys, (size_t)ccols * n);
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
    DiagProver p;
    ZK_TRY(diag_back_half_upload(p, device, tpolys, cpolys, ccols, n, ext));
    const Planes b = planes(p, ext);
    with_kx(ext, [&](auto kx) {
        typedef Chal<decltype(kx)::value> X;
        ood_eval(p->st, coeff_plain(p->polys, n), W, p->cpolys, ccols, ilog2(n), X::make(zv), X::make(zgv), b.ood_tab,
                 b.partials, p->ood, rank, G);
        return 0;
    });
    return p.down(out, p->ood, (size_t)ext * (2 * W + ccols));
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
    DiagProver p;
    ZK_TRY(diag_back_half_upload(p, device, tpolys, cpolys, ccols, n, ext));
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
        return p.down(out, Dk, (size_t)KX * n);
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
    if (ok && tpolys) ok = diag_read_bnd(coeff_b, bnd1, ext, K);
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
    DiagProver p;
    ZK_TRY(p.open(device, n, blowup, true, ext));
    const Planes b = planes(p, ext);
    ZK_TRY(p.up(b.comp, comp, (size_t)ext * 8 * n));
    if (tpolys) ZK_TRY(p.up(p->polys, tpolys, (size_t)W * n));
    uint8_t root[32];
    unsigned degree_flag = 0;
    ZK_TRY(composition_stage(p, p.pl, ext, ncols, b.comp, b.ctmp, b.clde, root, tpolys ? K : nullptr, nce));
    ZK_TRY(d2h_small(p, &degree_flag, p->flag, 4));
    ZK_TRY(d2h_flush(p));  // root and flag
    ZK_TRY(p.down(polys_out, p->cpolys, (size_t)ext * ncols * n));
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
    DiagProver p;
    ZK_TRY(p.open(device, n, 8, true, ext));
    Plan *pl = p.pl;
    const Planes b = planes(p, ext);
    const int log_n = pl->log_n;
    const size_t kg = n / parts, slice = (size_t)ncols * ext * kg;
    ZK_TRY(p.up(b.comp, comp, (size_t)ext * 8 * n));
    if (tpolys) ZK_TRY(p.up(p->polys, tpolys, (size_t)W * n));
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
    std::vector<fe> h((size_t)parts * slice);
    ZK_TRY(p.down(h.data(), out, h.size()));
    for (int g = 0; g < parts; g++)
        for (int c = 0; c < ncols * ext; c++)
            memcpy(polys_out + 16 * ((size_t)c * n + g * kg), &h[g * slice + (size_t)c * kg], kg * sizeof(fe));
    return p.down(flag_out, p->flag, 1);
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
    ok = diag_read_bnd(coeff_b, bnd1, ext, K) && ok;
    if (!ok) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_coeff_sources: canonical values, modes 0 .. 2, c non-zero");
    DiagProver p;
    ZK_TRY(p.open(device, n, 8, false, ext));
    ZK_TRY(p.up(p->polys, tplanes, (size_t)(W + 1) * n));  // (polys holds 32 planes)
    ZK_TRY(p.up(p->cpolys, cpolys, (size_t)ccols * n));
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
        ZK_TRY(p.down(raw.data(), p->ood, raw.size()));
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
        ZK_TRY(p.down(deep_out, Dk, (size_t)KX * n));
        ZK_CHECK_HIP(hipMemsetAsync(p->flag, 0, 4, p->st));
        ZK_CHECK_HIP(hipMemsetAsync(p->ctmp, 0, (size_t)KX * n * 16, p->st));
        for (int j = 0; j < KX; j++)
            boundary_poly_add(p->st, TS, wv, log_n, K[j], cv, p->dscratch, p->ctmp + (size_t)j * n, p->flag);
        ZK_TRY(p.down(col0_out, p->ctmp, (size_t)KX * n));
        return p.down(flag_out, p->flag, 1);
    });
}

// One FRI layer through commit_fri_layer and fri_fold_launch: `layer` holds L values as the
// kernels read them (over E planar: L a components, then L b components; lb > 0: coset-major over 2^lb cosets,
// FriLayout), folded by `fold` at `alpha` (16 bytes, 32 over E) with x_r = 3 w_L^r taken from the tables of a plan of
// N = L wstride points.  root_out: the layer's Merkle root (32 bytes; of a one-row layer, L = fold, the zero digest:
// commit_fri_layer); next_out: the L / fold folded values (planar).
extern "C" int zk_diag_fri_layer(int device, const uint8_t *layer, size_t L, int ext, int fold, int lb, size_t wstride,
                                 const uint8_t *alpha, uint8_t *root_out, uint8_t *next_out) {
    fe2 av;
    const size_t N = L * wstride;
    const bool ok = layer && alpha && root_out && next_out && (ext == 1 || ext == 2) &&
                    (fold == 2 || fold == 4 || fold == 8 || fold == 16) && L && !(L & (L - 1)) && wstride &&
                    !(wstride & (wstride - 1)) && (L >= 4 * (size_t)fold || L == (size_t)fold) && N >= 128 &&
                    N <= ((size_t)1 << 22) && lb >= 0 && ((size_t)1 << lb) <= L / fold;
    if (!ok || !diag_read_fe(alpha, ext, &av))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_fri_layer: L and wstride powers of two, 128 <= L wstride <= 2^22, fold 2 .. 16, "
                                    "at least 4 rows or the single row of an overfolded last layer, 2^lb <= L / fold, "
                                    "alpha canonical");
    DiagProver p;
    ZK_TRY(p.open(device, N / 8, 8, true, ext));
    const Planes b = planes(p, ext);
    const size_t rows = L / fold;
    uint8_t *leaves = p->fri_dig, *nodes = leaves + 32 * rows;
    // (the digests' area as a proof's later layers find it: not zero.  A one-row layer's root slot lies 32 bytes past
    // its 64 rows bytes, as in fri_lead_layers)
    ZK_CHECK_HIP(hipMemsetAsync(leaves, 0xA5, 64 * rows + 64, p->st));
    ZK_TRY(p.up(b.deep, layer, (size_t)ext * L));
    ZK_TRY(with_kx(ext, [&](auto kx) -> int {
        const auto F = fold_consts<decltype(kx)::value>(av, (uint32_t)fold);
        ZK_CHECK_HIP(hipMemcpy(b.fold_consts, &F, sizeof F, hipMemcpyHostToDevice));
        return ZK_OK;
    }));
    commit_fri_layer(p->st, ext, b.deep, L, fold, leaves, nodes, lb);
    fri_fold_launch(p->st, ext, b.deep, L, fold, b.fold_consts, p.pl->TN, wstride, b.fri, lb);
    ZK_TRY(p.down(root_out, nodes + 32, 32));
    return p.down(next_out, b.fri, (size_t)ext * rows);
}

// ---- the Merkle tree builder on leaves of the caller's choice (tests/test_gpu_merkle.py; the reference is
// tests/merkle_ref.py).  merkle_tree_cfg over nl 32-byte leaf digests (nl a power of two in [2, 2^24]) with the
// launcher's constants given: levels of at least 2^l3_min_log nodes through k_merge_level3_pf on at most pf_blocks
// blocks, the rest through k_merge_block with up to block_p threads (merkle_tree itself: 17, 2048, 512).  Checked here,
// not in the launcher: l3_min_log in [2, 62] (a level of fewer than 4 nodes gives the three-level kernel no group),
// pf_blocks in [1, 2^20], block_p a power of two in [1, 512].
// The heap lies between two guard regions of ZK_DIAG_MERKLE_GUARD bytes, the leaves after the upper one; guards and heap
// are filled with 0xA5 before the launches.  nodes_out: the heap, 32 nl bytes (slot 0, which no kernel writes, still
// 0xA5; node i at 32 i); guard_out: the lower guard, then the upper; leaves_out: the leaf buffer after the launches.  A
// store outside the heap's nodes thus comes back as a changed byte.
// positions != NULL: also the batch opening of the k positions, as zk_lde_query forms it (query_positions,
// batch_proof_bytes: the same refusals), into proof_out; *proof_len in: its capacity, out: the length.
constexpr size_t ZK_DIAG_MERKLE_GUARD = 4096;
extern "C" int zk_diag_merkle(int device, const uint8_t *leaves, size_t nl, int l3_min_log, uint32_t pf_blocks,
                              uint32_t block_p, uint8_t *nodes_out, uint8_t *guard_out, uint8_t *leaves_out,
                              const uint64_t *positions, size_t k, uint8_t *proof_out, size_t *proof_len) {
    if (!leaves || !nodes_out || !guard_out || !leaves_out || nl < 2 || (nl & (nl - 1)) || nl > ((size_t)1 << 24))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_merkle: nl a power of two in [2, 2^24]");
    if (l3_min_log < 2 || l3_min_log > 62 || pf_blocks < 1 || pf_blocks > (1u << 20) || block_p < 1 || block_p > 512 ||
        (block_p & (block_p - 1)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_merkle: l3_min_log in [2, 62], pf_blocks in [1, 2^20], block_p a power of two "
                                    "in [1, 512]");
    if (positions && !proof_len) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_merkle: positions without proof_len");
    std::vector<uint64_t> pos;
    if (positions) ZK_TRY(query_positions(positions, k, nl, pos));
    const size_t G = ZK_DIAG_MERKLE_GUARD, heap = 32 * nl;
    DiagBuf buf;  // lower guard, heap, upper guard, leaves
    ZK_TRY(buf.alloc(device, 2 * G + 2 * heap));
    uint8_t *d_nodes = buf.d + G, *d_leaves = buf.d + 2 * G + heap;
    ZK_CHECK_HIP(hipMemset(buf.d, 0xA5, 2 * G + heap));
    ZK_CHECK_HIP(hipMemcpy(d_leaves, leaves, heap, hipMemcpyHostToDevice));
    merkle_tree_cfg(nullptr, d_leaves, nl, d_nodes, MerkleCfg{l3_min_log, pf_blocks, block_p});
    ZK_CHECK_HIP(hipGetLastError());
    ZK_CHECK_HIP(hipMemcpy(nodes_out, d_nodes, heap, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(guard_out, buf.d, G, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(guard_out + G, d_nodes + heap, G, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(leaves_out, d_leaves, heap, hipMemcpyDeviceToHost));
    if (positions) ZK_TRY(batch_proof_bytes(nl, pos, d_leaves, d_nodes, proof_out, proof_len));
    return ZK_OK;
}

// The CE layout conversion (ce_layout) on values of the caller's choice, with the launcher's grid cap given: `in` holds
// 8 ext n elements, to_natural != 0: ext coset-major planes (plane[k][r n + q]) -> `out` in natural interleaved order
// (component k of element r + 8 q at element (r + 8 q) ext + k); to_natural = 0: the inverse.  n in [1, 2^22], not
// only the powers of two a proof has: a partial last tile is n mod 64 q-values.  max_blocks = 0: the launcher's own cap.
// The destination lies between two guard regions of ZK_DIAG_CE_GUARD bytes, all three filled with 0xA5 before the
// launch; guard_out: the lower guard, then the upper.
constexpr size_t ZK_DIAG_CE_GUARD = 4096;
extern "C" int zk_diag_ce_layout(int device, const uint8_t *in, size_t n, int ext, int to_natural, uint32_t max_blocks,
                                 uint8_t *out, uint8_t *guard_out) {
    if (!in || !out || !guard_out || n < 1 || n > ((size_t)1 << 22) || (ext != 1 && ext != 2) ||
        max_blocks > (1u << 20))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_ce_layout: n in [1, 2^22], ext 1 or 2, max_blocks at most 2^20");
    const size_t G = ZK_DIAG_CE_GUARD, bytes = (size_t)ext * 8 * n * sizeof(fe);
    DiagBuf buf;  // source, lower guard, destination, upper guard
    ZK_TRY(buf.alloc(device, 2 * bytes + 2 * G));
    uint8_t *d_dst = buf.d + bytes + G;
    ZK_CHECK_HIP(hipMemcpy(buf.d, in, bytes, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemset(buf.d + bytes, 0xA5, bytes + 2 * G));
    ce_layout(nullptr, (const fe *)buf.d, n, ext, to_natural != 0, (fe *)d_dst, max_blocks);
    ZK_CHECK_HIP(hipGetLastError());
    ZK_CHECK_HIP(hipMemcpy(out, d_dst, bytes, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(guard_out, d_dst - G, G, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(guard_out + G, d_dst + bytes, G, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// The bulk row read (rows_to_host: rows_layout chunk by chunk, then contiguous copies) on planes of the caller's
// choice: `planes` holds ncols * blowup * n elements, element (c, i) at (c*blowup + i mod blowup)*n + i div blowup; out
// takes rows (first + k) mod N, k < count, of ncols elements.  n in [1, 2^22], not only the powers of two an LDE has;
// blowup 8, 16, 32 or 64; ncols in [1, 28]; first < N; 1 <= count <= N + blowup.  max_blocks = 0: the launcher's own
// cap.  cap_rows: the rows the staging buffer holds, so small shapes cross chunk boundaries; 0: the 28 * 8 * n / ncols a
// prover of this size gives.  The staging buffer lies between two guard regions of ZK_DIAG_ROWS_GUARD bytes, all three
// filled with 0xA5 before the first launch; guard_out: the lower guard, then the upper.
constexpr size_t ZK_DIAG_ROWS_GUARD = 4096;
extern "C" int zk_diag_rows_layout(int device, const uint8_t *planes, size_t n, uint32_t blowup, int ncols, size_t first,
                                   size_t count, uint32_t max_blocks, size_t cap_rows, uint8_t *out,
                                   uint8_t *guard_out) {
    if (!planes || !out || !guard_out || n < 1 || n > ((size_t)1 << 22) || blowup < 8 || blowup > 64 ||
        (blowup & (blowup - 1)) || ncols < 1 || ncols > 28 || max_blocks > (1u << 20))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_rows_layout: n in [1, 2^22], blowup 8 .. 64, ncols in [1, 28], max_blocks at "
                                    "most 2^20");
    const size_t N = n * blowup;
    if (first >= N || count == 0 || count > N + blowup)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_rows_layout: first below N and 1 <= count <= N + blowup");
    if (!cap_rows) cap_rows = std::max<size_t>((size_t)W * 8 * n / ncols, 1);
    cap_rows = std::min(cap_rows, N);
    const size_t G = ZK_DIAG_ROWS_GUARD, src_bytes = (size_t)ncols * N * sizeof(fe),
                 stage_bytes = cap_rows * ncols * sizeof(fe);
    DiagBuf buf;  // source, lower guard, staging buffer, upper guard
    ZK_TRY(buf.alloc(device, src_bytes + stage_bytes + 2 * G));
    uint8_t *d_stage = buf.d + src_bytes + G;
    ZK_CHECK_HIP(hipMemcpy(buf.d, planes, src_bytes, hipMemcpyHostToDevice));
    ZK_CHECK_HIP(hipMemset(buf.d + src_bytes, 0xA5, stage_bytes + 2 * G));
    ZK_TRY(rows_to_host(nullptr, (const fe *)buf.d, ncols, n, blowup, first, count, (fe *)d_stage, cap_rows, out,
                        max_blocks));
    ZK_CHECK_HIP(hipGetLastError());
    ZK_CHECK_HIP(hipMemcpy(guard_out, d_stage - G, G, hipMemcpyDeviceToHost));
    ZK_CHECK_HIP(hipMemcpy(guard_out + G, d_stage + stage_bytes, G, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// One grind_launch over the nonces [start, start + count) with the result preset to ~0: *best_out = the smallest
// nonce whose BLAKE3(seed32 || nonce_le64) starts with >= bits trailing zero bits, ~0 when the window holds none.
extern "C" int zk_diag_grind(int device, const uint8_t *seed32, uint64_t start, uint32_t count, int bits,
                             uint64_t *best_out) {
    if (!seed32 || !best_out || count == 0 || bits < 0 || bits > 64 || start > UINT64_MAX - count)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_grind: count >= 1, 0 <= bits <= 64, start + count below 2^64");
    DiagProver p;
    ZK_TRY(p.open(device, 16, 8));
    ZK_CHECK_HIP(p->arena.alloc(&p->pow_seed, 8));
    ZK_CHECK_HIP(p->arena.alloc(&p->pow_best, 1));
    unsigned long long best = ~0ULL;
    ZK_TRY(p.up(p->pow_seed, seed32, 8));
    ZK_TRY(p.up(p->pow_best, &best, 1));
    grind_launch(p->st, p->pow_seed, start, count, bits, p->pow_best);
    ZK_TRY(p.down(&best, p->pow_best, 1));
    *best_out = best;
    return ZK_OK;
}

// ---------------------------------------------------------------- sharded proofs: agreement and validation windows
// The pure rule of shard_agree.hpp on caller-built records (world x 256 bytes, AgreeRecord's layout): the outcome, its
// text (empty when OK) and the outcome's code as the status.
extern "C" int zk_diag_agree(const uint8_t *records, int world, zk_agreement *out, char *msg, size_t cap) {
    if (!records || !out || world < 1 || world > 8) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_agree: records of 1 .. 8 ranks");
    std::vector<AgreeRecord> R((size_t)world);
    memcpy(R.data(), records, R.size() * sizeof(AgreeRecord));
    const Agreed A = agree(R.data(), world);
    *out = A.a;
    if (msg && cap) snprintf(msg, cap, "%s", A.msg.c_str());
    g_err = A.msg;
    return A.a.code;
}
// The window of rank g of G (val_window): out[3] = first, count, assertion mask
extern "C" int zk_diag_val_window(uint64_t n, int g, int G, uint64_t *out) {
    if (!out || G < 1 || g < 0 || g >= G || n < 16) ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_val_window: rank g < G, n >= 16");
    const ValWindow w = val_window(n, g, G);
    out[0] = w.first, out[1] = w.count, out[2] = w.amask;
    return ZK_OK;
}
// The merge of `world` validation partials (world x sizeof(ValPartial) bytes) of a trace of n rows into the report and
// status a sharded proof returns (validation_from_partials; the message in zk_last_error()).  No GPU.
extern "C" int zk_diag_merge_validation(const uint8_t *partials, int world, size_t n, const zk_pub_inputs *pub,
                                        zk_validation *out) {
    if (!partials || !pub || !out || world < 1 || world > 8 || n < 16)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_merge_validation: partials of 1 .. 8 ranks, n >= 16");
    std::vector<ValPartial> P((size_t)world);
    memcpy(P.data(), partials, P.size() * sizeof(ValPartial));
    return validation_from_partials(P.data(), world, n, pub, nullptr, 0, out);
}
// One window launch of the validator (validate_window_partial) on a prover of its own: steps first .. first + count - 1
// of the trace (28 x n column-major host bytes) with the assertions of amask.  packed = 0: the whole trace goes up and
// the window is read in place (ld = n), as a sharded proof reads a device trace; packed = 1: only rows first .. first +
// count of each column go up (ld = count + 1), as it uploads a host trace.  partial_out: sizeof(ValPartial) bytes.
extern "C" int zk_diag_validate_window(int device, const uint8_t *trace, size_t n, size_t first, size_t count,
                                       uint32_t amask, const zk_pub_inputs *pub, int packed, uint8_t *partial_out) {
    if (!trace || !pub || !partial_out) ZK_FAIL(ZK_ERR_INVALID_ARG, "null argument");
    if (n < 16 || (n & (n - 1)) || !count || first > n - 2 || count > n - 2 - first)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_validate_window: steps first .. first + count - 1 within 0 .. n - 3");
    if (((amask & ZK_ASSERT_ROW0) && first != 0) || ((amask & ZK_ASSERT_LAST) && first + count != n - 2) || (amask >> 22))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_validate_window: an assertion whose row the window does not hold");
    if (pub->lwe_size == 0 || pub->lwe_size > 5) ZK_FAIL(ZK_ERR_INVALID_ARG, "lwe_size must be in [1, 5]");
    DiagProver p;
    ZK_TRY(p.open(device, n, 8));
    const fe *win = p->d_trace + first;
    size_t ld = n;
    if (packed) {
        ld = count + 1;
        win = p->d_trace;
        for (int c = 0; c < W; c++) ZK_TRY(p.up(p->d_trace + (size_t)c * ld, trace + ((size_t)c * n + first) * sizeof(fe), ld));
    } else {
        ZK_TRY(p.up(p->d_trace, trace, (size_t)W * n));
    }
    ValPartial P;
    const int rc = validate_window_partial(p, win, ld, n, ValWindow{first, count, amask}, pub, 0, &P);
    memcpy(partial_out, &P, sizeof P);
    return rc;
}

// ---------------------------------------------------------------- sharded proofs: the degree check's merge and ranges
// The merge of `world` degree partials (world x sizeof(DegPartial) bytes) of a trace of n rows into the report and
// status a sharded degree check returns (degrees_from_partials; the message in zk_last_error()).  No GPU.
extern "C" int zk_diag_merge_degrees(const uint8_t *partials, int world, size_t n, zk_degrees *out) {
    if (!partials || !out || world < 1 || world > 8 || n < 16 || (n & (n - 1)))
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_merge_degrees: partials of 1 .. 8 ranks, n a power of two >= 16");
    std::vector<DegPartial> P((size_t)world);
    memcpy(P.data(), partials, P.size() * sizeof(DegPartial));
    return degrees_from_partials(P.data(), world, n, nullptr, 0, out);
}

// Steps 3 to 6 of a sharded degree check (shard.hip DegreesSharded) on quotient VALUES of the caller's choice, on one
// device in rank order, split into G = 2, 4 or 8 ranges exactly as G ranks split them.  quot: count <= 20 planes of 8n
// canonical values over the CE domain in transition_quotients' layout, quot[k 8n + r n + q] = Q_k(3 w_8n^r w_n^q).
// Rank s's planes (k, j) are cosets s Bl + j: its per-coset inverse transforms go to its own area [k Bl + j][n], the
// production pack kernel (k_sh_pack_coset, count Bl planes) fills its send area, the all-to-all is device copies
// (send area of s, chunk g -> receive area of g, chunk s), and per range g the production fused kernel
// (cross_degrees, max_blocks as given) fills a report of its own, which becomes partial g.  partials_out: G x
// sizeof(DegPartial); merged_out: the production merge's report (polynomials >= count read as zero); coeffs_out
// (optional: the fused kernel then writes coefficients): count x 8n elements, coefficient i of polynomial k at
// k 8n + i, assembled from the ranges' slices [k][k2][kl].  The status is the merge's (ZK_OK or ZK_ERR_DEGREES).
extern "C" int zk_diag_degrees_parts(int device, const uint8_t *quot, size_t n, int count, int G, uint32_t max_blocks,
                                     uint8_t *partials_out, zk_degrees *merged_out, uint8_t *coeffs_out) {
    bool ok = quot && partials_out && merged_out && n >= 16 && !(n & (n - 1)) && n <= ((size_t)1 << 20) && count >= 1 &&
              count <= NUM_TCONS && (G == 2 || G == 4 || G == 8) && n / (size_t)(G ? G : 1) >= 8;
    for (size_t i = 0; ok && i < (size_t)count * 8 * n; i++) ok = fe_canonical(fe_from_bytes(quot + 16 * i));
    if (!ok)
        ZK_FAIL(ZK_ERR_INVALID_ARG, "zk_diag_degrees_parts: 1 .. 20 planes of 8n canonical values, n a power of two in "
                                    "[16, 2^20], 2, 4 or 8 ranges of at least 8 coefficients");
    DiagProver p;
    ZK_TRY(p.open(device, n, 8, true));
    Plan *pl = p.pl;
    const int log_n = pl->log_n, Bl = 8 / G, planes = count * Bl;
    const size_t CE = 8 * n, kg = n / (size_t)G, area = (size_t)planes * n;  // area: one rank's planes, = count 8 kg
    fe *vals = p->tmp, *scratch = p->tmp + (size_t)NUM_TCONS * CE, *per = p->lde, *send = p->tmp, *recv = p->lde,
       *coeffs = p->tmp;
    ZK_TRY(p.up(vals, quot, (size_t)count * CE));
    for (int s = 0; s < G; s++)
        for (int k = 0; k < count; k++)
            ntt(p->st, pl->Tn, vals + (size_t)k * CE + (size_t)s * Bl * n, n, per + s * area + (size_t)k * Bl * n, n, Bl,
                true, nullptr, nullptr, scratch);
    for (int s = 0; s < G; s++) diag_pack_coset(p->st, per + s * area, n, log_n, planes, ilog2(kg), send + s * area);
    for (int g = 0; g < G; g++)
        for (int s = 0; s < G; s++)
            ZK_CHECK_HIP(hipMemcpyAsync(recv + g * area + (size_t)s * planes * kg, send + s * area + (size_t)g * planes * kg,
                                        (size_t)planes * kg * sizeof(fe), hipMemcpyDeviceToDevice, p->st));
    std::vector<DegPartial> parts((size_t)G);
    const fe scale = h_inv(fe_make(CE)), w8inv = h_inv(h_root_of_unity(3)), inv3n = h_inv(h_pow(fe_make(3), n));
    for (int g = 0; g < G; g++) {
        DegCrossMap m;
        m.c = recv + g * area;
        for (int r = 0; r < 8; r++) m.off[r] = ((size_t)(r / Bl) * planes + (size_t)(r % Bl)) * kg;
        m.cstride = (size_t)Bl * kg;
        m.k0 = (size_t)g * kg;
        m.kcount = kg;
        m.log_n = log_n;
        m.first = 0;
        m.count = count;
        m.coeffs = coeffs_out ? coeffs + g * area : nullptr;
        ZK_CHECK_HIP(hipMemsetAsync(p->deg_rep, 0, sizeof(DegReport), p->st));
        cross_degrees(p->st, m, pl->Tce, pl->inv3, scale, w8inv, inv3n, p->deg_rep, max_blocks);
        ZK_CHECK_HIP(hipGetLastError());
        DegReport R;
        ZK_TRY(d2h_small(p, &R, p->deg_rep, sizeof R));
        ZK_TRY(d2h_flush(p));
        DegPartial &P = parts[g];
        memset(&P, 0, sizeof P);
        P.version = ZK_AGREE_VERSION;
        P.rank = (uint32_t)g;
        P.first = (uint64_t)g * kg;
        P.count = kg;
        P.nonzero = R.nonzero;
        for (int k = 0; k < NUM_TCONS; k++) P.top[k] = R.top[k];
    }
    memcpy(partials_out, parts.data(), parts.size() * sizeof(DegPartial));
    if (coeffs_out) {
        std::vector<uint8_t> sl((size_t)count * CE * sizeof(fe));
        ZK_TRY(p.down(sl.data(), coeffs, (size_t)count * CE));
        for (int g = 0; g < G; g++)
            for (int k = 0; k < count; k++)
                for (int k2 = 0; k2 < 8; k2++)
                    memcpy(coeffs_out + 16 * ((size_t)k * CE + (size_t)k2 * n + (size_t)g * kg),
                           sl.data() + 16 * ((size_t)g * area + ((size_t)k * 8 + k2) * kg), 16 * kg);
    }
    return degrees_from_partials(parts.data(), G, n, nullptr, 0, merged_out);
}
