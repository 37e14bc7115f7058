// zk_internal.hpp -- shared declarations of the gfx950 prove path (kernels.hip, prover.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "chal.hpp"
#include "f128.hpp"

namespace zk {

static inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// ---------------------------------------------------------------- kernel profiler
// When enabled, every kernel launch is bracketed by a pair of HIP events on its own stream, so
// per-kernel device time is measured on the stream the kernel actually runs on.
struct KernelProfiler {
    bool on = false;
    struct Rec {
        const char *name;
        hipEvent_t a, b;
        double bytes;  // algorithmic HBM bytes of this launch (DESIGN.md "Roofline accounting")
        double muls, addsubs;  // algorithmic f128 multiplies / additions+subtractions (0 = not modelled)
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e;
            hipEventCreate(&e);
            pool.push_back(e);
        }
        return pool[used++];
    }
    void begin(hipStream_t st, const char *name, double bytes, double muls = 0, double addsubs = 0) {
        Rec r{name, get(), nullptr, bytes, muls, addsubs};
        hipEventRecord(r.a, st);
        recs.push_back(r);
    }
    void end(hipStream_t st) {
        recs.back().b = get();
        hipEventRecord(recs.back().b, st);
    }
    void reset() {
        recs.clear();
        used = 0;
    }
};
KernelProfiler &profiler();
// ZK_PROF with the launch's algorithmic f128 operation counts (for the VALU roofline)
#define ZK_PROF_OPS(st, name, bytes, muls, addsubs, ...)                               \
    do {                                                                             \
        ::zk::KernelProfiler &P_ = ::zk::profiler();                                 \
        if (P_.on) P_.begin(st, name, (double)(bytes), (double)(muls), (double)(addsubs)); \
        __VA_ARGS__;                                                                 \
        if (P_.on) P_.end(st);                                                       \
    } while (0)
#define ZK_PROF(st, name, bytes, ...)        \
    do {                                     \
        ::zk::KernelProfiler &P_ = ::zk::profiler(); \
        if (P_.on) P_.begin(st, name, (double)(bytes)); \
        __VA_ARGS__;                         \
        if (P_.on) P_.end(st);               \
    } while (0)

// ---------------------------------------------------------------- twiddle plans
// Every power table the kernels need for one NTT size n, resident in HBM.
//   dft_fwd / dft_inv : w_4096^t, t < 2048  (DFT stages of the in-LDS engine; smaller sizes stride)
//   big_lo / big_hi   : w_n^t = big_lo[t & 2047] * big_hi[t >> 11]  (inter-pass twiddles, x values)
struct NttTables {
    int log_n = 0;
    fe *dft_fwd = nullptr, *dft_inv = nullptr;
    fe_ws *dft_fwd_ws = nullptr, *dft_inv_ws = nullptr;  // their W sets (f128.hpp fe_mul_uniform)
    fe_w2 *dft_fwd_w2 = nullptr, *dft_inv_w2 = nullptr;  // and two-part forms (f128.hpp fe_mul_w2)
    fe *fwd_lo = nullptr, *fwd_hi = nullptr, *inv_lo = nullptr, *inv_hi = nullptr;
    // four-step inter-pass twiddles w^(j2*k1) laid out as pass 1 consumes them, [k1 * n2 + j2]
    // (n elements each; only for log_n > 12, else null)
    fe *fwd_pass = nullptr, *inv_pass = nullptr;
    // optional: inv_pass * n^-1, used when an inverse NTT is post-scaled by n^-1 (interpolation): the
    // scale rides on the pass-1 twiddle instead of costing a multiply per element in pass 2
    fe *inv_pass_n = nullptr;
    fe inv_n = {0, 0};
};
// Four-step split of a size-2^L NTT (L > 12): log2 of the pass-1 line length n2 (pass-2 lines are
// n1 = 2^(L - log_n2)).  Pass 1 reads strided and writes contiguous runs; pass 2 reads and writes
// LPB-element row segments at stride n2, so pass 2 gets the shorter lines when the split is uneven:
// at L = 22 the balanced 11/11 split leaves pass 2 with 32-B segments (2 lines of 2048 per
// 4096-element tile) and an extra radix-2 LDS stage; 12/10 gives it the 64-B segments of 2^20.
// Every table builder and the NTT dispatcher use this one function, so they always agree.
// (the balanced ceil(L/2) split measured slower at 2^22: DESIGN.md "NTT")
int ntt_log_n2(int L);
// fill NttTables::fwd_pass / inv_pass (allocated by the caller, n elements each)
void make_pass_twiddles(hipStream_t st, NttTables &T);
// out[k1*n2 + j2] = s^k1 * fwd_pass[k1*n2 + j2] (s^t from split tables): CosetTables::pass of one coset
void coset_pass_tables(hipStream_t st, const fe *s_lo, const fe *s_hi, const fe *fwd_pass, int log_n, int log_n2,
                       fe *out);

// A power series s^k, k < n, as split tables (s^k = lo[k & 2047] * hi[k >> 11])
struct PowTable {
    fe *lo = nullptr, *hi = nullptr;  // s^t = lo[t & 2047] * hi[t >> 11]
    fe *full = nullptr;               // optional s^t for every t < n (one multiply less per use)
};
// out[t] = lo[t & 2047] * hi[t >> 11] for t < n
void pow_expand(hipStream_t st, const fe *lo, const fe *hi, size_t n, fe *out);

// Sparse columns of a trace batch: column c (flags at nz[col0 + c]) is zero in every row but the last when
// nz[col0 + c] == 0 (sparse_detect); then its interpolation is last[col0 + c] * lagr (the interpolant of e_(n-1))
// and its coset LDE last * lagr_lde (coset r at r n): the NTT passes skip its DFTs.  Four-step sizes only.
struct SparseCols {
    const unsigned *nz;
    const fe *last;
    const fe *lagr, *lagr_lde;
    int col0;
    // width flags (sparse_detect only): wstride > 0 sets nz[wstride + c] when column c has an entry of 8 bits or more
    // and nz[2 wstride + c] when one of 32 bits or more (last row excluded) -- the next proof's narrow-upload hint
    int wstride = 0;
    // fused: the interpolation's pass 1 writes the flags (nz, and with wstride the width flags) of the columns it
    // reads and skips none; the coset LDE then skips none either (host-resident traces once the hints are learned:
    // no separate detection pass over the uploaded columns)
    bool fused = false;
    // all: the host knows every column of the call is sparse (the hinted columns of a host trace): no transform is
    // launched, one streaming pass writes last * fill into every column (k_sparse_fill)
    bool all = false;
    // idoff > 0: column 0 is also checked for being the AIR clock (rows 0 .. n-2 hold 0 .. n-2; nz[idoff] = 1 when it
    // is not); such a column transforms to id + (last - (n-1)) * fill (id_poly / id_lde: the identity column's
    // interpolant and coset LDE, like lagr / lagr_lde) and skips its DFTs like a sparse one
    const fe *id_poly = nullptr, *id_lde = nullptr;
    int idoff = 0;
    // the cosets lagr_lde / id_lde hold: coset r at slot (r - lde_r0) >> lde_shift (Plan::lde_slot)
    int lde_r0 = 0, lde_shift = 0;
};
void sparse_detect(hipStream_t st, const fe *trace, size_t n, int c0, int nc, const SparseCols &sp);
void sparse_detect_rows(hipStream_t st, const fe *trace, size_t n, int c0, int nc, const SparseCols &sp, size_t r0,
                        size_t r1);
// Narrow trace columns uploaded packed (zk_prove from host columns): column col[k]'s rows 0 .. n-2 as width[k]-byte
// integers (1 or 4) at src + off[k], its last row last[k]; written out as field elements into trace column col[k].
struct NarrowCols {
    int count;
    int col[28];
    int width[28];
    size_t off[28];
    fe last[28];
};
void expand_narrow(hipStream_t st, const uint8_t *src, const NarrowCols &nc, size_t n, fe *trace);

// NTT of `batch` polynomials of size 2^log_n, each at in + b*in_stride -> out + b*out_stride.
//   inverse     : use w^-1 (no 1/n scale; fold it into post_scale)
//   pre         : optional s^k pre-scale of input coefficient k (coset evaluation), may be null
//   post_scale  : optional constant multiplied into every output (e.g. 1/n)
// in and out must not alias.  tmp must hold batch * n elements when log_n > 12.
// sp (optional, interpolations with post_scale = 1/n only): sparse columns of the batch (SparseCols)
void ntt(hipStream_t st, const NttTables &T, const fe *in, size_t in_stride, fe *out, size_t out_stride,
         int batch, bool inverse, const PowTable *pre, const fe *post_scale, fe *tmp, const SparseCols *sp = nullptr);

// Coset-LDE tables of one plan (LDE coset r < B, s_r = 3 w_N^r):
//   n <= 4096 (single pass): full[r*n + k] = s_r^k (input pre-scale)
//   four-step (n = n1*n2):   stage[r*4096 + h + j] = c_r^(n2/2h) w_2h^j, c_r = s_r^n1 (DIT stage twiddles of
//                            the pass-1 line DFT over the coset c_r <w_n2>), pass[r*n + k1*n2 + j2] = (s_r w_n^j2)^k1
struct CosetTables {
    fe *full = nullptr, *stage = nullptr, *pass = nullptr;
    fe_ws *stage_ws = nullptr;  // W sets of `stage` (four-step plans)
    fe_w2 *stage_w2 = nullptr;  // two-part forms of `stage`
};
// Forward coset LDE: for columns c < ncols (at in + c*in_stride) and coset slots j < ncos (coset r0 + j*rstride),
// the n evaluations over coset r to out + c*out_cstride + j*out_jstride.  tmp: ncols*min(ncos, 8)*n
// (four-step; launches of up to 8 cosets).
void ntt_lde(hipStream_t st, const NttTables &T, const CosetTables &CT, const fe *in, size_t in_stride, int ncols,
             int r0, int rstride, int ncos, fe *out, size_t out_cstride, size_t out_jstride, fe *tmp,
             const SparseCols *sp = nullptr);
// out[i] = F[i] + d * L[i] for i < cnt (d given by its W set)
void axpy_fill(hipStream_t st, const fe *F, const fe *L, const fe_ws &d, size_t cnt, fe *out);

// grinding: atomicMin into *best_dev of the nonces in [start, start+count) with >= bits trailing zeros
void grind_launch(hipStream_t st, const uint32_t *seed_dev, uint64_t start, uint32_t count, int bits,
                  unsigned long long *best_dev);

// ---------------------------------------------------------------- hashing
// leaf[i] = BLAKE3(row i) for natural LDE index i < N = B*n of a coset-major column set:
// element (column c, index i) lives at base[(c*B + i%B)*n + i/B].
// leaves (N x 32 B) and the heap-ordered Merkle tree nodes[1..N) of coset-major rows / FRI layer rows
// leaf digests of the rows of LDE cosets r0 .. r0 + 2^log_rc - 1 (coset-major columns), natural leaf order
void hash_rows_cosets(hipStream_t st, const fe *base, int ncols, int log_n, int log_b, int r0, int log_rc,
                      uint8_t *leaves);
void commit_rows_coset_major(hipStream_t st, const fe *base, int ncols, int log_n, int log_b, uint8_t *leaves,
                             uint8_t *nodes);
// blocks b0 .. b1 - 1 of the leaf hashes of all B n rows of a coset-major column set of ncols (a multiple of 4,
// <= 64) columns: columns 4 b .. 4 b + 3 compressed into the chaining value each leaf slot carries between launches
// Virtual trace columns (host traces, trace_commit.hip): sparse columns whose LDE is never written; the row hashing forms
// column c's value at LDE point (coset r, position q) as last[c] * lagr_lde[r n + q], last[c] the column's last row.
// last_ws[c] = make_fe_ws(last[c]): the value is uniform over the launch, so the product goes through
// fe_mul_uniform, as in fixed_hash
struct VirtCols {
    uint32_t mask = 0;
    const fe_ws *last_ws = nullptr;
    const fe *lagr_lde = nullptr;
};
void hash_rows_blocks(hipStream_t st, const fe *base, int ncols, int log_n, int log_b, int b0, int b1, uint8_t *leaves,
                      VirtCols virt = VirtCols());
// Blocks 0 .. nb - 1 of every row (IV, then as hash_rows_blocks(0, nb)) with the columns' LDE formed in the same pass:
// per column c < 4 nb
//   FORM        lde column c = src[c] + ws_dev[wsi[c]] * lagr_lde  (src[c]: a coset-major plane of B n), stored and hashed
//   FORM_NOSRC  lde column c = ws_dev[wsi[c]] * lagr_lde, stored and hashed
//   LOAD        lde column c is already written: hashed only
// (the fixed / preprocessed columns and the clock: trace_commit.hip, prover.hip fixed_prefix).  ncols as hash_rows_blocks.
struct FixedHashCols {
    enum : uint8_t { FORM = 0, FORM_NOSRC = 1, LOAD = 2 };
    static constexpr int MAXC = 28;  // the trace width: 7 blocks
    const fe *src[MAXC];
    uint8_t wsi[MAXC];
    uint8_t mode[MAXC];
};
void fixed_hash(hipStream_t st, const FixedHashCols &A, const fe *lagr_lde, const fe_ws *ws_dev, fe *lde, int ncols,
                int log_n, int log_b, int nb, uint8_t *leaves);
// Where the consumers that are linear in the trace polynomials (ood_eval, deep_poly, boundary_poly_add) read trace
// column c's n coefficients.  A column formed as base_c + w_c e_(n-1) (the derived clock, the fixed class, the hinted
// sparse columns of a host trace: trace_commit.hip) is read at its source, the sum never written:
//   PLAIN  plane[c][k]
//   BASE   plane[c][k] + w_c lagr[k]
//   ZERO   w_c lagr[k]  (no plane)
// lagr: e_(n-1)'s coefficients, read once per consumer with the w_c folded into one scalar per linear combination; null
// when every column is PLAIN.  The scalars w_c are the caller's (host values, passed beside the table).
struct CoeffSrc {
    enum : uint8_t { PLAIN = 0, BASE = 1, ZERO = 2 };
    static constexpr int MAXC = 28;
    const fe *plane[MAXC];
    uint8_t mode[MAXC];
    const fe *lagr;
    bool derived(int c) const { return mode[c] != PLAIN; }
};
// every column PLAIN over ncols (<= 28) column-major planes of n coefficients: the consumers behave as without a table
inline CoeffSrc coeff_plain(const fe *tpolys, size_t n, int ncols = CoeffSrc::MAXC) {
    CoeffSrc S{};
    for (int c = 0; c < ncols; c++) S.plane[c] = tpolys + (size_t)c * n;
    return S;
}

// Storage of a FRI layer of L values: natural order (lb = 0), or coset-major over 2^lb cosets of 2^lcn
// points (natural index i at (i mod 2^lb) 2^lcn + i / 2^lb): layer 0 as the DEEP coset LDE leaves it
struct FriLayout {
    int lb, lcn;
};
FriLayout fri_layout(size_t L, int lb);
// nodes[1..nl) of a binary Merkle tree over nl leaves (nodes[nl/2..nl) = merges of leaf pairs)
// nl a power of two.  With nl = 1 nothing is launched and no node is written.  Two callers can pass 1: the sharded
// upper tree (dist_commit: Q / 2 leaves, Q >= G >= 2), whose one leaf sits at nodes + 32 and so is the root already;
// and commit_fri_layer for a one-row layer, whose leaf does not, and which therefore sets the root itself.  The trace
// and composition trees have n blowup >= 128 leaves.
void merkle_tree(hipStream_t st, const uint8_t *leaves, size_t nl, uint8_t *nodes);
// merkle_tree with its launch constants as arguments: levels of at least 2^l3_min_log nodes take the three-level kernel
// on a grid of at most pf_blocks blocks, the rest blocks of up to block_p threads (production: 17, 2048, 512).  The
// kernels need l3_min_log >= 2, pf_blocks >= 1 and block_p a power of two in [1, 512]; the caller sees to that.
struct MerkleCfg {
    int l3_min_log;
    unsigned pf_blocks;
    unsigned block_p;
};
void merkle_tree_cfg(hipStream_t st, const uint8_t *leaves, size_t nl, uint8_t *nodes, MerkleCfg cfg);
// out[k] = src[idx[k]] for 32-byte digests
// out[t] = the 16 bytes at device address addr[t] (query openings: LDE values and Merkle digests)
constexpr size_t ZK_GATHER_CAP = 1 << 17;
void gather_chunks(hipStream_t st, const uint64_t *addr, size_t k, fe *out);
// Up to ZK_COPY_LIST_MAX device -> pinned-host copies (32-bit words) in one launch: blockIdx.y picks
// the entry.  dst must be host memory from hipHostMalloc (device-accessible, coherent).
constexpr int ZK_COPY_LIST_MAX = 32;
struct CopyList {
    int n;
    const uint32_t *src[ZK_COPY_LIST_MAX];
    uint32_t *dst[ZK_COPY_LIST_MAX];
    uint32_t words[ZK_COPY_LIST_MAX];
};
hipError_t copy_to_host(hipStream_t st, const CopyList &L, size_t max_words);
void gather_digests(hipStream_t st, const uint8_t *src, const uint64_t *idx, size_t k, uint8_t *out);
// out[q*ncols + c] = element (c, pos[q]) of a coset-major column set
void gather_rows(hipStream_t st, const fe *base, int ncols, int log_n, int log_b, const uint64_t *pos, size_t k,
                 fe *out);

// ---------------------------------------------------------------- AIR / composition
struct AirConsts {
    fe coeff_t[20];
    fe coeff_b[22];
    int assert_col[22];
    int assert_grp[22];  // 0: step 0, 1: step n-2
    fe assert_val[22];
    fe inv_zn[8];   // 1 / (x^n - 1) on the 8 CE cosets
    fe xr[8];       // 3 * w_CE^r
    fe g_last2, g_last1;
    fe delta;
    fe bnd1;  // sum_k coeff_b[12+k] * assert_val[12+k]: the step n-2 group's values, subtracted once per row
    int lwe_size;
    // pv[j] = sum_r (-coeff_t[12+r]) periodic[j][1+r] over the 128 CE steps j = i mod 128: the round constants' share
    // of constraints 12..15, folded with this plane's coefficients (air_fold_periodic)
    fe pv[128];
    // W sets (f128.hpp make_fe_ws) of every launch-uniform multiplier of k_eval_constraints, read there by scalar
    // loads; built by air_build_ws once the coefficients are set.  Indices: EvalWs.
    fe_ws ws[50];
};
// AirConsts::ws[...]: EW_CT + k = coeff_t[k], but for k = 12..15 coeff_t[k] 3^-72 (the adjugate path's cubes carry
// 3^72); EW_NCT + r = -coeff_t[12 + r], r < 2 (the opcode and push terms); EW_U + k = air_fold_mds(coeff_t + 12, k);
// EW_D89 = coeff_t[9] - coeff_t[8]; EW_DELTA = delta; EW_CB + k = coeff_b[k]
enum EvalWs { EW_CT = 0, EW_NCT = 20, EW_U = 22, EW_D89 = 26, EW_DELTA = 27, EW_CB = 28, EW_COUNT = 50 };
static_assert(EW_COUNT == sizeof(AirConsts::ws) / sizeof(fe_ws), "AirConsts::ws holds one W set per EvalWs index");
// (kernels.hip, beside the kernel that reads them; needs coeff_t, coeff_b and delta)
void air_build_ws(AirConsts &K);
// |MDS| of the Rescue round (crypto/src/rescue.rs:197-214): row r = (-a, +b, -c, +d), every entry below 2^26
ZK_HD uint32_t mds_abs(int i) {
    constexpr uint32_t M[16] = {729, 1080, 390, 40, 29160, 42471, 14520, 1210,
                                882090, 1277640, 429429, 33880, 24698520, 35708310, 11935560, 925771};
    return M[i];
}
// Constraints 12..15 are ct_r (v_r - m0_r) with m0_r = (MDS x)_r + ark_r (+ opcode, + push) linear in the cubes x: their
// linear half sum_r (-ct_r) m0_r is folded per proof into u_k = sum_r (-ct_r) MDS[r][k] and the table pv above, so a row
// pays four products u_k x_k and no MDS row.  ct = coeff_t + 12.  (Four 128 x 26-bit products stay below 2^160.)
ZK_HD fe air_fold_mds(const fe *ct, int k) {
    acc160 a = acc160_zero();
    for (int r = 0; r < 4; r++) acc160_madd(a, ct[r], mds_abs(4 * r + k));
    const fe s = acc160_reduce(a);  // column k is negative for even k: (-ct_r)(-|M|) = ct_r |M|
    return (k & 1) ? fe_neg(s) : s;
}
// per: the 128 x 9 table of the periodic columns over the CE steps (the evaluator's `periodic`, on the host)
inline void air_fold_periodic(const fe *ct, const fe *per, fe pv[128]) {
    const fe nct[4] = {fe_neg(ct[0]), fe_neg(ct[1]), fe_neg(ct[2]), fe_neg(ct[3])};
    for (int j = 0; j < 128; j++) {
        fe s = fe_zero();
        for (int r = 0; r < 4; r++) s = fe_add(s, fe_mul(nct[r], per[9 * j + 1 + r]));  // (host fe_mul: ~5 ns)
        pv[j] = s;
    }
}
// inverse of (x - a) * (x - b) over the B cosets, written coset-major: out[r*n + q] for the point
// x = xr[r] * w_n^q (natural domain index i = r + B*q)
void batch_inv_pairs(hipStream_t st, const NttTables &Tn, const fe *xr, int log_b, int log_n, fe a, fe b,
                     fe *out);
struct Fe8 {
    fe v[8];
};
// The evaluator's per-row divisor factors over 2^log_cos cosets (offsets xr, coset-major, planes of
// P = 2^(log_cos + log_n)): out[i] = (x - g2)(x - g1) inv_zn[coset], out[P + i] = 1/(x - 1),
// out[2P + i] = 1/(x - g2); inv_zn[c] = 1/(xr[c]^n - 1).  3P elements.
void divisor_tables(hipStream_t st, const NttTables &Tn, const fe *xr, int log_cos, int log_n, fe g1, fe g2,
                    const Fe8 &inv_zn, fe *out);
// Which CE cosets one launch evaluates: local coset jl < nce is global CE coset ce0 + cestep*jl, and its
// LDE rows are LDE coset slot jl << lshift of a buffer holding lde_cosets cosets per column.  dplane: the stride of
// the divisor tables' planes (0: nce * n, the launch's own cosets; a launch over one coset of several passes theirs).
struct EvalMap {
    int nce, ce0, cestep, lshift, lde_cosets;
    size_t dplane = 0;
};
// Rescue MDS / inverse-MDS __constant__ tables on the current device (once per device; thread-safe).
// zk_prover_create calls it; the evaluator launches check it again (the plug point may run first).
hipError_t upload_rescue_consts(hipStream_t st);
// the map of a launch over a whole LDE of blowup 2^log_b: CE cosets 0 .. nce-1 (8: all; 7: the composition stage
// derives the last one, bnd = false; with bnd always 8)
EvalMap eval_map_whole(int log_b, int nce, bool bnd);
// Composition evaluations over the CE cosets of `map`, written coset-major: comp[jl*n + q].  KX coefficient planes
// (chal.hpp): consts = {a components} or, KX = 2, {a components, b components}, the b plane written at comp + plane.
// bnd: the boundary (assertion) terms are evaluated per row (else: boundary_poly_add after interpolation)
hipError_t eval_constraints(hipStream_t st, int KX, const fe *lde, int log_n, EvalMap map, const fe *periodic,
                            const fe *divs, const AirConsts *consts, size_t plane, fe *comp, bool bnd);
// The project's own soundness checks, trace validation and transition constraint degrees: three kernels over one plain
// reading of the 20 transition constraints (kernels.hip transition_constraints), apart from eval_constraints' tuned one.
// Trace validation (kernels.hip k_validate_trace; zk_validate_device): the device report of one launch.  The host
// initialises it in-stream: counts 0, firsts UINT64_MAX, a_mask 0 and a_found[k] = the value assertion k asserts
// (get_assertions order, air/src/lib.rs:170-195), which the kernel replaces with the asserted cell's value.
struct ValReport {
    unsigned long long t_count[20];  // per transition constraint: steps s < n - 2 where it is non-zero
    unsigned long long t_first[20];  // the lowest such step
    unsigned long long failing_steps;
    unsigned a_mask, pad_;
    fe a_found[22];
};
static_assert(sizeof(ValReport) < 1024, "the validation report stays a small transfer");
// per_tab: the raw periodic table, 16 rows of CYCLE_MASK || 8 round constants (air/src/lib.rs:201-225); trace:
// 28 x n column-major, n >= 16
hipError_t validate_trace(hipStream_t st, const fe *trace, size_t n, const fe *per_tab, fe delta, int lwe_size,
                          ValReport *rep);
// The windowed form: steps first .. first + count - 1 (global) of a trace whose columns are ld elements apart, win[c ld +
// i] = row first + i of column c, i <= count (count + 1 rows; ld >= count + 1, count >= 1).  amask: the assertions
// checked (bit k; row-0 cells at window index 0, row n - 2 cells at window index count).  Reported steps are global.
hipError_t validate_window(hipStream_t st, const fe *win, size_t ld, size_t first, size_t count, unsigned amask,
                           const fe *per_tab, fe delta, int lwe_size, ValReport *rep);
// Transition constraint degrees (kernels.hip k_transition_quotients, k_poly_degrees; zk_degrees_device).
// transition_quotients: quot[k 8n + jl n + q] = C_k / D at CE row (jl, q) of `map` for the 20 constraints k of
// evaluate_transition, the values validate_trace tests for zero, no coefficients; lde, periodic and divs (plane 0 of
// divisor_tables) as eval_constraints.
hipError_t transition_quotients(hipStream_t st, const fe *lde, int log_n, EvalMap map, const fe *periodic,
                                const fe *divs, fe delta, int lwe_size, fe *quot);
// top[k]: the highest non-zero coefficient index of polynomial k; nonzero bit k: it has one.  Zeroed in-stream.
struct DegReport {
    unsigned long long top[20];
    unsigned nonzero, pad_;
};
// polys: count (<= 20) polynomials of len coefficients each, one after the other
void poly_degrees(hipStream_t st, const fe *polys, size_t len, int count, DegReport *rep);
// Inputs of the cross-coset step for coefficients k0 .. k0+kcount: c[r][kl] = c_r[k0 + kl]; output
// polys[k2 * pstride + kl].
struct CrossMap {
    const fe *c[8];
    size_t k0, kcount, pstride;
    // derive7: coset 7 was not evaluated (c[7] unused).  A composition polynomial of degree < 7n has a zero
    // top block, b_7 = sum_r w8^(7r) ... = 0, which fixes d_7 = sum_{r<7} k7[r] d_r with k7[r] = -w_8^(r+1).
    int derive7 = 0;
    fe k7[7] = {};
};
// add the boundary terms' quotient polynomial (one coefficient plane K) into col0 (n coefficients);
// c = g^(n-2); scratch: DeepScratch (KX = 1); sets *flag when an assertion fails.  S: the trace coefficients' sources;
// w: the 28 scalars w_c of its BASE and ZERO columns (host; may be null when every column is PLAIN)
void boundary_poly_add(hipStream_t st, const CoeffSrc &S, const fe *w, int log_n, const AirConsts &K, fe c, fe *scratch,
                       fe *col0, unsigned *flag);
// boundary_poly_add split over a sharded rank's coefficient range [k0, k0 + kn) (kn a multiple of
// ZK_DEEP_RANGE_QUANTUM): begin -> the range's 2 sums on the device; end adds the quotient's range into col0
// (global index) given ext = the sums of every later range.  The remainder flag is raised by the rank with k0 = 0.
const fe *boundary_range_begin(hipStream_t st, const CoeffSrc &S, const fe *w, int log_n, const AirConsts &K, fe c,
                               fe *scratch, size_t k0, size_t kn);
void boundary_range_end(hipStream_t st, int log_n, fe c, fe *scratch, size_t k0, size_t kn, const fe *ext, fe *col0,
                        unsigned *flag);
// cross-coset step of the size-8n interpolation: per k1 < n, from the 8 per-coset inverse NTTs
// (c_r[k1]), produce coefficients a[k1 + n*k2] = 3^-(k1+n k2) / (8n) * sum_r w8^(-r k2) w_8n^(-r k1) c_r[k1]
// and write column k2 < ncols of the segmented composition polynomial, for the k1 range of the CrossMap.
void comp_cross_mapped(hipStream_t st, const CrossMap &m, const NttTables &T8n, const PowTable &inv3, fe scale,
                       fe w8inv, fe inv3n, int ncols, fe *polys, unsigned *nonzero_flag);
// The cross-coset step of a batch of `count` (<= 20) polynomials over the coefficient range k0 .. k0 + kcount, fused
// with the degree scan (a sharded degree check: shard.hip DegreesSharded).  Inputs: c_r[k0 + kl] of polynomial k at
// c[off[r] + k cstride + kl].  rep (zeroed in-stream): top[first + k] takes the highest GLOBAL index k1 + n k2 whose
// coefficient is non-zero, bit first + k of nonzero that there is one.  coeffs = null: no coefficient is written (nor
// scaled: the scale is non-zero).  Else coefficient k1 + n k2 of polynomial k goes to coeffs[((first + k) 8 + k2)
// kcount + kl], bit-identical to comp_cross_mapped's.  max_blocks: the grid's x extent (0: the default), past which
// a block strides.
struct DegCrossMap {
    const fe *c;
    size_t off[8], cstride;
    size_t k0, kcount;
    int log_n, first, count;
    fe *coeffs;
};
void cross_degrees(hipStream_t st, const DegCrossMap &m, const NttTables &T8n, const PowTable &inv3, fe scale, fe w8inv,
                   fe inv3n, DegReport *rep, unsigned max_blocks = 0);

// ---------------------------------------------------------------- OOD / DEEP / FRI
// Written once over the challenge field (chal.hpp): KX = 1 the base field, KX = 2 FieldExtension::Quadratic.  A
// launcher that gets the point z takes its KX from z's type (fe or fe2); the FRI launchers, which get no point, take
// KX as an argument.  What KX = 2 means for the buffers:
//   * every E-valued buffer another stage reads is planar, component a at [0, M) and b at [M, 2M): the OOD partial sums
//     (M = np nw) and frame (M = np), the DEEP coefficients (M = n) and their LDE (M = N), a FRI layer (M = L);
//   * the composition columns stay base columns: E column j is P_2j + X P_2j+1, so the OOD `C` counts 2 C base columns
//     while DEEP's `ccols` counts the C E columns it pairs them into;
//   * constants in device memory (DeepConsts, FoldConsts) hold E values as (a, b) pairs.
//
// OOD frame in one pass: out = [T_c(z)]_W ++ [T_c(zg)]_W ++ [H_j(z)]_C, np = 2W + C values (KX planes of np).
// tab: KX (128 + 2 ood_waves(n)) elements, partials: KX np ood_waves(n) elements of scratch.
// (rank, G): only this rank's share of the coefficient range (waves [rank nw / G, (rank + 1) nw / G)), so that the G
// partial sums of each value add up to it (the sharded prover all-gathers them); (0, 1) = the whole range
// S: the trace coefficients' sources (W <= 28 columns).  With BASE or ZERO columns (S.lagr set) e_(n-1) is evaluated as
// one more polynomial: out then holds KX planes of np + 2 values, e(z) and e(zg) last, a BASE column's slots its base's
// values and a ZERO column's slots zero; ood_fold_sources makes the frame of them on the host.
int ood_waves(size_t n);
template <class T>
void ood_eval(hipStream_t st, const CoeffSrc &S, int W, const fe *cpolys, int C, int log_n, T z, T zg, fe *tab,
              fe *partials, fe *out, int rank = 0, int G = 1);
// values per plane of ood_eval's output
inline int ood_out_values(const CoeffSrc &S, int W, int C) { return 2 * W + C + (S.lagr ? 2 : 0); }
// Host: ood_eval's output `raw` (KX planes of ood_out_values) -> hv, KX planes of np = 2 W + C values: T_c(z) =
// base_c(z) + w_c e(z) and T_c(zg) likewise for the BASE and ZERO columns, in exact field arithmetic (w_c is a base
// element, so it multiplies each component of an E value)
void ood_fold_sources(int KX, int W, int C, const CoeffSrc &S, const fe *w, const fe *raw, fe *hv);
void sum_partials(hipStream_t st, const fe *partials, int npolys, int nblk, fe *out, int b0 = 0, int b1 = -1);
// DEEP constants in device memory (the combine kernel reads alpha_t and alpha_c in place).  alpha_t[ZK_DEEP_LAGR] weighs
// e_(n-1)'s coefficients when the trace is read through a CoeffSrc with BASE or ZERO columns: sum_c alpha_t[c] w_c over
// them (deep_source_weight), zero otherwise
constexpr int ZK_DEEP_LAGR = 28;
template <int KX>
struct DeepConsts {
    typename Chal<KX>::T alpha_t[32];
    typename Chal<KX>::T alpha_c[16];
    typename Chal<KX>::T k1, k2, z, zg;
};
static_assert(sizeof(DeepConsts<1>) == 52 * sizeof(fe) && sizeof(DeepConsts<2>) == 52 * sizeof(fe2), "DeepConsts layout");
// Host: D.alpha_t[ZK_DEEP_LAGR] for the sources S with the scalars w (28, host)
template <int KX>
inline void deep_source_weight(DeepConsts<KX> &D, const CoeffSrc &S, const fe *w) {
    typedef Chal<KX> X;
    typename X::T s = X::zero();
    if (S.lagr)
        for (int c = 0; c < CoeffSrc::MAXC; c++)
            if (S.derived(c)) s = X::add(s, X::mulb(D.alpha_t[c], w[c]));
    D.alpha_t[ZK_DEEP_LAGR] = s;
}
// LDE of one n-coefficient polynomial over `count` cosets r0 + stride*j: out[j*n ..], coset-major.  ntt_tmp: 8n.
void lde_cosets(hipStream_t st, const NttTables &Tn, const CosetTables &CT, const fe *coeffs, size_t n, size_t r0,
                size_t stride, int count, fe *out, fe *ntt_tmp);
// The DEEP scratch for n coefficients over KX planes, in elements: 4 power tables of 2048 + H values (lo, hi halves of
// z, zg, 1/z, 1/zg), g1 and g2 (n values each), the KX output planes of n, 2 KX sums per phase-1 block of
// ZK_DEEP_BLOCK coefficients (after the scan: the block's carries), and a range's 2 KX totals (deep_range_*).  The
// boundary quotient (boundary_poly_add, boundary_range_*) uses the KX = 1 layout.
constexpr size_t ZK_DEEP_BLOCK = 256;
struct DeepScratch {
    size_t H;
    fe *pw, *g1, *g2, *out, *bs, *total;
    DeepScratch(fe *s, size_t n, int KX)
        : H(n / 2048 + 2),  // hi[] covers every t < nb * 2048 + 8
          pw(s),
          g1(pw + 4 * KX * (2048 + H)),
          g2(g1 + KX * n),
          out(g2 + KX * n),
          bs(out + KX * n),
          total(bs + 2 * KX * ((n + ZK_DEEP_BLOCK - 1) / ZK_DEEP_BLOCK)) {}
    static size_t size(size_t n, int KX) { return KX * (4 * (2048 + n / 2048 + 2) + 3 * n + 2 * (n / ZK_DEEP_BLOCK + 1)); }
};
// The DEEP polynomial's coefficients (KX planes of n) computed into scratch (returned); consts: DeepConsts<KX>
template <class T>
const fe *deep_poly(hipStream_t st, const CoeffSrc &S, const fe *cpolys, int ccols, int log_n,
                    const void *deep_consts_dev, T z, T zg, fe *scratch);
// The same split by coefficient range over the ranks of a sharded proof: rank g computes the range [k0, k0 + kn)
// (kn a multiple of ZK_DEEP_RANGE_QUANTUM) in two steps around one exchange.  deep_range_begin returns a device
// pointer to the range's totals (2 KX base elements); deep_range_end takes `ext`, the sum of the totals of every later
// range (the suffix carried into this one), and returns the coefficient buffer with this range filled in.
constexpr size_t ZK_DEEP_RANGE_QUANTUM = 2048;
template <class T>
const fe *deep_range_begin(hipStream_t st, const CoeffSrc &S, const fe *cpolys, int ccols, int log_n,
                           const void *deep_consts_dev, T z, T zg, fe *scratch, size_t k0, size_t kn);
template <class T>
const fe *deep_range_end(hipStream_t st, int log_n, T z, T zg, fe *scratch, size_t k0, size_t kn, const fe *ext);
// DEEP through coefficient form (kernels.hip): the DEEP polynomial (S - S(z))/(x - z) + (A - A(zg))/(x - zg)
// by suffix sums over the combined coefficients, one LDE per plane over the B cosets (CosetTables) into ulde
// (coset-major, KX planes of N), and (out != nullptr) a natural-order copy in out.  scratch: DeepScratch; ntt_tmp: 8n.
template <class T>
void deep_coeff_launch(hipStream_t st, const NttTables &Tn, const CoeffSrc &S, const fe *cpolys, int ccols, int log_n,
                       int log_b, const void *deep_consts_dev, T z, T zg, const CosetTables &CT, fe *scratch,
                       fe *ulde, fe *ntt_tmp, fe *out);
// FRI fold constants in device memory; fri_coin_launch writes alpha (KX components) in place
template <int KX>
struct FoldConsts {
    fe zinv[16];  // zeta^-t, t < fold
    typename Chal<KX>::T alpha;
    fe inv_offset, inv_fold;
};
static_assert(sizeof(FoldConsts<1>) == 19 * sizeof(fe) && offsetof(FoldConsts<1>, alpha) == 16 * sizeof(fe) &&
                  offsetof(FoldConsts<2>, alpha) == 16 * sizeof(fe),
              "FoldConsts layout");
// FRI layer leaves: row r of a layer of L values (rows = L / fold) is [e[r + k rows]]_k, an E value hashed as (a, b)
void commit_fri_layer(hipStream_t st, int KX, const fe *layer, size_t L, int fold, uint8_t *leaves, uint8_t *nodes,
                      int lb = 0);
// FRI fold: next[r] = p_r(alpha) over rows r < L / fold (consts: FoldConsts<KX> in device memory)
void fri_fold_launch(hipStream_t st, int KX, const fe *layer, size_t L, int fold, const void *fold_consts_dev,
                     const NttTables &TN, size_t wstride, fe *next, int lb = 0);
void coset_major_to_natural(hipStream_t st, const fe *src, int log_n, int log_b, fe *dst);
// The composition values between the library's layout and winterfell's (kernels.hip, CE layout conversion): `ext`
// coset-major component planes of 8n values, plane[k][r*n + q], and the natural interleaved order, component k of
// element i = r + 8q at fe index i*ext + k.  to_natural: src the planes, dst the natural values; else the inverse.
// src and dst are distinct buffers of 8 ext n elements.  max_blocks = 0: the launcher's grid cap.
constexpr unsigned ZK_CE_LAYOUT_BLOCKS = 2048;  // 8 blocks for each of 256 CUs; a block's LDS image is 8 ext KiB
void ce_layout(hipStream_t st, const fe *src, size_t n, int ext, bool to_natural, fe *dst, unsigned max_blocks = 0);
// Rows [first, first + count) of a coset-major LDE (element (c, i) at base[(c*B + i mod B)*n + i div B], B = 2^log_b,
// log_b in [3, 6], ncols in [1, 28], any n >= 1) as a row matrix: row i at dst + (i - first)*ncols.  first + count
// <= n B: the caller splits a window that wraps.  max_blocks = 0: the launcher's own cap.
constexpr unsigned ZK_ROWS_LAYOUT_BLOCKS = 1280;  // 5 blocks for each of 256 CUs; a block's LDS image is 1040 ncols bytes
void rows_layout(hipStream_t st, const fe *base, int ncols, size_t n, int log_b, size_t first, size_t count, fe *dst,
                 unsigned max_blocks = 0);
// The E column polynomials of a composition with two planes, base column (c, k) at src[(2c + k)*n], as ncols columns
// of n interleaved (a, b) values in dst (2 ncols n elements, distinct from src)
void interleave_columns(hipStream_t st, const fe *src, size_t n, int ncols, fe *dst);
// FRI commit-phase coin on the device: seed = merge(seed, root_dev), alpha (k = 1 or 2 components) drawn
// into alpha_dev (where the fold reads it) and alpha_log (the per-layer record the host replay is checked
// against)
void fri_coin_launch(hipStream_t st, uint32_t *seed_dev, const uint8_t *root_dev, int k, fe *alpha_dev,
                     fe *alpha_log);

// out[k] = src[idx[k]] for field elements
void gather_fe(hipStream_t st, const fe *src, const uint64_t *idx, size_t k, fe *out);

}  // namespace zk
