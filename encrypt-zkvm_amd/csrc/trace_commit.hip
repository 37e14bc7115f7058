// trace_commit.hip -- S2 of the single-GPU prove path: interpolate the 28 trace columns (winter-math interpolate_poly
// over <w_n>), extend them over the B cosets of the LDE domain (coset r: the coefficients scaled by (3 w_N^r)^k) and
// commit to the rows; for a host-resident trace also its upload, the column classes that spare most of it (decided by
// upload_plan.hpp) with their host checks, and the hints a proof leaves for the next one of its (length, program).
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>

#include "host_pool.hpp"
#include "prover_internal.hpp"

using namespace zk;

// ---------------------------------------------------------------- switches
// Sparse trace columns (SparseCols): a column that is zero in every row but the last (the VM's stack registers past
// the program's maximum depth, five of the benchmark's 28) interpolates to last * lagr and extends to last * lagr_lde;
// sparse_detect flags them on the device and the NTT passes skip their DFTs.  Exact: the same polynomials and LDE.
// ZK_SPARSE=0 transforms every column.
bool zk::sparse_on() { static const bool on = env_switch("ZK_SPARSE"); return on; }
// Narrow columns (host-resident traces): ZK_NARROW=0 uploads every column whole.
bool zk::narrow_on() { static const bool on = env_switch("ZK_NARROW"); return on; }
// The AIR clock (ZK_CLOCK=0 turns its derivation off)
bool zk::clock_on() { static const bool on = env_switch("ZK_CLOCK"); return on; }
// Fixed columns (zk_prover::FixedSnap).  ZK_FIXED=0 turns the class off.
bool zk::fixed_on() { static const bool on = env_switch("ZK_FIXED"); return on; }
// ZK_FIXED_FUSE=0: their LDE (and the clock's, and zk_vm_prove's preprocessed columns') by the streaming passes and
// hash_rows_blocks instead of inside the row hash of their blocks (fixed_hash)
bool zk::fixed_fuse_on() { static const bool on = env_switch("ZK_FIXED_FUSE"); return on; }
// Virtual columns (upload_plan.hpp ZK_VIRT_MIN_COL): ZK_VIRTUAL=0 writes their LDE
static bool virtual_on() { static const bool on = env_switch("ZK_VIRTUAL"); return on; }
// Coefficient sources (UploadPlan::coeff_src): ZK_COEFF_SRC=0 writes the derived columns' coefficients into polys
bool zk::coeff_src_on() { static const bool on = env_switch("ZK_COEFF_SRC"); return on; }

// ---------------------------------------------------------------- hint sets and snapshots
// forget snapshot i (its device buffers stay allocated for the next snapshot of that size)
static void fixed_drop(zk_prover *p, int i) {
    if (i < 0) return;
    zk_prover::FixedSnap &s = p->fix_snaps[i];
    if (s.owner >= 0 && p->hint_sets[s.owner].snap == i) p->hint_sets[s.owner].snap = -1;
    s.live = false;
    s.owner = -1;
    s.mask = 0;
    for (auto &h : s.host) h.reset();
    if (p->tc.fix_pending == i) p->tc.fix_pending = -1;
}

// A snapshot slot for hint set `owner` with buffers for k planes of n and B n elements: a free slot (one whose
// buffers already have that size first), else the least recently used one.  -1 if the memory is not to be had.
static int fixed_slot(zk_prover *p, int owner, size_t n, uint32_t B, int k) {
    const size_t np = (size_t)k * n, nl = np * B;
    int best = -1;
    for (int i = 0; i < zk_prover::ZK_FIXED_SNAPS; i++) {
        const auto &s = p->fix_snaps[i];
        if (s.live) continue;
        if (best < 0 || (s.cap_polys == np && s.cap_lde == nl)) best = i;
    }
    if (best < 0) {
        best = 0;
        for (int i = 1; i < zk_prover::ZK_FIXED_SNAPS; i++)
            if (p->fix_snaps[i].used < p->fix_snaps[best].used) best = i;
        fixed_drop(p, best);
    }
    zk_prover::FixedSnap &s = p->fix_snaps[best];
    if (s.cap_polys != np || s.cap_lde != nl) {
        // (the previous proofs on this prover have drained: nothing reads the old buffers)
        (void)hipFree(s.fpolys);
        (void)hipFree(s.flde);
        s.fpolys = s.flde = nullptr;
        s.cap_polys = s.cap_lde = 0;
        if (hipMalloc((void **)&s.fpolys, np * sizeof(fe)) != hipSuccess ||
            hipMalloc((void **)&s.flde, nl * sizeof(fe)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(s.fpolys);
            s.fpolys = s.flde = nullptr;
            return -1;
        }
        s.cap_polys = np;
        s.cap_lde = nl;
    }
    s.owner = owner;
    s.n = n;
    s.B = B;
    s.k = k;
    return best;
}

// The hint set of (n, program), or null (prover state: zk_prover::HintSet)
static zk_prover::HintSet *hint_find(zk_prover *p, size_t n, const uint8_t *key) {
    if (!key) return nullptr;
    for (auto &h : p->hint_sets)
        if (h.n == n && !memcmp(h.key, key, 32)) return &h;
    return nullptr;
}
// ... found or made, evicting the least recently used set
static zk_prover::HintSet *hint_slot(zk_prover *p, size_t n, const uint8_t *key) {
    zk_prover::HintSet *h = hint_find(p, n, key);
    if (h) return h;
    h = &p->hint_sets[0];
    for (auto &e : p->hint_sets)
        if (e.used < h->used) h = &e;
    fixed_drop(p, h->snap);  // an evicted set's snapshot goes with it
    *h = zk_prover::HintSet{};
    h->n = n;
    memcpy(h->key, key, 32);
    return h;
}

// rows [r0, r1) of a host column against a snapshot's host copy
bool zk::same_rows(const uint8_t *col, const uint8_t *snap, size_t r0, size_t r1, int width) {
    if (width == 16) return !memcmp(col + 16 * r0, snap + 16 * r0, 16 * (r1 - r0));
    const uint64_t *v = reinterpret_cast<const uint64_t *>(col);
    uint64_t bad = 0;
    if (width == 1) {
        for (size_t i = r0; i < r1; i++) bad |= (v[2 * i] ^ (uint64_t)snap[i]) | v[2 * i + 1];
    } else {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(snap);
        for (size_t i = r0; i < r1; i++) bad |= (v[2 * i] ^ (uint64_t)s[i]) | v[2 * i + 1];
    }
    return bad == 0;
}

// rows [r0, r1) of a host column: row i holds i (the AIR clock)
bool zk::clock_rows(const uint8_t *col, size_t r0, size_t r1) {
    const uint64_t *v = reinterpret_cast<const uint64_t *>(col);
    uint64_t bad = 0;
    for (size_t i = r0; i < r1; i++) bad |= (v[2 * i] ^ (uint64_t)i) | v[2 * i + 1];
    return bad == 0;
}

// rows [r0, r1) of a host column as `width`-byte integers (1 or 4) at dst + width * row; false if a value does not fit
bool zk::pack_rows(const uint8_t *col, size_t r0, size_t r1, int width, uint8_t *dst) {
    const uint64_t *v = reinterpret_cast<const uint64_t *>(col);
    uint64_t over = 0;
    if (width == 1) {
        for (size_t i = r0; i < r1; i++) {
            const uint64_t lo = v[2 * i], hi = v[2 * i + 1];
            over |= (lo >> 8) | hi;
            dst[i] = (uint8_t)lo;
        }
    } else {
        uint32_t *d = reinterpret_cast<uint32_t *>(dst);
        for (size_t i = r0; i < r1; i++) {
            const uint64_t lo = v[2 * i], hi = v[2 * i + 1];
            over |= (lo >> 32) | hi;
            d[i] = (uint32_t)lo;
        }
    }
    return over == 0;
}

// rows [r0, r1) of a host column all zero
bool zk::zero_rows(const uint8_t *col, size_t r0, size_t r1) {
    const uint64_t *v = reinterpret_cast<const uint64_t *>(col);
    uint64_t any = 0;
    for (size_t i = 2 * r0; i < 2 * r1; i++) any |= v[i];
    return any == 0;
}

int zk::plan_rank_tables(zk_prover *p, Plan *pl, int r0, int G) {
    if (p->shard_world <= 1 || !pl->lagr) return ZK_OK;  // a full prover's tables hold every coset
    const size_t n = (size_t)1 << pl->log_n, Bl = ((size_t)1 << pl->log_b) >> ilog2((size_t)G);
    // the rank's block of cosets r0 .. r0 + Bl - 1 (shard.hip: rank g owns g Bl + j)
    if (pl->lagr_lde && pl->lde_r0 == r0 && pl->lde_shift == 0 && pl->lde_cos == (int)Bl) return ZK_OK;
    if (!pl->lagr_lde) ZK_CHECK_HIP(p->arena.alloc(&pl->lagr_lde, Bl * n));
    ntt_lde(p->st, pl->Tn, pl->ct, pl->lagr, n, 1, r0, 1, (int)Bl, pl->lagr_lde, Bl * n, n, p->tmp);
    if (pl->id_lde) ntt_lde(p->st, pl->Tn, pl->ct, pl->id_poly, n, 1, r0, 1, (int)Bl, pl->id_lde, Bl * n, n, p->tmp);
    pl->lde_r0 = r0;
    pl->lde_shift = 0;
    pl->lde_cos = (int)Bl;
    ZK_CHECK_HIP(hipStreamSynchronize(p->st));
    return ZK_OK;
}

// the identity column 0, 1, ..., n-1 interpolated and extended over the cosets the plan's fill tables hold
// (Plan::id_poly / id_lde, lde_r0 / lde_shift / lde_cos: all B for a full prover), once per plan
int zk::clock_tables(zk_prover *p, Plan *pl) {
    if (pl->id_poly) return ZK_OK;
    if (!pl->lde_cos) ZK_FAIL(ZK_ERR_INVALID_ARG, "internal error: the plan's rank tables are not built");
    const size_t n = (size_t)1 << pl->log_n, nc = (size_t)pl->lde_cos;
    fe *poly = nullptr, *lde = nullptr;
    ZK_CHECK_HIP(p->arena.alloc(&poly, n));
    ZK_CHECK_HIP(p->arena.alloc(&lde, nc * n));
    std::vector<fe> id(n);
    for (size_t i = 0; i < n; i++) id[i] = fe_make(i);
    fe *d = nullptr;
    ZK_CHECK_HIP(hipMalloc(&d, n * sizeof(fe)));
    hipError_t err = hipMemcpy(d, id.data(), n * sizeof(fe), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        const fe inv_n = h_inv(fe_make(n));
        ntt(p->st, pl->Tn, d, n, poly, n, 1, true, nullptr, &inv_n, p->tmp);
        ntt_lde(p->st, pl->Tn, pl->ct, poly, n, 1, pl->lde_r0, 1 << pl->lde_shift, (int)nc, lde, nc * n, n, p->tmp);
        err = hipStreamSynchronize(p->st);
    }
    (void)hipFree(d);
    ZK_CHECK_HIP(err);
    pl->id_poly = poly;
    pl->id_lde = lde;
    return ZK_OK;
}

int zk::sparse_begin(zk_prover *p, Plan *pl, SparseCols *out, const SparseCols **sp) {
    *sp = nullptr;
    if (!sparse_on() || !pl->lagr || !pl->lagr_lde) return ZK_OK;
    if (!p->sp_nz) {
        ZK_CHECK_HIP(p->arena.alloc(&p->sp_nz, 4 * W));  // nonzero, 8-bit, 32-bit flags; [3W]: column 0 not the clock
        ZK_CHECK_HIP(p->arena.alloc(&p->sp_last, W));
        ZK_CHECK_HIP(p->arena.alloc(&p->sp_last_ws, W));
        ZK_CHECK_HIP(hipHostMalloc((void **)&p->sp_h, 3 * W * sizeof(unsigned), hipHostMallocDefault));
    }
    ZK_CHECK_HIP(hipMemsetAsync(p->sp_nz, 0, 4 * W * sizeof(unsigned), p->st));
    *out = SparseCols{p->sp_nz, p->sp_last, pl->lagr, pl->lagr_lde, 0};
    out->lde_r0 = pl->lde_r0;
    out->lde_shift = pl->lde_shift;
    if (clock_on()) {  // the AIR clock of column 0, detected with the sparse columns (device-side traces)
        ZK_TRY(clock_tables(p, pl));
        out->id_poly = pl->id_poly;
        out->id_lde = pl->id_lde;
        out->idoff = 3 * W;
    }
    *sp = out;
    return ZK_OK;
}

int zk::ensure_pack(zk_prover *p, size_t bytes) {
    if (bytes <= p->h_pack_cap) return ZK_OK;  // (the previous proof's copies from it have drained: CopyGuard)
    if (p->h_pack) (void)hipHostFree(p->h_pack);
    p->h_pack = nullptr;
    p->h_pack_cap = 0;
    ZK_CHECK_HIP(hipHostMalloc((void **)&p->h_pack, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    p->h_pack_cap = bytes;
    return ZK_OK;
}

// ---------------------------------------------------------------- the commitment
// Column groups of a host-resident trace upload.  The copy engine streams group g + 1 while the CUs interpolate and
// extend group g; more groups overlap more of the copy but add a launch drain per NTT pass and group.  A/B on one box
// (3 provers in flight): 1 group 12.73-13.02 ms per proof at 22.7 ms latency, 2 groups 13.15-13.24 / 18.7, 4 groups
// 13.16-13.32 / 16.8, 7 groups of 4 13.02-13.04 / 15.9 (device-resident 12.15-12.32).  Round 4: the rows are hashed
// block by block as their columns' LDEs complete (hash_rows_blocks: a 28-element row is 7 BLAKE3 blocks of 4
// columns), and the last 4 columns go up as two groups of 2, so after the last copy only 2 columns' NTTs, one
// compression per row and the Merkle tree remain (latency 15.3-15.4 -> 13.9-14.2 ms against 7 groups of 4, all rows
// hashed at the end; profiles/r04_ab_queues_pass1.txt).

// hipMemcpyAsync from page-locked memory (zk_host_alloc, zk_host_register, any hipHostMalloc'd or
// hipHostRegister'ed buffer) is a DMA in stream order; from pageable memory the runtime stages the copy
// through its own pinned buffers and returns once the source has been read (the host thread copies).
// Both are correct here; the pinned form is the fast one (DESIGN.md "Host-resident trace").
// Columns that are contiguous in host memory (zk_prove's single buffer) go up as one copy per run.
static int upload_trace_group(zk_prover *p, const TraceSrc &src, size_t n, int c0, int nc) {
    const size_t col = n * sizeof(fe);
    p->tc.up_bytes += (uint64_t)nc * col;
    for (int c = c0; c < c0 + nc;) {
        int e = c + 1;
        while (e < c0 + nc && src.cols[e] == src.cols[e - 1] + col) e++;
        ZK_CHECK_HIP(hipMemcpyAsync(p->d_trace + (size_t)c * n, src.cols[c], (size_t)(e - c) * col, hipMemcpyHostToDevice,
                                    p->up));
        c = e;
    }
    return ZK_OK;
}

void zk::fixed_coeff_src(zk_prover *p, const FixedCols &fx, size_t n) {
    for (int c = 0; c < W; c++) {
        if (c >= 12 && c < 12 + fx.md) continue;
        p->csrc.plane[c] = c < 12 ? fx.fpolys + (size_t)c * n : nullptr;
        p->csrc.mode[c] = c < 12 ? CoeffSrc::BASE : CoeffSrc::ZERO;
        p->csrc_w[c] = fx.last[c];
        p->tc.coeff_src |= 1u << c;
    }
    p->csrc.lagr = fx.lagr;
}

// zk_vm_prove: interpolate and extend the dynamic stack columns only; the preprocessed ones by one pass (their
// coefficients are read at their source, not written: fixed_coeff_src)
static int commit_device_fixed(zk_prover *p, Plan *pl, const TraceSrc &src, size_t n, uint8_t root[32]) {
    const FixedCols &fx = *src.fixed;
    if (coeff_src_on()) fixed_coeff_src(p, fx, n);
    const fe inv_n = h_inv(fe_make(n));
    const size_t B = (size_t)1 << pl->log_b, c0 = 12;
    if (fx.md > 0) {
        ntt(p->st, pl->Tn, src.dev + c0 * n, n, p->polys + c0 * n, n, fx.md, true, nullptr, &inv_n, p->tmp);
        ntt_lde(p->st, pl->Tn, pl->ct, p->polys + c0 * n, n, fx.md, 0, 1, (int)B, p->lde + c0 * B * n, B * n, n, p->tmp);
    }
    const int pre = p->fix_prefix_blocks;  // (zk_vm_prove: the preprocessed part went first, fixed_prefix)
    p->fix_prefix_blocks = 0;
    if (pre) {
        hash_rows_blocks(p->st, p->lde, W, pl->log_n, pl->log_b, pre, W / 4, p->leaves);
    } else {
        if (!p->fix_ws) ZK_CHECK_HIP(p->arena.alloc(&p->fix_ws, W));
        fe_ws ws[W];
        for (int c = 0; c < W; c++) ws[c] = make_fe_ws(fx.last[c]);
        ZK_TRY(h2d_small(p, p->fix_ws, ws, sizeof ws));
        fixed_axpy(p->st, fx, p->fix_ws, n, B, p->polys, p->lde, 0, !coeff_src_on());
        hash_rows_cosets(p->st, p->lde, W, pl->log_n, pl->log_b, 0, pl->log_b, p->leaves);
    }
    merkle_tree(p->st, p->leaves, n * B, p->nodes);
    return d2h_small(p, root, p->nodes + 32, 32);
}

// a trace resident in HBM: every column detected, interpolated and extended at once
static int commit_device(zk_prover *p, Plan *pl, const TraceSrc &src, size_t n, const SparseCols *sp, uint8_t root[32]) {
    const fe inv_n = h_inv(fe_make(n));
    const size_t B = (size_t)1 << pl->log_b;
    if (sp) sparse_detect(p->st, src.dev, n, 0, W, *sp);
    ntt(p->st, pl->Tn, src.dev, n, p->polys, n, W, true, nullptr, &inv_n, p->tmp, sp);
    ntt_lde(p->st, pl->Tn, pl->ct, p->polys, n, W, 0, 1, (int)B, p->lde, B * n, n, p->tmp, sp);
    hash_rows_cosets(p->st, p->lde, W, pl->log_n, pl->log_b, 0, pl->log_b, p->leaves);
    merkle_tree(p->st, p->leaves, n * B, p->nodes);
    return d2h_small(p, root, p->nodes + 32, 32);
}

namespace {

// The commitment to W host columns.  The trace goes up on the upload stream in the items of the upload plan; each item's
// event gates its columns' interpolation and coset LDE on the compute stream.  (The device trace buffer is free: the
// previous proof on this prover returned only after its stream drained.)  Host threads check every value the hints of
// the previous proof of this (length, program) spare: a narrow column that does not fit goes up whole; a sparse, clock
// or fixed one that is not what the hint says voids the proof (prove_impl redoes it without hints).
struct HostTraceCommit {
    zk_prover *const p;
    Plan *const pl;
    const TraceSrc &src;
    const size_t n, B;
    SparseCols spc;
    const SparseCols *const sp;  // null: no detection, so no hints either
    const fe inv_n = h_inv(fe_make(n));
    zk_prover::HintSet *H = nullptr;
    bool fresh = false;                  // H holds a completed proof's findings
    zk_prover::FixedSnap *FS = nullptr;  // the snapshot the fixed columns are formed from
    zk_prover::FixedSnap *snap = nullptr;  // ... or the one this proof takes
    UploadPlan u;
    bool ready[W] = {};  // the column's LDE is written (or virtual)
    int hashed = 0;      // BLAKE3 blocks hashed
    // the host tasks read the caller's columns: every latch is waited for on every way out
    Latch packed[W], checked, clocked, compared, copied;
    std::atomic<uint32_t> pack_bad{0}, sparse_bad{0}, clock_bad{0}, fixed_bad{0}, copy_bad{0};
    static constexpr size_t R = (size_t)1 << 18;  // rows per host task
    fe_ws clk_d{};                                 // the clock's last row minus n - 1
    // Upload items, each one copy (or a run of column copies) and an event on the shared upload stream.  The next
    // item's copy is queued before the host waits for the current one's event (the compute stream never parks on the
    // upload stream: a parked stream would hold up the kernels of other provers that share its hardware queue), so the
    // copy engine always has the next group.
    struct Item {
        const int *cols = nullptr;
        int nc = 0, part = -1, ev = 0;  // part: narrow part (packed), or -1 (whole columns)
    };
    int fallback[W], nfb = 0, good[W], ev = 0, gi = 0, di = 0;
    bool narrow_done[2] = {}, fb_done = false;
    NarrowCols G[W] = {};    // the columns of each narrow part that went up packed
    size_t part_off[W + 1];  // byte range of each part in h_pack
    uint8_t *const stage = reinterpret_cast<uint8_t *>(p->ctmp);  // composition scratch: free until S4

    HostTraceCommit(zk_prover *p_, Plan *pl_, const TraceSrc &s, size_t n_, const SparseCols &c, bool detect)
        : p(p_), pl(pl_), src(s), n(n_), B((size_t)1 << pl_->log_b), spc(c), sp(detect ? &spc : nullptr) {}
    ~HostTraceCommit() {
        for (auto &l : packed) l.wait();
        for (Latch *l : {&checked, &clocked, &compared, &copied}) l->wait();
    }

    void classify() {
        H = sp && src.hint_ok ? hint_find(p, n, src.key) : nullptr;
        UploadPlanIn in;
        fresh = H && H->have;
        if (H) {
            in.have = H->have, in.sparse = H->sparse, in.nw8 = H->nw8, in.nw32 = H->nw32;
            in.clk_off = H->clk_off, in.fixed_off = H->fixed_off;
            if (H->snap >= 0) {
                zk_prover::FixedSnap &s = p->fix_snaps[H->snap];
                if (s.live && s.n == n && s.B == B && s.lwe == src.lwe) FS = &s;
            }
            in.snap = FS != nullptr;
            in.snap_mask = FS ? FS->mask : 0u;
        }
        in.hint_ok = src.hint_ok, in.no_virtual = src.no_virtual, in.lat_sched = p->lat_sched, in.detect = sp != nullptr;
        in.sparse_on = sparse_on(), in.narrow_on = narrow_on(), in.clock_on = clock_on();
        in.fixed_on = fixed_on(), in.fixed_fuse_on = fixed_fuse_on(), in.virtual_on = virtual_on(), in.n = n;
        in.coeff_src_on = coeff_src_on();
        u = upload_plan(in);
        if (!u.fix_ok) FS = nullptr;
        else if (!FS && H->snap >= 0) fixed_drop(p, H->snap);  // snap for another blowup or lwe_size: snap again
        if (FS) FS->used = ++p->hint_stamp;
        zk_prover::TraceOutcome &tc = p->tc;
        tc.clk_used = u.clk;
        tc.fix_used = u.fixm;
        tc.clk_bad = tc.fix_bad = false;
        tc.fix_pending = -1;
        tc.sp_hinted = tc.up_sparse = u.hint;
        // (a narrow column snap as fixed stays listed under its narrow class; none of its bytes cross the link)
        tc.up_nw8 = u.nw8 & u.fixm;
        tc.up_nw32 = u.nw32 & u.fixm;
        if (sp) spc.wstride = W;  // width flags for the next proof's narrow hint
        narrow_done[0] = u.np < 1, narrow_done[1] = u.np < 2;
        for (int k = 0; k <= u.np; k++) part_off[k] = u.pb[k] < u.nn ? u.off[u.pb[k]] : u.pack_bytes;
    }

    fe last_of(int c) const { return fe_from_bytes(src.cols[c] + (n - 1) * sizeof(fe)); }  // the column's last row
    // column c's coefficients are plane (or nothing) + w e_(n-1), read there by S3 .. S5 and not written (u.coeff_src)
    void source(int c, uint8_t mode, const fe *plane, fe w) {
        p->csrc.plane[c] = plane;
        p->csrc.mode[c] = mode;
        p->csrc.lagr = pl->lagr;
        p->csrc_w[c] = w;
        p->tc.coeff_src |= 1u << c;
    }
    // interpolation and / or coset LDE of columns [c0, c0 + nc).  fused: the interpolation's pass 1 writes the columns'
    // flags; all: every column is sparse, the fills alone (SparseCols)
    enum { INTERP = 1, LDE = 2 };
    int transform(int c0, int nc, bool fused, bool all = false, int what = INTERP | LDE) {
        SparseCols g = spc;
        g.col0 = c0, g.fused = fused, g.all = all;
        const SparseCols *gs = sp ? &g : nullptr;
        const size_t o = (size_t)c0 * n;
        if (what & INTERP) ntt(p->st, pl->Tn, p->d_trace + o, n, p->polys + o, n, nc, true, nullptr, &inv_n, p->tmp, gs);
        if (what & LDE)
            ntt_lde(p->st, pl->Tn, pl->ct, p->polys + o, n, nc, 0, 1, (int)B, p->lde + o * B, B * n, n, p->tmp, gs);
        return ZK_OK;
    }
    // the blocks whose 4 columns are extended, at least two per launch but the last
    void hash_ready(bool last) {
        int b = hashed;
        while (b < W / 4 && ready[4 * b] && ready[4 * b + 1] && ready[4 * b + 2] && ready[4 * b + 3]) b++;
        if (b - hashed >= 2 || (last && b > hashed)) {
            hash_rows_blocks(p->st, p->lde, W, pl->log_n, pl->log_b, hashed, b, p->leaves,
                             VirtCols{p->tc.virt, p->sp_last_ws, pl->lagr_lde});
            hashed = b;
        }
    }
    // The kernels of an uploaded column list: detection (flags for the next proof's hints), transforms, hashing.  With
    // the hints learned the flags come from the interpolation's pass 1 (no separate pass over the columns; one found
    // sparse there is transformed in full this time and hinted next time).
    int process(const int *cols, int nc) {
        if (sp && !fresh)
            ZK_TRY(for_runs(cols, nc, [this](int c0, int k) {
                sparse_detect(p->st, p->d_trace, n, c0, k, spc);
                return ZK_OK;
            }));
        ZK_TRY(for_runs(cols, nc, [this](int c0, int k) { return transform(c0, k, fresh); }));
        for (int i = 0; i < nc; i++) ready[cols[i]] = true;
        hash_ready(false);
        return ZK_OK;
    }

    // Host checks of the hints: one pool task per quarter million rows of a hinted column, the narrow ones packing rows
    // 0 .. n-2 (1 or 4 bytes each) into pinned h_pack as they go (64 K-row tasks on the latency schedule, so each part
    // is ready in ~0.1-0.2 ms)
    int start_checks() {
        ZK_TRY(ensure_pack(p, u.pack_bytes));
        for (int i = 0, k = 0; i < u.nn; i++) {
            if (i == u.pb[k + 1]) k++;  // part k holds narrow column i
            row_tasks(packed[k], i, 0, n - 1, u.lat ? (size_t)1 << 16 : R, [this](int j, size_t r0, size_t r1) {
                uint8_t *dst = p->h_pack + u.off[j];
                if (!pack_rows(src.cols[u.nar[j]], r0, r1, u.width[j], dst)) pack_bad.fetch_or(1u << u.nar[j]);
                if (r1 == n - 1) memset(dst + (size_t)u.width[j] * (n - 1), 0, u.width[j]);  // (the last row's slot)
            });
        }
        for (int i = 0; i < u.nh; i++)
            row_tasks(checked, u.hin[i], 0, n - 1, R, [this](int c, size_t r0, size_t r1) {
                if (!zero_rows(src.cols[c], r0, r1)) sparse_bad.fetch_or(1u << c);
            });
        return ZK_OK;
    }

    // hinted sparse columns: their coefficients and LDE are last * e_(n-1)'s (the NTT passes' sparse fill).  No
    // transform: the fills alone -- the coefficients of every hinted column, the LDE of the non-virtual ones
    int fill_sparse() {
        if (!u.nh) return ZK_OK;
        fe lastv[W] = {};
        for (int i = 0; i < u.nh; i++) lastv[u.hin[i]] = last_of(u.hin[i]);
        ZK_TRY(h2d_small(p, p->sp_last, lastv, sizeof lastv));
        if (u.virt) {  // the row hash multiplies e_(n-1)'s LDE by these through their W sets
            fe_ws ws[W] = {};
            for (int c = 0; c < W; c++)
                if ((u.virt >> c) & 1u) ws[c] = make_fe_ws(lastv[c]);
            ZK_TRY(h2d_small(p, p->sp_last_ws, ws, sizeof ws));
        }
        if (u.coeff_src)
            for (int i = 0; i < u.nh; i++) source(u.hin[i], CoeffSrc::ZERO, nullptr, lastv[u.hin[i]]);
        else
            ZK_TRY(for_runs(u.hin, u.nh, [this](int c0, int nc) { return transform(c0, nc, false, true, INTERP); }));
        ZK_TRY(for_runs(u.hnv, u.nhv, [this](int c0, int nc) { return transform(c0, nc, false, true, LDE); }));
        p->tc.virt = u.virt;
        memcpy(p->tc.virt_last, lastv, sizeof lastv);
        p->tc.virt_lagr = pl->lagr_lde;
        for (int i = 0; i < u.nh; i++) ready[u.hin[i]] = true;
        return ZK_OK;
    }

    // column 0 from the identity column's tables; host threads check rows 0 .. n-2 while the other columns go up
    int derive_clock() {
        if (!u.clk) return ZK_OK;
        ZK_TRY(clock_tables(p, pl));
        row_tasks(clocked, 0, 0, n - 1, R, [this](int, size_t r0, size_t r1) {
            if (!clock_rows(src.cols[0], r0, r1)) clock_bad.store(1u);
        });
        const fe d = fe_sub(last_of(0), fe_make(n - 1));
        clk_d = make_fe_ws(d);
        if (u.coeff_src) source(0, CoeffSrc::BASE, pl->id_poly, d);
        else axpy_fill(p->st, pl->id_poly, pl->lagr, clk_d, n, p->polys);
        if (!u.fuse_nb) axpy_fill(p->st, pl->id_lde, pl->lagr_lde, clk_d, B * n, p->lde);
        ready[0] = true;
        return ZK_OK;
    }

    // the fixed columns: the snapshot's f_c plus last[c] times e_(n-1)'s coefficients / LDE, in one pass each; only
    // the last-row values go up.  Their BLAKE3 blocks (0 .. 2 when the clock is derived too) start at once.
    int form_fixed() {
        if (!u.fixm) return ZK_OK;
        if (!p->fix_ws) ZK_CHECK_HIP(p->arena.alloc(&p->fix_ws, W));
        fe_ws ws[W] = {};
        FixedColList L;
        for (int c = 0; c < W; c++) {
            if (!((u.fixm >> c) & 1u)) continue;
            const fe last = last_of(c);
            ws[c] = make_fe_ws(last);
            L.col[L.count] = (uint8_t)c;
            L.slot[L.count] = FS->slot[c];
            L.count++;
            if (u.coeff_src) source(c, CoeffSrc::BASE, FS->fpolys + (size_t)FS->slot[c] * n, last);
        }
        if (u.fuse_nb) ws[0] = clk_d;  // (column 0 is never in the fixed class: its W set slot carries the clock's d)
        ZK_TRY(h2d_small(p, p->fix_ws, ws, sizeof ws));
        fixed_cols_axpy(p->st, L, false, FS->fpolys, FS->flde, pl->lagr, pl->lagr_lde, p->fix_ws, n, B, p->polys, p->lde,
                        4 * u.fuse_nb, !u.coeff_src);
        for (int k = 0; k < L.count; k++) ready[L.col[k]] = true;
        if (u.fuse_nb) {
            FixedHashCols A{};
            for (int c = 0; c < 4 * u.fuse_nb; c++) {
                A.wsi[c] = (uint8_t)c;
                A.mode[c] = FixedHashCols::LOAD;  // hinted sparse: filled above
                if ((u.clk && c == 0) || ((u.fixm >> c) & 1u)) {
                    A.mode[c] = FixedHashCols::FORM;
                    A.src[c] = c == 0 ? pl->id_lde : FS->flde + (size_t)FS->slot[c] * B * n;
                }
            }
            fixed_hash(p->st, A, pl->lagr_lde, p->fix_ws, p->lde, W, pl->log_n, pl->log_b, u.fuse_nb, p->leaves);
            hashed = u.fuse_nb;
        }
        hash_ready(false);
        // the host check: every row 0 .. n-2 of the caller's columns against the snapshot's host copy
        for (int k = 0; k < L.count; k++)
            row_tasks(compared, L.col[k], 0, n - 1, R, [this](int c, size_t r0, size_t r1) {
                if (!same_rows(src.cols[c], FS->host[c].get(), r0, r1, FS->width[c])) fixed_bad.fetch_or(1u << c);
            });
        return ZK_OK;
    }

    // part k's columns once packed (the host waits for its packing), its unpackable ones to the fallback list
    bool narrow_item(int k, Item *it) {
        packed[k].wait();
        if (k < 2) narrow_done[k] = true;
        const uint32_t bad = pack_bad.load();
        NarrowCols &g = G[k];
        int *gd = good + u.pb[k], ng = 0;
        for (int i = u.pb[k]; i < u.pb[k + 1]; i++) {
            const int c = u.nar[i];
            if ((bad >> c) & 1u) {  // a value that does not fit: this column goes up whole
                fallback[nfb++] = c;
                continue;
            }
            g.col[g.count] = c;
            g.width[g.count] = u.width[i];
            g.off[g.count] = u.off[i];
            g.last[g.count] = last_of(c);
            g.count++;
            gd[ng++] = c;
        }
        if (!ng) return false;
        *it = Item{gd, ng, k, -1};
        return true;
    }
    void count_part(int k) {  // part k's packed bytes cross the link
        zk_prover::TraceOutcome &tc = p->tc;
        tc.up_bytes += part_off[k + 1] - part_off[k];
        const NarrowCols &g = G[k];
        for (int i = 0; i < g.count; i++) (g.width[i] == 1 ? tc.up_nw8 : tc.up_nw32) |= 1u << g.col[i];
    }
    int issue(const Item &it) {
        std::lock_guard<std::mutex> lk(*p->up_mu);
        // a copy that fails part-way through the item still gets the item's event behind the copies queued before
        // it, so upload_drain (CopyGuard) waits for every DMA that reads the caller's columns
        UploadEvent rec{p->ev_up[it.ev], p->up};
        if (it.part >= 0) {
            const size_t a = part_off[it.part];
            ZK_CHECK_HIP(hipMemcpyAsync(stage + a, p->h_pack + a, part_off[it.part + 1] - a, hipMemcpyHostToDevice, p->up));
            count_part(it.part);
        } else {
            ZK_TRY(for_runs(it.cols, it.nc, [this](int c0, int k) { return upload_trace_group(p, src, n, c0, k); }));
        }
        return rec.record();
    }
    bool next_dense(Item *it) {
        if (gi >= u.ngroups) return false;
        *it = Item{u.dense + di, u.gsz[gi], -1, ev++};
        di += u.gsz[gi++];
        return true;
    }

    // The latency schedule (this proof alone on the device): dense groups 0 and 1 start crossing the link at once,
    // group g + 2 once group g has landed; the narrow parts in order as they are packed, each part's expansion kernel
    // reading the pinned packed bytes itself (no copy engine: that is busy with the dense groups), so the first kernels
    // start ~0.2 ms into the call and the device has the narrow columns' work while the first dense groups cross.
    int run_latency() {
        Item dn[W];
        int nq = 0;  // dense groups issued
        for (int g = 0; g < 2; g++)
            if (next_dense(&dn[nq])) ZK_TRY(issue(dn[nq++]));
        // (h_pack is pinned and mapped; part k's bytes are written by the pool threads before packed[k] opens and the
        // expansion kernel is launched after that, and a kernel dispatch acquires at system scope, so the kernel
        // reads this proof's bytes -- tests/test_gpu_parity.py changes a narrow column between proofs on this path)
        uint8_t *hp = nullptr;
        ZK_CHECK_HIP(hipHostGetDevicePointer((void **)&hp, p->h_pack, 0));
        for (int k = 0; k < u.np; k++) {
            Item it;
            if (!narrow_item(k, &it)) continue;
            count_part(k);
            expand_narrow(p->st, hp, G[k], n, p->d_trace);
            ZK_TRY(process(it.cols, it.nc));
        }
        for (int g = 0; g < u.ngroups; g++) {
            ZK_CHECK_HIP(hipEventSynchronize(p->ev_up[dn[g].ev]));
            if (next_dense(&dn[nq])) ZK_TRY(issue(dn[nq++]));
            ZK_TRY(process(dn[g].cols, dn[g].nc));
        }
        narrow_done[0] = narrow_done[1] = true;  // (the fallback columns, if any, go through run_throughput)
        return ZK_OK;
    }

    // The throughput schedule (other proofs in flight on the device): the first narrow part before anything else
    // (packed by the host threads in ~0.3 ms, a few MB over PCIe: the first kernels start then instead of after a
    // 64-MB dense group; one call alone -0.45 ms, 14.32-14.36 vs 14.76-14.84 ms over 3 x 31 calls,
    // profiles/r05d_latency_ab.txt), the second as soon as it is packed, the dense groups in between; narrow columns
    // that did not fit, whole, last.
    bool next_item(Item *it) {
        if ((!narrow_done[0] && narrow_item(0, it)) ||
            (!narrow_done[1] && (packed[1].ready() || gi == u.ngroups) && narrow_item(1, it))) {
            it->ev = ev++;
            return true;
        }
        if (next_dense(it)) return true;
        if (narrow_done[0] && narrow_done[1] && nfb && !fb_done) {
            fb_done = true;
            *it = Item{fallback, nfb, -1, ev++};
            return true;
        }
        return false;
    }
    int run_throughput() {
        Item cur;
        bool have = next_item(&cur);
        if (have) ZK_TRY(issue(cur));
        while (have) {
            Item nxt;
            const bool more = next_item(&nxt);
            if (more) ZK_TRY(issue(nxt));
            ZK_CHECK_HIP(hipEventSynchronize(p->ev_up[cur.ev]));
            if (cur.part >= 0) expand_narrow(p->st, stage, G[cur.part], n, p->d_trace);
            ZK_TRY(process(cur.cols, cur.nc));
            cur = nxt;
            have = more;
        }
        return ZK_OK;
    }

    int finish() {
        hash_ready(true);
        merkle_tree(p->st, p->leaves, n * B, p->nodes);
        return sp ? d2h_small(p, p->sp_h, p->sp_nz, 3 * W * sizeof(unsigned)) : ZK_OK;  // for the next proof's hints
    }

    // The snapshot of the fixed class: f_c = column - last[c] e_(n-1), coefficients and LDE, from this proof's own polys
    // and LDE, and rows 0 .. n-2 of the caller's columns for the later proofs' host check (narrow ones packed; one
    // whose values do not fit its class is left out).  Memory that is not to be had turns the class off for this hint
    // set; it never fails the proof.
    int take_snapshot() {
        const uint32_t cand = u.snap_now ? ZK_FIXED_CAND & ~u.hint : 0u;
        if (!cand) return ZK_OK;
        const int si = fixed_slot(p, (int)(H - p->hint_sets), n, (uint32_t)B, __builtin_popcount(cand));
        bool ok = si >= 0;
        snap = ok ? &p->fix_snaps[si] : nullptr;
        FixedColList L;
        fe_ws ws[W] = {};
        for (int c = 0; ok && c < W; c++) {
            if (!((cand >> c) & 1u)) continue;
            snap->width[c] = ((H->nw8 >> c) & 1u) ? 1 : ((H->nw32 >> c) & 1u) ? 4 : 16;
            snap->host[c].reset(new (std::nothrow) uint8_t[(size_t)snap->width[c] * n]);
            if (!snap->host[c]) ok = false;
            snap->slot[c] = (uint8_t)L.count;
            L.col[L.count] = (uint8_t)c;
            L.slot[L.count] = (uint8_t)L.count;
            L.count++;
            ws[c] = make_fe_ws(fe_sub(fe_zero(), last_of(c)));
        }
        if (ok && !p->fix_ws && p->arena.alloc(&p->fix_ws, W) != hipSuccess) {
            (void)hipGetLastError();
            ok = false;
        }
        if (!ok) {
            if (si >= 0) fixed_drop(p, si);
            H->fixed_off = true;
            return ZK_OK;
        }
        ZK_TRY(h2d_small(p, p->fix_ws, ws, sizeof ws));
        fixed_cols_axpy(p->st, L, true, p->polys, p->lde, pl->lagr, pl->lagr_lde, p->fix_ws, n, B, snap->fpolys, snap->flde);
        for (int k = 0; k < L.count; k++)
            row_tasks(copied, L.col[k], 0, n - 1, R, [this](int c, size_t r0, size_t r1) {
                uint8_t *dst = snap->host[c].get();
                if (snap->width[c] == 16) memcpy(dst + 16 * r0, src.cols[c] + 16 * r0, 16 * (r1 - r0));
                else if (!pack_rows(src.cols[c], r0, r1, snap->width[c], dst)) copy_bad.fetch_or(1u << c);
            });
        copied.wait();
        snap->mask = cand & ~copy_bad.load();
        snap->lwe = src.lwe;
        snap->live = true;
        snap->used = ++p->hint_stamp;
        p->tc.fix_pending = si;
        return ZK_OK;
    }

    void collect_verdicts() {
        for (Latch *l : {&checked, &clocked, &compared}) l->wait();
        p->tc.sp_bad = sparse_bad.load();
        p->tc.clk_bad = clock_bad.load() != 0;
        p->tc.fix_bad = fixed_bad.load() != 0;
    }

    int run(uint8_t root[32]) {
        classify();
        if (u.status != ZK_OK) ZK_FAIL(u.status, "too many upload groups");
        ZK_TRY(start_checks());
        ZK_TRY(fill_sparse());
        ZK_TRY(derive_clock());
        ZK_TRY(form_fixed());
        if (u.lat) ZK_TRY(run_latency());
        ZK_TRY(run_throughput());
        ZK_TRY(finish());
        ZK_TRY(take_snapshot());
        collect_verdicts();
        return d2h_small(p, root, p->nodes + 32, 32);
    }
};

}  // namespace

int zk::trace_lde_commit(zk_prover *p, Plan *pl, const TraceSrc &src, size_t n, uint8_t root[32]) {
    zk_prover::TraceOutcome &tc = p->tc;
    tc.up_bytes = 0;
    tc.up_sparse = tc.up_nw8 = tc.up_nw32 = tc.virt = 0;  // (virt: the host path may take some columns as virtual)
    // every column's coefficients in polys, unless the host path reads some at their source (HostTraceCommit::source)
    tc.coeff_src = 0;
    p->csrc = coeff_plain(p->polys, n);
    memset(p->csrc_w, 0, sizeof p->csrc_w);
    SparseCols spc{};
    const SparseCols *sp = nullptr;
    if (!src.fixed) ZK_TRY(sparse_begin(p, pl, &spc, &sp));
    tc.sp_used = sp != nullptr;
    if (src.dev) return src.fixed ? commit_device_fixed(p, pl, src, n, root) : commit_device(p, pl, src, n, sp, root);
    return HostTraceCommit(p, pl, src, n, spc, sp != nullptr).run(root);
}

// ---------------------------------------------------------------- the hints' bookkeeping (prove_impl)
bool zk::trace_hints_refuted(zk_prover *p, const TraceSrc &src, size_t n, int rc) {
    zk_prover::TraceOutcome &tc = p->tc;
    const bool voided = tc.sp_bad || tc.clk_bad || tc.fix_bad;
    // the snapshot this proof took serves the next ones only if the proof stands
    if (tc.fix_pending >= 0) {
        const int si = tc.fix_pending;
        tc.fix_pending = -1;
        if (rc == ZK_OK && !voided && src.cols && tc.sp_used) p->hint_sets[p->fix_snaps[si].owner].snap = si;
        else fixed_drop(p, si);
    }
    if (!src.cols || !tc.sp_used || !voided) return false;
    // a hint of this (n, program) was refuted: forget its column classes (and stop speculating the clock or the
    // fixed class for it if that was refuted) and its snapshot, prove again from every column
    if (zk_prover::HintSet *h = hint_find(p, n, src.key)) {
        if (tc.clk_bad) h->clk_off = true;
        if (tc.fix_bad) h->fixed_off = true;
        fixed_drop(p, h->snap);
        h->have = false;
        h->sparse = h->nw8 = h->nw32 = 0;
    }
    p->hint_redos++;
    tc = {};
    return true;
}

void zk::trace_hints_learn(zk_prover *p, const TraceSrc &src, size_t n, int rc) {
    const zk_prover::TraceOutcome &tc = p->tc;
    const bool completed = rc == ZK_OK || rc == ZK_ERR_DEGREE || rc == ZK_ERR_BUFFER_TOO_SMALL;
    if (!src.cols || !src.key || !tc.sp_used || !completed) return;
    // (the hinted sparse columns were not detected on the device: their flags stayed 0, and the host checked them)
    uint32_t found = 0, w8 = 0, w32 = 0;
    for (int c = 0; c < W; c++) {
        if (p->sp_h[c] == 0) found |= 1u << c;
        else if (p->sp_h[W + c] == 0) w8 |= 1u << c;
        else if (p->sp_h[2 * W + c] == 0) w32 |= 1u << c;
    }
    if (tc.clk_used) {  // (its flags were not detected on the device) the clock stays in the 32-bit class
        found &= ~1u;
        w8 &= ~1u;
        w32 |= 1u;
    }
    // the fixed columns were not detected either: they keep the classes the set holds them under
    const uint32_t fix_cols = tc.fix_used;
    zk_prover::HintSet *h = hint_slot(p, n, src.key);
    h->have = true;
    h->sparse = found & ~fix_cols;
    h->nw8 = (w8 & ~fix_cols) | (h->nw8 & fix_cols);
    h->nw32 = (w32 & ~fix_cols) | (h->nw32 & fix_cols);
    h->used = ++p->hint_stamp;
}
