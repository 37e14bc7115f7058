// upload_plan.hpp -- everything the host-trace commitment (trace_commit.hip) decides before it touches the device: the
// column classes of this proof, the upload items and the fused hash prefix, as one pure function of the hint set, the
// snapshot, the schedule and the switches.  No HIP (tests/test_upload_plan_cpu.py drives it: zk_diag_upload_plan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkvm_gpu.h"

namespace zk {

// a host-resident trace is uploaded in up to this many column groups (one upload event each; shard.hip: one per round
// of its column split, ceil(W / G) rounds)
static constexpr int ZK_UPLOAD_GROUPS_MAX = 14;
// Virtual columns: the first trace column no transition constraint or assertion reads -- the evaluator reads columns
// 0 .. 12 + 2 lwe_size - 1 <= 21 (enforce_add2 reads 2 lwe_size stack items, lwe_size <= 5; constrains.rs) -- so a
// hinted sparse column from here on needs no LDE in memory (ZK_VIRTUAL=0 writes it)
constexpr int ZK_VIRT_MIN_COL = 22;
constexpr uint32_t ZK_FIXED_CAND = 0xFFEu;  // the fixed class: columns 1 .. 11

struct UploadPlanIn {
    // the hint set of (n, program) (zk_prover::HintSet; have = false without one)
    bool have = false, clk_off = false, fixed_off = false;
    uint32_t sparse = 0, nw8 = 0, nw32 = 0;
    bool snap = false;       // the set has a usable snapshot (zk_prover::FixedSnap) ...
    uint32_t snap_mask = 0;  // ... of these columns
    bool hint_ok = true, no_virtual = false;  // TraceSrc
    bool lat_sched = false, detect = true;  // detect: the detection runs; without it no hint is used or learned
    // the switches (ZK_SPARSE, ZK_NARROW, ZK_CLOCK, ZK_FIXED, ZK_FIXED_FUSE, ZK_VIRTUAL, ZK_COEFF_SRC)
    bool sparse_on = true, narrow_on = true, clock_on = true, fixed_on = true, fixed_fuse_on = true, virtual_on = true;
    bool coeff_src_on = true;
    size_t n = 0;
};

struct UploadPlan {
    static constexpr int W = ZK_TRACE_WIDTH;
    int status = ZK_OK;  // ZK_ERR_INVALID_ARG: more upload items than ZK_UPLOAD_GROUPS_MAX
    // hinted sparse (zero but the last row: nothing goes up but that value); narrow (8- or 32-bit before the last row:
    // packed); fixm: formed from the snapshot; virt: hinted sparse and never written
    uint32_t hint = 0, nw8 = 0, nw32 = 0, fixm = 0, virt = 0;
    bool clk = false;       // column 0 derived from the AIR clock
    bool fix_ok = false;    // the fixed class is on for this proof: with a snapshot it is used (fixm), ...
    bool snap_now = false;  // ... without one this proof takes it
    bool lat = false;       // the latency schedule's issue order (only with narrow columns)
    // the columns that go up whole, the hinted sparse ones (hnv: those whose LDE is written), the narrow ones
    int dense[W] = {}, nd = 0, hin[W] = {}, nh = 0, hnv[W] = {}, nhv = 0, nar[W] = {}, nn = 0;
    // narrow column nar[i]: bytes per row and its 16-byte-rounded offset in h_pack
    int width[W] = {};
    size_t off[W] = {}, pack_bytes = 0;
    int pb[W + 1] = {}, np = 0;    // narrow part k: nar[pb[k]] .. nar[pb[k + 1] - 1]
    int gsz[W] = {}, ngroups = 0;  // the dense groups' sizes, in dense[] order
    int fuse_nb = 0;               // leading BLAKE3 blocks whose columns' LDE is formed inside their row hash
    // The coefficients of the derived clock, the fixed columns and the hinted sparse columns are not written: the stages
    // that read trace coefficients (boundary quotient, OOD frame, DEEP) take them at their source (CoeffSrc)
    bool coeff_src = false;
};

inline UploadPlan upload_plan(const UploadPlanIn &in) {
    constexpr int W = UploadPlan::W;
    UploadPlan P;
    const bool fresh = in.detect && in.sparse_on && in.hint_ok && in.have;
    P.hint = fresh ? in.sparse : 0u;
    P.nw8 = fresh && in.narrow_on ? in.nw8 & ~P.hint : 0u;
    P.nw32 = fresh && in.narrow_on ? in.nw32 & ~P.hint & ~P.nw8 : 0u;
    // The AIR clock: constraint 0 (clk' = clk + 1, air/src/constrains.rs) and the assertion clk[0] = 0 force rows
    // 0 .. n-2 of column 0 of any trace the AIR accepts to 0 .. n-2, so its interpolant and LDE are the identity column's
    // plus (last - (n - 1)) times e_(n-1)'s: no upload, no transform.  Taken once a proof found column 0 32-bit.
    P.clk = fresh && in.clock_on && (P.nw32 & 1u) && !in.clk_off;
    if (P.clk) P.nw32 &= ~1u;
    // Fixed columns: the columns the set's snapshot holds (but the ones hinted sparse) are formed from it; without one,
    // this proof takes it
    P.fix_ok = fresh && in.fixed_on && !in.fixed_off;
    const bool snap = P.fix_ok && in.snap;
    P.fixm = snap ? in.snap_mask & ~P.hint : 0u;
    P.snap_now = P.fix_ok && !snap;
    P.virt = !in.no_virtual && in.virtual_on ? P.hint & ~((1u << ZK_VIRT_MIN_COL) - 1u) : 0u;
    for (int c = 0; c < W; c++) {
        if ((P.clk && c == 0) || ((P.fixm >> c) & 1u)) continue;
        if ((P.hint >> c) & 1u) {
            P.hin[P.nh++] = c;
            if (!((P.virt >> c) & 1u)) P.hnv[P.nhv++] = c;
        } else if (((P.nw8 | P.nw32) >> c) & 1u) {
            P.nar[P.nn++] = c;
        } else {
            P.dense[P.nd++] = c;
        }
    }
    for (int i = 0; i < P.nn; i++) {
        P.width[i] = ((P.nw8 >> P.nar[i]) & 1u) ? 1 : 4;
        P.off[i] = P.pack_bytes;
        P.pack_bytes += ((size_t)P.width[i] * in.n + 15) & ~(size_t)15;
    }
    // narrow parts: 1, 2, 2, ... columns on the latency schedule (each packed in ~0.1-0.2 ms), else two halves
    P.lat = in.lat_sched && P.nn > 0;
    if (P.lat) {
        for (int i = 0; i < P.nn;) {
            i += P.np == 0 ? 1 : 2;
            if (i > P.nn) i = P.nn;
            P.pb[++P.np] = i;
        }
    } else if (P.nn) {
        P.pb[1] = (P.nn + 1) / 2;
        P.pb[2] = P.nn;
        P.np = P.pb[1] < P.nn ? 2 : 1;
    }
    // The wide columns in groups of 4, the last 4 as 2 + 2: after the last copy only 2 columns' NTTs, the last hash
    // blocks and the Merkle tree remain (a first group of 1 or 2 columns, so the first kernels start after a shorter
    // copy, measured slower: latency 13.90-13.95 vs 13.73-13.79 ms, throughput unchanged; r04h_ab_first_group.txt;
    // round 5, 3 x 31 single calls: 14.75-14.78 / 14.67-14.70 vs 14.76-14.84 ms, profiles/r05d_latency_ab.txt).
    for (int left = P.nd; left > 0; left -= P.gsz[P.ngroups - 1]) {
        const int k = left > 4 ? 4 : left > 2 ? 2 : left;
        P.gsz[P.ngroups++] = left == 4 ? 2 : k;
    }
    if (P.ngroups + (P.lat ? 1 : P.np + 1) > ZK_UPLOAD_GROUPS_MAX) P.status = ZK_ERR_INVALID_ARG;
    // The fused prefix: with the fixed class in use, the leading blocks whose columns are each fixed, the derived clock,
    // or hinted sparse with their LDE filled get their columns' LDE formed inside their row hash (fixed_hash: blocks
    // 0 .. 2 of the benchmark program).  Empty without the derived clock (column 0 is in block 0).
    if (P.fixm && in.fixed_fuse_on) {
        const uint32_t pre = (P.clk ? 1u : 0u) | P.fixm | (P.hint & ~P.virt);
        while (P.fuse_nb < W / 4 && ((pre >> (4 * P.fuse_nb)) & 0xFu) == 0xFu) P.fuse_nb++;
    }
    // Coefficient sources: the proofs that form columns from a snapshot (steady state).  The proof that takes the
    // snapshot reads its own fully written polys, and a caller that reads the trace polynomials (stage dumps:
    // no_virtual) gets every plane written.
    P.coeff_src = in.coeff_src_on && !in.no_virtual && P.fixm != 0;
    return P;
}

}  // namespace zk
