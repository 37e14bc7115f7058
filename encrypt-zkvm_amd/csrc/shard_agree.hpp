// shard_agree.hpp -- what the ranks of a coset-sharded proof (shard.hip) agree on before anything touches the GPU, and
// how the row windows of a sharded trace validation are merged.  Every rank builds one AgreeRecord from its own
// arguments and state, the records are all-gathered over the communicator's control channel (comm.hpp control_gather),
// and agree() maps the `world` records to ONE outcome: the same on every rank, because every rank runs the same pure
// function on the same bytes.  No HIP (tests/test_shard_agree_cpu.py drives both rules through zk_diag_agree and
// zk_diag_merge_validation).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../include/zkvm_gpu.h"
#include "air_shape.hpp"

namespace zk {

constexpr uint32_t ZK_AGREE_VERSION = 1;
constexpr int ZK_AGREE_MSG = 120;

// One rank's record, 256 bytes, little-endian, in this (layout) order.  Must match on every rank: world, n, every
// member of zk_options, the BLAKE3 of zk_pub_inputs, the trace source, and the communicator's two settings (both
// change the number of collectives).  Decided from all records: detect, clock, the hint set, validate,
// validate_degrees (the first 4 of the once 16 reserved bytes: a record of an older build reads as "off").
enum { ZK_SRC_HOST = 0, ZK_SRC_DEVICE = 1, ZK_SRC_FIXED = 2 };
struct AgreeRecord {
    uint32_t version, world, rank;
    int32_t status;  // the code this rank's own checks produced (ZK_OK if none), its text in msg
    uint64_t n;
    uint32_t opt[6];       // zk_options, member by member
    uint8_t pub_hash[32];  // BLAKE3 of the zk_pub_inputs bytes
    uint32_t source;       // ZK_SRC_*
    int32_t split_rep;     // zk_comm_set_trace_split
    uint32_t measure;      // zk_comm_set_measure
    uint32_t validate;     // zk_prover_set_validate of this rank's prover(s)
    uint32_t detect;       // bit 0: sparse_begin would return a detector here; bit 1: the clock may be derived here
    // the hint set this rank would use for a host trace (shard.hip classify_host), all zero when not fresh
    uint32_t hint_fresh, hint_S, hint_clk, hint_N8, hint_N32;
    char msg[ZK_AGREE_MSG];  // the first bytes of the status' message, NUL-padded
    uint32_t validate_degrees;  // zk_prover_set_validate_degrees of this rank's prover(s)
    uint8_t reserved[12];
};
static_assert(sizeof(AgreeRecord) == 256, "the control record is a fixed 256-byte layout");

struct HintSet {
    uint32_t fresh = 0, S = 0, clk = 0, N8 = 0, N32 = 0;
    bool operator==(const HintSet &o) const {
        return fresh == o.fresh && S == o.S && clk == o.clk && N8 == o.N8 && N32 == o.N32;
    }
};

// the outcome (zk_agreement carries the public part) and the hint set the ranks use
struct Agreed {
    zk_agreement a = {};
    HintSet hints;
    std::string msg;  // the text of a non-OK outcome, the same on every rank
};

static const char *const ZK_OPT_NAMES[6] = {"options.num_queries",     "options.blowup",      "options.grinding",
                                            "options.field_extension", "options.fri_folding", "options.fri_rem_max_deg"};

namespace agree_detail {
inline std::string hex8(const uint8_t *b) {
    char t[20];
    for (int i = 0; i < 8; i++) snprintf(t + 2 * i, 3, "%02x", b[i]);
    return std::string(t) + "..";
}
// the two lowest ranks holding different values of one field: rank 0 and the first rank that differs from it
template <class Same>
inline int first_other(int world, Same same) {
    for (int r = 1; r < world; r++)
        if (!same(r)) return r;
    return -1;
}
}  // namespace agree_detail

// The rule.  1: a record of another layout version is refused.  2: a rank with a non-OK status -- the lowest is named,
// code ZK_ERR_PEER (that rank itself returns its own code and text: shard.hip).  3: a must-match field differs -- the
// first in layout order is named with the two lowest ranks that hold different values, code ZK_ERR_INVALID_ARG.
// 4: the decisions: detect and clock = AND, validate and validate_degrees = OR, hints = rank 0's set if every rank's
// set is equal.
inline Agreed agree(const AgreeRecord *R, int world) {
    using namespace agree_detail;
    Agreed A;
    zk_agreement &a = A.a;
    a.world = (uint32_t)world;
    a.rank_a = a.rank_b = -1;
    auto disagree = [&](const char *field, int rb, const std::string &va, const std::string &vb) {
        a.code = ZK_ERR_INVALID_ARG;
        a.rank_a = 0;
        a.rank_b = rb;
        snprintf(a.field, sizeof a.field, "%s", field);
        A.msg = std::string("sharded proof: ranks disagree on ") + field + " (rank 0: " + va + ", rank " +
                std::to_string(rb) + ": " + vb + ")";
    };
    for (int r = 0; r < world; r++)
        if (R[r].version != ZK_AGREE_VERSION) {
            a.code = ZK_ERR_INVALID_ARG;
            a.rank_a = r;
            snprintf(a.field, sizeof a.field, "version");
            A.msg = "sharded proof: rank " + std::to_string(r) + " sent a control record of layout version " +
                    std::to_string(R[r].version) + " (this library: " + std::to_string(ZK_AGREE_VERSION) + ")";
            return A;
        }
    for (int r = 0; r < world; r++)
        if (R[r].status != ZK_OK) {
            a.code = ZK_ERR_PEER;
            a.rank_a = r;
            snprintf(a.field, sizeof a.field, "status");
            char m[ZK_AGREE_MSG + 1];
            memcpy(m, R[r].msg, ZK_AGREE_MSG);
            m[ZK_AGREE_MSG] = 0;
            A.msg = "rank " + std::to_string(r) + " refused the proof: " + std::to_string(R[r].status) + ": " + m;
            return A;
        }
    int o;
    auto u = [](uint64_t v) { return std::to_string(v); };
    if ((o = first_other(world, [&](int r) { return R[r].world == R[0].world; })) >= 0)
        return disagree("world", o, u(R[0].world), u(R[o].world)), A;
    if (R[0].world != (uint32_t)world) {
        a.code = ZK_ERR_INVALID_ARG;
        snprintf(a.field, sizeof a.field, "world");
        A.msg = "sharded proof: the control records are of world " + u(R[0].world) + ", the communicator of " + u(world);
        return A;
    }
    if ((o = first_other(world, [&](int r) { return R[r].n == R[0].n; })) >= 0)
        return disagree("n", o, u(R[0].n), u(R[o].n)), A;
    for (int k = 0; k < 6; k++)
        if ((o = first_other(world, [&](int r) { return R[r].opt[k] == R[0].opt[k]; })) >= 0)
            return disagree(ZK_OPT_NAMES[k], o, u(R[0].opt[k]), u(R[o].opt[k])), A;
    if ((o = first_other(world, [&](int r) { return !memcmp(R[r].pub_hash, R[0].pub_hash, 32); })) >= 0)
        return disagree("public inputs (BLAKE3)", o, hex8(R[0].pub_hash), hex8(R[o].pub_hash)), A;
    static const char *const src[3] = {"host", "device", "preprocessed"};
    auto sn = [&](uint32_t s) { return std::string(s < 3 ? src[s] : "?"); };
    if ((o = first_other(world, [&](int r) { return R[r].source == R[0].source; })) >= 0)
        return disagree("trace source", o, sn(R[0].source), sn(R[o].source)), A;
    if ((o = first_other(world, [&](int r) { return R[r].split_rep == R[0].split_rep; })) >= 0)
        return disagree("comm.trace_split", o, std::to_string(R[0].split_rep), std::to_string(R[o].split_rep)), A;
    if ((o = first_other(world, [&](int r) { return R[r].measure == R[0].measure; })) >= 0)
        return disagree("comm.measure", o, u(R[0].measure), u(R[o].measure)), A;
    uint32_t det = 3u, val = 0, vdeg = 0;
    bool same = true;
    const HintSet h0{R[0].hint_fresh, R[0].hint_S, R[0].hint_clk, R[0].hint_N8, R[0].hint_N32};
    for (int r = 0; r < world; r++) {
        det &= R[r].detect;
        val |= R[r].validate;
        vdeg |= R[r].validate_degrees;
        same = same && HintSet{R[r].hint_fresh, R[r].hint_S, R[r].hint_clk, R[r].hint_N8, R[r].hint_N32} == h0;
    }
    a.code = ZK_OK;
    a.detect = (int32_t)(det & 1u);
    a.clock = (int32_t)((det >> 1) & 1u);
    a.validate = val ? 1 : 0;
    a.validate_degrees = vdeg ? 1 : 0;
    a.hints_equal = same ? 1 : 0;
    a.hints = same && h0.fresh ? 1 : 0;
    if (a.hints) A.hints = h0;
    return A;
}

// ---------------------------------------------------------------- sharded trace validation: one rank's window
// Rank g of G checks steps [g n / G, min((g + 1) n / G, n - 2)); the rank that holds row 0 checks the twelve row-0
// assertions, the rank whose window ends at row n - 2 the ten there (assertion k of get_assertions: k = 0, 1 and the
// even k >= 2 are at row 0, the odd k >= 2 at row n - 2).
constexpr uint32_t ZK_ASSERT_ROW0 = 0x155557u, ZK_ASSERT_LAST = 0x2aaaa8u;
static_assert((ZK_ASSERT_ROW0 ^ ZK_ASSERT_LAST) == 0x3fffffu && !(ZK_ASSERT_ROW0 & ZK_ASSERT_LAST), "22 assertions");
struct ValWindow {
    uint64_t first, count;
    uint32_t amask;
};
inline ValWindow val_window(uint64_t n, int g, int G) {
    const uint64_t a = n * (uint64_t)g / (uint64_t)G, e = n * (uint64_t)(g + 1) / (uint64_t)G;
    const uint64_t end = e < n - 2 ? e : n - 2;
    ValWindow w{a, end - a, 0};
    if (a == 0) w.amask |= ZK_ASSERT_ROW0;
    if (end == n - 2) w.amask |= ZK_ASSERT_LAST;
    return w;
}

// One rank's partial report, 1160 bytes, little-endian.  t_value[k] is filled by the rank whose window holds
// t_first[k] (the host evaluator at that step); a_found[k] by the rank whose amask has bit k.
struct ValPartial {
    uint32_t version, rank;
    int32_t status;  // ZK_OK, or the code of an error (not a failing trace) on this rank, its text in msg
    uint32_t amask;  // the assertions this rank checked
    uint64_t first, count;
    uint64_t failing_steps;
    uint64_t t_count[20], t_first[20];  // t_first: global steps, UINT64_MAX if none
    uint8_t t_value[20][16];
    uint32_t a_mask, pad_;
    uint8_t a_found[22][16];
    char msg[ZK_AGREE_MSG];
};
static_assert(sizeof(ValPartial) == 1160, "the validation partial is a fixed layout");

// The merge: counts add, firsts take the minimum (the value comes from the rank that reported that minimum), masks OR,
// found cells from the rank that checked them.  Fills the counted fields of V (failing_steps, t_*, a_mask, a_failed,
// a_found); the caller fills what follows from n and the public inputs.  Returns ZK_OK, or ZK_ERR_PEER with the lowest
// rank whose partial carries an error in *bad (that rank's own code is P[*bad].status).
inline int merge_validation(const ValPartial *P, int world, zk_validation *V, int *bad) {
    *bad = -1;
    for (int r = 0; r < world; r++)
        if (P[r].status != ZK_OK || P[r].version != ZK_AGREE_VERSION) {
            *bad = r;
            return ZK_ERR_PEER;
        }
    V->failing_steps = 0;
    V->a_mask = 0;
    for (int k = 0; k < 20; k++) {
        V->t_count[k] = 0;
        V->t_first[k] = UINT64_MAX;
        memset(V->t_value[k], 0, 16);
    }
    for (int r = 0; r < world; r++) {
        V->failing_steps += P[r].failing_steps;
        V->a_mask |= P[r].a_mask & P[r].amask;
        for (int k = 0; k < 20; k++) {
            V->t_count[k] += P[r].t_count[k];
            if (P[r].t_count[k] && P[r].t_first[k] < V->t_first[k]) {
                V->t_first[k] = P[r].t_first[k];
                memcpy(V->t_value[k], P[r].t_value[k], 16);
            }
        }
        for (int k = 0; k < 22; k++)
            if ((P[r].amask >> k) & 1u) memcpy(V->a_found[k], P[r].a_found[k], 16);
    }
    V->a_failed = (uint32_t)__builtin_popcount(V->a_mask);
    return ZK_OK;
}

// ---------------------------------------------------------------- sharded degree check: one rank's coefficient range
// Rank g of G receives, of every quotient Q_k, the 8 per-coset coefficient slices k1 in [g n / G, (g + 1) n / G) and
// forms the coefficients k1 + n k2, k2 < 8, from them (kernels.hip k_cross_degrees).  One rank's partial report, 312
// bytes, little-endian: top[k] is the highest GLOBAL index k1 + n k2 it found non-zero in Q_k (0 if none: bit k of
// nonzero tells the two apart, as DegReport does).
struct DegPartial {
    uint32_t version, rank;
    int32_t status;    // ZK_OK, or the code of an error on this rank, its text in msg
    uint32_t nonzero;  // bit k: Q_k has a non-zero coefficient in this rank's range
    uint64_t first, count;  // the k1 range
    uint64_t top[20];
    char msg[ZK_AGREE_MSG];
};
static_assert(sizeof(DegPartial) == 312, "the degree partial is a fixed layout");

// Rust's {:>3?} of a Vec<usize>: every element right-aligned in 3 columns
inline std::string rust_vec3(const uint64_t *v, int k) {
    std::string s = "[";
    for (int i = 0; i < k; i++) {
        std::string e = std::to_string(v[i]);
        if (e.size() < 3) e.insert(0, 3 - e.size(), ' ');
        s += (i ? ", " : "") + e;
    }
    return s + "]";
}
// The report of a degree check from the 20 tops and the non-zero bits (zk_degrees_device on one GPU, merge_degrees
// over the ranks): expected from the AIR's declared degrees, the masks, max_actual and ce_len_needed.
inline void degrees_report(size_t n, const uint64_t *top, uint32_t nonzero, zk_degrees *D) {
    memset(D, 0, sizeof *D);
    D->trace_len = n;
    D->ce_len = 8 * (uint64_t)n;
    const DeclaredDegrees &decl = air_declared_degrees();
    for (int k = 0; k < 20; k++) {
        D->expected[k] = decl.evaluation_degree(k, n) - (n - 2);
        D->actual[k] = top[k];
        if (!((nonzero >> k) & 1u)) D->zero_mask |= 1u << k;
        if (D->actual[k] != D->expected[k]) D->mismatch_mask |= 1u << k;
        if (D->actual[k] > D->expected[k]) D->over_mask |= 1u << k;
        D->max_actual = std::max(D->max_actual, D->actual[k]);
    }
    D->ce_len_needed = 1;
    while (D->ce_len_needed < std::max<uint64_t>(D->max_actual, n + 1)) D->ce_len_needed *= 2;
}
// winterfell's three-line message of a mismatch
inline std::string degrees_message(const zk_degrees &D) {
    return "transition constraint degrees didn't match\nexpected: " + rust_vec3(D.expected, 20) +
           "\nactual:   " + rust_vec3(D.actual, 20);
}

// The merge: top = the maximum over the ranks of the global index (a rank with a lower k1 range wins with a higher
// block k2), nonzero = OR; the rest of the report as degrees_report fills it.  ZK_OK, or ZK_ERR_PEER with the lowest
// rank whose partial carries an error, another layout version or a coefficient outside the domain in *bad.
inline int merge_degrees(const DegPartial *P, int world, size_t n, zk_degrees *D, int *bad) {
    *bad = -1;
    for (int r = 0; r < world; r++) {
        bool ok = P[r].status == ZK_OK && P[r].version == ZK_AGREE_VERSION;
        for (int k = 0; ok && k < 20; k++) ok = P[r].top[k] < 8 * (uint64_t)n;
        if (!ok) {
            *bad = r;
            return ZK_ERR_PEER;
        }
    }
    uint64_t top[20] = {};
    uint32_t nonzero = 0;
    for (int r = 0; r < world; r++) {
        nonzero |= P[r].nonzero & 0xfffffu;
        for (int k = 0; k < 20; k++)
            if ((P[r].nonzero >> k) & 1u) top[k] = std::max(top[k], P[r].top[k]);
    }
    degrees_report(n, top, nonzero, D);
    return ZK_OK;
}

}  // namespace zk
