// shard_plan.hpp -- the two decisions of the coset-sharded prover (shard.hip) that need no device: which column each
// rank interpolates in each round of the trace split and where a round's all-gather lands, and which rank and buffer
// holds a node of a Merkle tree split over the ranks.  No HIP (tests/test_shard_plan_cpu.py drives them through
// zk_diag_shard_rounds and zk_diag_shard_locate).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkvm_gpu.h"

namespace zk {

// The trace split: of the nU columns U[] (ascending) the first `rep` are interpolated by every rank itself; the rest,
// US[0 .. nS), go round robin: in round k rank g interpolates US[G k + g], and an all-gather fills the round's columns
// on every rank.  A round whose columns are consecutive is gathered in place, rank g's chunk landing on column
// first + g: the padding chunks of a short last round (g >= real) then land above every column of U -- on columns that
// are formed after the rounds, or past W (the coefficient buffer holds 8 ceil(W / 8) columns).
struct ShardRounds {
    const int *US = nullptr;
    int nS = 0, G = 1, rounds = 0;
    int real(int k) const { return nS - G * k < G ? nS - G * k : G; }  // round k's columns (a last round may be short)
    int first(int k) const { return US[G * k]; }
    int column(int k, int g) const { return G * k + g < nS ? US[G * k + g] : -1; }  // rank g's column, or none
    bool inplace(int k) const {
        constexpr int W = ZK_TRACE_WIDTH;
        return US[G * k + real(k) - 1] - first(k) == real(k) - 1 && first(k) + G <= 8 * ((W + 7) / 8);
    }
};
inline ShardRounds shard_round_plan(const int *U, int nU, int G, int rep) {
    return {U + rep, nU - rep, G, (nU - rep + G - 1) / G};
}

// A Merkle tree split over G ranks: M leaves in natural order (leaf 8q + r: group q, coset r).  Levels 0 .. Lb
// (Lb = log2 Bl) live in each coset owner's block buffer (level l: node (q, i) at lvl_off(l) + q (Bl >> l) + i); above
// them rank d holds the subtree over level-Lb nodes [d Q, (d+1) Q) (Q = M / 8) as a heap (level Lb + 1 at [Q/2, Q), ...,
// its root at 1); the top (heap nodes below G) is kept on the host.
struct TreeGeom {
    size_t M = 0, Mr = 0, Q = 0;
    int G = 1, Bl = 1, Lb = 0;
    void shape(size_t leaves, int world) {
        M = leaves, G = world, Mr = M / G, Q = M / 8, Bl = 8 / G;
        Lb = Bl == 4 ? 2 : Bl == 2 ? 1 : 0;
    }
    // chunk source of global leaf idx (is_node 0) or heap node idx (leaves are M + i): owner rank, buffer (1 subtree
    // nodes, 2 block buffer), byte offset; owner -1 = host top node
    struct Loc {
        int owner;
        int which;
        size_t off;
    };
    size_t lvl_off(int l) const {  // level l's first node in a block buffer
        size_t o = 0;
        for (int t = 0; t < l; t++) o += Q * (size_t)(Bl >> t);
        return o;
    }
    Loc locate(int is_node, uint64_t idx) const {
        int L = 0;
        uint64_t i = idx;
        if (is_node) {
            L = 1;
            while ((M >> L) > idx) L++;
            i = idx - (M >> L);
        }
        if (L <= Lb) {  // a block level: on the owner of the node's cosets
            const uint64_t per = (uint64_t)8 >> L, bl = (uint64_t)Bl >> L, q = i / per, rr = i % per;
            return {(int)(rr / bl), 2, 32 * (lvl_off(L) + q * bl + rr % bl)};
        }
        const size_t c = Mr >> L;
        if (c == 0) return {-1, 0, 32 * idx};
        return {(int)(i / c), 1, 32 * (c + i % c)};
    }
};

}  // namespace zk
