// shard_plan_sweep.cpp -- csrc/shard_plan.hpp under the sanitizers, as a host program of its own: the sweeps of
// tests/test_shard_plan_cpu.py (every G, rep and column set; every leaf and heap node of trees of 64, 256 and 1024
// leaves) with the same properties checked in C++.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o shard_plan_sweep \
//       tools/asan/shard_plan_sweep.cpp && ./shard_plan_sweep
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../../encrypt-zkvm_amd/csrc/shard_plan.hpp"

using namespace zk;
constexpr int W = ZK_TRACE_WIDTH;

#define REQUIRE(c)                                                \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                              \
        }                                                         \
    } while (0)

static size_t check_rounds(const std::vector<int> &U, int G, int rep) {
    // exactly the plan's columns on the heap, so that a read past either end is an error
    std::vector<int> cols(U);
    const ShardRounds r = shard_round_plan(cols.data(), (int)cols.size(), G, rep);
    const std::vector<int> split(U.begin() + rep, U.end());
    REQUIRE(r.rounds == ((int)split.size() + G - 1) / G);
    size_t seen = 0;
    for (int k = 0; k < r.rounds; k++) {
        const int real = std::min<int>(G, (int)split.size() - G * k);
        REQUIRE(r.real(k) == real && real >= 1);
        bool consecutive = true;
        for (int g = 0; g < G; g++) {
            REQUIRE(r.column(k, g) == (g < real ? split[G * k + g] : -1));
            if (g > 0 && g < real) consecutive &= split[G * k + g] == split[G * k + g - 1] + 1;
            seen += g < real;
        }
        REQUIRE(r.inplace(k) == (consecutive && split[G * k] + G <= 32));
        for (int g = real; r.inplace(k) && g < G; g++) {  // padding: past W or on no interpolated column
            const int pad = r.first(k) + g;
            REQUIRE(pad >= W || std::find(U.begin(), U.end(), pad) == U.end());
        }
    }
    REQUIRE(seen == split.size());
    return (size_t)r.rounds;
}

static void check_tree(size_t M, int G) {
    TreeGeom T;
    T.shape(M, G);
    const int Bl = 8 / G, Lb = Bl == 4 ? 2 : Bl == 2 ? 1 : 0;
    const size_t Q = M / 8;
    std::map<std::tuple<int, int, size_t>, size_t> used;
    for (size_t x = 0; x < M; x++) {
        const TreeGeom::Loc L = T.locate(0, x);
        REQUIRE(L.owner == (int)(x % 8) / Bl && L.which == 2 && L.off % 32 == 0 && L.off < 32 * (2 * Bl - 1) * Q);
        REQUIRE(used.emplace(std::make_tuple(L.owner, L.which, L.off), x).second);
    }
    for (size_t idx = 1; idx < M; idx++) {
        int lv = 1;
        while ((M >> lv) > idx) lv++;
        const size_t i = idx - (M >> lv);
        const TreeGeom::Loc L = T.locate(1, idx);
        REQUIRE((L.owner == -1) == (idx < (size_t)G));
        if (L.owner < 0) continue;
        REQUIRE(L.off % 32 == 0 && L.off < 32 * (lv <= Lb ? (2 * Bl - 1) * Q : Q));
        REQUIRE(L.which == (lv <= Lb ? 2 : 1));
        REQUIRE(L.owner == (lv <= Lb ? (int)((i << lv) % 8) / Bl : (int)((i << (lv - Lb)) / Q)));
        if (lv > Lb + 1) {
            const TreeGeom::Loc a = T.locate(1, 2 * idx), b = T.locate(1, 2 * idx + 1);
            REQUIRE(a.owner == L.owner && b.owner == L.owner && a.off == 2 * L.off && b.off == 2 * L.off + 32);
        }
        REQUIRE(used.emplace(std::make_tuple(L.owner, L.which, L.off), M + idx).second);
    }
}

int main() {
    std::vector<std::vector<int>> sets;
    std::vector<int> all(W);
    for (int c = 0; c < W; c++) all[c] = c;
    sets.push_back(all);
    for (int md = 1; md <= 16; md++) sets.emplace_back(all.begin() + 12, all.begin() + 12 + md);
    for (int c = 0; c < W; c++) {
        std::vector<int> u(all);
        u.erase(u.begin() + c);
        sets.push_back(u);
    }
    std::mt19937 rng(20240607);
    for (int t = 0; t < 2000; t++) {
        std::vector<int> u;
        const uint32_t mask = rng() & ((1u << W) - 1);
        for (int c = 0; c < W; c++)
            if ((mask >> c) & 1u) u.push_back(c);
        sets.push_back(u);
    }
    size_t plans = 0, rounds = 0;
    for (int G : {2, 4, 8})
        for (const auto &U : sets)
            for (int rep : {0, 3, 4, (int)U.size()}) {
                rounds += check_rounds(U, G, std::min(rep, (int)U.size()));
                plans++;
            }
    for (size_t M : {64, 256, 1024})
        for (int G : {2, 4, 8}) check_tree(M, G);
    printf("shard_plan_sweep ok: %zu round plans (%zu rounds), 9 trees\n", plans, rounds);
    return 0;
}
