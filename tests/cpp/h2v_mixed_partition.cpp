// Stand-alone test of the host side of mixed-key batches (csrc/h2v_mixed.hpp: partition, group_offsets).  Host code only: built
// with -fsanitize=address,undefined and run as a program (tests/test_mixed_keys.py).  Every check compares with a direct
// restatement: walk the caller's order once, keeping per-plan lists and running source offsets.
// Prints "ok <checks>" and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed.hpp"
#include "../../include/h2v.h"

using namespace h2vmixed;

static int checks = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        checks++;                                                                           \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

// the four shapes the GPU tests mix: (proof_len, public inputs, committed instances) of simple_mul, lookup_table, trashcan_mix, ivc
static const PlanShape SHAPES[4] = {{1120, 3, 0}, {2544, 1, 0}, {2352, 5, 1}, {1840, 28, 0}};

static void verify(const std::vector<PlanShape> &shapes, const std::vector<uint32_t> &plan_of, const std::vector<uint64_t> &off) {
    const uint32_t n = (uint32_t)plan_of.size(), K = (uint32_t)shapes.size();
    Partition p;
    std::string err;
    CHECK(partition(shapes.data(), K, plan_of.data(), n, p, &err));
    CHECK(p.n == n && p.n_plans == K && p.perm.size() == n);
    // restatement
    std::vector<std::vector<uint32_t>> members(K);
    std::vector<uint64_t> src_inst(n);
    std::vector<uint32_t> src_ci(n, H2V_MIXED_NONE);
    uint64_t run_inst = 0, cap = 0;
    uint32_t run_ci = 0;
    for (uint32_t i = 0; i < n; i++) {
        const PlanShape &s = shapes[plan_of[i]];
        members[plan_of[i]].push_back(i);
        src_inst[i] = run_inst;
        run_inst += 32ull * s.n_pi;
        if (s.n_ci) src_ci[i] = run_ci++;
        cap += s.proof_len;
    }
    CHECK(p.inst_total == run_inst && p.ci_total == run_ci && p.proof_cap == cap);
    uint32_t g = 0, ci_at = 0;
    uint64_t inst_at = 0;
    std::vector<bool> seen(n, false);
    for (uint32_t k = 0; k < K; k++) {
        CHECK(p.count[k] == members[k].size());
        CHECK(p.base[k] == g && p.inst_base[k] == inst_at && p.ci_base[k] == ci_at);
        for (uint32_t j = 0; j < members[k].size(); j++, g++) {
            const uint32_t i = members[k][j];
            CHECK(p.perm[g] == i);                                   // grouped by plan, the caller's order kept inside a plan: stable
            CHECK(!seen[i]);
            seen[i] = true;
            CHECK(p.len_cap[g] == shapes[k].proof_len && p.inst_len[g] == 32 * shapes[k].n_pi);
            CHECK(p.inst_src[g] == src_inst[i] && p.inst_dst[g] == inst_at + 32ull * shapes[k].n_pi * j);
            CHECK(p.ci_src[g] == src_ci[i]);
            CHECK(p.ci_dst[g] == (shapes[k].n_ci ? ci_at + j : H2V_MIXED_NONE));
        }
        inst_at += 32ull * shapes[k].n_pi * members[k].size();
        if (shapes[k].n_ci) ci_at += (uint32_t)members[k].size();
    }
    CHECK(g == n);
    if (!off.empty()) {
        std::vector<uint64_t> grouped(n + 1, ~0ull);
        group_offsets(p, off.data(), grouped.data());
        CHECK(grouped[0] == 0);
        for (uint32_t q = 0; q < n; q++) {
            const uint64_t len = off[p.perm[q] + 1] - off[p.perm[q]];
            CHECK(grouped[q + 1] - grouped[q] == (len < p.len_cap[q] ? len : p.len_cap[q]));
        }
        CHECK(grouped[n] <= p.proof_cap);
    }
}

int main() {
    const std::vector<PlanShape> four(SHAPES, SHAPES + 4);
    // n = 0, also with no plan at all
    verify(four, {}, {0});
    verify({}, {}, {0});
    // n = 1, for each shape
    for (uint32_t k = 0; k < 4; k++) verify(four, {k}, {7, 7 + SHAPES[k].proof_len});
    // an interleaved batch with a listed plan that has no proof (index 1), full-length, truncated and over-long records
    {
        std::vector<uint32_t> plan_of;
        std::vector<uint64_t> off{0};
        uint32_t x = 12345;
        for (int i = 0; i < 145; i++) {
            x = x * 1664525u + 1013904223u;
            const uint32_t k = (x >> 16) % 3, plan = k == 1 ? 3 : k;          // plans 0, 2, 3
            plan_of.push_back(plan);
            const uint32_t full = SHAPES[plan].proof_len;
            off.push_back(off.back() + (i % 7 == 3 ? full - 1 : i % 11 == 5 ? full + 9 : full));
        }
        verify(four, plan_of, off);
    }
    // every proof of one plan; five proofs of four plans
    verify(four, std::vector<uint32_t>(70, 2), {});
    verify(four, {3, 0, 2, 1, 0}, {});
    // H2V_MIXED_MAX_PLANS plans of one proof each, listed in reverse
    {
        std::vector<PlanShape> many;
        std::vector<uint32_t> plan_of;
        for (uint32_t k = 0; k < H2V_MIXED_MAX_PLANS; k++) { many.push_back(SHAPES[k % 4]); plan_of.push_back(H2V_MIXED_MAX_PLANS - 1 - k); }
        verify(many, plan_of, {});
    }
    // an out-of-range plan_of is refused, and named
    {
        Partition p;
        std::string err;
        const uint32_t bad[3] = {0, 4, 1};
        CHECK(!partition(four.data(), 4, bad, 3, p, &err));
        CHECK(err.find("plan_of[1]") != std::string::npos);
        const uint32_t edge[1] = {0};
        CHECK(!partition(four.data(), 0, edge, 1, p, &err));
    }
    std::printf("ok %d\n", checks);
    return 0;
}
