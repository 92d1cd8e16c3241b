// Mixed-key batches with H2V_MIXED_GROUPED (include/h2v.h): phase 1 of EVERY groupable plan in one launch per kernel.  HOST CODE
// ONLY - no HIP call and no HIP header in this file, so that a stand-alone C++ program can include and test it
// (tests/cpp/h2v_mixed_group.cpp).  The kernels that read these tables are in h2v_mixed_group_dev.hpp.
//
// A plan is GROUPABLE when it is foldable (h2v_mixed_fold.hpp) and its combiner register file fits LDS (P = vm_lds_slots != 0).
// The proofs of the groupable plans that have proofs, in list order, form the GROUPED POSITIONS 0 .. G: plan k owns
// [gbase[k], gbase[k] + count[k]).  Phase 1 runs over chunk ranges [g0, g1) of them - one range [0, G) on an ordinary workspace,
// ranges of `chunk` positions on a laned one - and a range may begin and end inside a plan and span many plans.  A GROUP is what
// one plan has in one range.  group_tables() gives per range
//   rec[]      one GroupRec per group, in plan order: the plan record (narrow schedule), the group's first position WITHIN the
//              range and its count, where its proofs lie in the grouped staging (off / inst / ci), where its phase-1 results go
//              in the workspace buffers - group g's sub-batch starts at `first` proofs of the UNION strides (u_terms scalars,
//              u_slots point slots per proof: the largest of the call's groupable plans, so the sub-batches cannot overlap) and
//              is laid out inside with the plan's own strides, as every per-plan kernel lays it out - and where its terms go in
//              the call's pool (term_base: its first proof's first R-term; part_base: the Fr record of its first block sum)
//   comb[t][]  prefix array of the combiner blocks of transcript kind t: ceil(count / P) for a group of that kind, 0 for the other
//   dec[]      prefix array of 64-point decompression units: ceil(count x slots / 64) per group - a unit never spans two groups
//   terms[]    prefix array of 64-proof terms blocks: ceil(count / 64) per group
// each of n_groups + 1 entries; block (unit) b belongs to the group g with prefix[g] <= b < prefix[g + 1] (group_find: binary
// search; a group with no block of that kind is never found) and is block b - prefix[g] of it.
// THE VK-BASE SUMS keep FoldLayout's ownership rule - blocks of 64 proofs within a plan, per chunk - but the chunks are those of
// the grouped positions: plan k owns one block per 64 proofs of every group it has, in range order (group_fold_blocks rewrites
// n_blocks / block_base / part_base / n_parts of the groupable plans; a call whose ranges are whole plans gets fold_layout's
// numbers back).  k_mixed_vk_sum adds a plan's blocks whatever cut produced them, and the sums are exact in Fr.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "h2v_mixed.hpp"
#include "h2v_mixed_fold.hpp"
#include "h2v_plan.h"

#ifndef H2V_GROUP_HD
#define H2V_GROUP_HD inline
#endif

// what a block of a grouped kernel reads of its group (device memory; uniform per block or unit)
struct H2vGroupRec {
    H2vDevPlan plan;            // the narrow schedule
    uint32_t first, count;      // first grouped position within the range; proofs
    uint32_t P, plan_index;     // combiner proofs per block (vm_lds_slots); the plan's place in the call's list
    uint32_t n_var, n_fix, slots, pad;
    uint64_t off_idx;           // staging position of the group's first proof: entry of the grouped offsets and of perm
    uint64_t inst_off;          // byte offset of its public inputs in the grouped staging
    uint64_t ci_idx;            // 48-byte record of its committed instance in the grouped staging
    uint64_t scal_base;         // dwords into the workspace's scalars
    uint64_t pts_base;          // point slots into pts (x 24 dwords) / valid / valid_sub
    uint64_t term_base;         // R-term of the group's first proof's first term
    uint64_t part_base;         // Fr record of the group's first block's first VK-base sum
};

// the group of block (unit) b: the g with prefix[g] <= b < prefix[g + 1].  prefix: n_groups + 1 non-decreasing entries,
// prefix[0] = 0, b < prefix[n_groups]
H2V_GROUP_HD uint32_t h2v_group_find(const uint32_t *prefix, uint32_t n_groups, uint32_t b) {
    uint32_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

namespace h2vmixed {

struct GroupShape {
    H2vDevPlan d;               // the plan record (pointers: device; the layout reads its sizes only)
    uint32_t n_var, n_fix;
    uint32_t P;                 // vm_lds_slots(d): 0 = the register file does not fit LDS
    bool foldable;
};

struct GroupSpace {
    uint32_t n_plans = 0, chunk = 0;        // chunk = 0: one range over everything
    uint32_t total = 0;                     // G
    uint32_t n_groupable = 0, n_other = 0;  // plans with proofs: groupable / every other one
    uint32_t u_terms = 0, u_slots = 0;      // union strides of the groupable plans with proofs
    std::vector<uint8_t> groupable;         // n_plans: groupable AND has proofs
    std::vector<uint32_t> gbase;            // n_plans
};

inline void group_space(const GroupShape *shapes, const uint32_t *count, uint32_t n_plans, uint32_t chunk, GroupSpace &out) {
    out = GroupSpace();
    out.n_plans = n_plans; out.chunk = chunk;
    out.groupable.assign(n_plans, 0); out.gbase.assign(n_plans, 0);
    for (uint32_t k = 0; k < n_plans; k++) {
        if (!count[k]) continue;
        if (!shapes[k].foldable || shapes[k].P == 0) { out.n_other++; continue; }
        out.groupable[k] = 1; out.n_groupable++;
        out.gbase[k] = out.total;
        out.total += count[k];
        const uint32_t slots = H2V_SLOTS(shapes[k].d);
        if (shapes[k].d.n_terms > out.u_terms) out.u_terms = shapes[k].d.n_terms;
        if (slots > out.u_slots) out.u_slots = slots;
    }
}
inline uint32_t group_ranges(const GroupSpace &s) { return s.total == 0 ? 0u : s.chunk == 0 ? 1u : (s.total + s.chunk - 1) / s.chunk; }
inline void group_range(const GroupSpace &s, uint32_t c, uint32_t &g0, uint32_t &g1) {
    if (s.chunk == 0) { g0 = 0; g1 = s.total; return; }
    g0 = c * s.chunk;
    g1 = s.total - g0 < s.chunk ? s.total : g0 + s.chunk;
}
// blocks of 64 proofs that the positions [a, b) own in the ranges that start before position `upto` (a multiple of the chunk, or
// anything >= b for all of them)
inline uint32_t group_blocks(uint32_t a, uint32_t b, uint32_t chunk, uint32_t upto) {
    if (b <= a) return 0;
    if (chunk == 0) return upto > a ? (b - a + 63) / 64 : 0u;
    uint32_t blocks = 0;
    for (uint32_t c = a / chunk; c <= (b - 1) / chunk; c++) {
        const uint64_t lo64 = (uint64_t)c * chunk, hi64 = lo64 + chunk;
        if (lo64 >= upto) break;
        const uint32_t lo = lo64 > a ? (uint32_t)lo64 : a, hi = hi64 < b ? (uint32_t)hi64 : b;
        blocks += (hi - lo + 63) / 64;
    }
    return blocks;
}
// the per-block VK-base sums of a grouped call: the groupable plans own blocks by the ranges of the grouped positions, every
// other foldable plan by fold_layout's rule
inline void group_fold_blocks(const GroupSpace &s, const GroupShape *shapes, const uint32_t *count, FoldLayout &lay) {
    lay.total_blocks = 0; lay.n_parts = 0;
    for (uint32_t k = 0; k < s.n_plans; k++) {
        if (!lay.foldable[k]) continue;
        lay.block_base[k] = lay.total_blocks;
        lay.n_blocks[k] = s.groupable[k] ? group_blocks(s.gbase[k], s.gbase[k] + count[k], s.chunk, 0xffffffffu) : fold_blocks(count[k], lay.chunk);
        lay.total_blocks += lay.n_blocks[k];
        lay.part_base[k] = lay.n_parts;
        lay.n_parts += (uint64_t)lay.n_blocks[k] * shapes[k].n_fix;
    }
}

struct GroupTables {
    std::vector<H2vGroupRec> rec;
    std::vector<uint32_t> comb[2], dec, terms;     // n_groups + 1 each
    uint32_t lds[2] = {0, 0};                      // dynamic LDS of the combiner launch of each kind: the largest n_regs x 32 x P
    uint32_t n = 0;                                // positions of the range
};
// the tables of range [g0, g1).  false (err says why): a group's results or terms would lie outside what the caller gave room for
// (cap_proofs proofs of the union strides are always enough; pool_terms / pool_parts: the call's term pool)
inline bool group_tables(const GroupSpace &s, const GroupShape *shapes, const Partition &pt, const FoldLayout &lay, uint32_t g0, uint32_t g1,
                         uint64_t pool_terms, uint64_t pool_parts, GroupTables &out, std::string *err) {
    out = GroupTables();
    out.n = g1 - g0;
    for (auto *v : {&out.comb[0], &out.comb[1], &out.dec, &out.terms}) v->assign(1, 0u);
    for (uint32_t k = 0; k < s.n_plans; k++) {
        if (!s.groupable[k]) continue;
        const uint32_t a = s.gbase[k], b = a + pt.count[k];
        const uint32_t lo = a > g0 ? a : g0, hi = b < g1 ? b : g1;
        if (lo >= hi) continue;
        const GroupShape &sh = shapes[k];
        const uint32_t j0 = lo - a, m = hi - lo, slots = H2V_SLOTS(sh.d), kind = sh.d.tr_kind;
        H2vGroupRec r = {};
        r.plan = sh.d;
        r.first = lo - g0; r.count = m; r.P = sh.P; r.plan_index = k;
        r.n_var = sh.n_var; r.n_fix = sh.n_fix; r.slots = slots;
        r.off_idx = (uint64_t)pt.base[k] + j0;
        r.inst_off = pt.inst_base[k] + (uint64_t)j0 * sh.d.n_pi * 32;
        r.ci_idx = (uint64_t)pt.ci_base[k] + (sh.d.n_ci ? j0 : 0u);
        r.scal_base = (uint64_t)r.first * s.u_terms * 8;
        r.pts_base = (uint64_t)r.first * s.u_slots;
        r.term_base = (uint64_t)lay.term_base[k] + (uint64_t)j0 * sh.n_var;
        r.part_base = lay.part_base[k] + (uint64_t)group_blocks(a, b, s.chunk, g0) * sh.n_fix;
        if (kind >= 2 || sh.P == 0 || (sh.P & (sh.P - 1)) || sh.P > 64 || sh.d.n_terms > s.u_terms || slots > s.u_slots) {
            if (err) *err = "internal: plan " + std::to_string(k) + " cannot be grouped";
            return false;
        }
        if (r.term_base + (uint64_t)m * sh.n_var > pool_terms || r.part_base + (uint64_t)((m + 63) / 64) * sh.n_fix > pool_parts) {
            if (err) *err = "internal: a group's terms lie outside the call's term pool";
            return false;
        }
        out.rec.push_back(r);
        out.comb[kind].push_back(out.comb[kind].back() + (m + sh.P - 1) / sh.P);
        out.comb[kind ^ 1].push_back(out.comb[kind ^ 1].back());
        out.dec.push_back(out.dec.back() + (uint32_t)(((uint64_t)m * slots + 63) / 64));
        out.terms.push_back(out.terms.back() + (m + 63) / 64);
        const uint32_t lds = sh.d.n_regs * 32 * sh.P;
        if (lds > out.lds[kind]) out.lds[kind] = lds;
    }
    return true;
}

}   // namespace h2vmixed
