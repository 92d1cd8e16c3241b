// Mixed-key batches (include/h2v.h: h2v_verify_mixed): the host side of the partition.  HOST CODE ONLY - no HIP call and no
// HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_mixed_partition.cpp).
//
// A mixed batch is n proofs in the CALLER's order, proof i of plan plan_of[i]; instances and committed instances are
// concatenated in that order, so their offsets depend on the plans of all proofs before.  The device pipeline wants the proofs
// of one plan side by side.  partition() builds, from plan_of and the plans' shapes alone:
//   count / base      per plan: its number of proofs, and the grouped index of its first one (plans in list order)
//   perm              grouped index g -> position in the caller's order.  STABLE: within a plan the caller's order is kept.
//                     It is also "every proof's position in the caller's order": what k_mixed_pairs writes its pair to.
//   inst_src / _dst   byte offset of proof perm[g]'s public inputs in the caller's `instances` / in the grouped staging,
//                     where plan k's block starts at inst_base[k] and is count[k] x 32 n_pi(k) bytes
//   inst_len          32 n_pi of the proof's plan
//   ci_src / ci_dst   index of the proof's 48-byte committed instance among the caller's / in the grouped staging (plan k's
//                     block starts at record ci_base[k]); H2V_MIXED_NONE for a plan without one
// group_offsets() then gives the grouped proof offsets - ONE array of n + 1 entries, plan k's proof_off array being the
// count[k] + 1 entries from base[k] on (neighbouring plans share the boundary entry) - from the caller's proof_off, with the
// rule the coalescing kernels use (h2v_coalesce.hpp): a proof keeps its length when it is shorter than its plan's proof_len
// (the kernels reject it by that alone) and is cut to proof_len otherwise (trailing bytes are never read), so the grouped bytes
// fit sum_k count[k] x proof_len(k).  The device form cannot read the caller's proof_off on the host: there k_mixed_offsets
// computes the same array (h2v_mixed_dev.hpp).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#define H2V_MIXED_NONE 0xffffffffu

namespace h2vmixed {

struct PlanShape { uint32_t proof_len, n_pi, n_ci; };

struct Partition {
    uint32_t n = 0, n_plans = 0;
    std::vector<uint32_t> count, base;            // n_plans
    std::vector<uint64_t> inst_base;              // n_plans (bytes)
    std::vector<uint32_t> ci_base;                // n_plans (48-byte records)
    std::vector<uint32_t> perm, len_cap, inst_len, ci_src, ci_dst;   // n, indexed by grouped position
    std::vector<uint64_t> inst_src, inst_dst;     // n
    uint64_t inst_total = 0, proof_cap = 0;       // bytes of all public inputs; sum of count x proof_len
    uint32_t ci_total = 0;                        // committed instances in the call
};

// false: plan_of[i] >= n_plans for some i (err names it).  n = 0 and plans without a proof are fine.
inline bool partition(const PlanShape *shapes, uint32_t n_plans, const uint32_t *plan_of, uint64_t n, Partition &out, std::string *err) {
    out = Partition();
    if (n > 0xffffffffull) { if (err) *err = "more than 2^32 proofs"; return false; }
    out.n = (uint32_t)n; out.n_plans = n_plans;
    out.count.assign(n_plans, 0); out.base.assign(n_plans, 0); out.inst_base.assign(n_plans, 0); out.ci_base.assign(n_plans, 0);
    for (uint64_t i = 0; i < n; i++) {
        if (plan_of[i] >= n_plans) {
            if (err) *err = "plan_of[" + std::to_string(i) + "] = " + std::to_string(plan_of[i]) + " is out of range: " + std::to_string(n_plans) + " plans listed";
            return false;
        }
        out.count[plan_of[i]]++;
    }
    uint32_t run = 0, ci_run = 0;
    uint64_t inst_run = 0;
    for (uint32_t k = 0; k < n_plans; k++) {
        out.base[k] = run; out.inst_base[k] = inst_run; out.ci_base[k] = ci_run;
        run += out.count[k];
        inst_run += (uint64_t)out.count[k] * shapes[k].n_pi * 32;
        if (shapes[k].n_ci) ci_run += out.count[k];
        out.proof_cap += (uint64_t)out.count[k] * shapes[k].proof_len;
    }
    out.inst_total = inst_run; out.ci_total = ci_run;
    out.perm.assign(out.n, 0); out.len_cap.assign(out.n, 0); out.inst_len.assign(out.n, 0);
    out.ci_src.assign(out.n, H2V_MIXED_NONE); out.ci_dst.assign(out.n, H2V_MIXED_NONE);
    out.inst_src.assign(out.n, 0); out.inst_dst.assign(out.n, 0);
    std::vector<uint32_t> fill(n_plans, 0);
    uint64_t src_inst = 0;
    uint32_t src_ci = 0;
    for (uint32_t i = 0; i < out.n; i++) {               // the caller's order: a plan's proofs keep it (stable)
        const uint32_t k = plan_of[i], j = fill[k]++, g = out.base[k] + j;
        const PlanShape &s = shapes[k];
        out.perm[g] = i;
        out.len_cap[g] = s.proof_len;
        out.inst_len[g] = s.n_pi * 32;
        out.inst_src[g] = src_inst;
        out.inst_dst[g] = out.inst_base[k] + (uint64_t)j * s.n_pi * 32;
        src_inst += (uint64_t)s.n_pi * 32;
        if (s.n_ci) { out.ci_src[g] = src_ci++; out.ci_dst[g] = out.ci_base[k] + j; }
    }
    return true;
}

// grouped[0 .. n]: the grouped proof offsets from the caller's proof_off (n + 1 entries, non-decreasing)
inline void group_offsets(const Partition &p, const uint64_t *proof_off, uint64_t *grouped) {
    uint64_t run = 0;
    grouped[0] = 0;
    for (uint32_t g = 0; g < p.n; g++) {
        const uint64_t len = proof_off[p.perm[g] + 1] - proof_off[p.perm[g]];
        run += len < p.len_cap[g] ? len : p.len_cap[g];
        grouped[g + 1] = run;
    }
}

}   // namespace h2vmixed
