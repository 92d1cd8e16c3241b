// Mixed-key calls across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS): the host side of the SRS classes.  HOST CODE ONLY - no
// HIP call and no HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_mixed_srs.cpp).
//
// The listed plans of a call are classed by the digest of their s_g2 line tables.  Classes are numbered in the order in which a
// listed plan first carries them; a class WITHOUT a proof is dropped - no bucket problem, no Miller loop, nothing against the
// limit - and the classes WITH proofs keep their relative order as the call's "used" classes 0 .. n_used - 1.  classes() builds,
// from the digests, plan_of and the partition's per-plan counts alone:
//   class_of_plan     per listed plan: its class among ALL classes of the list (first-carry order)
//   used_of_class     per class: its number among the classes with proofs, or H2V_SRS_NONE
//   rep_plan          per used class: the first listed plan of the class that has a proof (its line table serves the class)
//   count / base      per used class: its proofs, and the class-major slot of its first one
//   P                 call position i -> class-major slot: the proofs of lower classes + the rank of i within its class in the
//                     caller's order.  A permutation of 0 .. n - 1, stable within a class; ONE class gives P(i) = i
//   pos               its inverse: slot q -> call position.  Class k's slice is pos[base[k] .. base[k] + count[k])
// More than max_used classes with proofs: false, *limit set (H2V_E_LIMIT).
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "h2v_mixed.hpp"

#define H2V_SRS_NONE 0xffffffffu

namespace h2vsrs {

struct Digest { uint64_t w[2]; };

struct Classes {
    uint32_t n = 0, n_classes = 0, n_used = 0;
    std::vector<uint32_t> class_of_plan;          // n_plans
    std::vector<uint32_t> used_of_class;          // n_classes
    std::vector<uint32_t> rep_plan, count, base;  // n_used
    std::vector<uint32_t> P, pos;                 // n
};

inline bool classes(const Digest *digests, const h2vmixed::Partition &pt, const uint32_t *plan_of, uint32_t max_used, Classes &out, bool *limit, std::string *err) {
    out = Classes();
    if (limit) *limit = false;
    const uint32_t n_plans = pt.n_plans;
    out.n = pt.n;
    out.class_of_plan.assign(n_plans, 0);
    std::vector<uint32_t> first_plan;             // per class: the listed plan that first carries it
    for (uint32_t k = 0; k < n_plans; k++) {
        uint32_t c = 0;
        while (c < first_plan.size() && memcmp(&digests[first_plan[c]], &digests[k], sizeof(Digest))) c++;
        if (c == first_plan.size()) first_plan.push_back(k);
        out.class_of_plan[k] = c;
    }
    out.n_classes = (uint32_t)first_plan.size();
    std::vector<uint32_t> proofs(out.n_classes, 0), rep(out.n_classes, H2V_SRS_NONE);
    for (uint32_t k = 0; k < n_plans; k++) {
        const uint32_t c = out.class_of_plan[k];
        if (pt.count[k] && rep[c] == H2V_SRS_NONE) rep[c] = k;
        proofs[c] += pt.count[k];
    }
    out.used_of_class.assign(out.n_classes, H2V_SRS_NONE);
    uint32_t run = 0;
    for (uint32_t c = 0; c < out.n_classes; c++) {
        if (!proofs[c]) continue;
        out.used_of_class[c] = out.n_used++;
        out.rep_plan.push_back(rep[c]); out.count.push_back(proofs[c]); out.base.push_back(run);
        run += proofs[c];
    }
    if (out.n_used > max_used) {
        if (limit) *limit = true;
        if (err) *err = "at most " + std::to_string(max_used) + " SRS may have proofs in one H2V_MIXED_ACROSS_SRS call, this one has " + std::to_string(out.n_used);
        return false;
    }
    out.P.assign(out.n, 0); out.pos.assign(out.n, 0);
    std::vector<uint32_t> fill(out.n_used, 0);
    for (uint32_t i = 0; i < out.n; i++) {        // the caller's order: a class's proofs keep it (stable)
        const uint32_t u = out.used_of_class[out.class_of_plan[plan_of[i]]];
        const uint32_t q = out.base[u] + fill[u]++;
        out.P[i] = q; out.pos[q] = i;
    }
    return true;
}

}   // namespace h2vsrs
