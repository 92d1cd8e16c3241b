// Stand-alone test of the SRS classes of a mixed call across several SRS (csrc/h2v_mixed_srs.hpp: host code only), built with
// ASan + UBSan by tests/test_mixed_across_srs.py.  Every expectation is restated here from the rule - classes numbered in the
// order in which a listed plan first carries them, classes without a proof dropped, P(i) = the proofs in lower classes + the rank
// of i within its class in the caller's order - by a quadratic count that shares nothing with the header's one pass.
// prints "ok <checks>" (exit 0) or the first failed check (exit 1).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed_srs.hpp"

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

using h2vsrs::Classes;
using h2vsrs::Digest;

// srs_of_plan: an SRS label per listed plan; plan_of: the call.  Returns classes()'s verdict.
static bool run(const std::vector<uint32_t> &srs_of_plan, const std::vector<uint32_t> &plan_of, uint32_t max_used, Classes &cl, bool *limit, std::string *err) {
    const uint32_t n_plans = (uint32_t)srs_of_plan.size();
    std::vector<h2vmixed::PlanShape> shapes(n_plans, h2vmixed::PlanShape{100, 1, 0});
    h2vmixed::Partition pt;
    std::string perr;
    CHECK(h2vmixed::partition(shapes.data(), n_plans, plan_of.data(), plan_of.size(), pt, &perr));
    std::vector<Digest> dg(n_plans);
    for (uint32_t k = 0; k < n_plans; k++) dg[k] = Digest{{0x1000ull + srs_of_plan[k], ~(uint64_t)srs_of_plan[k]}};
    return h2vsrs::classes(dg.data(), pt, plan_of.data(), max_used, cl, limit, err);
}
// the rule, restated
static void hold(const std::vector<uint32_t> &srs_of_plan, const std::vector<uint32_t> &plan_of, const Classes &cl) {
    const uint32_t n = (uint32_t)plan_of.size(), n_plans = (uint32_t)srs_of_plan.size();
    // classes in first-carry order over the LISTED plans
    std::vector<uint32_t> labels;
    for (uint32_t k = 0; k < n_plans; k++) {
        bool seen = false;
        for (uint32_t l : labels) seen = seen || l == srs_of_plan[k];
        if (!seen) labels.push_back(srs_of_plan[k]);
    }
    CHECK(cl.n_classes == labels.size() && cl.class_of_plan.size() == n_plans && cl.n == n);
    for (uint32_t k = 0; k < n_plans; k++) CHECK(labels[cl.class_of_plan[k]] == srs_of_plan[k]);
    // the classes with proofs, in that order
    uint32_t used = 0, run = 0;
    for (uint32_t c = 0; c < labels.size(); c++) {
        uint32_t cnt = 0, rep = H2V_SRS_NONE;
        for (uint32_t i = 0; i < n; i++)
            if (srs_of_plan[plan_of[i]] == labels[c]) cnt++;
        for (uint32_t k = n_plans; k-- > 0;) {
            bool has = false;
            for (uint32_t i = 0; i < n; i++) has = has || plan_of[i] == k;
            if (has && srs_of_plan[k] == labels[c]) rep = k;
        }
        if (!cnt) { CHECK(cl.used_of_class[c] == H2V_SRS_NONE); continue; }
        CHECK(cl.used_of_class[c] == used);
        CHECK(cl.count[used] == cnt && cl.base[used] == run && cl.rep_plan[used] == rep);
        CHECK(srs_of_plan[cl.rep_plan[used]] == labels[c]);
        used++; run += cnt;
    }
    CHECK(cl.n_used == used && run == n && cl.count.size() == used && cl.base.size() == used && cl.rep_plan.size() == used);
    // P: proofs in lower classes + rank within the class; a permutation; pos its inverse; stable within a class
    CHECK(cl.P.size() == n && cl.pos.size() == n);
    std::vector<uint8_t> hit(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t ci = cl.class_of_plan[plan_of[i]];
        uint32_t lower = 0, rank = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t cj = cl.class_of_plan[plan_of[j]];
            if (cj < ci) lower++;
            if (cj == ci && j < i) rank++;
        }
        CHECK(cl.P[i] == lower + rank);
        CHECK(cl.P[i] < n && !hit[cl.P[i]]);
        hit[cl.P[i]] = 1;
        CHECK(cl.pos[cl.P[i]] == i);
        const uint32_t u = cl.used_of_class[ci];
        CHECK(cl.P[i] >= cl.base[u] && cl.P[i] < cl.base[u] + cl.count[u]);
    }
    for (uint32_t u = 0; u < cl.n_used; u++)
        for (uint32_t q = cl.base[u] + 1; q < cl.base[u] + cl.count[u]; q++) CHECK(cl.pos[q - 1] < cl.pos[q]);
}
static void accept(const std::vector<uint32_t> &srs_of_plan, const std::vector<uint32_t> &plan_of, uint32_t want_used) {
    Classes cl;
    bool limit = true;
    std::string err;
    CHECK(run(srs_of_plan, plan_of, 16, cl, &limit, &err));
    CHECK(!limit && err.empty() && cl.n_used == want_used);
    hold(srs_of_plan, plan_of, cl);
}

int main() {
    // interleaved: three SRS, five plans, plans 1 and 3 repeat SRS 7
    accept({7, 9, 7, 8, 9}, {4, 0, 3, 1, 2, 0, 4, 4, 1, 3, 2, 0}, 3);
    // one class: P is the identity
    {
        Classes cl;
        bool limit;
        std::string err;
        const std::vector<uint32_t> srs{5, 5, 5}, po{2, 0, 1, 1, 0, 2, 2};
        CHECK(run(srs, po, 16, cl, &limit, &err));
        CHECK(cl.n_classes == 1 && cl.n_used == 1 && cl.count[0] == po.size() && cl.base[0] == 0 && cl.rep_plan[0] == 0);
        for (uint32_t i = 0; i < po.size(); i++) CHECK(cl.P[i] == i && cl.pos[i] == i);
        hold(srs, po, cl);
    }
    // a class without proofs: in the middle (SRS 2: plan 1), at the front (SRS 1: plan 0) and at the end
    accept({1, 2, 3}, {0, 2, 2, 0}, 2);
    accept({1, 2, 3}, {1, 2, 2, 1, 1}, 2);
    accept({1, 2, 3}, {1, 0, 0}, 2);
    // ... and a class whose FIRST listed plan has no proof: the representative is the first plan of the class WITH one
    {
        Classes cl;
        bool limit;
        std::string err;
        const std::vector<uint32_t> srs{4, 6, 4, 6}, po{3, 2, 3};
        CHECK(run(srs, po, 16, cl, &limit, &err));
        CHECK(cl.n_used == 2 && cl.rep_plan[0] == 2 && cl.rep_plan[1] == 3 && cl.count[0] == 1 && cl.count[1] == 2);
        CHECK(cl.P[0] == 1 && cl.P[1] == 0 && cl.P[2] == 2);
        hold(srs, po, cl);
    }
    // listed plans repeating an SRS, every plan with proofs
    accept({3, 3, 4, 4, 3}, {0, 1, 2, 3, 4, 4, 3, 2, 1, 0}, 2);
    // an empty call, and plans without any proof
    accept({1, 2}, {}, 0);
    // 16 classes with proofs pass; a 17th listed WITHOUT a proof passes; a 17th WITH a proof is the limit
    {
        std::vector<uint32_t> srs, po;
        for (uint32_t k = 0; k < 17; k++) srs.push_back(100 + k);
        for (uint32_t k = 0; k < 16; k++) po.push_back(15 - k);
        accept(std::vector<uint32_t>(srs.begin(), srs.begin() + 16), po, 16);
        accept(srs, po, 16);
        po.push_back(16);
        Classes cl;
        bool limit = false;
        std::string err;
        CHECK(!run(srs, po, 16, cl, &limit, &err));
        CHECK(limit && err.find("17") != std::string::npos && err.find("16") != std::string::npos);
        // (the limit is the caller's number: the same call under a limit of 17 passes)
        CHECK(run(srs, po, 17, cl, &limit, &err) && !limit && cl.n_used == 17);
        hold(srs, po, cl);
    }
    // a larger seeded layout: 9 plans on 4 SRS, 300 proofs
    {
        std::vector<uint32_t> srs{0, 1, 2, 3, 0, 1, 2, 0, 0}, po;
        uint32_t x = 12345;
        for (int i = 0; i < 300; i++) { x = x * 1664525u + 1013904223u; po.push_back((x >> 16) % 9); }
        accept(srs, po, 4);
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
