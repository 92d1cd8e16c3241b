// Stand-alone test of the group tables of H2V_MIXED_GROUPED (csrc/h2v_mixed_group.hpp).  Host code only: built with
// -fsanitize=address,undefined and run as a program (tests/test_mixed_grouped.py).  Every check compares with a brute-force
// enumeration: walk every block (unit) of every prefix array of every range, mark what it covers in a plain array and look for a
// cell marked twice or never; restate where a grouped position lies in the staging proof by proof.
// Prints "ok <checks>" and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed_group.hpp"

using namespace h2vmixed;

static long checks = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        checks++;                                                                           \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Key { uint32_t proof_len, n_pi, n_ci, n_points, ivc, n_terms, n_var, n_fix, n_regs, P, kind; bool foldable; };
// shapes in the spirit of simple_mul, lookup_table, trashcan_mix (a committed instance), ivc (recursive: not foldable), a key
// whose register file does not fit LDS (P = 0), and a blake2b-512 flavoured key; the figures only have to differ from key to key
static const Key KEYS[6] = {
    {1000, 3, 0, 10, 0, 16, 10, 6, 70, 32, 0, true},  {1500, 1, 0, 19, 0, 30, 19, 11, 150, 16, 0, true}, {1300, 5, 1, 16, 0, 30, 17, 13, 40, 64, 0, true},
    {4000, 28, 0, 30, 1, 33, 33, 0, 200, 8, 0, false}, {2000, 2, 0, 23, 0, 35, 23, 12, 900, 0, 0, true},  {1000, 3, 0, 10, 0, 16, 10, 6, 70, 32, 1, true}};

static GroupShape shape_of(const Key &k) {
    GroupShape s = {};
    s.d.proof_len = k.proof_len; s.d.n_pi = k.n_pi; s.d.n_ci = k.n_ci; s.d.n_points = k.n_points; s.d.ivc = k.ivc; s.d.n_terms = k.n_terms;
    s.d.n_regs = k.n_regs; s.d.vm_lanes = 1; s.d.tr_kind = k.kind;
    s.n_var = k.n_var; s.n_fix = k.n_fix; s.P = k.P; s.foldable = k.foldable;
    return s;
}

static void verify(const std::vector<Key> &keys, const std::vector<uint32_t> &plan_of, uint32_t chunk) {
    const uint32_t K = (uint32_t)keys.size(), n = (uint32_t)plan_of.size();
    std::vector<PlanShape> ps(K);
    std::vector<GroupShape> gs(K);
    std::vector<FoldShape> fs(K);
    for (uint32_t k = 0; k < K; k++) { ps[k] = {keys[k].proof_len, keys[k].n_pi, keys[k].n_ci}; gs[k] = shape_of(keys[k]); fs[k] = {keys[k].n_var, keys[k].n_fix, keys[k].foldable}; }
    Partition pt;
    std::string err;
    CHECK(partition(ps.data(), K, plan_of.data(), n, pt, &err));
    FoldLayout lay, plain;
    CHECK(fold_layout(fs.data(), pt.count.data(), K, chunk, lay, &err));
    plain = lay;
    GroupSpace sp;
    group_space(gs.data(), pt.count.data(), K, chunk, sp);
    group_fold_blocks(sp, gs.data(), pt.count.data(), lay);
    // ---- the space: which plans, where, the union strides
    uint32_t G = 0, other = 0, ut = 0, us = 0;
    for (uint32_t k = 0; k < K; k++) {
        const bool want = pt.count[k] && keys[k].foldable && keys[k].P;
        CHECK((sp.groupable[k] != 0) == want);
        if (want) {
            CHECK(sp.gbase[k] == G);
            G += pt.count[k];
            if (keys[k].n_terms > ut) ut = keys[k].n_terms;
            const uint32_t slots = keys[k].n_points + keys[k].n_ci + 2 * keys[k].ivc;
            if (slots > us) us = slots;
        } else if (pt.count[k]) other++;
    }
    CHECK(sp.total == G && sp.n_other == other && sp.u_terms == ut && sp.u_slots == us);
    // (nothing but the block sums of the groupable plans moves in the fold layout)
    CHECK(lay.n_r == plain.n_r && lay.term_base == plain.term_base && lay.vk_base == plain.vk_base && lay.pair_base == plain.pair_base && lay.fix_base == plain.fix_base);
    // ---- brute force: grouped position -> (plan, proof within the plan)
    std::vector<uint32_t> plan_at(G), j_at(G);
    for (uint32_t k = 0, g = 0; k < K; k++)
        if (sp.groupable[k]) for (uint32_t j = 0; j < pt.count[k]; j++, g++) { plan_at[g] = k; j_at[g] = j; }
    std::vector<uint8_t> term((size_t)lay.n_r, 0), part((size_t)lay.n_parts, 0);
    auto own = [&](std::vector<uint8_t> &v, uint64_t at) { CHECK(at < v.size()); CHECK(v[(size_t)at] == 0); v[(size_t)at] = 1; checks -= 2; };
    const uint32_t nr = group_ranges(sp);
    CHECK(nr == (G == 0 ? 0u : chunk == 0 ? 1u : (G + chunk - 1) / chunk));
    uint32_t covered = 0;
    for (uint32_t c = 0; c < nr; c++) {
        uint32_t g0, g1;
        group_range(sp, c, g0, g1);
        CHECK(g0 == covered && g1 > g0 && g1 <= G && (chunk == 0 || g1 - g0 <= chunk) && (chunk == 0 || g0 % chunk == 0));
        covered = g1;
        GroupTables t;
        CHECK(group_tables(sp, gs.data(), pt, lay, g0, g1, lay.n_r, lay.n_parts, t, &err));
        const uint32_t ng = (uint32_t)t.rec.size(), m = g1 - g0;
        CHECK(t.n == m && ng >= 1);
        for (const auto *v : {&t.comb[0], &t.comb[1], &t.dec, &t.terms}) {
            CHECK(v->size() == ng + 1 && (*v)[0] == 0);
            for (uint32_t g = 0; g < ng; g++) CHECK((*v)[g] <= (*v)[g + 1]);
        }
        // the records against the restatement; workspace regions disjoint and inside m proofs of the union strides
        std::vector<uint8_t> scal((size_t)m * ut, 0), slot((size_t)m * us, 0);
        uint32_t next = 0;
        for (uint32_t g = 0; g < ng; g++) {
            const H2vGroupRec &r = t.rec[g];
            CHECK(r.first == next && r.count >= 1);                 // groups tile the range in plan order
            next += r.count;
            const uint32_t k = plan_at[g0 + r.first], j0 = j_at[g0 + r.first];
            const Key &key = keys[k];
            CHECK(r.plan_index == k && r.P == key.P && r.n_var == key.n_var && r.n_fix == key.n_fix && r.slots == key.n_points + key.n_ci + 2 * key.ivc);
            CHECK(r.plan.n_terms == key.n_terms && r.plan.proof_len == key.proof_len && r.plan.tr_kind == key.kind);
            for (uint32_t i = 0; i < r.count; i++) CHECK(plan_at[g0 + r.first + i] == k && j_at[g0 + r.first + i] == j0 + i);   // one plan, consecutive
            CHECK(g + 1 == ng || plan_at[g0 + r.first + r.count] != k);     // ... and all the range has of it
            CHECK(r.off_idx == (uint64_t)pt.base[k] + j0);
            CHECK(r.inst_off == pt.inst_dst[pt.base[k] + j0]);
            if (key.n_ci) CHECK(r.ci_idx == pt.ci_dst[pt.base[k] + j0]);
            CHECK(r.term_base == (uint64_t)lay.term_base[k] + (uint64_t)j0 * key.n_var);
            CHECK(r.scal_base == (uint64_t)r.first * ut * 8 && r.pts_base == (uint64_t)r.first * us);
            for (uint32_t i = 0; i < r.count; i++) {
                for (uint32_t q = 0; q < key.n_terms; q++) own(scal, r.scal_base / 8 + (uint64_t)i * key.n_terms + q);
                for (uint32_t q = 0; q < r.slots; q++) own(slot, r.pts_base + (uint64_t)i * r.slots + q);
                for (uint32_t q = 0; q < key.n_var; q++) own(term, r.term_base + (uint64_t)i * key.n_var + q);
            }
            for (uint32_t b = 0; b < (r.count + 63) / 64; b++)
                for (uint32_t f = 0; f < key.n_fix; f++) {
                    const uint64_t at = r.part_base + (uint64_t)b * key.n_fix + f;
                    CHECK(at >= lay.part_base[k] && at < lay.part_base[k] + (uint64_t)lay.n_blocks[k] * key.n_fix);   // inside what k_mixed_vk_sum adds for plan k
                    own(part, at);
                }
            CHECK(t.lds[key.kind] >= key.n_regs * 32 * key.P);
        }
        CHECK(next == m);
        // every position in exactly one block of exactly one group: combiner (both kinds together), terms; every point in one unit
        std::vector<uint8_t> hit(m, 0);
        for (int kind = 0; kind < 2; kind++)
            for (uint32_t b = 0; b < t.comb[kind].back(); b++) {
                const uint32_t g = h2v_group_find(t.comb[kind].data(), ng, b), bb = b - t.comb[kind][g];
                CHECK(g < ng && t.comb[kind][g] <= b && b < t.comb[kind][g + 1]);
                const H2vGroupRec &r = t.rec[g];
                CHECK(r.plan.tr_kind == (uint32_t)kind && bb * r.P < r.count);
                for (uint32_t q = 0; q < r.P && bb * r.P + q < r.count; q++) own(hit, r.first + bb * r.P + q);
            }
        for (uint32_t i = 0; i < m; i++) CHECK(hit[i] == 1);
        hit.assign(m, 0);
        for (uint32_t b = 0; b < t.terms.back(); b++) {
            const uint32_t g = h2v_group_find(t.terms.data(), ng, b), bb = b - t.terms[g];
            CHECK(g < ng && t.terms[g] <= b && b < t.terms[g + 1] && bb * 64 < t.rec[g].count);
            for (uint32_t q = 0; q < 64 && bb * 64 + q < t.rec[g].count; q++) own(hit, t.rec[g].first + bb * 64 + q);
        }
        for (uint32_t i = 0; i < m; i++) CHECK(hit[i] == 1);
        std::vector<uint8_t> pts((size_t)m * us, 0);
        for (uint32_t u = 0; u < t.dec.back(); u++) {
            const uint32_t g = h2v_group_find(t.dec.data(), ng, u), uu = u - t.dec[g];
            CHECK(g < ng && t.dec[g] <= u && u < t.dec[g + 1]);
            const H2vGroupRec &r = t.rec[g];
            CHECK((uint64_t)uu * 64 < (uint64_t)r.count * r.slots);      // a unit lies inside ONE group: its points are that group's
            for (uint32_t q = 0; q < 64 && (uint64_t)uu * 64 + q < (uint64_t)r.count * r.slots; q++) own(pts, r.pts_base + (uint64_t)uu * 64 + q);
        }
        for (size_t i = 0; i < pts.size(); i++) CHECK(pts[i] == slot[i]);   // exactly the slots the groups own
    }
    CHECK(covered == G);
    // the terms of the groupable plans and every block sum of theirs are owned exactly once; what is left belongs to the others
    for (uint32_t k = 0; k < K; k++) {
        if (!lay.foldable[k]) continue;
        for (uint64_t e = 0; e < (uint64_t)pt.count[k] * keys[k].n_var; e++) CHECK(term[(size_t)(lay.term_base[k] + e)] == (sp.groupable[k] ? 1 : 0));
        for (uint64_t e = 0; e < (uint64_t)lay.n_blocks[k] * keys[k].n_fix; e++) CHECK(part[(size_t)(lay.part_base[k] + e)] == (sp.groupable[k] ? 1 : 0));
        if (!sp.groupable[k]) CHECK(lay.n_blocks[k] == fold_blocks(pt.count[k], chunk));
    }
    uint64_t parts = 0;
    for (uint32_t k = 0; k < K; k++) { CHECK(!lay.foldable[k] || lay.part_base[k] == parts); parts += (uint64_t)lay.n_blocks[k] * keys[k].n_fix; }
    CHECK(parts == lay.n_parts);
    // ranges that are whole plans: one piece, or every groupable plan a multiple of the chunk - fold_layout's ownership
    bool whole = true;
    for (uint32_t k = 0; k < K; k++) if (sp.groupable[k] && chunk && pt.count[k] % chunk) whole = false;
    if (whole) CHECK(lay.n_blocks == plain.n_blocks && lay.block_base == plain.block_base && lay.part_base == plain.part_base && lay.n_parts == plain.n_parts && lay.total_blocks == plain.total_blocks);
}

static std::vector<uint32_t> shuffled(const std::vector<uint32_t> &count, uint32_t seed) {
    std::vector<uint32_t> v;
    for (uint32_t k = 0; k < count.size(); k++) v.insert(v.end(), count[k], k);
    uint64_t s = seed * 2654435761u + 1;
    for (size_t i = v.size(); i > 1; i--) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(v[i - 1], v[(size_t)((s >> 33) % i)]);
    }
    return v;
}

int main() {
    // group_find on tables with empty groups at the head, in the middle and at the end
    {
        const uint32_t p[] = {0, 0, 3, 3, 3, 4, 9, 9};
        const uint32_t want[] = {1, 1, 1, 4, 5, 5, 5, 5, 5};
        for (uint32_t b = 0; b < 9; b++) CHECK(h2v_group_find(p, 7, b) == want[b]);
        const uint32_t one[] = {0, 5};
        for (uint32_t b = 0; b < 5; b++) CHECK(h2v_group_find(one, 1, b) == 0);
    }
    const std::vector<Key> all(KEYS, KEYS + 6);
    // the GPU tests' counts (70 / 65 / 9 / ivc 1), a listed key without a proof, the blake2b-512 key; chunk 40 puts borders inside
    // the first two plans and lets a range span three plans; 1 = one proof of one plan per range
    for (uint32_t chunk : {0u, 1u, 7u, 40u, 64u, 65u, 100u, 4096u})
        for (uint32_t seed = 0; seed < 3; seed++) {
            verify(all, shuffled({70, 65, 9, 1, 0, 5}, seed), chunk);
            verify(all, shuffled({70, 65, 9, 1, 3, 0}, seed), chunk);
            verify(all, shuffled({0, 65, 0, 0, 0, 2}, seed), chunk);          // plans without proofs between two with proofs
            verify(all, shuffled({1, 0, 0, 0, 0, 0}, seed), chunk);          // n = 1
            verify(all, shuffled({0, 0, 0, 4, 2, 0}, seed), chunk);          // nothing groupable: no range at all
            verify(all, shuffled({0, 0, 0, 0, 0, 130}, seed), chunk);        // only the second transcript kind
            verify(all, shuffled({128, 64, 192, 0, 0, 64}, seed), chunk);    // multiples of 64: whole-plan ranges at chunk 64
        }
    // H2V_MIXED_GROUPED_MAX_PLANS keys of one proof each (every sixth one not groupable), in one piece and in small ranges
    {
        std::vector<Key> many;
        std::vector<uint32_t> count;
        for (uint32_t k = 0; k < 1024; k++) { many.push_back(KEYS[k % 6]); many.back().n_pi = 1 + k % 4; count.push_back(1); }
        for (uint32_t chunk : {0u, 1u, 3u, 40u, 512u}) verify(many, shuffled(count, chunk), chunk);
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
