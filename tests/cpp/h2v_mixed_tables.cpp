// Stand-alone test of the table block of the mixed-key calls (csrc/h2v_mixed_tables.hpp).  Host code only: built with
// -fsanitize=address,undefined and run as a program (tests/test_mixed_tables.py).
//   1. prints the layout over a grid, one line per point, in the format of tests/golden/mixed_table_layout.txt (which the
//      hand-written offsets of the code before this header produced); the Python test compares line for line
//   2. at every grid point: the regions are disjoint, 16-byte aligned, inside the extent, and in the order the line names
//   3. packs real Partitions (with and without host offsets) and real GroupTables into a vector of EXACTLY `extent` bytes - one
//      byte too many is ASan's to see - and reads every array back
// Prints "ok <checks>" last and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed_tables.hpp"

using namespace h2vmixed;
using mixedtab::Region;
using mixedtab::TableBlock;

static long checks = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        checks++;                                                                           \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

static std::vector<Region> regions_of(const TableBlock &B) {
    std::vector<Region> v = {B.offsets, B.inst_src, B.inst_dst, B.perm, B.len_cap, B.inst_len, B.ci_src, B.ci_dst, B.fold};
    for (const auto &r : B.range) for (const Region &g : {r.recs, r.comb[0], r.comb[1], r.dec, r.terms}) v.push_back(g);
    return v;
}
static void grid_point(size_t n, size_t fold_bytes, const std::vector<uint32_t> &groups) {
    const TableBlock B = mixedtab::table_block(n, fold_bytes, groups.data(), groups.size());
    std::printf("n=%zu fold_bytes=%zu groups=", n, fold_bytes);
    for (size_t c = 0; c < groups.size(); c++) std::printf("%s%u", c ? "," : "", groups[c]);
    if (groups.empty()) std::printf("-");
    std::printf(" | offsets=%zu inst_src=%zu inst_dst=%zu perm=%zu len_cap=%zu inst_len=%zu ci_src=%zu ci_dst=%zu fold=%zu", B.offsets.off, B.inst_src.off,
                B.inst_dst.off, B.perm.off, B.len_cap.off, B.inst_len.off, B.ci_src.off, B.ci_dst.off, B.fold.off);
    for (size_t c = 0; c < B.range.size(); c++)
        std::printf(" | r%zu: recs=%zu comb0=%zu comb1=%zu dec=%zu terms=%zu", c, B.range[c].recs.off, B.range[c].comb[0].off, B.range[c].comb[1].off,
                    B.range[c].dec.off, B.range[c].terms.off);
    std::printf(" | extent=%zu\n", B.extent);
    // the regions in order: aligned, each behind the end of the one before (so: pairwise disjoint), the last inside the extent
    CHECK(B.range.size() == groups.size());
    CHECK(B.offsets.bytes == (n + 1) * 8 && B.inst_src.bytes == n * 8 && B.inst_dst.bytes == n * 8 && B.fold.bytes == fold_bytes);
    for (const Region *g : {&B.perm, &B.len_cap, &B.inst_len, &B.ci_src, &B.ci_dst}) CHECK(g->bytes == n * 4);
    for (size_t c = 0; c < groups.size(); c++) {
        CHECK(B.range[c].recs.bytes == (size_t)groups[c] * sizeof(H2vGroupRec));
        for (const Region *g : {&B.range[c].comb[0], &B.range[c].comb[1], &B.range[c].dec, &B.range[c].terms}) CHECK(g->bytes == ((size_t)groups[c] + 1) * 4);
    }
    size_t end = 0;
    for (const Region &g : regions_of(B)) {
        CHECK(g.off % 16 == 0);
        CHECK(g.off >= end);
        end = g.off + g.bytes;
        CHECK(end <= B.extent);
    }
}

struct Key { uint32_t proof_len, n_pi, n_ci, n_points, ivc, n_terms, n_var, n_fix, n_regs, P, kind; bool foldable; };
// the shapes of tests/cpp/h2v_mixed_group.cpp
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
template <class T> static bool same(const uint8_t *block, const Region &g, const std::vector<T> &src) {
    return g.bytes == src.size() * sizeof(T) && (g.bytes == 0 || memcmp(block + g.off, src.data(), g.bytes) == 0);
}
// one call's block: packed into exactly `extent` bytes, every array read back.  grouped: the ranges of group_tables at `chunk`
static void pack_case(const std::vector<Key> &keys, const std::vector<uint32_t> &plan_of, bool with_off, bool grouped, uint32_t chunk, size_t fold_bytes) {
    const uint32_t K = (uint32_t)keys.size(), n = (uint32_t)plan_of.size();
    std::vector<PlanShape> ps(K);
    std::vector<GroupShape> gs(K);
    std::vector<FoldShape> fs(K);
    for (uint32_t k = 0; k < K; k++) { ps[k] = {keys[k].proof_len, keys[k].n_pi, keys[k].n_ci}; gs[k] = shape_of(keys[k]); fs[k] = {keys[k].n_var, keys[k].n_fix, keys[k].foldable}; }
    Partition pt;
    std::string err;
    CHECK(partition(ps.data(), K, plan_of.data(), n, pt, &err));
    std::vector<GroupTables> gt;
    if (grouped) {
        FoldLayout lay;
        CHECK(fold_layout(fs.data(), pt.count.data(), K, chunk, lay, &err));
        GroupSpace sp;
        group_space(gs.data(), pt.count.data(), K, chunk, sp);
        group_fold_blocks(sp, gs.data(), pt.count.data(), lay);
        gt.resize(group_ranges(sp));
        for (uint32_t c = 0; c < gt.size(); c++) {
            uint32_t g0, g1;
            group_range(sp, c, g0, g1);
            CHECK(group_tables(sp, gs.data(), pt, lay, g0, g1, lay.n_r, lay.n_parts, gt[c], &err));
        }
    }
    std::vector<uint32_t> ng(gt.size());
    for (size_t c = 0; c < gt.size(); c++) ng[c] = (uint32_t)gt[c].rec.size();
    const TableBlock B = mixedtab::table_block(n, fold_bytes, ng.data(), ng.size());
    std::vector<uint64_t> off(n + 1);
    for (uint32_t i = 0; i <= n; i++) off[i] = 1000ull * i + 7;
    std::vector<uint8_t> block(B.extent, 0xa5);              // EXACTLY the extent
    std::vector<mixedtab::RangeInfo> info;
    mixedtab::pack_tables(block.data(), B, pt, with_off ? off.data() : nullptr, gt, info);
    if (with_off) CHECK(same(block.data(), B.offsets, off));
    else for (size_t i = 0; i < B.offsets.bytes; i++) CHECK(block[B.offsets.off + i] == 0xa5);       // left for the device
    CHECK(same(block.data(), B.inst_src, pt.inst_src) && same(block.data(), B.inst_dst, pt.inst_dst));
    CHECK(same(block.data(), B.perm, pt.perm) && same(block.data(), B.len_cap, pt.len_cap) && same(block.data(), B.inst_len, pt.inst_len));
    CHECK(same(block.data(), B.ci_src, pt.ci_src) && same(block.data(), B.ci_dst, pt.ci_dst));
    for (size_t i = 0; i < B.fold.bytes; i++) CHECK(block[B.fold.off + i] == 0xa5);                    // the caller's
    CHECK(info.size() == gt.size());
    for (size_t c = 0; c < gt.size(); c++) {
        const GroupTables &t = gt[c];
        const mixedtab::RangeRegions &r = B.range[c];
        CHECK(same(block.data(), r.recs, t.rec));
        CHECK(same(block.data(), r.comb[0], t.comb[0]) && same(block.data(), r.comb[1], t.comb[1]) && same(block.data(), r.dec, t.dec) && same(block.data(), r.terms, t.terms));
        const mixedtab::RangeInfo &i = info[c];
        CHECK(i.n_groups == t.rec.size() && i.n == t.n && i.units == t.dec.back() && i.blocks_terms == t.terms.back());
        for (int q = 0; q < 2; q++) CHECK(i.blocks_comb[q] == t.comb[q].back() && i.lds[q] == t.lds[q]);
    }
}

int main() {
    // ---- 1 and 2: the grid of the golden file
    std::vector<size_t> ns;
    for (size_t n = 0; n <= 40; n++) ns.push_back(n);
    for (size_t n : {(size_t)63, (size_t)64, (size_t)65, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)1 << 22}) ns.push_back(n);
    constexpr size_t FOLD_PLAN = 48;          // sizeof(H2vFoldPlan), a device struct this program does not see
    for (size_t n : ns) for (size_t f : {0, 1, 3, 64}) grid_point(n, f * FOLD_PLAN, {});
    const std::vector<std::vector<uint32_t>> lists = {{0}, {1}, {5}, {64}, {1, 5}, {64, 0}, {5, 5}, {0, 1, 5}, {5, 64, 1}, {64, 64, 64}, {1, 0, 64}};
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)40, (size_t)65, (size_t)4097, (size_t)1 << 22})
        for (size_t f : {1, 3, 64})
            for (const auto &l : lists) grid_point(n, f * FOLD_PLAN, l);
    // ---- 3: the packer.  1..5 plans, n up to 40, with and without host offsets, without a fold layout / with one / grouped
    const std::vector<Key> all(KEYS, KEYS + 6);
    for (uint32_t K = 1; K <= 5; K++)
        for (uint32_t n : {1u, 2u, 3u, 7u, 16u, 33u, 40u}) {
            const std::vector<Key> keys(KEYS, KEYS + K);
            std::vector<uint32_t> count(K, n / K);
            count[0] += n % K;
            for (uint32_t seed = 0; seed < 2; seed++)
                for (bool with_off : {false, true}) {
                    pack_case(keys, shuffled(count, seed), with_off, false, 0, 0);
                    pack_case(keys, shuffled(count, seed), with_off, false, 0, K * FOLD_PLAN);
                    for (uint32_t chunk : {0u, 1u, 7u, 40u}) pack_case(keys, shuffled(count, seed), with_off, true, chunk, K * FOLD_PLAN);
                }
        }
    // the shapes of tests/cpp/h2v_mixed_group.cpp
    for (uint32_t chunk : {0u, 7u, 40u, 64u, 100u})
        for (bool with_off : {false, true}) {
            pack_case(all, shuffled({70, 65, 9, 1, 0, 5}, chunk), with_off, true, chunk, 5 * FOLD_PLAN);
            pack_case(all, shuffled({0, 65, 0, 0, 0, 2}, chunk), with_off, true, chunk, 2 * FOLD_PLAN);
            pack_case(all, shuffled({0, 0, 0, 4, 2, 0}, chunk), with_off, true, chunk, 1 * FOLD_PLAN);      // nothing groupable: no range
            pack_case(all, shuffled({128, 64, 192, 0, 0, 64}, chunk), with_off, true, chunk, 4 * FOLD_PLAN);
        }
    {
        std::vector<Key> many;
        std::vector<uint32_t> count;
        for (uint32_t k = 0; k < 1024; k++) { many.push_back(KEYS[k % 6]); many.back().n_pi = 1 + k % 4; count.push_back(1); }
        for (uint32_t chunk : {0u, 3u, 512u}) pack_case(many, shuffled(count, chunk), true, true, chunk, 64 * FOLD_PLAN);
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
