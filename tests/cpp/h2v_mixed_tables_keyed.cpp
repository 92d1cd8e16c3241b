// Stand-alone test of the table block of a mixed-key call with keyed leaves (H2V_RLC_SEED_KEYED; csrc/h2v_mixed_tables.hpp): the
// two regions the digest launch reads - the plan index of every grouped position, 32 bytes of key tag per listed plan - lie behind
// every other region.  Host code only: built with -fsanitize=address,undefined and run as a program (tests/test_keyed_seed_tables.py).
//   1. n = 0, 1, 64, 65 x 1, 3, 1024 listed plans, with and without a fold table and grouped ranges: every region disjoint from
//      every other, 16-byte aligned, inside the extent; the block without keyed plans is what it was (the defaults)
//   2. real Partitions packed into a vector of EXACTLY `extent` bytes - one byte too many is ASan's to see - and read back:
//      plan_idx[g] = plan_of[perm[g]], the tags as given, the older regions untouched by the new ones
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
    v.push_back(B.plan_idx); v.push_back(B.key_tags);
    return v;
}
static void layout_point(size_t n, size_t plans, size_t fold_bytes, const std::vector<uint32_t> &groups) {
    const TableBlock B = mixedtab::table_block(n, fold_bytes, groups.data(), groups.size(), plans);
    const TableBlock old = mixedtab::table_block(n, fold_bytes, groups.data(), groups.size());
    CHECK(B.plan_idx.bytes == n * 4 && B.key_tags.bytes == plans * 32);
    CHECK(old.plan_idx.bytes == 0 && old.key_tags.bytes == 0);
    // behind every existing region: what was there lies where it lay, and the old extent is where the new regions start
    CHECK(B.plan_idx.off == old.extent && old.extent <= B.extent);
    const std::vector<Region> now = regions_of(B), was = regions_of(old);
    for (size_t q = 0; q + 2 < now.size(); q++) CHECK(now[q].off == was[q].off && now[q].bytes == was[q].bytes);
    size_t end = 0;
    for (const Region &g : now) {      // in order, aligned, each behind the end of the one before (so: pairwise disjoint), inside the extent
        CHECK(g.off % 16 == 0);
        CHECK(g.off >= end);
        end = g.off + g.bytes;
        CHECK(end <= B.extent);
    }
    for (size_t a = 0; a < now.size(); a++)
        for (size_t b = a + 1; b < now.size(); b++)
            CHECK(now[a].bytes == 0 || now[b].bytes == 0 || now[a].off + now[a].bytes <= now[b].off || now[b].off + now[b].bytes <= now[a].off);
}
static void pack_point(uint32_t n, uint32_t plans, bool with_off, size_t fold_bytes) {
    std::vector<PlanShape> ps(plans);
    for (uint32_t k = 0; k < plans; k++) ps[k] = {1000u + k, k % 4, k % 3 == 1 ? 1u : 0u};
    std::vector<uint32_t> plan_of(n ? n : 1);
    for (uint32_t i = 0; i < n; i++) plan_of[i] = (uint32_t)((i * 7u + i / 5u) % plans);
    Partition pt;
    std::string err;
    CHECK(partition(ps.data(), plans, plan_of.data(), n, pt, &err));
    std::vector<uint8_t> tags((size_t)plans * 32);
    for (size_t q = 0; q < tags.size(); q++) tags[q] = (uint8_t)(q * 31 + 5);
    const TableBlock B = mixedtab::table_block(n, fold_bytes, nullptr, 0, plans);
    std::vector<uint64_t> off(n + 1);
    for (uint32_t i = 0; i <= n; i++) off[i] = 900ull * i + 3;
    std::vector<uint8_t> block(B.extent, 0xa5);              // EXACTLY the extent
    std::vector<mixedtab::RangeInfo> info;
    mixedtab::pack_tables(block.data(), B, pt, with_off ? off.data() : nullptr, {}, info, plan_of.data(), tags.data());
    CHECK(B.key_tags.bytes == tags.size() && memcmp(block.data() + B.key_tags.off, tags.data(), tags.size()) == 0);
    for (uint32_t g = 0; g < n; g++) {
        uint32_t v;
        memcpy(&v, block.data() + B.plan_idx.off + (size_t)g * 4, 4);
        CHECK(v == plan_of[pt.perm[g]] && v < plans);
    }
    CHECK(B.perm.bytes == (size_t)n * 4 && (n == 0 || memcmp(block.data() + B.perm.off, pt.perm.data(), B.perm.bytes) == 0));
    CHECK(n == 0 || memcmp(block.data() + B.ci_dst.off, pt.ci_dst.data(), B.ci_dst.bytes) == 0);
    for (size_t i = 0; i < B.fold.bytes; i++) CHECK(block[B.fold.off + i] == 0xa5);                    // the caller's
    if (!with_off) for (size_t i = 0; i < B.offsets.bytes; i++) CHECK(block[B.offsets.off + i] == 0xa5);
    // without the keyed arguments the packer writes nothing into the two regions
    std::vector<uint8_t> plain(B.extent, 0x5a);
    mixedtab::pack_tables(plain.data(), B, pt, nullptr, {}, info);
    for (size_t i = B.plan_idx.off; i < B.extent; i++) CHECK(plain[i] == 0x5a);
}

int main() {
    constexpr size_t FOLD_PLAN = 48;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)64, (size_t)65})
        for (size_t plans : {(size_t)1, (size_t)3, (size_t)1024}) {
            for (size_t f : {(size_t)0, (size_t)3}) {
                layout_point(n, plans, f * FOLD_PLAN, {});
                layout_point(n, plans, f * FOLD_PLAN, {5});
                layout_point(n, plans, f * FOLD_PLAN, {1, 0, 64});
                for (bool with_off : {false, true}) pack_point((uint32_t)n, (uint32_t)plans, with_off, f * FOLD_PLAN);
            }
        }
    layout_point((size_t)1 << 22, 1024, 64 * FOLD_PLAN, {64, 64});
    std::printf("ok %ld\n", checks);
    return 0;
}
