// Mixed-key calls: where everything lies in the ONE pinned block of tables a call sends up (and in the device copy its kernels
// read).  HOST CODE ONLY - no HIP call and no HIP header in this file, so that a stand-alone C++ program can include and test it
// (tests/cpp/h2v_mixed_tables.cpp): table_block() is pure arithmetic on sizes, pack_tables() copies between host buffers.
// h2v_capi.hip allocates what `extent` says and addresses the block through these regions alone.
//
//   offsets (n + 1 x 8) | inst_src | inst_dst (n x 8) | perm | len_cap | inst_len | ci_src | ci_dst (n x 4) | fold plans |
//   per grouped range:  group records | comb[0] | comb[1] | dec | terms  (n_groups + 1 x 4 each)
//   a call with keyed leaves (H2V_RLC_SEED_KEYED), behind everything else:  plan_idx (n x 4, by grouped position) | key_tags (n_plans x 32)
//   a call across several SRS (H2V_MIXED_ACROSS_SRS), behind those:  class_pos (n x 4: class-major slot -> call position)
// every region at a multiple of 16, an absent one (no fold layout, no grouped range) empty.  The fold-plan entries hold device
// pointers: the caller writes them into the region named here, and gives its size in bytes - the device struct is not known here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "h2v_mixed.hpp"
#include "h2v_mixed_group.hpp"

namespace mixedtab {
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Region { size_t off, bytes; };
struct RangeRegions { Region recs, comb[2], dec, terms; };
struct TableBlock {
    Region offsets, inst_src, inst_dst, perm, len_cap, inst_len, ci_src, ci_dst, fold;
    std::vector<RangeRegions> range;
    Region plan_idx, key_tags;              // keyed leaves only (else empty): behind every other region
    Region class_pos;                       // a call across several SRS only (else empty): the last region
    size_t extent;                          // bytes of the block
};
// n proofs, fold_bytes of fold-plan table (0: none), n_ranges grouped ranges of n_groups[c] groups each; keyed_plans: the plans
// listed in a call with keyed leaves (0: no such call - the two regions are empty and the block is what it was without them);
// across_srs: the call carries its class-major position list (h2v_mixed_srs.hpp: Classes::pos; the caller copies it in)
static inline TableBlock table_block(uint64_t n, size_t fold_bytes, const uint32_t *n_groups, size_t n_ranges, size_t keyed_plans = 0, bool across_srs = false) {
    TableBlock b{};
    size_t at = 0;
    auto put = [&at](Region &g, size_t bytes) { g = {at, bytes}; at += up16(bytes); };
    put(b.offsets, ((size_t)n + 1) * 8);
    put(b.inst_src, (size_t)n * 8); put(b.inst_dst, (size_t)n * 8);
    put(b.perm, (size_t)n * 4); put(b.len_cap, (size_t)n * 4); put(b.inst_len, (size_t)n * 4);
    put(b.ci_src, (size_t)n * 4); put(b.ci_dst, (size_t)n * 4);
    put(b.fold, fold_bytes);
    b.range.resize(n_ranges);
    for (size_t c = 0; c < n_ranges; c++) {
        RangeRegions &r = b.range[c];
        const size_t ng = n_groups[c];
        put(r.recs, ng * sizeof(H2vGroupRec));
        put(r.comb[0], (ng + 1) * 4); put(r.comb[1], (ng + 1) * 4); put(r.dec, (ng + 1) * 4); put(r.terms, (ng + 1) * 4);
    }
    put(b.plan_idx, keyed_plans ? (size_t)n * 4 : 0); put(b.key_tags, keyed_plans * 32);
    put(b.class_pos, across_srs ? (size_t)n * 4 : 0);
    b.extent = at;
    return b;
}

// what a grouped launch needs of a packed range beside its regions
struct RangeInfo { uint32_t n_groups, n, blocks_comb[2], units, blocks_terms, lds[2]; };

// Packs the partition, the grouped proof offsets when the host knows them (host_off: n + 1 entries, or NULL - the region is then
// left for the device to fill) and every range's group tables into `block` (B.extent bytes; B = table_block(pt.n, .., the ranges'
// rec.size())).  The fold region is the caller's.  info[c]: range c's counts.  Keyed leaves (B.key_tags is not empty): plan_of
// (pt.n entries, the caller's order) gives the plan index of every grouped position, key_tags the 32 bytes of every listed plan.
static inline void pack_tables(uint8_t *block, const TableBlock &B, const h2vmixed::Partition &pt, const uint64_t *host_off,
                               const std::vector<h2vmixed::GroupTables> &gt, std::vector<RangeInfo> &info,
                               const uint32_t *plan_of = nullptr, const uint8_t *key_tags = nullptr) {
    auto put = [block](const Region &g, const void *src) { if (g.bytes) memcpy(block + g.off, src, g.bytes); };
    if (host_off) put(B.offsets, host_off);
    put(B.inst_src, pt.inst_src.data()); put(B.inst_dst, pt.inst_dst.data());
    put(B.perm, pt.perm.data()); put(B.len_cap, pt.len_cap.data()); put(B.inst_len, pt.inst_len.data());
    put(B.ci_src, pt.ci_src.data()); put(B.ci_dst, pt.ci_dst.data());
    info.assign(gt.size(), RangeInfo{});
    for (size_t c = 0; c < gt.size(); c++) {
        const h2vmixed::GroupTables &t = gt[c];
        const RangeRegions &r = B.range[c];
        RangeInfo &i = info[c];
        put(r.recs, t.rec.data());
        for (int q = 0; q < 2; q++) { put(r.comb[q], t.comb[q].data()); i.blocks_comb[q] = t.comb[q].back(); i.lds[q] = t.lds[q]; }
        put(r.dec, t.dec.data()); i.units = t.dec.back();
        put(r.terms, t.terms.data()); i.blocks_terms = t.terms.back();
        i.n_groups = (uint32_t)t.rec.size(); i.n = t.n;
    }
    if (B.plan_idx.bytes && plan_of)
        for (uint32_t g = 0; g < pt.n; g++) memcpy(block + B.plan_idx.off + (size_t)g * 4, &plan_of[pt.perm[g]], 4);
    if (key_tags) put(B.key_tags, key_tags);
}
}   // namespace mixedtab
