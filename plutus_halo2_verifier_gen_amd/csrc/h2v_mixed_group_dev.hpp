// Mixed-key batches with H2V_MIXED_GROUPED (include/h2v.h), device side: the three phase-1 kernels that take their plan from a
// table per block instead of from the kernel argument (tables: h2v_mixed_group.hpp).
//   k_transcript_combiner_grouped(_b512)   block -> group -> vm_run<RegsLds, KIND> on the group's plan record, P and L from the
//                                          record; one launch per transcript kind present (the other kind's groups have no block
//                                          in the launch's prefix array)
//   k_g1_decompress_queue_grouped          k_g1_decompress_queue's walk (subgroup units, then roots) over the units of all groups:
//                                          dec_group with the unit's group record and the unit's index within its group, no tables
//   k_mixed_terms_grouped                  k_mixed_terms' body (h2v_mixed_terms_body.inc) with the block's group as its sub-batch
// The record is uniform per block (unit): it is read through recs + g with g made wave-uniform, from memory no kernel writes, so
// the loads can be scalar; nothing of it is copied into a private array.
// Included behind h2v_mixed_fold_dev.hpp (uses vm_run, dec_group and the terms body).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "h2v_mixed_group.hpp"

struct GroupCombinerArgs {
    const H2vGroupRec *recs;
    const uint32_t *prefix;      // n_groups + 1: combiner blocks of this launch's transcript kind
    uint32_t n_groups;
    const uint8_t *proofs;       // the grouped staging
    const uint64_t *off;
    const uint8_t *inst, *ci;
    uint32_t *scalars, *status;  // the workspace's
};
template <uint32_t TRK> H2V_DI void combiner_grouped_block(const GroupCombinerArgs &a, uint32_t *sbuf, uint32_t *st_red) {
    const int lane = threadIdx.x;
    const uint32_t g = __builtin_amdgcn_readfirstlane(h2v_group_find(a.prefix, a.n_groups, blockIdx.x));
    const H2vGroupRec &rec = a.recs[g];
    const uint32_t bb = blockIdx.x - a.prefix[g];
    const uint32_t P = rec.P, L = rec.plan.vm_lanes, n = rec.count;
    const uint32_t q = (uint32_t)lane & (P - 1);
    const uint32_t sub = L > 1 ? ((uint32_t)lane / P) % L : 0u;
    const uint32_t i = bb * P + q;
    const bool live = (uint32_t)lane < P * L && i < n;
    const uint32_t ii = i < n ? i : n - 1;
    const RegsLds rf = {P, q};
    vm_run<RegsLds, TRK>(rec.plan, rf, sbuf, lane, i, ii, live, L, sub, st_red, P, a.proofs, a.off + rec.off_idx, a.inst + rec.inst_off,
                         a.ci + rec.ci_idx * 48, a.scalars + rec.scal_base, a.status + rec.first, nullptr);
}
extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner_grouped(GroupCombinerArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    __shared__ uint32_t st_red[64];
    combiner_grouped_block<H2V_TR_CARDANO_BLAKE2B_256>(a, sbuf, st_red);
}
extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner_grouped_b512(GroupCombinerArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    __shared__ uint32_t st_red[64];
    combiner_grouped_block<H2V_TR_BLAKE2B_512>(a, sbuf, st_red);
}

struct GroupDecompressArgs {
    const H2vGroupRec *recs;
    const uint32_t *prefix;      // n_groups + 1: 64-point units
    uint32_t n_groups, n_units;  // n_units = prefix[n_groups]
    const uint8_t *proofs;
    const uint64_t *off;
    const uint8_t *inst, *ci;
    uint32_t *pts;               // the workspace's
    uint8_t *valid, *valid_sub;
    uint32_t *counter;           // zeroed by the host
};
extern "C" __global__ void __launch_bounds__(256, 2)
k_g1_decompress_queue_grouped(GroupDecompressArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    for (;;) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(a.counter, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= 2 * a.n_units) break;
        const uint32_t role = u < a.n_units ? 1u : 0u, unit = role ? u : u - a.n_units;
        const uint32_t g = __builtin_amdgcn_readfirstlane(h2v_group_find(a.prefix, a.n_groups, unit));
        const H2vGroupRec &rec = a.recs[g];
        dec_group(rec.plan, rec.count, a.proofs, a.off + rec.off_idx, a.ci + rec.ci_idx * 48, a.inst + rec.inst_off, a.pts + rec.pts_base * 24,
                  a.valid + rec.pts_base, nullptr, role ? 2u : 1u, a.valid_sub + rec.pts_base, unit - a.prefix[g], role, lane, nullptr);
    }
}

struct GroupTermsArgs {
    const H2vGroupRec *recs;
    const uint32_t *prefix;      // n_groups + 1: 64-proof blocks
    uint32_t n_groups;
    const uint32_t *scalars, *status;   // the workspace's phase-1 results
    const uint8_t *valid, *valid_sub;
    const uint32_t *pts;
    const uint32_t *pos;         // grouped index -> position in the call (the call's perm)
    uint32_t seed[8];
    uint32_t *r_scal, *r_pts;    // the call's term pool from R-term 0 on
    uint32_t *l_scal, *l_pts;
    uint32_t *vk_part;           // the call's per-block sums from Fr record 0 on
    uint8_t *good;
    uint32_t *status_out;
    const uint32_t *seed_dev;    // as MixedTermsArgs: NULL, or the call's derived seed in device memory
};
// what the terms body reads of a sub-batch (MixedTermsArgs without the seed)
struct MixedTermsView {
    uint32_t n, n_var, n_fix, slots, pi_point, scal_stride;
    const uint32_t *terms, *scalars, *status;
    const uint8_t *valid, *valid_sub;
    const uint32_t *pts, *pos;
    uint32_t *r_scal, *r_pts, *l_scal, *l_pts, *vk_part;
    uint8_t *good;
    uint32_t *status_out;
};
extern "C" __global__ void __launch_bounds__(64)
k_mixed_terms_grouped(GroupTermsArgs ga) {
    __shared__ uint32_t sbuf[32 * 64];
    const uint32_t g = __builtin_amdgcn_readfirstlane(h2v_group_find(ga.prefix, ga.n_groups, blockIdx.x));
    const H2vGroupRec &rec = ga.recs[g];
    const MixedTermsView a = {rec.count, rec.n_var, rec.n_fix, rec.slots, rec.plan.pi_point, rec.plan.n_terms,
                              rec.plan.terms, ga.scalars + rec.scal_base, ga.status + rec.first,
                              ga.valid + rec.pts_base, ga.valid_sub + rec.pts_base, ga.pts + rec.pts_base * 24, ga.pos + rec.off_idx,
                              ga.r_scal + rec.term_base * 8, ga.r_pts + rec.term_base * 24, ga.l_scal, ga.l_pts, ga.vk_part + rec.part_base * 8,
                              ga.good, ga.status_out};
    const uint32_t blk = blockIdx.x - ga.prefix[g];
#define MT_BLK blk
#define MT_SEED ga
#include "h2v_mixed_terms_body.inc"
#undef MT_BLK
#undef MT_SEED
}
