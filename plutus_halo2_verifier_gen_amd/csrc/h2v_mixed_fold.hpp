// Mixed-key batches with H2V_MIXED_FOLD_MSM (include/h2v.h): the layout of the call-level term pool.  HOST CODE ONLY - no HIP
// call and no HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_mixed_terms.cpp).
//
// The fold form sums the whole call in ONE bucket MSM: R = sum over N_R terms (scalar, copied affine point), L = sum over the n
// proofs (r_i, L_i) at their call positions.  A plan is FOLDABLE when it has the batch form of DESIGN.md 12 (per-proof terms plus
// VK bases whose scalars can be summed in Fr first); any other plan - a recursive one above all - runs its own MSM and joins the
// sums as one pair per proof.  The R-terms of a call, in this order:
//   [term_base[k], + count[k] x n_var(k))   foldable plan k, proof j of the plan (grouped order), term t at term_base[k] + j n_var + t
//   [vk_base[k],   + n_fix(k))              foldable plan k, its VK bases with the summed scalars
//   [pair_base[k], + count[k])              non-foldable plan k, proof j: (r, R_j)
// so N_R = sum_{foldable k with proofs} (count[k] n_var(k) + n_fix(k)) + (proofs of non-foldable plans); a plan without a proof
// has no term.  More than 2^22 terms is H2V_E_LIMIT (fold_layout returns false and says so).
// The VK-base scalars are summed per block of 64 proofs first (k_mixed_terms), and a plan's proofs may run in chunks of
// `chunk` proofs on different lanes: chunk c of plan k owns the blocks [block_base[k] + c ceil(chunk / 64), + ceil(m_c / 64)),
// where m_c is the chunk's size, and block b of plan k its n_fix(k) sums from Fr record part_base[k] + (b - block_base[k]) n_fix(k) on.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace h2vmixed {

#define H2V_MIXED_FOLD_MAX_TERMS (1ull << 22)

struct FoldShape { uint32_t n_var, n_fix; bool foldable; };

struct FoldLayout {
    uint32_t n_plans = 0, chunk = 0;               // chunk = 0: every plan's proofs in one piece
    std::vector<uint8_t> foldable;                 // n_plans: foldable AND has proofs
    std::vector<uint32_t> term_base, vk_base, pair_base;   // n_plans; 0 where they do not apply
    std::vector<uint32_t> block_base, n_blocks;    // n_plans: blocks of 64 proofs of foldable plans (0 blocks otherwise)
    std::vector<uint64_t> part_base;               // n_plans: first Fr record of the plan's per-block sums
    std::vector<uint32_t> fix_base;                // n_plans: VK bases of the foldable plans before it (the lane index of k_mixed_vk_sum)
    uint64_t n_r = 0, n_parts = 0;                 // terms of R; Fr records of all per-block sums
    uint32_t total_blocks = 0, total_fix = 0, n_pairs = 0, n_foldable = 0;
};

// blocks of 64 proofs that `count` proofs take when they run in chunks of `chunk` (0: one piece)
inline uint32_t fold_blocks(uint32_t count, uint32_t chunk) {
    if (chunk == 0 || chunk >= count) return (count + 63) / 64;
    const uint32_t full = count / chunk, rest = count % chunk;
    return full * ((chunk + 63) / 64) + (rest + 63) / 64;
}
// the first block (within its plan) of the chunk that starts at proof `first` of the plan
inline uint32_t fold_chunk_block(uint32_t first, uint32_t chunk) {
    return chunk == 0 ? 0u : (first / chunk) * ((chunk + 63) / 64);
}

// false: the call has more than 2^22 terms (err says how many).  count[k]: proofs of plan k (Partition::count).
inline bool fold_layout(const FoldShape *shapes, const uint32_t *count, uint32_t n_plans, uint32_t chunk, FoldLayout &out, std::string *err) {
    out = FoldLayout();
    out.n_plans = n_plans; out.chunk = chunk;
    out.foldable.assign(n_plans, 0);
    out.term_base.assign(n_plans, 0); out.vk_base.assign(n_plans, 0); out.pair_base.assign(n_plans, 0);
    out.block_base.assign(n_plans, 0); out.n_blocks.assign(n_plans, 0); out.part_base.assign(n_plans, 0); out.fix_base.assign(n_plans, 0);
    uint64_t run = 0;                                   // (64-bit throughout: the bases below are only read when n_r is within the limit)
    for (uint32_t k = 0; k < n_plans; k++) {            // the per-proof terms
        if (!count[k] || !shapes[k].foldable) continue;
        out.foldable[k] = 1; out.n_foldable++;
        out.term_base[k] = (uint32_t)run;
        run += (uint64_t)count[k] * shapes[k].n_var;
        out.block_base[k] = out.total_blocks; out.n_blocks[k] = fold_blocks(count[k], chunk);
        out.total_blocks += out.n_blocks[k];
        out.part_base[k] = out.n_parts;
        out.n_parts += (uint64_t)out.n_blocks[k] * shapes[k].n_fix;
        out.fix_base[k] = out.total_fix;
        out.total_fix += shapes[k].n_fix;
    }
    for (uint32_t k = 0; k < n_plans; k++)              // the VK bases
        if (out.foldable[k]) { out.vk_base[k] = (uint32_t)run; run += shapes[k].n_fix; }
    for (uint32_t k = 0; k < n_plans; k++)              // one pair per proof of the other plans
        if (count[k] && !out.foldable[k]) { out.pair_base[k] = (uint32_t)run; run += count[k]; out.n_pairs += count[k]; }
    out.n_r = run;
    if (run > H2V_MIXED_FOLD_MAX_TERMS) {
        if (err) *err = "the fold form sums at most 2^22 terms in one call, this one has " + std::to_string(run) + ": split it, or leave H2V_MIXED_FOLD_MSM out";
        return false;
    }
    return true;
}

}   // namespace h2vmixed
