// Mixed-key batches with H2V_MIXED_FOLD_MSM (include/h2v.h), device side: the kernels that emit the terms of the call's ONE
// bucket MSM into call-level pools (layout: h2v_mixed_fold.hpp).  The pools own what the tail reads - scalars AND points are
// copied - because the lanes' point buffers are recycled by the chunks that follow.
//   k_mixed_terms        a chunk of a FOLDABLE plan after phase 1 (k_rlc_prepare's work, keyed by the position in the CALL):
//                        good / status / (r, pi) at pos[i]; the n_var scaled scalars and copied points of the proof; the
//                        per-block Fr sums of the VK-base products
//   k_mixed_vk_sum       one lane per (plan, VK base): adds the plan's block sums, appends the term with a copy of the base
//   k_mixed_pair_terms   proofs of the other plans (their pairs are in the call's pool: k_mixed_pairs): (r, R) among the
//                        R-terms, (r, L) as the position's L-term
// r = low 128 bits of blake2b-256(seed || LE32(position in the call)), 1 if that is 0, 0 for a proof that takes no part.
// Included behind h2v_mixed_dev.hpp (uses the transcript hash and the field helpers of h2v_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the batch coefficient of call position `at` as four dwords; every lane of the block calls it (the hash works through sbuf)
// (a: the kernel's argument struct - its seed stays in the argument segment, read at a run-time index by scalar loads; with
// a.seed_dev - a call with keyed leaves, H2V_RLC_SEED_KEYED - the words come from device memory instead: seed_word, no chunk tweak)
template <class A> H2V_DI void mixed_coeff(uint32_t (&r)[4], const A &a, uint32_t at, bool good, uint32_t *sbuf, int lane) {
    Transcript tr;
    tr_init(tr);
#pragma unroll 1
    for (int k = 0; k < 32; k++) tr_put(tr, sbuf, lane, (seed_word(a.seed, a.seed_dev, 0u, k >> 2) >> (8 * (k & 3))) & 0xffu);
#pragma unroll 1
    for (int k = 0; k < 4; k++) tr_put(tr, sbuf, lane, (at >> (8 * k)) & 0xffu);
    uint64_t h[4];
    tr_digest(tr, sbuf, lane, h);
    r[0] = (uint32_t)h[0]; r[1] = (uint32_t)(h[0] >> 32); r[2] = (uint32_t)h[1]; r[3] = (uint32_t)(h[1] >> 32);
    if ((r[0] | r[1] | r[2] | r[3]) == 0) r[0] = 1;
    if (!good) { r[0] = 0; r[1] = 0; r[2] = 0; r[3] = 0; }
}
// one 24-dword affine record (16-byte aligned on both sides) - or 24 zero dwords
H2V_DI void mixed_copy_point(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, bool take) {
    const uint4 *s4 = (const uint4 *)src;
    uint4 *d4 = (uint4 *)dst;
#pragma unroll
    for (int k = 0; k < 6; k++) d4[k] = take ? s4[k] : make_uint4(0u, 0u, 0u, 0u);
}

struct MixedTermsArgs {
    uint32_t n, n_var, n_fix, slots, pi_point, scal_stride;
    const uint32_t *terms;      // the plan's (kind, index) table: [0, n_var) per-proof slots, then the VK bases
    const uint32_t *scalars;    // n x scal_stride x 8, canonical (the combiner's)
    const uint32_t *status;     // n: the chunk's status words
    const uint8_t *valid, *valid_sub;
    const uint32_t *pts;        // n x slots x 24: the chunk's decompressed points
    const uint32_t *pos;        // n: position in the call
    uint32_t seed[8];
    uint32_t *r_scal, *r_pts;   // the chunk's first R-term: n x n_var records of 8 / 24 dwords
    uint32_t *l_scal, *l_pts;   // the call's L-terms, by position
    uint32_t *vk_part;          // the chunk's first block: ceil(n / 64) x n_fix x 8 (Montgomery)
    uint8_t *good;              // by position
    uint32_t *status_out;       // by position (H2V_ST_BAD_POINT folded in)
    const uint32_t *seed_dev;   // NULL: `seed` above, bit for bit; else the call's derived seed in device memory (8 dwords)
};

extern "C" __global__ void __launch_bounds__(64)
k_mixed_terms(MixedTermsArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
#define MT_BLK blockIdx.x
#define MT_SEED a
#include "h2v_mixed_terms_body.inc"
#undef MT_BLK
#undef MT_SEED
}

// what k_mixed_vk_sum reads of a foldable plan with proofs (h2v_mixed_fold.hpp: FoldLayout)
struct H2vFoldPlan {
    const uint32_t *vk_bases;   // the plan's VK bases, 24-dword affine records
    const uint32_t *terms;      // the plan's term table
    uint32_t n_var, n_fix;
    uint32_t fix_base;          // VK bases of the plans before it: its lanes are [fix_base, fix_base + n_fix)
    uint32_t n_blocks;          // blocks of 64 proofs that hold sums of this plan
    uint32_t vk_base;           // R-term of its first VK base
    uint32_t pad;
    uint64_t part_base;         // Fr record of block 0's first sum
};
extern "C" __global__ void __launch_bounds__(64)
k_mixed_vk_sum(const H2vFoldPlan *__restrict__ plans, uint32_t n_plans, uint32_t total_fix, const uint32_t *__restrict__ vk_part,
               uint32_t *__restrict__ r_scal, uint32_t *__restrict__ r_pts) {
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= total_fix) return;
    uint32_t k = 0;
    while (k + 1 < n_plans && g >= plans[k].fix_base + plans[k].n_fix) k++;
    const H2vFoldPlan pl = plans[k];
    const uint32_t f = g - pl.fix_base;
    Fr acc, c;
    FrF::set_zero(acc);
#pragma unroll 1
    for (uint32_t b = 0; b < pl.n_blocks; b++) {
        Fr p;
#pragma unroll
        for (int l = 0; l < 8; l++) p.v[l] = vk_part[(pl.part_base + (uint64_t)b * pl.n_fix + f) * 8 + l];
        fr_add(acc, acc, p);
    }
    fr_from_mont(c, acc);
    const size_t e = (size_t)pl.vk_base + f;
#pragma unroll
    for (int l = 0; l < 8; l++) r_scal[e * 8 + l] = c.v[l];
    const uint32_t *bp = pl.vk_bases + (size_t)pl.terms[2 * (pl.n_var + f) + 1] * 24;   // (a section of the plan blob: dword loads)
#pragma unroll
    for (int l = 0; l < 24; l++) r_pts[e * 24 + l] = bp[l];
}

// n proofs of a plan that is not foldable; pos[j]: their positions in the call, where k_mixed_pairs left (L, R), good and status
struct MixedPairTermsArgs {
    uint32_t n, term_base;      // the plan's proofs; R-term of its first one
    const uint32_t *pos;        // n
    const uint32_t *pool;       // call x 2 x 24: the pairs, by position
    const uint8_t *good;        // by position
    uint32_t seed[8];
    uint32_t *r_scal, *r_pts, *l_scal, *l_pts;
    const uint32_t *seed_dev;   // as MixedTermsArgs
};
extern "C" __global__ void __launch_bounds__(64)
k_mixed_pair_terms(MixedPairTermsArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * 64 + lane;
    const bool live = j < a.n;
    const uint32_t jj = live ? j : a.n - 1;
    const uint32_t at = a.pos[jj];
    const bool good = live && a.good[at] != 0;
    uint32_t r[4];
    mixed_coeff(r, a, at, good, sbuf, lane);
    if (!live) return;
    const size_t e = (size_t)a.term_base + j;
#pragma unroll
    for (int l = 0; l < 8; l++) { const uint32_t v = l < 4 ? r[l] : 0u; a.r_scal[e * 8 + l] = v; a.l_scal[(size_t)at * 8 + l] = v; }
    mixed_copy_point(a.l_pts + (size_t)at * 24, a.pool + (size_t)at * 48, good);
    mixed_copy_point(a.r_pts + e * 24, a.pool + (size_t)at * 48 + 24, good);
}
