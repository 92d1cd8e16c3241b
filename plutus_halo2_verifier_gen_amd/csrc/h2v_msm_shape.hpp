// Per-proof G1 MSM: the launch-shape model.  Which kernel of the family in h2v_msm.hpp runs, on how many lanes per term, in
// which block size, cut into how many segments, with or without the fixed-base launch beside it.  HOST CODE ONLY - no HIP
// call and no HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_msm_shape.cpp):
// every function is a pure function of (terms, proofs, in-flight hint, MsmModel).  h2v_capi.hip fills the MsmModel from the
// device's SIMD count and the workspace's H2V_OPT_MSM_* options and launches what these functions decide.
//
// MSM launch shape from a cost model fitted to MI355X measurements:
//  * lanes per term: 2 = one lane per GLV half, chain of ~1250 multiplications; 1 = both halves on one accumulator,
//    chain ~1600 but 36 % less work per proof and half the waves;
//  * a wave alone on its SIMD runs ~1.7x faster than two sharing one (2048 proofs: 1.50 ms, 4096: 2.6 ms), and the
//    dispatcher only spreads one wave per SIMD for 64- and 256-thread blocks (128 / 192 / 320 / 384 / 448 / 512
//    put two waves of a block on the same SIMD: 2.5 ms where 64 / 256 take 1.5 ms at 1024 waves).
// cost = chain x (1 if every wave can sit alone, else 1.7 x whole rounds of two waves per SIMD: the waves of a
// launch all take the same time, so a partly filled round costs a full one).
#pragma once
#include <stdint.h>

// what the model reads besides its arguments: the SIMDs of the device (4 per CU) and the four H2V_OPT_MSM_* options (0: auto)
struct MsmModel {
    double n_simd;
    int lanes_per_term;    // H2V_OPT_MSM_LANES_PER_TERM: 1, 2, 8
    uint32_t block_size;   // H2V_OPT_MSM_BLOCK_SIZE: 64 .. 512 in steps of 64
    int terms_per_lane;    // H2V_OPT_MSM_TERMS_PER_LANE: 1 .. 4
    int fixed_split;       // H2V_OPT_MSM_FIXED_SPLIT: 1 .. 4 bases per lane, -1 never
};
// n_seg > 1: a segmented shape (h2v_msm.hpp: k_g1_msm_seg) - n_seg segments of seg_terms terms, then the fold launch
struct MsmShape { uint32_t lpt, bs; double cost, waves; uint32_t n_seg = 1, seg_terms = 0; };
// max_seg below: the segments the partial-sum buffer of the launch has room for ([segment][proof][36 dwords]); 0: the launch
// may not be segmented.
//
// lanes_per_proof lanes of chain length `chain` per proof (of each of n_seg segments); other_waves: waves of a launch running
// beside this one
static inline void msm_try_shape(const MsmModel &m, MsmShape &best, uint32_t lpt, uint32_t lpp, double chain, uint32_t n, double other_waves,
                                 uint32_t force_bs, uint32_t n_seg = 1, uint32_t seg_terms = 0) {
    for (uint32_t cand = 64; cand <= 512; cand += 64) {
        if (cand < lpp || (force_bs && cand != force_bs)) continue;
        const uint32_t pb = cand / lpp;
        const double waves = (double)n_seg * (double)((n + pb - 1) / pb) * (cand / 64), rho = (waves + other_waves) / m.n_simd;
        const bool spreads = cand == 64 || cand == 256;
        const double rounds = rho > 2.0 ? (double)(uint64_t)((rho + 1.999) / 2.0) : 1.0;
        double cost = chain * ((spreads && rho <= 1.0) ? 1.0 : 1.7 * rounds);
        // ties: 256-thread blocks first (four waves, one per SIMD of a CU whatever the dispatcher's state: after a
        // launch of 128-thread blocks, 1024 one-wave blocks of this kernel measured 2.47 ms instead of 1.86, 256-thread
        // blocks 1.87), then one-wave blocks, then fewer idle lanes
        cost *= 1.0 + (cand == 256 ? 0.0 : cand == 64 ? 0.004 : 0.01) + 0.005 * (double)(cand - pb * lpp) / cand;
        // the fold of a segmented shape: a launch of one lane per proof, n_seg - 1 complete additions (16 multiplications of
        // the 12-limb field each) deep.  NOT MEASURED: an estimate in the ladder's units (~60 per addition plus 40 for the
        // launch's own gap) whose only job is to break ties towards fewer segments; sums of <= 64 terms never reach it
        if (n_seg > 1) cost += 60.0 * (n_seg - 1) + 40.0;
        if (cost < best.cost) { best.cost = cost; best.lpt = lpt; best.bs = cand; best.waves = waves; best.n_seg = n_seg; best.seg_terms = seg_terms; }
    }
}
// Segments a sum of T terms can be cut into (0: never, T <= 64): the fewest segments that fit a block at two lanes per term
// in a 64-thread block, ceil(T / 32), and up to two more (msm_ladder_shape).  Sizes the partial-sum buffer.
static inline uint32_t msm_max_segments(uint32_t T) { return T <= 64 ? 0u : (T + 31) / 32 + 2; }
// Shapes whose LPT x T lanes fit one block (cost 1e300: none under the forced options)
static inline MsmShape msm_ladder_fit(const MsmModel &m, uint32_t n_terms, uint32_t n, double other_waves, bool quad_ok) {
    const int env_lpt = m.lanes_per_term;
    const uint32_t env_bs = m.block_size;
    MsmShape best = {2, 512, 1e300, 0};
    for (uint32_t cl = 2; cl >= 1; cl--) {
        if (env_lpt && (uint32_t)env_lpt != cl) continue;
        msm_try_shape(m, best, cl, cl * n_terms, cl == 2 ? 1250.0 : 1600.0, n, other_waves, env_bs);
    }
    // a quad per GLV half (h2v_msm.hpp: msm_body, LPT = 8)
    // Only on request (H2V_OPT_MSM_LANES_PER_TERM = 8): alone it shortens a T = 16 launch of 64-512 proofs from 1.35 to 1.17-1.27 ms, but it issues
    // four times the instructions, and with four steps in flight - how small batches are run for throughput - the step got
    // slower at 64 and 512 proofs (1.30 -> 1.40, 1.66 -> 1.90 ms) and faster only at 256 (1.57 -> 1.47).
    if (quad_ok && 8 * n_terms <= 512 && env_lpt == 8) {
        MsmShape q = {8, 512, 1e300, 0};
        msm_try_shape(m, q, 8, 8 * n_terms, 1080.0, n, other_waves, env_bs);
        if (q.cost < 1e300) best = q;
    }
    return best;
}
// max_seg != 0: sums of more than 64 terms may also be segmented - when no shape fits one block (forced options included:
// a forced LPT 8 segments at two lanes per term), or when the cost model prefers it.  Per (LPT, block size) it prices the fewest
// segments that fit and the next two (fuller blocks), all waves of all segments plus the fold.  Sums of at most 64 terms are
// never segmented: they keep the shape they always had, a forced shape that does not fit included (the widest block, which
// holds 2 x 64 lanes).  bs == 0: nothing fits and the sum may not be segmented (the launchers then launch nothing and report 0).
static inline MsmShape msm_ladder_shape(const MsmModel &m, uint32_t n_terms, uint32_t n, double other_waves, bool quad_ok = false, uint32_t max_seg = 0) {
    MsmShape best = msm_ladder_fit(m, n_terms, n, other_waves, quad_ok);
    if (max_seg && n_terms > 64) {
        const int env_lpt = m.lanes_per_term;
        const uint32_t env_bs = m.block_size;
        for (uint32_t cl = 2; cl >= 1; cl--) {
            if (env_lpt && (env_lpt == 8 ? cl != 2 : (uint32_t)env_lpt != cl)) continue;
            for (uint32_t cand = 64; cand <= 512; cand += 64) {
                if (env_bs && cand != env_bs) continue;
                const uint32_t per = cand / cl, s0 = (n_terms + per - 1) / per;
                for (uint32_t S = s0 < 2 ? 2 : s0; S <= s0 + 2; S++) {
                    const uint32_t ts = (n_terms + S - 1) / S, s_real = (n_terms + ts - 1) / ts;
                    if (s_real > max_seg) continue;
                    msm_try_shape(m, best, cl, cl * ts, cl == 2 ? 1250.0 : 1600.0, n, other_waves, cand, s_real, ts);
                }
            }
        }
    }
    if (best.cost == 1e300) {
        if (2 * n_terms <= 512) {   // forced shape that does not fit: fall back to the widest block (it fits)
            const uint32_t pb = 512 / (2 * n_terms);
            best.lpt = 2; best.bs = 512; best.waves = (double)((n + pb - 1) / pb) * 8;
        } else {
            best.bs = 0;
        }
    }
    return best;
}
// H2V_OPT_MSM_TERMS_PER_LANE = 2 .. 4: k_g1_msm_multi (several terms per lane share the doublings: less work, fewer and longer waves;
// for callers that keep several batches in flight).  Single-group launches with prebuilt tables only.
// Without the option the caller's hint decides (h2v_workspace_hint_in_flight): a caller that keeps >= 4 batches in flight is
// bound by the instructions issued, not by chain length, and two terms per lane issue 26 % fewer multiply-adds per proof
// (measured, simple_mul x 4096: 5 in flight 5.12 -> 4.66 ms per step; with 3 in flight 5.04 -> 5.01).
// Terms per lane of the ladder kernel for callers that keep the chip full: more terms per lane share more doublings and make
// fewer, longer waves - as many as still leave the launch a quarter of a wave per SIMD (two at least).  ms per batch, eight
// batches in flight, terms per lane 2 / 3 / 4: simple_mul x 4096 (10 terms: 320 / 256 / 192 waves) 3.73 / 3.64 / 3.84;
// lookup_table x 2048 (25 terms: 416 / 288 / 224) 3.42 / 3.36 / -; x 4096 6.82 / 6.71 / 6.59; atms x 2048 (20 terms: 320 / 224 /
// 160) 3.55 / 3.72 / 4.05; sha256 shape in chunks of 1024 (25 terms: 208 / 144) 2.26 / 2.35.
static inline int msm_terms_per_lane(const MsmModel &m, uint32_t in_flight_hint, uint32_t n = 0, uint32_t n_terms = 0) {
    if (m.terms_per_lane >= 1) return m.terms_per_lane;
    if (in_flight_hint < 4) return 1;
    for (int t = 4; t > 2; t--)
        if ((double)n * ((n_terms + t - 1) / t) / 64.0 >= m.n_simd / 4.0) return t;
    return 2;
}
// The lane shape of the multi-term launch (h2v_msm.hpp: k_g1_msm_multi): halves per lane and lanes per proof for T = n_terms
// terms at `tpl` terms per lane (msm_terms_per_lane; forced: the option set it).  The launcher admits tpl <= T <= 256 tpl.
// MSM_MAX_HALVES: the most halves a lane of that kernel carries (its digit and table arrays).
#define MSM_MAX_HALVES 8
struct MsmMultiShape { uint32_t hpl, lpp; };
static inline MsmMultiShape msm_multi_shape(uint32_t n_terms, int tpl, bool tpl_forced) {
    // lanes per proof as for `tpl` whole terms per lane, then the proof's 2 T GLV halves dealt out evenly over them: ten terms
    // on four lanes are 5 + 5 + 5 + 5 halves, not 6 + 6 + 6 + 2 (a forced tpl keeps its 2 tpl halves per lane)
    const uint32_t lpp0 = (n_terms + tpl - 1) / tpl;
    const uint32_t hpl = tpl_forced ? 2u * (uint32_t)tpl : (2 * n_terms + lpp0 - 1) / lpp0;
    const uint32_t lpp = (2 * n_terms + hpl - 1) / hpl;
    return {hpl, lpp};
}
// Fixed-base split of the plan's own MSM (non-recursive plans, tables present): the per-proof terms [0, n_var) as ladders
// and, beside them on another stream, the VK-base terms as one lane per term that walks the all-window table of its base
// (65 mixed additions, no doubling: 0.88 ms alone).  Measured (2048 proofs): T = 50 with 30 VK bases 3.37 -> 2.52 ms,
// T = 34 with 9 VK bases 3.42 -> 2.68 ms; but where the single launch already has every SIMD to itself the split is
// slower (simple_mul x 4096: 1.87 -> 2.50 ms, sha256 shape x 1024: 1.99 -> 2.56 ms) - waves of two concurrent launches
// pair up on SIMDs even when there would be room for all of them alone.  So the rule is: split (one base per lane) only
// when the single launch cannot have one wave per SIMD and most terms are VK bases.  H2V_OPT_MSM_FIXED_SPLIT = k forces a split with k bases per lane, -1 forbids it.
struct MsmSplit { bool on; MsmShape var, fix; uint32_t k; };
// the term counts of a plan that may split: per-proof terms, VK-base terms (fixed-base tables present), the proof's own sum
struct MsmSplitTerms { uint32_t n_var, n_fix, n_main_terms; };
static inline MsmSplit msm_split_shape(const MsmModel &m, const MsmSplitTerms &d, uint32_t n, const MsmShape &single, uint32_t in_flight_hint = 1,
                                       uint32_t max_seg = 0) {
    const int opt_fix = m.fixed_split;                                       // 0 auto, 1 .. 4 bases per lane, -1 never
    const int env_fix = opt_fix == 0 ? -1 : opt_fix < 0 ? 0 : opt_fix;       // (-1 auto, 0 never, k forced: the form the rule below is written in)
    const uint32_t env_bs = m.block_size;
    MsmSplit out = {false, {}, {}, 0};
    if (!d.n_fix || !d.n_var || env_fix == 0) return out;
    // (and only when the VK bases are the majority of the terms: with 9 of 34 the MSM gained 0.8 ms and the pairing kernel
    // that followed the three launches lost as much of its own placement; with 6 of 16 at 8192 proofs the split was slower)
    // A caller that keeps the chip full (hint >= 4: the lanes) is bound by the instructions issued: the VK-base terms then
    // ALWAYS go through the all-window tables, two bases per lane (65 mixed additions each and no doubling, where a ladder
    // lane shares 128 doublings between two terms) - measured with six batches in flight, ms per batch: simple_mul x 4096
    // 4.39 -> 4.30, sha256 shape x 1024 2.67 -> 2.56, atms x 2048 4.43 -> 4.21, lookup_table x 2048 and secp256k1 x 512
    // unchanged (+-1 %); launches below a quarter of a wave per SIMD keep the single ladder launch (sha256 x 128: 1.17 -> 1.26).
    const bool in_flight = in_flight_hint >= 4 && d.n_fix >= 2 && (double)n * d.n_main_terms / 64.0 >= m.n_simd / 4.0;
    if (env_fix < 0 && !in_flight && (single.waves <= m.n_simd || d.n_fix < d.n_var)) return out;
    const uint32_t k = env_fix > 0 ? (uint32_t)(env_fix > 4 ? 4 : env_fix) : in_flight ? (d.n_fix >= 16 ? 4u : 2u) : 1u;   // (bases per lane: +-1 % either way)
    const uint32_t lanes = (d.n_fix + k - 1) / k;
    MsmShape fx = {1, 512, 1e300, 0};
    msm_try_shape(m, fx, 1, lanes, k * 800.0, n, 0.0, env_bs);
    if (fx.cost == 1e300) return out;
    out.on = true;
    out.k = k;
    out.fix = fx;
    out.var = msm_ladder_shape(m, d.n_var, n, fx.waves, false, max_seg);   // (the per-proof part may be segmented)
    if (out.var.bs == 0) out.on = false;
    return out;
}
