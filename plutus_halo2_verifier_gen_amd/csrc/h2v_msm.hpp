// ============================================================================ K4: per-proof G1 MSM
// Included by h2v_kernels.hip (uses its field, curve and plan headers).  The launch shapes are decided on the host:
// h2v_msm_shape.hpp; the launch sites are in h2v_capi.hip (launch_msm_ladders, launch_msm_fixed, launch_msm_range).
//
// er = sum_t s_t * B_t with T = n_terms (16 ... ~70 for real keys) 255-bit scalars per proof.  T is far too small for bucket
// (Pippenger) accumulation to pay - 2^c buckets per window would outnumber the terms - so the mapping is:
//   * TWO lanes per (proof, term): the GLV split k = k1 + k2*lambda gives lane 0 the pair (k1, P) and lane 1
//     (k2, phi(P) = (beta' x, y)), both scalars below 2^128 (half the doubling chain, twice the waves);
//   * per lane a signed 4-bit window ladder on the lazily reduced field: table [1..8]*P, affine, in a per-lane slab
//     of the workspace; 33 windows of 4 doublings + one mixed addition (digits in [-8, 8]);
//   * a segmented tree reduction of the 2*T partial sums of each (proof, term group) through LDS.
// Bytes per term: 32 (scalar) + 96 (affine base) in, 144 per proof out (Jacobian).
// One launch sums a RANGE of a term table (the proof's own MSM; with recursion also acc_left, acc_right + fixed bases,
// and the two folds el + c*acc_left, er + c*acc_right over the fold's own point / scalar buffers):
#pragma once
#include "h2v_msm_shape.hpp"
struct H2vMsmArgs {
    const uint32_t *terms;     // (kind, index) pairs; kind = VK base or per-proof slot of `pts`
    uint32_t term_base;        // first term of the range
    uint32_t n_terms;          // terms in the range (LPT * n_terms lanes per proof, <= the block; wider: segments, k_g1_msm_seg)
    uint32_t scal_stride;      // scalars per proof in `scalars`
    uint32_t scal_col_base;    // column of the range's first term
    uint32_t slots;            // point slots per proof in `pts`
    // the range is cut into up to three consecutive groups, each summed into its own output (recursion: the proof's
    // MSM, acc_left and acc_right + fixed bases in ONE launch): group g = terms [grp_end[g-1], grp_end[g])
    uint32_t grp_end[3];
    uint32_t *out[3];          // n x 36 dwords each (Jacobian); unused groups: grp_end == n_terms
    // window tables built ahead of the MSM (2 x 224 dwords per point: P and phi(P)): per-proof slots by the
    // decompression kernel, VK bases at plan load.  NULL: every lane builds its own table into `tabws` (fold MSMs).
    const uint32_t *pt_tab;    // [proof][slot][2][224]
    const uint32_t *vk_tab;    // [base][2][224]
    // fixed-base launches (k_g1_msm_fixed; one group, every term of the range a VK base): lane f of a proof's n_fixl
    // lanes sums the fix_k terms f * fix_k ... of the range from the all-window tables fix_tab [base][65 windows][8][28]
    const uint32_t *fix_tab;
    uint32_t fix_k, n_fixl;
    // RLC batch mode: the per-proof MSM queued behind the batch check (k_g1_msm*_cond) returns at once when *skip != 0
    const uint32_t *skip;
};

// ---------------------------------------------------------------------------- the pieces every kernel of the family shares
// a Jacobian point as the kernels exchange it: 36 dwords, x | y | z
H2V_DI void g1j_load36(G1J &p, const uint32_t *src) {
#pragma unroll
    for (int k = 0; k < 12; k++) { p.x.v[k] = src[k]; p.y.v[k] = src[12 + k]; p.z.v[k] = src[24 + k]; }
}
H2V_DI void g1j_store36(uint32_t *dst, const G1J &p) {
#pragma unroll
    for (int k = 0; k < 12; k++) { dst[k] = p.x.v[k]; dst[12 + k] = p.y.v[k]; dst[24 + k] = p.z.v[k]; }
}
// Term `term` of the range for proof i: where its affine base (24 dwords), its scalar (8 dwords) and its window tables (P,
// and 224 dwords on phi(P); meaningful only with prebuilt tables, ma.pt_tab != NULL) are.
// terms[] as uploaded by h2v_plan_load: kind is VK base (1) or per-proof slot (0); the committed instance has
// been rewritten to slot n_points there.  Two-way integer selects only: a nested three-way pointer select was
// miscompiled by ROCm 7.2 (the copy of i feeding the scalar address was left undefined on the third path).
// vk_only (a constant of the caller): every term of the range is a VK base and its kind is not read.
struct MsmTerm { bool is_vk; uint32_t idx; const uint32_t *base, *scal; };
H2V_DI MsmTerm msm_term(const H2vDevPlan &plan, const H2vMsmArgs &ma, const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ pts,
                        const uint32_t i, const uint32_t term, const bool vk_only = false) {
    MsmTerm t;
    t.idx = ma.terms[2 * (ma.term_base + term) + 1];
    t.is_vk = vk_only || ma.terms[2 * (ma.term_base + term)] == H2V_TERM_VK_BASE;
    const uint32_t *src = t.is_vk ? plan.vk_bases : pts;
    const size_t elem = t.is_vk ? (size_t)t.idx : (size_t)i * ma.slots + t.idx;
    t.base = src + elem * 24;
    t.scal = scalars + ((size_t)i * ma.scal_stride + ma.scal_col_base + term) * 8;
    return t;
}
// ... and its prebuilt window tables (ma.pt_tab != NULL): P, and 224 dwords on phi(P)
H2V_DI const uint32_t *msm_term_tab(const H2vMsmArgs &ma, const MsmTerm &t, const uint32_t i) {
    return t.is_vk ? ma.vk_tab + (size_t)t.idx * 448 : ma.pt_tab + ((size_t)i * ma.slots + t.idx) * 448;
}
// signed 4-bit recoding of a 128-bit GLV half, least significant digit first: dg[q] in [-8, 8], q = 0 .. 32.
// !use: all digits zero (a half that contributes nothing).
H2V_DI void msm_recode4(int8_t (&dg)[33], const uint32_t *kk /* four words */, const bool use = true) {
    uint32_t carry = 0;
#pragma unroll 1
    for (int q = 0; q < 32; q++) {
        uint32_t d = ((kk[q >> 3] >> (4 * (q & 7))) & 15u) + carry;
        carry = d > 8 ? 1u : 0u;
        dg[q] = use ? (int8_t)(carry ? (int)d - 16 : (int)d) : (int8_t)0;
    }
    dg[32] = use ? (int8_t)carry : (int8_t)0;
}
// signed c-bit digits of a 256-bit scalar, least significant first (c = plan.fix_c: 4, 8 or 12; W windows; the last window takes the
// carry: for c = 4 / 8 it is a window of its own, for c = 12 the top window holds 4 bits and has the room)
H2V_DI void msm_recode_c(int16_t (&dg)[65], const uint32_t (&sc)[8], const uint32_t c, const uint32_t W) {
    const uint32_t E = 1u << (c - 1), mask = (1u << c) - 1u;
    uint32_t carry = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < W; q++) {
        const uint32_t bit = q * c, word = bit >> 5, sh = bit & 31;
        uint64_t two = 0;
        if (word < 8) two = (uint64_t)sc[word] | (word + 1 < 8 ? (uint64_t)sc[word + 1] << 32 : 0ull);
        uint32_t d = ((uint32_t)(two >> sh) & mask) + carry;
        carry = d > E ? 1u : 0u;
        dg[q] = (int16_t)(carry ? (int)d - (int)(mask + 1u) : (int)d);
    }
}
// The first non-zero digit of a ladder: the accumulator becomes the affine table entry Q = (qx, qy), negated for a negative
// digit.  How later entries are added - unchecked or by the complete law - is each ladder's own rule, argued where it stands.
H2V_DI void msm_acc_start(G1J28 &acc, bool &acc_inf, const F28 &qx, const F28 &qy, const bool neg) {
    acc.x = qx;
    acc.y = qy;
    if (neg) { F28_NEG(acc.y, qy, 3, 1); f28_carry(acc.y); }
    f28_set_one(acc.z);
    acc_inf = false;
}
// ... and the complete addition of such an entry
H2V_DI void msm_acc_add_affine(G1J28 &acc, bool &acc_inf, const F28 &qx, const F28 &qy, const bool neg) {
    G1J28 o;
    o.x = qx; o.y = qy;
    f28_set_one(o.z);
    g1j28_acc_add(acc, acc_inf, o, neg);
}
// Segmented reduction over the lanes of each (proof, group), still on the lazy field: 42 limbs + the flag per lane
// in LDS (dword d of thread t at red[d*bs + t]); the lane gsub == 0 of a group ends up with the group's sum.
// in_block: this lane belongs to one of the block's proofs; gsub / glen: its position in, and the length of, its group's lanes.
// MSM_LDS_BYTES: the dynamic LDS of every launch of the family.
#define MSM_RED_DWORDS 43
#define MSM_LDS_BYTES(bs) ((size_t)(bs) * MSM_RED_DWORDS * 4)
H2V_DI void msm_red_store(uint32_t *red, const G1J28 &lad, const bool lad_inf) {
    const uint32_t tid = threadIdx.x, bs = blockDim.x;
#pragma unroll
    for (int k = 0; k < 14; k++) {
        red[k * bs + tid] = lad.x.l[k]; red[(14 + k) * bs + tid] = lad.y.l[k]; red[(28 + k) * bs + tid] = lad.z.l[k];
    }
    red[42 * bs + tid] = lad_inf ? 1u : 0u;
}
H2V_DI void msm_reduce(G1J28 &lad, bool &lad_inf, uint32_t *red, const uint32_t lanes_per_proof, const bool in_block, const uint32_t gsub,
                       const uint32_t glen) {
    const uint32_t tid = threadIdx.x, bs = blockDim.x;
    msm_red_store(red, lad, lad_inf);
    __syncthreads();
    uint32_t top = 1;
    while (top < lanes_per_proof) top <<= 1;
    for (uint32_t s = top >> 1; s >= 1; s >>= 1) {
        if (in_block && gsub < s && gsub + s < glen) {
            if (red[42 * bs + tid + s] == 0) {
                G1J28 other;
#pragma unroll
                for (int k = 0; k < 14; k++) {
                    other.x.l[k] = red[k * bs + tid + s];
                    other.y.l[k] = red[(14 + k) * bs + tid + s];
                    other.z.l[k] = red[(28 + k) * bs + tid + s];
                }
                g1j28_acc_add(lad, lad_inf, other, false);   // complete: equal / opposite partial sums, infinity
                msm_red_store(red, lad, lad_inf);
            }
        }
        __syncthreads();
    }
}
// only the lane that ends up with a group's sum converts it back
H2V_DI void msm_write_sum(uint32_t *out, const uint32_t i, const G1J28 &lad, const bool lad_inf) {
    G1J acc;
    g1j28_to_g1j(acc, lad, lad_inf);
    g1j_store36(out + (size_t)i * 36, acc);
}

// A proof owns exactly LPT * n_terms consecutive lanes of a block (no power-of-two padding: 34 terms used to occupy
// 128 lanes); the block holds as many whole proofs as fit, the rest of its lanes idle.
//
// LPT = lanes per term.  2: one lane per GLV half (128 doublings + 33 additions per lane).
// 8: a QUAD per GLV half (h2v_curve28.hpp: quad-cooperative arithmetic): the four lanes hold the same accumulator and
// share the multiplications of every doubling (depth 3 instead of 7) and addition (6 instead of 11): 33 x (4 x 3 + 6) =
// 594 multiplications deep instead of 1287, on four times the lanes - for launches that leave most SIMDs idle anyway.
// Measured, it buys far less than the depth suggests: T = 16 x 64 proofs 1.35 -> 1.17 ms; T = 58 (464 lanes per proof: a
// 512-thread block, two waves per SIMD) 1.35 -> 1.69 ms; a quad per TERM (both halves, 780 deep, 256-thread blocks) 1.45-1.51
// ms, slower than two plain lanes per term.  A lone wave is bound by the latency of its dependent multiply-adds, and the one-lane
// formulas already overlap their independent multiplications (A = X^2, B = Y^2, ...) inside the lane; a level of the quad
// schedule is exactly one multiplication between two barriers (select, multiply, broadcast).  Kept as a forced shape
// (H2V_MSM_LPT=8, parity-tested), never chosen by the launcher: see msm_ladder_shape.
// 1: one lane runs both halves of its term on ONE accumulator, so the 128 doublings are shared (128 doublings + 66
// additions per lane, 36 % less work per proof, half the waves).  Measured on MI355X one wave per SIMD of this code
// already reaches 85 % of what two deliver (2048 proofs: 1.54 ms, 4096: 2.60 ms with LPT = 2), so whenever the batch
// still fills the SIMDs with one lane per term the smaller total wins; the launcher picks (h2v_capi.hip).
// FIX (with LPT = 1): a fixed-base launch over a range of VK-base terms.  The VK bases are the same for every proof, so
// ALL their window multiples [d] 16^w V (w = 0..64, d = 1..8) are precomputed at plan load and a VK term costs 65 mixed
// additions and no doubling; a lane sums fix_k of them (one accumulator per base - additions inside one base's sum
// cannot be exceptional, see below - merged with complete additions).  It runs beside the ladder launch of the
// per-proof terms (separate waves: one wave mixing the two kinds would execute them one after the other) and leaves
// fewer lanes per proof: for T >= 34 at 2048 proofs that brings the MSM back to one wave per SIMD.
template <int LPT, bool FIX = false, bool MADD_INL = false>
H2V_DI void msm_body(const H2vDevPlan &plan, const H2vMsmArgs &ma, uint32_t n, uint32_t per_block,
                     const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ pts, uint32_t *__restrict__ tabws,
                     uint32_t *red /* Jacobian partial sums, dword d of thread t at red[d*blockDim.x + t] */,
                     const uint32_t bid /* logical block: blockIdx.x, or the loop index of a conditional launch */) {
    static_assert(!FIX || LPT == 1, "fixed-base mode runs merged ladders");
    static_assert(LPT == 1 || LPT == 2 || LPT == 8, "one lane per term, one per GLV half, or a quad per GLV half");
    constexpr bool QUAD = LPT >= 4;                 // four lanes share one accumulator
    constexpr bool SPLIT = LPT == 2 || LPT == 8;    // one GLV half per lane (or quad); otherwise both halves on one accumulator
    constexpr int NH = SPLIT ? 1 : 2;               // GLV halves per accumulator
    const uint32_t tid = threadIdx.x;
    const uint32_t lanes_per_proof = FIX ? ma.n_fixl : LPT * ma.n_terms;
    const uint32_t seg = tid / lanes_per_proof;       // which of the block's proofs
    const uint32_t sub = tid - seg * lanes_per_proof; // position inside the proof's segment
    const bool fix_lane = FIX;   // a fixed-base launch has no ladder lanes (a wave mixing the two kinds would run them one after the other)
    const uint32_t term = FIX ? 0u : (LPT == 8 ? sub >> 3 : LPT == 2 ? sub >> 1 : sub), half = LPT == 8 ? (sub >> 2) & 1 : LPT == 2 ? sub & 1 : 0;
    const uint32_t i = bid * per_block + seg;
    const bool active = seg < per_block && i < n;
    // this lane's group: position and length of its reduction segment inside the proof's lanes
    const uint32_t grp = FIX ? 0u : (term < ma.grp_end[0] ? 0u : (term < ma.grp_end[1] ? 1u : 2u));
    const uint32_t g_lo = grp == 0 ? 0u : ma.grp_end[grp - 1];
    const uint32_t gsub = FIX ? sub : sub - LPT * g_lo, glen = FIX ? lanes_per_proof : LPT * (ma.grp_end[grp] - g_lo);
    // this lane's partial sum, on the lazily reduced field with an explicit infinity flag (h2v_curve28.hpp); idle
    // lanes and skipped terms contribute the point at infinity
    G1J28 lad;
    bool lad_inf = true;
    if (FIX && active && fix_lane) {
        // The accumulator of one base is [a]V with a = the signed-digit prefix read so far (most significant window first),
        // a multiple of B^(w+1), B = 2^c; adding [d B^w]V is exceptional iff a -+ d B^w = 0 mod r.  As integers |a -+ d B^w| <
        // 2^265, so that means a -+ d B^w = m r with |m| small: 0 is excluded by the digits' size (|d| <= B/2 < B) unless
        // a = d = 0, and m r is not = -+d B^w modulo B^(w+1) for w > 0 (r is odd: m r = 0 mod B^w needs B^w | m).  So the
        // additions of the windows w > 0 are unchecked.  For w = 0 the sum a + d_0 is the whole scalar (canonical, not 0: never
        // the inverse), but the DOUBLING case a = d_0 mod r is reachable: r = 1 mod 2^32, so the scalar r - 2 recodes to
        // d_0 = -1 with prefix a = r - 1, i.e. acc = -V and the entry added is -V (the one such scalar, for c = 4, 8 and 12 -
        // ADVICE r3).  The last window of a base therefore goes through the complete law (one addition in 22 .. 65); sums of
        // different bases meet in complete ones as well.
        const uint32_t f0 = sub * ma.fix_k;
#pragma unroll 1
        for (uint32_t j = 0; j < ma.fix_k; j++) {
            if (f0 + j >= ma.n_terms) break;
            const MsmTerm t = msm_term(plan, ma, scalars, pts, i, f0 + j, true);
            uint32_t any_b = 0, sc[8], any_s = 0;
#pragma unroll
            for (int k = 0; k < 24; k++) any_b |= t.base[k];
#pragma unroll
            for (int k = 0; k < 8; k++) { sc[k] = t.scal[k]; any_s |= sc[k]; }
            if (any_b == 0 || any_s == 0) continue;
            const uint32_t W = plan.fix_W, E = 1u << (plan.fix_c - 1);
            int16_t dg[65];
            msm_recode_c(dg, sc, plan.fix_c, W);
            G1J28 acc;
            bool acc_inf = true;
            const uint32_t *tabb = ma.fix_tab + (size_t)t.idx * W * E * 28;
#pragma unroll 1
            for (int q = (int)W - 1; q >= 0; q--) {
                const int d = dg[q];
                if (d == 0) continue;
                const uint32_t *ent = tabb + ((size_t)q * E + (uint32_t)((d < 0 ? -d : d) - 1)) * 28;
                F28 qx, qy;
#pragma unroll
                for (int k = 0; k < 14; k++) { qx.l[k] = ent[k]; qy.l[k] = ent[14 + k]; }
                if (acc_inf) msm_acc_start(acc, acc_inf, qx, qy, d < 0);
                else if (q == 0) msm_acc_add_affine(acc, acc_inf, qx, qy, d < 0);   // w = 0: complete (see above)
                else g1j28_madd_ladder(acc, acc, qx, qy, d < 0);
            }
            if (!acc_inf) g1j28_acc_add(lad, lad_inf, acc, false);   // complete
        }
    }
    if (active && !fix_lane) {
        const MsmTerm t = msm_term(plan, ma, scalars, pts, i, term);
        G1A base;
#pragma unroll
        for (int k = 0; k < 12; k++) { base.x.v[k] = t.base[k]; base.y.v[k] = t.base[12 + k]; }
        uint32_t s[8], k1[4], k2[4];
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = t.scal[k];
        glv_split(k1, k2, s);
        uint32_t any = 0;
        if (SPLIT) {
#pragma unroll
            for (int k = 0; k < 4; k++) any |= half ? k2[k] : k1[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) any |= k1[k] | k2[k];
        }
        if (!g1a_is_inf(base) && any != 0) {
            // signed 4-bit recoding, least significant digit first: digit = dg[h][q] in [-8, 8]
            int8_t dg[NH][33];
#pragma unroll
            for (int h = 0; h < NH; h++) {
                uint32_t kk[4];
#pragma unroll
                for (int k = 0; k < 4; k++) kk[k] = (SPLIT ? half != 0 : h != 0) ? k2[k] : k1[k];
                msm_recode4(dg[h], kk);
            }
            // table[m-1] = m*P (half 0) or m*phi(P) (half 1), m = 1..8, AFFINE (x, y: 2 x 14 limbs), 112 contiguous
            // bytes per entry, the two halves 224 dwords apart.  Normally it was built ahead of this kernel -
            // per-proof points by the decompression kernel (its square-root wave has the slack), VK bases at plan
            // load - and is only read here; the fold MSMs of the recursion path build theirs on the spot in a per-lane
            // slab of the workspace.  The multiples are affine (one inversion through Montgomery's trick) so that the
            // window additions are mixed ones.
            const uint32_t *tab;   // of this lane's first half
            if (ma.pt_tab) {
                tab = msm_term_tab(ma, t, i) + half * 224;
            } else if (SPLIT) {   // (the quad shapes are only launched with prebuilt tables)
                uint32_t *mine = tabws + (((size_t)i * ma.n_terms + term) * 2 + half) * 224;
                if (half) {  // phi(P)
                    Fp beta;
#pragma unroll
                    for (int k = 0; k < 12; k++) beta.v[k] = FP_BETA_GLV[k];
                    fp_mul(base.x, base.x, beta);
                }
                g1_build_window_table(mine, base);
                tab = mine;
            } else {
                uint32_t *mine = tabws + ((size_t)i * ma.n_terms + term) * 448;
                g1_build_window_tables_glv(mine, base);
                tab = mine;
            }
            // The ladder runs on the lazily reduced 28-bit field (h2v_fp28.hpp / h2v_curve28.hpp) and is only ever
            // touched by inlined code, so `lad` stays in VGPRs.
            //
            // Exceptional additions.  The accumulator is [a]P + [b]phi(P) = [a + b lambda]P with (a, b) the signed
            // prefixes read so far (not both zero once a digit was non-zero: a signed-digit prefix with a non-zero
            // leading digit is non-zero).  Adding [d]P (or [d]phi(P)) is exceptional iff (a -+ d, b) (or (a, b -+ d))
            // lies in the lattice {(u, v): u + v lambda = 0 mod r}, whose non-zero vectors are longer than 2^126
            // (reduced basis (lambda, -1), (1, lambda + 1), lambda = x^2 - 1 > 2^127).  With one half per lane b = 0
            // and a < 2^129 < r: never.  With both halves on one lane the prefixes stay below 2^(4 (33 - q)) + 8 in
            // window q, so windows q >= 2 are safe and only the last two take the complete addition.
#pragma unroll 1
            for (int q = 32; q >= 0; q--) {
                if (q != 32 && !lad_inf) {
                    if (QUAD) g1j28_dbl_n_coop3(lad, 4);   // the quad's lanes share the multiplications of a doubling: depth 3 instead of 7
                    else {
#pragma unroll 1
                        for (int rep = 0; rep < 4; rep++) g1j28_dbl_t<true>(lad, lad);   // multiplier inlined: no argument marshalling
                    }
                }
#pragma unroll 1
                for (int h = 0; h < NH; h++) {
                    const int d = dg[h][q];
                    if (d == 0) continue;
                    const uint32_t *ent = tab + h * 224 + ((d < 0 ? -d : d) - 1) * 28;
                    F28 qx, qy;
#pragma unroll
                    for (int k = 0; k < 14; k++) { qx.l[k] = ent[k]; qy.l[k] = ent[14 + k]; }
                    if (lad_inf) msm_acc_start(lad, lad_inf, qx, qy, d < 0);
                    else if (QUAD && (SPLIT || q >= 2)) g1j28_madd_quad(lad, qx, qy, d < 0);   // never exceptional (above); depth 6 instead of 11
                    else if (SPLIT || q >= 2) g1j28_madd_ladder_t<MADD_INL>(lad, lad, qx, qy, d < 0);   // never an exceptional case (above)
                    else msm_acc_add_affine(lad, lad_inf, qx, qy, d < 0);
                }
            }
        }
    }
    if (QUAD && (sub & 3) != 0) lad_inf = true;   // the quad's four lanes hold the same sum: its first lane carries it
    msm_reduce(lad, lad_inf, red, lanes_per_proof, seg < per_block, gsub, glen);
    if (gsub == 0 && seg < per_block && i < n) msm_write_sum(grp == 0 ? ma.out[0] : (grp == 1 ? ma.out[1] : ma.out[2]), i, lad, lad_inf);
}

// ---------------------------------------------------------------------------- segmented per-proof MSM
// A sum whose LPT x T lanes do not fit one block (or that the launcher's cost model prefers to cut: T > 64 only) is cut into
// S segments of Ts terms, segment s = terms [s Ts, min((s + 1) Ts, T)) of the range, one segment per blockIdx.y.  Each block
// runs the unchanged msm_body over its segment and writes the segment's sum to parts[s][proof][36] (Jacobian, proof stride n);
// k_g1_sum_segments then folds the S partial sums of every proof in a second launch on the same stream: blocks of one launch
// never exchange data.  Single-group ranges with prebuilt window tables only (the launcher guarantees both): the per-lane
// table slabs of `tabws` are numbered by the range's own terms.
H2V_DI H2vMsmArgs msm_segment_args(const H2vMsmArgs &ma, uint32_t seg_terms, uint32_t s, uint32_t n, uint32_t *parts) {
    H2vMsmArgs a = ma;
    const uint32_t lo = s * seg_terms, hi = lo + seg_terms < ma.n_terms ? lo + seg_terms : ma.n_terms;
    a.term_base = ma.term_base + lo;
    a.scal_col_base = ma.scal_col_base + lo;
    a.n_terms = hi - lo;
    a.grp_end[0] = a.grp_end[1] = a.grp_end[2] = hi - lo;
    uint32_t *o = parts + (size_t)s * n * 36;
    a.out[0] = a.out[1] = a.out[2] = o;
    return a;
}
// COND: the same ladders as the fall-back of the RLC batch mode: they return at once when the batch check passed.  (Separate
// entry points: the check costs the parity path's kernels nothing, not even a different register allocation.)  The grid
// is small and walks the logical blocks in a loop: a launch that only has to find out that it is not needed should not
// cost a thousand workgroup dispatches (40-50 us per skipped kernel on the RLC mode's critical path before).
// skip[1 + g] != 0: group g (proofs 64 g .. 64 g + 63) passed its own check after the batch check failed (k_pairing_rlc_groups)
// and needs no per-proof verdicts; a logical block is skipped when every group it touches passed
H2V_DI bool msm_groups_passed(const uint32_t *__restrict__ skip, uint32_t bid, uint32_t per_block, uint32_t n) {
    const uint32_t p0 = bid * per_block, p1 = (p0 + per_block < n ? p0 + per_block : n) - 1;
    bool all = true;
    for (uint32_t g = p0 >> 6; g <= (p1 >> 6); g++) all = all && skip[1 + g] != 0;
    return all;
}
// The four unconditional ladder entry points: LPT 2 (k_g1_msm) or 1 (_merged); SEG: one segment of the range per blockIdx.y
// (_seg; seg_terms and parts are read by these only).
template <int LPT, bool SEG>
H2V_DI void msm_ladder_entry(const H2vDevPlan &plan, const H2vMsmArgs &ma, uint32_t n, uint32_t per_block, uint32_t seg_terms, uint32_t *__restrict__ parts,
                             const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ pts, uint32_t *__restrict__ tabws) {
    extern __shared__ uint32_t red[];
    // (the unsegmented forms run on the kernel's own argument, not on a copy of it)
    if (SEG) msm_body<LPT, false, true>(plan, msm_segment_args(ma, seg_terms, blockIdx.y, n, parts), n, per_block, scalars, pts, tabws, red, blockIdx.x);
    else msm_body<LPT, false, true>(plan, ma, n, per_block, scalars, pts, tabws, red, blockIdx.x);
}
// ... and the body of the four conditional ones, the walk over the logical blocks.  PRE; declares what A names (the segment's
// arguments).  A macro on purpose: as a COND flag of the template above the same text compiled k_g1_msm_merged_cond to another
// register allocation (248 instead of 251 VGPRs, 54 more SGPR spill moves); expanded in the kernel it compiles as it always has.
#define MSM_COND_BODY(LPT, PRE, A)                                                                       \
    {                                                                                                    \
        extern __shared__ uint32_t red[];                                                                \
        if (ma.skip[0]) return; /* (uniform over the launch: before any barrier) */                      \
        PRE;                                                                                             \
        const uint32_t n_blocks = (n + per_block - 1) / per_block;                                       \
        for (uint32_t bid = blockIdx.x; bid < n_blocks; bid += gridDim.x) {                              \
            if (msm_groups_passed(ma.skip, bid, per_block, n)) continue; /* (uniform over the block) */  \
            msm_body<LPT, false, true>(plan, A, n, per_block, scalars, pts, tabws, red, bid);            \
            __syncthreads();                                                                             \
        }                                                                                                \
    }
#define MSM_ARGS H2vDevPlan plan, H2vMsmArgs ma, uint32_t n, uint32_t per_block /* proofs per block */
#define MSM_BUFS const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ pts, uint32_t *__restrict__ tabws
#define MSM_SEG_ARGS MSM_ARGS, uint32_t seg_terms, uint32_t *__restrict__ parts
#define MSM_SEG_PRE const H2vMsmArgs sa = msm_segment_args(ma, seg_terms, blockIdx.y, n, parts)
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm(MSM_ARGS, MSM_BUFS) { msm_ladder_entry<2, false>(plan, ma, n, per_block, 0, nullptr, scalars, pts, tabws); }
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_merged(MSM_ARGS, MSM_BUFS) { msm_ladder_entry<1, false>(plan, ma, n, per_block, 0, nullptr, scalars, pts, tabws); }
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_cond(MSM_ARGS, MSM_BUFS) MSM_COND_BODY(2, , ma)
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_merged_cond(MSM_ARGS, MSM_BUFS) MSM_COND_BODY(1, , ma)
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_seg(MSM_SEG_ARGS, MSM_BUFS) { msm_ladder_entry<2, true>(plan, ma, n, per_block, seg_terms, parts, scalars, pts, tabws); }
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_merged_seg(MSM_SEG_ARGS, MSM_BUFS) { msm_ladder_entry<1, true>(plan, ma, n, per_block, seg_terms, parts, scalars, pts, tabws); }
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_cond_seg(MSM_SEG_ARGS, MSM_BUFS) MSM_COND_BODY(2, MSM_SEG_PRE, sa)
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_merged_cond_seg(MSM_SEG_ARGS, MSM_BUFS) MSM_COND_BODY(1, MSM_SEG_PRE, sa)
#undef MSM_SEG_PRE
#undef MSM_COND_BODY
#undef MSM_SEG_ARGS
// the quad and the fixed-base form: plain launches only
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_quad(MSM_ARGS, MSM_BUFS) {
    extern __shared__ uint32_t red[];
    msm_body<8, false, true>(plan, ma, n, per_block, scalars, pts, tabws, red, blockIdx.x);
}
extern "C" __global__ void __launch_bounds__(512, 2) k_g1_msm_fixed(MSM_ARGS, MSM_BUFS) {
    extern __shared__ uint32_t red[];
    msm_body<1, true>(plan, ma, n, per_block, scalars, pts, tabws, red, blockIdx.x);
}


// Several GLV halves per lane (H = 4 .. 8: two to four terms): the halves a lane carries share ONE accumulator and therefore the
// 128 doublings - per lane 128 doublings + 33 H mixed additions instead of one ladder per half (H = 4: 26 % fewer multiply-adds
// per proof, H = 8: 39 %), on 2 / H of the waves with a chain (128 x 7 + 33 H x 11) / 1622 as long.  It loses when the launch
// is alone on the chip (half or a quarter of the SIMDs get a wave) and wins when other kernels fill them: several steps in
// flight, where the step time is the instruction count.  Non-recursive plans with prebuilt tables.
// The proof's 2 T halves are dealt out H per lane in order (half hh = 2 term + glv half): lanes of one proof differ by at most
// the last one's load, and no lane waits through addition slots of halves it does not have - with whole terms per lane ten terms
// on four lanes were 3 + 3 + 3 + 1 and every wave ran six addition slots per window for five halves per lane on average.
// One accumulator over DIFFERENT points has no lattice argument against exceptional additions (crafted proofs can make
// P_2 = [m] P_1), so the ladder runs unchecked and is judged once at the end: an exceptional addition or doubling leaves
// Z = 0, which every later Z inherits; such a lane (never an honest one) redoes its ladder with the complete group law.
// (MSM_MAX_HALVES: h2v_msm_shape.hpp, where host code sees the bound)
template <bool COMPLETE>
H2V_DN void msm_multi_ladder(G1J28 &out, bool &out_inf, const int8_t (&dg)[MSM_MAX_HALVES][33], const uint32_t *const (&tab)[MSM_MAX_HALVES], const int H) {
    G1J28 lad;
    bool lad_inf = true;
    // The table entry of the NEXT addition slot is fetched one slot ahead (round 4): a slot's entry is a scattered 112-byte read
    // out of a 73 MB table whose address hangs on a digit in private memory - two dependent round trips (~2 k cycles) in front of
    // every 11-multiplication addition otherwise.  The first slot of the next window is fetched across the four doublings.
    F28 nx, ny;
    int nd;
    auto fetch = [&](const int q, const int h) {
        nd = dg[h][q];
        const int e = nd < 0 ? -nd : nd;
        const uint32_t *ent = tab[h] + (e ? e - 1 : 0) * 28;      // (a zero digit reads entry 0 and does not use it)
#pragma unroll
        for (int k = 0; k < 14; k++) { nx.l[k] = ent[k]; ny.l[k] = ent[14 + k]; }
    };
    fetch(32, 0);
#pragma unroll 1
    for (int q = 32; q >= 0; q--) {
        if (q != 32 && !lad_inf) {
#pragma unroll 1
            for (int rep = 0; rep < 4; rep++) g1j28_dbl_t<true>(lad, lad);
        }
#pragma unroll 1
        for (int h = 0; h < H; h++) {
            const F28 qx = nx, qy = ny;
            const int d = nd;
            if (h + 1 < H) fetch(q, h + 1);
            else if (q > 0) fetch(q - 1, 0);
            if (d == 0) continue;
            if (lad_inf) {
                        lad.x = qx;
                        lad.y = qy;
                        if (d < 0) { F28_NEG(lad.y, qy, 3, 1); f28_carry(lad.y); }
                        f28_set_one(lad.z);
                        lad_inf = false;
                    } else if (!COMPLETE) {
                g1j28_madd_ladder_t<true>(lad, lad, qx, qy, d < 0);
            } else {
                        G1J28 o;
                        o.x = qx; o.y = qy;
                        f28_set_one(o.z);
                        g1j28_acc_add(lad, lad_inf, o, d < 0);
                    }
        }
    }
    out = lad;
    out_inf = lad_inf;
}
H2V_DI void msm_multi_body(const H2vDevPlan &plan, const H2vMsmArgs &ma, uint32_t n, uint32_t per_block, const uint32_t H,
                           const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ pts, uint32_t *red) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lanes_per_proof = (2 * ma.n_terms + H - 1) / H;
    const uint32_t seg = tid / lanes_per_proof, sub = tid - seg * lanes_per_proof;
    const uint32_t i = blockIdx.x * per_block + seg;
    const bool active = seg < per_block && i < n;
    G1J28 lad;
    bool lad_inf = true;
    if (active) {
        int8_t dg[MSM_MAX_HALVES][33];
        const uint32_t *tab[MSM_MAX_HALVES];
#pragma unroll 1
        for (uint32_t j = 0; j < H; j++) {
            const uint32_t hh = sub * H + j, term = hh >> 1, h = hh & 1;
            bool use = term < ma.n_terms;
            const MsmTerm t = msm_term(plan, ma, scalars, pts, i, use ? term : 0u);
            uint32_t any_b = 0, s[8], any_s = 0;
#pragma unroll
            for (int k = 0; k < 24; k++) any_b |= t.base[k];
#pragma unroll
            for (int k = 0; k < 8; k++) { s[k] = t.scal[k]; any_s |= s[k]; }
            use = use && any_b != 0 && any_s != 0;       // the point at infinity / a zero scalar contribute nothing
            uint32_t k1[4], k2[4];
            glv_split(k1, k2, s);                        // (a term whose halves sit in two lanes is split in both)
            tab[j] = msm_term_tab(ma, t, i) + h * 224;
            msm_recode4(dg[j], h ? k2 : k1, use);
        }
        msm_multi_ladder<false>(lad, lad_inf, dg, tab, (int)H);
        if (!lad_inf) {
            Fp zc;
            F28 z = lad.z;
            f28_carry(z);
            f28_to_fp(zc, z);
            if (fp_is_zero(zc)) msm_multi_ladder<true>(lad, lad_inf, dg, tab, (int)H);   // crafted points only
        }
    }
    // reduction over the lanes of each proof (as in msm_body: lazy field, complete additions)
    msm_reduce(lad, lad_inf, red, lanes_per_proof, seg < per_block, sub, lanes_per_proof);
    if (sub == 0 && seg < per_block && i < n) msm_write_sum(ma.out[0], i, lad, lad_inf);
}
extern "C" __global__ void __launch_bounds__(256, 2) k_g1_msm_multi(MSM_ARGS, uint32_t halves_per_lane, MSM_BUFS) {
    extern __shared__ uint32_t red[];
    (void)tabws;
    msm_multi_body(plan, ma, n, per_block, halves_per_lane, scalars, pts, red);
}
#undef MSM_ARGS
#undef MSM_BUFS

// er += er_fix (complete Jacobian addition, one lane per proof): joins the two launches of a split MSM
extern "C" __global__ void __launch_bounds__(64)
k_g1_sum_pairs(uint32_t n, uint32_t *__restrict__ er, const uint32_t *__restrict__ er_fix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1J a, b, r;
    g1j_load36(a, er + (size_t)i * 36);
    g1j_load36(b, er_fix + (size_t)i * 36);
    g1j_add(r, a, b);
    g1j_store36(er + (size_t)i * 36, r);
}
// out[i] = sum_s parts[s][i] with the complete law (one lane per proof, 64-lane blocks): a crafted proof can make two segment
// sums equal, opposite or the point at infinity.  skip (RLC fall-back, else NULL): the batch check passed (skip[0]) or this
// block's 64 proofs - exactly one group of the check (skip[1 + g]) - passed their group check, and nothing reads their sums.
extern "C" __global__ void __launch_bounds__(64)
k_g1_sum_segments(uint32_t n, uint32_t S, const uint32_t *__restrict__ parts, uint32_t *__restrict__ out, const uint32_t *__restrict__ skip) {
    if (skip && (skip[0] || skip[1 + blockIdx.x])) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1J acc, b, r;
    g1j_load36(acc, parts + (size_t)i * 36);
#pragma unroll 1
    for (uint32_t s = 1; s < S; s++) {
        g1j_load36(b, parts + ((size_t)s * n + i) * 36);
        g1j_add(r, acc, b);
        acc = r;
    }
    g1j_store36(out + (size_t)i * 36, acc);
}
