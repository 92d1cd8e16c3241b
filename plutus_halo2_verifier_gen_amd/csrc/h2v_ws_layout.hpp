// Workspace memory: what every buffer set of a workspace holds and how large each buffer is.  HOST CODE ONLY - no HIP call and no
// HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_ws_layout.cpp): every function
// is pure arithmetic on sizes.  h2v_capi.hip allocates each set row by row through its Owner - every buffer an allocation of its
// own, in the order of the table - and h2v_probe_device_memory counts what is live, so a test can hold the two against each other.
//
// A set is a Table: rows {name, bytes, fill}, indexed by the set's enum.  A row of 0 bytes is a buffer this shape does not have.
// THE SLACK RULES are stated here once: a block that grows on demand takes a quarter more than was asked for (grown); the fold
// form's term pool does the same, capped at H2V_MIXED_FOLD_MAX_TERMS terms, and never shrinks (fold_caps).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "h2v_mixed_fold.hpp"
#include "h2v_msm_shape.hpp"
#include "h2v_pip_sizes.hpp"
#include "h2v_plan.h"

namespace wslayout {
// the records that more than one set holds
constexpr size_t JAC_DW = 36, JAC_BYTES = JAC_DW * 4;      // a Jacobian sum (er, el, the accumulator sums, a segment's partial sum)
constexpr size_t AFF_BYTES = 96;                           // an affine point: 24 dwords
constexpr size_t TAB_BYTES = 448 * 4;                      // the window table of one point: [1..8]P and [1..8]phi(P), 2 x 14 x 28-bit limbs
constexpr size_t PAIR_BYTES = 48 * 4;                      // a two-slot record (L, R) of affine points
constexpr size_t FR_BYTES = 32, CI_BYTES = 48;
constexpr uint32_t RING = 64, NEV = 12;                    // h2v_workspace::RING call records of NEV events each

enum Fill : int { NONE = -1, ZERO = 0, ONES = 1 };
struct Row { const char *name; size_t bytes; Fill fill; };
template <int N> struct Table {
    static constexpr int n = N;
    Row row[N];
    size_t total() const { size_t s = 0; for (const Row &r : row) s += r.bytes; return s; }
    uint32_t blocks() const { uint32_t c = 0; for (const Row &r : row) c += r.bytes != 0; return c; }
};
static inline size_t grown(size_t need) { return need + need / 4; }

// ---- the shape a workspace is sized for: a plan fits iff each of its values is <= the workspace's
struct Shape {
    uint32_t terms = 0, main_terms = 0, slots = 0;
    uint32_t regs = 0;         // registers of a combiner that keeps its register file in global memory; 0: the file lives in LDS
    uint32_t trace = 0;
    bool ivc = false, fix = false;
    uint32_t width = 0;        // the widest MSM sum
    uint32_t segs = 0;         // msm_max_segments(width): the partial sums of a segmented MSM
};
// Proofs per block of the transcript + combiner launch with the register file in LDS: a block is one wave, its 64 lanes are P
// proofs x L lanes per proof.  A single-lane plan whose register file does not fit 64 proofs runs 32 / 16 / 8 per block; 0: below
// 8, the register file goes to the workspace's global buffer.
static inline uint32_t vm_lds_slots(const H2vDevPlan &d) {
    if (d.vm_lanes > 1) return 64 / d.vm_lanes;   // validated at load: fits
    uint32_t P = 64;
    while (P >= 8 && !vm_fits_lds(d.n_regs, 64 / P)) P >>= 1;
    return P >= 8 ? P : 0;
}
// the widest sum of a plan: the proof's own MSM; with recursion also acc_right + the fixed bases
static inline uint32_t msm_sum_width(const H2vDevPlan &d) {
    const uint32_t f = d.ivc && d.n_terms > d.n_main_terms + 1 ? d.n_terms - d.n_main_terms - 1 : 0;
    return d.n_main_terms > f ? d.n_main_terms : f;
}
static inline Shape shape_of(const H2vDevPlan &d, bool with_trace) {
    Shape s;
    s.terms = d.n_terms; s.main_terms = d.n_main_terms; s.slots = (uint32_t)H2V_SLOTS(d);
    s.regs = vm_lds_slots(d) == 0 ? d.n_regs : 0;
    s.trace = with_trace ? d.n_trace : 0;
    s.ivc = d.ivc != 0; s.fix = d.fix_tab != nullptr;
    s.width = msm_sum_width(d); s.segs = msm_max_segments(s.width);
    return s;
}
// the smallest shape that both fit (h2v_workspace_create_multi)
static inline Shape shape_union(const Shape &a, const Shape &b) {
    auto mx = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
    Shape u;
    u.terms = mx(a.terms, b.terms); u.main_terms = mx(a.main_terms, b.main_terms); u.slots = mx(a.slots, b.slots);
    u.regs = mx(a.regs, b.regs); u.trace = mx(a.trace, b.trace);
    u.ivc = a.ivc || b.ivc; u.fix = a.fix || b.fix;
    u.width = mx(a.width, b.width); u.segs = mx(a.segs, b.segs);
    return u;
}
// Why a plan of shape p (shape_of(d, true): its trace counts only when the call wants one) does not fit a workspace of shape w, in
// the order the checks have always had
enum class Fit { OK, SMALLER_PLAN, REGISTER_FILE, NOT_RECURSIVE, NO_FIXED_SUM, NARROWER_SUMS, NO_TRACE };
static inline Fit fits(const Shape &w, const Shape &p, bool want_trace) {
    if (p.terms > w.terms || p.slots > w.slots) return Fit::SMALLER_PLAN;
    if (p.regs > w.regs) return Fit::REGISTER_FILE;
    if (p.ivc && !w.ivc) return Fit::NOT_RECURSIVE;
    if (p.fix && !w.fix) return Fit::NO_FIXED_SUM;
    if (p.segs > w.segs) return Fit::NARROWER_SUMS;
    if (want_trace && p.trace > w.trace) return Fit::NO_TRACE;
    return Fit::OK;
}
static inline const char *fit_message(Fit f) {
    switch (f) {
    case Fit::SMALLER_PLAN: return "workspace was created for a smaller plan (MSM terms / point slots)";
    case Fit::REGISTER_FILE: return "workspace has no (or too small a) global register file for this plan";
    case Fit::NOT_RECURSIVE: return "workspace was created for a non-recursive plan";
    case Fit::NO_FIXED_SUM: return "workspace lacks the fixed-base sum buffer of this plan";
    case Fit::NARROWER_SUMS: return "workspace was created for a plan with narrower MSM sums (no room for the partial sums of a segmented MSM)";
    case Fit::NO_TRACE: return "workspace has no trace buffer for this plan";
    default: return "";
    }
}

// ---- the pipeline buffers of a workspace (or of a lane) of `cap` proofs; with them 5 untimed events and RING x NEV timed ones
enum Pipe { P_REGS, P_SCALARS, P_PTS, P_VALID, P_VALID_SUB, P_DEC_CTR, P_ER_FIX, P_MSM_PARTS, P_ER, P_PT_TAB, P_MSM_TAB, P_STATUS, P_ACCEPT,
            P_TRACE, P_ACCL, P_ACCR, P_EL2, P_ER2, P_FOLD_PTS, P_FOLD_SCAL, P_COUNT };
constexpr uint32_t PIPE_EVENTS = 5 + RING * NEV;
static inline Table<P_COUNT> pipeline(const Shape &s, uint64_t cap) {
    const size_t n = (size_t)cap, stride = (n + 63) / 64 * 64, ivc = s.ivc ? n : 0;
    return {{{"regs", (size_t)s.regs * 8 * stride * 4, NONE},                 // 0: the register file lives in LDS
             {"scalars", n * s.terms * FR_BYTES, NONE},
             {"pts", n * s.slots * AFF_BYTES, NONE},
             {"valid", n * s.slots, NONE},
             {"valid_sub", n * s.slots, NONE},
             {"dec_ctr", 4, NONE},
             {"er_fix", s.fix ? n * JAC_BYTES : 0, NONE},
             {"msm_parts", n * s.segs * JAC_BYTES, NONE},
             {"er", n * JAC_BYTES, NONE},
             {"pt_tab", n * s.slots * TAB_BYTES, NONE},
             {"msm_tab", ivc * 4 * 2 * 8 * 112, NONE},                        // fold MSMs build their four tables on the spot
             {"status", n * 4, NONE},
             {"accept", n, NONE},
             {"trace", n * s.trace * FR_BYTES, NONE},
             {"accl", ivc * JAC_BYTES, NONE},
             {"accr", ivc * JAC_BYTES, NONE},
             {"el2", ivc * JAC_BYTES, NONE},
             {"er2", ivc * JAC_BYTES, NONE},
             {"fold_pts", ivc * 4 * AFF_BYTES, NONE},
             {"fold_scal", ivc * 4 * FR_BYTES, NONE}}};
}
// a laned workspace itself: accept[] of the largest call and one untimed event; per lane one more event and a pipeline set of `chunk`
static inline size_t laned_accept(uint64_t cap) { return (size_t)cap; }

// ---- one bucket MSM over at most cap_n terms of `halves` scalar halves (h2v_pippenger.hpp)
enum Pip { B_PTS28, B_DIG, B_LIST, B_CNT, B_OFF, B_ORDER, B_CLS, B_PARTIAL, B_WSUM, B_COUNT };
static inline Table<B_COUNT> bucket_msm(uint32_t cap_n, uint32_t halves) {
    const size_t nbmax = (size_t)PIP_MAX_W * (1u << (PIP_MAX_C - 1));
    const size_t ent = (size_t)cap_n * halves * PIP_MAX_W;
    return {{{"pts28", (size_t)(cap_n ? cap_n : 1) * PIP_PT_DW * 4, NONE},
             {"dig", (ent ? ent : 1) * 2, NONE},
             {"list", (ent ? ent : 1) * 4, NONE},
             {"cnt", nbmax * 4, NONE},
             {"off", (nbmax + 1) * 4, NONE},
             {"order", nbmax * 4, NONE},
             {"cls", PIP_CLS_DW * 4, NONE},
             {"partial", nbmax * PIP_PART_DW * 4, NONE},
             {"wsum", (size_t)PIP_MAX_W * PIP_PART_DW * 4, NONE}}};
}

// ---- the RLC set, in its three shapes.  A plan: n_var per-proof terms and n_fix VK-base terms.  Pairs (n_fix == 0): one variable
// term per pair, 128-bit scalars, ONE scalar array for both sums (no l_scal of its own).  The fold form of a mixed call: cap_t
// term records and cap_p block sums by the call's layout (fold_caps), no index arrays, and the copied points of the terms.
// R.cap_n / R.halves and L.cap_n: the two bucket-MSM sets that follow the rows (bucket_msm).
enum Rlc { R_R_SCAL, R_R_IDX, R_L_SCAL, R_L_IDX, R_VK_PART, R_GOOD, R_SUMS, R_MISC, R_FLAGS, R_FOLD_RPTS, R_FOLD_LPTS, R_COUNT };
struct RlcSet {
    Table<R_COUNT> t;
    uint32_t r_cap_n, r_halves, l_cap_n;
    size_t total() const { return t.total() + bucket_msm(r_cap_n, r_halves).total() + bucket_msm(l_cap_n, 1).total(); }
    uint32_t blocks() const { return t.blocks() + 2 * B_COUNT; }
};
static inline RlcSet rlc_rows(size_t cap, size_t r_terms, size_t r_idx, size_t l_scal, size_t l_idx, size_t parts, size_t rpts, size_t lpts, uint32_t halves) {
    const size_t blocks = (cap + 63) / 64;
    return {{{{"r_scal", r_terms * FR_BYTES, NONE},
              {"r_idx", r_idx * 4, NONE},
              {"l_scal", l_scal * FR_BYTES, NONE},
              {"l_idx", l_idx * 4, NONE},
              {"vk_part", parts * FR_BYTES, NONE},
              {"good", cap, NONE},
              {"sums", 2 * JAC_BYTES, NONE},                   // er then el: the two MSM results
              {"misc", 32 * 4, ZERO},
              {"flags", (blocks + 2) * 4, ZERO},
              {"fold_rpts", rpts * AFF_BYTES, NONE},
              {"fold_lpts", lpts * AFF_BYTES, NONE}}},
            (uint32_t)r_terms, halves, (uint32_t)cap};
}
static inline RlcSet rlc_plan(uint64_t cap, uint32_t n_var, uint32_t n_fix) {
    const size_t n = (size_t)cap, nr = n * n_var + n_fix, blocks = (n + 63) / 64;
    const bool pairs = n_fix == 0;
    return rlc_rows(n, nr, nr, pairs ? 0 : n, n, blocks * (n_fix ? n_fix : 1), 0, 0, pairs ? 1 : 2);
}
static inline RlcSet rlc_pairs(uint64_t cap) { return rlc_plan(cap, 1, 0); }
static inline size_t rlc_pair_pool(uint64_t cap) { return (size_t)cap * PAIR_BYTES; }     // the folded pairs' own pool (H2V_RLC_FOLD_PAIRS)
static inline RlcSet rlc_fold(uint64_t cap, size_t cap_t, size_t cap_p) { return rlc_rows((size_t)cap, cap_t, 0, (size_t)cap, 0, cap_p, cap_t, (size_t)cap, 2); }
// the fold pool's capacities for a call that needs need_t terms and need_p block sums on a pool that has have_t / have_p
struct FoldCaps { size_t terms, parts; };
static inline FoldCaps fold_caps(size_t need_t, size_t need_p, size_t have_t, size_t have_p) {
    FoldCaps c = {grown(need_t), grown(need_p) + 1};
    if (c.terms > H2V_MIXED_FOLD_MAX_TERMS) c.terms = (size_t)H2V_MIXED_FOLD_MAX_TERMS;
    if (c.terms < have_t) c.terms = have_t;
    if (c.parts < have_p) c.parts = have_p;
    return c;
}

// ---- the group stage of the RLC fall-back: G groups of 64 proofs, `stride` right-hand terms per group, every group two small
// bucket MSMs with GRP_C-bit windows whose buffers are carved out of ONE pool (group_pool).  With every (re)built argument array
// goes one pinned copy of it (group_args_bytes).
constexpr uint32_t GRP_C = 7, GRP_W = 128 / GRP_C + 1, GRP_NB = 1u << (GRP_C - 1);
enum Grp { G_SCAL, G_IDX, G_ER, G_EL, G_PTS, G_STATUS, G_VALID, G_ACCEPT, G_POOL, G_ARGS, G_COUNT };
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
// Where the buffers of bucket MSM (group q, side) lie in the pool: side 0 is the group's right-hand sum (`stride` terms of
// `halves` scalar halves), side 1 its left-hand sum (64 terms, one half).  The counters of all 2 G problems come first (cnt_bytes:
// one memset zeroes them), then per problem pts28, dig, list, off, order, cls, partial, wsum, each at a multiple of 256.
// total is sized for TWO halves on the right whatever `halves` is: the pairs shape (one half) leaves part of it unused, and the
// allocation stays what it has always been.
struct GroupPool {
    uint32_t G, stride, halves;
    size_t cnt_bytes, per_r, per_l, total;
    struct At { size_t cnt, pts28, dig, list, off, order, cls, partial, wsum, end; };
    static size_t span(size_t cap_n, size_t h) {
        const size_t nb = (size_t)GRP_W * GRP_NB;
        return up256(cap_n * PIP_PT_DW * 4) + up256(cap_n * h * GRP_W * 2) + up256(cap_n * h * GRP_W * 4) + up256((nb + 1) * 4) + up256(nb * 4) +
               up256(PIP_CLS_DW * 4) + up256(nb * PIP_PART_DW * 4) + up256((size_t)GRP_W * PIP_PART_DW * 4);
    }
    At at(uint32_t q, int side) const {
        const size_t nb = (size_t)GRP_W * GRP_NB, cap_n = side == 0 ? stride : 64, h = side == 0 ? halves : 1;
        At a;
        a.cnt = (size_t)(2 * q + side) * up256(nb * 4);
        a.pts28 = cnt_bytes + (size_t)q * (per_r + per_l) + (side ? per_r : 0);
        a.dig = a.pts28 + up256(cap_n * PIP_PT_DW * 4);
        a.list = a.dig + up256(cap_n * h * GRP_W * 2);
        a.off = a.list + up256(cap_n * h * GRP_W * 4);
        a.order = a.off + up256((nb + 1) * 4);
        a.cls = a.order + up256(nb * 4);
        a.partial = a.cls + up256(PIP_CLS_DW * 4);
        a.wsum = a.partial + up256(nb * PIP_PART_DW * 4);
        a.end = a.wsum + up256((size_t)GRP_W * PIP_PART_DW * 4);
        return a;
    }
};
static inline GroupPool group_pool(uint32_t G, uint32_t stride, uint32_t halves) {
    GroupPool p = {G, stride, halves, 0, 0, 0, 0};
    p.cnt_bytes = (size_t)2 * G * up256((size_t)GRP_W * GRP_NB * 4);
    p.per_r = GroupPool::span(stride, halves); p.per_l = GroupPool::span(64, 1);
    p.total = p.cnt_bytes + (size_t)G * (GroupPool::span(stride, 2) + p.per_l);
    return p;
}
static inline Table<G_COUNT> group_stage(uint32_t G, uint32_t stride) {
    const size_t g = G;
    return {{{"g_scal", g * stride * FR_BYTES, NONE},
             {"g_idx", g * stride * 4, NONE},
             {"er_g", g * JAC_BYTES, NONE},
             {"el_g", g * JAC_BYTES, NONE},
             {"pts_g", g * AFF_BYTES, ZERO},
             {"status_g", g * 4, NONE},
             {"valid_g", g, ONES},
             {"accept_g", g, NONE},
             {"pool", group_pool(G, stride, 2).total, NONE},
             {"args_d", 2 * g * PIP_ARGS_BYTES, NONE}}};
}
static inline size_t group_args_bytes(uint32_t G) { return (size_t)2 * G * PIP_ARGS_BYTES; }   // the pinned copy

// ---- the base buffers of the mixed-key calls (with them the 4 untimed events of the table slots); the grouped staging and the
// table slots grow on demand (grown)
enum Mixed { M_POOL, M_STATUS, M_GOOD, M_ONES, M_COUNT };
constexpr uint32_t MIXED_EVENTS = 4;
static inline Table<M_COUNT> mixed_base(uint64_t cap) {
    const size_t n = (size_t)cap;
    return {{{"pool", n * PAIR_BYTES, NONE}, {"status", n * 4, NONE}, {"good", n, NONE}, {"ones", n * 2, ONES}}};
}

// ---- a lane's staging of coalesced calls: cap = the lane's chunk; the proof and instance blocks only ever grow
enum Co { C_PROOFS, C_INST, C_CI, C_ACCEPT, C_FAIL, C_STATUS, C_COUNT };
static inline size_t co_proof_bytes(uint32_t cap, uint32_t proof_len) { return (size_t)cap * proof_len + 64; }
static inline size_t co_inst_bytes(uint32_t cap, uint32_t n_pi) { return (size_t)cap * (n_pi ? n_pi : 1) * FR_BYTES; }
static inline Table<C_COUNT> coalesce(uint32_t cap, size_t proof_bytes, size_t inst_bytes) {
    const size_t n = cap;
    return {{{"proofs", proof_bytes, NONE},
             {"inst", inst_bytes, NONE},
             {"ci", n * CI_BYTES, NONE},
             {"accept", n, NONE},
             {"fail", (n + 2) * 8, NONE},             // the group's verdict word, and behind it off[0 .. cap]
             {"status", n * 4, NONE}}};
}

// ---- the small sets.  The pair view of a check call; the routing counters and verdict words of the RLC calls (h_rlc_stats is
// pinned host memory); the ring of derived seeds (its digest buffer grows on demand: grown(32 x the tree's extent))
enum PairView { V_PTS, V_OFF, V_COUNT };
static inline Table<V_COUNT> pair_view(uint64_t cap) { return {{{"pair_pts", 8, NONE}, {"pair_off", ((size_t)cap + 1) * 8, NONE}}}; }
enum Stats { S_REC_FAIL, S_RLC_STATS, S_H_RLC_STATS, S_COUNT };
static inline Table<S_COUNT> rlc_stats() { return {{{"rec_fail", RING * 4, NONE}, {"rlc_stats", 8, ZERO}, {"h_rlc_stats", 8, NONE}}}; }
static inline size_t seed_ring_bytes() { return RING * 32; }

// ---- the set of h2v_check_pairs_multi (one batch check across several SRS), created by the first such call on a workspace of
// `cap` pairs - an ordinary or a laned one: the call runs as one piece, so the set has the decoding buffers of its own that a
// lane's chunk could not hold.  With it go an RLC set of the pairs shape (rlc_pairs(cap): coefficients, index arrays, good, flags,
// the bucket-MSM sets of R and of the first range's L), one bucket-MSM set per further range, sized by that range's count when a
// call first needs it (multi_range_cap), MULTI_ARG_SLOTS untimed events and as many pinned copies of an argument array.
constexpr uint32_t MULTI_MAX = 16, MULTI_ARG_SLOTS = 8;      // H2V_MULTI_SRS_MAX; calls whose argument arrays may be in flight
enum Multi { X_PTS, X_VALID, X_VALID_SUB, X_DEC_CTR, X_STATUS, X_ER, X_PAIR_PTS, X_PAIR_OFF, X_SUMS, X_ARGS, X_COUNT };
static inline size_t multi_args_bytes() { return (size_t)(MULTI_MAX + 1) * PIP_ARGS_BYTES; }     // one call's: R, then every range's L
static inline Table<X_COUNT> multi_srs(uint64_t cap) {
    const size_t n = (size_t)cap;
    return {{{"pts", n * PAIR_BYTES, NONE},
             {"valid", n * 2, NONE},
             {"valid_sub", n * 2, NONE},
             {"dec_ctr", 4, NONE},
             {"status", n * 4, NONE},
             {"er", n * JAC_BYTES, NONE},
             {"pair_pts", 8, NONE},
             {"pair_off", (n + 1) * 8, NONE},
             {"sums", (size_t)(MULTI_MAX + 1) * JAC_BYTES, NONE},      // R, then L_0 ..: RlcWs::sums, continued
             {"args_d", MULTI_ARG_SLOTS * multi_args_bytes(), NONE}}};
}
// the capacity a further range's bucket-MSM set is (re)allocated with for `count` pairs: the next power of two, at least 64
static inline uint32_t multi_range_cap(uint64_t count) {
    uint32_t c = 64;
    while ((uint64_t)c < count) c <<= 1;
    return c;
}

// ---- the set of the mixed calls ACROSS several SRS (H2V_MIXED_ACROSS_SRS), created by the first such call on a workspace of `cap`
// proofs and owned by its mixed-call staging: the (1 + MULTI_MAX) sums of the one multi-pairing, the argument ring of its bucket
// MSMs (MULTI_ARG_SLOTS device arrays; with them as many pinned copies and untimed events), the class-major L-terms of the fold
// form (scalars and point indices), and what the per-pair fall-back of the pairs form works on: the gathered pool, its status
// words and verdicts, and R of every pair as a Jacobian point.  With it go one bucket-MSM set per further class, sized by that
// class's count when a call first needs it (multi_range_cap), and - the pairs form only, at its first call - an RLC set of the
// pairs shape (rlc_pairs(cap): coefficients, index arrays, good, flags, the bucket-MSM sets of R and of the first class's L).
enum Across { A_SUMS, A_ARGS, A_CL_SCAL, A_CL_IDX, A_POOL_G, A_STATUS_G, A_ACCEPT_G, A_ER, A_COUNT };
static inline Table<A_COUNT> across_srs(uint64_t cap) {
    const size_t n = (size_t)cap;
    return {{{"sums", (size_t)(MULTI_MAX + 1) * JAC_BYTES, NONE},      // R, then L_0 ..: the layout k_pairing_rlc_multi reads
             {"args_d", MULTI_ARG_SLOTS * multi_args_bytes(), NONE},
             {"cl_scal", n * FR_BYTES, NONE},
             {"cl_idx", n * 4, NONE},
             {"pool_g", n * PAIR_BYTES, NONE},
             {"status_g", n * 4, NONE},
             {"accept_g", n, NONE},
             {"er", n * JAC_BYTES, NONE}}};
}
}   // namespace wslayout
