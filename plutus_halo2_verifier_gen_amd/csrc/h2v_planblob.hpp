// The plan blob, read ONCE, on the host: validation of the untrusted bytes (parse) and every host-side fact the loader derives
// from them.  HOST CODE ONLY - no GPU runtime call and no GPU header in this file, so that a stand-alone C++ program can include
// it and run it under sanitizers over a recorded corpus (tests/cpp/h2v_planblob.cpp, tests/golden/plan_load_verdicts.txt).
// parse is a trust boundary: what it lets through becomes register, constant and proof offsets that the kernels dereference
// without further checks.  It reads nothing outside [blob, blob + len).  h2v_plan_load_ex (h2v_capi.hip) is its only caller
// in the library and reads the blob through the View alone.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/h2v.h"
#include "h2v_hostmath.hpp"
#include "h2v_plan.h"
#include "h2v_seed.hpp"

namespace planblob {

struct Program { uint32_t off, n_instr, n_regs, lanes; };   // byte offset of the records, records, registers, records per bundle
// everything the loader learns from the bytes
struct View {
    uint32_t proof_len, n_pi, n_ci, n_consts, n_points, n_bases, n_terms, n_trace, pi_point;
    uint32_t off_consts, off_points, off_bases, off_terms, off_lines_sg2, off_lines_g2, off_trace, off_lines28_sg2, off_lines28_g2;
    Program narrow, wide;                          // wide.lanes == 0: the plan has no second schedule (then all of `wide` is 0)
    uint32_t ivc, n_main_terms, acc_idx[8];
    uint32_t tr_kind, tr_key_off, tr_key_len;      // transcript hash of the key and its blake2b key's range in the blob
    uint32_t n_squeezes, stream_len;               // SQUEEZE records of the narrow program as counted here; the header's stream length
    uint32_t n_var, n_fix;   // terms [0, n_var) per proof, [n_var, n_var + n_fix) VK bases; 0 / 0 when the VK-base terms are not the
                             // tail of the term list, the plan has no VK base, or it is recursive (no fixed-base launch then)
    std::vector<uint32_t> trace_slots;
};

static inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// One program: every register / constant / offset the kernels will touch is in range (H2V_OPS says what each field is), and the
// bundle discipline the multi-lane interpreter relies on holds (h2v_plan.h).  `ip` addresses 8 n_rec readable bytes.
static inline int check_program(const uint8_t *ip, const Program &pr, const View &v, uint32_t *squeezes, std::string &err) {
    auto fail = [&](const std::string &msg) { err = msg; return H2V_E_PLAN; };
    const uint32_t lanes = pr.lanes, n_rec = pr.n_instr;
    if (lanes == 0 || lanes > 32 || (lanes & (lanes - 1)) || n_rec % lanes) return fail("bad lane count of the program");
    auto in_range = [&](uint8_t kind, uint32_t field, uint32_t off) {
        switch (kind) {
        case H2V_ARG_NONE: return true;
        case H2V_ARG_REG: return field < pr.n_regs;
        case H2V_ARG_CONST: return field < v.n_consts;
        case H2V_ARG_PI: return field < v.n_pi;
        case H2V_ARG_TERM: return field < v.n_terms;
        case H2V_ARG_OFF32: return (uint64_t)off + 32 <= v.proof_len;
        case H2V_ARG_OFF48: return (uint64_t)off + 48 <= v.proof_len;
        }
        return false;
    };
    bool has_end = false;
    uint32_t sq = 0;
    for (uint32_t base_k = 0; base_k < n_rec && !has_end; base_k += lanes) {
        uint32_t wr[32], n_wr = 0;
        bool lane0_serial = false;
        for (uint32_t l = 0; l < lanes; l++) {
            const uint32_t k = base_k + l;
            const uint8_t op = ip[8 * k];
            const uint32_t dst = rd16(ip + 8 * k + 2), a = rd16(ip + 8 * k + 4), b = rd16(ip + 8 * k + 6);
            if (!h2v_op_known(op)) return fail("instruction " + std::to_string(k) + " out of range");
            const H2vOpInfo &info = H2V_OPS[op];
            if (!in_range(info.dst, dst, 0) || !in_range(info.a, a, a | (b << 16)) || !in_range(info.b, b, 0) || (info.needs_ci && v.n_ci != 1))
                return fail("instruction " + std::to_string(k) + " out of range");
            has_end = has_end || op == H2V_OP_END;
            sq += op == H2V_OP_SQUEEZE;
            if (info.serial && l != 0) return fail("transcript operation off lane 0 (record " + std::to_string(k) + ")");
            if (l == 0) lane0_serial = info.serial;
            else if (lane0_serial && op != H2V_OP_NOP) return fail("transcript operation shares its bundle (record " + std::to_string(k) + ")");
            if (h2v_op_writes(op)) wr[n_wr++] = dst;
        }
        // independence inside the bundle: no register is written twice, none that is written is read by any lane
        for (uint32_t x = 0; x < n_wr; x++) {
            for (uint32_t y = x + 1; y < n_wr; y++)
                if (wr[y] == wr[x]) return fail("two lanes of a bundle write one register");
            for (uint32_t l = 0; l < lanes; l++) {
                const uint32_t k = base_k + l;
                const uint8_t op = ip[8 * k];
                if (lanes > 1 && ((h2v_op_reads_a(op) && rd16(ip + 8 * k + 4) == wr[x]) || (h2v_op_reads_b(op) && rd16(ip + 8 * k + 6) == wr[x])))
                    return fail("a bundle reads a register it writes (record " + std::to_string(k) + ")");
            }
        }
    }
    if (!has_end) return fail("program has no END");
    if (squeezes) *squeezes = sq;
    // the interpreter's trip count is n_rec / lanes - 1: END is the last bundle and nowhere else
    bool end_is_last = ip[8 * (n_rec - lanes)] == H2V_OP_END;
    for (uint32_t k = 0; k + lanes < n_rec; k++) end_is_last = end_is_last && ip[8 * k] != H2V_OP_END;
    return end_is_last ? H2V_OK : fail("END must be the last bundle of the program");
}

// H2V_OK, H2V_E_PLAN or H2V_E_LIMIT (then `err` says why); on H2V_OK `v` is complete
static inline int parse(const uint8_t *blob, size_t len, View &v, std::string &err) {
    auto fail = [&](int code, const std::string &msg) { err = msg; return code; };
    v = View();
    const size_t hdr = 8 + 4 * H2V_PLAN_HDR_WORDS;
    if (len < hdr || memcmp(blob, H2V_PLAN_MAGIC, 8) != 0) return fail(H2V_E_PLAN, "bad magic / truncated header");
    uint32_t w[H2V_PLAN_HDR_WORDS];
    for (int i = 0; i < H2V_PLAN_HDR_WORDS; i++) w[i] = rd32(blob + 8 + 4 * i);
    if (w[H2V_HW_VERSION] != H2V_PLAN_VERSION && w[H2V_HW_VERSION] != H2V_PLAN_VERSION_FLAVOURED) return fail(H2V_E_PLAN, "unsupported plan version");
    if (w[H2V_HW_TOTAL_LEN] != len) return fail(H2V_E_PLAN, "length mismatch");
    // transcript hash of the key: version 4 knows the Cardano flavour only (its three words are spare and zero)
    v.tr_kind = w[H2V_HW_TR_KIND]; v.tr_key_off = w[H2V_HW_TR_KEY_OFF]; v.tr_key_len = w[H2V_HW_TR_KEY_LEN];
    if (w[H2V_HW_VERSION] == H2V_PLAN_VERSION && (v.tr_kind || v.tr_key_off || v.tr_key_len)) return fail(H2V_E_PLAN, "a version-4 plan names a transcript hash");
    if (v.tr_kind >= H2V_TR_KIND_COUNT) return fail(H2V_E_PLAN, "unknown transcript hash kind " + std::to_string(v.tr_kind));
    if (v.tr_key_len > H2V_TR_KEY_MAX) return fail(H2V_E_PLAN, "transcript hash key longer than 64 bytes");
    if (v.tr_kind == H2V_TR_CARDANO_BLAKE2B_256 && (v.tr_key_len || v.tr_key_off)) return fail(H2V_E_PLAN, "the Cardano transcript hash is unkeyed");
    if (v.tr_key_len ? (v.tr_key_off < hdr || (uint64_t)v.tr_key_off + v.tr_key_len > len) : v.tr_key_off != 0)
        return fail(H2V_E_PLAN, "transcript hash key out of bounds");
    v.proof_len = w[H2V_HW_PROOF_LEN]; v.n_pi = w[H2V_HW_N_PI]; v.n_ci = w[H2V_HW_N_CI]; v.n_consts = w[H2V_HW_N_CONSTS];
    v.n_points = w[H2V_HW_N_POINTS]; v.n_bases = w[H2V_HW_N_VK_BASES]; v.n_terms = w[H2V_HW_N_TERMS]; v.n_trace = w[H2V_HW_N_TRACE];
    v.narrow = {w[H2V_HW_OFF_INSTR], w[H2V_HW_N_INSTR], w[H2V_HW_N_REGS], w[H2V_HW_VM_LANES]};
    struct Sec { int off_word; uint64_t bytes; uint32_t *off; };
    const Sec secs[] = {{H2V_HW_OFF_INSTR, 8ull * v.narrow.n_instr, &v.narrow.off}, {H2V_HW_OFF_CONSTS, 32ull * v.n_consts, &v.off_consts},
                        {H2V_HW_OFF_POINTS, 4ull * v.n_points, &v.off_points}, {H2V_HW_OFF_VK_BASES, 96ull * v.n_bases, &v.off_bases},
                        {H2V_HW_OFF_TERMS, 8ull * v.n_terms, &v.off_terms},
                        {H2V_HW_OFF_LINES_SG2, 192ull * H2V_MILLER_LINES, &v.off_lines_sg2}, {H2V_HW_OFF_LINES_G2, 192ull * H2V_MILLER_LINES, &v.off_lines_g2},
                        {H2V_HW_OFF_TRACE, 8ull * v.n_trace, &v.off_trace},
                        {H2V_HW_OFF_LINES28_SG2, 512ull * H2V_MILLER_LINES, &v.off_lines28_sg2}, {H2V_HW_OFF_LINES28_G2, 512ull * H2V_MILLER_LINES, &v.off_lines28_g2}};
    for (const Sec &s : secs) {
        const uint64_t off = *s.off = w[s.off_word];
        if (off < hdr || (off & 15) || off + s.bytes > len) return fail(H2V_E_PLAN, "section out of bounds");
    }
    if (v.narrow.n_instr == 0 || v.narrow.n_instr > (1u << 20) || v.narrow.n_regs == 0 || v.narrow.n_regs > 65535 || v.n_points == 0 ||
        v.n_points > 4096 || v.n_terms == 0 || v.n_ci > 1 || v.n_pi > (1u << 16) || v.proof_len > (1u << 24))
        return fail(H2V_E_PLAN, "implausible counts");
    const uint32_t ivc = v.ivc = w[H2V_HW_IVC], n_main = v.n_main_terms = w[H2V_HW_N_MAIN_TERMS], n_terms = v.n_terms;
    if (ivc > 1 || n_main == 0 || n_main > n_terms || (!ivc && n_main != n_terms) || (ivc && n_terms < n_main + 2))
        return fail(H2V_E_PLAN, "inconsistent recursion header");
    // the widest sum the launcher cuts into segments (H2V_MAX_MSM_TERMS; the partial-sum buffer is sized from it)
    const std::string cap = " terms; this backend sums at most " + std::to_string(H2V_MAX_MSM_TERMS) + " terms per MSM (H2V_MAX_MSM_TERMS)";
    if (n_main > H2V_MAX_MSM_TERMS)
        return fail(H2V_E_LIMIT, std::string(ivc ? "the proof's own MSM" : "the final MSM") + " has " + std::to_string(n_main) + cap);
    if (ivc && n_terms - n_main - 1 > H2V_MAX_MSM_TERMS)
        return fail(H2V_E_LIMIT, "the recursion sum acc_right + fixed bases has " + std::to_string(n_terms - n_main - 1) + cap);
    for (int k = 0; k < 8; k++) {
        v.acc_idx[k] = w[H2V_HW_ACC_IDX0 + k];
        if (ivc && v.acc_idx[k] >= v.n_pi) return fail(H2V_E_PLAN, "accumulator public-input index out of range");
    }
    v.pi_point = w[H2V_HW_PI_POINT];
    if (v.pi_point >= v.n_points) return fail(H2V_E_PLAN, "pi point index out of range");
    if (int rc = check_program(blob + v.narrow.off, v.narrow, v, &v.n_squeezes, err)) return rc;
    if (w[H2V_HW_VM2_LANES]) {
        v.wide = {w[H2V_HW_VM2_OFF_INSTR], w[H2V_HW_VM2_N_INSTR], w[H2V_HW_VM2_N_REGS], w[H2V_HW_VM2_LANES]};
        const uint64_t off = v.wide.off;
        if (off < hdr || (off & 15) || off + 8ull * v.wide.n_instr > len || v.wide.n_instr == 0 || v.wide.n_instr > (1u << 20) ||
            v.wide.n_regs == 0 || v.wide.n_regs > 65535)
            return fail(H2V_E_PLAN, "wide program section out of bounds");
        if (v.wide.lanes < 2 || !vm_fits_lds(v.wide.n_regs, v.wide.lanes)) return fail(H2V_E_PLAN, "wide program does not fit the LDS register file");
        if (int rc = check_program(blob + off, v.wide, v, nullptr, err)) return rc;
    }
    if (v.narrow.lanes > 1 && !vm_fits_lds(v.narrow.n_regs, v.narrow.lanes)) return fail(H2V_E_PLAN, "multi-lane program does not fit the LDS register file");
    for (uint32_t k = 0; k < v.n_points; k++)
        if ((uint64_t)rd32(blob + v.off_points + 4 * k) + 48 > v.proof_len) return fail(H2V_E_PLAN, "point offset out of range");
    const uint8_t *tp = blob + v.off_terms;
    for (uint32_t k = 0; k < n_terms; k++) {
        const uint32_t kind = rd32(tp + 8 * k), idx = rd32(tp + 8 * k + 4);
        const bool ok = (kind == H2V_TERM_PROOF_POINT && idx < v.n_points) || (kind == H2V_TERM_VK_BASE && idx < v.n_bases) ||
                        (kind == H2V_TERM_COMMITTED_INSTANCE && v.n_ci == 1) || (kind == H2V_TERM_ACC_POINT && ivc && idx < 2);
        if (!ok) return fail(H2V_E_PLAN, "MSM term out of range");
    }
    for (uint32_t k = 0; k < v.n_trace; k++)
        if (rd32(blob + v.off_trace + 8 * k + 4) >= v.narrow.n_regs) return fail(H2V_E_PLAN, "trace register out of range");
    // nothing below can fail.  Fixed-base launches of the MSM: non-recursive plans whose VK-base terms are the tail of the term
    // list, as plan.py orders them
    if (!ivc && v.n_bases) {
        uint32_t nv = 0;
        while (nv < n_terms && rd32(tp + 8 * nv) != H2V_TERM_VK_BASE) nv++;
        bool tail_ok = nv < n_terms;
        for (uint32_t k = nv; k < n_terms; k++) tail_ok = tail_ok && rd32(tp + 8 * k) == H2V_TERM_VK_BASE;
        if (tail_ok) { v.n_var = nv; v.n_fix = n_terms - nv; }
    }
    v.stream_len = w[H2V_HW_STREAM_LEN];
    for (uint32_t k = 0; k < v.n_trace; k++) v.trace_slots.push_back(rd32(blob + v.off_trace + 8 * k));
    return H2V_OK;
}

// The term table as the device sees it: committed-instance terms rewritten to "per-proof slot n_points" (the decompression
// kernel stores the committed instance there) and accumulator terms to the slots behind it (the kernel rebuilds the accumulator
// points there), so that the MSM kernel sees two term kinds only.  8 n_terms bytes, to be laid over the blob's at v.off_terms.
static inline std::vector<uint8_t> device_terms(const uint8_t *blob, const View &v) {
    std::vector<uint8_t> out(blob + v.off_terms, blob + v.off_terms + 8 * (size_t)v.n_terms);
    for (uint32_t k = 0; k < v.n_terms; k++) {
        uint8_t *t = out.data() + 8 * k;
        const uint32_t kind = rd32(t);
        if (kind != H2V_TERM_COMMITTED_INSTANCE && kind != H2V_TERM_ACC_POINT) continue;
        const uint32_t slot[2] = {H2V_TERM_PROOF_POINT, kind == H2V_TERM_COMMITTED_INSTANCE ? v.n_points : v.n_points + v.n_ci + rd32(t + 4)};
        memcpy(t, slot, 8);
    }
    return out;
}

// All-window tables of the VK bases, fix_tab[base][W][entries][28]: window width c = 12 bits (22 additions per VK term in every
// proof, 5 MB per base) unless that would take more than 2 GB, then 8; h2v_plan_opts.fixed_base_window_bits = 4 / 8 / 12 forces
// it.  Signed digits: 2^(c-1) entries per window, W windows over a scalar.
struct FixedTables { uint32_t c, W, entries; size_t bytes; };
static inline FixedTables fixed_tables(uint32_t n_bases, uint32_t forced_bits) {
    const uint32_t c = forced_bits ? forced_bits : (size_t)n_bases * 22 * 2048 * 112 <= ((size_t)2 << 30) ? 12u : 8u;
    const uint32_t W = c == 4 ? 65u : c == 8 ? 33u : 22u, entries = 1u << (c - 1);
    return {c, W, entries, (size_t)n_bases * W * entries * 28 * 4};
}

// The six-lane pairing engine multiplies by lines with a UNIT coefficient (h2v_pairing_six.hpp): from the blob's line records
// [-lambda, xi (-lambda), c, xi c] (28-bit Montgomery limbs) the constants A = -lambda / c, B = 1 / c of every line of both loops,
// laid out [line][loop][A0, A1, B0, B1][16 dwords], followed by [1, K1, K2, K1 K2] (2 x 12 Montgomery words each) with K_u the
// product of loop u's c along the Miller schedule (k <- k^2 per bit, k <- k c per line): K times the unit-line Miller value is
// the plan's.  One Fp2 inversion per line, 136 per plan load.  false: some c is zero (no table; the engine is not offered).
constexpr uint32_t SIX_NORM_DW = H2V_MILLER_LINES * 2 * 4 * 16;
static inline bool six_line_tables(const uint8_t *blob, const View &v, std::vector<uint32_t> &out) {
    using namespace h2vhost;
    auto slot_fp = [](const uint8_t *slot) { uint32_t limb[14]; memcpy(limb, slot, sizeof limb); return fp_from_limbs28(limb); };
    auto put_words = [](uint32_t *dst, const FpE &a) { uint8_t b[48]; fp_mont392_bytes(a, b); memcpy(dst, b, 48); };
    out.assign(SIX_NORM_DW + 4 * 24, 0);
    const uint8_t *src[2] = {blob + v.off_lines28_sg2, blob + v.off_lines28_g2};
    F2 K[2] = {f2_one(), f2_one()};
    int ln = 0;
    for (int bit = 62; bit >= 0; bit--) {
        const int steps = ((0xd201000000010000ull >> bit) & 1) ? 2 : 1;
        for (int u = 0; u < 2; u++) K[u] = f2_sqr(K[u]);
        for (int s2 = 0; s2 < steps; s2++, ln++)
            for (int u = 0; u < 2; u++) {
                const uint8_t *rec = src[u] + (size_t)ln * 8 * 64;
                const F2 nl = {slot_fp(rec), slot_fp(rec + 64)}, cc = {slot_fp(rec + 4 * 64), slot_fp(rec + 5 * 64)};
                if (f2_is_zero(cc)) return false;
                const F2 B = f2_inv(cc), A = f2_mul(nl, B);
                uint32_t *dst = out.data() + ((size_t)ln * 2 + u) * 4 * 16;     // (dwords 14 and 15 of a slot stay zero)
                fp_to_limbs28(A.a, dst); fp_to_limbs28(A.b, dst + 16); fp_to_limbs28(B.a, dst + 32); fp_to_limbs28(B.b, dst + 48);
                K[u] = f2_mul(K[u], cc);
            }
    }
    if (ln != H2V_MILLER_LINES) return false;
    const F2 ks[4] = {f2_one(), K[0], K[1], f2_mul(K[0], K[1])};
    for (int q = 0; q < 4; q++) { put_words(out.data() + SIX_NORM_DW + 24 * q, ks[q].a); put_words(out.data() + SIX_NORM_DW + 24 * q + 12, ks[q].b); }
    return true;
}

// Two 64-bit FNV-1a sums (different offset bases) over the s_g2 line-table section of the blob: equal line tables of s_g2 = one
// SRS (h2v_verify_mixed).  The keys of a host are its own configuration, not an adversary's input: the digest guards against a
// mistake, not an attack.
static inline void sg2_digest(const uint8_t *blob, const View &v, uint64_t out[2]) {
    const uint8_t *sec = blob + v.off_lines28_sg2;
    uint64_t a = 0xcbf29ce484222325ull, b = 0x84222325cbf29ce4ull;
    for (size_t k = 0; k < 512u * H2V_MILLER_LINES; k++) { a = (a ^ sec[k]) * 0x100000001b3ull; b = (b ^ (uint8_t)(sec[k] + 0x5a)) * 0x100000001b3ull; }
    out[0] = a; out[1] = b;
}
// blake2b-256(TAG key || the plan blob): what a derived batch seed binds the key with (h2v_seed.hpp)
static inline void key_tag(const uint8_t *blob, size_t len, uint8_t out[32]) {
    const h2vseed::TagWords kt = h2vseed::tag_words(h2vseed::TAG_KEY);
    h2vhost::b2_256_host((const uint8_t *)kt.w, h2vseed::TAG_BYTES, blob, len, out);
}
// The state every proof's transcript starts from under the keyed blake2b-512 flavour: parameter block, then the key block
// compressed here, once per plan (a transcript always hashes at least one byte before a digest is taken, so the key block is
// never the final one).  Returns the bytes compressed so far.
static inline uint32_t transcript_midstate(const uint8_t *blob, const View &v, uint64_t h0[8]) {
    return h2vhost::b2_keyed_midstate_host(h0, 64, blob + v.tr_key_off, v.tr_key_len);
}

}   // namespace planblob
