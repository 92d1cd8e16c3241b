// gfx950 kernels of the Halo2/KZG batch verifier (one independent proof per lane / lane group).
//
//   k_transcript_combiner   P1-P6 scalars: blake2b transcript replay + Fr combiner + final MSM scalar vector
//                           (interprets the plan's straight-line program; wave-uniform control flow)
//   k_g1_decompress         48-byte zcash G1 -> affine Montgomery, with on-curve + subgroup validation
//   k_g1_msm                er = sum_t s_t * B_t per proof: one lane per term, wave/LDS segmented reduction
//   k_pairing_check         accept <=> e(pi, s_g2) == e(er, G2): 2 Miller loops over precomputed lines of the
//                           FIXED G2 arguments + one final exponentiation, fused in one kernel
//
// Algorithm of record: /root/reference/aiken-verifier/templates/verification_h2.hbs:21-129 and the library it
// calls (aiken-verifier/aiken_halo2/lib/{transcript,lagrange,halo2_kzg,bls_utils}.ak); hash plug-in
// /root/reference/src/plutus_gen/adjusted_types/mod.rs:30-72.
#include <hip/hip_runtime.h>
#include "h2v_curve28.hpp"
#include "h2v_plan.h"
#include "h2v_tower.hpp"
#include "h2v_pairing_coop.hpp"
#include "h2v_pairing_six.hpp"

// ============================================================================ blake2b-256 (RFC 7693)
__device__ static constexpr uint64_t B2_IV[8] = {
    0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
    0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
__device__ static constexpr uint8_t B2_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

H2V_DI uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// One compression.  The 128-byte message block is read from LDS (dword d of the calling lane at msg[d * 64]) and the
// twelve rounds are a real loop whose message schedule is looked up per round (a scalar load of the sigma row, sixteen
// 64-bit LDS reads): 2.5 KB of code instead of the 24 KB of the unrolled form.  On the combiner's lone waves the
// unrolled form ran at the speed of instruction fetch - every instruction executed once per call, 32k cycles per
// compression - while this one stays in the instruction cache.
typedef __attribute__((address_space(3))) uint32_t h2v_lds_u32;
H2V_DN void b2_compress_lds(uint64_t (&h)[8], const uint32_t *msg_generic, uint64_t t, bool last) {
    const h2v_lds_u32 *msg = (const h2v_lds_u32 *)msg_generic;
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = B2_IV[i]; }
    v[12] ^= t;
    if (last) v[14] = ~v[14];
#define B2G(a, b, c, d, x, y)                                                                             \
    v[a] = v[a] + v[b] + (x); v[d] = rotr64(v[d] ^ v[a], 32); v[c] = v[c] + v[d]; v[b] = rotr64(v[b] ^ v[c], 24); \
    v[a] = v[a] + v[b] + (y); v[d] = rotr64(v[d] ^ v[a], 16); v[c] = v[c] + v[d]; v[b] = rotr64(v[b] ^ v[c], 63);
#pragma unroll 1
    for (int r = 0; r < 12; r++) {
        uint64_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t sg = B2_SIGMA[r][i];
            w[i] = (uint64_t)msg[(2 * sg) * 64] | ((uint64_t)msg[(2 * sg + 1) * 64] << 32);
        }
        B2G(0, 4, 8, 12, w[0], w[1])
        B2G(1, 5, 9, 13, w[2], w[3])
        B2G(2, 6, 10, 14, w[4], w[5])
        B2G(3, 7, 11, 15, w[6], w[7])
        B2G(0, 5, 10, 15, w[8], w[9])
        B2G(1, 6, 11, 12, w[10], w[11])
        B2G(2, 7, 8, 13, w[12], w[13])
        B2G(3, 4, 9, 14, w[14], w[15])
    }
#undef B2G
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

// Running transcript hash of one lane.  The 128-byte block buffer lives in LDS, dword d of lane l at
// sbuf[d*64 + l] (conflict-free); fill level and byte counter are identical in every lane (the proof layout is
// static), so they are wave-uniform scalars.
struct Transcript {
    uint64_t h[8];
    uint32_t t;       // bytes already compressed
    uint32_t buflen;  // bytes waiting in the LDS block
};

H2V_DI void tr_init(Transcript &s) {
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] = B2_IV[i];
    s.h[0] ^= 0x01010000ull ^ 32ull;  // digest 32, key 0, fanout 1, depth 1 (blake2b_simd Params::new().hash_length(32))
    s.t = 0;
    s.buflen = 0;
}
// A hash that starts from a state worked out on the host (the keyed blake2b-512 transcript: parameter block and key block
// are the same for every proof of a plan, h2v_plan.h: tr_h0 / tr_t0)
H2V_DI void tr_init_state(Transcript &s, const uint64_t *h0, uint32_t t0) {
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] = h0[i];
    s.t = t0;
    s.buflen = 0;
}
H2V_DI void tr_put(Transcript &s, uint32_t *sbuf, int lane, uint32_t byte) {
    if (s.buflen == 128) {  // full and more input follows: not the last block
        s.t += 128;
        // through a copy: handing s.h itself to the out-of-line function would pin the whole struct - fill level and
        // byte counter included - in private memory, and every tr_put would then wait for a scratch round trip
        uint64_t hh[8];
#pragma unroll
        for (int i = 0; i < 8; i++) hh[i] = s.h[i];
        b2_compress_lds(hh, sbuf + lane, s.t, false);
#pragma unroll
        for (int i = 0; i < 8; i++) s.h[i] = hh[i];
        s.buflen = 0;
    }
    reinterpret_cast<uint8_t *>(&sbuf[(s.buflen >> 2) * 64 + lane])[s.buflen & 3] = (uint8_t)byte;
    s.buflen++;
}
// digest of everything absorbed so far, leaving the running state untouched (State::finalize on a clone).  The unused
// tail of the block buffer is zeroed in place (the padding of the last block); the pending bytes stay where they are.
// N = 4: the first 32 bytes of the state (a blake2b-256); N = 8: all 64 (a blake2b-512: the width is in the initial state).
template <int N>
H2V_DI void tr_digest(const Transcript &s, uint32_t *sbuf, int lane, uint64_t (&out)[N]) {
    static_assert(N == 4 || N == 8, "32- or 64-byte digest");
    uint64_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = s.h[i];
    const uint32_t bl = s.buflen;
    if (bl & 3) sbuf[(bl >> 2) * 64 + lane] &= (1u << (8 * (bl & 3))) - 1u;
#pragma unroll 1
    for (uint32_t d = (bl + 3) >> 2; d < 32; d++) sbuf[d * 64 + lane] = 0;
    b2_compress_lds(h, sbuf + lane, (uint64_t)s.t + bl, true);
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = h[i];
}
// blake2b-256 of a 32-byte message; borrows the lane's block buffer (saved and restored around the call)
H2V_DI void b2_hash32(const uint64_t (&in)[4], uint64_t (&out)[4], uint32_t *sbuf, int lane) {
    uint64_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = B2_IV[i];
    h[0] ^= 0x01010000ull ^ 32ull;
    uint32_t saved[32];
#pragma unroll
    for (int d = 0; d < 32; d++) saved[d] = sbuf[d * 64 + lane];
#pragma unroll
    for (int d = 0; d < 32; d++) sbuf[d * 64 + lane] = d < 8 ? (uint32_t)(in[d >> 1] >> (32 * (d & 1))) : 0u;
    b2_compress_lds(h, sbuf + lane, 32, true);
#pragma unroll
    for (int d = 0; d < 32; d++) sbuf[d * 64 + lane] = saved[d];
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = h[i];
}

// ============================================================================ K1+K3: transcript + Fr combiner
// Register file in global memory: limb l of register r of proof i at regs[(r*8 + l)*stride + i]
// (lanes of a wave touch consecutive dwords).
H2V_DI void reg_load(Fr &v, const uint32_t *regs, uint32_t r, uint32_t stride, uint32_t i) {
#pragma unroll
    for (int l = 0; l < 8; l++) v.v[l] = regs[(size_t)(r * 8 + l) * stride + i];
}
H2V_DI void reg_store(uint32_t *regs, uint32_t r, uint32_t stride, uint32_t i, const Fr &v) {
#pragma unroll
    for (int l = 0; l < 8; l++) regs[(size_t)(r * 8 + l) * stride + i] = v.v[l];
}
// The same register file in LDS when the plan is small enough for a few dozen proofs per CU: limb l of register r of
// the block's proof slot q at vm_lds[(r*8 + l)*P + q].  With 64 waves on a 256-CU chip this kernel is pure latency, and
// a dependent global load + store per instruction was most of it.
extern __shared__ uint32_t vm_lds[];
struct RegsGlobal {
    uint32_t *regs;
    uint32_t stride, i_load, i_store;
    H2V_DI void load(Fr &v, uint32_t r) const { reg_load(v, regs, r, stride, i_load); }
    H2V_DI void store(uint32_t r, const Fr &v) const { reg_store(regs, r, stride, i_store, v); }
};
struct RegsLds {
    uint32_t P, q;
    H2V_DI void load(Fr &v, uint32_t r) const {
#pragma unroll
        for (int l = 0; l < 8; l++) v.v[l] = vm_lds[(r * 8 + l) * P + q];
    }
    H2V_DI void store(uint32_t r, const Fr &v) const {
#pragma unroll
        for (int l = 0; l < 8; l++) vm_lds[(r * 8 + l) * P + q] = v.v[l];
    }
};
H2V_DI void fr_const(Fr &v, const uint32_t *c) {
#pragma unroll
    for (int l = 0; l < 8; l++) v.v[l] = c[l];
}
// absorb 0x01 || 32 little-endian bytes of a canonical (non-Montgomery) scalar
H2V_DI void tr_absorb_scalar(Transcript &s, uint32_t *sbuf, int lane, const Fr &plain) {
    tr_put(s, sbuf, lane, 1);
#pragma unroll
    for (int k = 0; k < 32; k++) tr_put(s, sbuf, lane, (plain.v[k >> 2] >> (8 * (k & 3))) & 0xff);   // static limb indices
}

// The program is a sequence of bundles of L records (h2v_plan.h); lane `sub` of the proof's L lanes executes record `sub`
// of each bundle.  The L lanes share the proof's register file (LDS), sit in the same wave, and a bundle's records are
// independent, so program order is all the synchronisation there is: LDS serves one wave's accesses in issue order.
// The transcript operations are on lane 0 by construction (the loader checks), so only that lane's hash state is real.
// TRK = the transcript hash of the plan's key (h2v_plan.h: H2V_TR_*), a compile-time choice: the Cardano instantiation is
// the code it was before there was a choice (its constants stay immediates), and the launcher picks by plan.tr_kind.
template <class RF, uint32_t TRK = H2V_TR_CARDANO_BLAKE2B_256>
H2V_DI void vm_run(const H2vDevPlan &plan, const RF rf, uint32_t *sbuf, const int lane, const uint32_t i, const uint32_t ii,
                   const bool live, const uint32_t L, const uint32_t sub, uint32_t *st_red /* 64 dwords of LDS */,
                   const uint32_t P /* proof slots of the block: lane l serves slot l & (P - 1) */,
                   const uint8_t *__restrict__ proofs, const uint64_t *__restrict__ proof_off,
                   const uint8_t *__restrict__ instances, const uint8_t *__restrict__ committed,
                   uint32_t *__restrict__ scalars, uint32_t *__restrict__ status, uint32_t *__restrict__ trace) {
    const uint64_t off0 = proof_off[ii];
    const uint64_t plen = proof_off[ii + 1] - off0;
    uint32_t st = 0;
    const bool short_proof = plen < plan.proof_len;
    if (short_proof) st |= H2V_ST_SHORT_PROOF;
    // a short proof is rejected up front; its lane replays a zero-length-safe window (no out-of-bounds reads)
    const uint8_t *proof = proofs + off0;
    // Pull the proof into the cache hierarchy up front: the proof's L lanes touch one byte per 64-byte line, all loads in
    // flight together.  Without it every READ_SCALAR / READ_POINT of the lone wave waits out an HBM miss of its own
    // (~11 k cycles per scalar read, 70 of them in the sha256 shape).  The bytes feed a value that is only stored under a
    // condition that never holds, so the loads stay.
    uint32_t warm = 0;
    if (!short_proof) {
#pragma unroll 1
        for (uint32_t o = 64 * sub; o < plan.proof_len; o += 64 * L) warm += proof[o];
    }
    Transcript tr;
    if constexpr (TRK == H2V_TR_BLAKE2B_512) tr_init_state(tr, plan.tr_h0, plan.tr_t0);
    else tr_init(tr);
    Fr a, b, r;
    // Record fetch: one 8-byte load per lane and bundle (the L lanes of a proof read L consecutive records), issued one
    // bundle ahead so that its latency - which a lone wave cannot hide behind anything else - overlaps the current bundle.
    // END is the last bundle (the loader checks), so the trip count is known without looking at the records.
    const uint64_t *code = reinterpret_cast<const uint64_t *>(plan.instr);
    uint64_t nxt = code[sub];
    for (uint32_t pc = 0; pc + L < plan.n_instr; pc += L) {
        const uint64_t rec = nxt;
        nxt = code[pc + L + sub];
        const struct { uint32_t x, y; } raw = {(uint32_t)rec, (uint32_t)(rec >> 32)};
        H2vInstr ins;
        ins.op = (uint8_t)(raw.x & 0xffu); ins.pad = 0; ins.dst = (uint16_t)(raw.x >> 16);
        ins.a = (uint16_t)(raw.y & 0xffffu); ins.b = (uint16_t)(raw.y >> 16);
        switch (ins.op) {
        case H2V_OP_ABSORB_REG: {
            rf.load(a, ins.a);
            fr_from_mont(b, a);
            tr_absorb_scalar(tr, sbuf, lane, b);
        } break;
        case H2V_OP_ABSORB_CI: {
            // (all the bytes are loaded before the first is hashed: a lone wave pays a full memory latency for every
            // load it waits on, and a load inside the byte loop is waited on 48 times)
            uint8_t raw[48];
#pragma unroll
            for (int k = 0; k < 48; k++) raw[k] = committed[(size_t)ii * 48 + k];
            tr_put(tr, sbuf, lane, 1);
#pragma unroll
            for (int k = 0; k < 48; k++) tr_put(tr, sbuf, lane, raw[k]);
        } break;
        case H2V_OP_LOAD_INSTANCE: {
            const uint8_t *p = instances + ((size_t)ii * plan.n_pi + ins.a) * 32;
#pragma unroll
            for (int l = 0; l < 8; l++)
                b.v[l] = (uint32_t)p[4 * l] | ((uint32_t)p[4 * l + 1] << 8) | ((uint32_t)p[4 * l + 2] << 16) | ((uint32_t)p[4 * l + 3] << 24);
            // public inputs are field elements on the reference side (Rust F / Aiken State<Scalar>): only the canonical
            // encoding exists there, so v + r is rejected here rather than verifying as a second encoding of v
            if (FrF::geq_mod(b.v)) st |= H2V_ST_BAD_SCALAR;
            fr_to_mont(r, b);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_READ_POINT: {
            const uint32_t off = (uint32_t)ins.a | ((uint32_t)ins.b << 16);
            // unconditional loads from one base (a short proof reads a table of the plan instead and is zeroed): a
            // load under a branch per byte is waited for before the next one issues - 560 cycles per byte on a lone wave
            const uint8_t *src = short_proof ? reinterpret_cast<const uint8_t *>(plan.lines_sg2) : proof + off;
            uint8_t raw[48];
#pragma unroll
            for (int k = 0; k < 48; k++) raw[k] = src[k];
#pragma unroll
            for (int k = 0; k < 48; k++) raw[k] = short_proof ? (uint8_t)0 : raw[k];
            tr_put(tr, sbuf, lane, 1);
#pragma unroll
            for (int k = 0; k < 48; k++) tr_put(tr, sbuf, lane, raw[k]);
        } break;
        case H2V_OP_READ_SCALAR: {
            const uint32_t off = (uint32_t)ins.a | ((uint32_t)ins.b << 16);
            const uint8_t *src = short_proof ? reinterpret_cast<const uint8_t *>(plan.lines_sg2) : proof + off;
            uint8_t raw[32];
#pragma unroll
            for (int k = 0; k < 32; k++) raw[k] = src[k];
#pragma unroll
            for (int k = 0; k < 32; k++) raw[k] = short_proof ? (uint8_t)0 : raw[k];
#pragma unroll
            for (int l = 0; l < 8; l++)
                b.v[l] = (uint32_t)raw[4 * l] | ((uint32_t)raw[4 * l + 1] << 8) | ((uint32_t)raw[4 * l + 2] << 16) | ((uint32_t)raw[4 * l + 3] << 24);
            tr_put(tr, sbuf, lane, 1);
#pragma unroll
            for (int k = 0; k < 32; k++) tr_put(tr, sbuf, lane, raw[k]);
            // canonical encodings only: the Rust reader (and Plinth's mkScalar, BlsTypes.hs:129-132) rejects >= r
            if (FrF::geq_mod(b.v)) st |= H2V_ST_BAD_SCALAR;
            fr_to_mont(r, b);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_SQUEEZE: {
            // adjusted_types/mod.rs:44-71: update(0x00); h = finalize; h2 = blake2b256(h);
            // challenge = from_uniform_bytes(h || h2) = LE(h) + LE(h2) * 2^256 mod r   (transcript.ak:85-106)
            // blake2b-512 (halo2's default blake2b_simd::State): update(0x00); out = the 64-byte digest of a copy of the
            // state, which goes on with the 0x00 in it; challenge = from_uniform_bytes(out), the same formula on out[0:32] || out[32:64]
            tr_put(tr, sbuf, lane, 0);
            Fr lo, hi, k;
            if constexpr (TRK == H2V_TR_BLAKE2B_512) {
                uint64_t h[8];
                tr_digest(tr, sbuf, lane, h);
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    lo.v[2 * l] = (uint32_t)h[l]; lo.v[2 * l + 1] = (uint32_t)(h[l] >> 32);
                    hi.v[2 * l] = (uint32_t)h[4 + l]; hi.v[2 * l + 1] = (uint32_t)(h[4 + l] >> 32);
                }
            } else {
                uint64_t h[4], h2[4];
                tr_digest(tr, sbuf, lane, h);
                b2_hash32(h, h2, sbuf, lane);
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    lo.v[2 * l] = (uint32_t)h[l]; lo.v[2 * l + 1] = (uint32_t)(h[l] >> 32);
                    hi.v[2 * l] = (uint32_t)h2[l]; hi.v[2 * l + 1] = (uint32_t)(h2[l] >> 32);
                }
            }
            fr_to_mont(a, lo);
            fr_const(k, FR_R3);
            fr_mul(b, hi, k);  // hi * 2^768 / 2^256 = (hi * 2^256) * R
            fr_add(r, a, b);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_CONST: {
            fr_const(r, plan.consts + (size_t)ins.a * 8);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_ADD: case H2V_OP_SUB: case H2V_OP_MUL: {
            rf.load(a, ins.a);
            rf.load(b, ins.b);
            if (ins.op == H2V_OP_ADD) fr_add(r, a, b);
            else if (ins.op == H2V_OP_SUB) fr_sub(r, a, b);
            else fr_mul(r, a, b);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_NEG: {
            rf.load(a, ins.a);
            FrF::neg(r, a);
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_INV: {
            rf.load(a, ins.a);
            // recip_eea of zero divides by zero in the reference (bls_utils.ak:151-154) => reject
            {
                Fr ia = a, ir;   // copies: fr_inv takes references, and a / r must not be pinned in private memory
                if (!fr_inv(ir, ia)) st |= H2V_ST_INVERSE_OF_ZERO;
                r = ir;
            }
            if (live) rf.store(ins.dst, r);
        } break;
        case H2V_OP_ASSERT_ZERO: {
            rf.load(a, ins.a);
            if (!FrF::is_zero(a)) st |= H2V_ST_RECURSION;   // expect transcript_rep == i_1 (emitters/aiken.rs:696)
        } break;
        case H2V_OP_OUT_SCALAR: {
            rf.load(a, ins.a);
            fr_from_mont(r, a);
            if (live) {
#pragma unroll
                for (int l = 0; l < 8; l++) scalars[((size_t)i * plan.n_terms + ins.dst) * 8 + l] = r.v[l];
            }
        } break;
        default: break;   // NOP: this lane idles through the bundle
        }
    }
    if (L > 1) {   // status bits of the proof's other lanes (inverse of zero, recursion check)
        st_red[lane] = st;
        __syncthreads();
        for (uint32_t k = 1; k < L; k++) st |= st_red[((uint32_t)lane & (P - 1)) + k * P];
    }
    if (live && sub == 0) {
        if (warm == 0xffffffffu) st |= 0x80000000u;   // never true (at most 2^24 / 64 bytes of 255 are summed): keeps `warm` live
        status[i] = st;
        if (trace) {
            for (uint32_t k = 0; k < plan.n_trace; k++) {
                rf.load(a, plan.trace[2 * k + 1]);
                fr_from_mont(r, a);
#pragma unroll
                for (int l = 0; l < 8; l++) trace[((size_t)i * plan.n_trace + k) * 8 + l] = r.v[l];
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner(H2vDevPlan plan, uint32_t n, uint32_t stride, const uint8_t *__restrict__ proofs,
                      const uint64_t *__restrict__ proof_off, const uint8_t *__restrict__ instances,
                      const uint8_t *__restrict__ committed, uint32_t *__restrict__ regs,
                      uint32_t *__restrict__ scalars, uint32_t *__restrict__ status, uint32_t *__restrict__ trace) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;  // dead lanes shadow the last proof (keeps control flow uniform), never write
    const RegsGlobal rf = {regs, stride, ii, i};
    vm_run(plan, rf, sbuf, lane, i, ii, live, 1u, 0u, nullptr, 64u, proofs, proof_off, instances, committed, scalars, status, trace);
}
// P proofs per block (power of two, <= 64), register file in dynamic LDS: P * n_regs * 32 bytes
extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner_lds(H2vDevPlan plan, uint32_t n, uint32_t P, const uint8_t *__restrict__ proofs,
                          const uint64_t *__restrict__ proof_off, const uint8_t *__restrict__ instances,
                          const uint8_t *__restrict__ committed, uint32_t *__restrict__ scalars,
                          uint32_t *__restrict__ status, uint32_t *__restrict__ trace) {
    __shared__ uint32_t sbuf[32 * 64];
    __shared__ uint32_t st_red[64];
    const int lane = threadIdx.x;
    const uint32_t L = plan.vm_lanes;
    const uint32_t q = (uint32_t)lane & (P - 1);            // proof slot of the block
    const uint32_t sub = L > 1 ? ((uint32_t)lane / P) % L : 0u;   // which of the proof's lanes
    const uint32_t i = blockIdx.x * P + q;
    // P * L may be below 64 (fewer proofs per block = less LDS per block = more blocks resident per CU, chosen by the
    // launcher): lanes >= P * L shadow a lane of the same proof (same work, same values) and never write
    const bool live = (uint32_t)lane < P * L && i < n;
    const uint32_t ii = i < n ? i : n - 1;
    // a dead slot of the last block shadows proof n-1 but must not touch a live slot's registers: it owns slot q anyway
    const RegsLds rf = {P, q};
    vm_run(plan, rf, sbuf, lane, i, ii, live, L, sub, st_red, P, proofs, proof_off, instances, committed, scalars, status, trace);
}
// The two kernels above for a key whose transcript hash is the keyed blake2b-512 (same geometry, same arguments)
extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner_b512(H2vDevPlan plan, uint32_t n, uint32_t stride, const uint8_t *__restrict__ proofs,
                           const uint64_t *__restrict__ proof_off, const uint8_t *__restrict__ instances,
                           const uint8_t *__restrict__ committed, uint32_t *__restrict__ regs,
                           uint32_t *__restrict__ scalars, uint32_t *__restrict__ status, uint32_t *__restrict__ trace) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;
    const RegsGlobal rf = {regs, stride, ii, i};
    vm_run<RegsGlobal, H2V_TR_BLAKE2B_512>(plan, rf, sbuf, lane, i, ii, live, 1u, 0u, nullptr, 64u, proofs, proof_off, instances, committed, scalars, status, trace);
}
extern "C" __global__ void __launch_bounds__(64)
k_transcript_combiner_lds_b512(H2vDevPlan plan, uint32_t n, uint32_t P, const uint8_t *__restrict__ proofs,
                               const uint64_t *__restrict__ proof_off, const uint8_t *__restrict__ instances,
                               const uint8_t *__restrict__ committed, uint32_t *__restrict__ scalars,
                               uint32_t *__restrict__ status, uint32_t *__restrict__ trace) {
    __shared__ uint32_t sbuf[32 * 64];
    __shared__ uint32_t st_red[64];
    const int lane = threadIdx.x;
    const uint32_t L = plan.vm_lanes;
    const uint32_t q = (uint32_t)lane & (P - 1);
    const uint32_t sub = L > 1 ? ((uint32_t)lane / P) % L : 0u;
    const uint32_t i = blockIdx.x * P + q;
    const bool live = (uint32_t)lane < P * L && i < n;
    const uint32_t ii = i < n ? i : n - 1;
    const RegsLds rf = {P, q};
    vm_run<RegsLds, H2V_TR_BLAKE2B_512>(plan, rf, sbuf, lane, i, ii, live, L, sub, st_red, P, proofs, proof_off, instances, committed, scalars, status, trace);
}

// ============================================================================ K2: G1 decompression
// zcash compressed encoding (bls_utils.ak:17-49, CompressUncompress.hs:53-100): bit7 compressed, bit6 infinity,
// bit5 "y is the lexicographically larger root"; y = (x^3+4)^((p+1)/4).
// Slot n_points is the committed instance when the circuit has one.
// out: affine Montgomery x||y (24 dwords, (0,0) = infinity); valid[...] = 1 iff the encoding is a point of G1.
//
// TWO waves per 64 points (block = 128 threads, the role is wave-uniform), because the square root and the subgroup
// test are the two long serial chains and the second does not need y:
//   wave 0: y = c^((p+1)/4) with c = x^3 + 4, y^2 == c, sign selection; then the point's MSM window tables;
//   wave 1: r-torsion test sigma(P) == [-x^2]P carried to the isomorphic curve E': Y^2 = X^3 + 4c^3 through
//           (x, y) -> (y^2 x, y^3 y) = (c x, c^2), which is known without the root.  The a = 0 group law does not
//           involve b, and the isomorphism commutes with sigma (X -> beta X), so the test on E' is the test on E for
//           either root y; when c is a non-residue wave 0 rejects and this result is ignored.  c == 0 means y == 0,
//           a 2-torsion point: rejected.
// Recursion (IVC) adds two slots per proof whose x and sign(y) are rebuilt from public inputs
// (g1_from_coords, aiken_halo2/lib/bls_utils.ak:32-49; limb packing emitters/aiken.rs:705-741):
//     coordinate = (1 + i_hi * 2^224 + i_lo) mod p ,  point = decompress(x with the parity flag of y).
#define H2V_DEC_PTS 64
H2V_DN void acc_coordinate(Fp &r, const uint8_t *ins, uint32_t idx_hi, uint32_t idx_lo) {
    Fp part[2];
#pragma unroll 1
    for (int q = 0; q < 2; q++) {
        const uint8_t *p = ins + (size_t)(q == 0 ? idx_hi : idx_lo) * 32;
        Fr b, m;
#pragma unroll
        for (int l = 0; l < 8; l++)
            b.v[l] = (uint32_t)p[4 * l] | ((uint32_t)p[4 * l + 1] << 8) | ((uint32_t)p[4 * l + 2] << 16) | ((uint32_t)p[4 * l + 3] << 24);
        FrF::to_mont(m, b);       // public inputs are field elements: reduced mod r exactly as LOAD_INSTANCE does
        FrF::from_mont(b, m);
        Fp plain;
#pragma unroll
        for (int l = 0; l < 12; l++) plain.v[l] = l < 8 ? b.v[l] : 0u;
        fp_to_mont(part[q], plain);
    }
    Fp c, one;
#pragma unroll
    for (int l = 0; l < 12; l++) c.v[l] = FP_TWO224[l];
    fp_set_one(one);
    fp_mul(r, part[0], c);
    fp_add(r, r, part[1]);
    fp_add(r, r, one);
}
// one group of 64 points (one wave): `role` 0 = square root (+ window tables), 1 = subgroup test
H2V_DI void dec_group(const H2vDevPlan &plan, uint32_t n, const uint8_t *__restrict__ proofs, const uint64_t *__restrict__ proof_off,
                      const uint8_t *__restrict__ committed, const uint8_t *__restrict__ instances,
                      uint32_t *__restrict__ pts, uint8_t *__restrict__ valid, uint32_t *__restrict__ pt_tab /* or NULL */,
                      const uint32_t mode, uint8_t *__restrict__ valid_sub, const uint32_t group, const uint32_t role,
                      const uint32_t lane, uint8_t *sub_ok) {
    // mode 0: both roles in one 128-thread block (valid = on curve && in G1);  modes 1 / 2: one role per wave, so that
    // the two chains can be scheduled apart: 1 = square root + tables (valid = encoding / on curve), 2 = subgroup test
    // (valid_sub)
    const uint32_t slots = H2V_SLOTS(plan);
    const uint32_t gid = group * H2V_DEC_PTS + lane;
    const bool live = gid < n * slots;
    const uint32_t gg = live ? gid : 0;
    const uint32_t i = gg / slots, j = gg - i * slots;
    bool ok = live;
    const uint8_t *src = nullptr;
    const bool is_acc = j >= plan.n_points + plan.n_ci;
    if (j < plan.n_points) {
        const uint64_t off0 = proof_off[i];
        if (proof_off[i + 1] - off0 < plan.proof_len) ok = false;  // short proof: nothing to read
        else src = proofs + off0 + plan.points[j];
    } else if (!is_acc) {
        src = committed + (size_t)i * 48;
    }
    uint32_t w[12];  // big-endian bytes -> little-endian limbs
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = 0;
    Fp acc_x;
    fp_set_zero(acc_x);
    if (is_acc) {
        // accumulator point: x (already a field element) and the parity of y; never the infinity encoding
        const uint32_t s4 = 4 * (j - plan.n_points - plan.n_ci);
        const uint8_t *ins = instances + (size_t)i * plan.n_pi * 32;
        Fp cy;
        acc_coordinate(acc_x, ins, plan.acc_idx[s4 + 0], plan.acc_idx[s4 + 1]);
        acc_coordinate(cy, ins, plan.acc_idx[s4 + 2], plan.acc_idx[s4 + 3]);
        w[11] = (4u | (fp_is_lex_larger(cy) ? 1u : 0u)) << 29;   // flags only; the limbs below stay unused
    } else if (ok) {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const uint8_t *p = src + 44 - 4 * k;
            w[k] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
        }
    }
    const uint32_t flags = w[11] >> 29;
    w[11] &= 0x1fffffffu;
    G1A out;
    g1a_set_inf(out);
    ok = ok && (flags & 4) != 0;
    bool finite = false;
    if (ok && (flags & 2)) {
        // infinity: all other bits must be clear
        uint32_t any = flags & 1;
#pragma unroll
        for (int k = 0; k < 12; k++) any |= w[k];
        ok = any == 0;
    } else if (ok) {
        ok = is_acc || !FpF::geq_mod(w);
        finite = ok;
    }
    if (finite) {
        Fp x, c, t, b4;
#pragma unroll
        for (int k = 0; k < 12; k++) { t.v[k] = w[k]; b4.v[k] = FP_B[k]; }
        fp_to_mont(x, t);
        if (is_acc) x = acc_x;
        fp_sqr(c, x); fp_mul(c, c, x); fp_add(c, c, b4);
        if (role == 0) {
            Fp y, chk;
            {
                F28 c28, y28;
                f28_from_fp(c28, c);
                f28_sqrt_chain(y28, c28);
                f28_to_fp(y, y28);
            }
            fp_sqr(chk, y);
            ok = fp_eq(chk, c);
            if (ok) {
                if (fp_is_lex_larger(y) != ((flags & 1) != 0)) fp_neg(y, y);
                out.x = x; out.y = y;
                // this wave is done at ~55 % of the subgroup wave's chain: it spends the slack on the MSM's window
                // tables of the point ([1..8]P and [1..8]phi(P), affine), which depend on the point alone
                if (pt_tab) g1_build_window_tables_glv(pt_tab + (size_t)gid * 448, out);
            }
        } else {
            ok = !fp_is_zero(c);
            if (ok) {
                G1A q;
                fp_mul(q.x, c, x);
                fp_sqr(q.y, c);
                ok = g1a_in_subgroup28(q);
            }
        }
    }
    if (mode == 2) {
        if (live) valid_sub[gid] = ok ? 1 : 0;
        return;
    }
    if (mode == 0) {
        if (role == 1) sub_ok[lane] = ok ? 1 : 0;
        __syncthreads();
    }
    if (role == 0 && live) {
        if (mode == 0) ok = ok && sub_ok[lane] != 0;
        if (!ok) g1a_set_inf(out);
#pragma unroll
        for (int k = 0; k < 12; k++) { pts[(size_t)gid * 24 + k] = out.x.v[k]; pts[(size_t)gid * 24 + 12 + k] = out.y.v[k]; }
        valid[gid] = ok ? 1 : 0;
    }
}

extern "C" __global__ void __launch_bounds__(128, 2)
k_g1_decompress(H2vDevPlan plan, uint32_t n, const uint8_t *__restrict__ proofs, const uint64_t *__restrict__ proof_off,
                const uint8_t *__restrict__ committed, const uint8_t *__restrict__ instances,
                uint32_t *__restrict__ pts, uint8_t *__restrict__ valid, uint32_t *__restrict__ pt_tab /* or NULL */,
                uint32_t mode, uint8_t *__restrict__ valid_sub) {
    __shared__ uint8_t sub_ok[H2V_DEC_PTS];
    const uint32_t role = mode == 0 ? threadIdx.x >> 6 : mode - 1;
    dec_group(plan, n, proofs, proof_off, committed, instances, pts, valid, pt_tab, mode, valid_sub, blockIdx.x, role, threadIdx.x & 63, sub_ok);
}
// The same work from a queue: the launch has at most one wave per SIMD (256-thread blocks: four waves, one per SIMD of
// a CU) and every wave takes the next 64-point unit until none is left - the n_groups subgroup tests first (the longer
// chain), then the n_groups square roots.  Separate launches left the pairing of waves on SIMDs to the dispatcher: some
// subgroup waves shared a SIMD with a root wave for their whole life and finished at 1.45 ms while most SIMDs idled
// from 1.06 ms on.  `counter` is zeroed by the host before the launch; a wave leaves when the counter passes the end.
extern "C" __global__ void __launch_bounds__(256, 2)
k_g1_decompress_queue(H2vDevPlan plan, uint32_t n, const uint8_t *__restrict__ proofs, const uint64_t *__restrict__ proof_off,
                      const uint8_t *__restrict__ committed, const uint8_t *__restrict__ instances,
                      uint32_t *__restrict__ pts, uint8_t *__restrict__ valid, uint32_t *__restrict__ pt_tab,
                      uint8_t *__restrict__ valid_sub, uint32_t *__restrict__ counter, uint32_t n_groups) {
    const uint32_t lane = threadIdx.x & 63;
    for (;;) {
        uint32_t u = 0;
        if (lane == 0) u = atomicAdd(counter, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= 2 * n_groups) break;
        if (u < n_groups) dec_group(plan, n, proofs, proof_off, committed, instances, pts, valid, pt_tab, 2u, valid_sub, u, 1u, lane, nullptr);
        else dec_group(plan, n, proofs, proof_off, committed, instances, pts, valid, pt_tab, 1u, valid_sub, u - n_groups, 0u, lane, nullptr);
    }
}

// ============================================================================ K4: per-proof G1 MSM
#include "h2v_msm.hpp"

// ============================================================================ K5: pairing check
// accept <=> e(el, s_g2) == e(er, G2)  (verification_h2.hbs:125-128), evaluated as
//   FE( ML(el; lines(s_g2)) * ML(-er; lines(G2)) ) == 1 .
// Both G2 arguments are fixed per plan, so their Miller-loop line coefficients (lambda, c) are precomputed at
// plan-compile time; with the untwist (x,y)->(x/w^2, y/w^3) a line at P=(xP,yP), scaled by w^3 (subfield
// element, killed by the final exponentiation), is  c + (-lambda xP) w^2 + yP w^3.
// Final exponentiation: easy part (p^6-1)(p^2+1); hard part via
//   3 (p^4-p^2+1)/r = (x-1)^2 (x+p)(x^2+p^2-1) + 3      (factor 3 is coprime to r: "== 1" unchanged).
H2V_DI void load_line(Fp2 &lam, Fp2 &c, const uint32_t *tab, int idx) {
    const uint32_t *p = tab + (size_t)idx * 48;
#pragma unroll
    for (int k = 0; k < 12; k++) { lam.c0.v[k] = p[k]; lam.c1.v[k] = p[12 + k]; c.c0.v[k] = p[24 + k]; c.c1.v[k] = p[36 + k]; }
}
H2V_DN void miller_loop(Fp12 &f, const G1A &p1, const uint32_t *lines1, bool skip1, const G1A &p2, const uint32_t *lines2, bool skip2) {
    fp12_set_one(f);
    int n = 0;
    Fp2 lam, c, b;
    for (int i = 62; i >= 0; i--) {
        fp12_sqr(f, f);
        const int steps = ((BLS_X_ABS >> i) & 1) ? 2 : 1;
        for (int s = 0; s < steps; s++) {
            if (!skip1) {
                load_line(lam, c, lines1, n);
                fp2_mul_fp(b, lam, p1.x); fp2_neg(b, b);
                fp12_mul_line(f, c, b, p1.y);
            }
            if (!skip2) {
                load_line(lam, c, lines2, n);
                fp2_mul_fp(b, lam, p2.x); fp2_neg(b, b);
                fp12_mul_line(f, c, b, p2.y);
            }
            n++;
        }
    }
    fp12_conj(f, f);  // x < 0
}
// a^x for a in the cyclotomic subgroup (x negative: conjugate)
H2V_DN void fp12_exp_x(Fp12 &r, const Fp12 &a) {
    Fp12 acc = a;
    for (int i = 62; i >= 0; i--) {
        fp12_sqr(acc, acc);
        if ((BLS_X_ABS >> i) & 1) fp12_mul(acc, acc, a);
    }
    fp12_conj(r, acc);
}
// (out, optional: the final value, for the probe's dump; f itself - zero - where f has no inverse)
H2V_DN bool final_exp_is_one(const Fp12 &f, Fp12 *out = nullptr) {
    Fp12 t, a, u, t0, t1, t2, t3;
    if (!fp12_inv(a, f)) { if (out) *out = f; return false; }
    fp12_conj(t, f); fp12_mul(t, t, a);                       // f^(p^6-1)
    fp12_frob(a, t); fp12_frob(a, a); fp12_mul(t, a, t);      // ^(p^2+1)
    fp12_exp_x(a, t); fp12_conj(u, t); fp12_mul(t0, a, u);    // t^(x-1)
    fp12_exp_x(a, t0); fp12_conj(u, t0); fp12_mul(t1, a, u);  // ^(x-1)
    fp12_exp_x(a, t1); fp12_frob(u, t1); fp12_mul(t2, a, u);  // ^(x+p)
    fp12_exp_x(a, t2); fp12_exp_x(a, a);
    fp12_frob(u, t2); fp12_frob(u, u); fp12_mul(t3, a, u);
    fp12_conj(u, t2); fp12_mul(t3, t3, u);                    // ^(x^2+p^2-1)
    fp12_sqr(u, t); fp12_mul(u, u, t);                        // t^3
    fp12_mul(t3, t3, u);
    if (out) *out = t3;
    return fp12_is_one(t3);
}

extern "C" __global__ void __launch_bounds__(64)
k_pairing_check(H2vDevPlan plan, uint32_t n, const uint32_t *__restrict__ pts, const uint8_t *__restrict__ valid, const uint8_t *__restrict__ valid_sub,
                const uint32_t *__restrict__ er_jac, const uint32_t *__restrict__ el_jac /* folded el (recursion) or NULL */,
                uint32_t *__restrict__ status, uint8_t *__restrict__ accept, uint32_t *__restrict__ dbg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slots = H2V_SLOTS(plan);
    uint32_t st = status[i];
    for (uint32_t j = 0; j < slots; j++)
        if (!valid[(size_t)i * slots + j] || (valid_sub && !valid_sub[(size_t)i * slots + j])) st |= H2V_ST_BAD_POINT;
    if (st == 0) {
        G1A el, er;
        G1J ej;
        const uint32_t *pp = pts + ((size_t)i * slots + plan.pi_point) * 24;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            el.x.v[k] = pp[k]; el.y.v[k] = pp[12 + k];
            ej.x.v[k] = er_jac[(size_t)i * 36 + k]; ej.y.v[k] = er_jac[(size_t)i * 36 + 12 + k]; ej.z.v[k] = er_jac[(size_t)i * 36 + 24 + k];
        }
        g1j_to_affine(er, ej);
        if (el_jac) {
#pragma unroll
            for (int k = 0; k < 12; k++) { ej.x.v[k] = el_jac[(size_t)i * 36 + k]; ej.y.v[k] = el_jac[(size_t)i * 36 + 12 + k]; ej.z.v[k] = el_jac[(size_t)i * 36 + 24 + k]; }
            g1j_to_affine(el, ej);
        }
        const bool el_inf = g1a_is_inf(el), er_inf = g1a_is_inf(er);
        fp_neg(er.y, er.y);  // -er (harmless on the infinity sentinel: skipped below)
        Fp12 f;
        miller_loop(f, el, plan.lines_sg2, el_inf, er, plan.lines_g2, er_inf);
        // records 0..11: f after the Miller loop, 12..23: after the final exponentiation; flat order (k, part): tower
        // c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)
        auto dump = [&](const Fp12 &v, int rec0) {
            const Fp2 *co[6] = {&v.c0.c0, &v.c1.c0, &v.c0.c1, &v.c1.c1, &v.c0.c2, &v.c1.c2};
            for (int k = 0; k < 6; k++) {
                Fp o0, o1;
                fp_from_mont(o0, co[k]->c0);
                fp_from_mont(o1, co[k]->c1);
                for (int q = 0; q < 12; q++) { dbg[((size_t)i * 24 + rec0 + 2 * k) * 12 + q] = o0.v[q]; dbg[((size_t)i * 24 + rec0 + 2 * k + 1) * 12 + q] = o1.v[q]; }
            }
        };
        if (dbg) dump(f, 0);
        Fp12 fin;
        if (!final_exp_is_one(f, dbg ? &fin : nullptr)) st |= H2V_ST_PAIRING;
        if (dbg) dump(fin, 12);
    }
    status[i] = st;
    accept[i] = st == 0 ? 1 : 0;
}

// ============================================================================ K4b: recursion (IVC) batching challenge
// c = LE(blake2b_256(compress(el) || compress(er) || compress(acc_left) || compress(acc_right_final))) mod r
// (emitters/aiken.rs:743-748).  One lane per proof: the three Jacobian sums are normalised with ONE inversion
// (Montgomery's trick), compressed (x big-endian + flags, sign = "y > (p-1)/2"), hashed, and the four affine points and
// the scalars {1, c, 1, c} are written for the two fold MSMs  el' = el + c acc_left ,  er' = er + c acc_right_final.
H2V_DN void g1_compress_dev(uint8_t (&out)[48], const G1A &a) {
    if (g1a_is_inf(a)) {
#pragma unroll
        for (int k = 0; k < 48; k++) out[k] = 0;
        out[0] = 0xc0;
        return;
    }
    Fp x;
    fp_from_mont(x, a.x);
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const uint32_t wv = x.v[11 - k];
        out[4 * k] = wv >> 24; out[4 * k + 1] = wv >> 16; out[4 * k + 2] = wv >> 8; out[4 * k + 3] = wv;
    }
    out[0] |= fp_is_lex_larger(a.y) ? 0xa0 : 0x80;
}
// Affine forms of N Jacobian points with ONE field inversion (Montgomery's trick).  A point at infinity contributes Z := 1 to
// the product, so the product is never zero, and comes out as the affine infinity sentinel.  Used by k_ivc_challenge (its
// three sums) and k_prepare_export (the pair L, R).
template <int N>
H2V_DI void g1j_to_affine_batch(G1A *out, const G1J *j) {
    Fp z[N], pre[N], inv, t;
    bool inf[N];
    for (int q = 0; q < N; q++) {
        inf[q] = g1j_is_inf(j[q]);
        z[q] = j[q].z;
        if (inf[q]) fp_set_one(z[q]);
    }
    pre[0] = z[0];
    for (int q = 1; q < N; q++) fp_mul(pre[q], pre[q - 1], z[q]);
    (void)fp_inv(inv, pre[N - 1]);          // never zero: every factor is a non-zero Z or 1
    for (int q = N - 1; q >= 0; q--) {
        Fp zi;
        if (q > 0) { fp_mul(zi, inv, pre[q - 1]); fp_mul(t, inv, z[q]); inv = t; } else zi = inv;
        G1A &o = out[q];
        if (inf[q]) { g1a_set_inf(o); continue; }
        Fp zi2;
        fp_sqr(zi2, zi);
        fp_mul(o.x, j[q].x, zi2);
        fp_mul(zi2, zi2, zi);
        fp_mul(o.y, j[q].y, zi2);
    }
}
extern "C" __global__ void __launch_bounds__(64)
k_ivc_challenge(H2vDevPlan plan, uint32_t n, const uint32_t *__restrict__ pts, const uint32_t *__restrict__ er_jac,
                const uint32_t *__restrict__ accl_jac, const uint32_t *__restrict__ accr_jac,
                uint32_t *__restrict__ fold_pts /* n x 4 x 24 */, uint32_t *__restrict__ fold_scal /* n x 4 x 8 */) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;
    const uint32_t slots = H2V_SLOTS(plan);
    G1A p[4];   // el, er, acc_left, acc_right_final
    {
        const uint32_t *pp = pts + ((size_t)ii * slots + plan.pi_point) * 24;
#pragma unroll
        for (int k = 0; k < 12; k++) { p[0].x.v[k] = pp[k]; p[0].y.v[k] = pp[12 + k]; }
    }
    {
        // batch normalisation of the three Jacobian points (g1j_to_affine_batch: one inversion)
        G1J j[3];
        const uint32_t *src[3] = {er_jac, accl_jac, accr_jac};
        for (int q = 0; q < 3; q++) {
#pragma unroll
            for (int k = 0; k < 12; k++) { j[q].x.v[k] = src[q][(size_t)ii * 36 + k]; j[q].y.v[k] = src[q][(size_t)ii * 36 + 12 + k]; j[q].z.v[k] = src[q][(size_t)ii * 36 + 24 + k]; }
        }
        g1j_to_affine_batch<3>(p + 1, j);
    }
    Transcript tr;
    tr_init(tr);
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        uint8_t enc[48];
        g1_compress_dev(enc, p[q]);
#pragma unroll 1
        for (int k = 0; k < 48; k++) tr_put(tr, sbuf, lane, enc[k]);
    }
    uint64_t h[4];
    tr_digest(tr, sbuf, lane, h);
    Fr c, cm;
#pragma unroll
    for (int l = 0; l < 4; l++) { c.v[2 * l] = (uint32_t)h[l]; c.v[2 * l + 1] = (uint32_t)(h[l] >> 32); }
    FrF::to_mont(cm, c);     // reduces the 256-bit integer mod r
    FrF::from_mont(c, cm);
    if (live) {
        const int order[4] = {0, 2, 1, 3};   // fold points: el, acc_left, er, acc_right_final
#pragma unroll 1
        for (int q = 0; q < 4; q++) {
            const G1A &o = p[order[q]];
            uint32_t *dp = fold_pts + ((size_t)i * 4 + q) * 24;
            uint32_t *ds = fold_scal + ((size_t)i * 4 + q) * 8;
#pragma unroll
            for (int k = 0; k < 12; k++) { dp[k] = o.x.v[k]; dp[12 + k] = o.y.v[k]; }
#pragma unroll
            for (int l = 0; l < 8; l++) ds[l] = (q & 1) ? c.v[l] : (l == 0 ? 1u : 0u);
        }
    }
}

// ============================================================================ K5': prepare (the pairing's two points, exported)
// What the pairing kernels would check for proof i, written out instead: L = the proof's pi point (or the folded el' of a
// recursive plan), R = er (or the folded er').  status folds valid / valid_sub into H2V_ST_BAD_POINT exactly as the pairing
// kernels do; a proof whose status is not 0 gets 96 zero bytes, which is not a valid encoding (compression flag unset).
// Otherwise pairs[i] = compress(L) || compress(R), normalised with one inversion (g1j_to_affine_batch) and written as 24
// dword stores (pairs: n x 24 dwords, 4-byte aligned).
extern "C" __global__ void __launch_bounds__(64)
k_prepare_export(H2vDevPlan plan, uint32_t n, const uint32_t *__restrict__ pts, const uint8_t *__restrict__ valid, const uint8_t *__restrict__ valid_sub,
                 const uint32_t *__restrict__ er_jac, const uint32_t *__restrict__ el_jac /* folded el (recursion) or NULL */,
                 uint32_t *__restrict__ status, uint32_t *__restrict__ pairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slots = H2V_SLOTS(plan);
    uint32_t st = status[i];
    for (uint32_t j = 0; j < slots; j++)
        if (!valid[(size_t)i * slots + j] || (valid_sub && !valid_sub[(size_t)i * slots + j])) st |= H2V_ST_BAD_POINT;
    status[i] = st;
    uint32_t words[24];
#pragma unroll
    for (int k = 0; k < 24; k++) words[k] = 0;
    if (st == 0) {
        G1J j[2];
        if (el_jac) {
#pragma unroll
            for (int k = 0; k < 12; k++) { j[0].x.v[k] = el_jac[(size_t)i * 36 + k]; j[0].y.v[k] = el_jac[(size_t)i * 36 + 12 + k]; j[0].z.v[k] = el_jac[(size_t)i * 36 + 24 + k]; }
        } else {
            G1A l;
            const uint32_t *pp = pts + ((size_t)i * slots + plan.pi_point) * 24;
#pragma unroll
            for (int k = 0; k < 12; k++) { l.x.v[k] = pp[k]; l.y.v[k] = pp[12 + k]; }
            g1j_from_affine(j[0], l);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) { j[1].x.v[k] = er_jac[(size_t)i * 36 + k]; j[1].y.v[k] = er_jac[(size_t)i * 36 + 12 + k]; j[1].z.v[k] = er_jac[(size_t)i * 36 + 24 + k]; }
        G1A a[2];
        g1j_to_affine_batch<2>(a, j);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            uint8_t enc[48];
            g1_compress_dev(enc, a[q]);
#pragma unroll
            for (int k = 0; k < 12; k++)
                words[12 * q + k] = (uint32_t)enc[4 * k] | ((uint32_t)enc[4 * k + 1] << 8) | ((uint32_t)enc[4 * k + 2] << 16) | ((uint32_t)enc[4 * k + 3] << 24);
        }
    }
    uint32_t *o = pairs + (size_t)i * 24;
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = words[k];
}
// The pair check's R as the pairing kernels take it: slot 1 of each two-slot record of `pts` (affine) -> Jacobian (n x 36 dwords)
// skip (the fall-back of the pairs' batch check, or NULL): return at once when *skip != 0
extern "C" __global__ void __launch_bounds__(64)
k_pairs_to_jac(uint32_t n, const uint32_t *__restrict__ pts, uint32_t *__restrict__ er_jac, const uint32_t *__restrict__ skip) {
    if (skip && skip[0]) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A a;
    const uint32_t *pp = pts + ((size_t)i * 2 + 1) * 24;
#pragma unroll
    for (int k = 0; k < 12; k++) { a.x.v[k] = pp[k]; a.y.v[k] = pp[12 + k]; }
    G1J j;
    g1j_from_affine(j, a);
    uint32_t *o = er_jac + (size_t)i * 36;
#pragma unroll
    for (int k = 0; k < 12; k++) { o[k] = j.x.v[k]; o[12 + k] = j.y.v[k]; o[24 + k] = j.z.v[k]; }
}

// ============================================================================ plan load: window tables of the VK bases
extern "C" __global__ void __launch_bounds__(64)
k_vk_tables(const uint32_t *__restrict__ vk_bases, uint32_t n, uint32_t *__restrict__ vk_tab) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    G1A base;
#pragma unroll
    for (int k = 0; k < 12; k++) { base.x.v[k] = vk_bases[(size_t)b * 24 + k]; base.y.v[k] = vk_bases[(size_t)b * 24 + 12 + k]; }
    if (g1a_is_inf(base)) return;   // the MSM skips an infinite base before it looks at the table
    g1_build_window_tables_glv(vk_tab + (size_t)b * 448, base);
}

// All-window tables of the VK bases for the fixed-base MSM lanes, window width c (4, 8, 12): for every base b and window w
// the multiples [e + 1] (2^(c w) V_b), e = 0 .. 2^(c-1) - 1, affine, at fix_tab[((b W + w) 2^(c-1) + e) 28 ...].  Plan-load
// work (once per key): the larger c is, the fewer additions a VK term costs in every proof (65 / 33 / 22 per base) - paid
// for in HBM, which this part has (c = 12: 5 MB per base).  Two launches: the window bases 2^(c w) V_b (one lane per
// (b, w): c w doublings), then one lane per table entry (double-and-add over the c - 1 bits of e + 1, one inversion).
extern "C" __global__ void __launch_bounds__(64)
k_vk_fixed_window_bases(const uint32_t *__restrict__ vk_bases, uint32_t n, uint32_t c, uint32_t W, uint32_t *__restrict__ wbase /* [n][W][24] affine, Montgomery; all-zero = infinity */) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = t / W, w = t - b * W;
    if (b >= n) return;
    G1A base;
#pragma unroll
    for (int k = 0; k < 12; k++) { base.x.v[k] = vk_bases[(size_t)b * 24 + k]; base.y.v[k] = vk_bases[(size_t)b * 24 + 12 + k]; }
    uint32_t *dst = wbase + (size_t)t * 24;
    if (g1a_is_inf(base)) {
#pragma unroll
        for (int k = 0; k < 24; k++) dst[k] = 0;
        return;
    }
    G1J28 p;
    g1j28_from_affine(p, base);
#pragma unroll 1
    for (uint32_t q = 0; q < c * w; q++) g1j28_dbl_ool(p, p);   // a point of prime order: never infinity
    G1J pj;
    g1j28_to_g1j(pj, p, false);
    G1A aff;
    g1j_to_affine(aff, pj);
#pragma unroll
    for (int k = 0; k < 12; k++) { dst[k] = aff.x.v[k]; dst[12 + k] = aff.y.v[k]; }
}
extern "C" __global__ void __launch_bounds__(64)
k_vk_fixed_tables(const uint32_t *__restrict__ wbase, uint32_t n_bw /* bases x windows */, uint32_t c, uint32_t *__restrict__ fix_tab) {
    const uint32_t E = 1u << (c - 1);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t bw = (uint32_t)(t / E), e = (uint32_t)(t - (uint64_t)bw * E);
    if (bw >= n_bw) return;
    G1A base;
    const uint32_t *src = wbase + (size_t)bw * 24;
#pragma unroll
    for (int k = 0; k < 12; k++) { base.x.v[k] = src[k]; base.y.v[k] = src[12 + k]; }
    if (g1a_is_inf(base)) return;             // (the MSM skips an infinite base before it looks at the table)
    G1J28 p, acc;
    g1j28_from_affine(p, base);
    bool inf = true;
    const uint32_t m = e + 1;                 // 1 .. 2^(c-1): up to c bits
#pragma unroll 1
    for (int bit = (int)c - 1; bit >= 0; bit--) {
        if (!inf) g1j28_dbl_ool(acc, acc);
        if ((m >> bit) & 1u) g1j28_acc_add(acc, inf, p, false);   // complete (m = 2: P + P)
    }
    G1J pj;
    g1j28_to_g1j(pj, acc, inf);
    G1A aff;
    g1j_to_affine(aff, pj);
    F28 x, y;
    f28_from_fp(x, aff.x);
    f28_from_fp(y, aff.y);
    g1_store_table_entry(fix_tab + (size_t)t * 28, x, y);
}

// ============================================================================ primitive probes (parity tests)
// op: 0 fp_mul, 1 fp_add, 2 fp_sub, 3 fp_inv, 4 fr_mul, 5 fr_inv (a, b canonical little-endian limbs; 12 or 8)
extern "C" __global__ void k_probe_field(int op, uint32_t n, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                         uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op < 4) {
        Fp x, y, r;
#pragma unroll
        for (int k = 0; k < 12; k++) { x.v[k] = a[(size_t)i * 12 + k]; y.v[k] = b[(size_t)i * 12 + k]; }
        fp_to_mont(x, x); fp_to_mont(y, y);
        if (op == 0) fp_mul(r, x, y);
        else if (op == 1) fp_add(r, x, y);
        else if (op == 2) fp_sub(r, x, y);
        else fp_inv(r, x);
        fp_from_mont(r, r);
#pragma unroll
        for (int k = 0; k < 12; k++) out[(size_t)i * 12 + k] = r.v[k];
    } else {
        Fr x, y, r;
#pragma unroll
        for (int k = 0; k < 8; k++) { x.v[k] = a[(size_t)i * 8 + k]; y.v[k] = b[(size_t)i * 8 + k]; }
        FrF::to_mont(x, x); FrF::to_mont(y, y);
        if (op == 4) fr_mul(r, x, y);
        else fr_inv(r, x);
        FrF::from_mont(r, r);
#pragma unroll
        for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = r.v[k];
    }
}
// dev probe: 2P + (neg ? -Q : Q) by the one-lane mixed addition and by the quad-cooperative one (P, Q affine canonical limbs);
// out: 5 x 42 dwords of raw lazily reduced limbs: the one-lane result, then the quad's lanes 0..3
extern "C" __global__ void __launch_bounds__(64)
k_probe_quad_madd(const uint32_t *__restrict__ pq, int neg, uint32_t *__restrict__ out) {
    G1A P, Q;
#pragma unroll
    for (int k = 0; k < 12; k++) { P.x.v[k] = pq[k]; P.y.v[k] = pq[12 + k]; Q.x.v[k] = pq[24 + k]; Q.y.v[k] = pq[36 + k]; }
    fp_to_mont(P.x, P.x); fp_to_mont(P.y, P.y); fp_to_mont(Q.x, Q.x); fp_to_mont(Q.y, Q.y);
    G1J28 p1, p2, a, b;
    g1j28_from_affine(p1, P);
    g1j28_dbl(p2, p1);
    F28 qx, qy;
    f28_from_fp(qx, Q.x);
    f28_from_fp(qy, Q.y);
    g1j28_madd_ladder(a, p2, qx, qy, neg != 0);
    b = p2;
    g1j28_madd_quad(b, qx, qy, neg != 0);
    const int l = threadIdx.x;
    if (l == 0)
        for (int k = 0; k < 14; k++) { out[k] = a.x.l[k]; out[14 + k] = a.y.l[k]; out[28 + k] = a.z.l[k]; }
    if (l < 4)
        for (int k = 0; k < 14; k++) { out[42 * (1 + l) + k] = b.x.l[k]; out[42 * (1 + l) + 14 + k] = b.y.l[k]; out[42 * (1 + l) + 28 + k] = b.z.l[k]; }
}
// dev probe of the merged products and of the three one-lane group formulas built on them, on RAW lazily reduced records (14
// limbs of 28 bits that may be uncarried: the bounds of h2v_fp28.hpp are the caller's to respect - or to sit on).
//   op & 15:  0: a b + c d   1: a^2 + c d   2: 2 a^2 + c d          (records of 14 dwords in a, b, c, d; out: 14 dwords)
//             3: a b         4: a^2           (the plain product and squaring, fp_mont28 / fp_montsqr28; c, d read and unused)
//             8: 2P          9: P + Q, Q affine (mixed)   10: P + Q  (P = 42 dwords X, Y, Z in a, Q likewise in b; out: 44 dwords:
//                                                                     X, Y, Z, the return code of g1j28_add, 0)
//   op & 16:  the inlined multiplier forms (ops 0..4, 8, 9)      op & 64: subtract Q (ops 9, 10)
extern "C" __global__ void __launch_bounds__(64)
k_probe_f28_dot2(int op, uint32_t n, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const uint32_t *__restrict__ c,
                 const uint32_t *__restrict__ d, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int what = op & 15;
    const bool inl = (op & 16) != 0, neg = (op & 64) != 0;
    if (what < 8) {
        F28 x, y, u, v, r;
#pragma unroll
        for (int k = 0; k < 14; k++) { x.l[k] = a[(size_t)i * 14 + k]; y.l[k] = b[(size_t)i * 14 + k]; u.l[k] = c[(size_t)i * 14 + k]; v.l[k] = d[(size_t)i * 14 + k]; }
        if (what == 0) { if (inl) f28_dot2_inl(r, x, y, u, v); else f28_dot2(r, x, y, u, v); }
        else if (what == 1) { if (inl) f28_dot2_sqr_inl<1>(r, x, u, v); else f28_dot2_sqr<1>(r, x, u, v); }
        else if (what == 2) { if (inl) f28_dot2_sqr_inl<2>(r, x, u, v); else f28_dot2_sqr<2>(r, x, u, v); }
        else if (what == 3) { if (inl) f28_mul_inl(r, x, y); else f28_mul(r, x, y); }
        else { if (inl) f28_sqr_inl(r, x); else f28_sqr(r, x); }
#pragma unroll
        for (int k = 0; k < 14; k++) out[(size_t)i * 14 + k] = r.l[k];
        return;
    }
    G1J28 P, Q, r;
#pragma unroll
    for (int k = 0; k < 14; k++) {
        P.x.l[k] = a[(size_t)i * 42 + k]; P.y.l[k] = a[(size_t)i * 42 + 14 + k]; P.z.l[k] = a[(size_t)i * 42 + 28 + k];
        Q.x.l[k] = what == 8 ? 0u : b[(size_t)i * 42 + k]; Q.y.l[k] = what == 8 ? 0u : b[(size_t)i * 42 + 14 + k];
        Q.z.l[k] = what == 8 ? 0u : b[(size_t)i * 42 + 28 + k];
    }
    r = P;
    int rc = 0;
    if (what == 8) { if (inl) g1j28_dbl_t<true>(r, P); else g1j28_dbl_t<false>(r, P); }
    else if (what == 9) { if (inl) g1j28_madd_ladder_t<true>(r, P, Q.x, Q.y, neg); else g1j28_madd_ladder_t<false>(r, P, Q.x, Q.y, neg); }
    else rc = g1j28_add(r, P, Q, neg);
#pragma unroll
    for (int k = 0; k < 14; k++) { out[(size_t)i * 44 + k] = r.x.l[k]; out[(size_t)i * 44 + 14 + k] = r.y.l[k]; out[(size_t)i * 44 + 28 + k] = r.z.l[k]; }
    out[(size_t)i * 44 + 42] = (uint32_t)rc;
    out[(size_t)i * 44 + 43] = 0u;
}
// blake2b-256 of n messages of `len` bytes each through the LDS transcript path (one message per lane)
extern "C" __global__ void __launch_bounds__(64)
k_probe_blake2b(uint32_t n, uint32_t len, const uint8_t *__restrict__ msgs, uint32_t *__restrict__ out) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    const uint32_t ii = i < n ? i : n - 1;
    Transcript tr;
    tr_init(tr);
    for (uint32_t k = 0; k < len; k++) tr_put(tr, sbuf, lane, msgs[(size_t)ii * len + k]);
    uint64_t h[4];
    tr_digest(tr, sbuf, lane, h);
    if (i < n) {
#pragma unroll
        for (int k = 0; k < 4; k++) { out[(size_t)i * 8 + 2 * k] = (uint32_t)h[k]; out[(size_t)i * 8 + 2 * k + 1] = (uint32_t)(h[k] >> 32); }
    }
}

// A keyed / unkeyed blake2b of either width through the same path, from a state the host worked out (h0, t0: the parameter
// block, and the key block behind it when a message follows).  `prefix` (prefix_len bytes, 0 or 128) is hashed in front of
// every message: the key block itself when the message is empty - it is then the final block, and no mid-state applies.
struct H2vProbeHash { uint64_t h0[8]; uint32_t t0, prefix_len, digest_words; };
extern "C" __global__ void __launch_bounds__(64)
k_probe_blake2b_ex(uint32_t n, uint32_t len, const uint8_t *__restrict__ msgs, H2vProbeHash ph, const uint8_t *__restrict__ prefix,
                   uint32_t *__restrict__ out) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    const uint32_t ii = i < n ? i : n - 1;
    Transcript tr;
    tr_init_state(tr, ph.h0, ph.t0);
    for (uint32_t k = 0; k < ph.prefix_len; k++) tr_put(tr, sbuf, lane, prefix[k]);
    for (uint32_t k = 0; k < len; k++) tr_put(tr, sbuf, lane, msgs[(size_t)ii * len + k]);
    uint64_t h[8];
    tr_digest(tr, sbuf, lane, h);
    if (i < n) {
        const uint32_t dw = 2 * ph.digest_words;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)(2 * k) < dw) { out[(size_t)i * dw + 2 * k] = (uint32_t)h[k]; out[(size_t)i * dw + 2 * k + 1] = (uint32_t)(h[k] >> 32); }
    }
}

// affine (24 dwords) or Jacobian (36 dwords) Montgomery points -> 96 bytes x||y big-endian canonical (zero = infinity)
extern "C" __global__ void k_export_points(uint32_t n, int jacobian, const uint32_t *__restrict__ in, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1A a;
    if (jacobian) {
        G1J j;
#pragma unroll
        for (int k = 0; k < 12; k++) { j.x.v[k] = in[(size_t)i * 36 + k]; j.y.v[k] = in[(size_t)i * 36 + 12 + k]; j.z.v[k] = in[(size_t)i * 36 + 24 + k]; }
        g1j_to_affine(a, j);
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) { a.x.v[k] = in[(size_t)i * 24 + k]; a.y.v[k] = in[(size_t)i * 24 + 12 + k]; }
    }
    Fp x, y;
    fp_from_mont(x, a.x);
    fp_from_mont(y, a.y);
    uint8_t *o = out + (size_t)i * 96;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const uint32_t wx = x.v[11 - k], wy = y.v[11 - k];
        o[4 * k] = wx >> 24; o[4 * k + 1] = wx >> 16; o[4 * k + 2] = wx >> 8; o[4 * k + 3] = wx;
        o[48 + 4 * k] = wy >> 24; o[48 + 4 * k + 1] = wy >> 16; o[48 + 4 * k + 2] = wy >> 8; o[48 + 4 * k + 3] = wy;
    }
}

// ============================================================================ RLC batch mode + bucket MSM
#include "h2v_seed_dev.hpp"
#include "h2v_rlc.hpp"
#include "h2v_coalesce.hpp"
