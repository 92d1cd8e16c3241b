// Derived batch seeds (H2V_RLC_SEED_TRANSCRIPT): the digest kernels.  Included by h2v_kernels.hip in front of h2v_rlc.hpp (uses
// its blake2b compression); the rule and the layout of the digest buffer are in h2v_seed.hpp.
//
//   k_seed_leaves   one leaf per lane: blake2b-256 over the leaf's header and the proof's own bytes (instance row, committed
//                   row, proof bytes), fed as whole 128-byte blocks
//   k_seed_leaves_mixed   the same for the keyed leaves of a mixed-key call (H2V_RLC_SEED_KEYED, form 3): every leaf carries the
//                   key tag of its own proof's plan; the per-proof facts come from the call's table block
//   k_seed_nodes    one node per lane over up to 64 child digests; launched once per level, and the launch whose level holds ONE
//                   node goes on to hash the root and stores the call's seed
//
// MAPPING.  A leaf is a chain of ~9 dependent compressions for a 1.1 KB proof, a node one of 17: short, latency-bound chains with
// nothing to share between lanes.  One lane per proof in one-wave blocks: every lane owns a column of the block buffer in LDS
// (dword d of lane l at sbuf[d * 64 + l], conflict-free, no barrier anywhere), a batch of 4096 proofs is 64 independent waves on 64
// CUs, and more lanes per proof would only add LDS traffic to a chain whose length is the message's.  The block buffer is filled
// with dword loads: every section of a leaf starts at a multiple of 4 in the hashed stream, so a stream dword never spans two
// sections; where the SOURCE address is not 4-byte aligned (proof_off[i] has no alignment) an interior dword comes from the two
// aligned words around it, and only the dwords that touch the proof's first or last aligned word go byte by byte.  No byte outside
// [proof_off[i], proof_off[i+1]) and the proof's own instance and committed rows is read.
#pragma once

// bytes s[k .. k + 4) of a section of `len` bytes as a little-endian dword; bytes at or behind len read as zero.  k % 4 == 0.
H2V_DI uint32_t seed_sec_dword(const uint8_t *__restrict__ s, uint32_t k, uint32_t len) {
    const uint32_t m = (uint32_t)((uintptr_t)(s + k) & 3u);
    if (k + 4u <= len && k + 4u > k) {
        if (m == 0) return *reinterpret_cast<const uint32_t *>(s + k);
        if (k >= m && k - m + 8u <= len) {      // both aligned words lie inside the section
            const uint32_t lo = *reinterpret_cast<const uint32_t *>(s + k - m), hi = *reinterpret_cast<const uint32_t *>(s + k - m + 4);
            return (lo >> (8u * m)) | (hi << (32u - 8u * m));
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
        if (k + b < len && k + b >= k) v |= (uint32_t)s[k + b] << (8u * b);
    return v;
}
H2V_DI void seed_b2_init(uint64_t (&h)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = B2_IV[i];
    h[0] ^= 0x01010000ull ^ 32ull;      // digest 32, no key, fanout 1, depth 1
}

struct SeedLeafArgs {
    uint32_t n, inst_len, ci_len, pair_form;      // bytes of a proof's instance / committed row; pair_form: proof i = proofs[96 i .. 96 i + 96)
    const uint8_t *proofs;
    const uint64_t *off;                          // n + 1 entries (unused with pair_form)
    const uint8_t *inst, *ci;
    uint32_t tag[4];
    uint32_t *digests;                            // leaf i at dwords [8 i, 8 i + 8)
};
extern "C" __global__ void __launch_bounds__(64)
k_seed_leaves(SeedLeafArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64 + lane;
    if (i >= a.n) return;
    uint64_t lo, hi;
    if (a.pair_form) { lo = 96ull * i; hi = lo + 96; }
    else { lo = a.off[i]; hi = a.off[i + 1]; }
    // (a descending pair of offsets is an empty proof here, never a length that wraps; |proof| is hashed as LE32)
    const uint32_t plen = hi > lo ? (hi - lo > 0xffffffffull ? 0xffffffffu : (uint32_t)(hi - lo)) : 0u;
    const uint8_t *const proof = a.proofs + lo;
    const uint8_t *const inst = a.inst_len ? a.inst + (size_t)i * a.inst_len : nullptr;
    const uint8_t *const ci = a.ci_len ? a.ci + (size_t)i * a.ci_len : nullptr;
    const uint32_t at_ci = 32u + a.inst_len, at_proof = at_ci + a.ci_len;      // section starts in the hashed stream: multiples of 4
    const uint64_t total = (uint64_t)at_proof + plen;
    const uint64_t n_blocks = (total + 127) / 128;                             // >= 1: the header alone is 32 bytes
    uint64_t h[8];
    seed_b2_init(h);
#pragma unroll 1
    for (uint64_t b = 0; b < n_blocks; b++) {
#pragma unroll 1
        for (uint32_t d = 0; d < 32; d++) {
            const uint64_t p = b * 128 + 4ull * d;
            uint32_t w = 0;
            if (p >= at_proof) {
                if (p < total) w = seed_sec_dword(proof, (uint32_t)(p - at_proof), plen);
            } else if (p < 16) w = a.tag[p >> 2];
            else if (p < 32) w = p == 16 ? a.inst_len : p == 20 ? a.ci_len : p == 24 ? plen : 0u;
            else if (p < at_ci) w = seed_sec_dword(inst, (uint32_t)p - 32u, a.inst_len);
            else w = seed_sec_dword(ci, (uint32_t)p - at_ci, a.ci_len);
            sbuf[d * 64 + lane] = w;
        }
        const bool last = b + 1 == n_blocks;
        b2_compress_lds(h, sbuf + lane, last ? total : (b + 1) * 128, last);
    }
    uint32_t *out = a.digests + (size_t)i * 8;
#pragma unroll
    for (int q = 0; q < 4; q++) { out[2 * q] = (uint32_t)h[q]; out[2 * q + 1] = (uint32_t)(h[q] >> 32); }
}

// Form 3, keyed leaves (H2V_RLC_SEED_KEYED, the mixed-key calls): a leaf binds the key of its own proof,
//   mleaf_i = B(TAG mleaf || LE32(|inst|) || LE32(|ci|) || LE32(|proof|) || LE32(0) || key_tag(plan of i) || inst || ci || proof)
// - a 64-byte header, so every section still starts at a multiple of 4 in the hashed stream and the block fill is k_seed_leaves' -
// and what differs per proof comes from the call's table block (h2v_mixed_tables.hpp): the instance offset and length, the
// committed index (H2V_MIXED_NONE: none), the plan index, and the table of key tags by plan.
//
// ITERATION.  Lane l of block b takes GROUPED position g = 64 b + l and stores to digests[perm[g]]; the alternative - call positions
// with inverse tables - was weighed and left.  Grouped: the six table reads per lane are coalesced and are the partition's own
// arrays (only the plan index is new); the digest store is one whole aligned 32-byte sector per lane whatever its address, so
// scattering it costs no extra traffic; the two proof_off reads are gathered, 16 bytes per lane once per leaf.  Above all the lanes
// of a wave then hold proofs of ONE plan (but at a boundary), so their leaves have the same number of blocks and the wave runs no
// longer than its own proofs need - in the caller's order a wave runs as long as the longest proof of any key among its 64.
// The seed does not depend on the iteration order: leaf i lies at digests[i] either way.
struct SeedMixedLeafArgs {
    uint32_t n;
    const uint32_t *perm;                         // grouped position -> position in the call
    const uint64_t *inst_src;                     // byte offset of the proof's instance bytes in `inst`
    const uint32_t *inst_len, *ci_src, *plan_idx; // bytes; index of the 48-byte committed row or H2V_MIXED_NONE; plan in the call's list
    const uint32_t *key_tags;                     // 8 dwords per listed plan
    const uint8_t *proofs;
    const uint64_t *off;                          // the CALLER's proof_off, n + 1 entries, by position in the call
    const uint8_t *inst, *ci;
    uint32_t tag[4];
    uint32_t *digests;                            // leaf i (position in the call) at dwords [8 i, 8 i + 8)
};
extern "C" __global__ void __launch_bounds__(64)
k_seed_leaves_mixed(SeedMixedLeafArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x * 64 + lane;
    if (g >= a.n) return;
    const uint32_t i = a.perm[g];
    const uint64_t lo = a.off[i], hi = a.off[i + 1];
    const uint32_t plen = hi > lo ? (hi - lo > 0xffffffffull ? 0xffffffffu : (uint32_t)(hi - lo)) : 0u;      // (descending: empty)
    const uint32_t inst_len = a.inst_len[g], ci_at = a.ci_src[g], ci_len = ci_at == 0xffffffffu ? 0u : 48u;
    const uint8_t *const proof = a.proofs + lo;
    const uint8_t *const inst = inst_len ? a.inst + a.inst_src[g] : nullptr;
    const uint8_t *const ci = ci_len ? a.ci + (size_t)ci_at * 48 : nullptr;
    const uint32_t *const kt = a.key_tags + (size_t)a.plan_idx[g] * 8;
    const uint32_t at_ci = 64u + inst_len, at_proof = at_ci + ci_len;
    const uint64_t total = (uint64_t)at_proof + plen;
    const uint64_t n_blocks = (total + 127) / 128;
    uint64_t h[8];
    seed_b2_init(h);
#pragma unroll 1
    for (uint64_t b = 0; b < n_blocks; b++) {
#pragma unroll 1
        for (uint32_t d = 0; d < 32; d++) {
            const uint64_t p = b * 128 + 4ull * d;
            uint32_t w = 0;
            if (p >= at_proof) {
                if (p < total) w = seed_sec_dword(proof, (uint32_t)(p - at_proof), plen);
            } else if (p < 16) w = a.tag[p >> 2];
            else if (p < 32) w = p == 16 ? inst_len : p == 20 ? ci_len : p == 24 ? plen : 0u;
            else if (p < 64) w = kt[(p - 32) >> 2];
            else if (p < at_ci) w = seed_sec_dword(inst, (uint32_t)p - 64u, inst_len);
            else w = seed_sec_dword(ci, (uint32_t)p - at_ci, ci_len);
            sbuf[d * 64 + lane] = w;
        }
        const bool last = b + 1 == n_blocks;
        b2_compress_lds(h, sbuf + lane, last ? total : (b + 1) * 128, last);
    }
    uint32_t *out = a.digests + (size_t)i * 8;
#pragma unroll
    for (int q = 0; q < 4; q++) { out[2 * q] = (uint32_t)h[q]; out[2 * q + 1] = (uint32_t)(h[q] >> 32); }
}

struct SeedNodeArgs {
    uint32_t level, below, count;                 // `count` nodes over `below` entries of the level underneath
    const uint32_t *src;                          // the level underneath, 8 dwords per entry
    uint32_t *dst;                                // this level
    uint32_t tag[4];
    // the launch with count == 1 forms the call's seed behind its one node
    uint32_t form, n_lo, n_hi;
    uint32_t root_tag[4], key_tag[8];
    uint32_t *seed_out;                           // 8 dwords
};
extern "C" __global__ void __launch_bounds__(64)
k_seed_nodes(SeedNodeArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * 64 + lane;
    if (j >= a.count) return;
    const uint32_t first = j * 64u, m = a.below - first < 64u ? a.below - first : 64u;
    const uint32_t *const kids = a.src + (size_t)first * 8;
    const uint32_t words = 8u + 8u * m, total = 4u * words, n_blocks = (total + 127u) / 128u;
    uint64_t h[8];
    seed_b2_init(h);
#pragma unroll 1
    for (uint32_t b = 0; b < n_blocks; b++) {
#pragma unroll 1
        for (uint32_t d = 0; d < 32; d++) {
            const uint32_t q = b * 32u + d;
            uint32_t w = 0;
            if (q >= 8u) { if (q < words) w = kids[q - 8u]; }
            else if (q < 4u) w = a.tag[q];
            else w = q == 4u ? a.level : q == 5u ? m : q == 6u ? j : 0u;      // LE32(level) || LE32(m) || LE64(index)
            sbuf[d * 64 + lane] = w;
        }
        const bool last = b + 1 == n_blocks;
        b2_compress_lds(h, sbuf + lane, last ? total : (b + 1u) * 128u, last);
    }
    uint32_t *out = a.dst + (size_t)j * 8;
#pragma unroll
    for (int q = 0; q < 4; q++) { out[2 * q] = (uint32_t)h[q]; out[2 * q + 1] = (uint32_t)(h[q] >> 32); }
    if (a.count != 1) return;
    // seed = B(TAG root || LE32(form) || LE32(0) || LE64(n) || key_tag || top node): 96 bytes, one block
#pragma unroll 1
    for (uint32_t d = 0; d < 32; d++) {
        uint32_t w = 0;
        if (d < 4u) w = a.root_tag[d];
        else if (d < 8u) w = d == 4u ? a.form : d == 6u ? a.n_lo : d == 7u ? a.n_hi : 0u;
        else if (d < 16u) w = a.key_tag[d - 8u];
        else if (d < 24u) w = out[d - 16u];      // (this lane's own digest, just stored)
        sbuf[d * 64 + lane] = w;
    }
    uint64_t r[8];
    seed_b2_init(r);
    b2_compress_lds(r, sbuf + lane, 96, true);
#pragma unroll
    for (int q = 0; q < 4; q++) { a.seed_out[2 * q] = (uint32_t)r[q]; a.seed_out[2 * q + 1] = (uint32_t)(r[q] >> 32); }
}

// Word q of the seed a coefficient kernel hashes: the by-value seed of its arguments, or - seed_dev != NULL, a derived seed - the
// word in device memory, word 7 xored with the chunk's tweak.  Wave-uniform.
H2V_DI uint32_t seed_word(const uint32_t (&by_value)[8], const uint32_t *seed_dev, uint32_t seed_xor7, int q) {
    if (!seed_dev) return by_value[q];
    return seed_dev[q] ^ (q == 7 ? seed_xor7 : 0u);
}
