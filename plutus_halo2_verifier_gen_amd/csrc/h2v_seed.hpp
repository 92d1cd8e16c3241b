// Derived batch seeds (H2V_RLC_SEED_TRANSCRIPT): what the host knows of the rule - the domain tags, the number of tree levels
// and where every level's digests lie in the call's digest buffer.  HOST CODE ONLY - no HIP call and no HIP header in this file,
// so that a stand-alone C++ program can include and test it (tests/cpp/h2v_seed_layout.cpp).  The kernels are in
// h2v_seed_dev.hpp; the rule itself is stated in DESIGN.md section 17 and restated in plutus_halo2_verifier_gen_amd/seed.py.
//
//   leaf_i = B(TAG leaf || LE32(|inst|) || LE32(|ci|) || LE32(|proof|) || LE32(0) || inst || ci || proof)
//   mleaf_i = B(TAG mleaf || the same four lengths || key_tag(plan of proof i) || inst || ci || proof)      form 3 (H2V_RLC_SEED_KEYED)
//   node   = B(TAG node || LE32(level) || LE32(m) || LE64(index) || child_0 .. child_{m-1})      64-ary, level 1 over the leaves
//   seed   = B(TAG root || LE32(form) || LE32(0) || LE64(n) || key_tag || top node)
// B: unkeyed blake2b-256.  A tag is its ASCII string zero-padded to 16 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace h2vseed {
constexpr uint32_t ARITY = 64;
constexpr uint64_t MAX_N = 1ull << 22;       // the RLC forms' own limit
constexpr uint32_t MAX_LEVELS = 4;           // 64^4 >= 2^22
constexpr uint32_t FORM_PROOFS = 1, FORM_PAIRS = 2, FORM_MIXED = 3;   // (3: keyed leaves, the mixed-key calls; its root hashes 32 zero bytes as key_tag)
constexpr size_t TAG_BYTES = 16, DIGEST_BYTES = 32;
constexpr char TAG_KEY[] = "h2v-seed-key/1";
constexpr char TAG_LEAF[] = "h2v-seed-leaf/1";
constexpr char TAG_MLEAF[] = "h2v-seed-mleaf/1";      // exactly 16 bytes: the keyed leaf's header is 64
constexpr char TAG_NODE[] = "h2v-seed-node/1";
constexpr char TAG_ROOT[] = "h2v-seed-root/1";
static_assert(sizeof TAG_KEY <= TAG_BYTES + 1 && sizeof TAG_LEAF <= TAG_BYTES + 1 && sizeof TAG_NODE <= TAG_BYTES + 1 && sizeof TAG_ROOT <= TAG_BYTES + 1 &&
                  sizeof TAG_MLEAF <= TAG_BYTES + 1,
              "a tag fits its 16 bytes");

// a tag as the four little-endian dwords the kernels put in front of a message
struct TagWords { uint32_t w[4]; };
static inline TagWords tag_words(const char *s) {
    uint8_t b[TAG_BYTES] = {};
    const size_t len = strlen(s);
    memcpy(b, s, len < TAG_BYTES ? len : TAG_BYTES);
    TagWords t{};
    for (int k = 0; k < 4; k++) t.w[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    return t;
}

// The digest buffer of one call, in digests of 32 bytes: the n leaves at 0, then level 1, level 2, ... each behind the one below.
// count[0] / off[0] are the leaves'; count[l] / off[l], l = 1 .. levels, the nodes of level l; count[levels] == 1.  n = 0 has no
// tree (levels = 0, extent 0): the calls return before they derive anything.
struct Tree {
    uint32_t levels;
    uint64_t count[MAX_LEVELS + 1], off[MAX_LEVELS + 1];
    uint64_t extent;                         // digests
};
static inline bool tree(uint64_t n, Tree *t) {
    memset(t, 0, sizeof *t);
    if (n == 0 || n > MAX_N) return n == 0;
    t->count[0] = n; t->off[0] = 0;
    uint64_t at = n, m = n;
    uint32_t l = 0;
    do {      // (n = 1 still has one level-1 node)
        if (l == MAX_LEVELS) return false;
        m = (m + ARITY - 1) / ARITY;
        l++;
        t->count[l] = m; t->off[l] = at;
        at += m;
    } while (m > 1);
    t->levels = l;
    t->extent = at;
    return true;
}
// children of node j of a level whose lower level has `below` entries
static inline uint32_t children(uint64_t below, uint64_t j) {
    const uint64_t lo = j * ARITY;
    return (uint32_t)(below - lo < ARITY ? below - lo : ARITY);
}
}   // namespace h2vseed
