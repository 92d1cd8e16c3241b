// Host-buffer calls: where everything lies.  The input block a caller's batch is packed into before it goes up in one copy, and
// the result block a blocking host-buffer form has its kernels write before the results come down.  HOST CODE ONLY - no HIP call
// and no HIP header in this file, so that a stand-alone C++ program can include and test it (tests/cpp/h2v_hostcall_layout.cpp):
// every function is pure arithmetic on sizes, and the packer copies between host buffers.  h2v_capi.hip allocates what `need` /
// `extent` say and addresses the blocks through these offsets alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace hostcall {
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- the input block:  offsets | instances | committed | proofs,  every section at a multiple of 16, PAD zero bytes behind the
// proofs (the transcript kernel reads whole words past a proof's end).  offsets: n + 1 entries, REBASED so that entry 0 is 0.
// The section sizes are the caller's: n * n_pi * 32 and n * n_ci * 48 for one key, the partition's totals for a mixed batch.
constexpr size_t PAD = 64;
struct InputBlock {
    size_t offsets, inst, ci, proofs;       // where each section starts (offsets: 0)
    size_t inst_bytes, ci_bytes, proof_bytes;
    size_t need;                            // bytes of the block, PAD included
};
static inline InputBlock input_block(uint64_t n, size_t inst_bytes, size_t ci_bytes, size_t proof_bytes) {
    InputBlock b{};
    b.inst_bytes = inst_bytes; b.ci_bytes = ci_bytes; b.proof_bytes = proof_bytes;
    b.offsets = 0;
    b.inst = up16(((size_t)n + 1) * 8);
    b.ci = b.inst + up16(inst_bytes);
    b.proofs = b.ci + up16(ci_bytes);
    b.need = b.proofs + up16(proof_bytes + PAD);
    return b;
}
// the one rule of a batch's offsets that is checked before anything is sized from them
static inline bool offsets_ascend(uint64_t n, const uint64_t *proof_off) {
    for (uint64_t i = 0; i < n; i++)
        if (proof_off[i + 1] < proof_off[i]) return false;
    return true;
}
// Packs a batch into `block` (L.need bytes; L = input_block(n, .., proof_off[n] - proof_off[0])): the offsets rebased to the first
// proof, and the proof bytes from proof_off[0] on - what lies in front of the first proof stays behind.
static inline void pack_input(uint8_t *block, const InputBlock &L, uint64_t n, const uint64_t *proof_off, const uint8_t *proofs,
                              const uint8_t *instances, const uint8_t *committed) {
    uint64_t *off = (uint64_t *)(block + L.offsets);
    for (uint64_t i = 0; i <= n; i++) off[i] = proof_off[i] - proof_off[0];
    if (L.inst_bytes) memcpy(block + L.inst, instances, L.inst_bytes);
    if (L.ci_bytes) memcpy(block + L.ci, committed, L.ci_bytes);
    if (L.proof_bytes) memcpy(block + L.proofs, proofs + proof_off[0], L.proof_bytes);
    memset(block + L.proofs + L.proof_bytes, 0, PAD);
}

// ---- the result block of a blocking host-buffer form: the regions its kernels write (and, the pair check, read), each at a
// multiple of 16, in the order the form has always had them, PAD bytes behind the last.  A region a form does not have is empty.
enum class Call { PREPARE, CHECK, AGGREGATE, MIXED };
struct Region { size_t off, bytes; };
struct ResultBlock {
    Region pairs;      // PREPARE (out) and CHECK (in): n x 96; AGGREGATE and MIXED: the call's one pair, 96
    Region status;     // n x 4
    Region accept;     // accept[n] / included[n]; PREPARE: empty
    size_t extent;     // bytes of the block
};
static inline ResultBlock result_block(Call kind, uint64_t n) {
    ResultBlock r{};
    size_t at = 0;
    auto put = [&at](Region &g, size_t bytes) { g = {at, bytes}; at = up16(at + bytes); };
    const size_t per_proof = kind == Call::PREPARE || kind == Call::CHECK ? (size_t)n * 96 : 96;
    if (kind == Call::MIXED) {
        put(r.accept, (size_t)n); put(r.status, (size_t)n * 4); put(r.pairs, per_proof);
    } else {
        put(r.pairs, per_proof); put(r.status, (size_t)n * 4);
        if (kind == Call::PREPARE) r.accept = {at, 0};
        else put(r.accept, (size_t)n);
    }
    r.extent = at + PAD;
    return r;
}

// ---- the pinned download block of a submitted batch: accept[n], then the RLC verdict word at the next multiple of 8.  A capacity
// is compared with accept_extent, never with n: the word of a batch whose accept bytes alone fitted once landed past the block.
static inline size_t accept_word(uint64_t n) { return (size_t)((n + 7) & ~(uint64_t)7); }
static inline size_t accept_extent(uint64_t n) { return accept_word(n) + 8; }
}   // namespace hostcall
