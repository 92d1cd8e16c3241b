// Stand-alone driver of the host-buffer calls' layouts and packer (csrc/h2v_hostcall_layout.hpp).  Host code only: built with
// -fsanitize=address,undefined and run as a program (tests/test_hostcall_layout.py).  Every property is checked here and a miss
// prints "FAIL ..." and makes the exit status 1; the lines "old ..." put the formulas the call sites had before the header
// existed beside the header's extents, for the test log.
#include <cstdio>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_hostcall_layout.hpp"

using namespace hostcall;
static int g_bad = 0;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                      \
    } while (0)

static const char *NAME[] = {"prepare", "check", "aggregate", "mixed"};
static const Call KINDS[] = {Call::PREPARE, Call::CHECK, Call::AGGREGATE, Call::MIXED};

static void result_layouts() {
    std::vector<uint64_t> ns;
    for (uint64_t n = 0; n <= 300; n++) ns.push_back(n);
    for (uint64_t n : {4095ull, 4096ull, 4097ull, 1ull << 22}) ns.push_back(n);
    for (int k = 0; k < 4; k++) {
        size_t last = 0;
        for (uint64_t n : ns) {
            const ResultBlock r = result_block(KINDS[k], n);
            const bool per_proof = KINDS[k] == Call::PREPARE || KINDS[k] == Call::CHECK;
            CHECK(r.pairs.bytes == (per_proof ? n * 96 : 96), "%s n=%llu", NAME[k], (unsigned long long)n);
            CHECK(r.status.bytes == n * 4, "%s n=%llu", NAME[k], (unsigned long long)n);
            CHECK(r.accept.bytes == (KINDS[k] == Call::PREPARE ? 0 : n), "%s n=%llu", NAME[k], (unsigned long long)n);
            const Region g[3] = {r.pairs, r.status, r.accept};
            for (int i = 0; i < 3; i++) {
                CHECK(g[i].off % 16 == 0, "%s n=%llu region %d at %zu", NAME[k], (unsigned long long)n, i, g[i].off);
                CHECK(g[i].off + g[i].bytes + PAD <= r.extent, "%s n=%llu region %d ends at %zu, extent %zu", NAME[k], (unsigned long long)n, i,
                      g[i].off + g[i].bytes, r.extent);
                for (int j = i + 1; j < 3; j++)
                    CHECK(g[i].off + g[i].bytes <= g[j].off || g[j].off + g[j].bytes <= g[i].off, "%s n=%llu regions %d and %d overlap", NAME[k],
                          (unsigned long long)n, i, j);
            }
            CHECK(r.extent >= last, "%s n=%llu: extent %zu below the one before, %zu", NAME[k], (unsigned long long)n, r.extent, last);
            last = r.extent;
        }
    }
    size_t last = 0;
    for (uint64_t n : ns) {     // the download block: accept[n], then the whole verdict word, at a multiple of 4
        CHECK(accept_word(n) >= n && accept_word(n) % 8 == 0, "n=%llu word at %zu", (unsigned long long)n, accept_word(n));
        CHECK(accept_word(n) + 4 <= accept_extent(n), "n=%llu word at %zu, extent %zu", (unsigned long long)n, accept_word(n), accept_extent(n));
        CHECK(accept_extent(n) >= last, "n=%llu", (unsigned long long)n);
        last = accept_extent(n);
    }
}

static void input_blocks() {
    for (uint64_t n = 0; n <= 40; n++)
        for (size_t inst : {(size_t)0, (size_t)32 * n, (size_t)96 * n})
            for (size_t ci : {(size_t)0, (size_t)48 * n})
                for (size_t pr : {(size_t)0, (size_t)1, (size_t)47, (size_t)48, (size_t)1120 * n}) {
                    const InputBlock b = input_block(n, inst, ci, pr);
                    CHECK(b.offsets == 0 && b.inst >= (n + 1) * 8, "n=%llu: %llu offsets do not fit in front of %zu", (unsigned long long)n,
                          (unsigned long long)n + 1, b.inst);
                    CHECK(b.inst % 16 == 0 && b.ci % 16 == 0 && b.proofs % 16 == 0, "n=%llu %zu %zu %zu", (unsigned long long)n, b.inst, b.ci, b.proofs);
                    CHECK(b.inst + inst <= b.ci && b.ci + ci <= b.proofs, "n=%llu: sections overlap", (unsigned long long)n);
                    CHECK(b.proofs + pr + PAD <= b.need, "n=%llu: the zero bytes end at %zu, need %zu", (unsigned long long)n, b.proofs + pr + PAD, b.need);
                    CHECK(b.inst_bytes == inst && b.ci_bytes == ci && b.proof_bytes == pr, "n=%llu", (unsigned long long)n);
                }
}

// the packer on host memory: junk bytes in front of the first proof (proof_off[0] = first) stay behind, the offsets come out rebased
static void packer(uint64_t first, bool no_inst /* a plan without public inputs: instances == NULL and an empty section */) {
    const uint64_t n = 5, len = 37;
    std::vector<uint64_t> off(n + 1);
    for (uint64_t i = 0; i <= n; i++) off[i] = first + i * len;
    std::vector<uint8_t> proofs(off[n]), inst(n * 32), ci(n * 48);
    for (size_t i = 0; i < proofs.size(); i++) proofs[i] = i < first ? 0xEE : (uint8_t)(1 + (i - first) % 199);
    for (size_t i = 0; i < inst.size(); i++) inst[i] = (uint8_t)(i * 7 + 3);
    for (size_t i = 0; i < ci.size(); i++) ci[i] = (uint8_t)(i * 5 + 1);
    CHECK(offsets_ascend(n, off.data()), "ascending offsets refused");
    const InputBlock L = input_block(n, no_inst ? 0 : inst.size(), ci.size(), off[n] - off[0]);
    std::vector<uint8_t> block(L.need, 0x77);       // exactly `need` bytes: ASan has the end
    pack_input(block.data(), L, n, off.data(), proofs.data(), no_inst ? nullptr : inst.data(), ci.data());
    const uint64_t *got = (const uint64_t *)block.data();
    for (uint64_t i = 0; i <= n; i++) CHECK(got[i] == i * len, "first=%llu: offset %llu is %llu", (unsigned long long)first, (unsigned long long)i, (unsigned long long)got[i]);
    CHECK(memcmp(block.data() + L.proofs, proofs.data() + first, n * len) == 0, "first=%llu: the proof bytes are not those from proof_off[0] on", (unsigned long long)first);
    if (!no_inst) CHECK(memcmp(block.data() + L.inst, inst.data(), inst.size()) == 0, "instances");
    CHECK(memcmp(block.data() + L.ci, ci.data(), ci.size()) == 0, "committed");
    for (size_t i = 0; i < PAD; i++) CHECK(block[L.proofs + n * len + i] == 0, "pad byte %zu", i);
    std::vector<uint64_t> bad = off;
    bad[3] = bad[2] - 1;
    CHECK(!offsets_ascend(n, bad.data()), "descending offsets accepted");
}

int main() {
    result_layouts();
    input_blocks();
    for (uint64_t first : {0ull, 48ull}) { packer(first, false); packer(first, true); }
    // what the call sites computed before: hp_ensure's one capacity n * 101 + 64 for prepare / check / aggregate and the last byte
    // each of them addressed in it; mixed_host's up16(up16(n) + 4 n) + 96 + 16
    for (uint64_t n : {1ull, 100ull, 186ull, 4096ull}) {
        const size_t old_used[4] = {(size_t)n * 100, (size_t)n * 101, 96 + (size_t)n * 5, up16(up16(n) + n * 4) + 96 + 16};
        for (int k = 0; k < 4; k++) {
            const size_t ext = result_block(KINDS[k], n).extent;
            std::printf("old n=%llu %s: addressed %zu of a block of %zu; now extent %zu\n", (unsigned long long)n, NAME[k], old_used[k],
                        k < 3 ? (size_t)n * 101 + 64 : old_used[k], ext);
            CHECK(ext >= old_used[k] + (k < 3 ? PAD : 0), "%s n=%llu: the block became smaller than what the form addressed", NAME[k], (unsigned long long)n);
        }
        std::printf("old n=%llu download block: (n + 7 & ~7) + 8 = %zu; now accept_extent %zu\n", (unsigned long long)n, (size_t)((n + 7) & ~7ull) + 8, accept_extent(n));
    }
    std::printf("%s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
