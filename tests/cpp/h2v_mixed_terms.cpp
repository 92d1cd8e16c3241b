// Stand-alone test of the term-pool layout of the fold form of mixed-key batches (csrc/h2v_mixed_fold.hpp: fold_layout).  Host
// code only: built with -fsanitize=address,undefined and run as a program (tests/test_mixed_fold.py).  Every check compares with
// a direct restatement: mark every term and every block that a (plan, chunk, proof, term) owns in a plain array and look for a
// cell marked twice or never.
// Prints "ok <checks>" and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed_fold.hpp"

using namespace h2vmixed;

static int checks = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        checks++;                                                                           \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

// (n_var, n_fix, foldable) of simple_mul, lookup_table, trashcan_mix, ivc, atms_with_lookups as the GPU tests list them; the
// figures only have to differ from plan to plan
static const FoldShape SHAPES[5] = {{10, 6, true}, {19, 11, true}, {17, 13, true}, {33, 0, false}, {23, 12, true}};

static void verify(const std::vector<FoldShape> &shapes, const std::vector<uint32_t> &count, uint32_t chunk) {
    const uint32_t K = (uint32_t)shapes.size();
    FoldLayout L;
    std::string err;
    CHECK(fold_layout(shapes.data(), count.data(), K, chunk, L, &err));
    // N_R by the formula of include/h2v.h
    uint64_t want = 0;
    uint32_t pairs = 0, fix = 0, foldable = 0;
    for (uint32_t k = 0; k < K; k++) {
        if (!count[k]) { CHECK(!L.foldable[k]); continue; }
        if (shapes[k].foldable) { want += (uint64_t)count[k] * shapes[k].n_var + shapes[k].n_fix; fix += shapes[k].n_fix; foldable++; }
        else { want += count[k]; pairs += count[k]; }
        CHECK((L.foldable[k] != 0) == shapes[k].foldable);
    }
    CHECK(L.n_r == want && L.n_pairs == pairs && L.total_fix == fix && L.n_foldable == foldable);
    // every term owned exactly once
    std::vector<uint8_t> term((size_t)L.n_r, 0), block(L.total_blocks, 0), part((size_t)L.n_parts, 0), lane(L.total_fix, 0);
    auto own = [&](std::vector<uint8_t> &v, uint64_t at) { CHECK(at < v.size()); CHECK(v[(size_t)at] == 0); v[(size_t)at] = 1; checks -= 2; };
    for (uint32_t k = 0; k < K; k++) {
        if (!count[k]) continue;
        if (!L.foldable[k]) {
            for (uint32_t j = 0; j < count[k]; j++) own(term, (uint64_t)L.pair_base[k] + j);
            CHECK(L.n_blocks[k] == 0);
            continue;
        }
        const FoldShape &s = shapes[k];
        // the chunks as the lanes cut them: [first, first + m) with first a multiple of the chunk size
        const uint32_t step = chunk == 0 || chunk >= count[k] ? count[k] : chunk;
        uint32_t blocks_seen = 0;
        for (uint32_t first = 0; first < count[k]; first += step) {
            const uint32_t m = count[k] - first < step ? count[k] - first : step;
            const uint32_t b0 = fold_chunk_block(first, chunk == 0 || chunk >= count[k] ? 0 : chunk);
            CHECK(b0 == fold_chunk_block(first, chunk) || chunk >= count[k]);
            for (uint32_t i = 0; i < m; i++)
                for (uint32_t t = 0; t < s.n_var; t++) own(term, (uint64_t)L.term_base[k] + (uint64_t)(first + i) * s.n_var + t);
            for (uint32_t b = 0; b < (m + 63) / 64; b++) {
                CHECK(b0 + b < L.n_blocks[k]);
                own(block, (uint64_t)L.block_base[k] + b0 + b);
                for (uint32_t f = 0; f < s.n_fix; f++) own(part, L.part_base[k] + (uint64_t)(b0 + b) * s.n_fix + f);
                blocks_seen++;
            }
        }
        CHECK(blocks_seen == L.n_blocks[k] && L.n_blocks[k] == fold_blocks(count[k], chunk));
        for (uint32_t f = 0; f < s.n_fix; f++) { own(term, (uint64_t)L.vk_base[k] + f); own(lane, (uint64_t)L.fix_base[k] + f); }
    }
    for (uint8_t v : term) CHECK(v == 1);
    for (uint8_t v : block) CHECK(v == 1);
    for (uint8_t v : part) CHECK(v == 1);
    for (uint8_t v : lane) CHECK(v == 1);
}

int main() {
    const std::vector<FoldShape> all(SHAPES, SHAPES + 5);
    for (uint32_t chunk : {0u, 40u, 64u, 4096u}) {
        verify(all, {70, 65, 9, 1, 0}, chunk);                       // the GPU tests' mix
        verify(all, {0, 9, 70, 1, 65}, chunk);
        verify(all, {0, 0, 0, 1, 0}, chunk);                         // all non-foldable, and a single proof
        verify({SHAPES[3], SHAPES[3]}, {70, 65}, chunk);             // all non-foldable, many proofs
        verify(all, {1, 0, 0, 0, 0}, chunk);                         // a single proof of a foldable plan
        verify(all, {0, 0, 0, 0, 0}, chunk);                         // no proof at all: no term
        verify({SHAPES[0]}, {4097}, chunk);
        verify({SHAPES[0]}, {128}, chunk);
        for (uint32_t c : {1u, 39u, 40u, 41u, 63u, 64u, 65u, 80u, 81u, 127u, 128u, 129u}) verify({SHAPES[1], SHAPES[3], SHAPES[2]}, {c, c, 70}, chunk);
    }
    // the limit is exactly 2^22 terms
    {
        FoldLayout L;
        std::string err;
        const FoldShape one = {1, 1, true}, pair = {5, 0, false};
        uint32_t c = (1u << 22) - 1;                                 // c + 1 VK base = 2^22
        CHECK(fold_layout(&one, &c, 1, 4096, L, &err) && L.n_r == (1ull << 22));
        c = 1u << 22;
        CHECK(!fold_layout(&one, &c, 1, 4096, L, &err) && L.n_r == (1ull << 22) + 1 && err.find("2^22") != std::string::npos);
        c = 1u << 22;
        CHECK(fold_layout(&pair, &c, 1, 0, L, &err) && L.n_r == (1ull << 22));
        c = (1u << 22) + 1;
        CHECK(!fold_layout(&pair, &c, 1, 0, L, &err));
        const FoldShape wide = {4000, 100, true};                    // a product beyond 32 bits is refused, not wrapped
        c = 0xffffffffu;
        CHECK(!fold_layout(&wide, &c, 1, 4096, L, &err));
        const FoldShape two[2] = {{1, 1, true}, {5, 0, false}};
        const uint32_t cc[2] = {(1u << 21) - 1, 1u << 21};           // 2^21 - 1 + 1 + 2^21 = 2^22
        CHECK(fold_layout(two, cc, 2, 40, L, &err) && L.n_r == (1ull << 22));
        const uint32_t cd[2] = {1u << 21, 1u << 21};
        CHECK(!fold_layout(two, cd, 2, 40, L, &err));
    }
    std::printf("ok %d\n", checks);
    return 0;
}
