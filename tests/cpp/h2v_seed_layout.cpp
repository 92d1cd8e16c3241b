// Stand-alone check of csrc/h2v_seed.hpp (host code only): the digest tree of a derived batch seed - levels, node counts and where
// every level lies in the call's digest buffer.  Built with -fsanitize=address,undefined by tests/test_derived_seed.py, which passes
// the model's node counts in:  one argument  n:c1,c2,..  per batch size (c_l = nodes of level l according to seed.py).
// Checks per n: the level count and every count equal the model's; every level ends in one node; the levels (leaves included) are
// disjoint, in order, without gaps and inside the extent; every node has 1 .. 64 children and the children of a level add up to the
// level below; digests written at the offsets into a buffer of exactly `extent` digests stay inside it (the sanitizer's part).
#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_seed.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static int failures = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            printf("FAIL %s: ", #cond);               \
            printf(__VA_ARGS__);                      \
            printf("\n");                             \
            failures++;                               \
        }                                             \
    } while (0)

static void check_n(uint64_t n, const std::vector<uint64_t> &model) {
    h2vseed::Tree t;
    const bool ok = h2vseed::tree(n, &t);
    CHECK(ok, "n=%llu", (unsigned long long)n);
    if (!ok) return;
    CHECK(t.levels == model.size(), "n=%llu levels %u, model %zu", (unsigned long long)n, t.levels, model.size());
    CHECK(t.levels >= 1 && t.levels <= h2vseed::MAX_LEVELS, "n=%llu levels %u", (unsigned long long)n, t.levels);
    if (t.levels != model.size() || t.levels < 1 || t.levels > h2vseed::MAX_LEVELS) return;
    CHECK(t.count[0] == n && t.off[0] == 0, "n=%llu leaves", (unsigned long long)n);
    CHECK(t.count[t.levels] == 1, "n=%llu: the top level has %llu nodes", (unsigned long long)n, (unsigned long long)t.count[t.levels]);
    uint64_t at = 0;
    for (uint32_t l = 0; l <= t.levels; l++) {
        if (l) CHECK(t.count[l] == model[l - 1], "n=%llu level %u: %llu nodes, model %llu", (unsigned long long)n, l, (unsigned long long)t.count[l], (unsigned long long)model[l - 1]);
        CHECK(t.off[l] == at, "n=%llu level %u starts at %llu, the level below ends at %llu", (unsigned long long)n, l, (unsigned long long)t.off[l], (unsigned long long)at);
        CHECK(t.count[l] >= 1, "n=%llu level %u is empty", (unsigned long long)n, l);
        if (l && l < t.levels) CHECK(t.count[l] > 1, "n=%llu level %u has one node below the top", (unsigned long long)n, l);
        at += t.count[l];
    }
    CHECK(t.extent == at, "n=%llu extent %llu, levels end at %llu", (unsigned long long)n, (unsigned long long)t.extent, (unsigned long long)at);
    // children: every node 1 .. 64, the sum is the level below, the last node takes the rest
    for (uint32_t l = 1; l <= t.levels; l++) {
        uint64_t sum = 0;
        const uint64_t below = t.count[l - 1];
        for (uint64_t j : {(uint64_t)0, t.count[l] / 2, t.count[l] - 1}) {
            const uint32_t m = h2vseed::children(below, j);
            CHECK(m >= 1 && m <= h2vseed::ARITY, "n=%llu level %u node %llu: %u children", (unsigned long long)n, l, (unsigned long long)j, m);
            CHECK(j * h2vseed::ARITY + m <= below, "n=%llu level %u node %llu reads past the level below", (unsigned long long)n, l, (unsigned long long)j);
        }
        if (t.count[l] <= 70000)
            for (uint64_t j = 0; j < t.count[l]; j++) sum += h2vseed::children(below, j);
        else sum = (t.count[l] - 1) * h2vseed::ARITY + h2vseed::children(below, t.count[l] - 1);
        CHECK(sum == below, "n=%llu level %u: the children add up to %llu of %llu", (unsigned long long)n, l, (unsigned long long)sum, (unsigned long long)below);
    }
    // the sanitizer's part: one mark per digest at the offsets, into exactly `extent` entries; nothing is marked twice
    if (n <= 300000) {
        std::vector<uint8_t> buf((size_t)t.extent, 0);
        for (uint32_t l = 0; l <= t.levels; l++)
            for (uint64_t j = 0; j < t.count[l]; j++) {
                uint8_t &b = buf[(size_t)(t.off[l] + j)];
                CHECK(b == 0, "n=%llu level %u entry %llu overlaps", (unsigned long long)n, l, (unsigned long long)j);
                b = 1;
            }
        size_t marked = 0;
        for (uint8_t b : buf) marked += b;
        CHECK(marked == buf.size(), "n=%llu: %zu of %zu entries belong to a level", (unsigned long long)n, marked, buf.size());
    }
}

int main(int argc, char **argv) {
    int checked = 0;
    for (int a = 1; a < argc; a++) {
        char *end = nullptr;
        const uint64_t n = strtoull(argv[a], &end, 10);
        std::vector<uint64_t> model;
        while (end && (*end == ':' || *end == ',')) model.push_back(strtoull(end + 1, &end, 10));
        if (!end || *end != 0 || model.empty()) { printf("FAIL bad argument %s\n", argv[a]); return 2; }
        check_n(n, model);
        checked++;
    }
    // outside the range: no tree
    h2vseed::Tree t;
    CHECK(h2vseed::tree(0, &t) && t.levels == 0 && t.extent == 0, "n=0");
    CHECK(!h2vseed::tree(h2vseed::MAX_N + 1, &t), "n=2^22+1 has a tree");
    // the tags: 16 bytes, zero-padded, the ASCII strings of the rule
    const h2vseed::TagWords leaf = h2vseed::tag_words(h2vseed::TAG_LEAF);
    uint8_t raw[16];
    memcpy(raw, leaf.w, 16);      // (a little-endian host, as the device)
    CHECK(memcmp(raw, "h2v-seed-leaf/1\0", 16) == 0, "leaf tag");
    printf("checked %d sizes\n", checked);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
