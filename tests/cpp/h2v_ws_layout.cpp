// Stand-alone driver of the workspace's size tables (csrc/h2v_ws_layout.hpp).  Host code only: built with
// -fsanitize=address,undefined and run as a program (tests/test_ws_layout.py).  It prints one line per (set, shape, capacity) with
// every row's name and bytes - tests/golden/workspace_layout.txt holds what the allocation sites computed before the tables
// existed - and checks the group pool's layout, Shape's fit rule and shape_union; a miss prints "FAIL ..." and makes the exit
// status 1.  With arguments it answers instead what the named sets add to the five counters of h2v_probe_device_memory - one line
// "device blocks, device bytes, pinned blocks, pinned bytes, events" per argument (tests/test_workspace_memory_gpu.py asks).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_mixed_tables.hpp"
#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_ws_layout.hpp"

using namespace wslayout;
static int g_bad = 0;
#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                      \
    } while (0)

// the facts of every built-in key (vk.BUILDERS, vk.WIDE_BUILDERS) as plan.compile_plan and the plan loader state them
struct Key { const char *name; uint32_t n_terms, n_main, n_points, n_ci, ivc, n_regs, vm_lanes, n_trace, n_var, n_fix, proof_len, n_pi; };
static const Key KEYS[] = {
    {"simple_mul", 16, 16, 10, 0, 0, 88, 2, 27, 10, 6, 1120, 3},
    {"lookup_table", 34, 34, 25, 0, 0, 119, 2, 44, 25, 9, 2544, 1},
    {"atms_with_lookups", 50, 50, 20, 0, 0, 137, 2, 36, 20, 30, 2816, 2},
    {"sha256", 60, 60, 24, 1, 0, 272, 4, 58, 25, 35, 3808, 32},
    {"secp256k1", 60, 60, 23, 1, 0, 211, 4, 55, 24, 36, 3728, 4},
    {"ivc", 45, 28, 17, 0, 1, 228, 4, 33, 0, 0, 1840, 28},
    {"trashcan_mix", 33, 33, 19, 1, 0, 168, 4, 36, 20, 13, 2352, 5},
    {"phased", 29, 29, 18, 0, 0, 113, 2, 33, 18, 11, 1920, 2},
    {"bls12381", 72, 72, 31, 1, 0, 242, 4, 60, 32, 40, 4944, 4},
    {"composite", 126, 126, 44, 1, 0, 277, 4, 50, 45, 81, 7584, 4},
    {"wide335", 335, 335, 63, 1, 0, 570, 8, 56, 64, 271, 16016, 4},
    {"wide677", 677, 677, 75, 1, 0, 953, 16, 64, 76, 601, 28112, 4},
    {"ivc_wide", 196, 81, 24, 0, 1, 586, 16, 41, 0, 0, 4192, 126},
    // the MSM widths around the segmentation threshold, and a combiner whose register file does not fit LDS
    {"width64", 64, 64, 10, 0, 0, 88, 2, 27, 58, 6, 1120, 3},
    {"width65", 65, 65, 10, 0, 0, 88, 2, 27, 59, 6, 1120, 3},
    {"width96", 96, 96, 10, 0, 0, 88, 2, 27, 90, 6, 1120, 3},
    {"global_regs", 16, 16, 10, 0, 0, 700, 1, 27, 10, 6, 1120, 3},
    // many terms in narrow sums (a recursive key: 50 of its own, 49 behind acc_right): room for a wide key's terms, none for its segments
    {"narrow_sums", 100, 50, 30, 0, 1, 228, 4, 33, 0, 0, 1840, 28},
};
static const uint64_t CAPS[] = {1, 63, 64, 65, 4096, 1ull << 24};
static const uint32_t dummy_table = 0;
// the device view of a key as far as a shape reads it; fix: the plan has its all-window tables (non-recursive keys with VK-base terms)
static H2vDevPlan plan_of(const Key &k, bool ivc, bool fix) {
    H2vDevPlan d = {};
    d.n_terms = k.n_terms; d.n_main_terms = k.n_main; d.n_points = k.n_points; d.n_ci = k.n_ci; d.ivc = ivc ? 1 : 0;
    d.n_regs = k.n_regs; d.vm_lanes = k.vm_lanes; d.n_trace = k.n_trace;
    d.fix_tab = fix ? &dummy_table : nullptr;
    return d;
}

struct Line {
    std::string s;
    void add(const Row &r) {
        if (!r.bytes) return;
        char b[96];
        std::snprintf(b, sizeof b, r.fill == NONE ? " %s=%zu" : " %s=%zu@%d", r.name, r.bytes, (int)r.fill);
        s += b;
    }
    template <int N> void add(const Table<N> &t, const char *prefix = "") {
        for (const Row &r : t.row) {
            if (!r.bytes) continue;
            const std::string nm = std::string(prefix) + r.name;
            add(Row{nm.c_str(), r.bytes, r.fill});
        }
    }
    void add(const RlcSet &r) {        // the set's own rows; its two bucket-MSM sets by their arguments (their rows: the bucket_msm lines)
        add(r.t);
        char b[96];
        std::snprintf(b, sizeof b, " R=bucket_msm(%u,%u) L=bucket_msm(%u,1)", r.r_cap_n, r.r_halves, r.l_cap_n);
        s += b;
    }
};

struct GridShape { std::string name; Shape s; };
static std::vector<GridShape> g_shapes;

// the keys whose plan-shaped sets (RLC, group stage, coalescing) are printed: the smallest, the smallest wide one, the widest
static bool printed_key(const Key &k) { return !strcmp(k.name, "simple_mul") || !strcmp(k.name, "bls12381") || !strcmp(k.name, "wide677"); }

static void print_grid() {
    // every key as it is (a recursive key has no fixed-base sum, every other one has); simple_mul and narrow_sums also with a
    // trace, with recursion flipped and with the fixed-base sum flipped
    std::printf("pipeline events=%u\n", PIPE_EVENTS);
    for (const Key &k : KEYS) {
        const bool all = !strcmp(k.name, "simple_mul") || !strcmp(k.name, "narrow_sums");
        const int ivc0 = (int)k.ivc, fix0 = k.n_fix != 0;
        const int variants[4][3] = {{0, ivc0, fix0}, {1, ivc0, fix0}, {0, !ivc0, fix0}, {0, ivc0, !fix0}};
        for (int v = 0; v < (all ? 4 : 1); v++) {
            const int trace = variants[v][0], ivc = variants[v][1], fix = variants[v][2];
            const Shape s = shape_of(plan_of(k, ivc != 0, fix != 0), trace != 0);
            char nm[96];
            std::snprintf(nm, sizeof nm, "%s trace=%d ivc=%d fix=%d", k.name, trace, ivc, fix);
            g_shapes.push_back({nm, s});
            for (uint64_t cap : CAPS) {
                Line l;
                l.add(pipeline(s, cap));
                std::printf("pipeline %s cap=%llu:%s\n", nm, (unsigned long long)cap, l.s.c_str());
            }
        }
    }
    for (uint32_t halves = 1; halves <= 2; halves++)
        for (uint64_t cap : {0ull, 1ull, 63ull, 64ull, 65ull, 4096ull, 1ull << 24}) {
            Line l;
            l.add(bucket_msm((uint32_t)cap, halves));
            std::printf("bucket_msm cap_n=%llu halves=%u:%s\n", (unsigned long long)cap, halves, l.s.c_str());
        }
    for (const Key &k : KEYS) {
        if (!printed_key(k)) continue;
        for (uint64_t cap : CAPS) {
            Line l;
            l.add(rlc_plan(cap, k.n_var, k.n_fix));
            std::printf("rlc plan %s n_var=%u n_fix=%u cap=%llu:%s\n", k.name, k.n_var, k.n_fix, (unsigned long long)cap, l.s.c_str());
        }
    }
    for (uint64_t cap : CAPS) {
        Line l;
        l.add(rlc_pairs(cap));
        std::printf("rlc pairs cap=%llu pool=%zu:%s\n", (unsigned long long)cap, rlc_pair_pool(cap), l.s.c_str());
    }
    const size_t needs[][4] = {{1, 1, 0, 0}, {5000, 3, 4000, 90}, {((size_t)1 << 22) - 5, 70000, 1000, 100000}};
    for (uint64_t cap : CAPS)
        for (const auto &nd : needs) {
            const FoldCaps c = fold_caps(nd[0], nd[1], nd[2], nd[3]);
            Line l;
            l.add(rlc_fold(cap, c.terms, c.parts));
            std::printf("rlc fold cap=%llu need_t=%zu need_p=%zu have_t=%zu have_p=%zu cap_t=%zu cap_p=%zu:%s\n", (unsigned long long)cap, nd[0], nd[1], nd[2],
                        nd[3], c.terms, c.parts, l.s.c_str());
        }
    for (uint32_t n : {256u, 260u, 4096u, 32768u}) {
        const uint32_t G = (n + 63) / 64;
        auto group_line = [&](const char *what, uint32_t stride, uint32_t halves) {
            Line l;
            l.add(group_stage(G, stride));
            const GroupPool p = group_pool(G, stride, halves);
            // every offset of the pool, folded into one number, and the last problem's in full
            uint64_t h = 1469598103934665603ull;
            for (uint32_t q = 0; q < G; q++)
                for (int side = 0; side < 2; side++) {
                    const GroupPool::At a = p.at(q, side);
                    for (size_t v : {a.cnt, a.pts28, a.dig, a.list, a.off, a.order, a.cls, a.partial, a.wsum}) h = (h ^ (uint64_t)v) * 1099511628211ull;
                }
            const GroupPool::At a = p.at(G - 1, 1);
            std::printf("group %s n=%u G=%u stride=%u halves=%u:%s pinned_args=%zu cnt_bytes=%zu offsets=%016llx last=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu\n", what, n, G,
                        stride, halves, l.s.c_str(), group_args_bytes(G), p.cnt_bytes, (unsigned long long)h, a.cnt, a.pts28, a.dig, a.list, a.off, a.order,
                        a.cls, a.partial, a.wsum);
        };
        for (const Key &k : KEYS)
            if (printed_key(k)) group_line(k.name, 64 * k.n_var + k.n_fix, 2);
        group_line("pairs", 64, 1);
    }
    for (uint64_t cap : CAPS) {
        Line l;
        l.add(mixed_base(cap));
        std::printf("mixed cap=%llu events=%u:%s\n", (unsigned long long)cap, MIXED_EVENTS, l.s.c_str());
    }
    for (const Key &k : KEYS)
        for (uint64_t cap : {1ull, 63ull, 64ull, 65ull, 4096ull}) {
            if (!printed_key(k)) continue;
            Line l;
            l.add(coalesce((uint32_t)cap, co_proof_bytes((uint32_t)cap, k.proof_len), co_inst_bytes((uint32_t)cap, k.n_pi)));
            std::printf("coalesce %s cap=%llu:%s\n", k.name, (unsigned long long)cap, l.s.c_str());
        }
    for (uint64_t cap : CAPS) {
        Line l;
        l.add(pair_view(cap)); l.add(rlc_stats());
        std::printf("small cap=%llu:%s seed_ring=%zu laned_accept=%zu\n", (unsigned long long)cap, l.s.c_str(), seed_ring_bytes(), laned_accept(cap));
    }
    for (size_t need : {(size_t)1, (size_t)3, (size_t)4, (size_t)65, (size_t)4096, (size_t)1 << 30}) std::printf("grown need=%zu: %zu\n", need, grown(need));
}

// The group pool, bound as the group stage binds it: every region of every (group, side) lies inside a heap block of exactly the
// total (ASan sees the first and the last byte written), and no two regions overlap (each byte is claimed once).
static void check_group_pool() {
    for (uint32_t n : {256u, 260u, 4096u, 32768u})
        for (int shape = 0; shape < (n <= 260 ? 3 : 2); shape++) {     // pairs, simple_mul's proofs, and - few groups only - wide677's
            const uint32_t G = (n + 63) / 64, stride = shape == 0 ? 64 : shape == 1 ? 64 * 10 + 6 : 64 * 76 + 601, halves = shape == 0 ? 1 : 2;
            const GroupPool p = group_pool(G, stride, halves);
            CHECK(p.total == group_stage(G, stride).row[G_POOL].bytes, "n=%u shape=%d", n, shape);
            std::vector<uint8_t> pool(p.total, 0);       // (a block of its own: ASan guards both ends)
            const size_t nb = (size_t)GRP_W * GRP_NB;
            size_t claimed = 0;
            for (uint32_t q = 0; q < G; q++)
                for (int side = 0; side < 2; side++) {
                    const GroupPool::At a = p.at(q, side);
                    const size_t cap_n = side == 0 ? stride : 64, h = side == 0 ? halves : 1;
                    const size_t reg[9][2] = {{a.cnt, nb * 4}, {a.pts28, cap_n * PIP_PT_DW * 4}, {a.dig, cap_n * h * GRP_W * 2}, {a.list, cap_n * h * GRP_W * 4},
                                              {a.off, (nb + 1) * 4}, {a.order, nb * 4}, {a.cls, PIP_CLS_DW * 4}, {a.partial, nb * PIP_PART_DW * 4},
                                              {a.wsum, (size_t)GRP_W * PIP_PART_DW * 4}};
                    for (const auto &r : reg) {
                        CHECK(r[0] % 256 == 0 && r[0] + r[1] <= p.total, "n=%u shape=%d group %u side %d: region at %zu + %zu, total %zu", n, shape, q, side, r[0], r[1],
                              p.total);
                        if (r[0] + r[1] > p.total) return;
                        uint8_t *base = pool.data() + r[0];
                        CHECK(base[0] == 0 && base[r[1] - 1] == 0, "n=%u shape=%d group %u side %d: region at %zu overlaps another", n, shape, q, side, r[0]);
                        memset(base, 1, r[1]);
                        claimed += r[1];
                    }
                    CHECK(a.end <= p.total, "n=%u shape=%d group %u side %d ends at %zu", n, shape, q, side, a.end);
                }
            size_t ones = 0;
            for (uint8_t b : pool) ones += b;
            CHECK(ones == claimed, "n=%u shape=%d: %zu bytes claimed, %zu distinct", n, shape, claimed, ones);
            CHECK((size_t)2 * G * up256(nb * 4) == p.cnt_bytes, "n=%u", n);
        }
}

// fits, against a plain restatement of the rule for every ordered pair of grid shapes; every reason occurs
static void check_fits() {
    int seen[7] = {};
    for (const GridShape &w : g_shapes)
        for (const GridShape &p : g_shapes)
            for (int want = 0; want < 2; want++) {
                const Shape &a = w.s, &b = p.s;
                Fit e = Fit::OK;
                if (b.terms > a.terms || b.slots > a.slots) e = Fit::SMALLER_PLAN;
                else if (b.regs != 0 && b.regs > a.regs) e = Fit::REGISTER_FILE;
                else if (b.ivc && !a.ivc) e = Fit::NOT_RECURSIVE;
                else if (b.fix && !a.fix) e = Fit::NO_FIXED_SUM;
                else if (msm_max_segments(b.width) > a.segs) e = Fit::NARROWER_SUMS;
                else if (want && b.trace > a.trace) e = Fit::NO_TRACE;
                const Fit got = fits(a, b, want != 0);
                CHECK(got == e, "[%s] in [%s] want_trace=%d: %d, expected %d", p.name.c_str(), w.name.c_str(), want, (int)got, (int)e);
                seen[(int)got]++;
                CHECK((got == Fit::OK) == (fit_message(got)[0] == 0), "message of %d", (int)got);
            }
    for (int k = 0; k < 7; k++) CHECK(seen[k] > 0, "reason %d never occurred", k);
}

// shape_union: both fit it (whatever trace either wants), and it is the smallest such shape field by field
static void check_union() {
    for (const GridShape &x : g_shapes)
        for (const GridShape &y : g_shapes) {
            const Shape &a = x.s, &b = y.s, u = shape_union(a, b);
            CHECK(fits(u, a, true) == Fit::OK && fits(u, b, true) == Fit::OK, "[%s] + [%s]", x.name.c_str(), y.name.c_str());
            auto mx = [](uint32_t p, uint32_t q) { return p > q ? p : q; };
            CHECK(u.terms == mx(a.terms, b.terms) && u.main_terms == mx(a.main_terms, b.main_terms) && u.slots == mx(a.slots, b.slots) &&
                      u.regs == mx(a.regs, b.regs) && u.trace == mx(a.trace, b.trace) && u.width == mx(a.width, b.width) && u.segs == mx(a.segs, b.segs) &&
                      u.ivc == (a.ivc || b.ivc) && u.fix == (a.fix || b.fix),
                  "[%s] + [%s]", x.name.c_str(), y.name.c_str());
            CHECK(u.segs == msm_max_segments(u.width), "[%s] + [%s]: segments of the union's width", x.name.c_str(), y.name.c_str());
        }
}

// One set per argument, "name,a,b,..": what creating it adds to the counters
struct Sum {
    uint64_t v[5] = {};
    template <int N> void dev(const Table<N> &t) { v[0] += t.blocks(); v[1] += t.total(); }
    void dev(size_t bytes) { v[0] += 1; v[1] += bytes; }
    void pinned(size_t bytes) { v[2] += 1; v[3] += bytes; }
    void rlc(const RlcSet &r) { v[0] += r.blocks(); v[1] += r.total(); }
};
static int answer(int argc, char **argv) {
    for (int k = 1; k < argc; k++) {
        std::vector<uint64_t> a;
        std::string name, arg = argv[k];
        size_t at = arg.find(',');
        name = arg.substr(0, at);
        while (at != std::string::npos) {
            const size_t next = arg.find(',', at + 1);
            a.push_back(std::strtoull(arg.substr(at + 1, next == std::string::npos ? next : next - at - 1).c_str(), nullptr, 10));
            at = next;
        }
        auto need = [&](size_t n) { if (a.size() != n) { std::printf("FAIL %s: %zu arguments\n", arg.c_str(), n); std::exit(2); } };
        Sum s;
        if (name == "pipeline") {          // terms, main terms, slots, global registers, trace, ivc, fix, width, cap
            need(9);
            Shape sh;
            sh.terms = (uint32_t)a[0]; sh.main_terms = (uint32_t)a[1]; sh.slots = (uint32_t)a[2]; sh.regs = (uint32_t)a[3]; sh.trace = (uint32_t)a[4];
            sh.ivc = a[5] != 0; sh.fix = a[6] != 0; sh.width = (uint32_t)a[7]; sh.segs = msm_max_segments(sh.width);
            s.dev(pipeline(sh, a[8])); s.v[4] += PIPE_EVENTS;
        } else if (name == "laned") { need(1); s.dev(laned_accept(a[0])); s.v[4] += 1; }
        else if (name == "events") { need(1); s.v[4] += a[0]; }
        else if (name == "rlc") { need(3); s.rlc(rlc_plan(a[0], (uint32_t)a[1], (uint32_t)a[2])); }
        else if (name == "pairs") { need(1); s.rlc(rlc_pairs(a[0])); }
        else if (name == "pairpool") { need(1); s.dev(rlc_pair_pool(a[0])); }
        else if (name == "fold") {         // cap, terms and block sums needed, terms and block sums the pool has
            need(5);
            const FoldCaps c = fold_caps(a[1], a[2], a[3], a[4]);
            s.rlc(rlc_fold(a[0], c.terms, c.parts));
        } else if (name == "group") { need(2); s.dev(group_stage((uint32_t)a[0], (uint32_t)a[1])); s.pinned(group_args_bytes((uint32_t)a[0])); }
        else if (name == "mixed") { need(1); s.dev(mixed_base(a[0])); s.v[4] += MIXED_EVENTS; }
        else if (name == "tabslot") {      // proofs, foldable plans with proofs: a table slot of a mixed call, pinned and on the device
            need(2);
            const size_t extent = mixedtab::table_block(a[0], (size_t)a[1] * 48, nullptr, 0).extent;
            s.pinned(grown(extent)); s.dev(grown(extent));
        } else if (name == "coalesce") { need(3); s.dev(coalesce((uint32_t)a[0], co_proof_bytes((uint32_t)a[0], (uint32_t)a[1]), co_inst_bytes((uint32_t)a[0], (uint32_t)a[2]))); }
        else if (name == "pairview") { need(1); s.dev(pair_view(a[0])); }
        else if (name == "stats") { need(0); const auto t = rlc_stats(); s.dev(t.row[S_REC_FAIL].bytes); s.dev(t.row[S_RLC_STATS].bytes); s.pinned(t.row[S_H_RLC_STATS].bytes); }
        else if (name == "seedring") { need(0); s.dev(seed_ring_bytes()); }
        else if (name == "grown") { need(1); s.dev(grown(a[0])); }
        else { std::printf("FAIL %s: no such set\n", arg.c_str()); return 2; }
        std::printf("%llu %llu %llu %llu %llu\n", (unsigned long long)s.v[0], (unsigned long long)s.v[1], (unsigned long long)s.v[2], (unsigned long long)s.v[3],
                    (unsigned long long)s.v[4]);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return answer(argc, argv);
    print_grid();
    check_group_pool();
    check_fits();
    check_union();
    std::printf("ok %zu\n", g_shapes.size());
    return g_bad ? 1 : 0;
}
