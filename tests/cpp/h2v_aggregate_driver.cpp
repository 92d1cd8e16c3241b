// Test driver for h2v::aggregate_batch and h2v::Aggregator (include/h2v.hpp).
//
// usage: h2v_aggregate_driver <plan.bin> <batch.bin> [<plan.bin> <batch.bin> ...] [<foreign plan.bin>]
//        (batch.bin as tests/cpp/h2v_cpp_driver.cpp reads it; the optional last argument is a key on ANOTHER SRS)
// Every (plan, batch) is one push of ONE Aggregator, in order; equal plan paths share one VerifyingKey.  Prints
//   "included <k> <bits>"   the included[] of push k's own aggregate call
//   "pair_ok <k> <0|1>"     check_pairs on that call's pair alone
//   "call <k> <bits>"       push k's accept vector from finish()
//   "reverified <k,k,...>"  (or "reverified -")
//   "foreign_refused <0|1>" with a foreign plan: pushing it into the same Aggregator throws Error(H2V_E_ARG) before anything runs
// or "error <code> <text>" (exit 2).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>

#include "h2v.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static uint32_t rd32(const std::vector<uint8_t> &b, size_t &o) {
    uint32_t v;
    std::memcpy(&v, b.data() + o, 4);
    o += 4;
    return v;
}
static std::string bits(const std::vector<uint8_t> &v) {
    std::string s;
    for (uint8_t a : v) s.push_back(a ? '1' : '0');
    return s;
}
struct Case {
    std::vector<uint8_t> proofs, inst, ci;
    std::vector<uint64_t> off{0};
    uint32_t n = 0;
    bool has_ci = false;
    h2v_batch batch() const { return h2v_batch{n, proofs.data(), off.data(), inst.empty() ? nullptr : inst.data(), has_ci ? ci.data() : nullptr}; }
};

int main(int argc, char **argv) {
    const char *foreign = (argc - 1) % 2 ? argv[argc - 1] : nullptr;
    if (foreign) argc--;
    if (argc < 3) { std::fprintf(stderr, "usage: %s plan.bin batch.bin [plan.bin batch.bin ...]\n", argv[0]); return 64; }
    h2v::ShutdownGuard shutdown_last;
    try {
        std::map<std::string, std::unique_ptr<h2v::VerifyingKey>> keys;
        std::vector<Case> cases((argc - 1) / 2);
        h2v::Aggregator agg;
        for (int k = 0; k < (argc - 1) / 2; k++) {
            const std::string plan_path = argv[1 + 2 * k];
            if (!keys.count(plan_path)) {
                const std::vector<uint8_t> blob = slurp(plan_path.c_str());
                keys[plan_path].reset(new h2v::VerifyingKey(blob.data(), blob.size(), 0));
            }
            const h2v::VerifyingKey &vk = *keys[plan_path];
            const std::vector<uint8_t> bb = slurp(argv[2 + 2 * k]);
            Case &c = cases[k];
            size_t o = 0;
            c.n = rd32(bb, o);
            const uint32_t n_pi = rd32(bb, o), has_ci = rd32(bb, o);
            c.has_ci = has_ci != 0;
            if (n_pi != vk.n_public_inputs() || has_ci != vk.n_committed_instances()) throw h2v::Error(H2V_E_ARG, "batch / plan mismatch");
            for (uint32_t i = 0; i < c.n; i++) {
                const uint32_t len = rd32(bb, o);
                c.proofs.insert(c.proofs.end(), bb.begin() + o, bb.begin() + o + len);
                o += len;
                c.off.push_back(c.proofs.size());
                c.inst.insert(c.inst.end(), bb.begin() + o, bb.begin() + o + 32 * n_pi);
                o += 32 * n_pi;
                if (has_ci) { c.ci.insert(c.ci.end(), bb.begin() + o, bb.begin() + o + 48); o += 48; }
            }
            const h2v_batch b = c.batch();
            const h2v::Aggregate a = h2v::aggregate_batch(vk, b);
            std::printf("included %d %s\n", k, bits(a.included).c_str());
            const h2v::PairVerdicts v = h2v::check_pairs(vk, std::vector<uint8_t>(a.pair, a.pair + 96));
            std::printf("pair_ok %d %d\n", k, v.accept[0] ? 1 : 0);
            agg.push(vk, b);
        }
        if (foreign) {
            const std::vector<uint8_t> blob = slurp(foreign);
            h2v::VerifyingKey other(blob.data(), blob.size(), 0);
            static const uint64_t zero_off[1] = {0};
            const h2v_batch none{0, nullptr, zero_off, nullptr, nullptr};
            int refused = 0;
            try { agg.push(other, none); } catch (const h2v::Error &e) { refused = e.code == H2V_E_ARG ? 1 : 0; }
            std::printf("foreign_refused %d\n", refused);
        }
        std::vector<size_t> reverified;
        const std::vector<std::vector<uint8_t>> out = agg.finish(&reverified);
        for (size_t k = 0; k < out.size(); k++) std::printf("call %zu %s\n", k, bits(out[k]).c_str());
        std::string rv;
        for (size_t k : reverified) rv += (rv.empty() ? "" : ",") + std::to_string(k);
        std::printf("reverified %s\n", rv.empty() ? "-" : rv.c_str());
        return 0;
    } catch (const h2v::Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
        return 2;
    }
}
