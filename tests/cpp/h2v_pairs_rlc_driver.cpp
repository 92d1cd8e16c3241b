// Test driver for h2v::check_pairs_rlc (include/h2v.hpp): prepare_batch -> check_pairs_rlc against verify_batch.
//
// usage: h2v_pairs_rlc_driver <plan.bin> <batch.bin>      (batch.bin as tests/cpp/h2v_cpp_driver.cpp reads it)
// prints "batch <bits>", "pairs_rlc <bits>", "pairs <bits>", "same_status <0|1>", "fell_back <0|1>", or "error <code> <text>" (exit 2).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

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

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s plan.bin batch.bin\n", argv[0]); return 64; }
    h2v::ShutdownGuard shutdown_last;
    try {
        const std::vector<uint8_t> blob = slurp(argv[1]), bb = slurp(argv[2]);
        h2v::VerifyingKey vk(blob.data(), blob.size(), 0);
        size_t o = 0;
        const uint32_t n = rd32(bb, o), n_pi = rd32(bb, o), has_ci = rd32(bb, o);
        if (n_pi != vk.n_public_inputs() || has_ci != vk.n_committed_instances()) throw h2v::Error(H2V_E_ARG, "batch / plan mismatch");
        std::vector<uint8_t> proofs, inst, ci;
        std::vector<uint64_t> off{0};
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t len = rd32(bb, o);
            proofs.insert(proofs.end(), bb.begin() + o, bb.begin() + o + len);
            o += len;
            off.push_back(proofs.size());
            inst.insert(inst.end(), bb.begin() + o, bb.begin() + o + 32 * n_pi);
            o += 32 * n_pi;
            if (has_ci) { ci.insert(ci.end(), bb.begin() + o, bb.begin() + o + 48); o += 48; }
        }
        h2v_batch batch{n, proofs.data(), off.data(), inst.data(), has_ci ? ci.data() : nullptr};
        const std::vector<uint8_t> acc = h2v::verify_batch(vk, batch);
        const h2v::PreparedBatch prep = h2v::prepare_batch(vk, batch);
        bool fell_back = false;
        const h2v::PairVerdicts rlc = h2v::check_pairs_rlc(vk, prep.pairs, nullptr, nullptr, &fell_back);
        const h2v::PairVerdicts per_pair = h2v::check_pairs(vk, prep.pairs);
        std::printf("batch %s\npairs_rlc %s\npairs %s\n", bits(acc).c_str(), bits(rlc.accept).c_str(), bits(per_pair.accept).c_str());
        std::printf("same_status %d\nfell_back %d\n", rlc.status == per_pair.status ? 1 : 0, fell_back ? 1 : 0);
        return 0;
    } catch (const h2v::Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
        return 2;
    }
}
