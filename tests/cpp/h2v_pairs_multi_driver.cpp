// Test driver for h2v::check_pairs_multi (include/h2v.hpp: ONE check over pairs on several SRS, h2v_check_pairs_multi).
//
// usage: h2v_pairs_multi_driver <plans.txt> <pairs.bin>
// plans.txt: one path per line, a plan blob (.bin) - range k of the call is checked against the SRS of line k's key
// pairs.bin: u32 ranges, `ranges` x u32 counts, then (sum counts) x 96 bytes compress(L) || compress(R)
// prints "multi <accept bits>", "status <one word per pair>", "fell_back <0|1>", "per_range <0|1>" (the same verdicts and status
// words from h2v::check_pairs range by range), "workspace <0|1>" (the same on a laned workspace of two lanes with chunks of three,
// with its record's verdict and msm_terms = n), or "error <code> <text>" (exit 2).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "h2v.hpp"

static std::vector<uint8_t> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s plans.txt pairs.bin\n", argv[0]); return 64; }
    h2v::ShutdownGuard shutdown_last;
    try {
        std::vector<std::unique_ptr<h2v::VerifyingKey>> keys;
        std::vector<const h2v::VerifyingKey *> vks;
        std::ifstream list(argv[1]);
        if (!list) throw std::runtime_error(std::string("cannot open ") + argv[1]);
        for (std::string line; std::getline(list, line);) {
            if (line.empty()) continue;
            const std::vector<uint8_t> blob = slurp(line);
            keys.emplace_back(new h2v::VerifyingKey(blob.data(), blob.size(), 0));
            vks.push_back(keys.back().get());
        }
        const std::vector<uint8_t> bb = slurp(argv[2]);
        uint32_t ranges = 0;
        if (bb.size() < 4) throw std::runtime_error("pairs file truncated");
        std::memcpy(&ranges, bb.data(), 4);
        if (ranges != vks.size() || bb.size() < 4 + 4 * (size_t)ranges) throw std::runtime_error("pairs file: one count per key");
        std::vector<uint64_t> counts;
        uint64_t n = 0;
        for (uint32_t k = 0; k < ranges; k++) {
            uint32_t c;
            std::memcpy(&c, bb.data() + 4 + 4 * k, 4);
            counts.push_back(c);
            n += c;
        }
        const std::vector<uint8_t> pairs(bb.begin() + 4 + 4 * (long)ranges, bb.end());
        if (pairs.size() != n * 96) throw std::runtime_error("pairs file: 96 bytes per pair");
        auto bits = [](const std::vector<uint8_t> &a) { std::string s; for (uint8_t x : a) s.push_back(x ? '1' : '0'); return s; };
        bool fell_back = false;
        const h2v::PairVerdicts mv = h2v::check_pairs_multi(vks, counts, pairs, nullptr, nullptr, &fell_back);
        std::printf("multi %s\nstatus", bits(mv.accept).c_str());
        for (uint32_t s : mv.status) std::printf(" %u", s);
        std::printf("\nfell_back %d\n", fell_back ? 1 : 0);
        bool same = true;
        size_t lo = 0;
        for (uint32_t k = 0; k < ranges; k++) {
            const std::vector<uint8_t> part(pairs.begin() + (long)(96 * lo), pairs.begin() + (long)(96 * (lo + counts[k])));
            const h2v::PairVerdicts pv = h2v::check_pairs(*vks[k], part);
            for (size_t i = 0; i < counts[k]; i++) same = same && pv.accept[i] == mv.accept[lo + i] && pv.status[i] == mv.status[lo + i];
            lo += counts[k];
        }
        std::printf("per_range %d\n", same ? 1 : 0);
        h2v::Workspace laned(vks, n ? n : 1, 2, 3);
        bool fb_ws = false;
        const h2v::PairVerdicts on_ws = h2v::check_pairs_multi(vks, counts, pairs, laned.handle(), nullptr, &fb_ws);
        uint32_t ok = 0;
        h2v_rlc_timings tm{};
        if (n) h2v::check(h2v_workspace_rlc_result(laned.handle(), 0, &ok, &tm));
        std::printf("workspace %d\n", on_ws.accept == mv.accept && on_ws.status == mv.status && fb_ws == fell_back && (n == 0 || ((ok != 0) == !fell_back && tm.msm_terms == n)) ? 1 : 0);
        return 0;
    } catch (const h2v::Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
        return 2;
    } catch (const std::exception &e) {
        std::printf("error 0 %s\n", e.what());
        return 2;
    }
}
