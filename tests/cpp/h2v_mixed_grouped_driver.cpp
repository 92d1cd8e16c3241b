// Test driver for the grouped form of h2v::verify_mixed / batch_verify / aggregate_mixed / Aggregator (include/h2v.hpp, grouped =
// true: H2V_MIXED_GROUPED / H2V_RLC_GROUPED): a mixed-key batch through the C++ surface, phase 1 of every key in one launch.
//
// usage: h2v_mixed_grouped_driver <plans.txt> <batch.bin>
// plans.txt: one path per line, a plan blob (.bin) or a key description (.json, compiled behind the C-ABI)
// batch.bin: u32 n, then per proof: u32 plan index, u32 len, bytes, u32 n_pi, n_pi * 32 B instances, u32 has_ci, [48 B committed]
// prints "grouped <bits>", "status <one word per proof>", "grouped_fell_back <0|1>", "msm_terms <N_R or 0 after a fall-back>",
// "batch_verify <ok|status>", "workspace <0|1>" (the same verdicts on a multi-plan workspace of two lanes with chunks of three
// proofs), "aggregate <included bits> <the pair's check> <N_R>" and "aggregator <accept bits> <calls verified again>", or
// "error <code> <text>" (exit 2).
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
static uint32_t rd32(const std::vector<uint8_t> &b, size_t &o) {
    if (o + 4 > b.size()) throw std::runtime_error("batch file truncated");
    uint32_t v;
    std::memcpy(&v, b.data() + o, 4);
    o += 4;
    return v;
}
static void take(const std::vector<uint8_t> &b, size_t &o, size_t len, std::vector<uint8_t> &out) {
    if (o + len > b.size()) throw std::runtime_error("batch file truncated");
    out.insert(out.end(), b.begin() + (long)o, b.begin() + (long)(o + len));
    o += len;
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s plans.txt batch.bin\n", argv[0]); return 64; }
    h2v::ShutdownGuard shutdown_last;
    try {
        std::vector<std::unique_ptr<h2v::VerifyingKey>> keys;
        std::vector<const h2v::VerifyingKey *> vks;
        std::ifstream list(argv[1]);
        if (!list) throw std::runtime_error(std::string("cannot open ") + argv[1]);
        for (std::string line; std::getline(list, line);) {
            if (line.empty()) continue;
            std::vector<uint8_t> blob = slurp(line);
            if (line.size() > 5 && line.substr(line.size() - 5) == ".json") blob = h2v::VerifyingKey::compile(std::string(blob.begin(), blob.end()));
            keys.emplace_back(new h2v::VerifyingKey(blob.data(), blob.size(), 0));
            vks.push_back(keys.back().get());
        }
        const std::vector<uint8_t> bb = slurp(argv[2]);
        size_t o = 0;
        const uint32_t n = rd32(bb, o);
        std::vector<uint32_t> plan_of;
        std::vector<uint8_t> proofs, inst, ci;
        std::vector<uint64_t> off{0};
        for (uint32_t i = 0; i < n; i++) {
            plan_of.push_back(rd32(bb, o));
            take(bb, o, rd32(bb, o), proofs);
            off.push_back(proofs.size());
            take(bb, o, (size_t)rd32(bb, o) * 32, inst);
            if (rd32(bb, o)) take(bb, o, 48, ci);
        }
        const h2v_mixed_batch batch{n, plan_of.data(), proofs.data(), off.data(), inst.empty() ? nullptr : inst.data(), ci.empty() ? nullptr : ci.data()};
        auto bits = [](const std::vector<uint8_t> &a) { std::string s; for (uint8_t x : a) s.push_back(x ? '1' : '0'); return s; };
        bool fell_back = false;
        h2v::Workspace multi(vks, n ? n : 1, 2, 3);          // two lanes, chunks of three proofs: ranges cut inside keys and across them
        const h2v::PairVerdicts pp = h2v::verify_mixed(vks, batch, nullptr, true, nullptr, &fell_back, true, true);
        std::printf("grouped %s\nstatus", bits(pp.accept).c_str());
        for (uint32_t s : pp.status) std::printf(" %u", s);
        std::printf("\ngrouped_fell_back %d\n", fell_back ? 1 : 0);
        bool fb_ws = false;
        const h2v::PairVerdicts on_ws = h2v::verify_mixed(vks, batch, multi.handle(), true, nullptr, &fb_ws, true, true);
        uint32_t ok = 0;
        h2v_rlc_timings tm{};
        if (n) h2v::check(h2v_workspace_rlc_result(multi.handle(), 0, &ok, &tm));
        std::printf("msm_terms %u\n", fb_ws ? 0u : tm.msm_terms);
        try {
            h2v::batch_verify(vks, batch, nullptr, true, true);
            std::printf("batch_verify ok\n");
        } catch (const h2v::VerifyError &e) { std::printf("batch_verify %u\n", e.status); }
        std::printf("workspace %d\n", on_ws.accept == pp.accept && on_ws.status == pp.status && fb_ws == fell_back && (n == 0 || (ok != 0) == !fell_back) ? 1 : 0);
        // the aggregate side: the grouped call's pair and included[], then ONE check through the Aggregator
        const h2v::Aggregate ag = h2v::aggregate_mixed(vks, batch, multi.handle(), nullptr, true);
        const h2v::PairVerdicts pv = h2v::check_pairs(*vks[0], std::vector<uint8_t>(ag.pair, ag.pair + 96));
        std::printf("aggregate %s %d %u\n", bits(ag.included).c_str(), pv.accept[0] ? 1 : 0, ag.info.msm_terms);
        h2v::Aggregator agg(true);
        agg.push_mixed(vks, batch);
        std::vector<size_t> again;
        const std::vector<std::vector<uint8_t>> acc = agg.finish(&again);
        std::printf("aggregator %s %zu\n", bits(acc.at(0)).c_str(), again.size());
        return 0;
    } catch (const h2v::Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
        return 2;
    } catch (const std::exception &e) {
        std::printf("error 0 %s\n", e.what());
        return 2;
    }
}
