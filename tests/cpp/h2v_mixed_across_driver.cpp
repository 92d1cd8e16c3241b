// Test driver for h2v::verify_mixed / h2v::batch_verify with across_srs = true (include/h2v.hpp; H2V_MIXED_ACROSS_SRS): a mixed-key
// batch whose keys are on several SRS through the C++ surface, ONE multi-pairing for the call.
//
// usage: h2v_mixed_across_driver <plans.txt> <batch.bin>
// plans.txt: one path per line, a plan blob (.bin) or a key description (.json, compiled behind the C-ABI)
// batch.bin: u32 n, then per proof: u32 plan index, u32 len, bytes, u32 n_pi, n_pi * 32 B instances, u32 has_ci, [48 B committed]
// prints "pairs <bits>" / "pairs_fell_back <0|1>" (the form without fold_msm), "fold <bits>" / "fold_fell_back <0|1>" (with it),
// "status <one word per proof>" (the fold form's), "one_srs <code>" (the same call WITHOUT the flag: its error code, 0 = none),
// "batch_verify <ok|status>" and "workspace <0|1>" (the same verdicts on a multi-plan workspace of two lanes with chunks of three
// proofs), or "error <code> <text>" (exit 2).
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
        bool fb_pairs = false, fb_fold = false, fb_ws = false;
        h2v::Workspace multi(vks, n ? n : 1, 2, 3);          // two lanes, chunks of three proofs
        const h2v::PairVerdicts pp = h2v::verify_mixed(vks, batch, nullptr, true, nullptr, &fb_pairs, false, false, false, true);
        std::printf("pairs %s\npairs_fell_back %d\n", bits(pp.accept).c_str(), fb_pairs ? 1 : 0);
        const h2v::PairVerdicts pf = h2v::verify_mixed(vks, batch, nullptr, true, nullptr, &fb_fold, true, false, false, true);
        std::printf("fold %s\nfold_fell_back %d\nstatus", bits(pf.accept).c_str(), fb_fold ? 1 : 0);
        for (uint32_t s : pf.status) std::printf(" %u", s);
        std::printf("\n");
        int one_srs = 0;
        try { (void)h2v::verify_mixed(vks, batch, nullptr, true); } catch (const h2v::Error &e) { one_srs = e.code; }
        std::printf("one_srs %d\n", one_srs);
        const h2v::PairVerdicts on_ws = h2v::verify_mixed(vks, batch, multi.handle(), true, nullptr, &fb_ws, true, true, false, true);
        uint32_t ok = 0;
        if (n) h2v::check(h2v_workspace_rlc_result(multi.handle(), 0, &ok, nullptr));
        try {
            h2v::batch_verify(vks, batch, nullptr, true, false, false, true);
            std::printf("batch_verify ok\n");
        } catch (const h2v::VerifyError &e) { std::printf("batch_verify %u\n", e.status); }
        std::printf("workspace %d\n", on_ws.accept == pf.accept && on_ws.status == pf.status && pp.status == pf.status && fb_ws == fb_fold && (n == 0 || (ok != 0) == !fb_fold) ? 1 : 0);
        return 0;
    } catch (const h2v::Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
        return 2;
    } catch (const std::exception &e) {
        std::printf("error 0 %s\n", e.what());
        return 2;
    }
}
