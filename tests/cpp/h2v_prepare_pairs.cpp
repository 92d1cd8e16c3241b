// The prepare / pair-check wrappers of include/h2v.hpp: h2v::prepare_batch, h2v::check_pairs and Guard::dual_msm.
// Usage: h2v_prepare_pairs PLAN_BLOB BATCH_FILE  (the files of tests/cpp/h2v_cpp_driver.cpp).  Prints one line per proof:
// "<status> <accept of check_pairs> <left hex> <right hex>", then "dual_msm <0|1>" for proof 0 (1: the pair Guard::dual_msm
// gives equals the batch's).  Exit 0 on success, 2 on an h2v::Error (its code first).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "h2v.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void hex(const uint8_t *p, size_t n) {
    for (size_t k = 0; k < n; k++) printf("%02x", p[k]);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s PLAN_BLOB BATCH_FILE\n", argv[0]);
        return 1;
    }
    h2v::ShutdownGuard shutdown_guard;
    try {
        const std::vector<uint8_t> plan = slurp(argv[1]), blob = slurp(argv[2]);
        h2v::VerifyingKey vk(plan.data(), plan.size());
        const uint32_t n = rd32(&blob[0]), n_pi = rd32(&blob[4]);
        std::vector<uint8_t> proofs, inst;
        std::vector<uint64_t> off{0};
        size_t at = 12;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t len = rd32(&blob[at]);
            at += 4;
            proofs.insert(proofs.end(), blob.begin() + at, blob.begin() + at + len);
            at += len;
            off.push_back(proofs.size());
            inst.insert(inst.end(), blob.begin() + at, blob.begin() + at + 32 * n_pi);
            at += 32 * n_pi;
        }
        const h2v_batch batch = {n, proofs.data(), off.data(), inst.empty() ? nullptr : inst.data(), nullptr};
        const h2v::PreparedBatch prep = h2v::prepare_batch(vk, batch);
        const h2v::PairVerdicts chk = h2v::check_pairs(vk, prep.pairs);
        for (uint32_t i = 0; i < n; i++) {
            printf("%u %u ", prep.status[i], chk.accept[i]);
            hex(&prep.pairs[96 * i], 48);
            printf(" ");
            hex(&prep.pairs[96 * i + 48], 48);
            printf("\n");
        }
        if (n && prep.status[0] == 0) {
            h2v::CircuitTranscript t = h2v::CircuitTranscript::init_from_bytes(std::vector<uint8_t>(proofs.begin(), proofs.begin() + off[1]));
            std::vector<std::vector<uint8_t>> scalars;
            for (uint32_t k = 0; k < n_pi; k++) scalars.emplace_back(inst.begin() + 32 * k, inst.begin() + 32 * (k + 1));
            h2v::Guard g = h2v::prepare(vk, {}, scalars, t);
            const h2v::DualMSM m = g.dual_msm();
            bool same = true;
            for (int k = 0; k < 48; k++) same = same && m.left[k] == prep.pairs[k] && m.right[k] == prep.pairs[48 + k];
            printf("dual_msm %d %d\n", same ? 1 : 0, m.check(vk) ? 1 : 0);
        }
    } catch (const h2v::Error &e) {
        printf("error %d %s\n", e.code, e.what());
        return 2;
    } catch (const h2v::VerifyError &e) {
        printf("verify_error %u\n", e.status);
        return 3;
    }
    return 0;
}
