// The transcript-hash surface of include/h2v.hpp: VerifyingKey::transcript_kind / transcript_key, the tag types
// CardanoFriendlyBlake2b / Blake2b512 and prepare()'s refusal of a transcript whose tag is not the key's.
// Usage: h2v_transcript_driver VK_JSON BATCH_FILE  (the files of tests/cpp/h2v_cpp_driver.cpp; the key description may name
// either hash).  Prints "kind <k>", "key <hex>", "single <0|1 per proof>" (prepare + verify under the key's own tag),
// "batch <0|1 per proof>", "status <one word per proof>" and "mismatch_refused <0|1>" (prepare under the OTHER tag threw
// h2v::Error(H2V_E_ARG)).  Exit 0 on success, 2 on an h2v::Error (its code first).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "h2v.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

template <class H>
static int verify_one(const h2v::VerifyingKey &vk, const std::vector<uint8_t> &proof, const std::vector<std::vector<uint8_t>> &scalars, uint32_t *status) {
    h2v::Transcript<H> t = h2v::Transcript<H>::init_from_bytes(proof);
    h2v::Guard g = h2v::prepare(vk, {}, scalars, t);
    try {
        g.verify();
    } catch (const h2v::VerifyError &e) {
        *status = e.status;
        return 0;
    }
    *status = 0;
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s VK_JSON BATCH_FILE\n", argv[0]);
        return 1;
    }
    h2v::ShutdownGuard shutdown_guard;
    try {
        const std::vector<uint8_t> json = slurp(argv[1]), blob = slurp(argv[2]);
        const std::vector<uint8_t> plan = h2v::VerifyingKey::compile(std::string(json.begin(), json.end()));
        printf("plan_version %u\n", rd32(&plan[8]));
        h2v::VerifyingKey vk(plan.data(), plan.size());
        const uint32_t kind = vk.transcript_kind();
        printf("kind %u\nkey ", kind);
        for (uint8_t b : vk.transcript_key()) printf("%02x", b);
        printf("\n");
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
        std::string single, st_line;
        bool refused = true;
        for (uint32_t i = 0; i < n; i++) {
            const std::vector<uint8_t> proof(proofs.begin() + off[i], proofs.begin() + off[i + 1]);
            std::vector<std::vector<uint8_t>> scalars;
            for (uint32_t k = 0; k < n_pi; k++) scalars.emplace_back(inst.begin() + (i * n_pi + k) * 32, inst.begin() + (i * n_pi + k + 1) * 32);
            uint32_t st = 0;
            const int ok = kind == h2v::Blake2b512::kind ? verify_one<h2v::Blake2b512>(vk, proof, scalars, &st)
                                                         : verify_one<h2v::CardanoFriendlyBlake2b>(vk, proof, scalars, &st);
            single += ok ? '1' : '0';
            st_line += (i ? " " : "") + std::to_string(st);
            try {   // the other tag: misuse, found before anything is launched
                uint32_t st2 = 0;
                if (kind == h2v::Blake2b512::kind) (void)verify_one<h2v::CardanoFriendlyBlake2b>(vk, proof, scalars, &st2);
                else (void)verify_one<h2v::Blake2b512>(vk, proof, scalars, &st2);
                refused = false;
            } catch (const h2v::Error &e) {
                refused = refused && e.code == H2V_E_ARG;
            }
        }
        printf("single %s\nstatus %s\n", single.c_str(), st_line.c_str());
        const h2v_batch batch = {n, proofs.data(), off.data(), inst.empty() ? nullptr : inst.data(), nullptr};
        std::string bl;
        for (uint8_t a : h2v::verify_batch(vk, batch)) bl += a ? '1' : '0';
        printf("batch %s\nmismatch_refused %d\n", bl.c_str(), refused ? 1 : 0);
    } catch (const h2v::Error &e) {
        printf("error %d %s\n", e.code, e.what());
        return 2;
    }
    return 0;
}
