// Stand-alone driver of csrc/h2v_planblob.hpp (host code only; built with -fsanitize=address,undefined by
// tests/test_plan_blob.py).  Every blob it parses lives in a heap block of EXACTLY its length, so that one byte read past the end is
// an AddressSanitizer report.
//   corpus <cases> <dir>  one line per case of <cases> ("id plan cut n_patches {offset hex}*", cut -1 = none; <dir>/<plan>.bin is the
//                         plan): "id<TAB>valid" or "id<TAB>code<TAB>message", as tests/golden/plan_load_verdicts.txt has them; an
//                         accepted blob also goes through device_terms, fixed_tables and six_line_tables
//   six <blob>            the dwords of six_line_tables, one per line, or "no table"
//   ops                   the opcode table: "op reads_a reads_b writes transcript serial"
//   slots <file>          per line of 96 hex digits (a canonical Fp value): its 64-byte operand slot in hex, after a round trip
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_planblob.hpp"

static std::vector<uint8_t> read_file(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s: %s\n", id.c_str(), #cond); exit(1); } } while (0)

// what the loader does with an accepted blob on the host
static void derive(const std::string &id, const uint8_t *blob, size_t len, const planblob::View &v) {
    const std::vector<uint8_t> terms = planblob::device_terms(blob, v);
    REQUIRE(terms.size() == 8 * (size_t)v.n_terms);
    for (uint32_t k = 0; k < v.n_terms; k++) {
        const uint32_t kind = planblob::rd32(terms.data() + 8 * k), idx = planblob::rd32(terms.data() + 8 * k + 4);
        REQUIRE(kind == H2V_TERM_PROOF_POINT ? idx < H2V_SLOTS(v) : kind == H2V_TERM_VK_BASE && idx < v.n_bases);
    }
    REQUIRE(v.n_var + v.n_fix == (v.n_fix ? v.n_terms : 0u));
    REQUIRE(v.trace_slots.size() == v.n_trace);
    for (uint32_t bits : {0u, 4u, 8u, 12u}) {
        const planblob::FixedTables ft = planblob::fixed_tables(v.n_bases, bits);
        REQUIRE((bits == 0 || ft.c == bits) && ft.entries == 1u << (ft.c - 1) && ft.W == (256 + ft.c) / ft.c);
        REQUIRE(ft.bytes == (size_t)v.n_bases * ft.W * ft.entries * 112);
        REQUIRE(bits != 0 || ft.c == 12 || (size_t)v.n_bases * 22 * 2048 * 112 > ((size_t)2 << 30));
    }
    std::vector<uint32_t> six;
    if (planblob::six_line_tables(blob, v, six)) REQUIRE(six.size() == planblob::SIX_NORM_DW + 96);
    uint64_t dg[2];
    uint8_t tag[32];
    planblob::sg2_digest(blob, v, dg);
    planblob::key_tag(blob, len, tag);
    if (v.tr_kind == H2V_TR_BLAKE2B_512) { uint64_t h0[8]; REQUIRE(planblob::transcript_midstate(blob, v, h0) == (v.tr_key_len ? 128u : 0u)); }
}

static int run_corpus(const char *cases_path, const std::string &dir) {
    std::ifstream cases(cases_path);
    std::map<std::string, std::vector<uint8_t>> plans;
    std::string line;
    while (std::getline(cases, line)) {
        std::istringstream in(line);
        std::string id, plan;
        long cut;
        int n_patches;
        in >> id >> plan >> cut >> n_patches;
        if (!plans.count(plan)) plans[plan] = read_file(dir + "/" + plan + ".bin");
        std::vector<uint8_t> m = plans[plan];
        for (int q = 0; q < n_patches; q++) {
            size_t off;
            std::string hex;
            in >> off >> hex;
            std::vector<uint8_t> bytes;
            REQUIRE(h2vhost::hex_to_bytes(hex, bytes) && off + bytes.size() <= m.size());
            memcpy(m.data() + off, bytes.data(), bytes.size());
        }
        REQUIRE(!in.fail());
        const size_t len = cut < 0 ? m.size() : (size_t)cut;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);      // (len = 0: a block of no bytes at all)
        memcpy(exact.get(), m.data(), len);
        planblob::View v;
        std::string err;
        const int rc = planblob::parse(exact.get(), len, v, err);
        if (rc == H2V_OK) {
            derive(id, exact.get(), len, v);
            printf("%s\tvalid\n", id.c_str());
        } else {
            REQUIRE(rc == H2V_E_PLAN || rc == H2V_E_LIMIT);
            printf("%s\t%d\t%s\n", id.c_str(), rc, err.c_str());
        }
    }
    return 0;
}

static int run_six(const char *path) {
    const std::vector<uint8_t> m = read_file(path);
    const std::string id = path;
    planblob::View v;
    std::string err;
    REQUIRE(planblob::parse(m.data(), m.size(), v, err) == H2V_OK);
    std::vector<uint32_t> six;
    if (!planblob::six_line_tables(m.data(), v, six)) { printf("no table\n"); return 0; }
    for (uint32_t dw : six) printf("%08x\n", dw);
    return 0;
}

static int run_ops() {
    for (int op = 0; op < H2V_OP_COUNT; op++)
        printf("%d %d %d %d %d %d\n", op, h2v_op_reads_a(op), h2v_op_reads_b(op), h2v_op_writes(op), h2v_op_transcript(op), H2V_OPS[op].serial);
    const std::string id = "ops";
    REQUIRE(!h2v_op_known(H2V_OP_COUNT) && !h2v_op_known(255) && !h2v_op_reads_a(H2V_OP_COUNT) && !h2v_op_writes(255));
    // 154624 bytes: 75 registers x 64 proofs on one lane, 151 x 32 on two, 2416 x 2 on 32
    REQUIRE(vm_fits_lds(75, 1) && !vm_fits_lds(76, 1) && vm_fits_lds(151, 2) && !vm_fits_lds(152, 2) && vm_fits_lds(2416, 32) && !vm_fits_lds(2417, 32));
    return 0;
}

static int run_slots(const char *path) {
    std::ifstream f(path);
    std::string id;
    while (f >> id) {
        const h2vhost::FpE x = h2vhost::fp_from_canonical(h2vhost::from_hex<6>(id.c_str()));
        uint32_t slot[16] = {};
        h2vhost::fp_to_limbs28(x, slot);
        REQUIRE(h2vhost::fp_eq(h2vhost::fp_from_limbs28(slot), x));
        for (uint32_t dw : slot) printf("%02x%02x%02x%02x", dw & 255, (dw >> 8) & 255, (dw >> 16) & 255, dw >> 24);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "corpus" && argc == 4) return run_corpus(argv[2], argv[3]);
    if (mode == "six" && argc == 3) return run_six(argv[2]);
    if (mode == "ops") return run_ops();
    if (mode == "slots" && argc == 3) return run_slots(argv[2]);
    fprintf(stderr, "usage: h2v_planblob corpus <cases> <dir> | six <blob> | ops | slots <file>\n");
    return 2;
}
