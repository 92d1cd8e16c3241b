// The division-step inverter (csrc/h2v_modinv.hpp) as a host program: the header itself, compiled for the CPU with the device
// qualifiers defined away, on operands given on stdin plus seeded random ones, every result checked against an independent
// computation (h2v_hostmath.hpp: x * out == 1 by a 64-bit-word Montgomery product, and out < M).  Host code only, its own
// main; tests/test_inverter_paths.py builds it with ASan + UBSan and runs it as a program.
//
// stdin: lines "FP <hex>" / "FR <hex>", 0 < value < modulus.  argv[1]: random operands per field (default 50000).
// stdout: one line per field, "<field> stdin <n> random <n> ok <n>".  Exit status 1 and a line on stderr per wrong result.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __device__
#define H2V_DI inline
#include "../../plutus_halo2_verifier_gen_amd/csrc/bls_consts.h"
#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_modinv.hpp"
#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_hostmath.hpp"

static uint64_t rng_state;
static uint64_t next64() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <int L, int NW, int N>
struct Run {
    const char *name;
    const h2vhost::Field<N> &F;
    const uint32_t *mod30;
    uint32_t minv30;
    long from_stdin = 0, from_rng = 0, ok = 0, bad = 0;

    static h2vhost::UInt<N> wide(const uint32_t (&w)[NW]) {
        h2vhost::UInt<N> r;
        for (int i = 0; i < NW; i++) r.w[i / 2] |= (uint64_t)w[i] << (32 * (i % 2));
        return r;
    }
    void one(const h2vhost::UInt<N> &x) {
        uint32_t in[NW], out[NW];
        for (int i = 0; i < NW; i++) in[i] = (uint32_t)(x.w[i / 2] >> (32 * (i % 2)));
        ModInv30<L>::template inverse<NW>(out, in, mod30, minv30);
        const h2vhost::UInt<N> y = wide(out);
        if (y < F.p && F.mul(F.to_mont(x), y) == h2vhost::UInt<N>(1)) { ok++; return; }
        bad++;
        fprintf(stderr, "%s: wrong inverse of ", name);
        for (int i = NW - 1; i >= 0; i--) fprintf(stderr, "%08x", in[i]);
        fprintf(stderr, "\n");
    }
    bool valid(const h2vhost::UInt<N> &x) const { return !x.is_zero() && x < F.p; }
    void random(long n, uint64_t seed) {
        rng_state = seed;
        const int top = F.p.bits();
        while (from_rng < n) {
            h2vhost::UInt<N> x;
            for (int i = 0; i < N; i++) x.w[i] = next64();
            for (int k = top; k < 64 * N; k++) x.w[k >> 6] &= ~(1ull << (k & 63));
            if (!valid(x)) continue;
            from_rng++;
            one(x);
        }
    }
    void report() const { printf("%s stdin %ld random %ld ok %ld\n", name, from_stdin, from_rng, ok); }
};

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? atol(argv[1]) : 50000;
    Run<13, 12, 6> fp{"FP", h2vhost::FP(), FP_MOD30, FP_MINV30};
    Run<9, 8, 4> fr{"FR", h2vhost::FR(), FR_MOD30, FR_MINV30};
    char tag[8], hex[128];
    int bad_lines = 0;
    while (scanf("%7s %127s", tag, hex) == 2) {
        try {
            if (!strcmp(tag, "FP")) {
                const h2vhost::U384 x = h2vhost::from_hex<6>(hex);
                if (!fp.valid(x)) throw std::invalid_argument("range");
                fp.from_stdin++;
                fp.one(x);
            } else if (!strcmp(tag, "FR")) {
                const h2vhost::U256 x = h2vhost::from_hex<4>(hex);
                if (!fr.valid(x)) throw std::invalid_argument("range");
                fr.from_stdin++;
                fr.one(x);
            } else {
                throw std::invalid_argument("field");
            }
        } catch (const std::invalid_argument &) {
            fprintf(stderr, "bad input line: %s %s\n", tag, hex);
            bad_lines++;
        }
    }
    fp.random(n_random, 1);
    fr.random(n_random, 2);
    fp.report();
    fr.report();
    return (fp.bad || fr.bad || bad_lines) ? 1 : 0;
}
