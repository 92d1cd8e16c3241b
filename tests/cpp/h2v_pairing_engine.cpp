// Stand-alone driver of the per-proof pairing's engine table and selection rule (csrc/h2v_pairing_engine.hpp).  Host code only:
// built with -fsanitize=address,undefined and run as a program (tests/test_pairing_engine_model.py), which compares the output with
// tests/golden/pairing_engine_table.txt - the launches of the chain of conditions as it stood in h2v_capi.hip before it moved there.
// One line per case, the answer as (engine, grid, lanes reported):
//   engine name option impl proofs_per_wave       the engine table
//   pipe n hint six_table option : ...            a pipeline's launch
//   probe n impl six_table option : ...           h2v_probe_pairing_states (no hint)
//   behind n : ...                                the conditional launch behind skip flags
//   tune m : options                              the engines h2v_workspace_tune tries at m proofs per launch
// --simds S (default 1024, an MI355X); --case n hint option six_table: that pipeline line alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_pairing_engine.hpp"

static const uint32_t NS[] = {1, 2, 10, 11, 63, 64, 65, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 8192};
static const uint32_t HINTS[] = {1, 3, 4, 7, 8, 16};
static const int32_t OPTIONS[] = {0, 1, 6, 12, 16, 32, 64};
static const int IMPLS[] = {-1, 0, 1, 2, 3, 5, 6};

static void answer(PairingEngine e, uint32_t grid) { std::printf(" : %s %u %d\n", PAIRING_ENGINES[e].name, grid, (int)PAIRING_ENGINES[e].option); }
static void pipe_line(double S, uint32_t n, uint32_t hint, int table, int32_t opt) {
    const PairingEngine e = pairing_engine(S, opt, n, hint, table != 0);
    std::printf("pipe %u %u %d %d", n, hint, table, (int)opt);
    answer(e, pairing_grid(e, n));
}

int main(int argc, char **argv) {
    double S = 1024.0;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--simds") && a + 1 < argc) S = atof(argv[++a]);
        else if (!strcmp(argv[a], "--case") && a + 4 < argc) {
            pipe_line(S, (uint32_t)atol(argv[a + 1]), (uint32_t)atol(argv[a + 2]), atoi(argv[a + 4]), atoi(argv[a + 3]));
            return 0;
        } else return 2;
    }
    for (const PairingEngineRow &r : PAIRING_ENGINES) std::printf("engine %s %d %d %u\n", r.name, (int)r.option, r.impl, r.per_wave);
    for (const uint32_t n : NS)
        for (const uint32_t hint : HINTS)
            for (int table = 1; table >= 0; table--)
                for (const int32_t opt : OPTIONS) pipe_line(S, n, hint, table, opt);
    for (const uint32_t n : NS)
        for (const int impl : IMPLS)
            for (int table = 1; table >= 0; table--)
                for (const int32_t opt : OPTIONS) {
                    const PairingEngine e = pairing_engine(S, opt, n, PAIRING_HINT_PROBE, table != 0, impl);
                    std::printf("probe %u %d %d %d", n, impl, table, (int)opt);
                    answer(e, pairing_grid(e, n));
                }
    for (const uint32_t n : NS) {
        std::printf("behind %u", n);
        answer(PE_COOP32, pairing_grid_behind(S, n));
    }
    for (const uint32_t m : NS) {
        const int32_t *eng = nullptr;
        const int k = pairing_tune_candidates(S, m, &eng);
        std::printf("tune %u :", m);
        for (int i = 0; i < k; i++) std::printf(" %d", (int)eng[i]);
        std::printf("\n");
    }
    return 0;
}
