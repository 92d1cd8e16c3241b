// Per-proof pairing: the engine table and the selection rule.  Which of the six engines (h2v_kernels.hip: k_pairing_check,
// h2v_pairing_six.hpp, h2v_pairing_coop.hpp) runs for a launch of n proofs, on what grid, which engines the tuner tries and which
// H2V_OPT_PAIRING_ENGINE values are legal.  HOST CODE ONLY - no HIP call and no HIP header in this file, so that a stand-alone C++
// program can include and test it (tests/cpp/h2v_pairing_engine.cpp): every function is a pure function of its arguments.
// h2v_capi.hip passes the device's SIMD count, the workspace's option and hint and launches what these functions decide.
// The k_pairing_rlc kernels are no per-proof engines and are not in here.
#pragma once
#include <stdint.h>

// One row per engine.  option: the H2V_OPT_PAIRING_ENGINE value that forces it, which is also the lanes per proof that
// h2v_timings.pairing_lanes_per_proof and the probes' lanes_out report; impl: the probes' number for "this engine whatever n";
// per_wave: proofs per 64-lane wave (a block is one wave).  The rows' order is PairingEngine's.
enum PairingEngine { PE_ONE_LANE, PE_SIX, PE_TWELVE, PE_NARROW, PE_COOP32, PE_WIDE, PE_COUNT };
struct PairingEngineRow { const char *name; int32_t option; int impl; uint32_t per_wave; };
static constexpr PairingEngineRow PAIRING_ENGINES[PE_COUNT] = {
    {"one_lane", 1, 0, 64},   // the cross-check kernel: one lane per proof
    {"six", 6, 5, 10},        // needs the plan-load line table (H2vDevPlan::six_norm28)
    {"twelve", 12, 6, 5},     // the narrow engine packed five proofs to a wave
    {"narrow", 16, 2, 4},     // one lane per coefficient
    {"coop32", 32, 4, 2},     // the normal engine; the only one with a conditional form (skip flags)
    {"wide", 64, 3, 1},       // four lanes per coefficient
};
// the probes' other impl values: the rule below, without (-1, and any number that names nothing) or with (1) the thread's
// H2V_OPT_PAIRING_ENGINE.  A pipeline's launch is impl 1 with the workspace's option and hint.
enum { PAIRING_IMPL_DEFAULT = -1, PAIRING_IMPL_RULE = 1 };
// The probes give no in-flight hint: wide up to #SIMDs, then the normal engine, no other preference.  Hint 0 stands for that;
// h2v_workspace_hint_in_flight cannot set it.
enum { PAIRING_HINT_PROBE = 0 };

static inline int pairing_engine_of_option(int32_t option) {
    for (int e = 0; e < PE_COUNT; e++) if (PAIRING_ENGINES[e].option == option) return e;
    return -1;
}
static inline int pairing_engine_of_impl(int impl) {
    for (int e = 0; e < PE_COUNT; e++) if (PAIRING_ENGINES[e].impl == impl) return e;
    return -1;
}
// H2V_OPT_PAIRING_ENGINE: 0 (the rule) or an engine's option value
static inline bool pairing_option_legal(int32_t value) { return value == 0 || pairing_engine_of_option(value) >= 0; }
static inline uint32_t pairing_grid(PairingEngine e, uint32_t n) { return (n + PAIRING_ENGINES[e].per_wave - 1) / PAIRING_ENGINES[e].per_wave; }
// The conditional form (the normal engine behind skip flags, the fall-back of a batch check): a walking grid of one wave per SIMD -
// finding out that the launch is not needed costs a few microseconds, and a launch that IS needed has the whole chip.
static inline uint32_t pairing_grid_behind(double n_simd, uint32_t n) {
    const uint32_t cap = 4 * (uint32_t)(n_simd / 4.0), nb = pairing_grid(PE_COOP32, n);
    return nb < cap ? nb : cap;
}

// The launcher's own choice for n proofs on S SIMDs from a caller with `hint` batches in flight; six_ok: the six-lane engine may be
// chosen (the plan has its line table).
static inline PairingEngine pairing_rule(double S, uint32_t n, uint32_t hint, bool six_ok) {
    const bool probe = hint == PAIRING_HINT_PROBE, full = hint >= 4, many = hint >= 8;
    // The SIX-lane engine (ten proofs per wave, h2v_pairing_six.hpp: a quarter fewer instructions per pairing than the narrow
    // one, a chain almost twice as long) wherever a caller that keeps the chip full would take the narrow one
    // from 4 * #SIMDs proofs up (410 waves; with eight or more batches in flight from 3 * #SIMDs: simple_mul x 3072 2.85 -> 2.69 ms per
    // batch against the twelve-lane engine, x 2048 the same either way).  ms per step, narrow -> six: simple_mul x 4096
    // 4.06 -> 3.88 with six batches in flight, 3.76 with eight; below that size its few long waves lose: lookup_table x 2048
    // 3.48 -> 3.65, atms x 2048 3.92 -> 5.10.
    if (six_ok && full && (double)n >= (many ? 3.0 : 4.0) * S) return PE_SIX;
    // The WIDE engine (one proof per wave, four lanes per coefficient: 3 / 2 / 1 terms per lane and call instead of 6 / 4 / 2)
    // when even one wave per proof leaves SIMDs free: n <= #SIMDs.  Above that the two-proofs-per-wave kernel does less
    // total work.  The conditional (RLC fall-back) launch is never wide.
    // (the wide engine issues twice the instructions of the normal one: a caller that keeps the chip full takes it only up to
    // #SIMDs / 2 proofs - sha256 shape x 1024, four in flight: wide 3.18, normal 2.98, narrow 3.12 ms per step; secp256k1 x 512:
    // wide 2.37, normal 2.47, narrow 2.64)
    // Eight or more batches in flight (the library's lanes): the chip is full whatever one launch brings, so the engine with the
    // fewest instructions that still has waves to spread wins much earlier - wide (2 x the normal engine's instructions) only up
    // to #SIMDs / 16 proofs, narrow from 3/8 #SIMDs.  ms per batch, wide / normal / narrow: secp256k1 shape x 64 0.55 / 0.58 / 0.63;
    // sha256 shape x 128 0.67 / 0.66 / 0.72; x 256 1.15 / 1.08 / 1.06; x 512 1.61 / 1.43 / 1.47; secp256k1 x 512 1.67 / 1.57 / 1.55;
    // simple_mul x 512 1.02 / 0.88 / 0.84; x 1024 - / 1.47 / 1.39; sha256 x 1024 - / 2.19 / 2.16.
    if ((double)n <= (many ? S / 16.0 : full ? S / 2.0 : S)) return PE_WIDE;
    // The NARROW engine (four proofs per wave, one lane per coefficient: 21 % fewer instructions per pairing, twice the chain).
    // Measured (simple_mul, pairing kernel alone / step with five batches in flight):
    //   n = 1536: normal 1.94 ms / 2.32 ms, narrow 2.60 / 2.40      n = 2048: 1.96 / 2.71, 2.61 / 2.64
    //   n = 3072: 2.99 / 3.71, 2.63 / 3.46     n = 4096: 3.00 / 4.81, 2.66 / 4.50     n = 8192: 5.65 / 9.59, 6.59 / 8.91
    // (a narrow block needs 22.5 KB of LDS: seven per CU, so its second wave per SIMD does not fit everywhere).  Rule: a caller
    // that keeps the chip full (hint >= 4) takes it from 2 * #SIMDs proofs up; one step at a time takes it exactly where the
    // normal kernel needs a second wave per SIMD and the narrow one does not.
    // (round 4, from the tuner's measurements: at #SIMDs / 4 proofs - sha256 / secp256k1 shape x 256 - the normal engine beats the
    //  twelve-lane one by 8-12 % in every run, 0.77-0.80 against 0.85-0.90 ms per batch; at x 512 neither wins by 3 %: the border is 3/8)
    const bool narrow = probe ? false : many ? (double)n >= 3.0 * S / 8.0 : full ? (double)n >= 2.0 * S : ((double)n > 2.0 * S && (double)n <= 4.0 * S);
    if (!narrow) return PE_COOP32;
    // ... and where the narrow engine would run, its twelve-lane packing (five proofs per wave instead of four with four idle lanes
    // each; the line products in a pass of their own): ms per batch, narrow -> twelve: sha256 shape x 1024 1.99 -> 1.96, secp256k1 x 512
    // 1.21 -> 1.17, lookup_table x 2048 3.26 -> 3.16, atms x 2048 3.40 -> 3.34, simple_mul x 1024 1.24 -> 1.17.
    return many ? PE_TWELVE : PE_NARROW;
}
// The engine of a launch.  option: H2V_OPT_PAIRING_ENGINE (0: the rule); six_table: the plan has the six-lane engine's line table (a
// plan without one - some line coefficient c is zero - never takes that engine); probe_impl: the impl argument of
// h2v_probe_pairing_states, whose launch has no hint (pass PAIRING_HINT_PROBE); a pipeline's is PAIRING_IMPL_RULE.  An impl that
// names an engine wins over the option, and every other impl but PAIRING_IMPL_RULE ignores it.
//
// Two answers that a reader would not guess.  They are what the launcher has always done, are recorded in
// tests/golden/pairing_engine_table.txt, and each is one line here for whoever decides to change it:
//  (1) a forced one-lane engine (option 1) still gives way to the twelve-lane engine wherever the rule, six-lane engine aside,
//      would run that one: hint >= 8 and n >= 3/8 #SIMDs;
//  (2) a forced six-lane engine on a plan without the line table falls to no one engine but back into the rule.
static inline PairingEngine pairing_engine(double S, int32_t option, uint32_t n, uint32_t hint, bool six_table, int probe_impl = PAIRING_IMPL_RULE) {
    int want = pairing_engine_of_impl(probe_impl);
    if (want < 0 && probe_impl == PAIRING_IMPL_RULE) want = pairing_engine_of_option(option);
    if (want < 0) return pairing_rule(S, n, hint, six_table);
    if (want == PE_ONE_LANE && pairing_rule(S, n, hint, false) == PE_TWELVE) return PE_TWELVE;   // (1)
    if (want == PE_SIX && !six_table) return pairing_rule(S, n, hint, false);                     // (2)
    return (PairingEngine)want;
}

// h2v_workspace_tune: the engines (option values) it measures against the rule's choice for m proofs per launch - the rule's
// neighbours at that size.  Returns their number.
static inline int pairing_tune_candidates(double S, uint32_t m, const int32_t **out) {
    static constexpr int32_t full[] = {6, 12, 16}, mid[] = {12, 16, 32}, low[] = {32, 64};
    *out = (double)m >= 2.0 * S ? full : (double)m >= S / 4.0 ? mid : low;
    return (double)m >= S / 4.0 ? 3 : 2;
}
