// Stand-alone driver of the per-proof MSM's launch-shape model (csrc/h2v_msm_shape.hpp).  Host code only: built with
// -fsanitize=address,undefined and run as a program (tests/test_msm_shape.py), which compares the output with
// tests/golden/msm_shape_table.txt - the decisions of the functions as they stood in h2v_capi.hip before they moved here.
// One line per case:
//   T n_var n_fix n hint option=value : lpt bs n_seg seg_terms waves : split_on k fixed_bs var_lpt var_bs var_n_seg var_seg_terms : terms_per_lane : max_seg fits
// (the single launch of the T terms; the fixed-base split of the same sum; terms per lane of the multi-term form; the room for
// segments and whether a shape fits one block).  1024 SIMDs: an MI355X.
#include <cstdio>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_msm_shape.hpp"

// (T, per-proof terms, VK-base terms): simple_mul 16 = 10 + 6, lookup_table 34 = 25 + 9, wide335 = 64 + 271, wide677 = 76 + 601 as
// the plans have them; 10 and 25 are the per-proof parts of simple_mul and lookup_table, 58 and 64 carry the 24 / 25 per-proof
// terms of secp256k1 / sha256, 96 the 32 of bls12381; the second splits of 16, 34, 58 and 96 put the majority on the other side
struct Sum { uint32_t T, n_var, n_fix; };
static const Sum SUMS[] = {{1, 1, 0}, {2, 1, 1}, {10, 6, 4}, {16, 10, 6}, {16, 6, 10}, {25, 10, 15}, {34, 25, 9}, {34, 9, 25}, {58, 24, 34},
                           {58, 40, 18}, {64, 25, 39}, {65, 25, 40}, {96, 32, 64}, {96, 60, 36}, {335, 64, 271}, {677, 76, 601}};
static const uint32_t NS[] = {1, 8, 64, 255, 256, 1024, 2048, 4096, 8192};
static const uint32_t HINTS[] = {1, 4, 8};
struct Opt { const char *name; MsmModel m; };
static const Opt OPTS[] = {
    {"none=0", {1024.0, 0, 0, 0, 0}},
    {"lpt=1", {1024.0, 1, 0, 0, 0}}, {"lpt=2", {1024.0, 2, 0, 0, 0}}, {"lpt=8", {1024.0, 8, 0, 0, 0}},
    {"bs=64", {1024.0, 0, 64, 0, 0}}, {"bs=256", {1024.0, 0, 256, 0, 0}}, {"bs=512", {1024.0, 0, 512, 0, 0}},
    {"tpl=2", {1024.0, 0, 0, 2, 0}}, {"tpl=3", {1024.0, 0, 0, 3, 0}}, {"tpl=4", {1024.0, 0, 0, 4, 0}},
    {"fix=-1", {1024.0, 0, 0, 0, -1}}, {"fix=1", {1024.0, 0, 0, 0, 1}}, {"fix=4", {1024.0, 0, 0, 0, 4}},
};

int main() {
    for (const Sum &s : SUMS)
        for (const uint32_t n : NS)
            for (const uint32_t hint : HINTS)
                for (const Opt &o : OPTS) {
                    const uint32_t max_seg = msm_max_segments(s.T);
                    const MsmShape single = msm_ladder_shape(o.m, s.T, n, 0.0, true, max_seg);
                    const MsmSplit sp = msm_split_shape(o.m, MsmSplitTerms{s.n_var, s.n_fix, s.T}, n, single, hint, max_seg);
                    const int tpl = msm_terms_per_lane(o.m, hint, n, s.T);
                    const bool fits = msm_ladder_fit(o.m, s.T, n, 0.0, true).cost != 1e300;
                    std::printf("%u %u %u %u %u %s : %u %u %u %u %.0f : %d %u %u %u %u %u %u : %d : %u %d\n", s.T, s.n_var, s.n_fix, n, hint, o.name,
                                single.lpt, single.bs, single.n_seg, single.seg_terms, single.waves,
                                (int)sp.on, sp.k, sp.on ? sp.fix.bs : 0u, sp.on ? sp.var.lpt : 0u, sp.on ? sp.var.bs : 0u, sp.on ? sp.var.n_seg : 0u,
                                sp.on ? sp.var.seg_terms : 0u, tpl, max_seg, (int)fits);
                }
    return 0;
}
