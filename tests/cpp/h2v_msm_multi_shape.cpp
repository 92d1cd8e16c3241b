// Stand-alone driver of the lane shape of the multi-term MSM launch (csrc/h2v_msm_shape.hpp: msm_multi_shape).  Host code only:
// built with -fsanitize=address,undefined and run as a program (tests/test_multi_ladder_model.py), which holds every line to the
// bounds the kernel relies on and to the dealing of tests/multi_ladder_model.py.  The first line is the bound itself:
//   max_halves MSM_MAX_HALVES
// then one line per (T, terms per lane, forced) the launcher admits (tpl <= T <= 256 tpl):
//   T tpl forced : hpl lpp
#include <cstdio>

#include "../../plutus_halo2_verifier_gen_amd/csrc/h2v_msm_shape.hpp"

int main() {
    std::printf("max_halves %d\n", MSM_MAX_HALVES);
    for (uint32_t T = 2; T <= 1024; T++)
        for (int tpl = 2; tpl <= 4; tpl++)
            for (int forced = 0; forced <= 1; forced++) {
                if (T < (uint32_t)tpl || T > 256u * (uint32_t)tpl) continue;
                const MsmMultiShape s = msm_multi_shape(T, tpl, forced != 0);
                std::printf("%u %d %d : %u %u\n", T, tpl, forced, s.hpl, s.lpp);
            }
    return 0;
}
