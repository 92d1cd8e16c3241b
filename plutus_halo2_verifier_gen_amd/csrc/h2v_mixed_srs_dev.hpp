// Mixed-key calls across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS), device side: the memory-bound kernels that put a
// call's left-hand terms CLASS-MAJOR, so that every SRS class is one contiguous bucket-MSM problem, and that carry the per-pair
// fall-back of the pairs form between the caller's order and the classes' slices.  pos[q]: the call position of class-major slot q
// (h2v_mixed_srs.hpp: Classes::pos), in the call's table block.
//   k_across_lterms    Form B: the L-terms of the fold form - scalars by call position (k_mixed_terms / k_mixed_pair_terms wrote
//                      them) - as class-major scalars and point indices into the call-position point pool
//   k_across_coeff     Form A: r for slot q = low 128 bits of B(seed' || LE32(q)) - the CLASS-MAJOR position, no chunk tweak -, 1 if
//                      0, 0 for a proof that takes no part; r_scal[q], the point indices of the pair at pos[q], good by call position
//   k_across_gather    behind the check's skip flags: the pairs and status words of the call, class-major, side by side
//   k_across_scatter   behind the same flags: accept / status of the per-pair kernels back at the call positions
// Included behind h2v_mixed_fold_dev.hpp (mixed_coeff).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one lane per slot: two 16-byte loads and stores of the scalar, one index
extern "C" __global__ void __launch_bounds__(256)
k_across_lterms(uint32_t n, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ l_scal, uint32_t *__restrict__ cl_scal, uint32_t *__restrict__ cl_idx) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const uint32_t at = pos[q];
    const uint4 *s = (const uint4 *)(l_scal + (size_t)at * 8);
    uint4 *d = (uint4 *)(cl_scal + (size_t)q * 8);
    d[0] = s[0]; d[1] = s[1];
    cl_idx[q] = at;
}

struct AcrossCoeffArgs {
    uint32_t n;
    const uint32_t *pos;        // n: slot -> call position
    const uint8_t *good_in;     // by call position (the sub-batches wrote it)
    uint32_t seed[8];
    uint32_t *scal, *l_idx, *r_idx;     // n x 8, n, n: by slot
    uint8_t *good;              // by call position: what the pairing's epilogue copies to accept[]
    const uint32_t *seed_dev;   // as MixedTermsArgs
};
extern "C" __global__ void __launch_bounds__(64)
k_across_coeff(AcrossCoeffArgs a) {
    __shared__ uint32_t sbuf[32 * 64];
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x * 64 + lane;
    const bool live = q < a.n;
    const uint32_t qq = live ? q : a.n - 1;
    const uint32_t at = a.pos[qq];
    const bool good = live && a.good_in[at] != 0;
    uint32_t r[4];
    mixed_coeff(r, a, qq, good, sbuf, lane);
    if (!live) return;
    uint4 *d = (uint4 *)(a.scal + (size_t)q * 8);
    d[0] = make_uint4(r[0], r[1], r[2], r[3]); d[1] = make_uint4(0u, 0u, 0u, 0u);
    a.l_idx[q] = 2 * at;
    a.r_idx[q] = 2 * at + 1;
    a.good[at] = good ? 1 : 0;
}

// a pair is 12 records of 16 bytes: lane t of the walk copies record t % 12 of slot t / 12 - the stores are dense, the loads dense
// within a pair -, and the lane of a pair's first record takes its status word along
extern "C" __global__ void __launch_bounds__(256)
k_across_gather(uint32_t n, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ pool, const uint32_t *__restrict__ status,
                const uint32_t *__restrict__ skip, uint32_t *__restrict__ pool_g, uint32_t *__restrict__ status_g) {
    if (skip && skip[0]) return;
    const uint64_t total = (uint64_t)n * 12;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const uint32_t q = (uint32_t)(t / 12), j = (uint32_t)(t % 12), at = pos[q];
        ((uint4 *)pool_g)[t] = ((const uint4 *)pool)[(uint64_t)at * 12 + j];
        if (j == 0) status_g[q] = status[at];
    }
}
extern "C" __global__ void __launch_bounds__(256)
k_across_scatter(uint32_t n, const uint32_t *__restrict__ pos, const uint8_t *__restrict__ accept_g, const uint32_t *__restrict__ status_g,
                 const uint32_t *__restrict__ skip, uint8_t *__restrict__ accept, uint32_t *__restrict__ status) {
    if (skip && skip[0]) return;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const uint32_t at = pos[q];
        accept[at] = accept_g[q];
        status[at] = status_g[q];
    }
}
