// Aggregate calls (h2v_aggregate_batch / h2v_aggregate_mixed): the one device step that replaces the batch pairing and
// everything queued behind it.  Included from h2v_capi.hip behind h2v_kernels.hip (uses its curve and compression helpers).
//
// Every chunk of an aggregate call ends with its two sums  R = sum r_i R_i  (36 dwords, canonical Jacobian) and
// L = sum r_i L_i  (36 more) copied into the call's parts buffer [n_parts][2][36] - a lane's own sums are overwritten by its
// next chunk.  When every chunk has finished, ONE launch of k_aggregate_export
//   - adds the parts per side with the complete addition law (g1j_add: infinity, equal and opposite operands all handled):
//     lane t of a side's 128 takes the parts t, t + 128, ... and the 128 partial sums are folded as a tree through LDS
//     (2^22 proofs in chunks of 64 are 65 536 parts: 512 per lane and 7 levels, not 65 536 additions on one lane);
//   - normalises the two totals with one inversion (g1j_to_affine_batch<2>) and writes  compress(L) || compress(R)  as 24
//     dword stores, the format of k_prepare_export.  An infinite total is 0xc0, 0, ...; n_parts = 0 gives (inf, inf).
// One block of 256 threads: threads [0, 128) sum R (side 0 of a part), threads [128, 256) sum L (side 1).
#pragma once

#define AGG_PART_DW 72u        // one part: R then L, 36 dwords each
#define AGG_SIDE_LANES 128u

extern "C" __global__ void __launch_bounds__(256)
k_aggregate_export(const uint32_t *__restrict__ parts, uint32_t n_parts, uint32_t *__restrict__ pair /* 24 dwords */) {
    __shared__ uint32_t red[36 * 256];
    const uint32_t t = threadIdx.x, side = t / AGG_SIDE_LANES, tl = t % AGG_SIDE_LANES;
    G1J acc;
    g1j_set_inf(acc);
#pragma unroll 1
    for (uint32_t q = tl; q < n_parts; q += AGG_SIDE_LANES) {
        const uint32_t *src = parts + (size_t)q * AGG_PART_DW + side * 36;
        G1J o;
#pragma unroll
        for (int k = 0; k < 12; k++) { o.x.v[k] = src[k]; o.y.v[k] = src[12 + k]; o.z.v[k] = src[24 + k]; }
        g1j_add(acc, acc, o);
    }
#define AGG_STORE()                                                                                                          \
    do {                                                                                                                     \
        _Pragma("unroll") for (int k = 0; k < 12; k++) {                                                                     \
            red[k * 256 + t] = acc.x.v[k]; red[(12 + k) * 256 + t] = acc.y.v[k]; red[(24 + k) * 256 + t] = acc.z.v[k];       \
        }                                                                                                                    \
    } while (0)
    AGG_STORE();
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = AGG_SIDE_LANES / 2; s >= 1; s >>= 1) {
        // (a level whose upper half holds nothing but infinity - few parts - costs its barrier and no addition)
        if (tl < s && tl + s < n_parts) {
            G1J o;
#pragma unroll
            for (int k = 0; k < 12; k++) { o.x.v[k] = red[k * 256 + t + s]; o.y.v[k] = red[(12 + k) * 256 + t + s]; o.z.v[k] = red[(24 + k) * 256 + t + s]; }
            g1j_add(acc, acc, o);
            AGG_STORE();
        }
        __syncthreads();
    }
#undef AGG_STORE
    if (t != 0) return;
    G1J j[2];   // L, R: the order of the exported pair
#pragma unroll
    for (int k = 0; k < 12; k++) {
        j[0].x.v[k] = red[k * 256 + AGG_SIDE_LANES]; j[0].y.v[k] = red[(12 + k) * 256 + AGG_SIDE_LANES]; j[0].z.v[k] = red[(24 + k) * 256 + AGG_SIDE_LANES];
    }
    j[1] = acc;
    G1A a[2];
    g1j_to_affine_batch<2>(a, j);
#pragma unroll 1
    for (int q = 0; q < 2; q++) {
        uint8_t enc[48];
        g1_compress_dev(enc, a[q]);
#pragma unroll
        for (int k = 0; k < 12; k++)
            pair[12 * q + k] = (uint32_t)enc[4 * k] | ((uint32_t)enc[4 * k + 1] << 8) | ((uint32_t)enc[4 * k + 2] << 16) | ((uint32_t)enc[4 * k + 3] << 24);
    }
}
