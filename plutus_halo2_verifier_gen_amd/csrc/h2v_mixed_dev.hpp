// Mixed-key batches (include/h2v.h: h2v_verify_mixed), device side.  Three small kernels around the per-plan pipelines:
//   k_mixed_offsets   the grouped proof offsets (h2v_mixed.hpp: group_offsets) when the caller's proof_off lives on the device
//   k_mixed_gather    every proof's bytes, public inputs and committed instance from the caller's order into the per-plan
//                     contiguous staging of the workspace: ONE wave per record, 16-byte accesses where source and destination
//                     are aligned alike (heads and tails by bytes), dwords or bytes otherwise
//   k_mixed_pairs     in place of k_prepare_export: each proof's pair (L, R) as a two-slot affine record - the layout of the
//                     workspace's point buffer - at the proof's position in the CALLER's order, with `good` and the
//                     pre-pairing status; one inversion per proof, no compression and no second decompression
// The table they read is built by h2vmixed::partition and uploaded in one copy (h2v_capi.hip: run_mixed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct H2vMixedTab {
    uint32_t n;
    const uint64_t *inst_src, *inst_dst;                               // n each (bytes)
    const uint32_t *perm, *len_cap, *inst_len, *ci_src, *ci_dst;       // n each; ci_*: 48-byte record index or 0xffffffff
};

// dst_off[0 .. n] = running sum over the grouped order of min(length of proof perm[g], len_cap[g]).  One block of 256 threads.
extern "C" __global__ void __launch_bounds__(256)
k_mixed_offsets(const uint64_t *__restrict__ src_off, H2vMixedTab t, uint64_t *__restrict__ dst_off) {
    __shared__ uint64_t part[256];
    const uint32_t th = threadIdx.x, n = t.n, per = (n + 255) / 256, lo = th * per < n ? th * per : n, hi = lo + per < n ? lo + per : n;
    auto len_of = [&](uint32_t g) -> uint64_t {
        const uint32_t i = t.perm[g];
        const uint64_t len = src_off[i + 1] - src_off[i];
        return len < t.len_cap[g] ? len : t.len_cap[g];
    };
    uint64_t sum = 0;
    for (uint32_t g = lo; g < hi; g++) sum += len_of(g);
    part[th] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < 256; s <<= 1) {            // inclusive scan of the 256 segment sums
        const uint64_t v = th >= s ? part[th - s] : 0;
        __syncthreads();
        part[th] += v;
        __syncthreads();
    }
    uint64_t run = th ? part[th - 1] : 0;
    if (th == 0) dst_off[0] = 0;
    for (uint32_t g = lo; g < hi; g++) {
        run += len_of(g);
        dst_off[g + 1] = run;
    }
}

// len bytes src -> dst by the 64 lanes of one wave
__device__ __forceinline__ void mixed_wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t len, uint32_t lane) {
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (((a ^ b) & 15u) == 0) {
        uint64_t head = (16u - (b & 15u)) & 15u;
        if (head > len) head = len;
        if (lane < head) dst[lane] = src[lane];
        const uint64_t body = (len - head) >> 4;
        const uint4 *s4 = (const uint4 *)(src + head);
        uint4 *d4 = (uint4 *)(dst + head);
        for (uint64_t k = lane; k < body; k += 64) d4[k] = s4[k];
        const uint64_t done = head + (body << 4);
        if (done + lane < len) dst[done + lane] = src[done + lane];        // (a tail of at most 15 bytes)
    } else if (((a ^ b) & 3u) == 0) {
        uint64_t head = (4u - (b & 3u)) & 3u;
        if (head > len) head = len;
        if (lane < head) dst[lane] = src[lane];
        const uint64_t body = (len - head) >> 2;
        const uint32_t *s1 = (const uint32_t *)(src + head);
        uint32_t *d1 = (uint32_t *)(dst + head);
        for (uint64_t k = lane; k < body; k += 64) d1[k] = s1[k];
        const uint64_t done = head + (body << 2);
        if (done + lane < len) dst[done + lane] = src[done + lane];
    } else {
        for (uint64_t k = lane; k < len; k += 64) dst[k] = src[k];
    }
}

// wave g (four to a block) copies grouped record g: proof perm[g] -> dst_proofs + dst_off[g] (dst_off[g + 1] - dst_off[g] bytes),
// its public inputs and its committed instance
extern "C" __global__ void __launch_bounds__(256)
k_mixed_gather(H2vMixedTab t, const uint8_t *__restrict__ src_proofs, const uint64_t *__restrict__ src_off, const uint8_t *__restrict__ src_inst,
               const uint8_t *__restrict__ src_ci, uint8_t *__restrict__ dst_proofs, const uint64_t *__restrict__ dst_off,
               uint8_t *__restrict__ dst_inst, uint8_t *__restrict__ dst_ci) {
    const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= t.n) return;
    const uint32_t i = t.perm[g];
    mixed_wave_copy(dst_proofs + dst_off[g], src_proofs + src_off[i], dst_off[g + 1] - dst_off[g], lane);
    if (t.inst_len[g]) mixed_wave_copy(dst_inst + t.inst_dst[g], src_inst + t.inst_src[g], t.inst_len[g], lane);
    if (t.ci_src[g] != 0xffffffffu) mixed_wave_copy(dst_ci + (size_t)t.ci_dst[g] * 48, src_ci + (size_t)t.ci_src[g] * 48, 48, lane);
}

// Proof i of a per-plan sub-batch: status folds valid / valid_sub into H2V_ST_BAD_POINT exactly as the pairing kernels,
// k_prepare_export and k_fold_pairs_affine fold it; L = the plan's pi point, or the folded el' of a recursive plan, R = er (or
// er').  Written at pos[i], the proof's position in the call: the two-slot affine record (infinity, all zero, for a proof whose
// status is not 0: it takes no part in anything after), good and the status word.  One lane per proof.
extern "C" __global__ void __launch_bounds__(64)
k_mixed_pairs(H2vDevPlan plan, uint32_t n, const uint32_t *__restrict__ pts, const uint8_t *__restrict__ valid, const uint8_t *__restrict__ valid_sub,
              const uint32_t *__restrict__ er_jac, const uint32_t *__restrict__ el_jac /* folded el (recursion) or NULL */,
              const uint32_t *__restrict__ status, const uint32_t *__restrict__ pos, uint32_t *__restrict__ pool /* call x 2 x 24 */,
              uint8_t *__restrict__ good, uint32_t *__restrict__ status_out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slots = H2V_SLOTS(plan);
    uint32_t st = status[i];
    for (uint32_t j = 0; j < slots; j++)
        if (!valid[(size_t)i * slots + j] || (valid_sub && !valid_sub[(size_t)i * slots + j])) st |= H2V_ST_BAD_POINT;
    G1J j[2];
    g1j_set_inf(j[0]); g1j_set_inf(j[1]);
    if (st == 0) {
        if (el_jac) {
#pragma unroll
            for (int k = 0; k < 12; k++) { j[0].x.v[k] = el_jac[(size_t)i * 36 + k]; j[0].y.v[k] = el_jac[(size_t)i * 36 + 12 + k]; j[0].z.v[k] = el_jac[(size_t)i * 36 + 24 + k]; }
        } else {
            G1A l;
            const uint32_t *pp = pts + ((size_t)i * slots + plan.pi_point) * 24;
#pragma unroll
            for (int k = 0; k < 12; k++) { l.x.v[k] = pp[k]; l.y.v[k] = pp[12 + k]; }
            g1j_from_affine(j[0], l);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) { j[1].x.v[k] = er_jac[(size_t)i * 36 + k]; j[1].y.v[k] = er_jac[(size_t)i * 36 + 12 + k]; j[1].z.v[k] = er_jac[(size_t)i * 36 + 24 + k]; }
    }
    G1A a[2];
    g1j_to_affine_batch<2>(a, j);
    const uint32_t at = pos[i];
    uint32_t *o = pool + (size_t)at * 48;
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < 12; k++) { o[24 * q + k] = a[q].x.v[k]; o[24 * q + 12 + k] = a[q].y.v[k]; }
    good[at] = st == 0 ? 1 : 0;
    status_out[at] = st;
}
