// The body of k_mixed_terms and k_mixed_terms_grouped: block MT_BLK (64 proofs) of the sub-batch `a` - MixedTermsArgs itself, or the
// view the grouped kernel makes of its block's group (h2v_mixed_group_dev.hpp); MT_SEED: the kernel's argument struct, which
// holds the call's seed (mixed_coeff reads it there at a run-time index, or through its seed_dev).  Included into both kernels' bodies, so that the per-plan
// kernel is compiled from the very text it always had; the includer defines MT_BLK and MT_SEED and declares sbuf.
    const int lane = threadIdx.x;
    const uint32_t i = MT_BLK * 64 + lane;
    const bool live = i < a.n;
    const uint32_t ii = live ? i : a.n - 1;
    const uint32_t at = a.pos[ii];
    uint32_t st = a.status[ii];
    for (uint32_t j = 0; j < a.slots; j++)
        if (!a.valid[(size_t)ii * a.slots + j] || (a.valid_sub && !a.valid_sub[(size_t)ii * a.slots + j])) st |= H2V_ST_BAD_POINT;
    const bool good = live && st == 0;
    uint32_t rw[4];
    mixed_coeff(rw, MT_SEED, at, good, sbuf, lane);
    Fr r, rm;
#pragma unroll
    for (int l = 0; l < 8; l++) r.v[l] = l < 4 ? rw[l] : 0u;
    fr_to_mont(rm, r);
    const uint32_t *pp = a.pts + (size_t)ii * a.slots * 24;
    if (live) {
        a.status_out[at] = st;
        a.good[at] = good ? 1 : 0;
#pragma unroll
        for (int l = 0; l < 8; l++) a.l_scal[(size_t)at * 8 + l] = r.v[l];
        mixed_copy_point(a.l_pts + (size_t)at * 24, pp + (size_t)a.pi_point * 24, good);
    }
    const uint32_t *sp = a.scalars + (size_t)ii * a.scal_stride * 8;
#pragma unroll 1
    for (uint32_t t = 0; t < a.n_var; t++) {
        Fr s, sm, p, pc;
#pragma unroll
        for (int l = 0; l < 8; l++) s.v[l] = sp[t * 8 + l];
        fr_to_mont(sm, s);
        fr_mul(p, sm, rm);
        fr_from_mont(pc, p);
        if (live) {
            const size_t e = (size_t)i * a.n_var + t;
#pragma unroll
            for (int l = 0; l < 8; l++) a.r_scal[e * 8 + l] = pc.v[l];
            mixed_copy_point(a.r_pts + e * 24, pp + (size_t)a.terms[2 * t + 1] * 24, good);
        }
    }
#pragma unroll 1
    for (uint32_t f = 0; f < a.n_fix; f++) {
        Fr s, sm, p;
#pragma unroll
        for (int l = 0; l < 8; l++) s.v[l] = sp[(a.n_var + f) * 8 + l];
        fr_to_mont(sm, s);
        fr_mul(p, sm, rm);               // 0 for lanes that take no part (rm = 0)
#pragma unroll 1
        for (int d = 32; d >= 1; d >>= 1) {
            Fr o;
#pragma unroll
            for (int l = 0; l < 8; l++) o.v[l] = __shfl_down(p.v[l], d);
            fr_add(p, p, o);
        }
        if (lane == 0) {
#pragma unroll
            for (int l = 0; l < 8; l++) a.vk_part[((size_t)MT_BLK * a.n_fix + f) * 8 + l] = p.v[l];
        }
    }
