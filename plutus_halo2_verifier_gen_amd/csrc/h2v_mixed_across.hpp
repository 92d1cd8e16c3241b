// Mixed-key calls across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS), the host side of the call's end.  Part of h2v_capi.hip,
// which includes this file behind the tails of the one-SRS forms - it uses that file's statics (Unit, MixedWs, MixedFold, RlcWs,
// PipWs, the records, launch_pairing, pair_view) and h2v_multi_srs.hpp's multi_sums_check, and is no translation unit of its own.
// The kernels are in h2v_mixed_srs_dev.hpp, the SRS classes in h2v_mixed_srs.hpp (host only).
#pragma once

// H2V_MIXED_ACROSS_SRS: the set of the call's ONE multi-pairing (h2v_ws_layout.hpp: across_srs), owned by the mixed-call staging.
// The fold form takes R's and the first class's bucket-MSM sets, good and the flags from the term pool (m->fold); the pairs form
// has an RLC set of the pairs shape of its own (r), allocated by its first call.
struct AcrossWs {
    Owner mem;                  // of the set's own blocks and events; r and the classes' bucket-MSM sets own theirs
    uint32_t *sums = nullptr, *cl_scal = nullptr, *cl_idx = nullptr, *pool_g = nullptr, *status_g = nullptr, *er = nullptr;
    uint8_t *accept_g = nullptr;
    PipArgs *args_d = nullptr;  // MULTI_ARG_SLOTS argument arrays of MULTI_MAX + 1 problems
    RlcWs *r = nullptr;
    PipWs Lx[wslayout::MULTI_MAX];     // the further classes' sets ([0] stays empty)
    void *h_args[wslayout::MULTI_ARG_SLOTS] = {};
    hipEvent_t ev[wslayout::MULTI_ARG_SLOTS] = {};
    bool used[wslayout::MULTI_ARG_SLOTS] = {};
    uint64_t next = 0;
    uint32_t fold_classes = 0;  // sums holds R and this many L_k of a fold call (h2v_probe_mixed_fold_sums_multi); 0: none ran
    MultiCore core() { return {sums, args_d, Lx, h_args, ev, used, &next}; }
};
static void across_release(MixedWs *m) {
    AcrossWs *x = m->across;
    if (!x) return;
    (void)multi_quiesce(x->core());
    if (x->r) rlc_release(x->r);
    for (PipWs &q : x->Lx) pip_free(q);
    x->mem.release();
    delete x;
    m->across = nullptr;
}
static void across_fold_reset(MixedWs *m) { if (m->across) m->across->fold_classes = 0; }
// before anything of the call is enqueued: the set itself, the pairs form's RLC set, and the further classes' bucket-MSM sets -
// grown once every earlier mixed call, and with them every user of the argument ring, has finished on the device
static int across_ensure(h2v_workspace *w, const h2vsrs::Classes &cl, bool pairs_form) {
    MixedWs *m = w->mixed;
    if (!m->across) {
        AcrossWs *x = new AcrossWs();
        m->across = x;
        const auto T = wslayout::across_srs(w->cap);
        bool ok = x->mem.alloc(x->sums, T.row[wslayout::A_SUMS]) && x->mem.alloc(x->args_d, T.row[wslayout::A_ARGS]) && x->mem.alloc(x->cl_scal, T.row[wslayout::A_CL_SCAL]) &&
                  x->mem.alloc(x->cl_idx, T.row[wslayout::A_CL_IDX]) && x->mem.alloc(x->pool_g, T.row[wslayout::A_POOL_G]) && x->mem.alloc(x->status_g, T.row[wslayout::A_STATUS_G]) &&
                  x->mem.alloc(x->accept_g, T.row[wslayout::A_ACCEPT_G]) && x->mem.alloc(x->er, T.row[wslayout::A_ER]);
        for (uint32_t q = 0; ok && q < wslayout::MULTI_ARG_SLOTS; q++)
            ok = x->mem.alloc_pinned(x->h_args[q], wslayout::multi_args_bytes()) && x->mem.event(x->ev[q], hipEventDisableTiming);
        if (!ok) { across_release(m); return fail(H2V_E_DEVICE, "allocation of the buffers of a mixed call across several SRS failed"); }
    }
    AcrossWs *x = m->across;
    if (pairs_form && !x->r && !(x->r = rlc_new(w->cap, 1, 0, wslayout::rlc_pairs(w->cap)))) return fail(H2V_E_DEVICE, "allocation of the buffers of a mixed call across several SRS failed");
    for (uint32_t j = 1; j < cl.n_used; j++) {
        if (x->Lx[j].cap_n >= cl.count[j]) continue;
        if (int rc = mixed_quiesce(m)) return rc;
        if (int rc = multi_quiesce(x->core())) return rc;
        pip_free(x->Lx[j]);
        if (int rc = pip_alloc(x->Lx[j], wslayout::multi_range_cap(cl.count[j]), 1)) return rc;
    }
    return H2V_OK;
}
// H2V_MIXED_ACROSS_SRS | H2V_MIXED_FOLD_MSM: what run_mixed_fold_tail enqueues in place of launch_sums and the one pairing, behind
// the terms of the call (its record's ev[4] is recorded here): the L-terms class-major (scalars and point indices; the points stay
// where they are), then R over the term pool (problem 0) and L_k over class k's slice (problem 1 + k) in the six `_many` launches,
// and ONE multi-pairing with the classes' line tables; no group stage, and after a failed check the HOST runs run_across_tail's
// form (run_mixed_call).  R and the first class's L are copied to where the one-SRS form leaves its two sums.
static int across_fold_sums(const Unit &u, h2v_workspace *w, CallRec &rec, hipStream_t st) {
    const MixedFold &f = *u.fold;
    const h2vmixed::FoldLayout &lay = *f.lay;
    const h2vsrs::Classes &cl = *f.cls;
    MixedWs *m = f.m;
    RlcWs *r = m->fold;
    AcrossWs *x = m->across;
    const uint32_t n = u.n;
    hipLaunchKernelGGL(k_across_lterms, dim3((n + 255) / 256), dim3(256), 0, st, n, f.d_cpos, (const uint32_t *)r->l_scal, x->cl_scal, x->cl_idx);
    HIPCHK(hipEventRecord(rec.ev[4], st));
    SumTerms prob[wslayout::MULTI_MAX + 1];
    const h2v_plan *cls_plan[wslayout::MULTI_MAX];
    prob[0] = {(uint32_t)lay.n_r, 2, r->r_scal, nullptr, m->fold_rpts, (uint32_t)lay.n_r, nullptr};
    for (uint32_t k = 0; k < cl.n_used; k++) {
        prob[1 + k] = {cl.count[k], 1, x->cl_scal + (size_t)cl.base[k] * 8, x->cl_idx + cl.base[k], m->fold_lpts, n, nullptr};
        cls_plan[k] = f.plans[cl.rep_plan[k]];
    }
    uint32_t *fail_ctr = u.fail_ctr;
    if (!fail_ctr) {
        fail_ctr = rec_word(w, rec);
        HIPCHK(hipMemsetAsync(fail_ctr, 0, 4, st));
    }
    uint32_t slot = 0;
    if (int rc = multi_sums_check(x->core(), r, prob, cl.n_used + 1, cls_plan, n, r->good, u.accept, fail_ctr, rec, st, &slot)) return rc;
    HIPCHK(hipMemcpyAsync(r->sums, x->sums, 2 * wslayout::JAC_BYTES, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(x->ev[slot], st));
    x->fold_classes = cl.n_used;
    m->fold_ran = true;
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, m->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}
// H2V_MIXED_ACROSS_SRS | H2V_MIXED_RLC, the tail over the call's pool of pairs (caller's order), ONE piece whatever the workspace:
// one coefficient launch over the class-major position list (r by P(i), the index arrays of the pairs at their call positions), R
// over all pairs (problem 0) and L_k over class k's slice of the one scalar array (problem 1 + k), ONE k_pairing_rlc_multi, and
// behind its skip flags the per-pair kernels of h2v_check_pairs per class - on the class's pairs gathered side by side, through a
// pair view of a plan of THAT class - with accept / status scattered back to the call positions.  Nothing comes back to the host in
// between.  w: the ordinary workspace, or the lane whose record the tail takes (its pair view is the only buffer of it in use).
// Events as run_pairs_rlc's (no decoding, no transcript).
static int run_across_tail(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const MixedFold &f = *u.fold;
    const h2vsrs::Classes &cl = *f.cls;
    MixedWs *m = f.m;
    AcrossWs *x = m->across;
    RlcWs *r = x->r;
    const uint32_t n = u.n, C = cl.n_used;
    LaunchOptsScope opts(w);
    int rc;
    if ((rc = pair_view_ensure(w))) return rc;
    if (!u.fail_ctr && (rc = rlc_stats_ensure(w))) return rc;
    CallRec &rec = rec_new(w, h2v_workspace::RLC);
    rec.no_vm = true;
    uint32_t *fail_ctr = u.fail_ctr;
    if (!fail_ctr) {
        fail_ctr = rec_word(w, rec);
        HIPCHK(hipMemsetAsync(fail_ctr, 0, 4, st));
    }
    for (int q : {0, 1, 2, 3, 10}) HIPCHK(hipEventRecord(rec.ev[q], st));
    AcrossCoeffArgs ca = {n, f.d_cpos, m->good, {}, r->r_scal, r->l_idx, r->r_idx, r->good, u.seed_dev};
    copy_seed(ca.seed, u.seed);
    hipLaunchKernelGGL(k_across_coeff, dim3((n + 63) / 64), dim3(64), 0, st, ca);
    HIPCHK(hipEventRecord(rec.ev[4], st));
    SumTerms prob[wslayout::MULTI_MAX + 1];
    const h2v_plan *cls_plan[wslayout::MULTI_MAX];
    prob[0] = {n, 1, r->r_scal, r->r_idx, m->pool, 2 * n, nullptr};
    for (uint32_t k = 0; k < C; k++) {
        prob[1 + k] = {cl.count[k], 1, r->r_scal + (size_t)cl.base[k] * 8, r->l_idx + cl.base[k], m->pool, 2 * n, nullptr};
        cls_plan[k] = f.plans[cl.rep_plan[k]];
    }
    uint32_t slot = 0;
    if ((rc = multi_sums_check(x->core(), r, prob, C + 1, cls_plan, n, r->good, u.accept, fail_ctr, rec, st, &slot))) return rc;
    // ---- the fall-back, skipped on the device when the check passed
    const uint32_t walk = (uint32_t)msm_n_simd();
    const uint32_t gather_blocks = (uint32_t)(((uint64_t)n * 12 + 255) / 256), scatter_blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_across_gather, dim3(gather_blocks < walk ? gather_blocks : walk), dim3(256), 0, st, n, f.d_cpos, (const uint32_t *)m->pool, (const uint32_t *)m->status,
                       (const uint32_t *)r->flags, x->pool_g, x->status_g);
    for (uint32_t k = 0; k < C; k++) {
        const uint32_t lo = cl.base[k], nk = cl.count[k];
        const H2vDevPlan vk = pair_view(cls_plan[k]->d, w);
        const uint32_t *ptsk = x->pool_g + (size_t)lo * 48;
        uint32_t *erk = x->er + (size_t)lo * 36;
        hipLaunchKernelGGL(k_pairs_to_jac, dim3((nk + 63) / 64), dim3(64), 0, st, nk, ptsk, erk, (const uint32_t *)r->flags);
        launch_pairing(vk, nk, ptsk, m->ones, nullptr, erk, nullptr, x->status_g + lo, x->accept_g + lo, nullptr, st, w->in_flight_hint, r->flags);
    }
    hipLaunchKernelGGL(k_across_scatter, dim3(scatter_blocks < walk ? scatter_blocks : walk), dim3(256), 0, st, n, f.d_cpos, (const uint8_t *)x->accept_g, (const uint32_t *)x->status_g,
                       (const uint32_t *)r->flags, u.accept, m->status);
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, m->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(x->ev[slot], st));
    return H2V_OK;
}
