// h2v_check_pairs_multi(_device): one batch check over pairs on several SRS (include/h2v.h).  Part of h2v_capi.hip, which includes
// this file behind h2v_check_pairs_rlc - it uses that file's statics (Unit, RlcWs, PipWs, pip_bind, launch_decompress,
// launch_pairing, the records, the host forms' result block) and is no translation unit of its own.
#pragma once

// ---- h2v_check_pairs_multi(_device): ONE batch check over pairs on SEVERAL SRS -------------------------------------------------
// The pairs come in ranges, range k against the s_g2 of plans[k].  With coefficients r_i drawn by position in the CALL,
//     prod_k e( sum_{i in k} r_i L_i , s_g2_k )  ==  e( sum_i r_i R_i , G2 )
// holds exactly when every pair passes its own equation, except with probability <= 2^-128 over the seed: C + 1 Miller loops and
// one final exponentiation (k_pairing_rlc_multi).  What is enqueued, all on `st`: ONE decoding launch over the n pairs, ONE
// k_rlc_pairs_prepare, the six bucket-MSM launches with C + 1 problems - R over all pairs, L_k over range k's slice of the one
// scalar array and of l_idx (views: ranges are contiguous) -, the pairing, and behind its skip flags the per-pair kernels of
// h2v_check_pairs on each range's slice through a pair view of that range's plan.  No 64-pair group stage: groups would straddle
// ranges.  The call is one piece whatever the workspace: its buffers are a set of their own (MultiWs; a laned workspace owns no
// kernel buffers and a lane's are a chunk's), and on a laned workspace it runs on the caller's stream behind a join of the lanes,
// its record one "chunk" on a lane, as the fold tail of a mixed call.  Ranges without pairs take no problem and no Miller loop.
// What "C + 1 bucket problems, then k_pairing_rlc_multi" needs of the set it runs on - h2v_check_pairs_multi's (MultiWs) or the one
// of the mixed calls across several SRS (AcrossWs): the (1 + MULTI_MAX) sums, the argument ring (device arrays, pinned copies, the
// events behind the calls that took a slot) and the bucket-MSM sets of the classes behind the first (Lx[0] stays empty).
struct MultiCore {
    uint32_t *sums;
    PipArgs *args_d;
    PipWs *Lx;
    void **h_args;
    hipEvent_t *ev;
    bool *used;
    uint64_t *next;
};
struct MultiWs {
    Owner mem;                  // of the set's own blocks and events; r and the ranges' bucket-MSM sets own theirs
    uint64_t cap = 0;
    uint32_t *pts = nullptr, *dec_ctr = nullptr, *status = nullptr, *er = nullptr, *pair_pts = nullptr, *sums = nullptr;
    uint8_t *valid = nullptr, *valid_sub = nullptr;
    uint64_t *pair_off = nullptr;
    PipArgs *args_d = nullptr;  // MULTI_ARG_SLOTS argument arrays of MULTI_MAX + 1 problems
    RlcWs *r = nullptr;         // the pairs shape: r_scal, r_idx, l_idx, good, flags; R's bucket-MSM set, and range 0's (L)
    PipWs Lx[wslayout::MULTI_MAX];     // the further ranges' sets ([0] stays empty)
    // a call takes the next argument slot: its pinned copy is rewritten, and its device copy overwritten, only when the call that
    // took the slot last has finished on the device (ev: recorded behind everything that call enqueued)
    void *h_args[wslayout::MULTI_ARG_SLOTS] = {};
    hipEvent_t ev[wslayout::MULTI_ARG_SLOTS] = {};
    bool used[wslayout::MULTI_ARG_SLOTS] = {};
    uint64_t next = 0;
    MultiCore core() { return {sums, args_d, Lx, h_args, ev, used, &next}; }
};
static_assert(wslayout::MULTI_MAX == H2V_MULTI_SRS_MAX && wslayout::MULTI_MAX == COOP_MULTI_MAX, "one limit: header, size table, kernel");
static int multi_quiesce(const MultiCore &m) {
    for (uint32_t q = 0; q < wslayout::MULTI_ARG_SLOTS; q++)
        if (m.used[q] && hipEventSynchronize(m.ev[q]) != hipSuccess) return fail(H2V_E_DEVICE, "waiting for an earlier multi-SRS check failed");
    return H2V_OK;
}
static int multi_quiesce(MultiWs *m) { return multi_quiesce(m->core()); }
// THE SUMS AND THE CHECK of a call across several SRS, all on `st`: np = C + 1 bucket problems side by side in the six `_many`
// launches - prob[0] is R, prob[1 + k] the left-hand sum of class k, whose line table is cls_plan[k]'s - into m.sums, and ONE
// k_pairing_rlc_multi over them, whose epilogue writes the skip flags (r->flags), counts a failed check in fail_ctr and, passed,
// copies good[0 .. n) to accept[].  Problem 0 runs on r->R, problem 1 on r->L, the further ones on m.Lx (sized by the caller).  The
// call takes the next slot of the argument ring: *slot_out, whose event the CALLER records behind everything it enqueues.  Events
// of the record: [5] .. [8] the bucket MSMs, [8]/[9] around the pairing; the record keeps R's shape.
static int multi_sums_check(const MultiCore &m, RlcWs *r, const SumTerms *prob, uint32_t np, const h2v_plan *const *cls_plan, uint32_t n, const uint8_t *good,
                            uint8_t *accept, uint32_t *fail_ctr, CallRec &rec, hipStream_t st, uint32_t *slot_out) {
    hipEvent_t *ev = rec.ev;
    const uint32_t C = np - 1;
    if (C < 1 || C > wslayout::MULTI_MAX) return fail(H2V_E_DEVICE, "internal: a multi-SRS check of no class or of too many");
    PipArgs pa[wslayout::MULTI_MAX + 1] = {};
    uint32_t max_n = 0, max_W = 0, max_NB = 0, max_acc_blocks = 0;
    for (uint32_t q = 0; q < np; q++) {
        PipArgs &a = pa[q];
        a.n = prob[q].n; a.halves = prob[q].halves;
        a.scal = prob[q].scal; a.pidx = prob[q].pidx;
        a.pool0 = prob[q].pool0; a.n_pool0 = prob[q].n_pool0; a.pool1 = prob[q].pool1; a.out = m.sums + 36 * q;
        const PipWs &pw = q == 0 ? r->R : q == 1 ? r->L : m.Lx[q - 1];
        if (a.n > pw.cap_n || a.halves > pw.cap_halves) return fail(H2V_E_DEVICE, "internal: bucket MSM workspace too small");
        pip_bind(pw, a);
        const uint64_t lanes = 2ull * a.n * a.halves * a.W / a.chain + (uint64_t)a.W * a.NB + 256ull * PIP_N_CLASSES;     // (as pip_launch)
        const uint32_t blocks = (uint32_t)((lanes + 255) / 256);
        max_n = a.n > max_n ? a.n : max_n; max_W = a.W > max_W ? a.W : max_W; max_NB = a.NB > max_NB ? a.NB : max_NB;
        max_acc_blocks = blocks > max_acc_blocks ? blocks : max_acc_blocks;
    }
    const uint32_t slot = (uint32_t)((*m.next)++ % wslayout::MULTI_ARG_SLOTS);
    if (m.used[slot]) HIPCHK(hipEventSynchronize(m.ev[slot]));
    m.used[slot] = true;
    *slot_out = slot;
    PipArgs *args_d = m.args_d + (size_t)slot * (wslayout::MULTI_MAX + 1);
    memcpy(m.h_args[slot], pa, np * sizeof(PipArgs));
    HIPCHK(hipMemcpyAsync(args_d, m.h_args[slot], np * sizeof(PipArgs), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ev[5], st));
    for (uint32_t q = 0; q < np; q++) HIPCHK(hipMemsetAsync(pa[q].cnt, 0, (size_t)pa[q].W * pa[q].NB * 4, st));
    const uint32_t *no_skip = nullptr;
    hipLaunchKernelGGL(k_pip_digits_many, dim3((max_n + 255) / 256, np), dim3(256), 0, st, (const PipArgs *)args_d, no_skip);
    hipLaunchKernelGGL(k_pip_scan_many, dim3(1, np), dim3(1024), 0, st, (const PipArgs *)args_d, no_skip);
    hipLaunchKernelGGL(k_pip_scatter_many, dim3((max_n + 255) / 256, np), dim3(256), 0, st, (const PipArgs *)args_d, no_skip);
    HIPCHK(hipEventRecord(ev[6], st));
    hipLaunchKernelGGL(k_pip_accumulate_many, dim3(max_acc_blocks, np), dim3(256), 0, st, (const PipArgs *)args_d, no_skip);
    HIPCHK(hipEventRecord(ev[7], st));
    const size_t lds = (size_t)43 * max_NB * 4;
    HIPCHK(hipFuncSetAttribute((const void *)k_pip_reduce_many, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_pip_reduce_many, dim3(max_W, np), dim3(max_NB), lds, st, (const PipArgs *)args_d, no_skip);
    hipLaunchKernelGGL(k_pip_combine_many, dim3(1, np), dim3(64), 0, st, (const PipArgs *)args_d, no_skip);
    HIPCHK(hipEventRecord(ev[8], st));
    HIPCHK(hipGetLastError());
    rec.rlc_c = pa[0].c; rec.rlc_W = pa[0].W; rec.rlc_chain = pa[0].chain; rec.rlc_terms = pa[0].n;
    // ---- the check
    CoopMultiLines tabs = {};
    tabs.n = C;
    for (uint32_t j = 0; j < C; j++) tabs.sg2[j] = cls_plan[j]->d.lines28_sg2;
    hipLaunchKernelGGL(k_pairing_rlc_multi, dim3(1), dim3(64), COOP_LDS_BYTES(1), st, tabs, cls_plan[0]->d.lines28_g2, (const uint32_t *)m.sums, n, good, accept,
                       r->flags, (n + 63) / 64, fail_ctr);
    HIPCHK(hipEventRecord(ev[9], st));
    return H2V_OK;
}
static void multi_release(h2v_workspace *w) {
    MultiWs *m = w->multi;
    if (!m) return;
    (void)multi_quiesce(m);
    if (m->r) rlc_release(m->r);
    for (PipWs &q : m->Lx) pip_free(q);
    m->mem.release();
    delete m;
    w->multi = nullptr;
}
static int multi_ensure(h2v_workspace *w) {
    if (w->multi) return H2V_OK;
    MultiWs *m = new MultiWs();
    w->multi = m;
    m->cap = w->cap;
    const auto T = wslayout::multi_srs(w->cap);
    bool ok = m->mem.alloc(m->pts, T.row[wslayout::X_PTS]) && m->mem.alloc(m->valid, T.row[wslayout::X_VALID]) && m->mem.alloc(m->valid_sub, T.row[wslayout::X_VALID_SUB]) &&
              m->mem.alloc(m->dec_ctr, T.row[wslayout::X_DEC_CTR]) && m->mem.alloc(m->status, T.row[wslayout::X_STATUS]) && m->mem.alloc(m->er, T.row[wslayout::X_ER]) &&
              m->mem.alloc(m->pair_pts, T.row[wslayout::X_PAIR_PTS]) && m->mem.alloc(m->pair_off, T.row[wslayout::X_PAIR_OFF]) && m->mem.alloc(m->sums, T.row[wslayout::X_SUMS]) &&
              m->mem.alloc(m->args_d, T.row[wslayout::X_ARGS]);
    for (uint32_t q = 0; ok && q < wslayout::MULTI_ARG_SLOTS; q++)
        ok = m->mem.alloc_pinned(m->h_args[q], wslayout::multi_args_bytes()) && m->mem.event(m->ev[q], hipEventDisableTiming);
    if (ok) {
        std::vector<uint64_t> off(w->cap + 1);
        for (uint64_t i = 0; i <= w->cap; i++) off[i] = 96 * i;
        const uint32_t slot_off[2] = {0, 48};
        ok = hipMemcpy(m->pair_pts, slot_off, 8, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(m->pair_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) ok = (m->r = rlc_new(w->cap, 1, 0, wslayout::rlc_pairs(w->cap))) != nullptr;
    if (!ok) { multi_release(w); return fail(H2V_E_DEVICE, "allocation of the multi-SRS check's buffers failed"); }
    return H2V_OK;
}
struct MultiRange { const h2v_plan *p; uint32_t lo, n; };     // a range WITH pairs: its plan, its first pair, its count
// u: p = the first range's plan, n, pairs, accept, status (device pointers), seed.  ws: the workspace of the call.
static int run_pairs_multi(const std::vector<MultiRange> &rg, const Unit &u, h2v_workspace *ws, hipStream_t st) {
    const uint32_t n = u.n, C = (uint32_t)rg.size(), np = C + 1;
    int rc;
    if ((rc = rlc_stats_ensure(ws)) || (rc = multi_ensure(ws))) return rc;
    MultiWs *m = ws->multi;
    RlcWs *r = m->r;
    // ---- the record: the workspace's own, or - laned - one "chunk" on a lane behind a join of the lanes
    h2v_workspace *rw = ws;
    uint32_t *fail_ctr = nullptr;
    if (ws->n_lanes) {
        if ((rc = lanes_join(ws, st))) return rc;
        CallRec &parent = rec_laned(ws, h2v_workspace::RLC, ws->n_lanes, n, n);
        fail_ctr = rec_word(ws, parent);
        const uint32_t l = (uint32_t)(ws->next_lane++ % ws->n_lanes);
        if ((rc = ensure_lane(ws, l))) return rc;
        rw = ws->lane[l];
    }
    LaunchOptsScope opts(rw);
    CallRec &rec = rec_new(rw, h2v_workspace::RLC);
    rec.no_vm = true;
    if (!fail_ctr) fail_ctr = rec_word(ws, rec);
    hipEvent_t *ev = rec.ev;
    HIPCHK(hipMemsetAsync(fail_ctr, 0, 4, st));
    // ---- the further ranges' bucket-MSM sets, grown behind everything that may still use them
    for (uint32_t j = 1; j < C; j++) {
        if (m->Lx[j].cap_n >= rg[j].n) continue;
        HIPCHK(hipStreamSynchronize(st));
        if ((rc = multi_quiesce(m))) return rc;
        pip_free(m->Lx[j]);
        if ((rc = pip_alloc(m->Lx[j], wslayout::multi_range_cap(rg[j].n), 1))) return rc;
    }
    // ---- decoding: one launch over the whole call, through a two-slot view (the view reads nothing of the plan but its shape)
    H2vDevPlan v = rg[0].p->d;
    v.proof_len = 96; v.n_points = 2; v.n_ci = 0; v.n_pi = 0; v.ivc = 0; v.pi_point = 0; v.points = m->pair_pts;
    for (int q : {0, 2, 3}) HIPCHK(hipEventRecord(ev[q], st));
    HIPCHK(hipMemsetAsync(m->status, 0, (size_t)n * 4, st));
    if ((rc = launch_decompress(v, n, u.pairs, m->pair_off, nullptr, nullptr, DecBufs{m->pts, m->valid, m->valid_sub, m->dec_ctr}, nullptr, st))) return rc;
    HIPCHK(hipEventRecord(ev[1], st));
    // ---- the coefficients, by position in the call
    HIPCHK(hipEventRecord(ev[10], st));
    RlcPairArgs ra = {n, m->status, m->valid, m->valid_sub, nullptr, {}, r->r_scal, r->l_idx, r->r_idx, r->good, nullptr, 0};
    copy_seed(ra.seed, u.seed);
    hipLaunchKernelGGL(k_rlc_pairs_prepare, dim3((n + 63) / 64), dim3(64), 0, st, ra);
    HIPCHK(hipEventRecord(ev[4], st));
    // ---- the sums and the check: problem 0 is R over all pairs, problem 1 + j is L of range j - views of the one scalar array
    // and of l_idx (ranges are contiguous)
    SumTerms prob[wslayout::MULTI_MAX + 1];
    const h2v_plan *cls_plan[wslayout::MULTI_MAX];
    prob[0] = {n, 1, r->r_scal, r->r_idx, m->pts, 2 * n, nullptr};
    for (uint32_t j = 0; j < C; j++) {
        prob[1 + j] = {rg[j].n, 1, r->r_scal + (size_t)rg[j].lo * 8, r->l_idx + rg[j].lo, m->pts, 2 * n, nullptr};
        cls_plan[j] = rg[j].p;
    }
    uint32_t slot = 0;
    if ((rc = multi_sums_check(m->core(), r, prob, np, cls_plan, n, r->good, u.accept, fail_ctr, rec, st, &slot))) return rc;
    // ---- the fall-back, skipped on the device when the check passed: h2v_check_pairs's two kernels, range by range
    for (uint32_t j = 0; j < C; j++) {
        const uint32_t lo = rg[j].lo, nj = rg[j].n;
        H2vDevPlan vj = rg[j].p->d;
        vj.proof_len = 96; vj.n_points = 2; vj.n_ci = 0; vj.n_pi = 0; vj.ivc = 0; vj.pi_point = 0; vj.points = m->pair_pts;
        const uint32_t *ptsj = m->pts + (size_t)lo * 48;
        uint32_t *erj = m->er + (size_t)lo * 36;
        hipLaunchKernelGGL(k_pairs_to_jac, dim3((nj + 63) / 64), dim3(64), 0, st, nj, ptsj, erj, (const uint32_t *)r->flags);
        launch_pairing(vj, nj, ptsj, m->valid + (size_t)lo * 2, m->valid_sub + (size_t)lo * 2, erj, nullptr, m->status + lo, u.accept + lo, nullptr, st, rw->in_flight_hint, r->flags);
    }
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, m->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(m->ev[slot], st));
    return H2V_OK;
}
// The argument rules, in the order the header lists them; everything here is decided on the host before a device is touched.
// n_out: the pairs of the call; rg (optional): the ranges with pairs.
static int multi_args(const h2v_plan *const *plans, uint32_t n_plans, const uint64_t *counts, const uint8_t *pairs, const uint8_t *accept, const h2v_rlc_opts *opts,
                      uint64_t *n_out, std::vector<MultiRange> *rg) {
    *n_out = 0;
    if (!plans || n_plans == 0) return fail(H2V_E_ARG, "a multi-SRS check needs at least one plan");
    if (n_plans > H2V_MULTI_SRS_MAX) return fail(H2V_E_LIMIT, "a multi-SRS check takes at most " + std::to_string(H2V_MULTI_SRS_MAX) + " ranges");
    if (opts && (opts->flags & (H2V_RLC_SEED_TRANSCRIPT | H2V_RLC_SEED_KEYED)))
        return fail(H2V_E_ARG, "a multi-SRS check takes no derived seed (H2V_RLC_SEED_TRANSCRIPT / H2V_RLC_SEED_KEYED): a rule that binds each range's key is not defined");
    if (opts && (opts->flags & (H2V_RLC_FOLD_PAIRS | H2V_RLC_GROUPED))) return fail(H2V_E_ARG, "H2V_RLC_FOLD_PAIRS / H2V_RLC_GROUPED mean nothing in a multi-SRS check");
    if (opts && (opts->flags & ~(H2V_RLC_SEED_GIVEN | H2V_RLC_ONE_STREAM))) return fail(H2V_E_ARG, "unknown flag in h2v_rlc_opts");
    if (!counts) return fail(H2V_E_ARG, "null argument: counts");
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_plans; k++) {
        if (!plans[k]) return fail(H2V_E_ARG, "null argument: plans[" + std::to_string(k) + "]");
        if (plans[k]->device != plans[0]->device) return fail(H2V_E_ARG, "the plans of a multi-SRS check are on different devices");
        if (counts[k] > (1ull << 22) || (n += counts[k]) > (1ull << 22)) return fail(H2V_E_LIMIT, "RLC batches are limited to 2^22 pairs");
        if (rg && counts[k]) rg->push_back({plans[k], (uint32_t)(n - counts[k]), (uint32_t)counts[k]});
    }
    if (!pairs) return fail(H2V_E_ARG, "null argument: pairs");
    if (!accept) return fail(H2V_E_ARG, "null argument: accept");
    *n_out = n;
    return H2V_OK;
}
// what both forms check of the workspace, and the call's unit
static int multi_common(const std::vector<MultiRange> &rg, uint64_t n, h2v_workspace *&ws, const void *stream, bool device_form, TmpWs &tmp) {
    for (const MultiRange &q : rg) ALIVE(q.p);
    // (the workspace rules of h2v_check_pairs for plans[0] - here: the first plan with pairs, whose shape the decoding view takes)
    return pairs_common(rg[0].p, n, ws, stream, device_form, tmp);
}
extern "C" int h2v_check_pairs_multi_device(const h2v_plan *const *plans, uint32_t n_plans, const uint64_t *counts, const uint8_t *pairs, uint8_t *accept,
                                            uint32_t *status, h2v_workspace *ws, void *stream, const h2v_rlc_opts *opts) {
    uint64_t n;
    std::vector<MultiRange> rg;
    if (int rc = multi_args(plans, n_plans, counts, pairs, accept, opts, &n, &rg)) return rc;
    if (n == 0) return H2V_OK;
    if (!ws) return fail(H2V_E_ARG, "the RLC entry points need a workspace (results of the batch check live in it)");
    TmpWs none;
    if (int rc = multi_common(rg, n, ws, stream, true, none)) return rc;
    Unit u = unit_of_pairs(UnitKind::PAIR_RLC, rg[0].p, n, pairs, accept, status);
    if (int rc = rlc_seed(opts, u.seed)) return rc;
    return run_pairs_multi(rg, u, ws, (hipStream_t)stream);
}
extern "C" int h2v_check_pairs_multi(const h2v_plan *const *plans, uint32_t n_plans, const uint64_t *counts, const uint8_t *pairs, uint8_t *accept, uint32_t *status,
                                     h2v_workspace *ws, const h2v_rlc_opts *opts, int *fell_back) {
    uint64_t n;
    std::vector<MultiRange> rg;
    if (int rc = multi_args(plans, n_plans, counts, pairs, accept, opts, &n, &rg)) return rc;
    if (fell_back) *fell_back = 0;
    if (n == 0) return H2V_OK;
    TmpWs tmp;
    if (int rc = multi_common(rg, n, ws, nullptr, false, tmp)) return rc;
    Unit u = unit_of_pairs(UnitKind::PAIR_RLC, rg[0].p, n, nullptr, nullptr, nullptr);
    int rc = rlc_seed(opts, u.seed);
    hostcall::ResultBlock R;
    if (rc == H2V_OK) rc = result_ensure(ws, hostcall::Call::CHECK, n, &R);
    if (rc) return rc;
    uint8_t *const d = ws->res.p;
    u.pairs = d + R.pairs.off; u.accept = d + R.accept.off; u.status = (uint32_t *)(d + R.status.off);
    if (hipMemcpyAsync(d + R.pairs.off, pairs, R.pairs.bytes, hipMemcpyHostToDevice, ws->hs) != hipSuccess) rc = fail(H2V_E_DEVICE, "upload of the pairs failed");
    if (rc == H2V_OK) rc = run_pairs_multi(rg, u, ws, ws->hs);
    return host_call_tail(ws, rc, {{accept, R.accept, "accept[]"}, {status, R.status, "the status words"}}, true, fell_back, "multi-SRS pair check");
}
