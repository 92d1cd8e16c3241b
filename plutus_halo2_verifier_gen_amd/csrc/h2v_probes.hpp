// ---------------------------------------------------------------------------------------------- trace
extern "C" int h2v_trace(const h2v_plan *p, const uint8_t *proof, size_t proof_len, const uint8_t *instances,
                         const uint8_t *committed, uint8_t *scalars_out, uint8_t *msm_scalars_out, uint8_t el_out[96],
                         uint8_t er_out[96], uint32_t *status_out, uint8_t *accept_out) {
    if (!p || !proof) return fail(H2V_E_ARG, "null argument");
    ALIVE(p);
    HIPCHK(hipSetDevice(p->device));
    h2v_workspace *ws = nullptr;
    int rc = ws_create_for(wslayout::shape_of(p->d, true), p->device, 1, &ws);
    if (rc) return rc;
    uint64_t off[2] = {0, proof_len};
    h2v_batch b = {1, proof, off, instances, committed};
    uint8_t *d_pts96 = nullptr;
    h2v_batch in;
    rc = stage_batch(p, &b, ws, ws->hslot[0], &in);
    if (rc == H2V_OK) {
        Unit u = unit_of_batch(UnitKind::VERIFY, p, &in, ws->accept, nullptr);
        u.trace = true;
        rc = run_pipeline(u, ws, ws->hs);
    }
    if (rc == H2V_OK && hipStreamSynchronize(ws->hs) != hipSuccess) rc = fail(H2V_E_DEVICE, "trace pipeline failed");
    do {
        if (rc) break;
        if (hipMalloc((void **)&d_pts96, 192) != hipSuccess) { rc = fail(H2V_E_DEVICE, "hipMalloc failed"); break; }
        // el / er as they enter the pairing: after the accumulator fold when the plan is recursive
        if (p->d.ivc) hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, 1u, 1, ws->el2, d_pts96);
        else hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, 1u, 0, ws->pts + (size_t)p->d.pi_point * 24, d_pts96);
        hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, 1u, 1, p->d.ivc ? ws->er2 : ws->er, d_pts96 + 96);
        if (hipDeviceSynchronize() != hipSuccess) { rc = fail(H2V_E_DEVICE, "trace kernels failed"); break; }
        uint8_t both[192];
        if (hipMemcpy(both, d_pts96, 192, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
        if (el_out) memcpy(el_out, both, 96);
        if (er_out) memcpy(er_out, both + 96, 96);
        if (scalars_out && p->d.n_trace && hipMemcpy(scalars_out, ws->trace, (size_t)p->d.n_trace * 32, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
        if (msm_scalars_out && hipMemcpy(msm_scalars_out, ws->scalars, (size_t)p->d.n_terms * 32, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
        if (status_out && hipMemcpy(status_out, ws->status, 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
        if (accept_out && hipMemcpy(accept_out, ws->accept, 1, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
    } while (0);
    if (d_pts96) (void)hipFree(d_pts96);
    h2v_workspace_free(ws);
    return rc;
}

// ---------------------------------------------------------------------------------------------- probes
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc(&p, n ? n : 8) == hipSuccess ? 0 : -1; }
    int upload(const void *src, size_t n) { return alloc(n) || hipMemcpy(p, src, n, hipMemcpyHostToDevice) != hipSuccess ? -1 : 0; }      // allocate + copy
    int download(void *dst, size_t n) const { return hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
    template <class T> T *as() { return (T *)p; }
};
// What the library's owners (h2v_capi.hip: Owner) hold on `device` right now: out[0] device blocks, [1] device bytes, [2] pinned
// host blocks, [3] pinned bytes, [4] events.  Everything a plan or a workspace allocates is counted, the temporary blocks of the
// probes in this file and the pool streams are not.  Counts only: no device call, and valid after h2v_shutdown.  For tests
// (tests/test_workspace_memory_gpu.py holds the counts against the size tables of h2v_ws_layout.hpp); not in include/h2v.h.
extern "C" int h2v_probe_device_memory(int device, uint64_t out[5]) {
    if (device < 0 || device >= 16 || !out) return fail(H2V_E_ARG, "bad argument");
    for (int k = 0; k < 5; k++) out[k] = g_mem_live[device][k].load();
    return H2V_OK;
}
static int pick_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(H2V_E_DEVICE, "no HIP device: the HIP backend is required (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(H2V_E_ARG, "device index out of range");
    ALIVE_DEV(device);
    HIPCHK(hipSetDevice(device));
    return H2V_OK;
}
extern "C" int h2v_probe_field(int device, int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (op < 0 || op > 5 || !a || !b || !out || n == 0) return fail(H2V_E_ARG, "bad argument");
    const size_t bytes = (size_t)n * (op < 4 ? 48 : 32);
    DevBuf da, db, dout;
    if (da.upload(a, bytes) || db.upload(b, bytes) || dout.alloc(bytes)) return fail(H2V_E_DEVICE, "probe setup failed");
    hipLaunchKernelGGL(k_probe_field, dim3((n + 63) / 64), dim3(64), 0, nullptr, op, n, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out, bytes) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
extern "C" int h2v_probe_quad_madd(int device, const uint32_t *pq /* 48 dwords */, int neg, uint32_t *out /* 210 dwords */) {
    int rc = pick_device(device);
    if (rc) return rc;
    DevBuf din, dout;
    if (din.upload(pq, 48 * 4) || dout.alloc(210 * 4)) return fail(H2V_E_DEVICE, "probe setup failed");
    hipLaunchKernelGGL(k_probe_quad_madd, dim3(1), dim3(64), 0, nullptr, din.as<uint32_t>(), neg, dout.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out, 210 * 4) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
extern "C" int h2v_probe_f28_dot2(int device, int op, uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                                  uint32_t *out) {
    int rc = pick_device(device);
    if (rc) return rc;
    const int what = op & 15;
    const bool field = what <= 4, point = what >= 8 && what <= 10;
    if ((op & ~(15 | 16 | 64)) != 0 || !(field || point) || (what == 10 && (op & 16)) || n == 0 || !a || !out) return fail(H2V_E_ARG, "bad argument");
    if (field ? (!b || !c || !d) : (what != 8 && !b)) return fail(H2V_E_ARG, "bad argument");
    const size_t in_b = (size_t)n * (field ? 14 : 42) * 4, out_b = (size_t)n * (field ? 14 : 44) * 4;
    DevBuf da, db, dc, dd, dout;
    if (da.upload(a, in_b) || db.alloc(in_b) || dc.alloc(in_b) || dd.alloc(in_b) || dout.alloc(out_b)) return fail(H2V_E_DEVICE, "probe setup failed");
    if (field || what != 8) HIPCHK(hipMemcpy(db.p, b, in_b, hipMemcpyHostToDevice));
    if (field) {
        HIPCHK(hipMemcpy(dc.p, c, in_b, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dd.p, d, in_b, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_probe_f28_dot2, dim3((n + 63) / 64), dim3(64), 0, nullptr, op, n, da.as<uint32_t>(), db.as<uint32_t>(),
                       dc.as<uint32_t>(), dd.as<uint32_t>(), dout.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out, out_b) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
// ONE call of the six-lane pairing engine per group (k_probe_six in h2v_pairing_six.hpp has the ops and the buffer layouts), on raw
// 14-dword limb vectors, so that operands can sit ON the bounds the engine's headroom argument states.  a: n x 12 vectors, always;
// b: n x 12 (MUL; LINE1 / LINE2: vectors 0..7 are the T slots); pts: n x 4 and lines: 8 vectors [A0, A1, B0, B1] of loop 1, then of
// loop 2 (PROD2, ROUND); flags: n words (LINE1, LINE2, ROUND); csqr_n: the run length (CSQR, 1..64).  out: (n + GUARD) x 168 dwords and
// ok_out (INV; else optional): n + GUARD words, GUARD = one block's ten groups - both preset to 0xA5 bytes and copied back whole, so
// what a dead group of the last wave or a shadow lane wrote shows behind group n - 1.  For tests; not in include/h2v.h.
#define H2V_PROBE_SIX_GUARD SIX_GROUPS
extern "C" int h2v_probe_six_call(int device, int op, uint32_t n_groups, uint32_t csqr_n, const uint32_t *a, const uint32_t *b, const uint32_t *pts,
                                  const uint32_t *flags, const uint32_t *lines, uint32_t *out, uint32_t *ok_out) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (op < 0 || op >= SIX_PROBE_N_OPS) return fail(H2V_E_ARG, "unknown op");
    if (n_groups == 0 || n_groups > (1u << 16)) return fail(H2V_E_ARG, "n_groups out of range (1 .. 65536)");
    if (op == SIX_PROBE_CSQR && (csqr_n == 0 || csqr_n > 64)) return fail(H2V_E_ARG, "CSQR: the run length is 1 .. 64");
    const bool lines_op = op == SIX_PROBE_LINE1 || op == SIX_PROBE_LINE2, round_op = op == SIX_PROBE_PROD2 || op == SIX_PROBE_ROUND;
    if (!a || !out || ((op == SIX_PROBE_MUL || lines_op) && !b) || (round_op && (!pts || !lines)) || ((lines_op || op == SIX_PROBE_ROUND) && !flags) ||
        (op == SIX_PROBE_INV && !ok_out))
        return fail(H2V_E_ARG, "a buffer this op reads or writes is missing");
    const size_t n = n_groups, cap = n + H2V_PROBE_SIX_GUARD, vec = SIX_SLOT_DW * 4;
    uint32_t lines16[8 * 16] = {};
    if (lines)
        for (int s = 0; s < 8; s++) memcpy(lines16 + 16 * s, lines + SIX_SLOT_DW * s, vec);
    DevBuf da, db, dp, df, dl, dout, dok;
    if (da.upload(a, n * 12 * vec) || (b ? db.upload(b, n * 12 * vec) : db.alloc(8)) || (pts ? dp.upload(pts, n * 4 * vec) : dp.alloc(8)) ||
        (flags ? df.upload(flags, n * 4) : df.alloc(8)) || dl.upload(lines16, sizeof lines16) || dout.alloc(cap * SIX_PROBE_OUT_DW * 4) || dok.alloc(cap * 4))
        return fail(H2V_E_DEVICE, "probe setup failed");
    HIPCHK(hipMemset(dout.p, 0xa5, cap * SIX_PROBE_OUT_DW * 4));
    HIPCHK(hipMemset(dok.p, 0xa5, cap * 4));
    hipLaunchKernelGGL(k_probe_six, dim3((n_groups + SIX_GROUPS - 1) / SIX_GROUPS), dim3(64), SIX_LDS_BYTES, nullptr, op, n_groups, (int)csqr_n,
                       da.as<uint32_t>(), db.as<uint32_t>(), dp.as<uint32_t>(), df.as<uint32_t>(), dl.as<uint32_t>(), dout.as<uint32_t>(), dok.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (dout.download(out, cap * SIX_PROBE_OUT_DW * 4) || (ok_out && dok.download(ok_out, cap * 4))) return fail(H2V_E_DEVICE, "download failed");
    return H2V_OK;
}
// ONE call of the cooperative pairing engine per group, in the shape of `engine`: 0 normal (two lanes per coefficient, two groups per
// wave), 1 wide (four lanes, one group), 2 narrow (one lane, four groups), 3 twelve (one lane, five groups).  k_probe_coop in
// h2v_pairing_coop.hpp has the ops and the buffer layouts.  a: n x 12 vectors, always; b: n x 12 (MUL; LINE1 / LINE2: vectors 0..3
// are the loop's T slots); pts: n x 4, lines: 4 x 8 vectors (loop 1's lines 0 and 1, then loop 2's) and flags: n words (LINE1, LINE2,
// PROD, ROUND; PROD - the twelve shape alone - takes no flags); csqr_n: the run length (CSQR, 1..64).  out: (n + GUARD) x 224 dwords
// and ok_out: (n + GUARD) x 2 words (`ok`, and whether the lanes of every pair or quad agreed), GUARD = one block's worth of groups
// at most - both preset to 0xA5 bytes and copied back whole, so what a dead group of the last wave or a spare lane wrote shows.
// For tests; not in include/h2v.h.
#define H2V_PROBE_COOP_GUARD COOP_GROUPS_TWELVE
extern "C" int h2v_probe_coop_call(int device, int engine, int op, uint32_t n_groups, uint32_t csqr_n, const uint32_t *a, const uint32_t *b,
                                   const uint32_t *pts, const uint32_t *flags, const uint32_t *lines, uint32_t *out, uint32_t *ok_out) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (engine < 0 || engine > 3) return fail(H2V_E_ARG, "unknown engine shape (0 normal, 1 wide, 2 narrow, 3 twelve)");
    if (op < 0 || op >= COOP_PROBE_N_OPS) return fail(H2V_E_ARG, "unknown op");
    if (n_groups == 0 || n_groups > (1u << 16)) return fail(H2V_E_ARG, "n_groups out of range (1 .. 65536)");
    if (op == COOP_PROBE_CSQR && (csqr_n == 0 || csqr_n > 64)) return fail(H2V_E_ARG, "CSQR: the run length is 1 .. 64");
    if (op == COOP_PROBE_PROD && engine != 3) return fail(H2V_E_ARG, "PROD: the twelve shape alone has a product pass");
    const bool line_op = op == COOP_PROBE_LINE1 || op == COOP_PROBE_LINE2, uses_lines = line_op || op == COOP_PROBE_PROD || op == COOP_PROBE_ROUND;
    if (!a || !out || !ok_out || ((op == COOP_PROBE_MUL || line_op) && !b) || (uses_lines && (!pts || !lines)) || ((line_op || op == COOP_PROBE_ROUND) && !flags))
        return fail(H2V_E_ARG, "a buffer this op reads or writes is missing");
    const size_t n = n_groups, cap = n + H2V_PROBE_COOP_GUARD, vec = 14 * 4;
    uint32_t lines16[4 * COOP_PROBE_LINE_DW] = {};
    if (lines)
        for (int s = 0; s < 32; s++) memcpy(lines16 + 16 * s, lines + 14 * s, vec);
    DevBuf da, db, dp, df, dl, dout, dok;
    if (da.upload(a, n * 12 * vec) || (b ? db.upload(b, n * 12 * vec) : db.alloc(8)) || (pts ? dp.upload(pts, n * 4 * vec) : dp.alloc(8)) ||
        (flags ? df.upload(flags, n * 4) : df.alloc(8)) || dl.upload(lines16, sizeof lines16) || dout.alloc(cap * COOP_PROBE_OUT_DW * 4) || dok.alloc(cap * 8))
        return fail(H2V_E_DEVICE, "probe setup failed");
    HIPCHK(hipMemset(dout.p, 0xa5, cap * COOP_PROBE_OUT_DW * 4));
    HIPCHK(hipMemset(dok.p, 0xa5, cap * 8));
    static const struct { void (*k)(int, uint32_t, int, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t *, uint32_t *); uint32_t per_wave; } shapes[4] = {
        {k_probe_coop, COOP_GROUPS_PER_WAVE}, {k_probe_coop_wide, 1}, {k_probe_coop_narrow, COOP_GROUPS_NARROW}, {k_probe_coop_twelve, COOP_GROUPS_TWELVE}};
    const uint32_t per_wave = shapes[engine].per_wave;
    hipLaunchKernelGGL(shapes[engine].k, dim3((n_groups + per_wave - 1) / per_wave), dim3(64), COOP_LDS_BYTES(per_wave), nullptr, op, n_groups, (int)csqr_n,
                       da.as<uint32_t>(), db.as<uint32_t>(), dp.as<uint32_t>(), df.as<uint32_t>(), dl.as<uint32_t>(), dout.as<uint32_t>(), dok.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (dout.download(out, cap * COOP_PROBE_OUT_DW * 4) || dok.download(ok_out, cap * 8)) return fail(H2V_E_DEVICE, "download failed");
    return H2V_OK;
}
extern "C" int h2v_probe_blake2b(int device, uint32_t n, uint32_t len, const uint8_t *msgs, uint8_t *digests) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!msgs || !digests || n == 0) return fail(H2V_E_ARG, "bad argument");
    DevBuf dm, dout;
    if (dm.alloc((size_t)n * len) || dout.alloc((size_t)n * 32)) return fail(H2V_E_DEVICE, "hipMalloc failed");
    if (len) HIPCHK(hipMemcpy(dm.p, msgs, (size_t)n * len, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_blake2b, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, len, dm.as<uint8_t>(), dout.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(digests, (size_t)n * 32) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
// the digest kernels of a derived seed alone, through seed_launch as run_call's seed_enqueue queues them.  The proof bytes go up
// from byte 0 of the caller's buffer, so that proof_off[0] decides the alignment the leaf kernel meets.
extern "C" int h2v_probe_batch_seed(int device, uint32_t form, const uint8_t key_tag[32], const h2v_batch *b, uint32_t n_pi, uint32_t n_ci, uint8_t seed[32]) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!key_tag || !b || !seed || !b->proofs) return fail(H2V_E_ARG, "null argument");
    if (form != h2vseed::FORM_PROOFS && form != h2vseed::FORM_PAIRS) return fail(H2V_E_ARG, "form: 1 (proofs) or 2 (pairs)");
    const bool pairs = form == h2vseed::FORM_PAIRS;
    h2vseed::Tree t;
    if (b->n == 0 || !h2vseed::tree(b->n, &t)) return fail(H2V_E_ARG, "n out of range (1 .. 2^22)");
    if (!pairs) {
        if (!b->proof_off || (n_pi && !b->instances) || (n_ci && !b->committed) || n_ci > 1 || n_pi > (1u << 16)) return fail(H2V_E_ARG, "bad argument");
        if (!hostcall::offsets_ascend(b->n, b->proof_off)) return fail(H2V_E_ARG, "proof offsets must ascend");
    }
    const size_t proof_bytes = pairs ? (size_t)b->n * 96 : (size_t)b->proof_off[b->n];
    DevBuf dp, doff, di, dc, dd, ds;
    if (dp.upload(b->proofs, proof_bytes) || dd.alloc((size_t)t.extent * 32) || ds.alloc(32)) return fail(H2V_E_DEVICE, "probe setup failed");
    if (!pairs && (doff.upload(b->proof_off, ((size_t)b->n + 1) * 8) || (n_pi && di.upload(b->instances, (size_t)b->n * n_pi * 32)) ||
                   (n_ci && dc.upload(b->committed, (size_t)b->n * n_ci * 48))))
        return fail(H2V_E_DEVICE, "probe setup failed");
    const SeedJob j = {form, b->n, n_pi * 32u, n_ci * 48u, dp.as<uint8_t>(), doff.as<uint64_t>(), di.as<uint8_t>(), dc.as<uint8_t>(), key_tag, dd.as<uint32_t>(), ds.as<uint32_t>()};
    if ((rc = seed_launch(j, nullptr))) return rc;
    HIPCHK(hipDeviceSynchronize());
    return ds.download(seed, 32) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
// the digest kernels of a keyed seed (form 3) alone, through seed_launch as mixed_seed queues them: the partition and the table
// regions are the calls' own (h2v_mixed.hpp, h2v_mixed_tables.hpp), the plans are (key_tag, n_pi, n_ci) triples.  The proof bytes
// go up from byte 0 of the caller's buffer to the largest offset, so that the offsets decide the alignment the leaf kernel meets.
extern "C" int h2v_probe_mixed_seed(int device, uint32_t n_plans, const uint8_t *key_tags, const uint32_t *n_pi, const uint32_t *n_ci,
                                    const h2v_mixed_batch *b, uint8_t seed[32]) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!key_tags || !n_pi || !n_ci || !b || !seed || !b->proofs || !b->proof_off || !b->plan_of) return fail(H2V_E_ARG, "null argument");
    h2vseed::Tree t;
    if (b->n == 0 || !h2vseed::tree(b->n, &t)) return fail(H2V_E_ARG, "n out of range (1 .. 2^22)");
    if (n_plans == 0 || n_plans > H2V_MIXED_GROUPED_MAX_PLANS) return fail(H2V_E_ARG, "n_plans out of range");
    std::vector<h2vmixed::PlanShape> shapes(n_plans);
    for (uint32_t k = 0; k < n_plans; k++) {
        if (n_ci[k] > 1 || n_pi[k] > (1u << 16)) return fail(H2V_E_ARG, "bad argument");
        shapes[k] = {0u, n_pi[k], n_ci[k]};
    }
    h2vmixed::Partition pt;
    std::string err;
    if (!h2vmixed::partition(shapes.data(), n_plans, b->plan_of, b->n, pt, &err)) return fail(H2V_E_ARG, err);
    if ((pt.inst_total && !b->instances) || (pt.ci_total && !b->committed)) return fail(H2V_E_ARG, "bad argument");
    const mixedtab::TableBlock B = mixedtab::table_block(pt.n, 0, nullptr, 0, n_plans);
    std::vector<uint8_t> block(B.extent);
    std::vector<mixedtab::RangeInfo> info;
    mixedtab::pack_tables(block.data(), B, pt, nullptr, {}, info, b->plan_of, key_tags);
    uint64_t proof_bytes = 0;
    for (uint64_t i = 0; i <= b->n; i++) proof_bytes = b->proof_off[i] > proof_bytes ? b->proof_off[i] : proof_bytes;
    DevBuf dt, dp, doff, di, dc, dd, ds;
    if (dt.upload(block.data(), B.extent) || dp.upload(b->proofs, proof_bytes ? (size_t)proof_bytes : 1u) || doff.upload(b->proof_off, ((size_t)b->n + 1) * 8) ||
        (pt.inst_total && di.upload(b->instances, (size_t)pt.inst_total)) || (pt.ci_total && dc.upload(b->committed, (size_t)pt.ci_total * 48)) ||
        dd.alloc((size_t)t.extent * 32) || ds.alloc(32))
        return fail(H2V_E_DEVICE, "probe setup failed");
    auto tab = [&](const mixedtab::Region &g) { return dt.as<uint8_t>() + g.off; };
    const SeedMixedLeafArgs ma = {pt.n, (const uint32_t *)tab(B.perm), (const uint64_t *)tab(B.inst_src), (const uint32_t *)tab(B.inst_len), (const uint32_t *)tab(B.ci_src),
                                  (const uint32_t *)tab(B.plan_idx), (const uint32_t *)tab(B.key_tags), dp.as<uint8_t>(), doff.as<uint64_t>(), di.as<uint8_t>(), dc.as<uint8_t>(), {}, nullptr};
    SeedJob j = {h2vseed::FORM_MIXED, b->n, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, dd.as<uint32_t>(), ds.as<uint32_t>()};
    j.mixed = &ma;
    if ((rc = seed_launch(j, nullptr))) return rc;
    HIPCHK(hipDeviceSynchronize());
    return ds.download(seed, 32) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
extern "C" int h2v_probe_blake2b_ex(int device, uint32_t n, uint32_t len, const uint8_t *msgs, uint32_t digest_len, const uint8_t *key,
                                    uint32_t key_len, uint8_t *digests) {
    int rc = pick_device(device);
    if (rc) return rc;
    if ((len && !msgs) || !digests || n == 0 || (digest_len != 32 && digest_len != 64) || key_len > H2V_TR_KEY_MAX || (key_len && !key))
        return fail(H2V_E_ARG, "bad argument");
    if ((uint64_t)n * len > ((uint64_t)1 << 31)) return fail(H2V_E_LIMIT, "messages larger than 2 GB");
    // with a message the hash starts behind the key block, from the state the plan loader computes on the host; an empty
    // message makes the key block the final block, which the kernel then hashes itself
    H2vProbeHash ph{};
    uint8_t block[128] = {};
    if (key_len) memcpy(block, key, key_len);
    const bool key_is_last = key_len != 0 && len == 0;
    ph.t0 = h2vhost::b2_keyed_midstate_host(ph.h0, digest_len, key, key_is_last ? 0u : key_len);
    if (key_is_last) ph.h0[0] ^= (uint64_t)key_len << 8;   // (the mid-state helper was asked for the unkeyed state: put the key length back)
    ph.prefix_len = key_is_last ? 128u : 0u;
    ph.digest_words = digest_len / 8;
    DevBuf dm, dk, dout;
    if (dm.alloc((size_t)n * len + 16) || dk.upload(block, 128) || dout.alloc((size_t)n * digest_len)) return fail(H2V_E_DEVICE, "probe setup failed");
    if (len) HIPCHK(hipMemcpy(dm.p, msgs, (size_t)n * len, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_blake2b_ex, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, len, dm.as<uint8_t>(), ph, dk.as<uint8_t>(), dout.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(digests, (size_t)n * digest_len) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
// A throw-away plan whose "proof" is `slots` consecutive compressed points and whose MSM takes them in order.
struct MiniPlan {
    H2vDevPlan d{};
    DevBuf points, terms;
    int build(uint32_t slots, uint32_t n_terms, const uint32_t *lines_sg2, const uint32_t *lines_g2) {
        std::vector<uint32_t> pts(slots), terms_h(2 * (n_terms ? n_terms : 1));
        for (uint32_t j = 0; j < slots; j++) pts[j] = 48 * j;
        for (uint32_t t = 0; t < n_terms; t++) { terms_h[2 * t] = H2V_TERM_PROOF_POINT; terms_h[2 * t + 1] = t; }
        if (points.upload(pts.data(), slots * 4) || terms.upload(terms_h.data(), terms_h.size() * 4)) return -1;
        d.proof_len = 48 * slots; d.n_points = slots; d.n_terms = n_terms; d.n_main_terms = n_terms; d.pi_point = 0;
        d.points = points.as<uint32_t>(); d.terms = terms.as<uint32_t>();
        d.lines_sg2 = lines_sg2; d.lines_g2 = lines_g2;
        return 0;
    }
};
static int upload_offsets(DevBuf &doff, uint32_t n, uint32_t rec) {
    std::vector<uint64_t> off(n + 1);
    for (uint32_t i = 0; i <= n; i++) off[i] = (uint64_t)i * rec;
    return doff.upload(off.data(), (n + 1) * 8);
}
extern "C" int h2v_probe_g1_decompress(int device, uint32_t n, const uint8_t *compressed, uint8_t *xy_be, uint8_t *valid) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!compressed || !xy_be || !valid || n == 0) return fail(H2V_E_ARG, "bad argument");
    MiniPlan mp;
    DevBuf din, doff, dpts, dvalid, dout;
    if (mp.build(1, 0, nullptr, nullptr) || upload_offsets(doff, n, 48) || din.upload(compressed, (size_t)n * 48) || dpts.alloc((size_t)n * 96) ||
        dvalid.alloc(n) || dout.alloc((size_t)n * 96)) return fail(H2V_E_DEVICE, "probe setup failed");
    hipLaunchKernelGGL(k_g1_decompress, dim3((n + 63) / 64), dim3(128), 0, nullptr, mp.d, n, din.as<uint8_t>(), doff.as<uint64_t>(), (const uint8_t *)nullptr, (const uint8_t *)nullptr, dpts.as<uint32_t>(), dvalid.as<uint8_t>(), (uint32_t *)nullptr, 0u, (uint8_t *)nullptr);
    hipLaunchKernelGGL(k_export_points, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, 0, dpts.as<uint32_t>(), dout.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(xy_be, (size_t)n * 96) || dvalid.download(valid, n) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
extern "C" int h2v_probe_g1_msm(int device, uint32_t n, uint32_t T, const uint8_t *scalars, const uint8_t *bases_compressed, uint8_t *out_xy_be) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!scalars || !bases_compressed || !out_xy_be || n == 0 || T == 0) return fail(H2V_E_ARG, "bad argument");
    if (T > H2V_MAX_MSM_TERMS)
        return fail(H2V_E_LIMIT, "the MSM has " + std::to_string(T) + " terms; this backend sums at most " + std::to_string(H2V_MAX_MSM_TERMS) +
                                     " terms per MSM (H2V_MAX_MSM_TERMS)");
    ProbeOpts probe_opts;
    MiniPlan mp;
    DevBuf din, doff, dsc, dpts, dvalid, der, dout, dtab, dparts;
    const uint32_t segs = msm_max_segments(T);
    if (mp.build(T, T, nullptr, nullptr) || upload_offsets(doff, n, 48 * T) || din.upload(bases_compressed, (size_t)n * T * 48) || dsc.upload(scalars, (size_t)n * T * 32) ||
        dpts.alloc((size_t)n * T * 96) || dvalid.alloc((size_t)n * T) || der.alloc((size_t)n * 144) || dout.alloc((size_t)n * 96) ||
        (segs && dparts.alloc((size_t)n * segs * 144)))
        return fail(H2V_E_DEVICE, "probe setup failed");
    if (dtab.alloc((size_t)n * T * 448 * 4)) return fail(H2V_E_DEVICE, "hipMalloc failed");
    hipLaunchKernelGGL(k_g1_decompress, dim3((n * T + 63) / 64), dim3(128), 0, nullptr, mp.d, n, din.as<uint8_t>(), doff.as<uint64_t>(), (const uint8_t *)nullptr, (const uint8_t *)nullptr, dpts.as<uint32_t>(), dvalid.as<uint8_t>(), dtab.as<uint32_t>(), 0u, (uint8_t *)nullptr);
    if (!launch_msm(mp.d, n, dsc.as<uint32_t>(), dpts.as<uint32_t>(), dtab.as<uint32_t>(), der.as<uint32_t>(), nullptr, nullptr, nullptr, 1, SegBuf{dparts.as<uint32_t>(), segs}))
        return fail(H2V_E_LIMIT, "no MSM launch shape fits this sum");
    hipLaunchKernelGGL(k_export_points, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, 1, der.as<uint32_t>(), dout.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out_xy_be, (size_t)n * 96) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}
// The multi-term ladder (k_g1_msm_multi) with a lane shape of the caller's choosing: h2v_probe_g1_msm's setup, then the launch as
// launch_msm_range makes it (256-thread blocks, 256 / lpp proofs per block) with `halves_per_lane` halves per lane - the odd
// shapes included, which the launcher reaches only unforced and in large batches.
extern "C" int h2v_probe_g1_msm_multi(int device, uint32_t n, uint32_t T, uint32_t halves_per_lane, const uint8_t *scalars, const uint8_t *bases_compressed,
                                      uint8_t *out_xy_be) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!scalars || !bases_compressed || !out_xy_be || n == 0 || T == 0) return fail(H2V_E_ARG, "bad argument");
    if (halves_per_lane < 3 || halves_per_lane > MSM_MAX_HALVES) return fail(H2V_E_ARG, "halves per lane: 3 .. 8");
    if (T > H2V_MAX_MSM_TERMS) return fail(H2V_E_LIMIT, "more terms than H2V_MAX_MSM_TERMS");
    const uint32_t bs = 256, lpp = (2 * T + halves_per_lane - 1) / halves_per_lane;
    if (lpp > bs) return fail(H2V_E_ARG, "more than 256 lanes per proof");
    MiniPlan mp;
    DevBuf din, doff, dsc, dpts, dvalid, der, dout, dtab;
    if (mp.build(T, T, nullptr, nullptr) || upload_offsets(doff, n, 48 * T) || din.upload(bases_compressed, (size_t)n * T * 48) || dsc.upload(scalars, (size_t)n * T * 32) ||
        dpts.alloc((size_t)n * T * 96) || dvalid.alloc((size_t)n * T) || der.alloc((size_t)n * 144) || dout.alloc((size_t)n * 96))
        return fail(H2V_E_DEVICE, "probe setup failed");
    if (dtab.alloc((size_t)n * T * 448 * 4)) return fail(H2V_E_DEVICE, "hipMalloc failed");
    hipLaunchKernelGGL(k_g1_decompress, dim3((n * T + 63) / 64), dim3(128), 0, nullptr, mp.d, n, din.as<uint8_t>(), doff.as<uint64_t>(), (const uint8_t *)nullptr, (const uint8_t *)nullptr, dpts.as<uint32_t>(), dvalid.as<uint8_t>(), dtab.as<uint32_t>(), 0u, (uint8_t *)nullptr);
    const H2vMsmArgs ma = msm_args(mp.d, 0, T, T, 0, H2V_SLOTS(mp.d), der.as<uint32_t>(), dtab.as<uint32_t>());
    const uint32_t per_block = bs / lpp, blocks = (n + per_block - 1) / per_block;
    hipLaunchKernelGGL(k_g1_msm_multi, dim3(blocks), dim3(bs), MSM_LDS_BYTES(bs), nullptr, mp.d, ma, n, per_block, halves_per_lane, dsc.as<uint32_t>(), dpts.as<uint32_t>(), (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_export_points, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, 1, der.as<uint32_t>(), dout.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out_xy_be, (size_t)n * 96) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}

// the fixed-base launch of a split MSM over the plan's own VK-base terms, scalars given by the caller
extern "C" int h2v_probe_g1_msm_fixed(const h2v_plan *p, uint32_t n, uint32_t k, const uint8_t *scalars, uint8_t *out_xy_be, uint32_t *n_fix_out) {
    if (!p) return fail(H2V_E_ARG, "bad argument");
    ALIVE(p);
    if (n_fix_out) *n_fix_out = p->n_fix;
    if (!p->fix_tab || !p->n_fix) return fail(H2V_E_ARG, "this plan has no fixed-base tables");
    if (!scalars || !out_xy_be || n == 0 || k == 0 || k > 4) return fail(H2V_E_ARG, "bad argument");
    HIPCHK(hipSetDevice(p->device));
    const H2vDevPlan &d = p->d;
    DevBuf dsc, der, dout;
    if (dsc.upload(scalars, (size_t)n * d.n_fix * 32) || der.alloc((size_t)n * 144) || dout.alloc((size_t)n * 96)) return fail(H2V_E_DEVICE, "probe setup failed");
    const H2vMsmArgs mf = msm_fixed_args(d, d.n_fix, 0, der.as<uint32_t>(), nullptr, k);
    const uint32_t bs = mf.n_fixl <= 64 ? 64u : mf.n_fixl <= 256 ? 256u : 512u;
    if (mf.n_fixl > bs) return fail(H2V_E_LIMIT, "too many VK bases for one block");
    launch_msm_fixed(d, mf, n, bs, dsc.as<uint32_t>(), nullptr, nullptr);
    hipLaunchKernelGGL(k_export_points, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, 1, der.as<uint32_t>(), dout.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return dout.download(out_xy_be, (size_t)n * 96) ? fail(H2V_E_DEVICE, "download failed") : (int)H2V_OK;
}

// The bucket MSM on its own, through pip_alloc / pip_launch as the RLC mode calls them: 1 or 2 problems side by side in every launch,
// each with its own term count, halves, scalars, point pool (compressed; decompressed here; split into pool0 / pool1 at n_pool0,
// which live in separate allocations) and optional index map; the grid of k_pip_accumulate capped at acc_grid_cap blocks (0: not
// capped); per problem an optional dump of what the launcher chose and k_pip_scan wrote (include/h2v.h has the layout).
extern "C" int h2v_probe_g1_msm_pippenger_ex(int device, uint32_t n_problems, const h2v_pip_probe *pr, uint32_t acc_grid_cap) {
    int rc = pick_device(device);
    if (rc) return rc;
    if (!pr || n_problems < 1 || n_problems > 2) return fail(H2V_E_ARG, "bad argument");
    static_assert(H2V_PIP_DUMP_DWORDS == 5 + PIP_CLS_DW + 2 * PIP_MAX_W * (1u << (PIP_MAX_C - 1)) + 1, "h2v.h: the dump holds the largest shape");
    for (uint32_t q = 0; q < n_problems; q++) {
        const h2v_pip_probe &p = pr[q];
        if (!p.scalars || !p.points_compressed || !p.out_xy_be || p.n == 0 || p.n > (1u << 24) || p.n_points == 0 || p.n_points > (1u << 24) ||
            (p.halves != 1 && p.halves != 2) || p.n_pool0 > p.n_points || (!p.pidx && p.n != p.n_points))
            return fail(H2V_E_ARG, "bad argument");
        if (p.pidx)
            for (uint32_t i = 0; i < p.n; i++)
                if (p.pidx[i] >= p.n_points) return fail(H2V_E_ARG, "point index " + std::to_string(p.pidx[i]) + " is outside the pool");
        if (p.halves == 1)
            for (uint32_t i = 0; i < p.n; i++)
                for (int k = 16; k < 32; k++)
                    if (p.scalars[(size_t)i * 32 + k]) return fail(H2V_E_ARG, "halves = 1 takes scalars below 2^128");
    }
    ProbeOpts probe_opts;
    MiniPlan mp;
    struct Prob {
        DevBuf din, doff, dsc, didx, dpts, dpool1, dvalid, dres;
        PipWs pw;
        ~Prob() { pip_free(pw); }
    } P[2];
    DevBuf dout;
    if (mp.build(1, 0, nullptr, nullptr) || dout.alloc(2 * 96)) return fail(H2V_E_DEVICE, "probe setup failed");
    PipArgs a[2] = {};
    const PipWs *pws[2] = {&P[0].pw, &P[1].pw};
    for (uint32_t q = 0; q < n_problems; q++) {
        const h2v_pip_probe &p = pr[q];
        Prob &b = P[q];
        const uint32_t n1 = p.n_points - p.n_pool0;
        if (upload_offsets(b.doff, p.n_points, 48) || b.din.upload(p.points_compressed, (size_t)p.n_points * 48) || b.dsc.upload(p.scalars, (size_t)p.n * 32) ||
            b.dpts.alloc((size_t)p.n_points * 96) || b.dvalid.alloc(p.n_points) || b.dres.alloc(144) || (p.pidx && b.didx.upload(p.pidx, (size_t)p.n * 4)) ||
            (n1 && b.dpool1.alloc((size_t)n1 * 96))) return fail(H2V_E_DEVICE, "probe setup failed");
        hipLaunchKernelGGL(k_g1_decompress, dim3((p.n_points + 63) / 64), dim3(128), 0, nullptr, mp.d, p.n_points, b.din.as<uint8_t>(), b.doff.as<uint64_t>(), (const uint8_t *)nullptr, (const uint8_t *)nullptr, b.dpts.as<uint32_t>(), b.dvalid.as<uint8_t>(), (uint32_t *)nullptr, 0u, (uint8_t *)nullptr);
        if (n1) {   // the records from n_pool0 on move to an allocation of their own and read as infinity where they were
            HIPCHK(hipMemcpy(b.dpool1.p, b.dpts.as<uint8_t>() + (size_t)p.n_pool0 * 96, (size_t)n1 * 96, hipMemcpyDeviceToDevice));
            HIPCHK(hipMemset(b.dpts.as<uint8_t>() + (size_t)p.n_pool0 * 96, 0, (size_t)n1 * 96));
        }
        if ((rc = pip_alloc(b.pw, p.n, p.halves))) return rc;
        // a bucket sum, window value or result the kernels fail to write must read as infinity, not as what an earlier run of the
        // same input left at the address the allocator hands out again
        HIPCHK(hipMemset(b.pw.partial, 0xff, (size_t)PIP_MAX_W * (1u << (PIP_MAX_C - 1)) * PIP_PART_DW * 4));
        HIPCHK(hipMemset(b.pw.wsum, 0xff, (size_t)PIP_MAX_W * PIP_PART_DW * 4));
        HIPCHK(hipMemset(b.dres.p, 0, 144));
        a[q].n = p.n; a[q].halves = p.halves; a[q].scal = b.dsc.as<uint32_t>(); a[q].pidx = p.pidx ? b.didx.as<uint32_t>() : nullptr;
        a[q].pool0 = b.dpts.as<uint32_t>(); a[q].n_pool0 = p.n_pool0; a[q].pool1 = n1 ? b.dpool1.as<uint32_t>() : nullptr; a[q].out = b.dres.as<uint32_t>();
    }
    uint32_t acc_blocks = 0;
    if ((rc = pip_launch(pws, a, n_problems, nullptr, nullptr, acc_grid_cap, &acc_blocks))) return rc;
    for (uint32_t q = 0; q < n_problems; q++)
        hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, 1u, 1, P[q].dres.as<uint32_t>(), dout.as<uint8_t>() + 96 * q);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(H2V_E_DEVICE, "bucket MSM kernels failed");
    for (uint32_t q = 0; q < n_problems; q++) {
        HIPCHK(hipMemcpy(pr[q].out_xy_be, dout.as<uint8_t>() + 96 * q, 96, hipMemcpyDeviceToHost));
        if (uint32_t *d = pr[q].dump) {
            const uint32_t nb = a[q].W * a[q].NB;
            d[0] = a[q].c; d[1] = a[q].W; d[2] = a[q].NB; d[3] = a[q].chain; d[4] = acc_blocks;
            HIPCHK(hipMemcpy(d + 5, P[q].pw.cls, PIP_CLS_DW * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(d + 5 + PIP_CLS_DW, P[q].pw.off, (size_t)(nb + 1) * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(d + 5 + PIP_CLS_DW + nb + 1, P[q].pw.order, (size_t)nb * 4, hipMemcpyDeviceToHost));
        }
    }
    return H2V_OK;
}
// sum_n s_n * P_n through the bucket MSM: n scalars (32 B LE, < r) and n compressed bases; out 96 B affine big-endian
extern "C" int h2v_probe_g1_msm_pippenger(int device, uint32_t n, const uint8_t *scalars, const uint8_t *bases_compressed, uint8_t *out_xy_be) {
    h2v_pip_probe p = {};
    p.n = n; p.halves = 2; p.scalars = scalars; p.n_points = n; p.n_pool0 = n; p.points_compressed = bases_compressed; p.out_xy_be = out_xy_be;
    return h2v_probe_g1_msm_pippenger_ex(device, 1, &p, 0);
}
// The two sums of the most recent H2V_MIXED_FOLD_MSM call on ws - L then R, affine, 96 bytes big-endian x || y each, all-zero for
// infinity - whether its check passed or the call fell back (the second pass does not touch them).  The call has synchronised its
// stream already; the conversion runs on the NULL stream and the device is synchronised behind it.
extern "C" int h2v_probe_mixed_fold_sums(h2v_workspace *ws, uint8_t out_xy_be[192]) {
    if (!ws || !out_xy_be) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    const MixedWs *m = ws->mixed;
    if (!m || !m->fold || !m->fold_ran) return fail(H2V_E_ARG, "no call with H2V_MIXED_FOLD_MSM has run on this workspace");
    HIPCHK(hipSetDevice(ws->device));
    DevBuf dout;
    if (dout.alloc(192)) return fail(H2V_E_DEVICE, "hipMalloc failed");
    HIPCHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, 2u, 1, (const uint32_t *)m->fold->sums, dout.as<uint8_t>());   // [0] = R, [1] = L
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_xy_be, (const uint8_t *)dout.p + 96, 96, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_xy_be + 96, dout.p, 96, hipMemcpyDeviceToHost));
    return H2V_OK;
}
// The sums of the most recent H2V_MIXED_ACROSS_SRS | H2V_MIXED_FOLD_MSM call on ws: R, then L_k of every class with proofs, in
// class order - (1 + *n_classes) affine records; cap: the classes the caller's buffer has room for.
extern "C" int h2v_probe_mixed_fold_sums_multi(h2v_workspace *ws, uint32_t cap, uint8_t *out_xy_be, uint32_t *n_classes) {
    if (!ws || !out_xy_be || !n_classes) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    const MixedWs *m = ws->mixed;
    if (!m || !m->across || !m->fold_ran || !m->across->fold_classes)
        return fail(H2V_E_ARG, "the most recent H2V_MIXED_FOLD_MSM call on this workspace (if any) did not carry H2V_MIXED_ACROSS_SRS");
    const uint32_t C = m->across->fold_classes;
    if (cap < C) return fail(H2V_E_ARG, "the call had " + std::to_string(C) + " SRS classes with proofs, the buffer has room for " + std::to_string(cap));
    HIPCHK(hipSetDevice(ws->device));
    DevBuf dout;
    if (dout.alloc((size_t)(C + 1) * 96)) return fail(H2V_E_DEVICE, "hipMalloc failed");
    HIPCHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_export_points, dim3(1), dim3(64), 0, nullptr, C + 1, 1, (const uint32_t *)m->across->sums, dout.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_xy_be, dout.p, (size_t)(C + 1) * 96, hipMemcpyDeviceToHost));
    *n_classes = C;
    return H2V_OK;
}
// The transcript + combiner launch alone, on a batch: status words, term scalars and (want_trace) the plan's trace registers of
// every proof.  Nothing behind launch_vm runs, so a plan whose OUT_SCALARs mean nothing to the MSM is safe here.  The outputs
// are preset (scalars and trace zero, status all ones), so what the kernel left unwritten is visible as such.
extern "C" int h2v_probe_vm(const h2v_plan *p, const h2v_batch *b, int want_trace, uint32_t *status_out, uint8_t *msm_scalars_out, uint8_t *trace_out) {
    if (!p || !b || !status_out || !msm_scalars_out) return fail(H2V_E_ARG, "null argument");
    if (b->n == 0 || b->n > (1ull << 24)) return fail(H2V_E_ARG, "batch size out of range");
    if (!b->proofs || !b->proof_off) return fail(H2V_E_ARG, "null batch buffers");
    if (p->d.n_pi && !b->instances) return fail(H2V_E_ARG, "plan has public inputs but instances == NULL");
    if (p->d.n_ci && !b->committed) return fail(H2V_E_ARG, "plan has a committed instance but committed == NULL");
    if (want_trace ? (!trace_out || !p->d.n_trace) : trace_out != nullptr)
        return fail(H2V_E_ARG, "trace_out goes with want_trace and a plan that has a trace table");
    ALIVE(p);
    HIPCHK(hipSetDevice(p->device));
    ProbeOpts probe_opts;
    const uint32_t n = (uint32_t)b->n;
    const H2vDevPlan &d = p->d;
    h2v_workspace *ws = nullptr;
    int rc = ws_create_for(wslayout::shape_of(d, want_trace != 0), p->device, n, &ws);
    if (rc) return rc;
    h2v_batch in;
    rc = stage_batch(p, b, ws, ws->hslot[0], &in);
    do {
        if (rc) break;
        const size_t sc_bytes = (size_t)n * d.n_terms * 32, tr_bytes = (size_t)n * d.n_trace * 32;
        if (hipMemsetAsync(ws->scalars, 0, sc_bytes, ws->hs) != hipSuccess || hipMemsetAsync(ws->status, 0xff, (size_t)n * 4, ws->hs) != hipSuccess ||
            (want_trace && hipMemsetAsync(ws->trace, 0, tr_bytes, ws->hs) != hipSuccess)) { rc = fail(H2V_E_DEVICE, "hipMemsetAsync failed"); break; }
        if ((rc = launch_vm(d, n, ws->stride, in.proofs, in.proof_off, in.instances, in.committed, ws->regs, ws->scalars, ws->status, want_trace ? ws->trace : nullptr, ws->hs))) break;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ws->hs) != hipSuccess) { rc = fail(H2V_E_DEVICE, "combiner kernel failed"); break; }
        if (hipMemcpy(status_out, ws->status, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(msm_scalars_out, ws->scalars, sc_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            (want_trace && hipMemcpy(trace_out, ws->trace, tr_bytes, hipMemcpyDeviceToHost) != hipSuccess)) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
    } while (0);
    h2v_workspace_free(ws);
    return rc;
}
// The decompression launch alone, on a batch, exactly as the pipelines make it (launch_decompress on a staged batch, with or
// without the window tables): every per-point output of k_g1_decompress_queue and the grid it ran on.  The outputs are preset
// (points, verdicts and tables to 0xA5 bytes), so what the kernel left unwritten is visible as such.
extern "C" int h2v_probe_decompress(const h2v_plan *p, const h2v_batch *b, int with_tables, uint8_t *xy_be, uint8_t *valid_out, uint8_t *valid_sub_out,
                                    uint32_t *tables_out, uint32_t *blocks_out) {
    if (!p || !b || !xy_be || !valid_out || !valid_sub_out || !blocks_out) return fail(H2V_E_ARG, "null argument");
    if (b->n == 0 || b->n > (1ull << 24)) return fail(H2V_E_ARG, "batch size out of range");
    if (!b->proofs || !b->proof_off) return fail(H2V_E_ARG, "null batch buffers");
    if (p->d.n_pi && !b->instances) return fail(H2V_E_ARG, "plan has public inputs but instances == NULL");
    if (p->d.n_ci && !b->committed) return fail(H2V_E_ARG, "plan has a committed instance but committed == NULL");
    if (tables_out && !with_tables) return fail(H2V_E_ARG, "tables_out goes with with_tables");
    ALIVE(p);
    HIPCHK(hipSetDevice(p->device));
    const uint32_t n = (uint32_t)b->n;
    const H2vDevPlan &d = p->d;
    const size_t n_pts = (size_t)n * H2V_SLOTS(d);
    h2v_workspace *ws = nullptr;
    int rc = ws_create_for(wslayout::shape_of(d, false), p->device, n, &ws);
    if (rc) return rc;
    DevBuf dout;
    h2v_batch in;
    rc = stage_batch(p, b, ws, ws->hslot[0], &in);
    do {
        if (rc) break;
        if (dout.alloc(n_pts * 96)) { rc = fail(H2V_E_DEVICE, "hipMalloc failed"); break; }
        if (hipMemsetAsync(ws->pts, 0xa5, n_pts * 96, ws->hs) != hipSuccess || hipMemsetAsync(ws->valid, 0xa5, n_pts, ws->hs) != hipSuccess ||
            hipMemsetAsync(ws->valid_sub, 0xa5, n_pts, ws->hs) != hipSuccess || hipMemsetAsync(ws->pt_tab, 0xa5, n_pts * 448 * 4, ws->hs) != hipSuccess) {
            rc = fail(H2V_E_DEVICE, "hipMemsetAsync failed"); break;
        }
        if ((rc = launch_decompress(d, n, in.proofs, in.proof_off, in.committed, in.instances, ws, with_tables ? ws->pt_tab : nullptr, ws->hs, blocks_out))) break;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ws->hs) != hipSuccess) { rc = fail(H2V_E_DEVICE, "decompression kernel failed"); break; }
        if (hipMemcpy(valid_out, ws->valid, n_pts, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(valid_sub_out, ws->valid_sub, n_pts, hipMemcpyDeviceToHost) != hipSuccess ||
            (tables_out && hipMemcpy(tables_out, ws->pt_tab, n_pts * 448 * 4, hipMemcpyDeviceToHost) != hipSuccess)) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
        // (a point slot the kernel left at the preset is no field element: k_export_points would reduce it; such a slot shows in
        //  valid[], which the preset makes neither 0 nor 1)
        hipLaunchKernelGGL(k_export_points, dim3((uint32_t)((n_pts + 63) / 64)), dim3(64), 0, ws->hs, (uint32_t)n_pts, 0, ws->pts, dout.as<uint8_t>());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ws->hs) != hipSuccess) { rc = fail(H2V_E_DEVICE, "export kernel failed"); break; }
        if (hipMemcpy(xy_be, dout.p, n_pts * 96, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(H2V_E_DEVICE, "download failed"); break; }
    } while (0);
    h2v_workspace_free(ws);
    return rc;
}
// The pairing launch alone on n pairs, with every entry state a pipeline can hand it.  impl: -1 default, 1 the same under
// H2V_OPT_PAIRING_ENGINE of h2v_probe_set_option, or an engine's number in h2v_pairing_engine.hpp's table - that engine whatever
// n; any other number is -1.  Optional inputs (NULL: as the pipelines' first launch has them): status_in (n words
// the proofs arrive with), valid_sub_in (n x 2 bytes, the subgroup verdicts of slots p1, p2; NULL: the kernels get no such array),
// el_jac_in (n x 36 dwords X, Y, Z, Montgomery limbs: the first argument, instead of slot p1).  Outputs, each optional: status_out
// (n + H2V_PROBE_PAIRING_GUARD words), accept (n + GUARD bytes), dbg ((n + GUARD) x 24 x 48 bytes: f after the Miller loop and after
// the final exponentiation, canonical LE limbs; NULL: the kernels get no dump buffer), lanes_out (launch_pairing's answer: the
// engine that ran).  The device outputs are allocated for n + GUARD proofs, preset to 0xA5 bytes and copied back whole: what a
// kernel left unwritten shows as such, and so does what a dead group of the last wave wrote behind proof n - 1.
extern "C" int h2v_probe_pairing_states(const h2v_plan *p, uint32_t n, const uint8_t *p1c, const uint8_t *p2c, int impl, const uint32_t *status_in,
                                        const uint8_t *valid_sub_in, const uint32_t *el_jac_in, uint32_t *status_out, uint8_t *accept, uint8_t *dbg,
                                        uint32_t *lanes_out) {
    if (!p || !p1c || !p2c || n == 0 || n > (1u << 24)) return fail(H2V_E_ARG, "bad argument");
    ALIVE(p);
    ProbeOpts probe_opts;
    HIPCHK(hipSetDevice(p->device));
    MiniPlan mp;
    DevBuf din, doff, dsc, dpts, dvalid, dsub, del, der, dst, dacc, dtab, ddbg;
    mp.d.lines28_sg2 = p->d.lines28_sg2;
    mp.d.lines28_g2 = p->d.lines28_g2;
    mp.d.six_norm28 = p->d.six_norm28;
    mp.d.six_k = p->d.six_k;
    const size_t cap = (size_t)n + H2V_PROBE_PAIRING_GUARD;
    if (mp.build(2, 1, p->d.lines_sg2, p->d.lines_g2) || upload_offsets(doff, n, 96) || din.alloc((size_t)n * 96) || dsc.alloc((size_t)n * 32) ||
        dpts.alloc((size_t)n * 192) || dvalid.alloc((size_t)n * 2) || der.alloc((size_t)n * 144) || dst.alloc(cap * 4) || dacc.alloc(cap) ||
        dtab.alloc((size_t)n * 2 * 448 * 4) || ddbg.alloc(dbg ? cap * 24 * 48 : 8) || (valid_sub_in && dsub.upload(valid_sub_in, (size_t)n * 2)) ||
        (el_jac_in && del.upload(el_jac_in, (size_t)n * 144)))
        return fail(H2V_E_DEVICE, "probe setup failed");
    // MSM "sum" is 1 * p2 (term 0 must read slot 1): patch the single term
    uint32_t term[2] = {H2V_TERM_PROOF_POINT, 1};
    HIPCHK(hipMemcpy(mp.terms.p, term, 8, hipMemcpyHostToDevice));
    std::vector<uint8_t> in((size_t)n * 96), one((size_t)n * 32, 0);
    for (uint32_t i = 0; i < n; i++) { memcpy(&in[(size_t)i * 96], p1c + (size_t)i * 48, 48); memcpy(&in[(size_t)i * 96 + 48], p2c + (size_t)i * 48, 48); one[(size_t)i * 32] = 1; }
    HIPCHK(hipMemcpy(din.p, in.data(), in.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsc.p, one.data(), one.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dst.p, 0xa5, cap * 4));
    HIPCHK(hipMemset(dacc.p, 0xa5, cap));
    if (dbg) HIPCHK(hipMemset(ddbg.p, 0xa5, cap * 24 * 48));
    if (status_in) HIPCHK(hipMemcpy(dst.p, status_in, (size_t)n * 4, hipMemcpyHostToDevice));
    else HIPCHK(hipMemset(dst.p, 0, (size_t)n * 4));
    hipLaunchKernelGGL(k_g1_decompress, dim3((n * 2 + 63) / 64), dim3(128), 0, nullptr, mp.d, n, din.as<uint8_t>(), doff.as<uint64_t>(), (const uint8_t *)nullptr, (const uint8_t *)nullptr, dpts.as<uint32_t>(), dvalid.as<uint8_t>(), dtab.as<uint32_t>(), 0u, (uint8_t *)nullptr);
    launch_msm(mp.d, n, dsc.as<uint32_t>(), dpts.as<uint32_t>(), dtab.as<uint32_t>(), der.as<uint32_t>(), nullptr, nullptr, nullptr);
    const uint32_t lanes = launch_pairing(mp.d, n, dpts.as<uint32_t>(), dvalid.as<uint8_t>(), valid_sub_in ? dsub.as<uint8_t>() : nullptr, der.as<uint32_t>(),
                                          el_jac_in ? del.as<uint32_t>() : nullptr, dst.as<uint32_t>(), dacc.as<uint8_t>(), dbg ? ddbg.as<uint32_t>() : nullptr, nullptr,
                                          PAIRING_HINT_PROBE, nullptr, impl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (lanes_out) *lanes_out = lanes;
    if ((status_out && dst.download(status_out, cap * 4)) || (accept && dacc.download(accept, cap)) || (dbg && ddbg.download(dbg, cap * 24 * 48)))
        return fail(H2V_E_DEVICE, "download failed");
    return H2V_OK;
}
// e(p1, s_g2) == e(p2, G2) with status 0 on entry: the first n verdicts (and, dbg given, the first n x 24 records) of the call above
extern "C" int h2v_probe_pairing_ex(const h2v_plan *p, uint32_t n, const uint8_t *p1c, const uint8_t *p2c, uint8_t *out, int impl, uint8_t *dbg) {
    if (!p || !p1c || !p2c || !out || n == 0 || n > (1u << 24)) return fail(H2V_E_ARG, "bad argument");
    const size_t cap = (size_t)n + H2V_PROBE_PAIRING_GUARD;
    std::vector<uint8_t> acc(cap), rec(dbg ? cap * 24 * 48 : 0);
    const int rc = h2v_probe_pairing_states(p, n, p1c, p2c, impl, nullptr, nullptr, nullptr, nullptr, acc.data(), dbg ? rec.data() : nullptr, nullptr);
    if (rc) return rc;
    memcpy(out, acc.data(), n);
    if (dbg) memcpy(dbg, rec.data(), (size_t)n * 24 * 48);
    return H2V_OK;
}
extern "C" int h2v_probe_pairing(const h2v_plan *p, uint32_t n, const uint8_t *p1c, const uint8_t *p2c, uint8_t *out) {
    return h2v_probe_pairing_ex(p, n, p1c, p2c, out, -1, nullptr);
}
