// Derived batch seeds, host side (H2V_RLC_SEED_TRANSCRIPT, and H2V_RLC_SEED_KEYED of the mixed-key calls): what the flags say, the
// digest launches of one derivation, THE enqueue site of a call's derivation (the seed ring, the digest buffer, the timed events)
// and the two getters.  Included by h2v_capi.hip at the place the code stood (it uses its workspace, records, units and error
// helpers); the rule is in h2v_seed.hpp, the kernels in h2v_seed_dev.hpp, the mixed calls' use of it in h2v_capi.hip (mixed_seed).
#pragma once
// ---- derived seeds (H2V_RLC_SEED_TRANSCRIPT): the seed is a digest of the whole call (h2v_seed.hpp has the rule), computed on the
// device in front of the call and read there by the coefficient kernels; nothing of it is known on the host when the call returns.
// what the flags of a batch-accept call say about its seed: *derive; the flag beside a given seed is a contradiction
// (H2V_RLC_SEED_KEYED is the mixed calls' flag: a single-key call names the reason it refuses it)
static int seed_keyed_refused(const h2v_rlc_opts *o) {
    if (o && (o->flags & H2V_RLC_SEED_KEYED))
        return fail(H2V_E_ARG, "H2V_RLC_SEED_KEYED belongs to the mixed-key calls (h2v_verify_mixed / h2v_aggregate_mixed): a single-key call derives its seed with H2V_RLC_SEED_TRANSCRIPT");
    return H2V_OK;
}
static int seed_flags(const h2v_rlc_opts *o, bool *derive) {
    *derive = false;
    if (int rc = seed_keyed_refused(o)) return rc;
    *derive = o && (o->flags & H2V_RLC_SEED_TRANSCRIPT);
    if (*derive && (o->flags & H2V_RLC_SEED_GIVEN)) return fail(H2V_E_ARG, "H2V_RLC_SEED_TRANSCRIPT and H2V_RLC_SEED_GIVEN exclude each other");
    return H2V_OK;
}
// The mixed forms: form 1 stays refused - a mixed leaf needs the key tag of its own proof's plan -, and H2V_RLC_SEED_KEYED asks for
// form 3, whose leaves have it.  rlc: the call has coefficients (H2V_MIXED_RLC; an aggregate call always).
static int seed_flags_mixed(const h2v_rlc_opts *o, bool rlc = true, bool *keyed = nullptr) {
    if (keyed) *keyed = false;
    const bool want = o && (o->flags & H2V_RLC_SEED_KEYED);
    if (want && (o->flags & H2V_RLC_SEED_TRANSCRIPT)) return fail(H2V_E_ARG, "H2V_RLC_SEED_KEYED and H2V_RLC_SEED_TRANSCRIPT exclude each other (the mixed calls derive with H2V_RLC_SEED_KEYED alone)");
    if (o && (o->flags & H2V_RLC_SEED_TRANSCRIPT)) return fail(H2V_E_ARG, "H2V_RLC_SEED_TRANSCRIPT is not available in the mixed calls");
    if (!want) return H2V_OK;
    if (o->flags & H2V_RLC_SEED_GIVEN) return fail(H2V_E_ARG, "H2V_RLC_SEED_KEYED and H2V_RLC_SEED_GIVEN exclude each other");
    if (!rlc) return fail(H2V_E_ARG, "H2V_RLC_SEED_KEYED needs H2V_MIXED_RLC: a per-proof mixed call has no coefficients to derive a seed for");
    if (keyed) *keyed = true;
    return H2V_OK;
}
// One derivation: the leaf launch, one node launch per level - the last forms the seed - on `st`.  Device pointers throughout;
// digests: room for the tree's extent; form 2 (pairs): proofs holds n x 96 bytes and off, inst, ci are not read.
struct SeedJob {
    uint32_t form; uint64_t n; uint32_t inst_len, ci_len;
    const uint8_t *proofs; const uint64_t *off; const uint8_t *inst, *ci;
    const uint8_t *key_tag;      // host, 32 bytes (form 3: not read - its root hashes 32 zero bytes)
    uint32_t *digests, *seed_out;
    // form 3 (keyed leaves): the leaf launch's arguments but for tag and digests; proofs .. ci above are not read
    const SeedMixedLeafArgs *mixed = nullptr;
};
static int seed_launch(const SeedJob &j, hipStream_t st) {
    h2vseed::Tree t;
    if (!h2vseed::tree(j.n, &t) || t.levels == 0) return fail(H2V_E_ARG, "internal: no digest tree for this batch size");
    const h2vseed::TagWords leaf = h2vseed::tag_words(h2vseed::TAG_LEAF), node = h2vseed::tag_words(h2vseed::TAG_NODE), root = h2vseed::tag_words(h2vseed::TAG_ROOT);
    const bool pairs = j.form == h2vseed::FORM_PAIRS, keyed = j.form == h2vseed::FORM_MIXED;
    if (keyed) {
        if (!j.mixed) return fail(H2V_E_ARG, "internal: keyed leaves without their tables");
        SeedMixedLeafArgs ma = *j.mixed;
        ma.n = (uint32_t)j.n; ma.digests = j.digests;
        memcpy(ma.tag, h2vseed::tag_words(h2vseed::TAG_MLEAF).w, 16);
        hipLaunchKernelGGL(k_seed_leaves_mixed, dim3((uint32_t)((j.n + 63) / 64)), dim3(64), 0, st, ma);
    } else {
        SeedLeafArgs la = {(uint32_t)j.n, pairs ? 0u : j.inst_len, pairs ? 0u : j.ci_len, pairs ? 1u : 0u, j.proofs, j.off, j.inst, j.ci, {}, j.digests};
        memcpy(la.tag, leaf.w, 16);
        hipLaunchKernelGGL(k_seed_leaves, dim3((uint32_t)((j.n + 63) / 64)), dim3(64), 0, st, la);
    }
    for (uint32_t l = 1; l <= t.levels; l++) {
        SeedNodeArgs na = {l, (uint32_t)t.count[l - 1], (uint32_t)t.count[l], j.digests + t.off[l - 1] * 8, j.digests + t.off[l] * 8, {},
                           j.form, (uint32_t)j.n, (uint32_t)(j.n >> 32), {}, {}, j.seed_out};
        memcpy(na.tag, node.w, 16); memcpy(na.root_tag, root.w, 16);
        if (!keyed) memcpy(na.key_tag, j.key_tag, 32);
        hipLaunchKernelGGL(k_seed_nodes, dim3((uint32_t)((t.count[l] + 63) / 64)), dim3(64), 0, st, na);
    }
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
// THE place where a call's digest launches are queued (run_call): on `st`, into the slot of the seed ring that the call's record
// - the next one of `ws` - indexes.  The digest buffer is one per workspace: a derivation waits for the one before it, on whatever
// stream that ran (its consumers read the ring, not the buffer).  Sets u.seed_dev.
// seed_enqueue_at: the same for a job whose record is not the next one - a mixed call (mixed_seed), whose seed belongs to its LAST
// record: `slot` is that record's, j.digests / j.seed_out are filled in here, *seed_dev is the slot.
static int seed_enqueue_at(h2v_workspace *ws, hipStream_t st, uint32_t slot, SeedJob j, const uint32_t **seed_dev) {
    if (!ws->seed_ring) {
        if (!ws->mem.alloc(ws->seed_ring, wslayout::seed_ring_bytes())) return fail(H2V_E_DEVICE, "allocation of the seed ring failed");
    }
    h2vseed::Tree t;
    if (!h2vseed::tree(j.n, &t)) return fail(H2V_E_LIMIT, "derived seeds are limited to 2^22 proofs");
    if (int rc = ws->seed_digests.ensure(ws->mem, (size_t)t.extent * 32, "the seed digests", [&]() -> int {
            if (ws->ev_seed_last) HIPCHK(hipEventSynchronize(ws->ev_seed_last));
            return H2V_OK;
        })) return rc;
    for (hipEvent_t &e : ws->ev_seed[slot]) if (int rce = lazy_event(ws->mem, e, hipEventDefault)) return rce;
    if (ws->ev_seed_last) HIPCHK(hipStreamWaitEvent(st, ws->ev_seed_last, 0));
    HIPCHK(hipEventRecord(ws->ev_seed[slot][0], st));
    j.digests = (uint32_t *)ws->seed_digests.p; j.seed_out = ws->seed_ring + (size_t)slot * 8;
    if (int rc = seed_launch(j, st)) return rc;
    HIPCHK(hipEventRecord(ws->ev_seed[slot][1], st));
    ws->ev_seed_last = ws->ev_seed[slot][1];
    *seed_dev = j.seed_out;
    return H2V_OK;
}
static int seed_enqueue(Unit &u, h2v_workspace *ws, hipStream_t st) {
    const bool pairs = u.kind == UnitKind::PAIR_RLC;
    const H2vDevPlan &d = u.p->d;
    const SeedJob j = {pairs ? h2vseed::FORM_PAIRS : h2vseed::FORM_PROOFS, u.n, d.n_pi * 32u, d.n_ci * 48u, pairs ? u.pairs : u.proofs, u.off, u.inst, u.ci,
                       u.p->key_tag, nullptr, nullptr};
    u.seed_xor7 = 0;
    return seed_enqueue_at(ws, st, (uint32_t)(ws->calls % h2v_workspace::RING), j, &u.seed_dev);
}
// After the call's stream has been synchronised: the seed a call derived (calls_back as h2v_workspace_rlc_result counts them).
extern "C" int h2v_workspace_seed_used(h2v_workspace *w, uint32_t calls_back, uint8_t seed[32]) {
    if (!w || !seed) return fail(H2V_E_ARG, "null argument");
    ALIVE(w);
    const CallRec *r;
    if (int rc = rec_lookup(w, calls_back, &r)) return rc;
    if (!r->derived || !w->seed_ring) return fail(H2V_E_ARG, "that call derived no seed");
    HIPCHK(hipSetDevice(w->device));
    HIPCHK(hipMemcpy(seed, w->seed_ring + (r->call % h2v_workspace::RING) * 8, 32, hipMemcpyDeviceToHost));
    return H2V_OK;
}
// ... and the device time of its digest launches, first start to last end (HIP events on the call's stream)
extern "C" int h2v_workspace_seed_ms(h2v_workspace *w, uint32_t calls_back, float *ms) {
    if (!w || !ms) return fail(H2V_E_ARG, "null argument");
    ALIVE(w);
    const CallRec *r;
    if (int rc = rec_lookup(w, calls_back, &r)) return rc;
    if (!r->derived) return fail(H2V_E_ARG, "that call derived no seed");
    HIPCHK(hipSetDevice(w->device));
    hipEvent_t *ev = w->ev_seed[r->call % h2v_workspace::RING];
    HIPCHK(hipEventSynchronize(ev[1]));
    HIPCHK(hipEventElapsedTime(ms, ev[0], ev[1]));
    return H2V_OK;
}
