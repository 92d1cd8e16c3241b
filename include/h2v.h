/* h2v - MI355X (gfx950) batch verifier backend for Halo2/KZG proofs over BLS12-381: the C-ABI boundary.
 *
 * This library is a drop-in for ONE hot path of input-output-hk/plutus-halo2-verifier-gen: the verification the
 * reference runs on the CPU as the two-call sequence re-exported at /root/reference/src/lib.rs:9-15
 *
 *     let guard = prepare(&vk, committed_instances, instances, &mut transcript)?;     // examples/simple_mul.rs:98
 *     guard.verify(&params.verifier_params())?;                                        // examples/simple_mul.rs:101
 *
 * (in the IVC example the guard is a DualMSM with `.check(&params) -> bool`, examples/ivc.rs:85-96,195-198), and
 * that it re-states as generated Plinth/Aiken code (aiken-verifier/templates/verification_h2.hbs:21-129).
 * The reference has no FFI for this path (Rust generics over midnight-proofs); these entry points are what a
 * `extern "C"` binding of that call pair needs - see INTEGRATION.md for the Rust-side stub.
 *
 * Conventions
 *   - plain pointers and sizes only; the library never retains caller pointers past return;
 *   - scalars: 32 bytes little-endian (the transcript wire format, transcript.ak:29-45);
 *     G1: 48 bytes zcash-compressed (bls_utils.ak:17-28);
 *   - return codes: 0 = ok, negative = API misuse / device error (H2V_E_*).  A malformed or invalid PROOF is
 *     never an API error: it is accept[i] = 0, mirroring `Err(_)` => reject on the Rust side;
 *   - no CPU fallback: every verify call runs on the GPU or fails with H2V_E_DEVICE.
 */
#ifndef H2V_H
#define H2V_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define H2V_OK 0
#define H2V_E_ARG (-1)     /* null / inconsistent argument */
#define H2V_E_PLAN (-2)    /* malformed plan blob */
#define H2V_E_DEVICE (-3)  /* HIP error (no device, out of memory, launch failure) */
#define H2V_E_LIMIT (-4)   /* plan exceeds a backend limit (e.g. an MSM sum of more than H2V_MAX_MSM_TERMS terms) */

/* Widest MSM sum a plan may have: the proof's own final MSM and, with recursion, each of its sums (acc_left; acc_right plus
 * the fixed bases).  h2v_plan_load and h2v_probe_g1_msm return H2V_E_LIMIT above it, and h2v_last_error() names the sum,
 * its width and this cap.  Sums wider than one workgroup are cut into segments whose partial sums are then added. */
#define H2V_MAX_MSM_TERMS 4096u

/* per-proof status bits (h2v_verify_batch_ex / trace): 0 = accepted */
#define H2V_ST_BAD_SCALAR 1u       /* non-canonical scalar encoding in the proof */
#define H2V_ST_INVERSE_OF_ZERO 2u  /* an inversion the verifier needs hit zero (recip_eea panics, bls_utils.ak:151-154); no proof can
                                    * steer a challenge there: produced by tests/test_vm_programs_gpu.py::test_status_bits_per_lane */
#define H2V_ST_SHORT_PROOF 4u      /* fewer bytes than the plan's proof layout */
#define H2V_ST_BAD_POINT 8u        /* a G1 encoding is malformed / off-curve / not in the subgroup */
#define H2V_ST_PAIRING 16u         /* e(pi, s_g2) != e(er, G2) */
#define H2V_ST_RECURSION 32u       /* IVC: the verifying-key hash in the public inputs is not this key's (aiken.rs:696) */

typedef struct h2v_plan h2v_plan;           /* replaces VerifyingKey<F,CS> + ParamsVerifierKZG for this path */
typedef struct h2v_workspace h2v_workspace; /* reusable device scratch for batches of up to max_batch proofs */

/* One batch of independent proofs for the same plan.  Replaces the arguments of `prepare`
 * (src/lib.rs:9-15; call sites examples/simple_mul.rs:98, examples/sha256.rs:131-137):
 *   proofs      concatenated proof bytes, proof i = proofs[proof_off[i] .. proof_off[i+1])   (transcript bytes)
 *   instances   n * n_public_inputs * 32 bytes  (instances: &[&[&[F]]], one public column)
 *   committed   n * 48 bytes or NULL            (committed_instances: &[&[CS::Commitment]], 0 or 1 per proof) */
typedef struct {
    uint64_t n;
    const uint8_t *proofs;
    const uint64_t *proof_off; /* n + 1 entries */
    const uint8_t *instances;
    const uint8_t *committed;
} h2v_batch;

/* optional per-stage device timings (milliseconds, HIP events on the streams the kernels run on).  `launches` is 1 for an
 * ordinary workspace and the number of chunks for a laned one: each *_ms is the SUM of that kernel's launch durations over
 * the chunks, total_ms the span from the first launch to the last end.  msm_lanes_per_term is the shape the MSM launcher chose for the call:
 * 2 = one lane per GLV half, 1 = both halves on one lane (shared doublings), 3 = ladders for the per-proof terms beside a
 * fixed-base launch for the VK bases, 8 = a quad of lanes per GLV half (small launches of few terms: the four lanes share
 * the multiplications of every doubling and addition), 18 / 20 = two / four terms per lane (H2V_MSM_TPL). */
typedef struct {
    float transcript_combiner_ms, g1_decompress_ms, g1_msm_ms, pairing_ms, total_ms;
    uint32_t launches;
    uint32_t msm_lanes_per_term;
    uint32_t pairing_lanes_per_proof;   /* 32: two proofs per wave; 64: the wide engine (small launches); 16: the narrow one (four
                                         * proofs per wave); 12: the narrow engine packed five proofs to a wave; 6: ten proofs per wave, a whole Fp2 coefficient
                                         * per lane (Karatsuba terms: fewest instructions, for full chips); 1: the one-lane cross-check kernel */
    /* (round 3) msm_lanes_per_term == 3: the MSM ran as TWO kernels side by side - g1_msm_ms is the ladder launch over the
     * per-proof terms (its shape: msm_var_lanes_per_term, coded like msm_lanes_per_term), g1_msm_fixed_ms the fixed-base
     * launch over the VK-base terms; 0 otherwise */
    float g1_msm_fixed_ms;
    uint32_t msm_var_lanes_per_term;
} h2v_timings;

/* ---- plan (VerifyingKey) lifecycle -------------------------------------------------------------------------
 * h2v_plan_load: parse + validate the plan blob (plutus_halo2_verifier_gen_amd.plan.compile_plan(vk).to_bytes())
 * and upload it to `device`.  Immutable after load; may be shared by threads (each with its own workspace). */
int h2v_plan_load(const uint8_t *plan, size_t len, int device, h2v_plan **out);
/* (round 4) the same with load-time options (what the environment variable H2V_FIX_C used to select): opts = NULL or all-zero
 * fields = h2v_plan_load.  fixed_base_window_bits: window width of the all-window tables of the VK bases that the split MSM's
 * fixed-base launch reads - 0: the library's choice (12 bits: 22 additions per base and proof, 5 MB of tables per base; 8
 * when 12 would take more than 2 GB), or 4 / 8 / 12.  Results never depend on it. */
typedef struct {
    uint32_t fixed_base_window_bits;
    uint32_t reserved[7];   /* zero */
} h2v_plan_opts;
int h2v_plan_load_ex(const uint8_t *plan, size_t len, int device, const h2v_plan_opts *opts, h2v_plan **out);
/* (round 3) The plan compiler behind the boundary: a verifying-key description - the JSON form frozen as docs/vk_schema.json
 * ("h2v-vk/1": what `extract_circuit` reads out of a midnight_proofs VerifyingKey + ParamsVerifierKZG,
 * /root/reference/src/plutus_gen/extraction/mod.rs:31-232, instantiation_data.rs:26-41; the serde exporter is in
 * INTEGRATION.md) - to the blob h2v_plan_load takes.  Host-only (no GPU needed), byte-identical with
 * plutus_halo2_verifier_gen_amd.plan.compile_plan(vk).to_bytes().  *blob_out is malloc'ed: release it with h2v_blob_free.
 * A description the reference itself could not emit a verifier for (Selector / Instance / Challenge nodes, a permutation
 * column without a query at the current rotation, commitments that are not G1 points ...) is H2V_E_ARG with the reason in
 * h2v_last_error(). */
int h2v_plan_compile(const char *vk_json, size_t len, uint8_t **blob_out, size_t *blob_len);
void h2v_blob_free(uint8_t *blob);
void h2v_plan_free(h2v_plan *plan);
/* plan facts: proof length in bytes, public inputs per proof, committed instances per proof (0/1), MSM terms T */
int h2v_plan_info(const h2v_plan *plan, uint32_t *proof_len, uint32_t *n_public_inputs, uint32_t *n_committed,
                  uint32_t *n_msm_terms);
/* The transcript hash of the plan's key: the H of the reference's CircuitTranscript<H>.  It is a property of the verifying
 * key (docs/vk_schema.json: transcript_hash), carried by the plan and read by the launcher; callers never pass it per call.
 *   H2V_TRANSCRIPT_CARDANO_BLAKE2B_256  CardanoFriendlyBlake2b (src/plutus_gen/adjusted_types/mod.rs:30-72): unkeyed
 *                                       blake2b-256, a challenge is h || blake2b-256(h).  Plans without the field (version 4).
 *   H2V_TRANSCRIPT_BLAKE2B_512          halo2's default blake2b_simd::State: blake2b with a 64-byte digest, keyed with a
 *                                       domain-separator key of up to 64 bytes; a challenge is the 64-byte digest of a copy of
 *                                       the running state.  Such plans are version 5: an older library refuses them.
 * *kind: one of the above; key_out: the blake2b key, zero-padded to 64 bytes; *key_len: its length (0 for the Cardano kind).
 * Any of the three may be NULL.
 * A proof made under ANOTHER hash than the plan's is not an API error: it replays to other challenges, its pairing equation
 * fails and it is REJECTED with H2V_ST_PAIRING, like any proof that does not verify under this key. */
#define H2V_TRANSCRIPT_CARDANO_BLAKE2B_256 0u
#define H2V_TRANSCRIPT_BLAKE2B_512 1u
int h2v_plan_transcript(const h2v_plan *plan, uint32_t *kind, uint8_t key_out[64], uint32_t *key_len);
/* 1 if the two plans carry the same SRS (the same s_g2: what h2v_verify_mixed demands of the plans of one call), 0 if not;
 * H2V_E_ARG for a null plan.  Host-only: needs no device. */
int h2v_plan_same_srs(const h2v_plan *a, const h2v_plan *b);
/* key_tag = blake2b-256(TAG("h2v-seed-key/1") || plan blob), computed at load: what a derived batch seed (H2V_RLC_SEED_TRANSCRIPT)
 * binds the verifying key with.  Host-only. */
int h2v_plan_key_tag(const h2v_plan *plan, uint8_t out[32]);

/* A workspace is sized from `plan` (MSM terms, point slots, register file, recursion / fixed-base buffers).  It may be
 * reused with ANOTHER plan only if that plan needs no more of any of these; otherwise the verify calls return H2V_E_ARG
 * (they never write past a buffer).  One workspace serves one call at a time. */
int h2v_workspace_create(const h2v_plan *plan, uint64_t max_batch, h2v_workspace **out);
void h2v_workspace_free(h2v_workspace *ws);
/* (round 3) LANES: the pipelining that callers used to build from several workspaces and streams, inside the library.
 * A laned workspace owns n_lanes sub-workspaces of `chunk` proofs each, every one with its own library-owned stream.  A verify
 * call on it (device-resident, host-buffer or RLC form, any n <= max_batch) is cut into chunks of at most `chunk` proofs
 * that go round robin through the lanes, so that the decompression / combiner kernels of one chunk run beside the MSM and
 * pairing kernels of others; accept[] / status[] are written in place, chunk by chunk, and the caller's stream waits for
 * the last one (unless joins are deferred, below).  Device memory is n_lanes x chunk proofs' worth, whatever max_batch is.
 * Verdicts never depend on n_lanes or chunk (tests/test_gpu_parity.py::test_verdicts_do_not_depend_on_the_chunking); in
 * RLC mode every chunk is its own batch check with coefficients of its own: chunk c draws r_i from i = the position within the
 * chunk, under the call's seed with 0x9e3779b9 * (c + 1) xored into its last 32-bit word (the one chunk of a call that fits a
 * chunk is chunk 0 and carries that tweak too; an ordinary workspace hashes the call's seed as it is).
 *   n_lanes = 0 / chunk = 0: the library's choice (chunk = 4096 proofs whatever the plan and whatever max_batch - the largest
 *   single call - is: small calls are gathered into the lanes, COALESCING below; 16 lanes, of which the per-proof mode cycles
 *   through 8 - all 16 for launches too small to fill the chip: h2v_workspace_depth).  An explicit chunk is cut to max_batch.
 *   h2v_workspace_create(plan, max_batch) itself returns a laned workspace when max_batch >= 4 x the batch that gives every kernel
 *   of the plan one wave per SIMD (4096 proofs for 16 MSM terms, 1024 for 60; an ordinary workspace below that).  n_lanes <= 16: that is also the
 *   most host batches h2v_verify_batch_submit keeps in flight on one workspace (h2v::BatchStream / backend.BatchStream: depth
 *   <= 16).  A laned workspace has no trace buffer (h2v_trace creates its own). */
int h2v_workspace_create_lanes(const h2v_plan *plan, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk, h2v_workspace **out);
/* One laned workspace for SEVERAL plans of one device - a node that verifies proofs of several circuits (BASELINE configs[2]: a
 * mixed batch of two circuits).  The lanes are sized for the largest of every dimension of the listed plans (a workspace
 * accepts any plan whose dimensions fit its buffers), so the calls of all of them - each names its plan as usual - go round
 * robin through ONE set of lanes and streams; with one laned workspace per plan the lanes of the two share the pool's sixteen
 * streams pairwise.  chunk = 0: the smallest of the plans' own chunks.  Everything else as h2v_workspace_create_lanes; options
 * (h2v_workspace_set_option, h2v_workspace_tune) hold for the workspace, i.e. for every plan on it.  The RLC mode keeps one set
 * of its buffers per plan shape on such a workspace (up to eight).  The reference has no counterpart: its verifier objects
 * are per proof (src/lib.rs:9-15) and a mixed batch is a Vec of (vk, proof) pairs. */
int h2v_workspace_create_multi(const h2v_plan *const *plans, uint32_t n_plans, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk,
                               h2v_workspace **out);
/* Deferred joins (laned workspaces): with defer = 1 a device-resident verify call returns without making the caller's stream
 * wait for its chunks, so the chunks of CONSECUTIVE calls overlap in the lanes - one workspace then does what five
 * workspaces on five streams did (a stream of batches: DESIGN.md section 6).  The inputs of a call must stay untouched, and
 * its accept[] / status[] unread, until h2v_workspace_join(ws, stream) has been called and `stream` has reached that point
 * (stream = NULL: the HOST blocks until every chunk submitted so far is done; nothing is enqueued on the NULL stream).  Calls
 * still start in submission order, each after whatever was enqueued on its `stream` argument before it.
 * THE NULL STREAM (round 4).  The lanes run on library-owned streams with hardware queues of their own
 * (hipExtStreamCreateWithCUMask), and those have the default flags: they are BLOCKING streams, ordered with the legacy NULL
 * stream.  Any work a host puts on the NULL stream - PyTorch's default stream is that stream - waits for every lane and holds
 * every lane back behind it, so the overlap of consecutive calls would be lost without an error.  Therefore, on a workspace
 * with deferred joins, h2v_verify_batch_device / h2v_verify_batch_rlc_device return H2V_E_ARG for stream = NULL: give the
 * calls a stream of their own (hipStreamCreateWithFlags(.., hipStreamNonBlocking); torch.cuda.Stream()) and keep other NULL-
 * stream work (synchronous hipMemcpy included) out of the submission loop.  Without deferred joins NULL is accepted: every
 * call then waits for its own chunks anyway.  tests/test_gpu_parity.py::test_null_stream_contract_of_deferred_joins. */
/* COALESCING (round 4).  With deferred joins a device-resident call (per proof or RLC) of at most HALF the workspace's chunk is not
 * launched by itself: its proofs are gathered - at once, behind whatever its `stream` held at the time of the call - behind
 * those of the small calls before it, and the kernels run ONCE over the group: when the next call would not fit the chunk, when
 * a call of another plan or another kind (large, RLC, host-buffer, tune) arrives, or at h2v_workspace_join.  Nothing changes for
 * the caller beyond what deferred joins already say - inputs untouched and accept[] / status[] unread until the join - but a
 * stream of 64-proof calls costs a 1024-proof launch per sixteen of them instead of sixteen chains of lone waves (the per-GPU
 * shares of a batch cut over eight GPUs: DESIGN.md section 6.1).  Verdicts do not depend on it.  h2v_workspace_timings of such
 * a call reports its share of the group's launch.  RLC calls are gathered among themselves: ONE batch check over the group.  Its
 * coefficients: the SEED is that of the call that opened the group - the OS's draw for that call, or its given seed with the call
 * count that call mixed in; every later call of the group still draws a seed (a given one ticks the count), which is not used -
 * and the POSITION of a proof is counted through the group: the number of proofs gathered before its call plus its index within
 * the call (no chunk tweak: a group is one piece).  So no two proofs of a group share a coefficient, whichever calls they came in
 * (tests/test_batch_cancellation_gpu.py::test_coalesced_rlc_group).  accept[] stays per proof and exact, h2v_workspace_rlc_result of each call reports the
 * GROUP's batch verdict (a rejecting proof of a neighbouring call fails the check for all of them) and the call's share of the
 * times.  An open group does not start by itself: a caller that stops submitting for a while and wants the GPU to get on with
 * what it has calls h2v_workspace_join(ws, stream) with a stream of its own - that runs the open groups and does not block the
 * host.  A workspace keeps one group open per plan and mode (at most four, and fewer than it has lanes).  Host-buffer calls
 * (h2v_verify_batch, _submit) are not gathered: a host that collects small batches concatenates them itself.
 * H2V_OPT_COALESCE = -1 switches it off for a workspace. */
int h2v_workspace_defer_joins(h2v_workspace *ws, int defer);
int h2v_workspace_join(h2v_workspace *ws, void *stream);
/* Launch-shape options of a workspace (round 3: what used to be reachable through environment variables only; results never
 * depend on them - tests/test_gpu_parity.py::test_workspace_options_change_the_shape_not_the_verdicts).  value 0 = the
 * launcher's own choice (DESIGN.md sections 4.1, 4.2, 6). */
#define H2V_OPT_MSM_TERMS_PER_LANE 1u /* per-proof MSM: 1 .. 4 terms per lane on one accumulator (shared doublings) */
#define H2V_OPT_PAIRING_ENGINE 2u     /* lanes per proof of the pairing kernel: 6 (ten proofs per wave), 12 (five), 16 (narrow: four), 32, 64 (wide), 1 (the one-lane cross-check kernel) */
#define H2V_OPT_STREAMS 3u            /* -1 auto, 0: two library streams per call, 1: everything on the caller's stream, 2: + one side stream */
/* (round 4) every remaining shape dimension, formerly H2V_* environment variables read once per process: */
#define H2V_OPT_MSM_LANES_PER_TERM 4u /* ladder launches: 1 (both GLV halves on one lane), 2 (one lane per half), 8 (a quad of lanes per half) */
#define H2V_OPT_MSM_BLOCK_SIZE 5u     /* threads per block of the MSM launches: 64 .. 512 in steps of 64 */
#define H2V_OPT_MSM_FIXED_SPLIT 6u    /* VK-base terms through the all-window tables beside the ladders: 1 .. 4 bases per lane; -1: never split */
#define H2V_OPT_COMBINER_SCHEDULE 7u  /* transcript + combiner kernel: 1 the plan's narrow bundle schedule, 2 the wide one */
#define H2V_OPT_COMBINER_PROOFS_PER_BLOCK 8u /* proofs per one-wave block of that kernel (a power of two <= what fits LDS) */
/* ids 9 and 10 are retired (forms of the decompression launch, sub-pipelines): not reused, refused with H2V_E_ARG */
#define H2V_OPT_RLC_GROUP_STAGE 11u   /* RLC fall-back: -1 skips the group checks (straight to the per-proof kernels) */
#define H2V_OPT_RLC_WINDOW_BITS 12u   /* bucket MSM: window width */
#define H2V_OPT_RLC_CHAIN 13u         /* bucket MSM: most entries one lane sums */
#define H2V_OPT_RLC_ROUTE 14u         /* RLC calls are routed by the observed rate of failing groups (h2v_verify_batch_rlc below); -1: always the batch check first */
#define H2V_OPT_COALESCE 15u          /* small device-resident calls on a deferring laned workspace are gathered into one launch per kernel (h2v_workspace_defer_joins below); -1: never */
#define H2V_OPT_COUNT 16u
int h2v_workspace_set_option(h2v_workspace *ws, uint32_t option, int32_t value);
int h2v_workspace_get_option(const h2v_workspace *ws, uint32_t option, int32_t *value);
/* (round 4) MEASURED launch shapes.  The launcher's own rules are thresholds calibrated on five circuit shapes; a circuit or a
 * batch size in between gets the nearest rule, unmeasured.  h2v_workspace_tune runs `batch` (device-resident, as for
 * h2v_verify_batch_device; its verdicts are discarded) repeatedly in the way the workspace is used - a laned workspace with as
 * many calls in flight as it has lanes for that size, an ordinary one call by call -, times the launcher's choice and its
 * neighbours (pairing engine, then MSM terms per lane: <= 8 measurements of three rounds of the lanes or ~120 ms each, whichever
 * is longer - about a second in all), and leaves the fastest on
 * the workspace as H2V_OPT_PAIRING_ENGINE / H2V_OPT_MSM_TERMS_PER_LANE (0 = the launcher's rule stays: a candidate must be
 * 3 % faster to replace it).  Call it once per (plan, batch size, workspace) at start-up, on `stream` (not NULL for a laned
 * workspace); it returns when the measurements are done.  flags: 0.  Results of later calls do not depend on it. */
typedef struct {
    uint32_t n_measured;          /* configurations timed */
    uint32_t calls_in_flight;     /* how the batch was run: calls kept in flight */
    float default_ms, best_ms;    /* ms per call: the launcher's own choice / the configuration now set */
    int32_t pairing_engine;       /* H2V_OPT_PAIRING_ENGINE now set (0: the launcher's rule) */
    int32_t msm_terms_per_lane;   /* H2V_OPT_MSM_TERMS_PER_LANE now set (0: the launcher's rule) */
    uint32_t reserved[4];
} h2v_tune_report;
int h2v_workspace_tune(const h2v_plan *plan, const h2v_batch *batch, h2v_workspace *ws, void *stream, uint32_t flags,
                       h2v_tune_report *report /* or NULL */);
/* the same options for the h2v_probe_* calls of the calling thread (they have no workspace) */
int h2v_probe_set_option(uint32_t option, int32_t value);
/* lanes and chunk size of a workspace (1 lane = not laned) */
int h2v_workspace_lanes(const h2v_workspace *ws, uint32_t *n_lanes, uint32_t *chunk);
/* how many calls of n proofs each (rlc != 0: RLC mode) the workspace keeps in flight before a call has to wait for a lane:
 * the lanes that mode cycles through for chunks of that size (1 for a workspace that is not laned).  Per-proof mode: 8 lanes
 * with the decompression on a side stream, or - chunks that give the MSM at most half a wave per SIMD - all 16, each
 * chunk on its lane's stream alone; RLC mode: all of them. */
int h2v_workspace_depth(const h2v_workspace *ws, uint64_t n, int rlc, uint32_t *batches_in_flight);
/* (new) Tuning hint: the caller keeps n_in_flight batches in flight on this device (each on its own workspace).  From 4 up
 * the launcher prefers shapes that issue fewer instructions over shapes with shorter dependent chains (per-proof MSM: two
 * terms per lane on one accumulator; the narrow pairing engine from 2 x #SIMDs proofs; from 6 the whole per-proof pipeline on
 * the caller's stream; RLC mode: from 3 the one-stream form, as with H2V_RLC_ONE_STREAM; from 8 the thresholds of a chip that
 * is full whatever one launch brings: DESIGN.md section 6.1).  Results do not depend on it.  Default 1.  A LANED workspace
 * estimates it per call by itself - all its lanes when joins are deferred or host batches are streamed, otherwise the number
 * of chunks of the call - unless this function was called: then the given value holds. */
int h2v_workspace_hint_in_flight(h2v_workspace *ws, uint32_t n_in_flight);
/* Per-kernel device times of a past call that used `ws` (calls_back = 0: the most recent; up to 63 back), from HIP
 * events recorded on the streams the kernels ran on.  Synchronise the launch stream before asking.  EVERY call on a workspace
 * takes one record - verify, prepare, check and RLC calls alike, on ordinary and laned workspaces - and calls_back counts them
 * all.  H2V_E_ARG: no such record (64 or more back; on a laned workspace also when a lane has made 64 calls since, "rings have
 * wrapped"), an RLC call that ran its batch check (h2v_workspace_rlc_result has its times; a call routed to the per-proof
 * kernels has its per-proof times here), or a coalesced call whose group has not run yet. */
int h2v_workspace_timings(h2v_workspace *ws, uint32_t calls_back, h2v_timings *out);

/* ---- verification (replaces prepare + Guard::verify / DualMSM::check) --------------------------------------
 * Host-buffer form: copies the batch to the device, verifies, copies accept[] (n bytes, 1 = accept) back.
 * ws may be NULL (a temporary workspace is created for the call). */
int h2v_verify_batch(const h2v_plan *plan, const h2v_batch *batch, uint8_t *accept, h2v_workspace *ws);

/* Asynchronous host-buffer form, for callers that stream batches: _submit copies the caller's buffers into pinned staging
 * memory of `ws` (they may be reused at once), enqueues ONE upload, the verification (per proof, or the RLC batch mode with
 * H2V_SUBMIT_RLC - see below) and the download of accept[] on the workspace's own stream, and returns; _wait blocks until
 * that batch is done and copies its accept bytes out.  An ordinary workspace holds one batch at a time (alternate two and
 * the upload of batch k+1 runs beside the kernels of batch k); a LANED workspace (h2v_workspace_create_lanes) holds as many as
 * the mode has lanes - every batch gets a staging slot of its own - and _wait collects the OLDEST: one workspace is a
 * whole stream of host batches.  h2v_verify_batch is _submit + _wait. */
#define H2V_SUBMIT_RLC 1u
struct h2v_rlc_opts_s;
int h2v_verify_batch_submit(const h2v_plan *plan, const h2v_batch *batch, h2v_workspace *ws, uint32_t flags,
                            const struct h2v_rlc_opts_s *rlc_opts /* or NULL */);
int h2v_verify_batch_wait(h2v_workspace *ws, uint8_t *accept, int *fell_back /* or NULL */);

/* Device-resident form: every pointer in `batch` and `accept`/`status` are DEVICE pointers on the plan's device
 * (e.g. torch tensors' data_ptr()); work is enqueued on `stream` (a hipStream_t, NULL = default stream) and the
 * call returns after enqueueing unless `timings` is given (then it synchronises to read the events).
 * status (n x uint32, may be NULL) receives the H2V_ST_* bits. */
int h2v_verify_batch_device(const h2v_plan *plan, const h2v_batch *batch, uint8_t *accept, uint32_t *status,
                            h2v_workspace *ws, void *stream, h2v_timings *timings);

/* ---- batch-accept fast path: random linear combination (RLC) of the batch's pairing equations -------------------
 * Same inputs and the same accept[] / status[] outputs as h2v_verify_batch(_device).  Instead of one MSM and one pairing
 * per proof, the batch is folded with 128-bit coefficients r_i (blake2b-256(seed || i), seed from the OS unless given)
 * into ONE check  e(sum_i r_i pi_i, s_g2) == e(sum_i r_i er_i, G2)  - the dual-MSM form of
 * aiken-verifier/aiken_halo2/lib/halo2_kzg.ak:37-43 and the pairing equation of verification_h2.hbs:125-128 summed over
 * the batch - computed by a bucketed (Pippenger) G1 MSM over every per-proof point of the batch.  Proofs that are rejected
 * before the pairing (malformed encodings, points off the curve or outside G1, inverse of zero ...) are rejected
 * individually and take no part in the combination.  If the batch check fails, the per-proof MSM and pairing kernels run
 * for the whole batch, so accept[] is always what the per-proof mode returns, except with probability <= 2^-128 over the
 * seed (a rejecting proof hidden by the combination).  Recursive (IVC) plans run per proof unless H2V_RLC_FOLD_PAIRS is set.
 * ws must not be NULL for the device form.
 * ROUTING (round 4): a failed batch check costs more than the per-proof mode it falls back to, so a workspace keeps a running
 * estimate of the rate of FAILING GROUPS (64 proofs each) among the groups its RLC calls have met, and while that rate is
 * above 0.10 it sends RLC calls straight to the per-proof kernels (back to the batch check below 0.05; the estimate moves a
 * quarter of the way per call: one rejecting proof per batch - one group in 64 - never switches, a batch in which half the
 * groups fail switches the next call, and some ten clean calls switch back).  accept[] is the same either way;
 * fell_back = 1 / batch_accepted = 0 say that the per-proof kernels produced it.  H2V_OPT_RLC_ROUTE = -1 switches routing off. */
#define H2V_RLC_SEED_GIVEN 1u /* TEST ONLY: soundness rests on the seed being unpredictable to the provers; without this flag
                               * the library draws 32 bytes from the OS per call (getrandom) and fails closed.  With it, a
                               * process-wide call counter is still mixed into the seed, so repeated calls differ: the count of
                               * seeded calls of EVERY form so far (RLC, pair check, mixed), xored into seed words 5 (low) and 6. */
#define H2V_RLC_ONE_STREAM 2u /* everything on the caller's stream (decompression before the combiner instead of beside it):
                               * 0.3 ms more per batch alone, but one stream per batch for callers that keep many batches in
                               * flight - more of them fit the hardware queues (measured: 2.47 M proofs/s with 7 in flight
                               * against 2.24 M with 5 on two streams each) */
#define H2V_RLC_FOLD_PAIRS 4u /* recursive (IVC) plans only, ignored on any other: the batch form that starts AFTER the fold.  The
                               * per-proof pipeline runs up to and including the fold (its challenge hashes each proof's own MSM
                               * result, so nothing before it can be combined); then every proof is a pair (el', er') like any
                               * other, and the pairs are checked as h2v_check_pairs_rlc checks pairs: ONE pairing for the batch,
                               * and after a failed check the per-proof pairing on the folded points (no MSM is repeated).
                               * accept[] / status[] are the per-proof mode's.  Never routed, never coalesced. */
#define H2V_RLC_GROUPED 16u   /* h2v_aggregate_mixed(_device) only: the H2V_MIXED_GROUPED form of the call (below) - same pair, same
                               * included[], same info; up to H2V_MIXED_GROUPED_MAX_PLANS plans.  H2V_E_ARG in any other aggregate call.
                               * (Bit 8 stays unassigned: the aggregate calls have always answered H2V_E_ARG to it, and callers
                               * and tests rely on that.) */
/* DERIVED SEED (Fiat-Shamir).  With this flag nothing is drawn: the call's seed is a blake2b-256 digest of everything that
 * determines the batch - the plan (key_tag = B(TAG("h2v-seed-key/1") || plan blob), h2v_plan_key_tag), the form, n, and per proof
 * the lengths and bytes of its instance row, committed row and proof - computed on the device in front of the call, over the WHOLE
 * call (a laned workspace tweaks it per chunk as it tweaks any seed).  B: unkeyed blake2b-256; TAG(s): s zero-padded to 16 bytes:
 *   leaf_i = B(TAG("h2v-seed-leaf/1") || LE32(|inst_i|) || LE32(|ci_i|) || LE32(|proof_i|) || LE32(0) || inst_i || ci_i || proof_i)
 *            (h2v_check_pairs_rlc: |inst| = |ci| = 0, proof_i = the 96 pair bytes)
 *   node   = B(TAG("h2v-seed-node/1") || LE32(level) || LE32(m) || LE64(index in its level) || child_0 .. child_{m-1}), 64-ary,
 *            level 1 over the leaves, levels added until one node is left (n = 1: one level-1 node)
 *   seed   = B(TAG("h2v-seed-root/1") || LE32(form: 1 proofs, 2 pairs) || LE32(0) || LE64(n) || key_tag || top node)
 * and the coefficients follow from the seed as from any other.  plutus_halo2_verifier_gen_amd/seed.py restates the rule with
 * hashlib: whoever holds the same key, the same inputs and the same chunk size recomputes the same seed and the same pair.
 * CLAIM: sound in the random-oracle model for blake2b - a prover making q hash evaluations gets a rejecting proof accepted with
 * probability at most q / 2^128 (2^-128 flat with a secret seed); nothing has to be kept from the provers.  It is still not a
 * succinct proof for someone without the inputs.
 * Accepted by h2v_verify_batch_rlc(_device), h2v_verify_batch_submit with H2V_SUBMIT_RLC, h2v_check_pairs_rlc(_device) and
 * h2v_aggregate_batch(_device) (recursive plans: on their fold-pairs route - the leaf binds the inputs, which determine the folded
 * pairs).  H2V_E_ARG: together with H2V_RLC_SEED_GIVEN; in h2v_verify_mixed(_device) / h2v_aggregate_mixed(_device) - a mixed leaf
 * needs the key tag of its own proof's plan: the mixed calls take H2V_RLC_SEED_KEYED (below) instead.  A call with the flag is never coalesced; it is routed as ever, and a
 * call that routing sends to the per-proof kernels derives nothing.  DESIGN.md section 17. */
#define H2V_RLC_SEED_TRANSCRIPT 32u
/* DERIVED SEED OF A MIXED-KEY CALL: form 3, "keyed leaves" (frozen).  As above, but every leaf binds the key of its own proof and
 * the root binds no key:
 *   mleaf_i = B(TAG("h2v-seed-mleaf/1") || LE32(|inst_i|) || LE32(|ci_i|) || LE32(|proof_i|) || LE32(0)
 *               || key_tag(plans[plan_of[i]]) || inst_i || ci_i || proof_i)
 *   seed    = B(TAG("h2v-seed-root/1") || LE32(3) || LE32(0) || LE64(n) || 32 zero bytes || top node)
 * B, TAG, node and the 64-ary tree as above.  The tag string is exactly 16 bytes, the leaf header 64.  Leaves enter in the CALLER's
 * order - the position the coefficients are drawn from; inst_i: the proof's own 32 n_pi(plan) bytes; ci_i: its 48 committed bytes,
 * or empty for a plan without a committed instance; proof_i: proofs[proof_off[i] .. proof_off[i + 1]) AS GIVEN, short or long (never
 * the copy the grouping kernels cut to proof_len); a descending pair of offsets is an empty proof.  So the seed does not depend on
 * the order in which the plans are listed, on listed plans without a proof, or on the call's other flags - the RLC, fold and
 * grouped forms, verify and aggregate, share ONE seed on the same batch (the fold form's fall-back reuses the words of its first
 * pass) - and it does depend on which key every position has.  A one-plan mixed call does NOT share its seed with the single-key
 * form 1 call on the same bytes.  Behind the seed nothing changes: r_i = low 128 bits of B(seed' || LE32(pos)); the H2V_MIXED_RLC
 * tail on a laned workspace tweaks word 7 per chunk by 0x9e3779b9 (c + 1); the fold tail is one piece.
 * Accepted by h2v_verify_mixed(_device) with H2V_MIXED_RLC (with or without _FOLD_MSM and _GROUPED) and by
 * h2v_aggregate_mixed(_device) (with or without H2V_RLC_GROUPED; H2V_AGGREGATE_SEED_SOURCE(info) = 1), recursive plans included
 * (they join as one pair per proof).  H2V_E_ARG: beside H2V_RLC_SEED_GIVEN or H2V_RLC_SEED_TRANSCRIPT; in a mixed call without
 * H2V_MIXED_RLC; in every single-key entry point.  n > 2^22: H2V_E_LIMIT; n = 0 derives nothing.  h2v_workspace_seed_used / _seed_ms
 * (calls_back = 0) answer for the call's last record, fallen back or not.  seed.py: mixed_seed.  DESIGN.md section 17.1. */
#define H2V_RLC_SEED_KEYED 64u
typedef struct h2v_rlc_opts_s {
    uint8_t seed[32];   /* used when flags & H2V_RLC_SEED_GIVEN (tests, reproducible measurements - never a service) */
    uint32_t flags;
} h2v_rlc_opts;
typedef struct {
    float transcript_combiner_ms, g1_decompress_ms, prepare_ms, bucket_sort_ms, bucket_accumulate_ms, bucket_reduce_ms,
          pairing_ms, total_ms;   /* total: first phase-1 launch .. the batch verdict (a fall-back run is not included) */
    uint32_t msm_terms, window_bits, windows, max_chain;   /* shape of the right-hand bucket MSM; max_chain: entries per lane */
} h2v_rlc_timings;
int h2v_verify_batch_rlc(const h2v_plan *plan, const h2v_batch *batch, uint8_t *accept, h2v_workspace *ws,
                         const h2v_rlc_opts *opts /* or NULL */, int *fell_back /* or NULL: 1 = the per-proof kernels ran */);
int h2v_verify_batch_rlc_device(const h2v_plan *plan, const h2v_batch *batch, uint8_t *accept, uint32_t *status,
                                h2v_workspace *ws, void *stream, const h2v_rlc_opts *opts /* or NULL */);
/* after synchronising the stream of an RLC call: the batch verdict (1 = passed) and the kernel times of that call.  calls_back
 * counts the workspace's records as h2v_workspace_timings does (every call takes one; up to 63 back).  A call routed to the
 * per-proof kernels reports (0, zeros); an aggregate call (h2v_aggregate_batch / _mixed, below) reports batch_accepted =
 * H2V_BATCH_NOT_CHECKED and pairing_ms = 0.  H2V_E_ARG: no such record or a lane's ring has wrapped since (as there), a call that
 * was not an RLC call, or a coalesced call whose group has not run yet. */
int h2v_workspace_rlc_result(h2v_workspace *ws, uint32_t calls_back, uint32_t *batch_accepted, h2v_rlc_timings *timings);
/* after synchronising the stream of a call made with H2V_RLC_SEED_TRANSCRIPT: the 32 bytes of the seed it derived (the call's
 * seed: a laned workspace's chunk tweaks are not in it).  calls_back as above.  H2V_E_ARG: no such record, or a call that derived
 * nothing (no flag, or routed to the per-proof kernels).  h2v_workspace_seed_ms: the device time of that call's digest launches,
 * first start to last end (HIP events on the call's stream); the same errors. */
int h2v_workspace_seed_used(h2v_workspace *ws, uint32_t calls_back, uint8_t seed[32]);
int h2v_workspace_seed_ms(h2v_workspace *ws, uint32_t calls_back, float *ms);

/* ---- prepare and pair check (the two halves of verification: the reference's `prepare` -> DualMSM -> `check`) -----------
 * h2v_prepare_batch(_device) runs the verify pipeline up to the final pairing check  e(L, s_g2) == e(R, G2)  and returns the
 * two points of every proof instead of checking them:
 *   pairs[96 i .. 96 i + 96) = compress(L) || compress(R), each 48-byte zcash compressed (as bls12_381.g1_compress);
 *   accept[i] of h2v_verify_batch == (status[i] == 0 && e(L, s_g2) == e(R, G2)).
 * L, R are exactly the points the pairing kernels use (the oracle's `el` / `er`): non-recursive keys L = the proof's pi
 * commitment and R = the multi-open MSM (the collapsed DualMSM, aiken_halo2/lib/halo2_kzg.ak:10-12); recursive (IVC) keys
 * the folded pair el' = el + c acc_left, er' = er + c acc_right_final.  status[i] (n x uint32, may be NULL) is what the
 * verify call reports with H2V_ST_PAIRING cleared (H2V_ST_RECURSION stays).  A proof rejected before the pairing
 * (status[i] != 0) gets 96 ZERO bytes: not a valid encoding (compression flag unset), so h2v_check_pairs rejects it with
 * H2V_ST_BAD_POINT - never (inf, inf), which would pass the pairing.
 * h2v_check_pairs(_device) checks n such pairs from anywhere: accept[i] (n bytes) = e(L_i, s_g2 of plan) == e(R_i, G2).  Both
 * points are decoded with the rules verify applies to proof points (flags, canonical x, on the curve, in G1, infinity
 * allowed); otherwise status[i] = H2V_ST_BAD_POINT; a failed equation sets H2V_ST_PAIRING.
 * Arguments and error codes as h2v_verify_batch(_device): the workspace must fit the plan (a workspace for max_batch proofs
 * takes up to max_batch pairs), no host batch may be in flight on it, and under deferred joins the device forms refuse
 * stream = NULL.  The device forms enqueue on `stream` and return (device pointers; pairs of the prepare form 4-byte
 * aligned); the host forms return when the outputs are written.  ws = NULL: a temporary workspace.  A laned workspace cuts
 * the call into chunks across its lanes as for verify (pairs offset by 96 bytes per proof); prepare and check calls are
 * never gathered into coalesced groups, and their arrival runs the open groups first.  h2v_workspace_timings of a prepare
 * call reports pairing_ms = 0. */
int h2v_prepare_batch(const h2v_plan *plan, const h2v_batch *batch, uint8_t *pairs /* n*96 */, uint32_t *status /* or NULL */,
                      h2v_workspace *ws /* or NULL */);
int h2v_prepare_batch_device(const h2v_plan *plan, const h2v_batch *batch, uint8_t *pairs, uint32_t *status, h2v_workspace *ws,
                             void *stream);
int h2v_check_pairs(const h2v_plan *plan, uint64_t n, const uint8_t *pairs /* n*96 */, uint8_t *accept, uint32_t *status /* or NULL */,
                    h2v_workspace *ws /* or NULL */);
int h2v_check_pairs_device(const h2v_plan *plan, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status,
                           h2v_workspace *ws, void *stream);
/* h2v_check_pairs_rlc(_device): h2v_check_pairs's contract - the same decoding of both points (the subgroup test stays per
 * point), the same accept[] / status[] - with the batch check deciding only which kernels produce them: the reference's "scale
 * each DualMSM by a random coefficient, add, check once".  L = sum r_i L_i and R = sum r_i R_i over the pairs that decoded
 * (r_i = low 128 bits of blake2b-256(seed || LE32(i)), never 0; an undecodable pair gets H2V_ST_BAD_POINT, accept 0 and
 * coefficient 0) are two bucket MSMs, followed by ONE pairing.  Passed: accept[i] = "decoded".  Failed: checks of groups of
 * 64 pairs and then the per-pair kernels of h2v_check_pairs run behind it on the device and set H2V_ST_PAIRING on the pairs
 * whose own equation fails; nothing comes back to the host in between.  Soundness <= 2^-128 over the seed, completeness exact;
 * (inf, inf) pairs pass, and so does a batch whose participating pairs sum to infinity on both sides (an empty one included).
 * The seed follows h2v_verify_batch_rlc's rules; H2V_RLC_ONE_STREAM is accepted and means nothing (one stream already).
 * Workspaces as for h2v_check_pairs; a laned one makes every chunk its own check.  The device form needs a workspace.  The call
 * takes one record of kind RLC: h2v_workspace_rlc_result reports its verdict and times (g1_decompress_ms: the decoding,
 * transcript_combiner_ms: 0, prepare_ms: the coefficient kernel, msm_terms: n), h2v_workspace_timings refuses it.  Never
 * routed, never coalesced, and the workspace's failing-group estimate does not move.  n > 2^22: H2V_E_LIMIT. */
int h2v_check_pairs_rlc(const h2v_plan *plan, uint64_t n, const uint8_t *pairs /* n*96 */, uint8_t *accept, uint32_t *status /* or NULL */,
                        h2v_workspace *ws /* or NULL */, const h2v_rlc_opts *opts /* or NULL */, int *fell_back /* or NULL */);
int h2v_check_pairs_rlc_device(const h2v_plan *plan, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status,
                               h2v_workspace *ws /* not NULL */, void *stream, const h2v_rlc_opts *opts /* or NULL */);
/* h2v_check_pairs_multi(_device): ONE batch check over pairs on SEVERAL SRS.  The pairs come grouped in ranges: the first
 * counts[0] pairs are checked against the SRS (s_g2) of plans[0], the next counts[1] against plans[1], and so on.  accept[] and
 * status[] are, position for position, what h2v_check_pairs(plans[k], ...) returns for range k alone - the same decoding,
 * H2V_ST_BAD_POINT for an undecodable pair (coefficient 0), H2V_ST_PAIRING for a failed equation -; the batch check only decides
 * which kernels produce them.  With r_i = low 128 bits of blake2b-256(seed' || LE32(i)), i the pair's position in the CALL (one
 * check: no two pairs share a coefficient), never 0,
 *     prod_k e( sum_{i in range k} r_i L_i , s_g2_k )  ==  e( sum_i r_i R_i , G2 )
 * holds exactly when every decoded pair passes its own equation, except with probability <= 2^-128 over the seed: one decoding
 * launch and one coefficient launch over the whole call, bucket MSMs of C + 1 problems (R over all pairs, L_k over range k), and
 * ONE pairing kernel of C + 1 Miller loops under one final exponentiation.  Passed: accept[i] = "decoded", and nothing else
 * runs.  Failed: the per-pair kernels of h2v_check_pairs run behind it on the device, range by range against that range's plan;
 * nothing comes back to the host in between.  The 64-pair group stage of h2v_check_pairs_rlc is left out of this form: groups
 * would straddle ranges.  The seed follows h2v_check_pairs_rlc's rules (OS randomness; H2V_RLC_SEED_GIVEN for tests).
 *   counts[k] = 0 is allowed and costs no Miller loop; n = sum counts = 0 is H2V_OK; (inf, inf) pairs pass; a range whose L_k
 *   sums to infinity skips its loop, R at infinity skips the G2 loop, an all-infinite call passes.  Ranges whose plans are on
 *   one SRS (h2v_plan_same_srs) are legal and take a loop each; the verdicts do not depend on it.
 *   H2V_E_ARG: n_plans = 0; a null plan; plans on different devices; H2V_RLC_SEED_TRANSCRIPT, H2V_RLC_SEED_KEYED,
 *   H2V_RLC_FOLD_PAIRS or H2V_RLC_GROUPED (a derived seed would need a rule that binds each range's key); stream = NULL under
 *   deferred joins; a host batch in flight on ws.  H2V_E_LIMIT: n_plans > H2V_MULTI_SRS_MAX; n > 2^22 - both decided on the host
 *   before anything is enqueued.
 *   WORKSPACE: any workspace h2v_check_pairs would take for the first plan with pairs and n pairs; ws = NULL in the host form: a
 *   temporary one.  The call keeps a buffer set of its own on the workspace (created by the first such call).  On a laned
 *   workspace it runs as ONE piece on the caller's stream behind a join of the lanes, like the fold tail of a mixed call: never
 *   chunked, routed or coalesced.  fell_back, h2v_workspace_rlc_result (one record of kind RLC, msm_terms = n) and the verdict
 *   word behave as in h2v_check_pairs_rlc.  n_plans = 1 gives the accept[] / status[] of h2v_check_pairs_rlc on the same bytes. */
#define H2V_MULTI_SRS_MAX 16u
int h2v_check_pairs_multi(const h2v_plan *const *plans, uint32_t n_plans, const uint64_t *counts /* n_plans */,
                          const uint8_t *pairs /* (sum counts) * 96 */, uint8_t *accept, uint32_t *status /* or NULL */,
                          h2v_workspace *ws /* or NULL */, const h2v_rlc_opts *opts /* or NULL */, int *fell_back /* or NULL */);
int h2v_check_pairs_multi_device(const h2v_plan *const *plans, uint32_t n_plans, const uint64_t *counts, const uint8_t *pairs,
                                 uint8_t *accept, uint32_t *status, h2v_workspace *ws /* not NULL */, void *stream,
                                 const h2v_rlc_opts *opts /* or NULL */);

/* ---- mixed-key batches: proofs of SEVERAL plans on one SRS in one call ---------------------------------------------------
 * The reference verifies a list of (vk, instances, proof) triples in one call and one final check
 * (midnight_zk_stdlib::batch_verify(&params, &vks, &instances, &proofs), src/circuits/schnorr_circuit.rs:223-231; BASELINE
 * configs[2] is such a batch).  h2v_verify_mixed(_device) is that call: proof i belongs to plans[plan_of[i]], and accept[] /
 * status[] come back in the caller's order.  The proofs are sorted by plan on the device (one small copy kernel), every plan's
 * sub-batch runs the verify pipeline up to the pairing - on a laned workspace the sub-batches of all plans are in flight
 * together - and ONE tail checks every proof's pair (L, R), which no longer knows its key: one pairing launch over all n proofs,
 * or, with H2V_MIXED_RLC, ONE pairing for the call (the batch check of h2v_check_pairs_rlc; after a failed check the per-pair
 * kernels run behind it on the device).
 *   accept[i] / status[i] are exactly what h2v_verify_batch_device(plans[plan_of[i]], ...) gives for that proof alone - with
 *   H2V_MIXED_RLC except with probability <= 2^-128 over the seed.  A proof rejected before the pairing keeps its status bits
 *   and takes no part in anything after.  Recursive (IVC) plans are allowed in both modes: their pair is the folded (el', er').
 *   ONE SRS PER CALL: every listed plan must carry the same s_g2 (the reference takes ONE `params` too); otherwise H2V_E_ARG,
 *   and h2v_last_error() names the two plans.  api.verify_mixed / h2v::verify_mixed group a list by SRS and make one call each.
 *   plan_of is HOST memory in both forms (like n: the host sizes the launches from the per-plan counts).  The other pointers
 *   of h2v_mixed_batch are host pointers in the host form and device pointers in the device form, as for h2v_batch.
 *   H2V_E_ARG: plan_of[i] >= n_plans; plans on different devices; a workspace that does not fit EVERY listed plan (take one
 *   from h2v_workspace_create_multi over the same plans or a superset; ws = NULL in the host form: a temporary one), or that is
 *   smaller than n; a host batch in flight on ws; stream = NULL on a workspace with deferred joins.  H2V_E_LIMIT: more than
 *   H2V_MIXED_MAX_PLANS plans; n > 2^22 with H2V_MIXED_RLC.  n = 0 is H2V_OK.  A listed plan without a proof costs nothing.
 *   DEFERRED JOINS: a mixed call is a join point - it runs the open coalesced groups first, and `stream` waits for the call's
 *   lanes inside the call (accept[] / status[] are the stream's when the call returns).  Never routed, never coalesced; the
 *   workspace's failing-group estimate does not move.
 *   RECORDS: every plan with proofs takes one record as a prepare call does, and the tail takes the LAST record of the call, of
 *   kind CHECK - or RLC with H2V_MIXED_RLC, so that h2v_workspace_rlc_result(ws, 0, ..) reports the call's batch verdict
 *   (msm_terms: the pairs of the tail's last chunk - n on a workspace whose chunk holds the call).  On a laned workspace the tail
 *   is cut into chunks like any check call, and every chunk is its own batch check.  fell_back = 1: that verdict is "failed".
 *   SEED: h2v_verify_batch_rlc's rules.  ONE seed per call; the coefficient of proof i is drawn from its position in the CALL
 *   (within its chunk of the tail - every chunk a check of its own under its own tweak of the seed, as for any RLC call on a laned
 *   workspace, and h2v_workspace_create_multi makes a laned one), never from its position within its key - with repeated
 *   coefficients two proofs of different keys could cancel each other's error.
 *   H2V_MIXED_FOLD_MSM (only together with H2V_MIXED_RLC; alone: H2V_E_ARG): the reference's whole batch_verify - every
 *   proof's DualMSM scaled by a random coefficient, added, ONE MSM and ONE pairing for the call.  H2V_MIXED_RLC alone folds only
 *   the pairings: every proof still runs its own ladder MSM.  With the flag, a plan that has the batch form of
 *   h2v_verify_batch_rlc (per-proof terms plus VK bases) runs phase 1 only and hands its terms - scalars scaled by the proof's
 *   coefficient, COPIES of the points, the VK-base scalars summed per plan - to ONE bucket MSM over the call; any other plan (a
 *   recursive one: its fold challenge hashes the proof's own MSM result) runs as without the flag and joins as one pair per proof.
 *   accept[] / status[] keep the contract above.
 *   TERM COUNT of a call: N_R = sum over the plans with the batch form that have proofs of (count_k * n_var_k + n_fix_k) + the
 *   number of proofs of the other plans (count_k: the plan's proofs in the call; n_var_k / n_fix_k: its per-proof and VK-base
 *   MSM terms).  N_R > 2^22 is H2V_E_LIMIT, decided on the host before anything is enqueued.  h2v_workspace_rlc_result(ws, 0, ..)
 *   reports msm_terms = N_R and the verdict; the tail's record is the call's last, of kind RLC, and is ONE piece on a laned
 *   workspace too (coefficients follow the position in the call, not in a chunk).
 *   FALL-BACK: when the one check fails, per-proof verdicts are needed and phase-1 results no longer exist (the lanes recycle
 *   them), so the HOST decides: the call downloads the verdict and synchronises `stream` ONCE - BOTH forms, the device form too,
 *   return only after the batch verdict is known - and after a failed check runs the H2V_MIXED_RLC path on the same inputs with
 *   the same seed; its accept[] / status[] are final, fell_back = 1, and the last record is that second pass's.  A failing call
 *   pays the attempt plus the call without the flag; a passing call never runs a ladder.
 * WHICH SHAPE IT IS FOR: many keys with few proofs each (a node that validates proofs of many scripts) - there the per-key
 * route is one chain of lone waves per key.  Without H2V_MIXED_FOLD_MSM it does not fold the MSMs of different keys into one
 * bucket MSM: for a batch dominated by ONE key h2v_verify_batch_rlc on that key stays the faster batch-accept form.  With the
 * flag it does, and on 16 keys x 64 proofs it is the fastest of the three routes measured (tools/bench_mixed.py --fold: 6.8 ms a
 * call against 10.3 without the flag and 12.7 for one h2v_verify_batch_rlc call per key); on 2 keys x 2048 proofs it LOSES to the
 * per-key h2v_verify_batch_rlc calls (7.1 against 3.3-4.8 ms), whose steps overlap in the lanes: few keys with many proofs each
 * stay with that route.  Measurements: DESIGN.md 15 / 15.1, profiles/mixed_fold.json.
 *   H2V_MIXED_GROUPED (only together with H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM; otherwise H2V_E_ARG): phase 1 of every key in ONE
 *   launch per kernel.  Without it every plan with proofs is a sub-batch of its own - a decompression launch, a combiner launch, a
 *   terms launch and a record per KEY, so the cost of a call grows with its keys, not with its proofs.  With it the proofs of all
 *   GROUPABLE plans - those that have the batch form above and whose combiner register file fits LDS - run as one unit over the
 *   grouped positions (the proofs sorted by plan): one decompression launch, one combiner launch per transcript hash present,
 *   one terms launch, each block finding its plan in a device table.  On a laned workspace the grouped positions are cut into
 *   chunks through the lanes like any unit; a chunk may begin and end inside a plan and span many plans (the lanes of
 *   h2v_workspace_create_multi are sized for the largest of every dimension).  Every other plan (recursive, or with a global
 *   register file) keeps its own sub-batch and joins the tail as without the flag.
 *   RESULTS are those of the same call without the flag under the same seed: accept[], status[], fell_back, and - the coefficient
 *   of a proof being drawn from its position in the CALL - the call's two sums bit for bit.
 *   RECORDS: the grouped part takes ONE record whatever the number of plans, every other plan with proofs one, the tail the last.
 *   LIMITS: up to H2V_MIXED_GROUPED_MAX_PLANS plans may be listed, of which at most H2V_MIXED_GROUPED_MAX_OTHER plans that are not
 *   groupable may have proofs (grouped part + 62 + tail = the 64 records of a workspace's ring); beyond either H2V_E_LIMIT, decided
 *   on the host before anything is enqueued.  H2V_MIXED_MAX_PLANS holds for every call without the flag.
 *   FALL-BACK as above.  With more than H2V_MIXED_MAX_PLANS plans with proofs the second pass - one sub-batch and one record per
 *   plan - runs its sub-batches in slices of at most 62 plans, each slice joined before the next, and ends in the ONE tail.
 *   OPTIONS: H2V_OPT_COMBINER_SCHEDULE and H2V_OPT_COMBINER_PROOFS_PER_BLOCK shape per-plan launches and do not apply to the
 *   grouped launch: every plan runs its narrow schedule with as many proofs per block as its register file allows in LDS.  The
 *   launch reserves the LDS of the largest register file among its plans for every block (one size class per transcript hash).
 *   WHICH SHAPE IT IS FOR: many keys with a handful of proofs each.  Measured (tools/bench_mixed.py --fold --grouped,
 *   profiles/mixed_grouped.json; 1024 accepting proofs, ms per call, five runs): 16 keys x 64 4.9-6.4 against 6.7-6.8 without the
 *   flag; 64 keys x 16 5.7-6.9 against 13.5-13.7 (48.6-49.0 for one h2v_verify_batch_rlc call per key); 256 keys x 4 5.7-7.5 (186-188
 *   per key; the call without the flag cannot take it) - it wins on all three by the project's rule.  NOT measured: 2 keys x 2048;
 *   expect no gain for few keys with thousands of proofs each, where the chunks of the grouped unit are what the per-plan
 *   sub-batches already were, and stay with the per-key h2v_verify_batch_rlc calls there.  The flag is opt-in.  DESIGN.md 15.2.
 *   H2V_MIXED_ACROSS_SRS (only together with H2V_MIXED_RLC; otherwise H2V_E_ARG): the listed plans may be on SEVERAL SRS, and the
 *   call still ends in ONE pairing: the multi-pairing of h2v_check_pairs_multi - one Miller loop per SRS and one for the right-hand
 *   sum under one final exponentiation,  prod_k e(sum_{i in k} r_i L_i, s_g2_k) == e(sum_i r_i R_i, G2).  Every proof of the call
 *   has a coefficient of its own, so the soundness argument of that call applies as it stands.  Without the flag every call
 *   behaves exactly as before, the H2V_E_ARG that names two plans on different SRS included.
 *   SRS CLASSES: the plans are classed by their s_g2; classes are numbered in the order in which a listed plan first carries
 *   them.  A class without a proof takes no bucket problem and no Miller loop and does not count against the limit.
 *   ARGUMENT RULES, decided on the host before anything is enqueued, in this order: the flag without H2V_MIXED_RLC is H2V_E_ARG;
 *   the plan-count limits and n > 2^22 as without the flag; more than H2V_MULTI_SRS_MAX classes WITH proofs is H2V_E_LIMIT; then
 *   N_R > 2^22 and the workspace and device rules as without the flag.  n = 0 is H2V_OK.
 *   RESULTS: accept[] / status[] keep the contract above.  With ONE class among the proofs a call with the flag returns what the
 *   same call without it returns.
 *   WITH H2V_MIXED_FOLD_MSM (with or without H2V_MIXED_GROUPED): phase 1 and the term pool are exactly those of the call without
 *   the flag - the SRS never enters phase 1 - and the coefficients follow the position in the CALL.  The tail sums R over the N_R
 *   terms and, per class k with proofs, L_k over class k's proofs, all in the same six bucket-MSM launches, and ONE multi-pairing
 *   follows; no group stage.  With one class R and L are the sums of the call without the flag.  FALL-BACK as above: after a
 *   failed check the host runs the form below on the same inputs with the same seed (fell_back = 1, the last record is the second
 *   pass's, ONE synchronisation per call).
 *   WITHOUT H2V_MIXED_FOLD_MSM: the sub-batches run as under H2V_MIXED_RLC, and ONE tail follows, in one piece whatever the
 *   workspace - on the caller's stream behind a join of the lanes, never chunked, routed or coalesced.  The coefficient of proof
 *   i is drawn by its CLASS-MAJOR position P(i) = the proofs in lower classes + the rank of i within its class in the caller's
 *   order (one class: P(i) = i):  r_i = low 128 bits of B(seed' || LE32(P(i))), 1 if 0, no chunk tweak.  Behind the multi-pairing's
 *   skip flags the per-pair kernels of h2v_check_pairs run per class, through a plan of THAT class, so H2V_ST_PAIRING lands where
 *   the per-key call puts it; nothing comes back to the host in between.  fell_back = 1: the check failed.
 *   RECORDS: the tail takes the call's LAST record, of kind RLC; h2v_workspace_rlc_result(ws, 0, ..) gives the verdict and
 *   msm_terms = N_R (with H2V_MIXED_FOLD_MSM) or n.  SEED: the rules above; H2V_RLC_SEED_KEYED binds each proof's own key, whose
 *   tag covers the key's s_g2 tables, and both forms derive the same seed.
 *   h2v_aggregate_mixed(_device) does not take the flag: one pair cannot span SRS.  Numbers: not measured.  DESIGN.md 15.3. */
#define H2V_MIXED_RLC 1u          /* batch-accept: ONE pairing for the call; otherwise one pairing per proof, in ONE launch */
#define H2V_MIXED_FOLD_MSM 2u     /* with H2V_MIXED_RLC: ONE bucket MSM over the call's per-proof terms as well; one host synchronisation */
#define H2V_MIXED_GROUPED 4u      /* with both: phase 1 of every groupable plan in ONE launch per kernel; up to 1024 plans */
#define H2V_MIXED_ACROSS_SRS 16u   /* with H2V_MIXED_RLC: the listed plans may be on several SRS; ONE multi-pairing for the call */
#define H2V_MIXED_MAX_PLANS 64u   /* more plans in one call without H2V_MIXED_GROUPED: H2V_E_LIMIT */
#define H2V_MIXED_GROUPED_MAX_PLANS 1024u /* more plans in one H2V_MIXED_GROUPED call: H2V_E_LIMIT */
#define H2V_MIXED_GROUPED_MAX_OTHER 62u   /* ... of which plans that are not groupable and have proofs */
typedef struct {
    uint64_t n;
    const uint32_t *plan_of;      /* HOST memory in BOTH forms: n entries, plan_of[i] < n_plans */
    const uint8_t *proofs;        /* as h2v_batch */
    const uint64_t *proof_off;    /* n + 1 entries */
    const uint8_t *instances;     /* proof i's 32 * n_public_inputs(plans[plan_of[i]]) bytes, concatenated in proof order */
    const uint8_t *committed;     /* 48 bytes for every proof whose plan has a committed instance, in proof order; NULL if no listed plan has one */
} h2v_mixed_batch;
int h2v_verify_mixed(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *accept,
                     uint32_t *status /* or NULL */, h2v_workspace *ws /* or NULL */, uint32_t flags,
                     const h2v_rlc_opts *opts /* or NULL */, int *fell_back /* or NULL */);
int h2v_verify_mixed_device(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *accept,
                            uint32_t *status, h2v_workspace *ws /* not NULL */, void *stream, uint32_t flags,
                            const h2v_rlc_opts *opts);

/* ---- aggregate calls: ONE pair (L, R) per batch, checked later and elsewhere ------------------------------------------------
 * Every batch-accept form above ends inside the call: it forms L = sum r_i L_i and R = sum r_i R_i, runs one pairing on them
 * and queues its fall-back behind that pairing.  The reference's callers keep exactly that value - the collapsed DualMSM of
 * the batch - and decide later when to check it: `dual_msm.scale(r)`, `acc.add_msm(..)`, then `check` once over everything
 * collected (examples/ivc.rs:85-96, 195-208; midnight_zk_stdlib::batch_verify).  h2v_aggregate_batch / h2v_aggregate_mixed are
 * that first half: they split batch-accept the way h2v_prepare_batch / h2v_check_pairs split per-proof verification - "prepare the
 * batch's pair" now, "check pairs from anywhere" (h2v_check_pairs for one, h2v_check_pairs_rlc for many: one pairing) later.
 *   PAIR.  pair = compress(L) || compress(R), two 48-byte zcash encodings: the format of h2v_prepare_batch.  L = sum r_i L_i and
 *   R = sum r_i R_i over the INCLUDED proofs, (L_i, R_i) being the pair h2v_prepare_batch returns for proof i (a non-recursive
 *   key: pi and the multi-open MSM; a recursive key: the folded (el', er')).  An infinite sum is encoded 0xc0, 0, ...; when
 *   nothing is included the pair is (inf, inf), which h2v_check_pairs accepts (as an empty RLC batch passes).  n = 0 is H2V_OK and
 *   writes (inf, inf).
 *   COEFFICIENTS.  Single-key form: exactly those the h2v_verify_batch_rlc call of the same shape would draw on that workspace -
 *   r_i = the low 128 bits of blake2b-256(seed' || LE32(pos)), or 1 if that is 0.  An ordinary workspace: seed' = seed_used, pos =
 *   the index in the call.  A laned workspace: chunk c (proofs c * chunk ..) hashes seed_used with 0x9e3779b9 * (c + 1) xored into
 *   its last 32-bit word, pos = the index within the chunk.  Mixed form: pos = the position in the CALL, no tweak (the rule of
 *   H2V_MIXED_FOLD_MSM); info->chunk is 0 for it.  h2v_aggregate_info carries what is needed to recompute them.
 *   included[i] (n bytes) = 1 iff proof i was not rejected before the pairing: phase-1 status zero with H2V_ST_BAD_POINT folded in,
 *   the RLC forms' good_i.  It is NOT a verdict: an included proof is accepted iff the pair's equation holds (up to the soundness
 *   error).  status[i] (may be NULL) is what h2v_prepare_batch reports: H2V_ST_PAIRING is never set, H2V_ST_RECURSION stays.
 *   WHERE THE CALLS STOP.  No pairing, no group stage, no per-proof MSM or pairing: nothing is queued behind the bucket MSMs but
 *   the export (one small kernel that adds the chunks' sums and compresses the two totals).  A recursive plan in
 *   h2v_aggregate_batch takes the H2V_RLC_FOLD_PAIRS route, flag or not: the per-proof pipeline through the fold, then the pairs
 *   are combined.  A non-recursive plan whose VK-base terms are not the tail of its term list (no plan.py plan) has no batch form:
 *   H2V_E_ARG.  h2v_aggregate_mixed is the H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM form without its verdict: the same layout, term count
 *   (info->msm_terms = N_R) and limits, one SRS per call, at most H2V_MIXED_MAX_PLANS plans, recursive plans join as one pair per
 *   proof; the device form returns after enqueueing - no download, no synchronisation of `stream`, no second pass.
 *   LANED WORKSPACES.  The call is a join point as a mixed call is: it runs the open coalesced groups first, and `stream` waits for
 *   the call's lanes inside the call (the per-chunk sums must meet).  Never coalesced, never routed; the failing-group estimate
 *   does not move.  Consecutive calls on ONE stream therefore run one after the other; calls issued on SEVERAL streams overlap in
 *   the lanes (a workspace keeps the sums of up to 16 calls of at most 128 chunks each apart; a call of more chunks waits for every
 *   export before it and holds the others back behind its own) - a caller that wants the throughput of deferred RLC
 *   calls gives every call in flight a stream of its own (DESIGN.md section 16 has what that measured).
 *   RECORDS.  One record of kind RLC (the mixed form: its tail's, the call's last): h2v_workspace_rlc_result reports its times
 *   with pairing_ms = 0 and batch_accepted = H2V_BATCH_NOT_CHECKED.
 *   ERRORS as h2v_verify_batch_rlc(_device) / h2v_verify_mixed(_device): n > 2^22 is H2V_E_LIMIT; stream = NULL under deferred
 *   joins, a host batch in flight on ws, ws = NULL in a device form are H2V_E_ARG; ws = NULL in a host form: a temporary workspace.
 *   opts->flags: H2V_RLC_SEED_GIVEN and H2V_RLC_ONE_STREAM as ever, H2V_RLC_SEED_TRANSCRIPT in the single-key forms (not beside
 *   H2V_RLC_SEED_GIVEN), H2V_RLC_SEED_KEYED in the mixed forms (not beside either), H2V_RLC_FOLD_PAIRS accepted and ignored,
 *   H2V_RLC_GROUPED in the mixed forms (phase 1 grouped as with H2V_MIXED_GROUPED: the same pair bit for bit), any other bit H2V_E_ARG.
 *   The device forms take device pointers (pair 4-byte aligned; plan_of stays host memory); info is HOST memory in both forms.
 *   SOUNDNESS.  DRAWN OR GIVEN SEED: a pair vouches for its proofs only to someone who trusts that seed_used was unpredictable to
 *   the provers - the same trust domain as the caller of h2v_verify_batch_rlc.  It is NOT a proof for third parties.  DERIVED SEED
 *   (H2V_RLC_SEED_TRANSCRIPT, single-key form; H2V_RLC_SEED_KEYED, mixed form): nothing has to be kept from the provers - in the random-oracle model for blake2b a
 *   prover making q hash evaluations gets a rejecting proof into an accepting pair with probability at most q / 2^128 - and anyone
 *   who holds the same key, the same inputs and the same chunk size recomputes the same seed and the same pair (seed.py), so a
 *   pair can be compared between nodes and re-derived by an auditor.  It is still not a succinct proof for someone without the
 *   inputs.  Whoever combines the pairs of several
 *   calls must scale them again with fresh coefficients - which is what h2v_check_pairs_rlc does; adding pairs unscaled lets the
 *   errors of two calls cancel (tests/test_aggregate_gpu.py). */
#define H2V_BATCH_NOT_CHECKED 2u  /* h2v_workspace_rlc_result: batch_accepted of an aggregate call */
typedef struct {
    uint8_t  seed_used[32];  /* the effective seed of THIS call: the OS draw, or the given seed with the call count mixed in */
    uint32_t chunk;          /* 0 on an ordinary workspace and for the mixed form; else the chunk size that cut the call (coefficients follow it) */
    uint32_t n_chunks;       /* 1 on an ordinary workspace and for the mixed form (and for n = 0 on any workspace) */
    uint32_t msm_terms;      /* terms of the right-hand bucket MSM(s), summed over chunks */
    uint32_t reserved;       /* the SEED SOURCE, under the name the word has always had (callers that zero `reserved` keep compiling; read it
                              * as H2V_AGGREGATE_SEED_SOURCE(info)).  0: seed_used was drawn or given; 1: derived (H2V_RLC_SEED_TRANSCRIPT / _KEYED) -
                              * the host form fills seed_used from its download, the device form writes zeros (the seed is not known
                              * when the call returns: h2v_workspace_seed_used has it once the stream is synchronised) */
} h2v_aggregate_info;        /* HOST memory, written before the call returns, in both forms; may be NULL */
#define H2V_AGGREGATE_SEED_SOURCE(info) ((info)->reserved)   /* seed_source: 0 drawn or given, 1 derived */
int h2v_aggregate_batch(const h2v_plan *plan, const h2v_batch *batch, uint8_t pair[96], uint8_t *included /* n */, uint32_t *status /* or NULL */,
                        h2v_workspace *ws /* or NULL */, const h2v_rlc_opts *opts /* or NULL */, h2v_aggregate_info *info /* or NULL */);
int h2v_aggregate_batch_device(const h2v_plan *plan, const h2v_batch *batch, uint8_t *pair, uint8_t *included, uint32_t *status,
                               h2v_workspace *ws /* not NULL */, void *stream, const h2v_rlc_opts *opts, h2v_aggregate_info *info);
int h2v_aggregate_mixed(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t pair[96], uint8_t *included,
                        uint32_t *status /* or NULL */, h2v_workspace *ws /* or NULL */, const h2v_rlc_opts *opts, h2v_aggregate_info *info);
int h2v_aggregate_mixed_device(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *pair, uint8_t *included,
                               uint32_t *status, h2v_workspace *ws /* not NULL */, void *stream, const h2v_rlc_opts *opts,
                               h2v_aggregate_info *info);

/* ---- parity / debugging surface ----------------------------------------------------------------------------
 * The reference's own intermediate-value trace (cargo feature plutus_debug, src/plutus_gen/emitters/plinth.rs:792-831):
 * theta, beta, gamma, x, y, hEval, vanishing_s, ..., every expression_i, plus el / er.
 * Host buffers.  scalars_out: n_trace * 32 bytes LE in the order of h2v_plan_trace_slots(); er_out / el_out:
 * 96 bytes affine x||y big-endian (all-zero = infinity). */
int h2v_plan_trace_slots(const h2v_plan *plan, uint32_t *slot_ids, uint32_t cap, uint32_t *n_out);
int h2v_trace(const h2v_plan *plan, const uint8_t *proof, size_t proof_len, const uint8_t *instances,
              const uint8_t *committed, uint8_t *scalars_out, uint8_t *msm_scalars_out /* T*32 or NULL */,
              uint8_t el_out[96], uint8_t er_out[96], uint32_t *status_out, uint8_t *accept_out);

/* The transcript + Fr-combiner interpreter ALONE on a batch of host buffers: no decompression, MSM or pairing runs, so the plan's
 * program may be any byte code h2v_plan_load accepts (the hand-assembled programs of tests/test_vm_programs_gpu.py), whatever
 * its OUT_SCALARs would mean to the rest of the pipeline.  status_out: n words, the H2V_ST_* bits the interpreter sets
 * (BAD_SCALAR, INVERSE_OF_ZERO, SHORT_PROOF, RECURSION); msm_scalars_out: n * n_terms * 32 bytes LE (a term no OUT_SCALAR
 * wrote reads zero); trace_out: n * n_trace * 32 bytes LE in the order of h2v_plan_trace_slots(), NULL unless want_trace.
 * want_trace != 0 forces the plan's NARROW schedule, whatever H2V_OPT_COMBINER_SCHEDULE says: the trace table names the narrow
 * schedule's registers; it needs a plan with a trace table.  The launch takes H2V_OPT_COMBINER_SCHEDULE and
 * H2V_OPT_COMBINER_PROOFS_PER_BLOCK from h2v_probe_set_option.  Argument errors return H2V_E_ARG. */
int h2v_probe_vm(const h2v_plan *plan, const h2v_batch *batch /* host buffers */, int want_trace,
                 uint32_t *status_out /* n */, uint8_t *msm_scalars_out /* n * n_terms * 32, LE */,
                 uint8_t *trace_out /* n * n_trace * 32, LE; NULL unless want_trace */);

/* The G1 decompression launch ALONE on a batch of host buffers, made exactly as the pipelines make it (one launch whose waves
 * take 64-point units from a queue: the subgroup tests, then the square roots): nothing behind it runs.  The points are those
 * of proof 0's slots, then proof 1's, ...; a proof has S = n_points + n_ci + 2 * ivc slots: the plan's proof points in plan
 * order (the last one is the opening proof pi), the committed instance if the plan has one, the left and the right
 * accumulator point if the plan is recursive.  Every buffer is the caller's, sized for n * S points:
 *   xy_be         n * S * 96    affine x || y, big-endian canonical; all-zero for infinity and wherever valid == 0
 *   valid         n * S         1: the encoding is well-formed (compression bit, a canonical x or the one infinity encoding; the
 *                               proof is not short) and x is on the curve; the point is stored, whether in G1 or not.  Else 0
 *   valid_sub     n * S         1: the encoding is well-formed and the r-torsion test passed for the curve points with this x
 *                               (the valid infinity encoding: 1).  It is taken without the square root: where x^3 + 4 is not
 *                               a square it says nothing, and only valid && valid_sub - "a point of G1" - is the verdict
 *   tables        n * S * 448   dwords, or NULL: the MSM window tables as the kernel left them - per point [1..8]P, then
 *                               [1..8]phi(P), each entry x, y as 14 + 14 limbs of 28 bits, Montgomery (R = 2^392), below 2p.
 *                               Only with with_tables != 0 (the launch is then given the workspace's tables; with 0 it builds
 *                               none, as the pair checks and the batch-accept forms run it).  The tables of a point with
 *                               valid == 0 are not written; those of a curve point outside G1 are unspecified
 *   blocks_out    1             the grid of the launch: blocks of four waves; 2 * ceil(n * S / 64) units go through the queue
 * Before the launch every output is preset to 0xA5 bytes, so that what the kernel left unwritten shows.
 * Argument errors return H2V_E_ARG. */
int h2v_probe_decompress(const h2v_plan *plan, const h2v_batch *batch /* host buffers */, int with_tables,
                         uint8_t *xy_be, uint8_t *valid, uint8_t *valid_sub, uint32_t *tables /* or NULL */, uint32_t *blocks_out);

/* primitive probes for the GPU parity tests (host buffers; canonical little-endian limbs) */
int h2v_probe_field(int device, int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out);
int h2v_probe_blake2b(int device, uint32_t n, uint32_t len, const uint8_t *msgs, uint8_t *digests);
/* The same through the code path of the keyed transcript flavour: blake2b with a digest of digest_len = 32 or 64 bytes, keyed
 * with key[0 .. key_len) (key_len <= 64; 0 = unkeyed, key may be NULL), of n messages of `len` bytes each; digests: n x
 * digest_len bytes.  The state behind the key block is worked out on the host as h2v_plan_load does it; an empty message
 * under a key (the key block is then the final block) is hashed on the device from the start. */
int h2v_probe_blake2b_ex(int device, uint32_t n, uint32_t len, const uint8_t *msgs, uint32_t digest_len, const uint8_t *key,
                         uint32_t key_len, uint8_t *digests);
/* The digest kernels of a derived seed (H2V_RLC_SEED_TRANSCRIPT) ALONE, as the calls queue them, on bytes that need not be proofs:
 * form 1 - batch as for h2v_verify_batch, n_pi rows of 32 instance bytes and n_ci (0 / 1) rows of 48 committed bytes per proof;
 * form 2 - batch->proofs holds n x 96 bytes, proof_off / instances / committed are ignored.  Host buffers; the proof bytes go up
 * at the alignment proof_off[0] has (mod 16).  seed: the 32 bytes.  n = 0 or n > 2^22: H2V_E_ARG. */
int h2v_probe_batch_seed(int device, uint32_t form, const uint8_t key_tag[32], const h2v_batch *batch /* host buffers */, uint32_t n_pi,
                         uint32_t n_ci, uint8_t seed[32]);
/* The digest kernels of a keyed seed (H2V_RLC_SEED_KEYED, form 3) ALONE, as the mixed calls queue them, on bytes that need not be
 * proofs: n_plans listed plans given by key_tags (n_plans x 32 bytes), n_pi[k] rows of 32 instance bytes and n_ci[k] (0 / 1) rows of
 * 48 committed bytes per proof of plan k; batch as for h2v_verify_mixed, host buffers (proof_off need not ascend: a descending pair
 * is an empty proof).  seed: the 32 bytes.  n = 0 or n > 2^22, n_plans = 0 or a plan_of out of range: H2V_E_ARG. */
int h2v_probe_mixed_seed(int device, uint32_t n_plans, const uint8_t *key_tags, const uint32_t *n_pi, const uint32_t *n_ci,
                         const h2v_mixed_batch *batch /* host buffers */, uint8_t seed[32]);
int h2v_probe_g1_decompress(int device, uint32_t n, const uint8_t *compressed, uint8_t *xy_be, uint8_t *valid);
/* sum_t s_t * B_t per group: n groups of T terms; scalars n*T*32 B LE, bases n*T*48 B compressed; out n*96 B affine BE */
int h2v_probe_g1_msm(int device, uint32_t n, uint32_t T, const uint8_t *scalars, const uint8_t *bases_compressed,
                     uint8_t *out_xy_be);
/* The same sums through the multi-term ladder alone (k_g1_msm_multi: several GLV halves per lane on one accumulator, unchecked
 * additions judged by one Z test at the end, the complete law for a lane that fails it), launched as the pipelines launch it
 * but with halves_per_lane = 3 .. 8 given by the caller: half 2 t + h of a proof goes to lane (2 t + h) / halves_per_lane.
 * Arguments as for h2v_probe_g1_msm.  H2V_E_ARG for halves_per_lane outside 3 .. 8 or more than 256 lanes per proof.  Crafted
 * exceptional additions in every lane shape: tests/test_msm_multi_ladder_gpu.py */
int h2v_probe_g1_msm_multi(int device, uint32_t n, uint32_t T, uint32_t halves_per_lane, const uint8_t *scalars,
                           const uint8_t *bases_compressed, uint8_t *out_xy_be);
/* the fixed-base launch of a split MSM on its own: sum over the plan's n_fix VK-base terms of s_t * B_t through the all-window
 * tables built at h2v_plan_load (k_g1_msm_fixed, bases_per_lane = 1 .. 4 as the launcher would pick); scalars n * n_fix * 32 B
 * LE in the order of the plan's VK-base terms, out n * 96 B affine BE; *n_fix_out (may be NULL) receives n_fix.  H2V_E_ARG for
 * plans without such tables (recursive plans).  Edge scalars of the signed-window recoding: tests/test_gpu_parity.py */
int h2v_probe_g1_msm_fixed(const h2v_plan *plan, uint32_t n, uint32_t bases_per_lane, const uint8_t *scalars, uint8_t *out_xy_be,
                           uint32_t *n_fix_out);
/* the bucket (Pippenger) MSM of the RLC mode on its own: sum_n s_n * B_n; scalars n*32 B LE (< r), bases n*48 B compressed
 * (encodings that do not decompress count as infinity); out 96 B affine BE (all-zero = infinity) */
int h2v_probe_g1_msm_pippenger(int device, uint32_t n, const uint8_t *scalars, const uint8_t *bases_compressed,
                               uint8_t *out_xy_be);
/* The same kernels as the RLC mode launches them: 1 or 2 problems side by side in every launch (the production calls run their
 * right- and left-hand sums that way), each with its own term count, halves, scalars, point pool and index map.
 *   halves            2: scalars < r, split by GLV; 1: scalars below 2^128 (H2V_E_ARG for a larger one)
 *   points_compressed n_points x 48 B, decompressed on the device; infinity and encodings that do not decompress give the all-zero
 *                     record.  Records [0, n_pool0) are served through the kernels' pool0, the rest through pool1 (n_pool0 ==
 *                     n_points: one pool).
 *   pidx              n indices into the pool (may repeat; one >= n_points is H2V_E_ARG), or NULL for the identity map, which
 *                     needs n == n_points
 *   out_xy_be         96 B affine big-endian, all-zero = infinity
 *   dump              NULL, or H2V_PIP_DUMP_DWORDS dwords: [0..4] the shape the launcher chose - window bits c, windows W, buckets
 *                     per window NB, chain - and the number of blocks k_pip_accumulate was launched with; [5..32] the size classes
 *                     k_pip_scan wrote (per class k = 0..8: first rank, end rank, first lane; then the lane total); then the
 *                     W NB + 1 exclusive offsets of the buckets' entry lists; then the W NB bucket ids by descending size
 * acc_grid_cap: test-only, 0 = none; caps the grid of k_pip_accumulate so that every block walks several logical blocks.
 * The shape options H2V_OPT_RLC_WINDOW_BITS / H2V_OPT_RLC_CHAIN of h2v_probe_set_option apply.  tests/test_bucket_msm_shapes_gpu.py */
#define H2V_PIP_DUMP_DWORDS 20514
typedef struct h2v_pip_probe {
    uint32_t n, halves;
    const uint8_t *scalars;            /* n x 32 B LE */
    uint32_t n_points, n_pool0;
    const uint8_t *points_compressed;
    const uint32_t *pidx;
    uint8_t *out_xy_be;
    uint32_t *dump;
} h2v_pip_probe;
int h2v_probe_g1_msm_pippenger_ex(int device, uint32_t n_problems, const h2v_pip_probe *problems, uint32_t acc_grid_cap);
/* test-only: the two sums of the most recent H2V_MIXED_FOLD_MSM call on ws, L = sum r_i L_i then R = sum r_i R_i: affine, 96 B
 * big-endian x || y each, all-zero = infinity.  Synchronises the device.  H2V_E_ARG when no such call has run on ws. */
int h2v_probe_mixed_fold_sums(h2v_workspace *ws, uint8_t out_xy_be[192]);
/* test-only: the sums of the most recent H2V_MIXED_ACROSS_SRS | H2V_MIXED_FOLD_MSM call on ws: R, then L_k of every SRS class with
 * proofs in class order, affine, 96 B each as above; *n_classes = the classes written.  cap: the classes out_xy_be has room for. */
int h2v_probe_mixed_fold_sums_multi(h2v_workspace *ws, uint32_t cap, uint8_t *out_xy_be /* (1 + cap) * 96 */, uint32_t *n_classes);
/* 2P + (neg ? -Q : Q) by the one-lane mixed addition and by the quad-cooperative one (the forced MSM shape H2V_MSM_LPT=8):
 * pq = x_P, y_P, x_Q, y_Q as 12 canonical LE dwords each; out = 5 x 42 dwords of lazily reduced limbs (X, Y, Z; 14 limbs of
 * 28 bits each, Montgomery form R = 2^392): the one-lane result, then lanes 0..3 of a quad.  Guards a compiler issue
 * (csrc/h2v_curve28.hpp: g1j28_madd_quad). */
int h2v_probe_quad_madd(int device, const uint32_t *pq, int neg, uint32_t *out);
/* The merged products of the lazily reduced field (csrc/h2v_fp28.hpp: f28_dot2) and the one-lane G1 formulas built on them, on
 * RAW records: 14 dwords = 14 limbs of 28 bits, Montgomery form R = 2^392, limbs and values as large as the bounds stated in
 * the headers allow (h2v_probe_field takes canonical operands and cannot carry such limbs).
 *   op & 15:  0: a b + c d    1: a^2 + c d    2: 2 a^2 + c d      n records each in a, b, c, d (b unused by 1, 2); out n x 14
 *             3: a b    4: a^2     the plain product and squaring (fp_mont28, fp_montsqr28); b (for 4), c and d are passed like
 *                                  the other ops' and unused
 *             8: 2P    9: P + Q with Q affine (mixed, unchecked)    10: P + Q (complete but for infinity)
 *                P = n x 42 dwords (X, Y, Z) in a, Q likewise in b (Z ignored by 9); c, d unused (may be NULL);
 *                out n x 44 dwords: X, Y, Z, the return code of the full addition (0 sum, 1 doubled, 2 infinity), 0
 *   op | 16:  the forms with the multiplier inlined (ops 0 .. 4, 8, 9)      op | 64: subtract Q (ops 9, 10)
 * tests/test_field_dot2_gpu.py, tests/test_field_carry_chain.py */
int h2v_probe_f28_dot2(int device, int op, uint32_t n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                       uint32_t *out);
/* e(p1, s_g2 of plan) == e(p2, G2) for n pairs of compressed G1 points; out[i] = 1/0 */
int h2v_probe_pairing(const h2v_plan *plan, uint32_t n, const uint8_t *p1_compressed, const uint8_t *p2_compressed,
                      uint8_t *out);
/* same with an explicit kernel (impl 0: one lane per proof, 1: cooperative - 32 lanes per proof, or the wide engine for small n,
 * as the launcher picks, or the engine H2V_OPT_PAIRING_ENGINE of h2v_probe_set_option names -, 2 / 3 / 5 / 6: its narrow (16 lanes
 * per proof) / wide (64) / six-lane / twelve-lane engine whatever n, -1: default) and an optional dump (n * 24 * 48 bytes): the 12 Fp
 * coefficients (flat order w^k, re/im; canonical LE) of f after the Miller loop (records 0..11) and after the final
 * exponentiation (records 12..23), from every kernel */
int h2v_probe_pairing_ex(const h2v_plan *plan, uint32_t n, const uint8_t *p1_compressed, const uint8_t *p2_compressed,
                         uint8_t *out, int impl, uint8_t *dbg);
/* The same launch with the entry states a pipeline can hand the pairing, and everything it writes.  Optional inputs (NULL: as
 * above): status_in - n status words the proofs arrive with; valid_sub_in - n x 2 bytes, the subgroup verdict of slot p1 and of
 * slot p2 (NULL: the kernel gets no such array); el_jac_in - n x 36 dwords X, Y, Z (12 x 32-bit limbs of the Montgomery form the kernels keep, R = 2^392;
 * infinity is Z = 0): the first argument in Jacobian form, taken instead of slot p1 as recursion and the fold-pairs batch form
 * pass it.  Outputs, each optional: status_out - n + H2V_PROBE_PAIRING_GUARD words; accept - n + GUARD bytes; dbg - (n + GUARD)
 * x 24 x 48 bytes, records as above; lanes_out - lanes per proof of the engine that ran (1, 6, 12, 16, 32, 64).  Every device
 * output is allocated for n + GUARD proofs, preset to 0xA5 bytes and copied back whole: a record no kernel wrote - a proof
 * rejected on entry, and everything behind proof n - 1, where the dead groups of the last wave would write - reads 0xA5.
 * tests/test_pairing_engines_gpu.py */
#define H2V_PROBE_PAIRING_GUARD 64u
int h2v_probe_pairing_states(const h2v_plan *plan, uint32_t n, const uint8_t *p1_compressed, const uint8_t *p2_compressed, int impl,
                             const uint32_t *status_in, const uint8_t *valid_sub_in, const uint32_t *el_jac_in,
                             uint32_t *status_out, uint8_t *accept, uint8_t *dbg, uint32_t *lanes_out);

/* ---- library lifecycle (round 4) ---------------------------------------------------------------------------------
 * h2v_shutdown(device) - device = -1: every device - quiesces and releases everything the library owns there: it waits
 * for the library's pool streams (the hardware queues the lanes run on), releases every live workspace of that device
 * (buffers, events, copy streams) and the device memory of every plan loaded on it, and destroys the pool streams.
 * Afterwards every entry point that needs that device returns H2V_E_DEVICE; workspace / plan handles stay valid as empty
 * shells (h2v_plan_info still answers) and are freed with the usual h2v_*_free.  Idempotent; not to be called while
 * another thread is inside a verify call.
 * Who calls it: a host calls it once, after its last verify call and before the process starts to exit - the Rust side in
 * the `Drop` of the object that owns the library, h2v.hpp through h2v::shutdown(), the Python binding
 * with atexit.  The reference's side is RAII throughout (the guard is consumed by value, examples/simple_mul.rs:98-104);
 * this is the one piece of process-wide state the backend adds.  As a backstop the library registers the call with
 * atexit() itself when it creates its first pool stream (i.e. after the HIP runtime has initialised, so that it runs
 * before the runtime's own exit handlers).  Why it exists: pool streams that were still alive when the HIP runtime and a
 * profiler's tool library ran their static destructors crashed the process at exit (SIGSEGV through __cxa_finalize under
 * rocprofv3, round 3). */
int h2v_shutdown(int device);

const char *h2v_last_error(void);
/* sha256 (hex) of the sources this binary was built from; "unknown" for a build outside __graft_entry__.build() */
const char *h2v_build_id(void);
int h2v_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
