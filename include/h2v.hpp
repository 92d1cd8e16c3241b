// C++ host-side mirror of the reference's verify interface for the hot path, header-only, over the C-ABI of h2v.h.
//
// The reference's toolchain (Rust) is absent from this image, so the layer a Rust maintainer would write above the
// FFI is given here in C++ with the reference's names and argument meaning:
//
//     let mut t = CircuitTranscript::<CardanoFriendlyBlake2b>::init_from_bytes(&proof);     // examples/simple_mul.rs:97
//     let guard = prepare(&vk, &[&[]], &[&[&instance]], &mut t)?;                            // examples/simple_mul.rs:98
//     guard.verify(&kzg_params.verifier_params())?;                                          // examples/simple_mul.rs:101
//
//     h2v::CircuitTranscript t = h2v::CircuitTranscript::init_from_bytes(proof);
//     h2v::Guard guard = h2v::prepare(vk, {}, {instance_scalars_le32}, t);                   // throws h2v::Error on misuse
//     guard.verify();                                                                        // throws h2v::VerifyError
//
// `VerifyingKey` wraps a plan: VerifyingKey::from_json(description) compiles one behind the C-ABI (h2v_plan_compile, the
// counterpart of extract_circuit, /root/reference/src/plutus_gen/extraction/mod.rs:31; the description is the JSON of
// docs/vk_schema.json), or it takes a blob made earlier (plutus_halo2_verifier_gen_amd.plan.compile_plan(vk).to_bytes()
// gives the same bytes).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "h2v.h"

namespace h2v {

struct Error : std::runtime_error {  // API misuse / device error (negative H2V_E_* codes)
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct VerifyError : std::runtime_error {  // Err(plonk::Error): the proof does not verify
    uint32_t status;                       // H2V_ST_* bits
    explicit VerifyError(uint32_t st) : std::runtime_error("proof rejected (status " + std::to_string(st) + ")"), status(st) {}
};
inline void check(int rc) {
    if (rc != H2V_OK) throw Error(rc, h2v_last_error());
}
/// h2v_shutdown: releases everything the library owns on `device` (-1: every device) - pool streams, workspaces, plans.
/// Call it once after the last verify call and before main() returns (or hold a ShutdownGuard in main): objects of this
/// header that are still alive afterwards are empty shells whose destructors only free host memory.
inline void shutdown(int device = -1) { check(h2v_shutdown(device)); }
struct ShutdownGuard {   // `h2v::ShutdownGuard guard;` as the first local of main(): runs after every other local is gone
    ShutdownGuard() = default;
    ShutdownGuard(const ShutdownGuard &) = delete;
    ShutdownGuard &operator=(const ShutdownGuard &) = delete;
    ~ShutdownGuard() { (void)h2v_shutdown(-1); }
};

class VerifyingKey {  // VerifyingKey<F, KZGCommitmentScheme<Bls12>> + ParamsVerifierKZG for this path
  public:
    VerifyingKey(const uint8_t *plan_blob, size_t len, int device = 0) { check(h2v_plan_load(plan_blob, len, device, &p_)); }
    /// from the verifying-key description (JSON, docs/vk_schema.json): h2v_plan_compile + h2v_plan_load, no Python in the loop
    static std::vector<uint8_t> compile(const std::string &vk_json) {
        uint8_t *blob = nullptr;
        size_t n = 0;
        check(h2v_plan_compile(vk_json.data(), vk_json.size(), &blob, &n));
        std::vector<uint8_t> out(blob, blob + n);
        h2v_blob_free(blob);
        return out;
    }
    static std::unique_ptr<VerifyingKey> from_json(const std::string &vk_json, int device = 0) {
        const std::vector<uint8_t> blob = compile(vk_json);
        return std::unique_ptr<VerifyingKey>(new VerifyingKey(blob.data(), blob.size(), device));
    }
    VerifyingKey(const VerifyingKey &) = delete;
    VerifyingKey &operator=(const VerifyingKey &) = delete;
    ~VerifyingKey() { h2v_plan_free(p_); }
    const h2v_plan *handle() const { return p_; }
    uint32_t proof_len() const { uint32_t v; check(h2v_plan_info(p_, &v, nullptr, nullptr, nullptr)); return v; }
    uint32_t n_public_inputs() const { uint32_t v; check(h2v_plan_info(p_, nullptr, &v, nullptr, nullptr)); return v; }
    uint32_t n_committed_instances() const { uint32_t v; check(h2v_plan_info(p_, nullptr, nullptr, &v, nullptr)); return v; }
    /// the transcript hash the key's proofs are made under (H2V_TRANSCRIPT_*), and its blake2b key (empty for the Cardano kind)
    uint32_t transcript_kind() const { uint32_t v; check(h2v_plan_transcript(p_, &v, nullptr, nullptr)); return v; }
    std::vector<uint8_t> transcript_key() const {
        uint8_t key[64];
        uint32_t n = 0;
        check(h2v_plan_transcript(p_, nullptr, key, &n));
        return std::vector<uint8_t>(key, key + n);
    }

  private:
    h2v_plan *p_ = nullptr;
};

// The H of the reference's CircuitTranscript<H>, as tag types.  The hash itself is a property of the verifying key (it is in
// the plan, h2v_plan_transcript) and runs on the GPU; the tag is what Rust's type parameter is: prepare() with a transcript
// whose H is not the key's throws h2v::Error(H2V_E_ARG) - misuse, where Rust does not compile - and never rejects.  A proof
// that was in fact made under another hash than its tag claims is rejected by the pairing like any other bad proof.
struct CardanoFriendlyBlake2b { static constexpr uint32_t kind = H2V_TRANSCRIPT_CARDANO_BLAKE2B_256; };   // adjusted_types/mod.rs:30-72
struct Blake2b512 { static constexpr uint32_t kind = H2V_TRANSCRIPT_BLAKE2B_512; };                       // blake2b_simd::State
// Transcript<H> is CircuitTranscript<H>; `CircuitTranscript` itself stays the name of the Cardano instantiation, as every
// caller written before there was a choice spells it (a C++ name cannot be a class and a template at once).
template <class H>
class Transcript {  // verifier-side transcript: a cursor over the proof bytes (hashing happens on the GPU)
  public:
    typedef H Hash;
    static Transcript init_from_bytes(std::vector<uint8_t> proof) { return Transcript(std::move(proof)); }
    const std::vector<uint8_t> &bytes() const { return proof_; }
    void mark_consumed(size_t n) { consumed_ = n; }
    void assert_empty() const {  // examples/ivc.rs:92-94
        if (consumed_ != proof_.size()) throw VerifyError(0);
    }

  private:
    explicit Transcript(std::vector<uint8_t> p) : proof_(std::move(p)) {}
    std::vector<uint8_t> proof_;
    size_t consumed_ = 0;
};
using CircuitTranscript = Transcript<CardanoFriendlyBlake2b>;
using CircuitTranscriptBlake2b512 = Transcript<Blake2b512>;

// The collapsed DualMSM of one proof: the two points of its final pairing check e(left, s_g2) == e(right, G2), 48-byte
// compressed each (h2v_prepare_batch).  check() runs that pairing (h2v_check_pairs).
struct DualMSM {
    uint8_t left[48], right[48];
    bool check(const VerifyingKey &vk) const {
        uint8_t pair[96], acc = 0;
        for (int k = 0; k < 48; k++) { pair[k] = left[k]; pair[48 + k] = right[k]; }
        h2v::check(h2v_check_pairs(vk.handle(), 1, pair, &acc, nullptr, nullptr));
        return acc != 0;
    }
};

class Guard {  // CS::VerificationGuard: consumed by verify() (Guard::verify), check() (DualMSM::check) or dual_msm()
  public:
    Guard(const VerifyingKey &vk, std::vector<uint8_t> proof, std::vector<uint8_t> instances, std::vector<uint8_t> committed)
        : vk_(vk), proof_(std::move(proof)), inst_(std::move(instances)), ci_(std::move(committed)) {}
    void verify() {
        const uint32_t st = run();
        if (st) throw VerifyError(st);
    }
    bool check() { return run() == 0; }
    /// the proof's pair (h2v_prepare_batch with n = 1); throws VerifyError for a proof rejected before the pairing
    DualMSM dual_msm() {
        if (used_) throw Error(H2V_E_ARG, "guard already consumed");
        used_ = true;
        const uint64_t off[2] = {0, proof_.size()};
        const h2v_batch b = {1, proof_.data(), off, inst_.empty() ? nullptr : inst_.data(), ci_.empty() ? nullptr : ci_.data()};
        uint8_t pair[96];
        uint32_t st = 0;
        h2v::check(h2v_prepare_batch(vk_.handle(), &b, pair, &st, nullptr));
        if (st) throw VerifyError(st);
        DualMSM m;
        for (int k = 0; k < 48; k++) { m.left[k] = pair[k]; m.right[k] = pair[48 + k]; }
        return m;
    }

  private:
    uint32_t run() {
        if (used_) throw Error(H2V_E_ARG, "guard already consumed");
        used_ = true;
        uint32_t st = 0;
        uint8_t acc = 0;
        h2v::check(h2v_trace(vk_.handle(), proof_.data(), proof_.size(), inst_.empty() ? nullptr : inst_.data(),
                             ci_.empty() ? nullptr : ci_.data(), nullptr, nullptr, nullptr, nullptr, &st, &acc));
        return acc ? 0u : (st ? st : H2V_ST_PAIRING);
    }
    const VerifyingKey &vk_;
    std::vector<uint8_t> proof_, inst_, ci_;
    bool used_ = false;
};

// prepare(&vk, committed_instances, instances, &mut transcript): committed = 0 or 1 compressed G1 (48 B),
// instances = the public-input scalars of the single public column, 32 B little-endian each.
template <class H>
inline Guard prepare(const VerifyingKey &vk, const std::vector<std::vector<uint8_t>> &committed_instances,
                     const std::vector<std::vector<uint8_t>> &instances, Transcript<H> &transcript) {
    if (vk.transcript_kind() != H::kind) throw Error(H2V_E_ARG, "transcript hash mismatch: the verifying key's proofs are made under another hash than this transcript's");
    if (instances.size() != vk.n_public_inputs()) throw Error(H2V_E_ARG, "wrong number of public inputs");
    if (committed_instances.size() != vk.n_committed_instances()) throw Error(H2V_E_ARG, "wrong number of committed instances");
    std::vector<uint8_t> inst, ci;
    for (const auto &s : instances) {
        if (s.size() != 32) throw Error(H2V_E_ARG, "instance scalars are 32 bytes little-endian");
        inst.insert(inst.end(), s.begin(), s.end());
    }
    for (const auto &c : committed_instances) {
        if (c.size() != 48) throw Error(H2V_E_ARG, "committed instances are 48-byte compressed G1");
        ci.insert(ci.end(), c.begin(), c.end());
    }
    transcript.mark_consumed(vk.proof_len());
    return Guard(vk, transcript.bytes(), std::move(inst), std::move(ci));
}

// The batched form the hardware wants: accept[i] for n independent proofs (host buffers).
inline std::vector<uint8_t> verify_batch(const VerifyingKey &vk, const h2v_batch &batch, h2v_workspace *ws = nullptr) {
    std::vector<uint8_t> accept(batch.n);
    check(h2v_verify_batch(vk.handle(), &batch, accept.data(), ws));
    return accept;
}
// The two halves of verify_batch: prepare_batch returns every proof's pair compress(L) || compress(R) (96 bytes; zero for a
// proof rejected before the pairing, whose status word says why) and check_pairs runs the pairing on pairs from anywhere.
// check_pairs(vk, prepare_batch(vk, b).pairs).accept == verify_batch(vk, b).
struct PreparedBatch {
    std::vector<uint8_t> pairs;    // n x 96
    std::vector<uint32_t> status;  // H2V_ST_* bits without H2V_ST_PAIRING
};
inline PreparedBatch prepare_batch(const VerifyingKey &vk, const h2v_batch &batch, h2v_workspace *ws = nullptr) {
    PreparedBatch r{std::vector<uint8_t>(batch.n * 96), std::vector<uint32_t>(batch.n)};
    check(h2v_prepare_batch(vk.handle(), &batch, r.pairs.data(), r.status.data(), ws));
    return r;
}
struct PairVerdicts {
    std::vector<uint8_t> accept;
    std::vector<uint32_t> status;  // H2V_ST_BAD_POINT / H2V_ST_PAIRING
};
inline PairVerdicts check_pairs(const VerifyingKey &vk, const std::vector<uint8_t> &pairs, h2v_workspace *ws = nullptr) {
    if (pairs.size() % 96) throw Error(H2V_E_ARG, "pairs: a multiple of 96 bytes");
    const uint64_t n = pairs.size() / 96;
    PairVerdicts r{std::vector<uint8_t>(n), std::vector<uint32_t>(n)};
    check(h2v_check_pairs(vk.handle(), n, pairs.data(), r.accept.data(), r.status.data(), ws));
    return r;
}
// check_pairs with ONE pairing for the batch (h2v_check_pairs_rlc): the reference's "scale each DualMSM by a random coefficient,
// add, check once" (examples/ivc.rs:85-96).  The same accept / status as check_pairs; fell_back (optional): the batch check
// failed and the per-pair kernels produced them.  seed: 32 bytes that provers cannot predict, or nullptr = drawn from the OS.
// derive_seed (H2V_RLC_SEED_TRANSCRIPT; not beside `seed`): the seed is a digest of the key and the pairs - nothing is drawn.
inline PairVerdicts check_pairs_rlc(const VerifyingKey &vk, const std::vector<uint8_t> &pairs, h2v_workspace *ws = nullptr,
                                    const uint8_t *seed = nullptr, bool *fell_back = nullptr, bool derive_seed = false) {
    if (pairs.size() % 96) throw Error(H2V_E_ARG, "pairs: a multiple of 96 bytes");
    const uint64_t n = pairs.size() / 96;
    PairVerdicts r{std::vector<uint8_t>(n), std::vector<uint32_t>(n)};
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    if (derive_seed) opts.flags |= H2V_RLC_SEED_TRANSCRIPT;
    int fb = 0;
    check(h2v_check_pairs_rlc(vk.handle(), n, pairs.data(), r.accept.data(), r.status.data(), ws, (seed || derive_seed) ? &opts : nullptr, &fb));
    if (fell_back) *fell_back = fb != 0;
    return r;
}
// ONE check over pairs on SEVERAL SRS (h2v_check_pairs_multi; at most H2V_MULTI_SRS_MAX ranges): the first counts[0] pairs are
// checked against the SRS of *vks[0], the next counts[1] against *vks[1], and so on - C + 1 Miller loops under one final
// exponentiation when every equation holds.  accept / status: position for position what check_pairs(*vks[k], ...) gives for
// range k.  fell_back (optional): the check failed and the per-pair kernels produced them.  seed: as check_pairs_rlc.
inline PairVerdicts check_pairs_multi(const std::vector<const VerifyingKey *> &vks, const std::vector<uint64_t> &counts, const std::vector<uint8_t> &pairs,
                                      h2v_workspace *ws = nullptr, const uint8_t *seed = nullptr, bool *fell_back = nullptr) {
    if (vks.size() != counts.size()) throw Error(H2V_E_ARG, "counts: one entry per key");
    uint64_t n = 0;
    for (uint64_t c : counts) n += c;
    if (pairs.size() != n * 96) throw Error(H2V_E_ARG, "pairs: 96 bytes per pair, sum(counts) pairs");
    std::vector<const h2v_plan *> plans;
    for (const VerifyingKey *vk : vks) plans.push_back(vk ? vk->handle() : nullptr);
    PairVerdicts r{std::vector<uint8_t>(n), std::vector<uint32_t>(n)};
    const uint8_t none = 0;
    uint8_t acc0 = 0;
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    int fb = 0;
    check(h2v_check_pairs_multi(plans.data(), (uint32_t)plans.size(), counts.data(), n ? pairs.data() : &none, n ? r.accept.data() : &acc0, r.status.data(), ws,
                                seed ? &opts : nullptr, &fb));
    if (fell_back) *fell_back = fb != 0;
    return r;
}
// The same vector through the batch-accept fast path (one random linear combination of the batch's pairing equations:
// one bucketed G1 MSM + one pairing; the per-proof kernels only if the batch check fails).  fell_back (optional) tells
// which of the two produced the vector.  seed: 32 bytes that provers cannot predict, or nullptr = drawn from the OS.
// derive_seed (H2V_RLC_SEED_TRANSCRIPT; not beside `seed`): the seed is a digest of the key and the batch (h2v.h has the rule):
// nothing is drawn, nothing has to be kept from the provers, and the call is reproducible.
inline std::vector<uint8_t> verify_batch_rlc(const VerifyingKey &vk, const h2v_batch &batch, h2v_workspace *ws = nullptr,
                                             bool *fell_back = nullptr, const uint8_t *seed = nullptr, bool fold_pairs = false,
                                             bool derive_seed = false) {
    std::vector<uint8_t> accept(batch.n);
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    if (fold_pairs) opts.flags |= H2V_RLC_FOLD_PAIRS;   // recursive keys: combine the pairs the fold leaves (ignored by other keys)
    if (derive_seed) opts.flags |= H2V_RLC_SEED_TRANSCRIPT;
    int fb = 0;
    check(h2v_verify_batch_rlc(vk.handle(), &batch, accept.data(), ws, (seed || fold_pairs || derive_seed) ? &opts : nullptr, &fb));
    if (fell_back) *fell_back = fb != 0;
    return accept;
}
// Mixed-key batches (h2v_verify_mixed): proof i of `batch` belongs to vks[batch.plan_of[i]]; every listed key must be on ONE
// SRS (otherwise Error(H2V_E_ARG) naming two keys: a host with several SRS makes one call per SRS).  accept / status in the
// caller's order, exactly the per-key verify call's.  rlc: ONE pairing for the call - the same vectors up to a 2^-128
// soundness error over the seed (32 bytes that provers cannot predict, or nullptr = drawn from the OS); fell_back (optional):
// that batch check failed and the per-pair kernels produced them.  fold_msm (only with rlc; H2V_MIXED_FOLD_MSM): ONE bucket MSM
// over the call's per-proof terms as well; a failed check runs the call again without it (fell_back).  grouped (only with
// fold_msm; H2V_MIXED_GROUPED): phase 1 of every key in one launch per kernel, up to H2V_MIXED_GROUPED_MAX_PLANS keys - many keys
// with few proofs each; the same vectors.  ws: one made for the same keys or a superset (Workspace(vks, max_batch)), or nullptr
// for a temporary one.  keyed_seed (only with rlc, not beside `seed`; H2V_RLC_SEED_KEYED): nothing is drawn - the seed is a digest
// of the call in which every leaf binds the key of its own proof (h2v.h has the rule), the same whatever fold_msm / grouped say.
// across_srs (only with rlc; H2V_MIXED_ACROSS_SRS): the listed keys may be on several SRS - at most H2V_MULTI_SRS_MAX of them with
// proofs - and the call ends in ONE multi-pairing; the same vectors.
inline PairVerdicts verify_mixed(const std::vector<const VerifyingKey *> &vks, const h2v_mixed_batch &batch, h2v_workspace *ws = nullptr,
                                 bool rlc = false, const uint8_t *seed = nullptr, bool *fell_back = nullptr, bool fold_msm = false,
                                 bool grouped = false, bool keyed_seed = false, bool across_srs = false) {
    std::vector<const h2v_plan *> plans;
    for (const VerifyingKey *k : vks) plans.push_back(k ? k->handle() : nullptr);
    PairVerdicts r{std::vector<uint8_t>(batch.n), std::vector<uint32_t>(batch.n)};
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    if (keyed_seed) opts.flags |= H2V_RLC_SEED_KEYED;
    int fb = 0;
    check(h2v_verify_mixed(plans.data(), (uint32_t)plans.size(), &batch, r.accept.data(), r.status.data(), ws,
                           (rlc ? H2V_MIXED_RLC : 0u) | (fold_msm ? H2V_MIXED_FOLD_MSM : 0u) | (grouped ? H2V_MIXED_GROUPED : 0u) |
                               (across_srs ? H2V_MIXED_ACROSS_SRS : 0u),
                           (seed || keyed_seed) ? &opts : nullptr, &fb));
    if (fell_back) *fell_back = fb != 0;
    return r;
}
// midnight_zk_stdlib::batch_verify(&params, &vks, &instances, &proofs) (src/circuits/schnorr_circuit.rs:223-231): one call and
// one final check for a list of (vk, instances, proof) triples on one SRS.  Throws VerifyError (with the first rejected proof's
// status) unless every proof is accepted.  across_srs: the list may span several SRS (verify_mixed), still one final check.
inline void batch_verify(const std::vector<const VerifyingKey *> &vks, const h2v_mixed_batch &batch, h2v_workspace *ws = nullptr,
                         bool fold_msm = false, bool grouped = false, bool keyed_seed = false, bool across_srs = false) {
    const PairVerdicts r = verify_mixed(vks, batch, ws, true, nullptr, nullptr, fold_msm, grouped, keyed_seed, across_srs);
    for (uint64_t i = 0; i < batch.n; i++)
        if (!r.accept[i]) throw VerifyError(r.status[i]);
}
// Aggregate calls (h2v_aggregate_batch / h2v_aggregate_mixed): the batch's ONE pair compress(L) || compress(R), L = sum r_i L_i and
// R = sum r_i R_i over the included proofs, instead of a pairing on it - the reference's `dual_msm.scale(r)` / `acc.add_msm(..)`;
// check_pairs(_rlc) is its `check`.  included[i] = 1: proof i was not rejected before the pairing (NOT a verdict: it is accepted
// iff the pair's equation holds); status as prepare_batch; info: the seed and chunking the coefficients follow.  seed: 32 bytes
// that provers cannot predict, or nullptr = drawn from the OS.  grouped (aggregate_mixed; H2V_RLC_GROUPED): phase 1 as
// verify_mixed(.., grouped) runs it - the same pair.  keyed_seed (aggregate_mixed; H2V_RLC_SEED_KEYED, not beside `seed`):
// H2V_AGGREGATE_SEED_SOURCE(&info) = 1 and info.seed_used is the digest of the call with keyed leaves.
struct Aggregate {
    uint8_t pair[96];
    std::vector<uint8_t> included;
    std::vector<uint32_t> status;
    h2v_aggregate_info info;
};
// derive_seed (aggregate_batch; H2V_RLC_SEED_TRANSCRIPT): H2V_AGGREGATE_SEED_SOURCE(&info) = 1 and info.seed_used is a digest of
// the key and the batch, so that anyone who holds the same inputs recomputes the same pair.
inline Aggregate aggregate_batch(const VerifyingKey &vk, const h2v_batch &batch, h2v_workspace *ws = nullptr, const uint8_t *seed = nullptr,
                                 bool derive_seed = false) {
    Aggregate r{{}, std::vector<uint8_t>(batch.n ? batch.n : 1), std::vector<uint32_t>(batch.n ? batch.n : 1), {}};
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    if (derive_seed) opts.flags |= H2V_RLC_SEED_TRANSCRIPT;
    check(h2v_aggregate_batch(vk.handle(), &batch, r.pair, r.included.data(), r.status.data(), ws, (seed || derive_seed) ? &opts : nullptr, &r.info));
    r.included.resize(batch.n); r.status.resize(batch.n);
    return r;
}
inline Aggregate aggregate_mixed(const std::vector<const VerifyingKey *> &vks, const h2v_mixed_batch &batch, h2v_workspace *ws = nullptr,
                                 const uint8_t *seed = nullptr, bool grouped = false, bool keyed_seed = false) {
    std::vector<const h2v_plan *> plans;
    for (const VerifyingKey *k : vks) plans.push_back(k ? k->handle() : nullptr);
    Aggregate r{{}, std::vector<uint8_t>(batch.n ? batch.n : 1), std::vector<uint32_t>(batch.n ? batch.n : 1), {}};
    h2v_rlc_opts opts{};
    if (seed) { for (int k = 0; k < 32; k++) opts.seed[k] = seed[k]; opts.flags = H2V_RLC_SEED_GIVEN; }
    if (grouped) opts.flags |= H2V_RLC_GROUPED;
    if (keyed_seed) opts.flags |= H2V_RLC_SEED_KEYED;
    check(h2v_aggregate_mixed(plans.data(), (uint32_t)plans.size(), &batch, r.pair, r.included.data(), r.status.data(), ws,
                              (seed || grouped || keyed_seed) ? &opts : nullptr, &r.info));
    r.included.resize(batch.n); r.status.resize(batch.n);
    return r;
}
// Collects the pairs of several calls - keys of ONE SRS - and checks them ONCE (examples/ivc.rs:85-96, 195-208: scale, add_msm,
// then one `check`).  push() aggregates a call and keeps its pair, included[] and a COPY of its inputs; finish() checks the K pairs
// with one pairing (check_pairs_rlc; check_pairs for K = 1): a call whose pair passes gets accept = included, a call whose pair
// fails is verified per proof (verify_batch) on the kept inputs.  Same semantics as api.Aggregator (there `params` names the SRS).  finish() returns the per-call accept vectors in push order and
// fills `reverified` with the indices of the calls verified again.  The keys must outlive the Aggregator; keep it inside one trust
// domain (a pair is only worth what the seed of its call is).  push_mixed() aggregates a call over several keys
// (aggregate_mixed; Aggregator(true): its grouped form) and is verified again, if its pair fails, with verify_mixed.
class Aggregator {
  public:
    /// derive_seed: every push derives its seed from its key and batch; single-key pushes only (push_mixed: Error(H2V_E_ARG)).
    /// keyed_seed: every push derives by the mixed calls' rule (H2V_RLC_SEED_KEYED) - push_mixed derives, and a single-key push goes
    /// out as a one-plan mixed call, so that every pair of the aggregator follows one rule.  Both: Error(H2V_E_ARG).
    explicit Aggregator(bool grouped = false, bool derive_seed = false, bool keyed_seed = false)
        : grouped_(grouped), derive_seed_(derive_seed), keyed_seed_(keyed_seed) {
        if (derive_seed && keyed_seed) throw Error(H2V_E_ARG, "Aggregator: derive_seed and keyed_seed exclude each other");
    }
    Aggregator(const Aggregator &) = delete;
    Aggregator &operator=(const Aggregator &) = delete;
    /// one SRS per Aggregator - that of the first key pushed: a key on another SRS is Error(H2V_E_ARG), before anything runs
    size_t push(const VerifyingKey &vk, const h2v_batch &b, const uint8_t *seed = nullptr) {
        if (keyed_seed_) {      // (a one-plan mixed call: the aggregator's one rule)
            const std::vector<uint32_t> plan_of(b.n ? b.n : 1, 0u);
            const h2v_mixed_batch mb = {b.n, plan_of.data(), b.proofs, b.proof_off, b.instances, b.committed};
            return push_mixed({&vk}, mb, seed);
        }
        if (!srs_) srs_ = &vk;
        const int same = h2v_plan_same_srs(srs_->handle(), vk.handle());
        if (same < 0) check(same);
        if (same != 1) throw Error(H2V_E_ARG, "Aggregator: this key is on another SRS than the keys pushed before (s_g2 differs)");
        Call c;
        c.vk = &vk;
        const Aggregate a = aggregate_batch(vk, b, nullptr, seed, derive_seed_);
        for (int k = 0; k < 96; k++) c.pair[k] = a.pair[k];
        c.included = a.included;
        c.off.assign(b.proof_off, b.proof_off + b.n + 1);
        const uint64_t base = c.off[0];
        for (uint64_t &o : c.off) o -= base;
        c.proofs.assign(b.proofs + base, b.proofs + base + c.off[b.n]);
        if (b.instances) c.inst.assign(b.instances, b.instances + b.n * 32 * vk.n_public_inputs());
        if (b.committed && vk.n_committed_instances()) c.ci.assign(b.committed, b.committed + b.n * 48);
        calls_.push_back(std::move(c));
        return calls_.size() - 1;
    }
    size_t push_mixed(const std::vector<const VerifyingKey *> &vks, const h2v_mixed_batch &b, const uint8_t *seed = nullptr) {
        if (derive_seed_) throw Error(H2V_E_ARG, "Aggregator: derive_seed takes single-key pushes only (the mixed calls have no derived seed)");
        if (vks.empty() || !vks[0]) throw Error(H2V_E_ARG, "Aggregator: no key");
        if (!srs_) srs_ = vks[0];
        for (const VerifyingKey *k : vks) {
            const int same = k ? h2v_plan_same_srs(srs_->handle(), k->handle()) : 0;
            if (same < 0) check(same);
            if (same != 1) throw Error(H2V_E_ARG, "Aggregator: this key is on another SRS than the keys pushed before (s_g2 differs)");
        }
        Call c;
        c.vk = vks[0];
        c.vks = vks;
        const Aggregate a = aggregate_mixed(vks, b, nullptr, seed, grouped_, keyed_seed_);
        for (int k = 0; k < 96; k++) c.pair[k] = a.pair[k];
        c.included = a.included;
        c.plan_of.assign(b.plan_of, b.plan_of + b.n);
        c.off.assign(b.proof_off, b.proof_off + b.n + 1);
        const uint64_t base = c.off[0];
        for (uint64_t &o : c.off) o -= base;
        c.proofs.assign(b.proofs + base, b.proofs + base + c.off[b.n]);
        uint64_t n_inst = 0, n_ci = 0;
        for (uint64_t i = 0; i < b.n; i++) { n_inst += 32ull * vks[b.plan_of[i]]->n_public_inputs(); n_ci += vks[b.plan_of[i]]->n_committed_instances() ? 48 : 0; }
        if (b.instances) c.inst.assign(b.instances, b.instances + n_inst);
        if (b.committed) c.ci.assign(b.committed, b.committed + n_ci);
        calls_.push_back(std::move(c));
        return calls_.size() - 1;
    }
    std::vector<std::vector<uint8_t>> finish(std::vector<size_t> *reverified = nullptr, const uint8_t *seed = nullptr) {
        std::vector<Call> calls;
        calls.swap(calls_);
        std::vector<std::vector<uint8_t>> out;
        if (reverified) reverified->clear();
        if (calls.empty()) return out;
        std::vector<uint8_t> pairs;
        for (const Call &c : calls) pairs.insert(pairs.end(), c.pair, c.pair + 96);
        const PairVerdicts v = calls.size() > 1 ? check_pairs_rlc(*calls[0].vk, pairs, nullptr, seed) : check_pairs(*calls[0].vk, pairs);
        for (size_t k = 0; k < calls.size(); k++) {
            const Call &c = calls[k];
            if (v.accept[k]) { out.push_back(c.included); continue; }
            if (reverified) reverified->push_back(k);
            if (!c.vks.empty()) {
                const h2v_mixed_batch mb{c.included.size(), c.plan_of.data(), c.proofs.data(), c.off.data(), c.inst.empty() ? nullptr : c.inst.data(),
                                         c.ci.empty() ? nullptr : c.ci.data()};
                out.push_back(verify_mixed(c.vks, mb).accept);
                continue;
            }
            const h2v_batch b{c.included.size(), c.proofs.data(), c.off.data(), c.inst.empty() ? nullptr : c.inst.data(), c.ci.empty() ? nullptr : c.ci.data()};
            out.push_back(verify_batch(*c.vk, b));
        }
        return out;
    }

  private:
    struct Call {
        const VerifyingKey *vk = nullptr;
        uint8_t pair[96];
        std::vector<uint8_t> included, proofs, inst, ci;
        std::vector<uint64_t> off;
        std::vector<const VerifyingKey *> vks;   // push_mixed: the call's keys and plan_of
        std::vector<uint32_t> plan_of;
    };
    std::vector<Call> calls_;
    const VerifyingKey *srs_ = nullptr;
    bool grouped_ = false, derive_seed_ = false, keyed_seed_ = false;
};

// A reusable workspace, and the streaming form: submit() returns once the batch is copied and everything is enqueued,
// wait() collects the accept vector.  Alternate two Workspaces to overlap the upload of one batch with the kernels of the
// previous one.
// (A Workspace, BatchStream or NodeStream keeps a reference to its VerifyingKey: the key must outlive it.)
class Workspace {
  public:
    Workspace(const VerifyingKey &vk, uint64_t max_batch) : vk_(vk) { check(h2v_workspace_create(vk.handle(), max_batch, &w_)); }
    /// a LANED workspace (h2v_workspace_create_lanes): calls are cut into chunks that the library pipelines through its own
    /// lanes and streams; n_lanes / chunk = 0: the library's choice
    Workspace(const VerifyingKey &vk, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk) : vk_(vk) {
        check(h2v_workspace_create_lanes(vk.handle(), max_batch, n_lanes, chunk, &w_));
    }
    /// ONE laned workspace for several keys of one device (h2v_workspace_create_multi: lanes sized for the largest of every
    /// dimension); submit(vk, batch) names the key of each batch, submit(batch) means the first key
    Workspace(const std::vector<const VerifyingKey *> &vks, uint64_t max_batch, uint32_t n_lanes = 0, uint32_t chunk = 0) : vk_(*vks.at(0)) {
        std::vector<const h2v_plan *> ps;
        for (const VerifyingKey *k : vks) ps.push_back(k->handle());
        check(h2v_workspace_create_multi(ps.data(), (uint32_t)ps.size(), max_batch, n_lanes, chunk, &w_));
    }
    Workspace(const Workspace &) = delete;
    Workspace &operator=(const Workspace &) = delete;
    ~Workspace() { h2v_workspace_free(w_); }
    h2v_workspace *handle() const { return w_; }
    const VerifyingKey &vk() const { return vk_; }
    /// tuning hint (h2v_workspace_hint_in_flight): the caller keeps n batches in flight, one workspace each; never changes results
    void hint_in_flight(uint32_t n) { check(h2v_workspace_hint_in_flight(w_, n)); }
    /// calls of n proofs the workspace keeps in flight before a call waits for a lane (h2v_workspace_depth)
    uint32_t depth(uint64_t n, bool rlc = false) const {
        uint32_t d = 1;
        check(h2v_workspace_depth(w_, n, rlc ? 1 : 0, &d));
        return d;
    }
    void submit(const h2v_batch &batch, bool rlc = false) { submit(vk_, batch, rlc); }
    void submit(const VerifyingKey &vk, const h2v_batch &batch, bool rlc = false) {
        check(h2v_verify_batch_submit(vk.handle(), &batch, w_, rlc ? H2V_SUBMIT_RLC : 0u, nullptr));
        n_ = batch.n;
    }
    std::vector<uint8_t> wait(bool *fell_back = nullptr) {
        std::vector<uint8_t> accept(n_ ? n_ : 1);
        int fb = 0;
        check(h2v_verify_batch_wait(w_, accept.data(), &fb));
        accept.resize(n_);
        if (fell_back) *fell_back = fb != 0;
        return accept;
    }

  private:
    const VerifyingKey &vk_;
    h2v_workspace *w_ = nullptr;
    uint64_t n_ = 0;
};

// A verifier that keeps up to `depth` host-buffer batches in flight on ONE laned workspace (`depth` lanes, one chunk per
// batch): push() hands a batch over (its host buffers may be reused at once) and, once `depth` batches are in flight,
// returns the accept vector of the OLDEST; drain() collects the rest in order.  depth 6 (per proof) / 11-16 (RLC) reach the
// device-resident throughput on one MI355X (tools/bench_host_path.py).  Every batch must fit `max_batch`.  (Round 2 needed
// `depth` workspaces for this.)
class BatchStream {
  public:
    BatchStream(const VerifyingKey &vk, uint64_t max_batch, unsigned depth, bool rlc = false)
        : depth_(depth), rlc_(rlc), ws_(vk, max_batch, depth == 0 || depth > 16 ? 1u : depth, (uint32_t)max_batch) {
        if (depth == 0 || depth > 16) throw Error(H2V_E_ARG, "BatchStream: depth must be 1 .. 16 (a laned workspace has at most 16 lanes)");
    }
    BatchStream(const BatchStream &) = delete;
    BatchStream &operator=(const BatchStream &) = delete;
    /// returns true and fills `done` when the oldest batch in flight has been collected (`depth` were in flight)
    bool push(const h2v_batch &batch, std::vector<uint8_t> *done = nullptr) {
        bool have = false;
        if (sizes_.size() >= depth_) {
            std::vector<uint8_t> acc = collect();
            if (done) *done = std::move(acc);
            have = true;
        }
        check(h2v_verify_batch_submit(ws_.vk().handle(), &batch, ws_.handle(), rlc_ ? H2V_SUBMIT_RLC : 0u, nullptr));
        sizes_.push_back(batch.n);
        return have;
    }
    /// accept vectors of the batches still in flight, oldest first
    std::vector<std::vector<uint8_t>> drain() {
        std::vector<std::vector<uint8_t>> out;
        while (!sizes_.empty()) out.push_back(collect());
        return out;
    }

  private:
    std::vector<uint8_t> collect() {
        std::vector<uint8_t> accept(sizes_.front() ? sizes_.front() : 1);
        int fb = 0;
        check(h2v_verify_batch_wait(ws_.handle(), accept.data(), &fb));
        accept.resize(sizes_.front());
        sizes_.pop_front();
        return accept;
    }
    unsigned depth_;
    bool rlc_;
    Workspace ws_;
    std::deque<uint64_t> sizes_;
};

// Every GPU of one node behind one object, in ONE process (proofs are independent, so a batch is
// cut into contiguous index ranges [g n / G, (g + 1) n / G), one per device; the plan is replicated; nothing is exchanged
// but the accept bytes, which come back through each device's own pinned staging buffer).  Per device: its own
// VerifyingKey (plan upload), a BatchStream of `depth` workspaces and a host thread that stages and submits that device's
// shard, so the shards of one batch are packed and uploaded side by side.  push() / drain() as BatchStream; verify() is
// the blocking form.  The same device may be listed more than once (two pipelines on one GPU: how the GPU test runs on a
// one-GPU box).
class NodeStream {
  public:
    NodeStream(const uint8_t *plan_blob, size_t len, const std::vector<int> &devices, uint64_t max_batch_per_device, unsigned depth,
               bool rlc = false) {
        if (devices.empty() || depth == 0) throw Error(H2V_E_ARG, "NodeStream: at least one device and depth >= 1");
        for (int dev : devices) {
            std::unique_ptr<Dev> d(new Dev());
            d->vk.reset(new VerifyingKey(plan_blob, len, dev));
            d->bs.reset(new BatchStream(*d->vk, max_batch_per_device, depth, rlc));
            devs_.push_back(std::move(d));
        }
        for (auto &d : devs_) d->worker = std::thread([dp = d.get()] { dp->run(); });
    }
    ~NodeStream() {
        for (auto &d : devs_) { { std::lock_guard<std::mutex> l(d->mu); d->stop = true; } d->cv.notify_all(); }
        for (auto &d : devs_) if (d->worker.joinable()) d->worker.join();
    }
    NodeStream(const NodeStream &) = delete;
    NodeStream &operator=(const NodeStream &) = delete;
    size_t n_devices() const { return devs_.size(); }
    /// shard g of n proofs: the contiguous range [lo, hi)  (plutus_halo2_verifier_gen_amd/shard.py: shard_range)
    static std::pair<uint64_t, uint64_t> shard_range(uint64_t n, size_t g, size_t G) { return {n * g / G, n * (g + 1) / G}; }
    /// hands a batch over (the caller's buffers may be reused when this returns); true + `done` = the accept vector of the
    /// batch pushed `depth` calls earlier, reassembled in proof order
    bool push(const h2v_batch &b, std::vector<uint8_t> *done = nullptr) {
        const size_t G = devs_.size();
        const uint32_t n_pi = devs_[0]->vk->n_public_inputs(), n_ci = devs_[0]->vk->n_committed_instances();
        for (size_t g = 0; g < G; g++) {
            const auto r = shard_range(b.n, g, G);
            Dev &d = *devs_[g];
            Job j;
            j.n = r.second - r.first;
            // offsets rebased to the shard's first byte, so that only the shard's bytes travel to its device
            j.off.resize(j.n + 1);
            for (uint64_t i = 0; i <= j.n; i++) j.off[i] = b.proof_off[r.first + i] - b.proof_off[r.first];
            j.proofs = b.proofs + b.proof_off[r.first];
            j.inst = b.instances ? b.instances + r.first * n_pi * 32 : nullptr;
            j.ci = (b.committed && n_ci) ? b.committed + r.first * 48 : nullptr;
            { std::lock_guard<std::mutex> l(d.mu); d.jobs.push_back(std::move(j)); d.staged = false; }
            d.cv.notify_all();
        }
        bool have = true;
        std::string err;
        for (auto &d : devs_) {   // until every device has staged its shard (then the caller's buffers are free again)
            std::unique_lock<std::mutex> l(d->mu);
            d->cv.wait(l, [&] { return d->staged; });
            if (!d->error.empty()) err = d->error;
            have = have && !d->results.empty();
        }
        if (!err.empty()) throw Error(H2V_E_DEVICE, err);
        sizes_.push_back(b.n);
        if (have && done) *done = collect();
        else if (have) (void)collect();
        return have;
    }
    std::vector<std::vector<uint8_t>> drain() {
        for (auto &d : devs_) {
            { std::lock_guard<std::mutex> l(d->mu); d->drain = true; d->staged = false; }
            d->cv.notify_all();
        }
        for (auto &d : devs_) {
            std::unique_lock<std::mutex> l(d->mu);
            d->cv.wait(l, [&] { return d->staged; });
            if (!d->error.empty()) throw Error(H2V_E_DEVICE, d->error);
        }
        std::vector<std::vector<uint8_t>> out;
        while (!sizes_.empty()) out.push_back(collect());
        return out;
    }
    std::vector<uint8_t> verify(const h2v_batch &b) {
        if (!sizes_.empty()) throw Error(H2V_E_ARG, "NodeStream::verify with batches in flight: drain() first");
        push(b);
        return drain().at(0);
    }

  private:
    struct Job { uint64_t n = 0; std::vector<uint64_t> off; const uint8_t *proofs = nullptr, *inst = nullptr, *ci = nullptr; };
    struct Dev {
        std::unique_ptr<VerifyingKey> vk;
        std::unique_ptr<BatchStream> bs;
        std::thread worker;
        std::mutex mu;
        std::condition_variable cv;
        std::deque<Job> jobs;
        std::deque<std::vector<uint8_t>> results;
        bool stop = false, drain = false, staged = true;
        std::string error;
        void run() {
            for (;;) {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return stop || drain || !jobs.empty(); });
                if (stop) return;
                try {
                    if (!jobs.empty()) {
                        Job j = std::move(jobs.front());
                        jobs.pop_front();
                        l.unlock();
                        std::vector<uint8_t> done;
                        bool have = false;
                        if (j.n) {
                            const h2v_batch sb{j.n, j.proofs, j.off.data(), j.inst, j.ci};
                            have = bs->push(sb, &done);
                        } else {
                            have = pending_empty_push(&done);
                        }
                        l.lock();
                        if (have) results.push_back(std::move(done));
                    } else {   // drain
                        l.unlock();
                        std::vector<std::vector<uint8_t>> rest = bs->drain();
                        l.lock();
                        for (auto &v : rest) results.push_back(std::move(v));
                        drain = false;
                    }
                } catch (const std::exception &e) {
                    if (!l.owns_lock()) l.lock();
                    error = e.what();
                    drain = false;
                }
                staged = true;
                l.unlock();
                cv.notify_all();
            }
        }
        // (a device whose shard is empty - fewer proofs than devices - still takes part in the lockstep of the streams)
        bool pending_empty_push(std::vector<uint8_t> *done) {
            static const uint64_t zero_off[1] = {0};
            const h2v_batch sb{0, nullptr, zero_off, nullptr, nullptr};
            return bs->push(sb, done);
        }
    };
    std::vector<uint8_t> collect() {   // the oldest batch: one result per device, concatenated in device (= proof) order
        std::vector<uint8_t> out;
        out.reserve(sizes_.front());
        for (auto &d : devs_) {
            std::lock_guard<std::mutex> l(d->mu);
            if (d->results.empty()) throw Error(H2V_E_ARG, "NodeStream: a device has no finished batch");
            out.insert(out.end(), d->results.front().begin(), d->results.front().end());
            d->results.pop_front();
        }
        sizes_.pop_front();
        return out;
    }
    std::vector<std::unique_ptr<Dev>> devs_;
    std::deque<uint64_t> sizes_;
};

}  // namespace h2v
