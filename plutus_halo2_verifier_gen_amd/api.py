"""Host-side mirror of the reference's verify interface for the hot path, over the C-ABI (include/h2v.h).

The reference runs the path as two calls re-exported at /root/reference/src/lib.rs:9-15

    let mut transcript = CircuitTranscript::<CardanoFriendlyBlake2b>::init_from_bytes(&proof);   // simple_mul.rs:97
    let guard = prepare(&vk, &[&[]], &[&[&instance]], &mut transcript)?;                          // simple_mul.rs:98
    guard.verify(&kzg_params.verifier_params())?;                                                 // simple_mul.rs:101

(`DualMSM::check(&params) -> bool` in examples/ivc.rs:195-198, `transcript.assert_empty()` in ivc.rs:92-94).
Same names, argument meaning and error behaviour here; the work itself happens on the GPU when the guard is
consumed, and `verify_batch` is the batched form the hardware wants (thousands of independent proofs per call).

Error behaviour mirrors the reference: malformed encodings surface from `prepare`/`verify` as `VerifyError`
(Rust: `Err(midnight_proofs::plonk::Error)`), a failed pairing as `VerifyError` from `verify`.  API misuse and device
problems raise `backend.H2VError`.  There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

from . import backend
from . import bls12_381 as bls
from .plan import Plan, compile_plan
from .vk import VerifyingKey

STATUS_TEXT = {
    backend.ST_BAD_SCALAR: "non-canonical scalar encoding in the proof",
    backend.ST_INVERSE_OF_ZERO: "division by zero in the verifier (x^n = 1 or x = omega^i)",
    backend.ST_SHORT_PROOF: "proof shorter than the verifier's read program",
    backend.ST_BAD_POINT: "invalid G1 encoding (malformed / off-curve / not in the subgroup)",
    backend.ST_PAIRING: "pairing check failed",
    backend.ST_RECURSION: "recursion: the verifying-key hash in the public inputs is not this key's",
}


class VerifyError(Exception):
    """The proof does not verify (Rust: Err(plonk::Error))."""

    def __init__(self, status: int):
        self.status = status
        reasons = [t for bit, t in STATUS_TEXT.items() if status & bit]
        super().__init__("; ".join(reasons) or "rejected")


@dataclass
class ParamsVerifierKZG:
    """`ParamsKZG::verifier_params()`: the verifier needs only s_g2 (and the G2 generator)."""
    s_g2: bytes  # 96-byte zcash-compressed G2


# The H of CircuitTranscript<H>, as a tag: Rust's type parameter.  The hash itself belongs to the verifying key
# (vk.transcript_hash) and is replayed on the GPU; the tag only says what the caller believes the proof was made under.
CARDANO_FRIENDLY_BLAKE2B = "cardano-blake2b-256"   # CardanoFriendlyBlake2b (adjusted_types/mod.rs:30-72)
BLAKE2B_512 = "blake2b-512"                        # blake2b_simd::State, halo2's and midnight's default


class CircuitTranscript:
    """CircuitTranscript<H> on the verifier side: a cursor over the proof bytes and the tag of H
    (CARDANO_FRIENDLY_BLAKE2B, the default, or BLAKE2B_512).  The hash is replayed on the GPU, not here
    (/root/reference/src/plutus_gen/adjusted_types/mod.rs:30-72 and the default flavour it is adjusted from)."""

    def __init__(self, proof: bytes, hash: str = CARDANO_FRIENDLY_BLAKE2B):
        from .vk import TRANSCRIPT_KINDS
        if hash not in TRANSCRIPT_KINDS:
            raise ValueError("unknown transcript hash %r (known: %s)" % (hash, ", ".join(sorted(TRANSCRIPT_KINDS))))
        self._proof = bytes(proof)
        self._consumed = 0
        self.hash = hash

    @classmethod
    def init_from_bytes(cls, proof: bytes, hash: str = CARDANO_FRIENDLY_BLAKE2B) -> "CircuitTranscript":
        return cls(proof, hash)

    @property
    def proof(self) -> bytes:
        return self._proof

    def assert_empty(self) -> None:
        """examples/ivc.rs:92-94: every byte of the proof must have been read."""
        if self._consumed != len(self._proof):
            raise VerifyError(backend.ST_SHORT_PROOF if self._consumed > len(self._proof) else 0)


class Verifier:
    """A VerifyingKey compiled to a plan and loaded on one GPU (h2v_plan*): the object behind `prepare`."""

    def __init__(self, vk: VerifyingKey, device: int = 0, plan: Optional[Plan] = None):
        self.vk = vk
        self.plan = plan or compile_plan(vk)
        self.device_plan = backend.DevicePlan(self.plan.to_bytes(), device)
        self._ws: Optional[backend.Workspace] = None

    def _workspace(self, n: int) -> backend.Workspace:
        if self._ws is None or self._ws.max_batch < n:
            self._ws = backend.Workspace(self.device_plan, max(n, 64))
        return self._ws

    def verify_batch(self, proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
                     committed: Optional[Sequence[Optional[bytes]]] = None, mode: str = "per-proof",
                     seed: Optional[bytes] = None, fold_pairs: bool = False, derive_seed: bool = False) -> List[bool]:
        """accept[i] for n independent proofs of this circuit (instances[i]: the public-input scalars of proof i;
        committed[i]: its committed instance as 48 compressed bytes, when the circuit has one).
        mode="rlc": the batch-accept fast path (one bucket MSM + one pairing for the batch, per-proof kernels only if
        the batch check fails; same accept vector up to a 2^-128 soundness error over `seed`, drawn from the OS when None).
        fold_pairs (mode="rlc", recursive circuits): combine the pairs the fold leaves instead of one pairing per proof.
        derive_seed (mode="rlc"; H2V_RLC_SEED_TRANSCRIPT): the seed is a digest of the key and the batch (seed.batch_seed) - nothing
        is drawn, nothing has to be kept from the provers, and the call is reproducible; not together with `seed`."""
        if derive_seed and mode != "rlc":
            raise ValueError("derive_seed needs mode='rlc'")
        n = len(proofs)
        if n == 0:
            return []
        proofs_b, off, inst, ci = self._pack(proofs, instances, committed)
        if mode == "rlc":
            acc, _fell_back = self.device_plan.verify_batch_rlc(proofs_b, off, inst, ci, ws=self._workspace(n), seed=seed,
                                                                   fold_pairs=fold_pairs, derive_seed=derive_seed)
        elif mode == "per-proof":
            acc = self.device_plan.verify_batch(proofs_b, off, inst, ci, ws=self._workspace(n))
        else:
            raise ValueError("mode is 'per-proof' or 'rlc'")
        return [bool(a) for a in acc]

    def prepare_batch(self, proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
                      committed: Optional[Sequence[Optional[bytes]]] = None):
        """The first half of verify_batch: (pairs, status).  pairs[i] = compress(L) || compress(R) (96 bytes), the two
        points of proof i's final check e(L, s_g2) == e(R, G2) - 96 zero bytes for a proof rejected before the pairing;
        status[i] = verify's status bits without ST_PAIRING (include/h2v.h: h2v_prepare_batch)."""
        n = len(proofs)
        if n == 0:
            return [], []
        raw, st = self.device_plan.prepare_batch(*self._pack(proofs, instances, committed), ws=self._workspace(n))
        return [raw[96 * i:96 * i + 96] for i in range(n)], st

    def check_pairs(self, pairs: Sequence[bytes], mode: str = "per-pair", seed: Optional[bytes] = None, derive_seed: bool = False):
        """The second half: (accept, status) for pairs compress(L) || compress(R) from anywhere (h2v_check_pairs).
        mode="rlc" (h2v_check_pairs_rlc): the same outputs from ONE pairing for the batch - "scale each DualMSM by a random
        coefficient, add, check once" - with the per-pair kernels only behind a failed check.  derive_seed (mode="rlc"): the
        coefficients follow from a digest of the key and the pairs (seed.pairs_seed), as for verify_batch."""
        if mode not in ("per-pair", "rlc"):
            raise ValueError("mode is 'per-pair' or 'rlc'")
        if derive_seed and mode != "rlc":
            raise ValueError("derive_seed needs mode='rlc'")
        n = len(pairs)
        if n == 0:
            return [], []
        if any(len(p) != 96 for p in pairs):
            raise ValueError("a pair is 96 bytes: compress(L) || compress(R)")
        raw = b"".join(bytes(p) for p in pairs)
        if mode == "rlc":
            acc, st, _fell_back = self.device_plan.check_pairs_rlc(raw, ws=self._workspace(n), seed=seed, derive_seed=derive_seed)
        else:
            acc, st = self.device_plan.check_pairs(raw, ws=self._workspace(n))
        return [bool(a) for a in acc], st

    def aggregate_batch(self, proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
                        committed: Optional[Sequence[Optional[bytes]]] = None, seed: Optional[bytes] = None, derive_seed: bool = False):
        """The batch's ONE pair instead of a verdict (h2v_aggregate_batch): (pair, included, status, info).  pair = compress(L) ||
        compress(R) with L = sum r_i L_i, R = sum r_i R_i over the included proofs - the reference's DualMSM of the batch, scaled
        and added, not yet checked; included[i] = "not rejected before the pairing" (not a verdict: an included proof is accepted
        iff the pair's equation holds); status as prepare_batch; info = backend.AggregateInfo.  check_pairs checks the pair -
        with mode="rlc" many of them in one pairing (Aggregator does that).  seed: tests only, as for verify_batch.  derive_seed:
        the seed is a digest of the key and the batch (seed.batch_seed; info.seed_source = 1, info.seed_used has it), so that
        anyone with the same inputs recomputes the same pair."""
        n = len(proofs)      # (n = 0 goes through the library too: (inf, inf), and the info carries the call's seed and n_chunks = 1)
        pair, inc, st, info = self.device_plan.aggregate_batch(*self._pack(proofs, instances, committed), ws=self._workspace(n) if n else None,
                                                               seed=seed, derive_seed=derive_seed)
        return pair, [bool(a) for a in inc], st, info

    def _pack(self, proofs, instances, committed):
        n = len(proofs)
        if len(instances) != n:
            raise ValueError("one instance list per proof")
        n_pi = self.plan.n_pi
        for ins in instances:
            if len(ins) != n_pi:
                raise ValueError("expected %d public inputs per proof" % n_pi)
        off = [0]
        for p in proofs:
            off.append(off[-1] + len(p))
        inst = b"".join((int(v) % bls.R).to_bytes(32, "little") for ins in instances for v in ins)
        ci = None
        if self.plan.n_ci:
            if committed is None or len(committed) != n:
                raise ValueError("this circuit takes one committed instance per proof")
            ci = b"".join(bls.g1_compress(None) if c is None else bytes(c) for c in committed)
        return b"".join(proofs), off, inst, ci


@dataclass
class DualMSM:
    """The collapsed DualMSM of one proof (aiken_halo2/lib/halo2_kzg.ak: `left` is the PI commitment): the two points of its
    final check e(left, s_g2) == e(right, G2), 48-byte compressed each.  check() runs that pairing on the GPU."""
    left: bytes
    right: bytes
    _verifier: Optional["Verifier"] = field(default=None, repr=False, compare=False)

    def check(self, params: Optional[ParamsVerifierKZG] = None) -> bool:
        if self._verifier is None:
            raise RuntimeError("this DualMSM has no verifying key to check against")
        if params is not None and bytes(params.s_g2) != bytes.fromhex(self._verifier.vk.s_g2):
            raise ValueError("verifier params do not match the verifying key's SRS (s_g2 differs)")
        acc, _st = self._verifier.check_pairs([bytes(self.left) + bytes(self.right)])
        return acc[0]


class Guard:
    """The VerificationGuard returned by `prepare`: consumed by `verify` (Guard::verify) or `check` (DualMSM::check)."""

    def __init__(self, verifier: Verifier, proof: bytes, instances: bytes, committed: Optional[bytes]):
        self._v = verifier
        self._proof, self._instances, self._committed = proof, instances, committed
        self._used = False

    def _run(self, params: Optional[ParamsVerifierKZG]) -> int:
        if self._used:
            raise RuntimeError("guard already consumed")  # Rust: moved value
        self._used = True
        if params is not None and bytes(params.s_g2) != bytes.fromhex(self._v.vk.s_g2):
            raise ValueError("verifier params do not match the verifying key's SRS (s_g2 differs)")
        tr = self._v.device_plan.trace(self._proof, self._instances, self._committed)
        return tr["status"] if not tr["accept"] else 0

    def verify(self, params: Optional[ParamsVerifierKZG] = None) -> None:
        st = self._run(params)
        if st:
            raise VerifyError(st)

    def check(self, params: Optional[ParamsVerifierKZG] = None) -> bool:
        return self._run(params) == 0

    def dual_msm(self) -> DualMSM:
        """The proof's pair (prepare with n = 1); raises VerifyError for a proof rejected before the pairing."""
        if self._used:
            raise RuntimeError("guard already consumed")
        self._used = True
        off = [0, len(self._proof)]
        raw, st = self._v.device_plan.prepare_batch(self._proof, off, self._instances, self._committed)
        if st[0]:
            raise VerifyError(st[0])
        return DualMSM(raw[:48], raw[48:96], self._v)


_VERIFIERS = {}


def verifier_for(vk: VerifyingKey, device: int = 0) -> Verifier:
    """One compiled plan per (verifying key CONTENT, device).  Keyed by the key's canonical JSON, not by id(vk): an
    object id is reused after garbage collection and would hand a new key a stale plan."""
    key = (vk.to_json(), device)
    if key not in _VERIFIERS:
        _VERIFIERS[key] = Verifier(vk, device)
    return _VERIFIERS[key]


def prepare(vk: VerifyingKey, committed_instances: Sequence[Sequence[Optional[bytes]]],
            instances: Sequence[Sequence[Sequence[int]]], transcript: CircuitTranscript, device: int = 0) -> Guard:
    """prepare(&vk, committed_instances: &[&[C]], instances: &[&[&[F]]], &mut transcript) for ONE proof
    (the outer slices have length 1, as at every call site of the reference)."""
    if len(instances) != 1 or len(committed_instances) != 1:
        raise ValueError("one proof per prepare() call; use Verifier.verify_batch for batches")
    # prepare::<F, KZG, CircuitTranscript<H>> with an H that is not the key's does not compile in Rust; here it is API misuse
    # (never a reject), found before anything is loaded or launched.  A proof that was MADE under another hash than its tag
    # says is a different matter: nobody can see that, and it is rejected by the pairing like any bad proof.
    from .vk import TRANSCRIPT_KINDS, transcript_kind
    if TRANSCRIPT_KINDS[transcript.hash] != transcript_kind(vk)[0]:
        want = [k for k, v in TRANSCRIPT_KINDS.items() if v == transcript_kind(vk)[0]][0]
        raise ValueError("transcript hash mismatch: the transcript is CircuitTranscript<%s>, the verifying key's is %s" % (transcript.hash, want))
    cols = instances[0]
    pub = list(cols[0]) if len(cols) else []
    v = verifier_for(vk, device)
    if len(pub) != v.plan.n_pi:
        raise ValueError("expected %d public inputs" % v.plan.n_pi)
    cis = list(committed_instances[0])
    if len(cis) != v.plan.n_ci:
        raise ValueError("expected %d committed instances" % v.plan.n_ci)
    ci = None
    if cis:
        ci = bls.g1_compress(None) if cis[0] is None else bytes(cis[0])
    inst = b"".join((int(x) % bls.R).to_bytes(32, "little") for x in pub)
    transcript._consumed = v.plan.proof_len
    return Guard(v, transcript.proof, inst, ci)


# ---- mixed-key batches: one key per proof (include/h2v.h: h2v_verify_mixed)
_MIXED_WS = {}


def _mixed_workspace(verifiers, n: int) -> backend.Workspace:
    """One multi-plan workspace per set of keys (grown when a larger batch comes along)."""
    key = tuple(id(v) for v in verifiers)
    ws = _MIXED_WS.get(key)
    if ws is None or ws.max_batch < n:
        if ws is not None:
            ws.close()
        ws = _MIXED_WS[key] = backend.Workspace.multi([v.device_plan for v in verifiers], max(n, 64))
    return ws


def check_pairs_multi(verifiers_and_pairs, seed: Optional[bytes] = None):
    """ONE check over pairs on several SRS (h2v_check_pairs_multi): verifiers_and_pairs is a sequence of (Verifier, pairs) - the
    pairs (96 bytes each: compress(L) || compress(R)) grouped by the verifier whose SRS they are checked against, in order; at
    most backend.MULTI_SRS_MAX groups.  Returns (accept, status), flat, in the order the pairs were given: what each verifier's
    own check_pairs gives for its group - from C + 1 Miller loops and one final exponentiation when every equation holds."""
    groups = [(v, [bytes(p) for p in pairs]) for v, pairs in verifiers_and_pairs]
    if any(len(p) != 96 for _v, pairs in groups for p in pairs):
        raise ValueError("a pair is 96 bytes: compress(L) || compress(R)")
    n = sum(len(pairs) for _v, pairs in groups)
    if n == 0:
        return [], []
    first = next(v for v, pairs in groups if pairs)
    acc, st, _fell_back = backend.check_pairs_multi([v.device_plan for v, _p in groups], [len(pairs) for _v, pairs in groups],
                                                    b"".join(p for _v, pairs in groups for p in pairs), ws=first._workspace(n), seed=seed)
    return [bool(a) for a in acc], st


def _params_list(params) -> List[ParamsVerifierKZG]:
    """`params` of Aggregator / batch_verify: one ParamsVerifierKZG, or a sequence of them (several SRS)"""
    return [params] if isinstance(params, ParamsVerifierKZG) else list(params)


def verify_mixed(vks: Sequence[VerifyingKey], proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
                 committed: Optional[Sequence[Optional[bytes]]] = None, mode: str = "per-proof", seed: Optional[bytes] = None,
                 device: int = 0, fold_msm: bool = False, grouped: bool = False, keyed_seed: bool = False,
                 across_srs: bool = False, one_call: bool = False) -> List[bool]:
    """accept[i] for n proofs, proof i under the key vks[i] (instances[i]: its public-input scalars; committed[i]: its
    committed instance as 48 compressed bytes when its circuit has one, else None).  The proofs are grouped by SRS on the
    host - one h2v_verify_mixed call per distinct s_g2, each over all its keys - and the verdicts come back in the caller's
    order.  mode="rlc": ONE pairing per call (the reference's batch_verify); same accept vector up to a 2^-128 soundness error
    over `seed` (from the OS when None).  fold_msm (mode="rlc" only): ONE bucket MSM over the call's per-proof terms as well
    (H2V_MIXED_FOLD_MSM); a failed check runs the call again without it.  grouped (with fold_msm only; H2V_MIXED_GROUPED): phase 1
    of every key in one launch per kernel and up to backend.MIXED_GROUPED_MAX_PLANS keys per call - for many keys with few proofs
    each; the same verdicts.  keyed_seed (mode="rlc"; H2V_RLC_SEED_KEYED, not beside `seed`): nothing is drawn - every call's
    seed is a digest of its proofs, instances and each proof's own key (seed.mixed_seed), the same whatever fold_msm / grouped say.
    across_srs (mode="rlc" only): ONE pairing for the whole list instead of one per SRS - per distinct s_g2 one aggregate call
    (h2v_aggregate_mixed: its pair and included[]), then one check_pairs_multi over the S pairs; an SRS whose pair fails is
    verified by today's per-SRS call.  The same verdicts.
    one_call (with across_srs only): ONE library call per slice of at most backend.MULTI_SRS_MAX SRS instead - h2v_verify_mixed
    with H2V_MIXED_ACROSS_SRS on one workspace over all the slice's keys: no pair leaves the device, nothing is decoded again and
    a failing list is localised inside the call.  The same verdicts."""
    if keyed_seed and mode != "rlc":
        raise ValueError("keyed_seed needs mode='rlc'")
    if across_srs and mode != "rlc":
        raise ValueError("across_srs needs mode='rlc'")
    if one_call and not across_srs:
        raise ValueError("one_call needs across_srs (and mode='rlc')")
    if one_call:
        return _verify_one_call(vks, proofs, instances, committed, seed, device, fold_msm, grouped, keyed_seed)[0]
    if across_srs:
        return _verify_across_srs(vks, proofs, instances, committed, seed, device, fold_msm, grouped, keyed_seed)[0]
    return _verify_mixed(vks, proofs, instances, committed, mode, seed, device, fold_msm, grouped, keyed_seed)[0]


def _mixed_calls(vks, proofs, instances, committed, device, srs_per_call: int = 1):
    """The proofs grouped by SRS: per distinct s_g2 (positions, verifiers, plan_of, proof bytes, offsets, instances, committed).
    srs_per_call > 1: per slice of that many SRS, in the order the list first carries them, the positions in the caller's order"""
    n = len(proofs)
    if len(vks) != n or len(instances) != n or (committed is not None and len(committed) != n):
        raise ValueError("one key, one instance list (and one committed instance or None) per proof")
    groups = {}                                   # s_g2 -> positions, in the caller's order
    for i, vk in enumerate(vks):
        groups.setdefault(vk.s_g2, []).append(i)
    per_srs = list(groups.values())
    for lo in range(0, len(per_srs), srs_per_call):
        idx = per_srs[lo] if srs_per_call == 1 else sorted(i for g in per_srs[lo:lo + srs_per_call] for i in g)
        verifiers, slot, plan_of = [], {}, []
        for i in idx:
            v = verifier_for(vks[i], device)
            if id(v) not in slot:
                slot[id(v)] = len(verifiers)
                verifiers.append(v)
            plan_of.append(slot[id(v)])
        off, inst, ci = [0], [], []
        for i, k in zip(idx, plan_of):
            pl = verifiers[k].plan
            if len(instances[i]) != pl.n_pi:
                raise ValueError("proof %d: expected %d public inputs" % (i, pl.n_pi))
            off.append(off[-1] + len(proofs[i]))
            inst.append(b"".join((int(x) % bls.R).to_bytes(32, "little") for x in instances[i]))
            if pl.n_ci:
                c = committed[i] if committed is not None else None
                ci.append(bls.g1_compress(None) if c is None else bytes(c))
        yield idx, verifiers, plan_of, b"".join(bytes(proofs[i]) for i in idx), off, b"".join(inst), b"".join(ci) or None


def _verify_mixed(vks, proofs, instances, committed, mode, seed, device, fold_msm=False, grouped=False, keyed_seed=False):
    """(accept, status) of verify_mixed"""
    if mode not in ("per-proof", "rlc"):
        raise ValueError("mode is 'per-proof' or 'rlc'")
    if fold_msm and mode != "rlc":
        raise ValueError("fold_msm needs mode='rlc'")
    if grouped and not fold_msm:
        raise ValueError("grouped needs mode='rlc' and fold_msm")
    out: List[bool] = [False] * len(proofs)
    status: List[int] = [0] * len(proofs)
    for idx, verifiers, plan_of, pbytes, off, inst, ci in _mixed_calls(vks, proofs, instances, committed, device):
        acc, st, _fb = backend.verify_mixed([v.device_plan for v in verifiers], plan_of, pbytes, off, inst, ci,
                                             ws=_mixed_workspace(verifiers, len(idx)), mode=mode, seed=seed, fold_msm=fold_msm, grouped=grouped,
                                             keyed_seed=keyed_seed)
        for i, a, s in zip(idx, acc, st):
            out[i], status[i] = bool(a), s
    return out, status


def _verify_one_call(vks, proofs, instances, committed, seed, device, fold_msm=False, grouped=False, keyed_seed=False):
    """(accept, status) of verify_mixed(mode="rlc", across_srs=True, one_call=True)"""
    if grouped and not fold_msm:
        raise ValueError("grouped needs mode='rlc' and fold_msm")
    out: List[bool] = [False] * len(proofs)
    status: List[int] = [0] * len(proofs)
    for idx, verifiers, plan_of, pbytes, off, inst, ci in _mixed_calls(vks, proofs, instances, committed, device, backend.MULTI_SRS_MAX):
        acc, st, _fb = backend.verify_mixed([v.device_plan for v in verifiers], plan_of, pbytes, off, inst, ci,
                                             ws=_mixed_workspace(verifiers, len(idx)), mode="rlc", seed=seed, fold_msm=fold_msm, grouped=grouped,
                                             keyed_seed=keyed_seed, across_srs=True)
        for i, a, s in zip(idx, acc, st):
            out[i], status[i] = bool(a), s
    return out, status


def _verify_across_srs(vks, proofs, instances, committed, seed, device, fold_msm=False, grouped=False, keyed_seed=False):
    """(accept, status) of verify_mixed(mode="rlc", across_srs=True)"""
    if grouped and not fold_msm:
        raise ValueError("grouped needs mode='rlc' and fold_msm")
    out: List[bool] = [False] * len(proofs)
    status: List[int] = [0] * len(proofs)
    calls = []
    for idx, verifiers, plan_of, pbytes, off, inst, ci in _mixed_calls(vks, proofs, instances, committed, device):
        plans, ws = [v.device_plan for v in verifiers], _mixed_workspace(verifiers, len(idx))
        pair, included, st, _info = backend.aggregate_mixed(plans, plan_of, pbytes, off, inst, ci, ws=ws, seed=seed, grouped=grouped,
                                                            keyed_seed=keyed_seed)
        calls.append((idx, verifiers, pair, included, st,
                      lambda plans=plans, plan_of=plan_of, pbytes=pbytes, off=off, inst=inst, ci=ci, ws=ws: backend.verify_mixed(
                          plans, plan_of, pbytes, off, inst, ci, ws=ws, mode="rlc", seed=seed, fold_msm=fold_msm, grouped=grouped,
                          keyed_seed=keyed_seed)))
    for lo in range(0, len(calls), backend.MULTI_SRS_MAX):       # (more SRS than one check takes: one check per slice)
        part = calls[lo:lo + backend.MULTI_SRS_MAX]
        ok, _st = check_pairs_multi([(c[1][0], [c[2]]) for c in part], seed=seed)
        for passed, (idx, _verifiers, _pair, included, st, again) in zip(ok, part):
            if not passed:
                included, st, _fb = again()
            for i, a, s in zip(idx, included, st):
                out[i], status[i] = bool(a), s
    return out, status


def batch_verify(params: ParamsVerifierKZG, vks: Sequence[VerifyingKey], instances: Sequence[Sequence[int]],
                 proofs: Sequence[bytes], committed: Optional[Sequence[Optional[bytes]]] = None, device: int = 0,
                 fold_msm: bool = False, grouped: bool = False, keyed_seed: bool = False, one_call: bool = False) -> None:
    """midnight_zk_stdlib::batch_verify(&params, &vks, &instances, &proofs) (src/circuits/schnorr_circuit.rs:223-231): one
    call and one final check for a list of (vk, instances, proof) triples on ONE SRS - the batch-accept mode of verify_mixed.
    Raises VerifyError unless every proof is accepted (Rust: Err(_)); a key on another SRS than `params` is a ValueError.
    fold_msm: one bucket MSM for the list as well; grouped: phase 1 of every key in one launch per kernel; keyed_seed: the seed is
    derived from the list itself (verify_mixed).  `params` may also be a sequence of ParamsVerifierKZG: a list that spans several
    SRS, still with one final check (verify_mixed(across_srs=True)); a key on none of them is a ValueError.  one_call (with a
    sequence of params only; otherwise ValueError): that list as ONE library call (verify_mixed(across_srs=True, one_call=True))."""
    if one_call and isinstance(params, ParamsVerifierKZG):
        raise ValueError("one_call needs across_srs: `params` as a sequence of ParamsVerifierKZG")
    known = [bytes(q.s_g2) for q in _params_list(params)]
    for i, vk in enumerate(vks):
        if bytes.fromhex(vk.s_g2) not in known:
            raise ValueError("verifier params do not match the SRS of vks[%d] (s_g2 differs)" % i)
    if one_call:
        acc, status = _verify_one_call(vks, proofs, instances, committed, None, device, fold_msm, grouped, keyed_seed)
    elif not isinstance(params, ParamsVerifierKZG):
        acc, status = _verify_across_srs(vks, proofs, instances, committed, None, device, fold_msm, grouped, keyed_seed)
    else:
        acc, status = _verify_mixed(vks, proofs, instances, committed, "rlc", None, device, fold_msm, grouped, keyed_seed)
    if not all(acc):
        raise VerifyError(next(s for a, s in zip(acc, status) if not a))


class Aggregator:
    """Collects the pairs of several calls and checks them ONCE: the reference's `dual_msm.scale(r)` / `acc.add_msm(..)` per call
    and one `check` over everything collected (examples/ivc.rs:85-96, 195-208).  One Aggregator per SRS (`params`); a key on
    another SRS is a ValueError.  `params` may also be a sequence of ParamsVerifierKZG: pushes on any of those SRS (one push is
    one pair on ONE of them), and finish() still runs one check - a multi-pairing over all of them (check_pairs_multi).

        agg = Aggregator(params)
        agg.push(vk_a, proofs_a, instances_a)         # h2v_aggregate_batch: no pairing runs
        agg.push(vk_b, proofs_b, instances_b)
        accepts, reverified = agg.finish()            # ONE pairing over the K pairs (h2v_check_pairs_rlc; h2v_check_pairs for K = 1)

    finish() returns the per-call accept lists in push order and the indices of the calls that had to be verified again: a call
    whose pair passes gets accept = included; a call whose pair fails is verified per proof (verify_batch) on the inputs push
    kept.  The pairs of different calls are scaled again with fresh coefficients by the check, so the errors of two calls cannot
    cancel.  A pair is only worth what the seed of its call is: keep an Aggregator inside one trust domain."""

    def __init__(self, params: ParamsVerifierKZG, device: int = 0, grouped: bool = False, derive_seed: bool = False,
                 keyed_seed: bool = False):
        """grouped: push_mixed runs phase 1 of every key in one launch per kernel (H2V_RLC_GROUPED) - the same pairs.
        derive_seed: every push derives its seed from its key and batch (H2V_RLC_SEED_TRANSCRIPT): its pair can be recomputed by
        anyone who holds the inputs.  Single-key pushes only: push_mixed raises ValueError (the mixed calls have no derived seed
        of that form).
        keyed_seed: every push derives its seed by the mixed calls' rule (H2V_RLC_SEED_KEYED; seed.mixed_seed - every leaf binds the
        key of its own proof).  push_mixed derives, and a single-key push goes out as a ONE-PLAN MIXED CALL, so that every pair
        of the aggregator follows one rule - its seed is NOT the one derive_seed would give the same batch.  Together with
        derive_seed: ValueError (one rule per aggregator)."""
        if derive_seed and keyed_seed:
            raise ValueError("derive_seed and keyed_seed exclude each other: one seed rule per Aggregator")
        self.params, self.device, self.grouped, self.derive_seed, self.keyed_seed = params, device, grouped, derive_seed, keyed_seed
        self._calls = []      # (a verifier on the SRS, pair, included, the call again per proof -> accept list, the SRS's index)

    def _srs_of(self, vks, listed: bool = True) -> int:
        """which of the aggregator's SRS every key of one push is on; ValueError for a key on none of them or keys on two"""
        found, srs = None, [bytes(q.s_g2) for q in _params_list(self.params)]
        for i, vk in enumerate(vks):
            s_g2 = bytes.fromhex(vk.s_g2)
            if s_g2 not in srs:
                raise ValueError("verifier params do not match the SRS of vks[%d] (s_g2 differs)" % i if listed else
                                 "verifier params do not match the verifying key's SRS (s_g2 differs)")
            if found is not None and srs.index(s_g2) != found:
                raise ValueError("one push is one pair on one SRS: vks[%d] is on another SRS than vks[0]" % i)
            found = srs.index(s_g2)
        return found or 0

    def push(self, vk: VerifyingKey, proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
             committed: Optional[Sequence[Optional[bytes]]] = None, seed: Optional[bytes] = None) -> int:
        """aggregates one call of proofs of `vk` and keeps its pair, included[] and a reference to the inputs; returns the call's index"""
        srs = self._srs_of([vk], listed=False)
        if self.keyed_seed:      # (a one-plan mixed call: the aggregator's one rule)
            if seed is not None:
                raise ValueError("keyed_seed derives the seed: none can be given")
            return self.push_mixed([vk] * len(proofs), proofs, instances, committed)
        v = verifier_for(vk, self.device)
        pair, included, _status, _info = v.aggregate_batch(proofs, instances, committed, seed=seed, derive_seed=self.derive_seed)
        self._calls.append((v, pair, included, lambda: v.verify_batch(proofs, instances, committed), srs))
        return len(self._calls) - 1

    def push_mixed(self, vks: Sequence[VerifyingKey], proofs: Sequence[bytes], instances: Sequence[Sequence[int]],
                   committed: Optional[Sequence[Optional[bytes]]] = None, seed: Optional[bytes] = None) -> int:
        """aggregates one call of proofs of SEVERAL keys, proof i under vks[i] (h2v_aggregate_mixed; with grouped=True the
        H2V_RLC_GROUPED form: up to backend.MIXED_GROUPED_MAX_PLANS keys); returns the call's index"""
        if self.derive_seed:
            raise ValueError("an Aggregator with derive_seed takes single-key pushes only: the mixed calls have no derived seed")
        srs = self._srs_of(list(vks))
        if not proofs:
            raise ValueError("no proofs")
        (idx, verifiers, plan_of, pbytes, off, inst, ci), = _mixed_calls(vks, proofs, instances, committed, self.device)
        pair, included, _status, _info = backend.aggregate_mixed([v.device_plan for v in verifiers], plan_of, pbytes, off, inst, ci,
                                                                 ws=_mixed_workspace(verifiers, len(idx)), seed=seed, grouped=self.grouped,
                                                                 keyed_seed=self.keyed_seed)
        self._calls.append((verifiers[0], pair, included, lambda: verify_mixed(vks, proofs, instances, committed, device=self.device), srs))
        return len(self._calls) - 1

    def finish(self, seed: Optional[bytes] = None):
        """(accepts, reverified): one check over the collected pairs, per-proof verification of the calls whose pair fails.  The
        Aggregator is empty afterwards."""
        calls, self._calls = self._calls, []
        if not calls:
            return [], []
        pairs = [c[1] for c in calls]
        if len({c[4] for c in calls}) == 1:
            ok, _st = calls[0][0].check_pairs(pairs, mode="rlc" if len(pairs) > 1 else "per-pair", seed=seed)
        else:
            # several SRS: the calls' pairs sorted by SRS, stably, and ONE multi-pairing; the verdicts back in push order
            order = sorted(range(len(calls)), key=lambda k: calls[k][4])
            groups = []
            for k in order:
                if not groups or groups[-1][0] != calls[k][4]:
                    groups.append((calls[k][4], calls[k][0], []))
                groups[-1][2].append(pairs[k])
            flat, _st = check_pairs_multi([(v, ps) for _srs, v, ps in groups], seed=seed)
            ok = [False] * len(calls)
            for k, a in zip(order, flat):
                ok[k] = a
        accepts, reverified = [], []
        for k, (_v, _pair, included, again, _srs) in enumerate(calls):
            if ok[k]:
                accepts.append(list(included))
            else:
                reverified.append(k)
                accepts.append(again())
        return accepts, reverified
