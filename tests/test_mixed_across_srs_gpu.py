"""GPU tests of the mixed-key call across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS - one call and ONE multi-pairing for
proofs whose keys sit on several SRS).  Form A = ACROSS | RLC (every proof's own ladder MSM, coefficients by class-major position),
Form B = ACROSS | RLC | FOLD_MSM (one bucket MSM, coefficients by call position), with or without GROUPED.

Six keys on four SRS (vk.on_srs; S_A .. S_C of tests/test_pairs_multi_srs.py and a fourth secret): simple_mul on S_A with 66
proofs - the class crosses a 64-lane wave -, simple_mul again and lookup_table on S_B (3 + 2: two keys in one class, the same
circuit on a second SRS), trashcan_mix (committed instance) and ivc (recursive: one pair in Form B) on S_C (2 + 1), and
atms_with_lookups on S_D listed without a proof.  74 proofs, interleaved by a seeded shuffle.  Expected verdicts come from the CPU
oracle per key, status words from h2v_verify_batch_device per key, sums from the big-integer model (tests/mixed_across_model.py)
over h2v_prepare_batch's per-proof pairs; nothing comes from the call under test."""
import json
import os
import random
import struct
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, seed as S, synth
from tests import cancel, mixed_across_model as AM
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import PKG, ROOT
from tests.test_mixed_keys_gpu import _per_key_device
from tests.test_pairs_multi_srs import S_A, S_B, S_C

pytestmark = pytest.mark.gpu
S_D = 0x5d4d << 64 | 19
SEED = bytes(range(32))
# (id, circuit, SRS label, proofs): the LISTED plans, in list order
KEYS = (("sm_a", "simple_mul", "A", 66), ("sm_b", "simple_mul", "B", 3), ("lt_b", "lookup_table", "B", 2), ("tm_c", "trashcan_mix", "C", 2),
        ("ivc_c", "ivc", "C", 1), ("atms_d", "atms_with_lookups", "D", 0))
SECRET = {"A": S_A, "B": S_B, "C": S_C, "D": S_D}
IDS = [k[0] for k in KEYS]
LABEL = {k[0]: k[2] for k in KEYS}
FORMS = {"A": (False, False), "B": (True, False), "BG": (True, True)}      # fold_msm, grouped


class Mix:
    """a mixed batch in the layout of h2v_mixed_batch over `listed` key ids: order = [(key id, index in that key's batch)]"""

    def __init__(self, keys, batches, order, listed=IDS):
        self.order, self.listed = list(order), list(listed)
        self.plan_of = [self.listed.index(kid) for kid, _ in self.order]
        self.srs = [LABEL.get(kid, kid) for kid, _ in self.order]
        proofs, inst, ci, self.off, self.expected = [], [], [], [0], []
        for kid, j in self.order:
            b, n_pi = batches[kid], keys[kid]["vk"].n_public_inputs
            proofs.append(b.proof(j))
            self.off.append(self.off[-1] + len(proofs[-1]))
            inst.append(b.instances[32 * n_pi * j:32 * n_pi * (j + 1)])
            if b.committed is not None:
                ci.append(b.ci(j))
            self.expected.append(b.expected[j])
        self.n = len(self.order)
        self.proofs, self.instances, self.committed = b"".join(proofs), b"".join(inst), b"".join(ci) or None


def _interleaved(batches, seed, ids=IDS):
    order = [(kid, j) for kid in ids if kid in batches for j in range(batches[kid].n)]
    random.Random(seed).shuffle(order)
    return order


def _entry(be, orc, circuit, s):
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td = V.on_srs(*V.BUILDERS[circuit](), s)
    pl = PL.compile_plan(vk)
    return {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0),
            "ov": orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))}


def _replaced(batch, j, proof, inst_bytes, n_pi, expected):
    """a copy of `batch` with proof j (and its instance bytes) replaced"""
    proofs = [batch.proof(i) if i != j else proof for i in range(batch.n)]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    inst = batch.instances[:32 * n_pi * j] + inst_bytes + batch.instances[32 * n_pi * (j + 1):]
    return synth.Batch(n=batch.n, proofs=b"".join(proofs), proof_off=off, instances=inst, committed=batch.committed,
                       expected=[e if i != j else expected for i, e in enumerate(batch.expected)])


def _held(fx, batches, ids):
    """per key id: the per-key device call's status words, after holding its verdicts and the construction to the oracle"""
    want = {}
    for kid in ids:
        e, b = fx["keys"][kid], batches[kid]
        ora = list(e["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4))
        assert ora == b.expected, kid
        acc, want[kid] = _per_key_device(e["dp"], b)
        assert acc == ora, kid
    return want


@pytest.fixture(scope="module")
def fx(be, orc):
    keys = {kid: _entry(be, orc, circuit, SECRET[label]) for kid, circuit, label, _n in KEYS}
    fx = {"keys": keys, "plans": [keys[kid]["dp"] for kid in IDS]}
    clean = {kid: synth.forge_batch(keys[kid]["vk"], keys[kid]["td"], n, seed=141 + k, plan=keys[kid]["pl"]) for k, (kid, _c, _l, n) in enumerate(KEYS) if n}
    fx["clean"] = clean
    want_clean = _held(fx, clean, clean)
    assert all(st == [0] * clean[kid].n for kid, st in want_clean.items())
    # the rejects: every kind of corruption on the 66, one pairing-only reject in class B, one proof forged under S_A but listed
    # under the S_B simple_mul key
    rej = dict(clean)
    e = keys["sm_a"]
    rej["sm_a"] = synth.with_rejects(e["pl"], clean["sm_a"], e["vk"].n_public_inputs, fraction=0.3, seed=151, kinds=list(synth.CORRUPTIONS))
    b, e = clean["lt_b"], keys["lt_b"]
    n_pi = e["vk"].n_public_inputs
    rej["lt_b"] = _replaced(b, 0, cancel.shift_pi(e["pl"], b.proof(0), 5), b.instances[:32 * n_pi], n_pi, 0)
    b, n_pi = clean["sm_b"], keys["sm_b"]["vk"].n_public_inputs
    assert keys["sm_a"]["vk"].n_public_inputs == n_pi and len(clean["sm_a"].proof(0)) == len(b.proof(1))
    rej["sm_b"] = _replaced(b, 1, clean["sm_a"].proof(0), clean["sm_a"].instances[:32 * n_pi], n_pi, 0)
    fx["rejects"] = rej
    fx["want_rej"] = _held(fx, rej, rej)
    assert 0 < sum(rej["sm_a"].expected) < 66
    assert fx["want_rej"]["lt_b"] == [be.ST_PAIRING, 0] and fx["want_rej"]["sm_b"] == [0, be.ST_PAIRING, 0]
    fx["mix_clean"] = Mix(keys, clean, _interleaved(clean, 161))
    fx["mix"] = Mix(keys, rej, _interleaved(rej, 162))
    assert fx["mix"].n == 74
    # N_R of the clean call: what a per-key h2v_verify_batch_rlc call on each foldable key's batch sums, plus one pair per ivc proof
    n_r = clean["ivc_c"].n
    for kid in ("sm_a", "sm_b", "lt_b", "tm_c"):
        b, dp = clean[kid], keys[kid]["dp"]
        kws = be.Workspace(dp, b.n)
        got, _fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=kws, seed=SEED)
        assert list(got) == b.expected
        n_r += kws.rlc_result()[1].msm_terms
        kws.close()
    fx["n_r"] = n_r
    return fx


def _host(be, fx, mix, form, ws=None, seed=SEED, plans=None, across=True, keyed=False):
    fold, grouped = FORMS[form]
    acc, st, fb = be.verify_mixed(plans or fx["plans"], mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, mode="rlc",
                                  seed=seed, fold_msm=fold, grouped=grouped, across_srs=across, keyed_seed=keyed)
    return list(acc), st, fb


def _device(be, fx, mix, form, ws, seed=SEED, plans=None):
    import torch
    dev = torch.device("cuda", 0)
    fold, grouped = FORMS[form]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    keep = [t(mix.proofs), torch.tensor(mix.off, dtype=torch.int64, device=dev), t(mix.instances), t(mix.committed)]
    acc = torch.full((mix.n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((mix.n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: x.data_ptr() if x is not None else None
    be.verify_mixed_device(plans or fx["plans"], mix.plan_of, mix.n, *[ptr(x) for x in keep], acc.data_ptr(), st.data_ptr(), ws=ws,
                           stream=s.cuda_stream, mode="rlc", seed=seed, fold_msm=fold, grouped=grouped, across_srs=True)
    s.synchronize()
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()]


def _want_status(want, mix):
    return [want[kid][j] for kid, j in mix.order]


# ---- 1
@pytest.mark.parametrize("form", sorted(FORMS))
def test_accepting_batch_is_one_pass_in_every_form(be, fx, form):
    mix = fx["mix_clean"]
    n, terms = mix.n, fx["n_r"] if FORMS[form][0] else mix.n
    assert n == 74 and fx["n_r"] > n
    assert _host(be, fx, mix, form, None) == ([1] * n, [0] * n, False)              # a temporary workspace
    for defer in (False, True):
        ws = be.Workspace.multi(fx["plans"], 80, lanes=2, chunk=8)
        assert ws.lanes() == (2, 8)
        if defer:
            ws.defer_joins(True)
        assert _device(be, fx, mix, form, ws) == ([1] * n, [0] * n)
        ok, tm = ws.rlc_result()
        assert (ok, tm.msm_terms, tm.transcript_combiner_ms) == (True, terms, 0)
        assert _host(be, fx, mix, form, ws) == ([1] * n, [0] * n, False)
        ok, tm = ws.rlc_result()
        assert (ok, tm.msm_terms) == (True, terms)
        ws.close()


# ---- 2
def _pairs_of(fx, batches, mix):
    """h2v_prepare_batch's pair of every proof of the call, as affine points"""
    per = {}
    for kid in {kid for kid, _ in mix.order}:
        b = batches[kid]
        raw, st = fx["keys"][kid]["dp"].prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
        assert list(st) == [0] * b.n
        per[kid] = [(bls.g1_decompress(raw[96 * j:96 * j + 48]), bls.g1_decompress(raw[96 * j + 48:96 * j + 96])) for j in range(b.n)]
    return [per[kid][j] for kid, j in mix.order]


def _learn(be, fx, ws, seed):
    """tests/cancel.py's learn_counter through a one-plan list (its call has no flag: one SRS)"""
    return cancel.learn_counter(be, {"keys": {"simple_mul": fx["keys"]["sm_a"]}, "clean": {"simple_mul": fx["clean"]["sm_a"]},
                                     "plans": [fx["keys"]["sm_a"]["dp"]]}, ws, seed)


def test_sums_of_the_fold_form_follow_the_model(be, fx):
    keys, clean = fx["keys"], fx["clean"]
    order = [(kid, j) for kid in ("sm_a", "sm_b", "lt_b", "tm_c", "ivc_c") for j in range(min(3, clean[kid].n))]
    random.Random(171).shuffle(order)
    mix = Mix(keys, clean, order)
    pairs = _pairs_of(fx, clean, mix)
    listed = [LABEL[kid] for kid in IDS]
    seed = bytes(range(100, 132))
    ws = be.Workspace.multi(fx["plans"], 16, lanes=2, chunk=2)
    counter = _learn(be, fx, ws, seed)
    for form in ("B", "BG"):
        assert _host(be, fx, mix, form, ws, seed=seed) == ([1] * mix.n, [0] * mix.n, False)
        counter += 1
        r_sum, l_sums = be.probe_mixed_fold_sums_multi(ws)
        want_r, want_l = AM.sums(listed, mix.srs, pairs, lambda pos: cancel.coeff(seed, counter, pos), "B")
        assert len(l_sums) == 3 and l_sums == want_l and r_sum == want_r and None not in l_sums
        assert AM.check([S_A, S_B, S_C], r_sum, l_sums)
        # the one-SRS probe still answers: R and the first class's L
        assert be.probe_mixed_fold_sums(ws) == (l_sums[0], r_sum)
    # one class among the proofs (keyed seed: the call derives the same seed with and without the flag): the same two sums
    sub = Mix(keys, clean, [o for o in order if LABEL[o[0]] == "B"], listed=["sm_b", "lt_b"])
    plans = [keys["sm_b"]["dp"], keys["lt_b"]["dp"]]
    got = []
    for across in (True, False):
        assert _host(be, fx, sub, "B", ws, seed=None, plans=plans, across=across, keyed=True) == ([1] * sub.n, [0] * sub.n, False)
        got.append((be.probe_mixed_fold_sums(ws), ws.seed_used()))
    assert got[0] == got[1] and got[0][0][0] is not None
    with pytest.raises(be.H2VError):
        be.probe_mixed_fold_sums_multi(ws)                 # the most recent fold call carried no flag
    ws.close()


# ---- 3
@pytest.mark.parametrize("form", sorted(FORMS))
def test_rejects_equal_the_per_key_calls(be, fx, form):
    mix = fx["mix"]
    want = (mix.expected, _want_status(fx["want_rej"], mix))
    assert 0 < sum(mix.expected) < mix.n and be.ST_PAIRING in want[1]
    assert _host(be, fx, mix, form, None) == want + (True,)
    ws = be.Workspace.multi(fx["plans"], 80, lanes=2, chunk=8)
    assert _host(be, fx, mix, form, ws) == want + (True,)
    # the call's last record is the pass that decided: Form A's, over the n pairs, failed
    ok, tm = ws.rlc_result()
    assert (ok, tm.msm_terms) == (False, mix.n)
    assert _device(be, fx, mix, form, ws) == want
    ok, tm = ws.rlc_result()
    assert (ok, tm.msm_terms) == (False, mix.n)
    ws.close()


# ---- 4
def test_a_class_of_malformed_proofs_takes_no_loop(be, fx):
    keys, clean = fx["keys"], fx["clean"]
    bad = dict(clean)
    e, b = keys["tm_c"], clean["tm_c"]
    n_pi = e["vk"].n_public_inputs
    rng = random.Random(181)
    for j, kind in enumerate(("point_not_on_curve", "truncated")):
        p, ins = synth.corrupt(e["pl"], clean["tm_c"].proof(j), b.instances[32 * n_pi * j:32 * n_pi * (j + 1)], kind, rng)
        bad["tm_c"] = _replaced(bad["tm_c"], j, p, bytes(ins), n_pi, 0)
    want = _held(fx, bad, ["tm_c"])
    assert all(s and s != be.ST_PAIRING for s in want["tm_c"])
    want.update({kid: [0] * clean[kid].n for kid in ("sm_a", "sm_b", "lt_b")})
    order = [("sm_a", 0), ("tm_c", 0), ("sm_b", 0), ("lt_b", 1), ("tm_c", 1), ("sm_a", 1)]      # class C: nothing but the two
    mix = Mix(keys, bad, order)
    ws = be.Workspace.multi(fx["plans"], 16)
    for form in sorted(FORMS):
        assert _host(be, fx, mix, form, ws) == ([1, 0, 1, 1, 0, 1], _want_status(want, mix), False), form
        assert ws.rlc_result(timings=False)[0]
    # Form B: class C's left-hand sum is the point at infinity, the others' are not
    _r, l_sums = be.probe_mixed_fold_sums_multi(ws)
    assert len(l_sums) == 3 and l_sums[2] is None and l_sums[0] is not None and l_sums[1] is not None
    ws.close()


# ---- 5
def test_cancellation_across_classes(be, fx):
    keys, clean = fx["keys"], fx["clean"]
    rec_a, rec_b = cancel.rec_of(keys["sm_a"], clean["sm_a"], 2), cancel.rec_of(keys["lt_b"], clean["lt_b"], 1)
    seed = bytes(range(60, 92))
    listed = [LABEL[kid] for kid in IDS]
    ws = be.Workspace.multi(fx["plans"], 16, lanes=2, chunk=2)
    counter = _learn(be, fx, ws, seed)
    n_a, n_b = keys["sm_a"]["vk"].n_public_inputs, keys["lt_b"]["vk"].n_public_inputs

    def call(form, order, pa, pb):
        bad = dict(clean)
        bad["sm_a"] = _replaced(clean["sm_a"], 2, pa, clean["sm_a"].instances[32 * n_a * 2:32 * n_a * 3], n_a, 0)
        bad["lt_b"] = _replaced(clean["lt_b"], 1, pb, clean["lt_b"].instances[32 * n_b:32 * n_b * 2], n_b, 0)
        return _host(be, fx, Mix(keys, bad, order), form, ws, seed=seed)

    # A' first and B' last, a proof of each one's class in between: exchanging the two changes their class-major positions too
    order = [("sm_a", 2), ("sm_a", 0), ("lt_b", 0), ("lt_b", 1)]
    swapped = [order[3], order[1], order[2], order[0]]
    for form in ("B", "A"):
        at = lambda o: (AM.positions(listed, [LABEL[k] for k, _ in o]) if form == "A" else list(range(4)))
        rejected = lambda o: ([int(x not in (("sm_a", 2), ("lt_b", 1))) for x in o], [0 if x not in (("sm_a", 2), ("lt_b", 1)) else be.ST_PAIRING for x in o], True)
        # equal weights: each error stands alone under the call's coefficients
        pa, pb = cancel.cancelling(rec_a, rec_b, 1, 1, 12345)
        assert call(form, order, pa, pb) == rejected(order), form
        counter += 1
        # the form's own coefficients of the NEXT call: the errors cancel, the check passes once ...
        pos = at(order)
        assert pos[0] != at(swapped)[3] or form == "B"
        w_a, w_b = cancel.coeff(seed, counter + 1, pos[0]), cancel.coeff(seed, counter + 1, pos[3])
        pa, pb = cancel.cancelling(rec_a, rec_b, w_a, w_b, 12345)
        assert call(form, order, pa, pb) == ([1] * 4, [0] * 4, False), form
        counter += 1
        # ... and never again: not under the next call's coefficients, and not at exchanged places
        assert call(form, order, pa, pb) == rejected(order), form
        counter += 1
        w_a, w_b = cancel.coeff(seed, counter + 1, pos[0]), cancel.coeff(seed, counter + 1, pos[3])
        pa, pb = cancel.cancelling(rec_a, rec_b, w_a, w_b, 12345)
        assert call(form, swapped, pa, pb) == rejected(swapped), form
        counter += 1
    ws.close()


# ---- 6
@pytest.fixture(scope="module")
def many(be, orc):
    """17 simple_mul keys on 17 SRS, one accepting proof each"""
    keys, batches = {}, {}
    for k in range(17):
        kid = "k%02d" % k
        keys[kid] = _entry(be, orc, "simple_mul", (0x6e00 + k) << 64 | (101 + 2 * k))
        batches[kid] = synth.forge_batch(keys[kid]["vk"], keys[kid]["td"], 1, seed=201 + k, plan=keys[kid]["pl"])
        b = batches[kid]
        assert list(keys[kid]["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=1)) == [1]
    return keys, batches


def test_limits(be, fx, many):
    keys, batches = many
    ids = sorted(keys)
    plans = [keys[kid]["dp"] for kid in ids]
    ws = be.Workspace.multi(plans, 32)
    sixteen = Mix(keys, batches, [(kid, 0) for kid in reversed(ids[:16])], listed=ids)
    for form in sorted(FORMS):
        # 16 classes with a proof each pass - with the 17th plan listed WITHOUT a proof too
        assert _host(be, fx, sixteen, form, ws, plans=plans) == ([1] * 16, [0] * 16, False), form
        assert _host(be, fx, Mix(keys, batches, sixteen.order, listed=ids[:16]), form, ws, plans=plans[:16]) == ([1] * 16, [0] * 16, False), form
    terms = ws.rlc_result()[1].msm_terms
    # a 17th class WITH a proof: H2V_E_LIMIT, and nothing was enqueued - the workspace's last record is still the call before
    seventeen = Mix(keys, batches, [(kid, 0) for kid in ids], listed=ids)
    for form in sorted(FORMS):
        with pytest.raises(be.H2VError, match=r"h2v error -4: at most 16 SRS may have proofs .* this one has 17"):
            _host(be, fx, seventeen, form, ws, plans=plans)
    assert ws.rlc_result()[1].msm_terms == terms
    # without the flag two SRS are still H2V_E_ARG, naming both plans
    two = Mix(keys, batches, [(ids[0], 0), (ids[1], 0)], listed=ids[:2])
    for form in sorted(FORMS):
        with pytest.raises(be.H2VError, match=r"h2v error -1: plans\[0\] and plans\[1\] are on different SRS"):
            _host(be, fx, two, form, ws, plans=plans[:2], across=False)
    assert _host(be, fx, two, "A", ws, plans=plans[:2]) == ([1, 1], [0, 0], False)
    ws.close()


# ---- 7
def test_keyed_seed_is_the_same_in_both_forms_and_any_list_order(be, fx):
    mix = fx["mix_clean"]
    keys = fx["keys"]
    shapes = lambda ids: [(keys[kid]["vk"].n_public_inputs, keys[kid]["dp"].n_ci) for kid in ids]
    want = S.mixed_seed_flat([keys[kid]["dp"].key_tag for kid in IDS], shapes(IDS), mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed or b"")
    ws = be.Workspace.multi(fx["plans"], 80, lanes=2, chunk=8)
    seeds = []
    for form in sorted(FORMS):
        assert _host(be, fx, mix, form, ws, seed=None, keyed=True) == ([1] * mix.n, [0] * mix.n, False)
        seeds.append(ws.seed_used())
    assert seeds == [want] * 3
    # the same list with the plans listed in another order (the classes are numbered differently): the same seed
    ids2 = ["atms_d", "ivc_c", "lt_b", "sm_a", "tm_c", "sm_b"]
    mix2 = Mix(keys, fx["clean"], mix.order, listed=ids2)
    assert mix2.plan_of != mix.plan_of and mix2.proofs == mix.proofs
    assert S.mixed_seed_flat([keys[kid]["dp"].key_tag for kid in ids2], shapes(ids2), mix2.plan_of, mix2.proofs, mix2.off, mix2.instances,
                             mix2.committed or b"") == want
    for form in ("A", "B"):
        assert _host(be, fx, mix2, form, ws, seed=None, plans=[keys[kid]["dp"] for kid in ids2], keyed=True) == ([1] * mix.n, [0] * mix.n, False)
        assert ws.seed_used() == want
    # a failing call: the second pass reuses the derived words
    bad = fx["mix"]
    want_bad = S.mixed_seed_flat([keys[kid]["dp"].key_tag for kid in IDS], shapes(IDS), bad.plan_of, bad.proofs, bad.off, bad.instances, bad.committed or b"")
    for form in ("A", "B"):
        assert _host(be, fx, bad, form, ws, seed=None, keyed=True) == (bad.expected, _want_status(fx["want_rej"], bad), True)
        assert ws.seed_used() == want_bad != want
    ws.close()


# ---- 8
def test_python_surface_in_one_call(be, fx, monkeypatch):
    from plutus_halo2_verifier_gen_amd import api
    keys = fx["keys"]
    calls = []
    real = be.verify_mixed
    monkeypatch.setattr(be, "verify_mixed", lambda *a, **kw: (calls.append(kw.get("across_srs")), real(*a, **kw))[1])
    monkeypatch.setattr(be, "check_pairs_multi", lambda *a, **kw: pytest.fail("one_call makes no check_pairs_multi call"))
    params = [api.ParamsVerifierKZG(bls.g2_compress(bls.g2_mul(bls.G2_GEN, SECRET[label]))) for label in "ABC"]
    for tag, batches in (("clean", fx["clean"]), ("rejects", fx["rejects"])):
        order = [(kid, j) for kid in ("sm_a", "sm_b", "lt_b", "tm_c", "ivc_c") for j in range(min(5, batches[kid].n))]
        random.Random(191).shuffle(order)
        vks = [keys[kid]["vk"] for kid, _ in order]
        proofs = [batches[kid].proof(j) for kid, j in order]
        inst = [batches[kid].instance_ints(j, keys[kid]["vk"].n_public_inputs) for kid, j in order]
        ci = [batches[kid].ci(j) for kid, j in order]
        expected = [bool(batches[kid].expected[j]) for kid, j in order]
        assert (tag == "clean") == all(expected)
        for fold in (False, True):
            del calls[:]
            assert api.verify_mixed(vks, proofs, inst, ci, mode="rlc", across_srs=True, one_call=True, fold_msm=fold) == expected
            assert calls == [True]                        # ONE library call for the three SRS
        if tag == "clean":
            api.batch_verify(params, vks, inst, proofs, ci, one_call=True, fold_msm=True)
        else:
            with pytest.raises(api.VerifyError):
                api.batch_verify(params, vks, inst, proofs, ci, one_call=True, fold_msm=True)
        with pytest.raises(ValueError, match="s_g2 differs"):
            api.batch_verify(params[:2], vks, inst, proofs, ci, one_call=True)


# ---- 9
def test_cpp_driver(be, fx, tmp_path):
    out = str(tmp_path / "h2v_mixed_across_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_across_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for k, kid in enumerate(IDS):
        e = fx["keys"][kid]
        path = str(tmp_path / ("%s.%s" % (kid, "json" if k % 2 else "bin")))      # both forms of a key
        with open(path, "wb") as f:
            f.write(e["vk"].to_json().encode() if k % 2 else e["pl"].to_bytes())
        paths.append(path)
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    for tag, batches, want in (("accept", fx["clean"], None), ("reject", fx["rejects"], fx["want_rej"])):
        order = [(kid, j) for kid in ("sm_a", "sm_b", "lt_b", "tm_c", "ivc_c") for j in range(min(4, batches[kid].n))]
        random.Random(195).shuffle(order)
        mix = Mix(fx["keys"], batches, order)
        status = _want_status(want, mix) if want else [0] * mix.n
        assert mix.n == 12 and (sum(mix.expected) == 12) == (tag == "accept")
        blob = struct.pack("<I", mix.n)
        for kid, j in mix.order:
            b, e = batches[kid], fx["keys"][kid]
            n_pi = e["vk"].n_public_inputs
            p = b.proof(j)
            blob += struct.pack("<II", IDS.index(kid), len(p)) + p + struct.pack("<I", n_pi) + b.instances[32 * n_pi * j:32 * n_pi * (j + 1)]
            blob += struct.pack("<I", 1) + b.ci(j) if b.committed is not None else struct.pack("<I", 0)
        with open(str(tmp_path / (tag + ".bin")), "wb") as f:
            f.write(blob)
        r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / (tag + ".bin"))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
        bits = "".join(str(a) for a in mix.expected)
        fell_back = "1" if be.ST_PAIRING in status else "0"
        assert got["pairs"] == got["fold"] == bits
        assert [int(x) for x in got["status"].split()] == status
        assert got["pairs_fell_back"] == got["fold_fell_back"] == fell_back
        assert got["one_srs"] == "-1"                      # the same call without the flag: H2V_E_ARG
        assert got["batch_verify"] == ("ok" if tag == "accept" else str(next(s for s in status if s)))
        assert got["workspace"] == "1"
