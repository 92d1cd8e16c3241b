"""GPU tests of keys whose commitments - the VK bases of every proof's MSM - are the point at infinity, repeated, or G / -G
(tests/degenerate_keys.py).  The plan loader leaves the table of an infinite base as hipMemset made it and every consumer must
skip the base before it reads the table; equal bases meet in one lane, one partial sum or one bucket, where only the complete
addition law is right.  Every path that carries VK-base terms is held to the CPU oracle here: per-proof pairs and verdicts under
every forced launch shape, the segmented ladders of a wide key, the recursion fold, the batch-accept mode with its fall-back
made visible, the aggregate call and the mixed-key calls.  Expected values come from the oracle and the big-integer models
(tests/agg_model.py, tests/cancel.py, tests/pip_model.py), never from the code under test.  /root/reference is NOT needed.

Which test notices a missing skip.  The table of an identity base is all zeros, so a consumer without its skip adds (0, 0) as
if it were a point and the sum is wrong - every identity meets a non-zero scalar here (asserted from the oracle's trace):
  msm_body, `!g1a_is_inf(base)` (h2v_msm.hpp; k_g1_msm, _merged, _quad)   test_forced_shapes[lpt1 / lpt2 / lpt8 / bs256], test_per_proof_pairs_and_verdicts
      ... its _seg forms and k_g1_sum_segments meeting an infinite partial sum          test_wide_key_segments
      ... its _cond forms behind a failed batch check, k_rlc_group_terms                test_batch_accept_one_reject_in_the_second_group
      ... the three-group launch and the fold of a recursive key                        test_recursive_key
  msm_multi_body, `any_b` (k_g1_msm_multi)                                               test_forced_shapes[tpl2 / tpl3 / tpl4]
  the fixed-base lanes, `any_b` (k_g1_msm_fixed)                                         test_forced_shapes[fix* / hint5]
  k_pip_digits, `any_p` (h2v_pippenger.hpp; pool 1 of the bucket MSM), k_rlc_vk_sum      test_batch_accept_clean_batch_does_not_fall_back, test_aggregate_pair_is_the_models
  k_mixed_vk_sum, the fold MSM over several keys' bases, the grouped phase 1             test_mixed_calls
The infinity branches of the plan-load kernels (k_vk_tables, k_vk_fixed_window_bases, k_vk_fixed_tables) only decide what an
unread table holds: no result depends on them, and what these tests hold is the other half of that bargain - that nothing reads
such a table."""
import random
import struct

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, plan as PL, synth, vk as V
from tests import agg_model, cancel, degenerate_keys as D, pip_model
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_grouped_gpu import Call, _n_records, _spread
from tests.test_mixed_keys import COMMON_S

pytestmark = pytest.mark.gpu
R = bls.R
PRE_PAIRING = ["bad_point_flag", "point_not_in_subgroup", "noncanonical_scalar", "truncated"]
PAIRING_ONLY = ["wrong_pi", "wrong_public_input"]
ACC = ["acc_limb", "acc_scalar", "acc_fixed_scalar", "acc_sign", "acc_vk_hash"]
LABELS = ["fixed0_inf", "perm_last_inf", "all_inf", "all_equal", "gen_and_neg"]
NARROW = [(name, label) for name in ("simple_mul", "lookup_table") for label in LABELS]
# where only the placement of the bases matters: an identity beside finite bases, nothing but identities, nothing but one point
PLACEMENT = [("simple_mul", "fixed0_inf"), ("simple_mul", "all_inf"), ("simple_mul", "all_equal"), ("simple_mul", "gen_and_neg"),
             ("lookup_table", "fixed0_inf"), ("lookup_table", "all_inf"), ("lookup_table", "all_equal")]
N = 130                     # two groups of 64 proofs and a ragged tail
SEED = bytes(range(7, 39))


class Key:
    """a variant with its plan on the device, its oracle, an all-accepting batch and one with rejects, and the oracle's answer to
    the latter: per proof (verdict, compress(el) || compress(er)); built once, never changed"""

    def __init__(self, be, orc, vk, td, n, seed, kinds, fraction=0.4):
        self.vk, self.td, self.n_pi = vk, td, vk.n_public_inputs
        self.pl = PL.compile_plan(vk)
        self.blob = self.pl.to_bytes()
        self.dp = be.DevicePlan(self.blob, 0) if be is not None else None     # (None: the CPU side alone, for choosing seeds)
        self.ov = D.oracle_vk(orc, vk)
        self._clean_traces = None
        self.clean = synth.forge_batch(vk, td, n, seed=seed, plan=self.pl, workers=8 if n >= 64 else 1)
        self.batch = synth.with_rejects(self.pl, self.clean, self.n_pi, fraction=fraction, seed=seed + 1, kinds=kinds)
        self.want = D.oracle_pairs(self.ov, orc, self.batch, self.n_pi)
        self.verdicts = [a for a, _ in self.want]
        self.pairs = b"".join(p for _, p in self.want)
        assert self.verdicts == self.batch.expected
        assert list(self.ov.verify_batch(self.clean.proofs, self.clean.proof_off, self.clean.instances, self.clean.committed, threads=8)) == [1] * n
        # the batch holds an accept, a reject before the pairing and a reject of the pairing alone
        assert any(self.verdicts), "no accepting proof"
        assert any(p == bytes(96) for _, p in self.want), "no reject before the pairing"
        assert any(not a and p != bytes(96) for a, p in self.want), "no reject of the pairing alone"
        # non-vacuity: an identity base meets a non-zero scalar (the oracle's trace), or a kernel's zero-scalar skip would do
        if D.expected_nones(vk)[0]:
            assert any(sc and all(sc) for sc in (D.identity_term_scalars(vk, self.ov, self.batch, i) for i in range(min(n, 8))))

    @staticmethod
    def args(b):
        return b.proofs, b.proof_off, b.instances, b.committed

    def clean_traces(self):
        """the oracle's trace of every proof of the all-accepting batch (computed once)"""
        if self._clean_traces is None:
            b, out = self.clean, []
            for i in range(b.n):
                ok, otr = self.ov.verify(b.proof(i), b.instance_ints(i, self.n_pi), b.ci(i), trace=True)
                assert ok
                out.append(otr)
            self._clean_traces = out
        return self._clean_traces


@pytest.fixture(scope="module")
def keys(be, orc):
    """(name, label) -> Key, built on first use"""
    cache = {}

    def get(name, label, n=N):
        if (name, label, n) not in cache:
            vk, td = D.variant(name, label)
            kinds = PRE_PAIRING + PAIRING_ONLY + (ACC if vk.recursion_vks is not None else [])
            cache[(name, label, n)] = Key(be, orc, vk, td, n, seed=31, kinds=kinds)
        return cache[(name, label, n)]
    return get


def _check(key, dp, ws, tag):
    """verdicts and pairs of the batch with rejects on ws; returns the verify call's timings"""
    b = key.batch
    assert list(dp.verify_batch(*Key.args(b), ws=ws)) == key.verdicts, tag
    tm = ws.timings()
    shape = (tm.msm_lanes_per_term, tm.msm_var_lanes_per_term, tm.g1_msm_fixed_ms)
    raw, st = dp.prepare_batch(*Key.args(b), ws=ws)
    for i in range(b.n):
        assert raw[96 * i:96 * i + 96] == key.want[i][1], (tag, i)
        assert (st[i] == 0) == (key.want[i][1] != bytes(96)), (tag, i)
    return shape


# ---- per-proof mode
@pytest.mark.parametrize("name,label", NARROW, ids=["%s-%s" % c for c in NARROW])
def test_per_proof_pairs_and_verdicts(be, keys, name, label):
    """prepare's pairs are the oracle's compress(el) || compress(er) proof by proof (96 zero bytes where it stops before the
    pairing), verify's verdicts the oracle's - the launcher's own shapes, an ordinary and a laned workspace, and the trace call"""
    key = keys(name, label)
    ws = be.Workspace(key.dp, N)
    _check(key, key.dp, ws, (name, label))
    ws.close()
    laned = be.Workspace(key.dp, N, lanes=2, chunk=50)            # (chunks of 50, 50, 30: none a multiple of 64)
    _check(key, key.dp, laned, (name, label, "laned"))
    laned.close()
    i = key.verdicts.index(1)
    ok, otr = key.ov.verify(key.batch.proof(i), key.batch.instance_ints(i, key.n_pi), key.batch.ci(i), trace=True)
    tr = key.dp.trace(key.batch.proof(i), key.batch.instances[32 * key.n_pi * i:32 * key.n_pi * (i + 1)], key.batch.ci(i))
    assert ok and tr["accept"] == 1 and tr["el"] == otr.point("el") and tr["er"] == otr.point("er")
    sc = D.oracle_vk_scalars(key.ov, otr)
    for t, (kind, idx) in enumerate(key.pl.terms):
        c = D._commitment_of_term(key.pl, t) if kind == PL.TERM_VK_BASE else None
        if c is not None:
            assert tr["msm_scalars"][t] == sc[c], (name, label, t)


# ---- every launch shape that carries VK-base terms
_O = dict(tpl=1, lpt=4, bs=5, fix=6)
SHAPES = {
    # id: (workspace options, fixed-base window bits of the plan or 0, in-flight hint, msm_lanes_per_term codes that prove the shape)
    "lpt1": (dict(lpt=1), 0, 0, (1,)), "lpt2": (dict(lpt=2), 0, 0, (2,)), "lpt8": (dict(lpt=8), 0, 0, (8,)),
    "tpl2": (dict(tpl=2), 0, 0, (18,)), "tpl3": (dict(tpl=3), 0, 0, (19,)), "tpl4": (dict(tpl=4), 0, 0, (20,)),
    "bs256": (dict(bs=256), 0, 0, (1, 2)), "lpt2_bs256": (dict(lpt=2, bs=256), 0, 0, (2,)),
    "fix1": (dict(fix=1), 0, 0, (3,)), "fix2": (dict(fix=2), 0, 0, (3,)), "fix4": (dict(fix=4), 0, 0, (3,)),
    "fix-1": (dict(fix=-1), 0, 0, (1, 2)),
    "fix2_c4": (dict(fix=2), 4, 0, (3,)), "fix1_c8": (dict(fix=1), 8, 0, (3,)), "fix4_c12": (dict(fix=4), 12, 0, (3,)),
    "hint5": ({}, 0, 5, (3,)),
}


def _repeat(b, k):
    off = [0]
    for _ in range(k):
        for i in range(b.n):
            off.append(off[-1] + b.proof_off[i + 1] - b.proof_off[i])
    return synth.Batch(n=b.n * k, proofs=b.proofs * k, proof_off=off, instances=b.instances * k,
                       committed=b.committed * k if b.committed is not None else None, expected=b.expected * k)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_shapes(be, keys, shape):
    """The per-proof MSM under every forced shape (h2v_workspace_set_option, the fixed-base window width of h2v_plan_load_ex, the
    in-flight hint): pairs and verdicts are the oracle's, and h2v_workspace_timings says the forced shape is the one that ran - a
    fall-through to the default shape would not go unnoticed.  With all_inf the fixed-base launch has nothing but skipped lanes;
    with fixed0_inf and two or four bases per lane an infinite and a finite base share a lane; with all_equal lanes and partial
    sums hold one and the same point (the reductions must double)."""
    opts, fix_c, hint, codes = SHAPES[shape]
    for name, label in PLACEMENT:
        key = keys(name, label)
        if hint and name != "simple_mul":
            continue
        dp = be.DevicePlan(key.blob, 0, fixed_base_window_bits=fix_c) if fix_c else key.dp
        ws = be.Workspace(dp, 8 * N if hint else N)
        for k, v in opts.items():
            ws.set_option(_O[k], v)
            assert ws.get_option(_O[k]) == v
        if hint:
            # the hint splits only launches of a quarter of a wave per SIMD (16 terms x 1040 proofs = 260 waves on 1024 SIMDs):
            # the batch eight times over - proof placement is what changes, the expected pairs repeat
            ws.hint_in_flight(hint)
            big = _repeat(key.batch, 8)
            assert list(dp.verify_batch(*Key.args(big), ws=ws)) == key.verdicts * 8, (shape, name, label)
            tm = ws.timings()
            code, fixed_ms = tm.msm_lanes_per_term, tm.g1_msm_fixed_ms
            raw, _st = dp.prepare_batch(*Key.args(big), ws=ws)
            assert raw == key.pairs * 8, (shape, name, label)
        else:
            code, _var, fixed_ms = _check(key, dp, ws, (shape, name, label))
        assert code in codes, (shape, name, label, code)
        assert (fixed_ms > 0) == (codes == (3,)), (shape, name, label, fixed_ms)
        ws.close()
        if dp is not key.dp:
            dp.close()


# ---- wide key
def test_wide_key_segments(be, orc):
    """wide335 last_segment_inf (335 terms: 64 per-proof, 270 commitments of which those of terms 112 .. 333 are the identity,
    -G1 last) through the segmented ladders.  By the shape model (tests/degenerate_keys.py: model_shape; 8 proofs, 1024 SIMDs):
    lpt=2 and the launcher's own choice cut 3 x 112 - segment 1 is nothing but identities, so k_g1_sum_segments adds the point at
    infinity in the middle of its fold, and segment 2 has one live lane; lpt=1 cuts 2 x 168 - segment 1 has one live lane; the
    forced split leaves all 271 VK bases to the fixed-base lanes, 222 of them skipped.  Pairs and verdicts are the oracle's."""
    import torch
    assert 4 * torch.cuda.get_device_properties(0).multi_processor_count == 1024      # (the SIMD count the shape table is for)
    n = D.SHAPE_N
    vk, td = D.variant("wide335", "last_segment_inf")
    key = Key(be, orc, vk, td, n, seed=33, kinds=["wrong_pi", "bad_point_flag"], fraction=0.5)
    T, n_var, n_fix = D.plan_counts(key.pl)
    for opt, oid, val, code in (("none=0", None, 0, 2), ("lpt=1", "lpt", 1, 1), ("lpt=2", "lpt", 2, 2), ("fix=1", "fix", 1, 3)):
        sh = D.model_shape(T, n_var, n_fix, opt)
        ws = be.Workspace(key.dp, n)
        if oid:
            ws.set_option(_O[oid], val)
        got, var, fixed_ms = _check(key, key.dp, ws, opt)
        assert got == code, (opt, got)
        if code == 3:
            assert sh["split"]["on"] == 1 and fixed_ms > 0 and var == sh["split"]["var_lpt"]
        else:
            assert sh["lpt"] == code and sh["n_seg"] > 1 and fixed_ms == 0
        ws.close()
    # the batch-accept mode on the accepting proofs: 222 identities in pool 1 of the bucket MSM
    ws = be.Workspace(key.dp, n)
    acc, fell_back = key.dp.verify_batch_rlc(*Key.args(key.clean), ws=ws, seed=SEED)
    assert list(acc) == [1] * n and not fell_back
    ws.close()


# ---- recursive key
@pytest.mark.parametrize("label", ["inner_fixed_inf", "all_inf"])
def test_recursive_key(be, keys, label):
    """ivc: the accumulator sum acc_right + F over the key's own and the inner key's bases, then the fold.  The three-group launch
    under lpt=1 / lpt=2 (the fold launch then builds its tables on the spot), the laned form, and the batch form over the folded
    pairs (H2V_RLC_FOLD_PAIRS): verdicts and pairs are the oracle's"""
    key = keys("ivc", label, 65)
    assert any(key.batch.expected[i] == 0 for i in range(65))
    for opts, codes in (({}, (1, 2)), (dict(lpt=1), (1,)), (dict(lpt=2, bs=256), (2,))):
        ws = be.Workspace(key.dp, 65)
        for k, v in opts.items():
            ws.set_option(_O[k], v)
        code, _var, _fx = _check(key, key.dp, ws, (label, opts))
        assert code in codes
        ws.close()
    laned = be.Workspace(key.dp, 65, lanes=2, chunk=21)
    _check(key, key.dp, laned, (label, "laned"))
    laned.close()
    # the accumulator's scalars of the identity bases are the interpreter's (public inputs, non-zero: asserted by Key)
    i = key.verdicts.index(1)
    tr = key.dp.trace(key.batch.proof(i), key.batch.instances[32 * key.n_pi * i:32 * key.n_pi * (i + 1)], None)
    m = key.pl.n_main_terms
    assert tr["msm_scalars"][m:] == PL.run_plan(key.pl, key.batch.proof(i), key.batch.instance_ints(i, key.n_pi), None)[0][m:]
    # the batch form: all accepting - one pair MSM, one pairing, no fall-back; with rejects - the oracle's verdicts
    ws = be.Workspace(key.dp, 65)
    acc, fell_back = key.dp.verify_batch_rlc(*Key.args(key.clean), ws=ws, seed=SEED, fold_pairs=True)
    assert list(acc) == [1] * 65 and not fell_back
    ok, tm = ws.rlc_result()
    assert ok and tm.msm_terms == 65
    acc, fell_back = key.dp.verify_batch_rlc(*Key.args(key.batch), ws=ws, seed=SEED, fold_pairs=True)
    assert list(acc) == key.verdicts and fell_back
    ws.close()


# ---- batch-accept mode
def _seed_counter(seed, seed_used):
    """the library's count of seeded calls, read from the seed an aggregate call reports (include/h2v.h: the given seed with the
    count xored into words 5 and 6)"""
    a, b = struct.unpack("<8I", seed), struct.unpack("<8I", bytes(seed_used))
    assert all(a[k] == b[k] for k in (0, 1, 2, 3, 4, 7))
    return (a[5] ^ b[5]) | ((a[6] ^ b[6]) << 32)


def _counter_now(key, seed=SEED):
    """the count the NEXT seeded call of this process mixes in: one aggregate call on two proofs, and one more"""
    two = synth.Batch(n=2, proofs=key.clean.proofs[:key.clean.proof_off[2]], proof_off=key.clean.proof_off[:3],
                      instances=key.clean.instances[:64 * key.n_pi], committed=None, expected=[1, 1])
    _pair, _inc, _st, info = key.dp.aggregate_batch(*Key.args(two), seed=seed)
    return _seed_counter(seed, info.seed_used) + 1


def _vk_sums(key, seed, counter):
    """sum_i r_i s_{i,f} per VK-base term f of the plan over the all-accepting batch, r_i = the coefficient of position i
    (tests/cancel.py), s_{i,f} from the oracle's trace: what k_rlc_vk_sum hands the bucket MSM for pool 1"""
    n_var = D.plan_counts(key.pl)[1]
    which = [D._commitment_of_term(key.pl, t) for t in range(n_var, key.pl.n_main_terms)]
    sums = [0] * len(which)
    for i, otr in enumerate(key.clean_traces()):
        sc, r = D.oracle_vk_scalars(key.ov, otr), cancel.coeff(seed, counter, i)
        for f, c in enumerate(which):
            sums[f] = (sums[f] + r * (sc[c] if c is not None else otr.scalar("v"))) % R
    return sums


def _shared_buckets(key, sums, c, W):
    """(window, half, |digit|, sign pattern) of every bucket of the right-hand bucket MSM that receives one POINT from two VK-base
    terms: equal bases whose signed digits (tests/pip_model.py) of one window of one GLV half have the same magnitude"""
    n_var = D.plan_counts(key.pl)[1]
    rows = {}
    for f, s in enumerate(sums):
        base = key.pl.vk_bases[key.pl.terms[n_var + f][1]]
        if base is None or s == 0:
            continue
        for half, row in enumerate(pip_model.digits(s, 2, c, W)):
            for w, d in enumerate(row):
                if d:
                    rows.setdefault((base, half, w, abs(d)), []).append(d > 0)
    return {k[1:]: v for k, v in rows.items() if len(v) > 1}


@pytest.mark.parametrize("name,label", NARROW, ids=["%s-%s" % c for c in NARROW])
def test_batch_accept_clean_batch_does_not_fall_back(be, keys, name, label):
    """An all-accepting batch in the batch-accept mode (given seed): every verdict 1 and fell_back False - a wrong sum would fall
    back to the per-proof kernels and still return the right verdicts, so fell_back is the only evidence that the bucket MSM
    handled an identity in pool 1 (any_p) and equal bases in one bucket.  The bucket MSM's shape is the model's.  For all_equal the
    seed is picked with the model so that a bucket receives one point twice with the same sign (the bucket sum must double), and
    the count of seeded calls that the coefficients depend on is read before the call and checked after it."""
    key = keys(name, label)
    b = key.clean
    n_terms = b.n * D.plan_counts(key.pl)[1] + D.plan_counts(key.pl)[2]
    c, W, _nb, _chain = pip_model.shape(n_terms, 2)
    seed = SEED
    if label == "all_equal":
        counter = _counter_now(key)
        for k in range(8):
            seed = bytes([k + 1]) * 32
            shared = _shared_buckets(key, _vk_sums(key, seed, counter), c, W)
            if any(len(set(signs)) == 1 for signs in shared.values()):
                break
        assert any(len(set(signs)) == 1 for signs in shared.values()), "no seed of eight puts one point twice into a bucket"
    ws = be.Workspace(key.dp, N)
    ws.set_option(be.OPT_RLC_ROUTE, -1)
    acc, fell_back = key.dp.verify_batch_rlc(*Key.args(b), ws=ws, seed=seed)
    assert list(acc) == [1] * N and not fell_back
    ok, tm = ws.rlc_result()
    assert ok and tm.msm_terms == n_terms and (tm.window_bits, tm.windows) == (c, W)
    ws.close()
    if label == "all_equal":
        assert _counter_now(key) == counter + 2       # (the call under test took `counter`, the reading after it counter + 1)
    # the laned form: every chunk its own check
    laned = be.Workspace(key.dp, N, lanes=2, chunk=50)
    laned.set_option(be.OPT_RLC_ROUTE, -1)
    acc, fell_back = key.dp.verify_batch_rlc(*Key.args(b), ws=laned, seed=seed)
    assert list(acc) == [1] * N and not fell_back
    laned.close()


def _one_reject(key, b, k, seed=9):
    """the all-accepting batch b with proof k replaced by one that only the pairing rejects; the oracle agrees"""
    n_pi = key.n_pi
    p2, i2 = synth.corrupt(key.pl, b.proof(k), b.instances[32 * n_pi * k:32 * n_pi * (k + 1)], "wrong_pi", random.Random(seed))
    proofs = [p2 if i == k else b.proof(i) for i in range(b.n)]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    one = synth.Batch(n=b.n, proofs=b"".join(proofs), proof_off=off, instances=b.instances[:32 * n_pi * k] + i2 + b.instances[32 * n_pi * (k + 1):],
                      committed=b.committed, expected=[int(i != k) for i in range(b.n)])
    assert list(key.ov.verify_batch(one.proofs, one.proof_off, one.instances, one.committed, threads=8)) == one.expected
    return one


@pytest.mark.parametrize("name,label", PLACEMENT, ids=["%s-%s" % c for c in PLACEMENT])
def test_batch_accept_one_reject_in_the_second_group(be, keys, name, label):
    """One pairing-only reject in the second group of a batch that is large enough for the group stage (the accepting batch twice:
    260 proofs = four groups of 64 and a ragged one of 4; the stage runs from 256 proofs).  The batch check fails,
    k_rlc_group_terms gives every group its own VK-base sums (identities among them), the other four groups pass their group
    checks, and the conditional ladders give group 1's other 63 proofs their sums: the verdicts are the oracle's under both ladder
    forms.  That the other groups PASSED is read from what the workspace does next (include/h2v.h, ROUTING): its estimate of
    the rate of failing groups moves a quarter of the way per call, so one failing group in five leaves it at 0.05 and the clean
    batch that follows still takes the batch check (fell_back False) - had every group failed, or with the group stage switched
    off (every group then counts as failed), the estimate is 0.25 > 0.10 and the clean batch is routed to the per-proof kernels."""
    key = keys(name, label)
    twice = _repeat(key.clean, 2)
    one = _one_reject(key, twice, 100)
    assert one.n == 260 >= 256 and one.expected.index(0) // 64 == 1
    for lpt, grp in ((0, 0), (1, 0), (2, 0), (0, -1)):
        ws = be.Workspace(key.dp, one.n)
        ws.set_option(be.OPT_MSM_LANES_PER_TERM, lpt)
        ws.set_option(be.OPT_RLC_GROUP_STAGE, grp)
        acc, fell_back = key.dp.verify_batch_rlc(*Key.args(one), ws=ws, seed=SEED)
        assert fell_back and list(acc) == one.expected, (lpt, grp)
        assert not ws.rlc_result(timings=False)[0]
        acc, fell_back = key.dp.verify_batch_rlc(*Key.args(twice), ws=ws, seed=SEED)
        assert list(acc) == [1] * twice.n and fell_back == (grp < 0), (lpt, grp)
        assert ws.rlc_result(timings=False)[0] == (grp >= 0)
        ws.close()


@pytest.mark.parametrize("opt,value", [("rlc_c", 5), ("rlc_c", 10), ("rlc_chain", 2), ("rlc_chain", 64)])
def test_batch_accept_options_on_an_identity_base(be, keys, opt, value):
    """the bucket MSM's window width and chain length forced (H2V_OPT_RLC_WINDOW_BITS, H2V_OPT_RLC_CHAIN) on fixed0_inf: the clean
    batch passes without a fall-back in the forced shape, the batch with rejects gets the oracle's verdicts"""
    for name in ("simple_mul", "lookup_table"):
        key = keys(name, "fixed0_inf")
        ws = be.Workspace(key.dp, N)
        ws.set_option(be.OPT_RLC_ROUTE, -1)
        ws.set_option({"rlc_c": be.OPT_RLC_WINDOW_BITS, "rlc_chain": be.OPT_RLC_CHAIN}[opt], value)
        acc, fell_back = key.dp.verify_batch_rlc(*Key.args(key.clean), ws=ws, seed=SEED)
        assert list(acc) == [1] * N and not fell_back
        ok, tm = ws.rlc_result()
        n_terms = N * D.plan_counts(key.pl)[1] + D.plan_counts(key.pl)[2]
        want = pip_model.shape(n_terms, 2, forced_c=value if opt == "rlc_c" else 0, forced_chain=value if opt == "rlc_chain" else 0)
        assert ok and (tm.window_bits, tm.windows) == want[:2]
        if opt == "rlc_chain":
            assert tm.max_chain <= value
        acc, fell_back = key.dp.verify_batch_rlc(*Key.args(key.batch), ws=ws, seed=SEED)
        assert list(acc) == key.verdicts and fell_back
        ws.close()


# ---- aggregate
@pytest.mark.parametrize("name", ["simple_mul", "lookup_table"])
@pytest.mark.parametrize("label", ["fixed0_inf", "all_inf"])
def test_aggregate_pair_is_the_models(be, keys, name, label):
    """h2v_aggregate_batch with a given seed: the pair is the big-integer model's (tests/agg_model.py) over the oracle's pairs bit
    for bit - on the batch with rejects (the pairing-only rejects are included, so the pair does not hold), ordinary and laned,
    and on the clean one (it holds for whoever knows the trapdoor)"""
    key = keys(name, label)
    reached = [int(p != bytes(96)) for _, p in key.want]
    for laned in (False, True):
        ws = be.Workspace(key.dp, N, lanes=2, chunk=50) if laned else be.Workspace(key.dp, N)
        pair, inc, st, info = key.dp.aggregate_batch(*Key.args(key.batch), ws=ws, seed=SEED)
        assert list(inc) == reached and info.chunk == (50 if laned else 0)
        assert pair == agg_model.model_pair([p for _, p in key.want], reached, bytes(info.seed_used), info.chunk), laned
        assert not agg_model.holds(pair, key.td.s)
        ws.close()
    clean_pairs = [bls.g1_compress(otr.point("el")) + bls.g1_compress(otr.point("er")) for otr in key.clean_traces()]
    ws = be.Workspace(key.dp, N)
    pair, inc, st, info = key.dp.aggregate_batch(*Key.args(key.clean), ws=ws, seed=SEED)
    assert list(inc) == [1] * N and st == [0] * N
    assert pair == agg_model.model_pair(clean_pairs, [1] * N, bytes(info.seed_used), info.chunk)
    assert agg_model.holds(pair, key.td.s) and pair != bls.g1_compress(None) * 2
    ws.close()


# ---- mixed-key calls
MIXED = ("lookup_table", "sm_fixed0_inf", "sm_all_inf")
FLAG_SETS = {"rlc": dict(mode="rlc"), "fold": dict(mode="rlc", fold_msm=True), "grouped": dict(mode="rlc", fold_msm=True, grouped=True)}


@pytest.fixture(scope="module")
def mx(be, orc):
    """three keys on one SRS: plain lookup_table, simple_mul fixed0_inf, simple_mul all_inf (its VK sum is [v](-G1) alone); 6 / 9 /
    9 accepting proofs; one batch of the all_inf key with a proof that only the pairing rejects"""
    keys, clean = {}, {}
    made = {"lookup_table": V.lookup_table_vk(), "sm_fixed0_inf": D.variant("simple_mul", "fixed0_inf"), "sm_all_inf": D.variant("simple_mul", "all_inf")}
    for k, name in enumerate(MIXED):
        vk, td = V.on_srs(*made[name], COMMON_S)
        pl = PL.compile_plan(vk)
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0), "ov": D.oracle_vk(orc, vk)}
        clean[name] = b = synth.forge_batch(vk, td, 6 if name == "lookup_table" else 9, seed=91 + k, plan=pl, workers=1)
        assert list(keys[name]["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == [1] * b.n
    e, b = keys["sm_all_inf"], clean["sm_all_inf"]
    n_pi = e["vk"].n_public_inputs
    p2, _i2 = synth.corrupt(e["pl"], b.proof(4), b.instances[32 * n_pi * 4:32 * n_pi * 5], "wrong_pi", random.Random(3))
    proofs = [p2 if i == 4 else b.proof(i) for i in range(b.n)]
    bad = dict(clean)
    bad["sm_all_inf"] = synth.Batch(n=b.n, proofs=b"".join(proofs), proof_off=list(b.proof_off), instances=b.instances, committed=None,
                                    expected=[int(i != 4) for i in range(b.n)])
    assert list(e["ov"].verify_batch(bad["sm_all_inf"].proofs, b.proof_off, b.instances, None, threads=2)) == bad["sm_all_inf"].expected
    order = _spread([(name, j) for name in MIXED for j in range(clean[name].n)])
    return {"keys": keys, "clean": clean, "bad": bad, "order": order}


def _mixed_ws(be, mx, laned):
    plans = [mx["keys"][name]["dp"] for name in MIXED]
    ws = be.Workspace.multi(plans, 64, lanes=2, chunk=8) if laned else be.Workspace(plans[0], 64)   # (lookup_table's fits the others)
    assert ws.lanes() == ((2, 8) if laned else (1, 64)) and _n_records(be, ws) == 0
    return ws


@pytest.mark.parametrize("laned", [False, True], ids=["ordinary", "lanes2x8"])
@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_mixed_calls(be, mx, laned, flags):
    """H2V_MIXED_RLC, | FOLD_MSM, | GROUPED over the three keys.  All accepting: every verdict 1 in ONE pass - the record counts are
    those tests/test_mixed_call_records_gpu.py pins for a single pass (one per phase-1 unit and the tail's), and the fold forms'
    sums are the model's L = sum r_i pi_i, R = [s] L: a key whose VK sum is all identities does not disturb its neighbours'.  With
    a pairing-only reject in the all_inf key the verdicts are the oracle's after the second pass."""
    keys, P = mx["keys"], len(MIXED)
    call = Call(keys, mx["clean"], MIXED, mx["order"])
    assert call.n == 24 and len(set(call.plan_of)) == P
    fold = "fold_msm" in FLAG_SETS[flags]
    counter = _counter_now_mixed(be, keys) if fold else None
    ws = _mixed_ws(be, mx, laned)
    acc, st, fb = be.verify_mixed(call.plans, call.plan_of, call.proofs, call.off, call.instances, call.committed, ws=ws, seed=SEED, **FLAG_SETS[flags])
    assert (list(acc), st, fb) == ([1] * 24, [0] * 24, False)
    assert ws.rlc_result(0, timings=False)[0]
    assert _n_records(be, ws) == (2 if flags == "grouped" else P + 1)
    if fold:
        pts = []
        for name, j in call.order:
            pl = keys[name]["pl"]
            o = pl.points[pl.pi_point]
            pts.append(bls.g1_decompress(mx["clean"][name].proof(j)[o:o + 48]))
        want_l = None
        for pos, p in enumerate(pts):
            want_l = bls.g1_add(want_l, bls.g1_mul(p, cancel.coeff(SEED, counter, pos)))
        got_l, got_r = be.probe_mixed_fold_sums(ws)
        assert got_l == want_l and want_l is not None
        assert got_r == bls.g1_mul(want_l, COMMON_S)
    ws.close()
    bad = Call(keys, mx["bad"], MIXED, mx["order"])
    hit = bad.order.index(("sm_all_inf", 4))
    ws = _mixed_ws(be, mx, laned)
    acc, st, fb = be.verify_mixed(bad.plans, bad.plan_of, bad.proofs, bad.off, bad.instances, bad.committed, ws=ws, seed=SEED, **FLAG_SETS[flags])
    assert (list(acc), st, fb) == ([int(i != hit) for i in range(24)], [be.ST_PAIRING if i == hit else 0 for i in range(24)], True)
    ws.close()


def _counter_now_mixed(be, keys):
    e = keys["sm_fixed0_inf"]
    b = synth.forge_batch(e["vk"], e["td"], 2, seed=97, plan=e["pl"], workers=1)
    _pair, _inc, _st, info = e["dp"].aggregate_batch(b.proofs, b.proof_off, b.instances, None, seed=SEED)
    return _seed_counter(SEED, info.seed_used) + 1
