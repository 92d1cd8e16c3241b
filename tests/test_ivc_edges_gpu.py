"""GPU tests of the recursion (IVC) fold at the accumulator's edges (tests/ivc_edges.py): the two accumulator slots of the
decompression kernel (acc_coordinate, the is_acc branch of dec_group), the three-group MSM launch or its three separate
ranges, k_ivc_challenge, the fold MSM whose lanes build their own tables, and the pairing engines' el_jac input - on
accumulators whose limbs wrap past p, whose sums are the point at infinity, whose reduction must double or cancel, at the
sign boundary of y, on a point of order 3, with scalars 0 and r - 1, and with the opening point at infinity.

Every expectation is the CPU oracle's (which tests/test_ivc_edges.py pins to the big-integer model on the same table), never
another device path's; every comparison is of integers, bytes or verdict bits.  Forging and the oracle's runs are module
fixtures."""
import json
from concurrent.futures import ThreadPoolExecutor

import pytest

from plutus_halo2_verifier_gen_amd import plan as PL
from tests import ivc_edges as E
from tests.test_gpu_parity import _permute, be  # noqa: F401  (be: the module's backend fixture)
from tests.test_mixed_keys_gpu import SEED, Mix, fx  # noqa: F401  (the shared-SRS fixture)
from tests.test_wide_keys_gpu import wide  # noqa: F401

pytestmark = pytest.mark.gpu
N = 65                                       # two blocks of k_ivc_challenge: 64 proofs and one alone
PAIRING_REACHED = ("accept", "pairing")


class Case:
    """one key, one forged batch of edge accumulators, and what the oracle says of each proof: reason, el', er', the pair"""

    def __init__(self, orc, vk, td, pl, dp, ov, names, seed):
        self.vk, self.td, self.pl, self.dp, self.ov, self.names = vk, td, pl, dp, ov, list(names)
        self.n_pi = vk.n_public_inputs
        self.batch = E.forge(vk, td, pl, self.names, seed)

        def one(i):
            ok, tr = ov.verify(self.batch.proof(i), self.batch.instance_ints(i, self.n_pi), None, trace=True)
            reason = orc.STATUS[tr.status]
            assert ok == (reason == "accept")
            if reason in PAIRING_REACHED:
                return reason, tr.point("el"), tr.point("er"), orc.g1_compress(tr.point("el")) + orc.g1_compress(tr.point("er"))
            return reason, None, None, bytes(96)

        with ThreadPoolExecutor(8) as ex:
            self.oracle = list(ex.map(one, range(self.batch.n)))
        self.reasons = [o[0] for o in self.oracle]
        self.want = [int(r == "accept") for r in self.reasons]
        # the oracle and the table agree (tests/test_ivc_edges.py checks the same on the CPU, with the model as the third)
        assert self.reasons == [E.BY_NAME[name].expected for name in self.names]
        assert self.want == self.batch.expected

    def args(self, idx=None):
        b = self.batch if idx is None else _permute(self.batch, list(idx), self.n_pi)
        return b.proofs, b.proof_off, b.instances, None

    def inst(self, i):
        return self.batch.instances[32 * self.n_pi * i:32 * self.n_pi * (i + 1)]


def _want_status(be, reason, st):
    """the status word the oracle's reason asks for, as test_ivc_fold_on_gpu checks it"""
    if reason == "accept":
        return st == 0
    if reason == "pairing":
        return st == be.ST_PAIRING
    return bool(st & {"point": be.ST_BAD_POINT, "scalar": be.ST_BAD_SCALAR}[reason])


@pytest.fixture(scope="module")
def case(be, orc):
    """the placement batch on the ivc key: 65 proofs cycling through every kind, pi_infinity first, right_equals_fixed in
    lane 63 of the challenge kernel's first block, left_scalar_0 (both accumulator sums infinite) alone in its second"""
    from plutus_halo2_verifier_gen_amd import vk as V
    vk, td = V.ivc_vk()
    pl = PL.compile_plan(vk)
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    c = Case(orc, vk, td, pl, be.DevicePlan(pl.to_bytes(), 0), ov, E.placement(N), seed=17)
    assert set(c.names) == set(E.NAMES) and (c.names[0], c.names[63], c.names[64]) == ("pi_infinity", "right_equals_fixed", "left_scalar_0")
    assert 0 < sum(c.want) < N
    return c


# ---- a
@pytest.mark.parametrize("n", [65, 64, 1])
def test_placement_batch_equals_the_oracle(be, case, n):
    """n = 65: the infinite-sum accumulator is alone in the second block of k_ivc_challenge and the 63 dead lanes beside it
    shadow it through the LDS-staged hash; n = 64: one full block with acc_right == acc_fixed in its last lane; n = 1: the
    opening point at infinity alone (63 dead lanes shadow an el whose encoding is 0xc0...)."""
    got = case.dp.verify_batch(*case.args(range(n)))
    assert list(got) == case.want[:n]
    if n > 1:
        assert 0 < sum(got) < n
    else:
        assert case.names[0] == "pi_infinity" and list(got) == [0]


# ---- b
@pytest.mark.parametrize("name", E.NAMES)
def test_values_per_kind(be, case, name):
    """h2v_trace on one proof of the kind: the verdict, the status word, and - wherever the oracle reaches the pairing - the
    folded el', er' bit for bit and the accumulator's part of the MSM scalars (the oracle's trace has no MSM scalars: those
    are the plan interpreter's, which the forger and the oracle tests already hold against it)."""
    i = case.names.index(name)
    reason, el, er, _pair = case.oracle[i]
    tr = case.dp.trace(case.batch.proof(i), case.inst(i), None)
    assert tr["accept"] == int(reason == "accept")
    assert _want_status(be, reason, tr["status"]), (name, tr["status"])
    if reason in PAIRING_REACHED:
        assert el is not None and er is not None
        assert tr["el"] == el and tr["er"] == er
        m = case.pl.n_main_terms
        assert tr["msm_scalars"][m:] == PL.run_plan(case.pl, case.batch.proof(i), case.batch.instance_ints(i, case.n_pi), None)[0][m:]


# ---- c
def _shape(be, **opts):
    ids = {"lpt": be.OPT_MSM_LANES_PER_TERM, "bs": be.OPT_MSM_BLOCK_SIZE, "tpl": be.OPT_MSM_TERMS_PER_LANE, "engine": be.OPT_PAIRING_ENGINE}
    return [(ids[k], v) for k, v in opts.items()]


SHAPES = {
    # name: (options, lanes per term the three-group launch reports, pairing lanes per proof or None)
    "lpt1": (dict(lpt=1), (1,), None),
    "lpt2_bs256": (dict(lpt=2, bs=256), (2,), None),
    "lpt8": (dict(lpt=8), (8,), None),
    "tpl2": (dict(tpl=2), (1, 2), None),
    "tpl4": (dict(tpl=4), (1, 2), None),
    "engine6": (dict(engine=6), (1, 2), 6),
    "engine64": (dict(engine=64), (1, 2), 64),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_launch_shapes_give_the_same_verdicts(be, case, shape):
    """The placement batch under forced shapes; the ivc key has 45 terms in three groups (28 | 1 | 16) and the fold 4 terms in
    two (2 | 2), and by msm_ladder_shape / launch_msm_range the options reach these launches so:
      lpt=1         three-group launch: one lane per term, 45 lanes per proof, both GLV halves on one accumulator (k_g1_msm_merged);
                    fold launch: 4 lanes per proof, every lane builds BOTH window tables of its point on the spot;
      lpt=2, bs=256 three-group: 90 lanes per proof, two proofs per 256-thread block; fold: 8 lanes per proof, 32 proofs per block,
                    three blocks for 65 proofs;
      lpt=8         three-group: a quad per GLV half (k_g1_msm_quad, 360 lanes: one proof per block, the groups reduced from the
                    quads' first lanes); fold: the quad needs prebuilt tables, which the fold has none of, so no forced shape fits
                    and it takes the fall-back of msm_ladder_shape, two lanes per term in 512-thread blocks (64 proofs per block:
                    proof 64 alone in the second);
      tpl=2, tpl=4  the several-terms-per-lane kernel takes one-group ranges with prebuilt tables only: NEITHER launch of this
                    key is one (three groups; no tables), so both must run exactly as without the option - what this case
                    checks is that the option is ignored, not misapplied (the wide key's separate ranges take it: see below);
      engine 6, 64  MSM shapes as by default; the six-lane and the one-proof-per-wave pairing engines read the folded el_jac.
    The verdicts are the oracle's in every case."""
    opts, lpts, engine = SHAPES[shape]
    ws = be.Workspace(case.dp, N)
    for opt, v in _shape(be, **opts):
        ws.set_option(opt, v)
    assert list(case.dp.verify_batch(*case.args(), ws=ws)) == case.want, shape
    tm = ws.timings()
    assert tm.msm_lanes_per_term in lpts, (shape, tm.msm_lanes_per_term)
    if engine is not None:
        assert tm.pairing_lanes_per_proof == engine
    ws.close()


def test_chunked_workspace_gives_the_same_verdicts(be, case):
    """a laned workspace whose chunk (21) is no multiple of 64 and cuts the 65 proofs into four chunks on two lanes (21, 21, 21,
    2): every chunk's challenge kernel is one partly dead block, and the last chunk holds nothing but acc_right == acc_fixed
    and the infinite sums, which its 62 dead lanes shadow"""
    ws = be.Workspace(case.dp, N, lanes=2, chunk=21)
    assert ws.lanes() == (2, 21) and -(-N // 21) == 4 and case.names[63:] == ["right_equals_fixed", "left_scalar_0"]
    assert list(case.dp.verify_batch(*case.args(), ws=ws)) == case.want
    ws.close()


# ---- d
def test_batch_form_of_the_accepting_kinds(be, case):
    """h2v_verify_batch_rlc with H2V_RLC_FOLD_PAIRS on every accepting proof of the placement batch - left_scalar_0 (both sums
    infinite: el' = el, er' = er), right_scalar_0 and fixed_all_0 (one summand of acc_right_final infinite) among them: one
    pair MSM and one pairing accept the batch without a fall-back."""
    idx = [i for i in range(N) if case.want[i]]
    assert {case.names[i] for i in idx} == set(E.ACCEPTING) and len(idx) > 32
    ws = be.Workspace(case.dp, N)
    acc, fell_back = case.dp.verify_batch_rlc(*case.args(idx), ws=ws, seed=SEED, fold_pairs=True)
    assert list(acc) == [1] * len(idx) and not fell_back
    ok, tm = ws.rlc_result()
    assert ok and tm.msm_terms == len(idx)
    ws.close()


def test_batch_form_falls_back_to_the_oracles_verdicts(be, case):
    ws = be.Workspace(case.dp, N)
    acc, fell_back = case.dp.verify_batch_rlc(*case.args(), ws=ws, seed=SEED, fold_pairs=True)
    assert list(acc) == case.want and fell_back            # (pairing-only rejects are in the batch)
    assert not ws.rlc_result(timings=False)[0]
    ws.close()


def test_prepare_exports_the_oracles_pairs(be, case):
    """h2v_prepare_batch: compress(el') || compress(er') of the oracle's trace for every proof with status 0 - the pairing-only
    rejects included -, 96 zero bytes for a proof rejected before the pairing; h2v_check_pairs on them: the oracle's verdicts"""
    raw, st = case.dp.prepare_batch(*case.args())
    for i in range(N):
        reason, _el, _er, pair = case.oracle[i]
        assert (st[i] == 0) == (reason in PAIRING_REACHED), (case.names[i], st[i])
        if st[i]:
            assert _want_status(be, reason, st[i]) and pair == bytes(96)
        assert raw[96 * i:96 * i + 96] == pair, case.names[i]
    assert raw[:1] != b"\xc0"                              # pi at infinity: el' = c acc_left is finite
    acc, cst = case.dp.check_pairs(raw)
    assert list(acc) == case.want
    for i in range(N):
        want = {"accept": 0, "pairing": be.ST_PAIRING}.get(case.reasons[i], be.ST_BAD_POINT)   # (a zero pair is no point)
        assert cst[i] == want, case.names[i]


# ---- e
@pytest.fixture(scope="module")
def wide_case(be, orc, wide):  # noqa: F811
    """16 proofs of the wide recursive key (81 + 1 + 114 terms): the first sixteen kinds of the table with pi_infinity first and
    left_scalar_0 last, two of the wrapping kinds giving way to the two whose right term doubles / cancels the fixed base it
    meets first in the reduction (term 64 of the 114 here)"""
    vk, td, pl, dp, ov = wide["ivc_wide"]
    names = E.placement(16)
    names[names.index("wrap1_left_y")], names[names.index("wrap1_right_x")] = "right_doubles_a_base", "right_cancels_a_base"
    c = Case(orc, vk, td, pl, dp, ov, names, seed=19)
    assert {"right_equals_fixed", "right_cancels_fixed", "left_scalar_0", "left_scalar_0_reject", "wrap_max_left_x"} <= set(c.names)
    return c


@pytest.mark.parametrize("lpt, bs, tpl", [(0, 0, 0), (2, 256, 0), (2, 64, 0), (2, 256, 2)], ids=["auto", "lpt2_bs256", "lpt2_bs64", "lpt2_bs256_tpl2"])
def test_wide_recursive_key(be, wide_case, lpt, bs, tpl):
    """ivc_wide: by default the three groups' 196 terms fit one block at one lane per term (the three-group launch, the
    reduction of group 2 over 114 lanes).  Two lanes per term in 256-thread blocks - what test_wide_ivc_fold_and_separate_ranges
    forces - do not fit, and the three sums run as separate ranges (162, 2 and 228 lanes per proof); in 64-thread blocks the
    first and the last range are segmented and folded by k_g1_sum_segments; with tpl=2 those two one-group ranges take the
    several-terms-per-lane kernel.  Verdicts and the exported pairs - right_equals_fixed and left_scalar_0 among them - are
    the oracle's under every shape (prepare runs the same launches on the workspace's options)."""
    c = wide_case
    ws = be.Workspace(c.dp, c.batch.n)
    ws.set_option(be.OPT_MSM_LANES_PER_TERM, lpt)
    ws.set_option(be.OPT_MSM_BLOCK_SIZE, bs)
    ws.set_option(be.OPT_MSM_TERMS_PER_LANE, tpl)
    assert list(c.dp.verify_batch(*c.args(), ws=ws)) == c.want and 0 < sum(c.want) < c.batch.n
    raw, st = c.dp.prepare_batch(*c.args(), ws=ws)
    for i, name in enumerate(c.names):
        assert (st[i] == 0) == (c.reasons[i] in PAIRING_REACHED), name
        assert raw[96 * i:96 * i + 96] == c.oracle[i][3], name
    ws.close()
    if (lpt, bs, tpl) == (0, 0, 0):
        for name in ("right_equals_fixed", "left_scalar_0"):
            i = c.names.index(name)
            tr = c.dp.trace(c.batch.proof(i), c.inst(i), None)
            assert tr["accept"] == 1 and tr["status"] == 0 and tr["el"] == c.oracle[i][1] and tr["er"] == c.oracle[i][2], name


# ---- f
MIXED_KINDS = ("left_scalar_0", "right_equals_fixed", "wrap_max_left_x", "right_cancels_fixed", "order3")


@pytest.fixture(scope="module")
def mixed_case(be, orc, fx):  # noqa: F811
    """five edge proofs of the ivc key as it stands on the shared SRS"""
    e = fx["keys"]["ivc"]
    return Case(orc, e["vk"], e["td"], e["pl"], e["dp"], e["ov"], MIXED_KINDS, seed=23)


@pytest.mark.parametrize("mode", ["per-proof", "rlc", "fold-msm"])
def test_mixed_key_call(be, fx, mixed_case, mode):  # noqa: F811
    """one h2v_verify_mixed call that interleaves simple_mul proofs with the five ivc proofs; per proof, with one pairing for
    the call (H2V_MIXED_RLC) and with one bucket MSM as well (H2V_MIXED_FOLD_MSM).  The verdicts are the oracle's; the batch
    modes fall back exactly when the call holds a proof the oracle rejects in the pairing (right_cancels_fixed) - order3 is
    rejected before it and left_scalar_0's infinite sums pass the batch check."""
    c = mixed_case
    sm = fx["clean"]["simple_mul"]
    batches = {"simple_mul": sm, "ivc": c.batch}
    kw = dict(mode="per-proof" if mode == "per-proof" else "rlc", seed=None if mode == "per-proof" else SEED, fold_msm=(mode == "fold-msm"))
    for kinds in (MIXED_KINDS, tuple(k for k in MIXED_KINDS if k != "right_cancels_fixed")):
        order = []
        for j, name in enumerate(kinds):
            order += [("simple_mul", 2 * j), ("ivc", MIXED_KINDS.index(name)), ("simple_mul", 2 * j + 1)]
        mix = Mix(fx["keys"], batches, order)
        reasons = [c.reasons[j] if name == "ivc" else "accept" for name, j in order]
        assert all(sm.expected[j] for name, j in order if name == "simple_mul")
        ws = be.Workspace.multi(fx["plans"], mix.n)
        acc, st, fell_back = be.verify_mixed(fx["plans"], mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, **kw)
        assert list(acc) == [int(r == "accept") for r in reasons], (mode, kinds)
        assert all(_want_status(be, r, s) for r, s in zip(reasons, st)), (mode, st)
        assert fell_back == (mode != "per-proof" and "pairing" in reasons), (mode, kinds)
        ws.close()
