"""Recursion (IVC) fold at the accumulator's edges (tests/ivc_edges.py), on the CPU: the C oracle and the big-integer model
(ivc.fold) - the two independent implementations DESIGN.md section 10 pins the block with - give every kind of the table the
same verdict, the same reason and the same folded pair, and the forger's accumulator hook leaves its default output alone.
The device path against the oracle on the same table: tests/test_ivc_edges_gpu.py."""
import hashlib
import json

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from plutus_halo2_verifier_gen_amd import ivc
from plutus_halo2_verifier_gen_amd import plan as PL
from plutus_halo2_verifier_gen_amd import synth
from plutus_halo2_verifier_gen_amd import vk as V
from tests import ivc_edges as E

P, R = bls.P, bls.R


@pytest.fixture(scope="module")
def case(orc):
    vk, td = V.ivc_vk()
    pl = PL.compile_plan(vk)
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    return vk, td, pl, ov, E.forge(vk, td, pl, E.NAMES, seed=3)


def test_the_table_builds_what_it_says(case):
    """the constructions themselves, on the forged public inputs: which limbs wrap, which sums are infinite, equal or opposite"""
    vk, td, pl, ov, batch = case
    lay, n_pi = ivc.layout(vk), vk.n_public_inputs
    inst = {name: batch.instance_ints(i, n_pi) for i, name in enumerate(E.NAMES)}
    raw = lambda name, key: inst[name][lay[key][0]] * ivc.B224 + inst[name][lay[key][1]] + 1
    for name in E.NAMES:
        assert ("limb_ge_r" in name) == any(v >= R for v in inst[name]), name
    for key in ("left_x", "left_y", "right_x", "right_y"):
        assert P <= raw("wrap1_" + key, key) < 2 * P
        assert all(raw("wrap1_" + key, k2) < P for k2 in ("left_x", "left_y", "right_x", "right_y") if k2 != key)
    top = raw("wrap_max_left_x", "left_x") - 1          # the largest t + k p whose hi stays below r: one more p would not
    assert top >> 98 > P and (top >> 224) < R <= ((top + P) >> 224)
    assert inst["lo_overlap"][lay["left_x"][1]] >= ivc.B224 and raw("lo_overlap", "left_x") < P
    assert raw("y_boundary_hi", "left_y") == (P + 1) // 2 and raw("y_boundary_lo", "left_y") == (P - 1) // 2
    assert raw("wrap1_left_y_boundary", "left_y") == (P + 1) // 2 + P
    assert raw("y_zero_accept", "left_y") == raw("y_zero_reject", "left_y") == P and raw("order3", "left_x") == P

    sums = lambda name: E.acc_sums(vk, inst[name])
    left, right, fixed = sums("left_scalar_0")
    assert left is None and right is not None and right == bls.g1_neg(fixed)
    left, right, fixed = sums("left_scalar_0_reject")
    assert left is None and bls.g1_add(right, fixed) is not None
    left, right, fixed = sums("right_equals_fixed")
    assert right == fixed and right is not None
    left, right, fixed = sums("right_cancels_fixed")
    assert right == bls.g1_neg(fixed) and left is not None
    left, right, fixed = sums("right_scalar_0")
    assert right is None and fixed is not None
    left, right, fixed = sums("fixed_all_0")
    assert fixed is None and right is not None
    # the right term equals / negates the term it meets first in the reduction of group 2, scalar and point
    k = E.reduction_partner(lay["F"]) - 1
    assert (lay["F"], k) == (15, 7)
    base = bls.g1_decompress(bytes.fromhex(ivc.fixed_bases(vk)[k]), False)
    for name, sign in (("right_doubles_a_base", 1), ("right_cancels_a_base", -1)):
        v = inst[name]
        assert v[lay["right_scalar"]] == v[lay["fixed_scalars"][k]] != 0
        assert ivc.coord(v[lay["right_x"][0]], v[lay["right_x"][1]]) == base[0]
        assert ivc.coord(v[lay["right_y"][0]], v[lay["right_y"][1]]) == (base[1] if sign == 1 else P - base[1])
    assert [E.reduction_partner(f) for f in (1, 2, 3, 4, 15, 16, 113)] == [1, 2, 2, 4, 8, 16, 64]
    v = inst["same_point"]
    assert [v[k] for k in lay["left_x"] + lay["left_y"]] == [v[k] for k in lay["right_x"] + lay["right_y"]]
    assert inst["left_scalar_max"][lay["left_scalar"]] == R - 1 and inst["right_scalar_0"][lay["right_scalar"]] == 0
    assert set(E.placement(65)) == set(E.NAMES)
    assert (E.placement(65)[0], E.placement(65)[63], E.placement(65)[64]) == ("pi_infinity", "right_equals_fixed", "left_scalar_0")


@pytest.mark.parametrize("name", E.NAMES)
def test_oracle_and_model_agree_with_the_table(case, orc, name):
    vk, td, pl, ov, batch = case
    i = E.NAMES.index(name)
    proof, inst = batch.proof(i), batch.instance_ints(i, vk.n_public_inputs)
    ok, tr = ov.verify(proof, inst, None, trace=True)
    want = E.BY_NAME[name].expected
    assert orc.STATUS[tr.status] == want and ok == (want == "accept") == bool(batch.expected[i])
    model = E.expected_fold(vk, pl, proof, inst)
    if want in ("accept", "pairing"):
        el2, er2, c = model
        assert tr.point("el") == el2 and tr.point("er") == er2
        assert el2 is not None and er2 is not None           # (a folded point at infinity would need a hash preimage)
        if name == "pi_infinity":                            # el' = c acc_left alone
            o = pl.points[pl.pi_point]
            assert bls.g1_decompress(proof[o:o + 48]) is None and el2 == bls.g1_mul(E.acc_sums(vk, inst)[0], c)
    else:
        assert isinstance(model, ivc.Reject) and model.reason == want


def test_left_scalar_0_folds_to_the_unfolded_pair(case):
    vk, td, pl, ov, batch = case
    i = E.NAMES.index("left_scalar_0")
    proof, inst = batch.proof(i), batch.instance_ints(i, vk.n_public_inputs)
    el2, er2, c = E.expected_fold(vk, pl, proof, inst)
    o = pl.points[pl.pi_point]
    assert el2 == bls.g1_decompress(proof[o:o + 48])
    assert ivc.fold(vk, inst, None, None)[:2] == (None, None)      # both accumulator sums are the point at infinity
    # er' = er: the pair is the plain KZG pair of the forged proof, e(pi, s G2) == e(s pi, G2)
    assert er2 == bls.g1_mul(el2, td.s)


def test_forger_default_is_unchanged_by_the_hook():
    """forge_batch without accumulator= writes the bytes it wrote before the hook existed, rng consumption included: the digest
    of a forged ivc batch (recorded before the change), and the hook handed ivc.make_accumulator reproduces it."""
    vk, td = V.ivc_vk()
    pl = PL.compile_plan(vk)

    def digest(b):
        return hashlib.sha256(b.proofs + b.instances + repr(b.proof_off).encode()).hexdigest()

    plain = synth.forge_batch(vk, td, 3, seed=5, plan=pl, workers=1)
    assert digest(plain) == FORGED_IVC_3_SEED_5
    calls = []

    def hook(vk_, td_, rng, inst, i):
        calls.append(i)
        ivc.make_accumulator(vk_, td_, rng, inst)

    assert digest(synth.forge_batch(vk, td, 3, seed=5, plan=pl, workers=1, accumulator=hook)) == FORGED_IVC_3_SEED_5
    assert calls == [0, 1, 2]
    # a non-recursive key never calls it; a pool of worker processes cannot take it
    sm, std = V.simple_mul_vk()
    spl = PL.compile_plan(sm)
    assert digest(synth.forge_batch(sm, std, 2, seed=5, plan=spl, workers=1, accumulator=hook)) == \
        digest(synth.forge_batch(sm, std, 2, seed=5, plan=spl, workers=1)) and calls == [0, 1, 2]
    with pytest.raises(ValueError):
        synth.forge_batch(vk, td, 64, seed=5, plan=pl, workers=2, accumulator=hook)


# sha256 over proofs || instances || offsets of forge_batch(ivc_vk, 3 proofs, seed=5, workers=1) at the commit before the hook
FORGED_IVC_3_SEED_5 = "ba262d20070884ba69e075baa71ebacc81d4db7a992b76059185cb8531ab69ee"
