"""CPU tests (no GPU) of keys whose final MSM has more than 64 terms in one sum (vk.WIDE_BUILDERS): the plan loader accepts
them up to H2V_MAX_MSM_TERMS terms per sum, both plan compilers agree on them, and the oracle accepts their forged proofs and
rejects the corruptions with the status the narrow keys reject them with."""
import json
import os
import random
import struct

import pytest

from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth
from plutus_halo2_verifier_gen_amd import vk as V
from tests.plan_loading import plan_loader, with_terms as _with_terms
from tests.test_host_logic import _set_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H2V_E_DEVICE, H2V_E_LIMIT = -3, -4
MAX_TERMS = 4096
# plan header words (csrc/h2v_plan.h)
HW_IVC, HW_N_MAIN_TERMS = 25, 26


def _wide(name):
    vk, td = V.WIDE_BUILDERS[name]()
    return vk, td, PL.compile_plan(vk)


def _load_rc(blob: bytes):
    return plan_loader()(blob)


def _has_gpu():
    return backend.lib().h2v_device_count() > 0


def _oracle_vk(orc, vk):
    return orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))


def test_wide_builders_are_wide_and_apart_from_builders():
    assert not set(V.WIDE_BUILDERS) & set(V.BUILDERS)
    for name in V.WIDE_BUILDERS:
        _, _, pl = _wide(name)
        width = max(pl.n_main_terms, pl.n_terms - pl.n_main_terms - 1) if pl.is_recursive else pl.n_terms
        assert 64 < width <= MAX_TERMS, (name, width)


@pytest.mark.parametrize("name", sorted(V.WIDE_BUILDERS))
def test_wide_plan_passes_host_validation(name):
    """The loader treats a wide plan as it treats simple_mul's: without a GPU it gets as far as the device (H2V_E_DEVICE),
    so every check of the plan itself passed; with one it loads.  (Before segmented sums: H2V_E_LIMIT, more than 64 MSM
    terms per sum.)"""
    ref_rc, _ = _load_rc(PL.compile_plan(V.simple_mul_vk()[0]).to_bytes())
    assert ref_rc == (0 if _has_gpu() else H2V_E_DEVICE)
    _, _, pl = _wide(name)
    rc, msg = _load_rc(pl.to_bytes())
    assert rc == ref_rc, (name, rc, msg)


def test_chip_alone_bls12381_passes_host_validation():
    ref_rc, _ = _load_rc(PL.compile_plan(V.simple_mul_vk()[0]).to_bytes())
    vk, _ = V.bls12381_vk(chip_alone=True)
    rc, msg = _load_rc(PL.compile_plan(vk).to_bytes())
    assert rc == ref_rc, msg


def test_sums_above_the_cap_are_refused():
    """H2V_MAX_MSM_TERMS terms per sum still load (as far as the device), one more is H2V_E_LIMIT naming the width and
    the cap - checked before any device call, so on every machine."""
    base = PL.compile_plan(V.simple_mul_vk()[0]).to_bytes()
    rc, msg = _load_rc(_with_terms(base, MAX_TERMS + 1, MAX_TERMS + 1))
    assert rc == H2V_E_LIMIT, msg
    assert str(MAX_TERMS + 1) in msg and str(MAX_TERMS) in msg and "H2V_MAX_MSM_TERMS" in msg
    if not _has_gpu():
        rc, msg = _load_rc(_with_terms(base, MAX_TERMS, MAX_TERMS))
        assert rc != H2V_E_LIMIT, msg


def test_recursion_sum_above_the_cap_is_refused():
    _, _, pl = _wide("ivc_wide")
    blob = pl.to_bytes()
    w = struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, blob, 8)
    assert w[HW_IVC] == 1
    n_main = w[HW_N_MAIN_TERMS]
    rc, msg = _load_rc(_with_terms(blob, n_main + 1 + MAX_TERMS + 1, n_main))
    assert rc == H2V_E_LIMIT, msg
    assert "acc_right" in msg and str(MAX_TERMS + 1) in msg


@pytest.mark.parametrize("name", sorted(V.WIDE_BUILDERS) + ["bls12381_chip_alone"])
def test_cpp_compiler_matches_plan_py_on_wide_keys(name):
    vk = V.bls12381_vk(chip_alone=True)[0] if name == "bls12381_chip_alone" else V.WIDE_BUILDERS[name]()[0]
    assert backend.plan_compile(vk.to_json()) == PL.compile_plan(vk).to_bytes()


@pytest.mark.parametrize("name", sorted(V.WIDE_BUILDERS))
def test_wide_forged_proofs_accept_and_corruptions_reject(orc, name):
    vk, td, pl = _wide(name)
    ov = _oracle_vk(orc, vk)
    assert pl.proof_len == ov.proof_len and pl.n_main_terms == ov.n_msm_terms
    b = synth.forge_batch(vk, td, 3, seed=5, plan=pl, workers=1)
    for i in range(b.n):
        assert ov.verify(b.proof(i), b.instance_ints(i, vk.n_public_inputs), b.ci(i))
    rng = random.Random(2)
    n_pi = vk.n_public_inputs
    expected_status = {"flip_first_scalar": "pairing", "flip_last_scalar": "pairing", "bad_point_flag": "point",
                       "point_not_on_curve": "point", "point_not_in_subgroup": "point", "noncanonical_scalar": "scalar",
                       "noncanonical_instance": "scalar",
                       "wrong_public_input": "pairing", "wrong_pi": "pairing", "truncated": "short",
                       "infinity_commitment": "pairing", "acc_limb": "point", "acc_scalar": "pairing",
                       "acc_fixed_scalar": "pairing", "acc_sign": "pairing", "acc_vk_hash": "recursion"}
    if vk.recursion_vks is not None:
        expected_status["wrong_public_input"] = "recursion"
    for kind in synth.CORRUPTIONS:
        res = synth.corrupt(pl, b.proof(1), b.instances[32 * n_pi:64 * n_pi], kind, rng)
        if res is None:
            continue
        p2, i2 = res
        inst = [int.from_bytes(i2[32 * k:32 * k + 32], "little") for k in range(n_pi)]
        ok, tr = ov.verify(p2, inst, b.ci(1), trace=True)
        assert not ok
        assert orc.STATUS[tr.status] == expected_status[kind] or (kind == "acc_limb" and orc.STATUS[tr.status] == "pairing"), kind


def test_bls12381_profile_matches_reference_fixture(orc):
    with open(os.path.join(ROOT, "tests", "golden", "chip_profiles.json")) as f:
        ref = json.load(f)["bls12381"]
    lit = dict(V.BLS12381_PROFILE)
    sets = lit.pop("commitment_map_sets")
    for k, v in lit.items():
        assert ref[k] == v, k
    assert [[row[0], len(row)] for row in ref["commitment_map"]] == sets
    vk, _ = V.bls12381_vk(chip_alone=True)
    pl = PL.compile_plan(vk)
    ov = _oracle_vk(orc, vk)
    assert _set_sizes(pl) == V.BLS12381_PROFILE["commitment_map_sets"]
    assert tuple(c for _, c in _set_sizes(pl)) == (41, 2, 5, 4, 11)
    assert len(ov.commitment_map()) == 63
    assert pl.n_terms == 69 == ov.n_msm_terms
    assert PL.compile_plan(V.bls12381_vk()[0]).n_terms == 72
