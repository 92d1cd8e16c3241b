"""h2v_check_pairs_multi (include/h2v.h: ONE batch check over pairs on several SRS - C + 1 Miller loops, one final exponentiation),
what can be said without a GPU: header, binding, Python API and C++ wrapper agree on the symbols and the constant; the argument
rules that are decided before a device is touched; no device is H2V_E_DEVICE in every layer; and the equation, the coefficient
rule and their soundness on cancelling errors in a big-integer model (tests/pairs_multi_model.py).  GPU legs:
tests/test_pairs_multi_srs_gpu.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import pairs_multi_model as M
from tests.test_mixed_keys import PKG, ROOT, be  # noqa: F401  (module fixture)

E_ARG, E_DEVICE, E_LIMIT = -1, -3, -4
S_A, S_B, S_C = 0x5a17 << 64 | 11, 0x5b29 << 64 | 13, 0x5c3b << 64 | 17        # the three SRS secrets of these tests
SEED = bytes(range(32))


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_and_constant_agree_in_header_binding_and_wrappers(be):
    h, hpp = _text("include", "h2v.h"), _text("include", "h2v.hpp")
    assert int(re.search(r"#define\s+H2V_MULTI_SRS_MAX\s+(\d+)u", h).group(1)) == 16 == be.MULTI_SRS_MAX
    for sym in ("h2v_check_pairs_multi", "h2v_check_pairs_multi_device"):
        assert re.search(r"\bint %s\(" % sym, h), sym
        assert sym in be.EXPORTS
        getattr(be.lib(), sym)                                   # the built library exports it
    assert "check_pairs_multi" in hpp and "h2v_check_pairs_multi(" in hpp
    # the header states the contract
    for phrase in ("grouped in ranges", "position in the CALL", "C + 1 Miller loops", "group stage of h2v_check_pairs_rlc is left out",
                   "n_plans > H2V_MULTI_SRS_MAX", "never\n *   chunked, routed or coalesced"):
        assert phrase in h, phrase
    from plutus_halo2_verifier_gen_amd import api
    assert inspect.signature(api.verify_mixed).parameters["across_srs"].default is False
    assert list(inspect.signature(api.check_pairs_multi).parameters) == ["verifiers_and_pairs", "seed"]
    assert list(inspect.signature(be.check_pairs_multi).parameters) == ["plans", "counts", "pairs", "ws", "seed"]
    assert "k_pairing_rlc_multi" in _text("plutus_halo2_verifier_gen_amd", "csrc", "h2v_pairing_coop.hpp")


def test_argument_rules_that_need_no_device(be):
    L = be.lib()
    acc = (C.c_uint8 * 4)()
    pairs = bytes(96)
    many = (C.c_void_p * (be.MULTI_SRS_MAX + 1))()               # null plans: the rules below come before anything looks at one
    counts = (C.c_uint64 * (be.MULTI_SRS_MAX + 1))(*([1] * (be.MULTI_SRS_MAX + 1)))
    host = lambda n_plans, opts=None: L.h2v_check_pairs_multi(many, n_plans, counts, pairs, acc, None, None, opts, None)
    dev = lambda n_plans, opts=None: L.h2v_check_pairs_multi_device(many, n_plans, counts, C.addressof(acc), C.addressof(acc), None, None, None, opts)
    for call in (host, dev):
        assert call(0) == E_ARG and "at least one plan" in L.h2v_last_error().decode()
        assert call(be.MULTI_SRS_MAX + 1) == E_LIMIT and "16" in L.h2v_last_error().decode()
        assert call(be.MULTI_SRS_MAX) == E_ARG and "plans[0]" in L.h2v_last_error().decode()        # a null plan
        assert call(1) == E_ARG and "plans[0]" in L.h2v_last_error().decode()
        for flag in (be.RLC_SEED_TRANSCRIPT, be.RLC_SEED_KEYED, be.RLC_FOLD_PAIRS, be.RLC_GROUPED):
            for extra in (0, be.RLC_SEED_GIVEN):
                o = be.RlcOpts((C.c_uint8 * 32)(), flag | extra)
                assert call(1, C.byref(o)) == E_ARG, (flag, extra)
                assert "plans[0]" not in L.h2v_last_error().decode()                                  # refused as a flag, not as a plan
        o = be.RlcOpts((C.c_uint8 * 32)(), 8)                    # the unassigned bit
        assert call(1, C.byref(o)) == E_ARG and "unknown flag" in L.h2v_last_error().decode()
        o = be.RlcOpts((C.c_uint8 * 32)(), be.RLC_SEED_GIVEN | be.RLC_ONE_STREAM)
        assert call(1, C.byref(o)) == E_ARG and "plans[0]" in L.h2v_last_error().decode()           # accepted flags: on to the plans
    assert L.h2v_check_pairs_multi(None, 1, counts, pairs, acc, None, None, None, None) == E_ARG
    # the Python layers refuse what they can see
    with pytest.raises(be.H2VError, match="one entry per plan"):
        be.check_pairs_multi([], [1], pairs)
    from plutus_halo2_verifier_gen_amd import api
    with pytest.raises(ValueError, match="across_srs needs mode='rlc'"):
        api.verify_mixed([], [], [], across_srs=True)
    assert api.verify_mixed([], [], [], mode="rlc", across_srs=True) == []
    assert api.check_pairs_multi([]) == ([], [])
    pa, pb = api.ParamsVerifierKZG(bls.g2_compress(M.s_g2(S_A))), api.ParamsVerifierKZG(bls.g2_compress(M.s_g2(S_B)))
    from plutus_halo2_verifier_gen_amd import vk as V
    vk_c = V.on_srs(*V.simple_mul_vk(seed=3), S_C)[0]
    vk_a, vk_b = V.on_srs(*V.simple_mul_vk(seed=1), S_A)[0], V.on_srs(*V.simple_mul_vk(seed=2), S_B)[0]
    agg = api.Aggregator([pa, pb])
    with pytest.raises(ValueError, match="s_g2 differs"):       # a key on none of them: today's error
        agg.push(vk_c, [], [])
    with pytest.raises(ValueError, match="one push is one pair on one SRS"):
        agg.push_mixed([vk_a, vk_b], [b"", b""], [[], []])
    with pytest.raises(ValueError, match="s_g2 differs"):
        api.Aggregator(pa).push(vk_b, [], [])                    # one SRS: as ever
    with pytest.raises(ValueError, match=r"vks\[1\]"):
        api.batch_verify([pa, pb], [vk_a, vk_c], [[], []], [b"", b""])
    assert agg.finish() == ([], [])


def test_no_device_is_an_error_in_every_layer(be, tmp_path):
    """without a GPU nothing loads a plan: the Python layers raise H2V_E_DEVICE from the key's upload and the C++ driver ends with
    error -3 - never a detour around the device"""
    if be.device_count() >= 1:
        return                  # (a machine with a GPU: tests/test_pairs_multi_srs_gpu.py drives the same layers to their results)
    from plutus_halo2_verifier_gen_amd import api, plan as PL, vk as V
    vk = V.on_srs(*V.simple_mul_vk(seed=1), S_A)[0]
    pl = PL.compile_plan(vk)
    with pytest.raises(be.H2VError) as e:
        api.check_pairs_multi([(api.verifier_for(vk), [M.compress(M.pair_on(S_A, 5))])])
    assert "h2v error %d" % E_DEVICE in str(e.value)
    out = str(tmp_path / "h2v_pairs_multi_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_pairs_multi_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    key = str(tmp_path / "simple_mul.bin")
    with open(key, "wb") as f:
        f.write(pl.to_bytes())
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write(key + "\n")
    with open(str(tmp_path / "pairs.bin"), "wb") as f:
        f.write((1).to_bytes(4, "little") + (1).to_bytes(4, "little") + M.compress(M.pair_on(S_A, 5)))
    r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / "pairs.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout.startswith("error -3 "), r.stdout + r.stderr


# ---- the big-integer model
@pytest.fixture(scope="module")
def srs():
    return {"a": (S_A, M.s_g2(S_A)), "b": (S_B, M.s_g2(S_B)), "c": (S_C, M.s_g2(S_C))}


def test_model_coefficient_rule():
    """by position through the whole call, 128 bits, never shared between two positions, and another call's are others"""
    rs = M.coefficients(SEED, 7, 6)
    assert len(set(rs)) == 6 and all(0 < r < 1 << 128 for r in rs)
    assert rs[4] == M.cancel.coeff(SEED, 7, 4)                       # position 4 of the CALL, whichever range it lies in
    assert not set(rs) & set(M.coefficients(SEED, 8, 6))


def test_model_accepting_ranges_pass(srs):
    (sa, qa), (sb, qb), (sc, qc) = srs["a"], srs["b"], srs["c"]
    ranges = [(qa, [M.pair_on(sa, 3), M.pair_on(sa, 4), (None, None)]), (qb, []), (qb, [M.pair_on(sb, 5)]), (qc, [M.pair_on(sc, 6)])]
    ok, loops = M.multi_check(ranges, M.coefficients(SEED, 1, 5))
    assert ok and loops == 4                                         # three ranges with pairs + G2; the empty range costs none
    # each pair's own equation is what the product is made of
    assert bls.pairing_check_eq(M.pair_on(sb, 5)[0], qb, M.pair_on(sb, 5)[1], bls.G2_GEN)
    assert not bls.pairing_check_eq(M.pair_on(sb, 5)[0], qa, M.pair_on(sb, 5)[1], bls.G2_GEN)
    # an all-infinite call: no loop at all, and it passes
    assert M.multi_check([(qa, [(None, None)]), (qb, [(None, None)])], M.coefficients(SEED, 2, 2)) == (True, 0)


def test_model_a_pair_in_the_wrong_range_fails(srs):
    (sa, qa), (sb, qb) = srs["a"], srs["b"]
    good = [(qa, [M.pair_on(sa, 3)]), (qb, [M.pair_on(sb, 5), M.pair_on(sb, 7)])]
    assert M.multi_check(good, M.coefficients(SEED, 3, 3))[0]
    moved = [(qa, [M.pair_on(sa, 3)]), (qb, [M.pair_on(sa, 5), M.pair_on(sb, 7)])]      # valid under s_a, placed in the s_b range
    assert not M.multi_check(moved, M.coefficients(SEED, 3, 3))[0]


def test_model_cancelling_errors_across_srs(srs):
    """R = [a1 s_a + d]G1 in range a, R = [a2 s_b - d]G1 in range b: the errors cancel under EQUAL weights - which is why the
    coefficients must differ - and under the rule's coefficients only when d is split by exactly those two"""
    (sa, qa), (sb, qb) = srs["a"], srs["b"]
    d = 0x1234567
    plain = [(qa, [M.pair_on(sa, 3), M.pair_on(sa, 9, d)]), (qb, [M.pair_on(sb, 5, -d)])]
    assert M.multi_check(plain, [1, 1, 1])[0]                        # equal weights: passes, though two pairs fail alone
    assert not bls.pairing_check_eq(plain[0][1][1][0], qa, plain[0][1][1][1], bls.G2_GEN)
    rs = M.coefficients(SEED, 4, 3)
    assert not M.multi_check(plain, rs)[0]                            # the rule's coefficients: rejected
    ea, eb = M.cancelling_errors(rs[1], rs[2], d)
    split = [(qa, [M.pair_on(sa, 3), M.pair_on(sa, 9, ea)]), (qb, [M.pair_on(sb, 5, eb)])]
    assert M.multi_check(split, rs)[0]                                # split by this call's own two coefficients: passes
    assert not M.multi_check(split, M.coefficients(SEED, 5, 3))[0]    # ... and the next call's reject it
    swapped = [(qa, [M.pair_on(sa, 9, ea), M.pair_on(sa, 3)]), (qb, [M.pair_on(sb, 5, eb)])]
    assert not M.multi_check(swapped, rs)[0]                          # ... and so does another position in the range
