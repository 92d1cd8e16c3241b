"""The case tables of tests/six_engine_cases.py hold what they are meant to hold: every op has a case ON each bound the six-lane
engine's headroom argument states (csrc/h2v_pairing_six.hpp, tools/gen_six_tables.py), the limb model stays inside its own assertions
on every case (building a table runs them), the real part's columns do go negative and W does wrap somewhere, and the launch layouts
put the hardest case into group 0, group 9 and a lone trailing group.  The device side of the same tables:
tests/test_six_engine_calls_gpu.py."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import six_engine_cases as S

P, g = S.P, S.g


def parts(op, key="a"):
    return [v for c in S.table(op)["cases"] for v in S.flat(c[key])]


@pytest.mark.parametrize("op", S.OPS)
def test_every_table_builds_inside_the_models_assertions(op):
    """table() runs the model on every case: an operand outside the headroom argument fires one of gen_six_tables' assertions here"""
    t = S.table(op)
    assert len(t["cases"]) >= 2 and len(t["cases"]) <= 35          # a few hundred groups per op at most, all of them launched
    for c in t["cases"]:
        wants = list(c["want"].values()) if op == "CSQR" else [c["want"]]
        for w in wants:
            assert len(w) == (8 if op == "PROD2" else 12)
            if op == "FOLD":
                assert all(len(v) == 14 and max(v) < 1 << 28 for v in w)
            else:
                assert all(0 <= v < 1 << 392 for v in w)


def test_mul_sits_on_its_bounds():
    for key in ("a", "b"):
        vals = parts("MUL", key)
        assert max(vals) == 6 * P - 1 and min(vals) == 0
        assert {0, 1, P - 1, P, P + 1, 6 * P - 1} <= set(vals)
    c = S.table("MUL")["cases"]
    assert S.flat(c[0]["a"]) == S.flat(c[0]["b"]) == [6 * P - 1] * 12                      # (max, max)
    assert any(all(re == 6 * P - 1 and im == 0 for re, im in x["a"]) and all(re == 0 and im == 6 * P - 1 for re, im in x["b"]) for x in c)
    assert any(S.flat(x["a"]) == S.flat(x["b"]) == [0] * 12 for x in c)
    assert max(w for x in c for w in x["want"]) < 3 * P                                    # "both below 3p"
    assert {v // P for x in c[11:] for v in S.flat(x["a"])} == set(range(6))               # every t of value + t p


def test_a_real_part_goes_negative_and_w_wraps():
    """re = U - V in two's complement columns: some case has negative columns AND a negative reduced value (the result is below p:
    the `+ p` at the end is what makes it a representative); W wraps modulo 2^64 in some case while W - U - V stays below it."""
    negative = wrapped = False
    for c in S.table("MUL")["cases"][:5]:
        s = S.slots()
        g.stage_a(s, c["a"], 1)
        g.stage_b(s, c["b"])
        for k in range(6):
            re, W = S.kara_columns(S.MT[k], s)
            assert -(1 << 63) < min(re) and max(re) < 1 << 63
            negative |= min(re) < 0 and c["want"][2 * k] < P
            wrapped |= max(W) >= 1 << 64
    assert negative and wrapped


def runs(op, cases):
    """the cases in which the op under test really runs: for the lines those whose own skip bit is clear - a skipped line hands `a` back
    and compares nothing with the model"""
    own = {"LINE1": 1, "LINE2": 2}.get(op, 0)
    return [c for c in cases if not c.get("flags", 0) & own]


@pytest.mark.parametrize("op", ["SQR", "LINE1", "LINE2", "ROUND"])
def test_miller_values_sit_on_the_staging_bounds(op):
    cases = runs(op, S.table(op)["cases"])
    assert S.RE_MAX == 12 * P and S.IM_MAX == 7 * P and g.MILLER_K == 11
    assert S.table(op)["cases"][0] is cases[0] and cases[0]["a"] == [(12 * P, 7 * P)] * 6
    res, ims = [re for c in cases for re, _ in c["a"]], [im for c in cases for _, im in c["a"]]
    assert max(res) == 12 * P and max(ims) == 7 * P and min(res) == 0 and min(ims) == 0
    if op != "ROUND":
        for corner in ((12 * P, 0), (0, 7 * P), (0, 0)):
            assert any(c["a"] == [corner] * 6 for c in cases)
        for v in (12 * P - 1, 12 * P):                                 # re on the bound in every coefficient, im anywhere
            assert any(all(re == v for re, _ in c["a"]) and len({im for _, im in c["a"]}) > 1 for c in cases)
        for v in (7 * P - 1, 7 * P):
            assert any(all(im == v for _, im in c["a"]) and len({re for re, _ in c["a"]}) > 1 for c in cases)
    else:
        assert any(c["a"] == [g.miller_round_bounds()[-1]] * 6 for c in cases)


@pytest.mark.parametrize("op", ["LINE1", "LINE2"])
def test_line_products_and_skips(op):
    cases = S.table(op)["cases"]
    own = 1 if op == "LINE1" else 2
    live, skipped = runs(op, cases), [c for c in cases if c["flags"] & own]
    for v in (0, P, 2 * P - 1):                                        # each T value in a case whose line RUNS
        assert any(c["T"] == [v] * 8 for c in live)
    assert max(v for c in live for v in c["T"]) == 2 * P - 1
    assert sum(1 for c in live if len(set(c["T"])) == 8) >= 10         # products of the model and random values below 2p
    assert cases[0]["T"] == [2 * P - 1] * 8 and cases[0]["flags"] == 0
    assert len(skipped) >= 5 and {c["flags"] for c in cases} == {0, 1, 2, 3}        # the other loop's bit must not matter
    for c in skipped:
        assert c["want"] == S.flat(c["a"]) and any(c["a"] == d["a"] for d in live)     # skip: `a` back unchanged
    for c in live:
        assert c["want"] == S.flat(S.model_line(own, c["a"], c["T"], False)) != S.flat(c["a"])
    # the line grows the staged value by (2p, p) and a little: the largest result is about 14p
    assert 13 * P < max(w for c in live for w in c["want"]) < 15 * P
    for n, order in S.launches(len(cases)):
        if n >= 10:                                                    # skipped groups between running neighbours in every block
            skips = [bool(cases[k]["flags"] & own) for k in order]
            assert any(not a and b and not c for a, b, c in zip(skips, skips[1:], skips[2:]))


def test_round_runs_all_four_skip_combinations_side_by_side():
    cases = S.table("ROUND")["cases"]
    assert cases[0]["flags"] == 0
    for n, order in S.launches(len(cases)):
        if n >= 10:
            assert {cases[k]["flags"] for k in order[:10]} == {0, 1, 2, 3}


@pytest.mark.parametrize("op", ["PROD2", "ROUND"])
def test_line_constants_and_points(op):
    t = S.table(op)
    assert {0, S.MONT1, P - S.MONT1, P - 1} <= set(t["lines"]) and max(t["lines"]) < P
    pts = [v for c in t["cases"] for v in c["pts"]]
    assert {0, S.MONT1, P - S.MONT1, P - 1} <= set(pts) and max(pts) == P - 1           # canonical: what the leader stores
    if op == "PROD2":
        assert max(w for c in t["cases"] for w in c["want"]) < 2 * P


def test_csqr_elements():
    cases = S.table("CSQR")["cases"]
    vals = parts("CSQR")
    assert max(vals) == 6 * P - 1 and min(vals) == 0 and S.flat(cases[0]["a"]) == [6 * P - 1] * 12
    for j, c in enumerate(cases):
        assert sorted(c["want"]) == list(S.CSQR_RUNS if j < S.CSQR_LONG else S.CSQR_RUNS[:4])
        assert len(c["fold_inputs"]) == 12 * max(c["want"])            # every squaring of the run, lane and part
    # the cyclotomic element squares as Fp12 does; the chain of the model is then x^(2^n)
    cyc = cases[S.CSQR_LONG - 1]
    x = S.unmont([(re % P, im % P) for re, im in cyc["a"]])
    assert bls.f12_mul(x, bls.f12_conj(x)) == bls.F12_ONE
    for n in S.CSQR_RUNS:
        w = cyc["want"][n]
        assert S.unmont([(w[2 * k] % P, w[2 * k + 1] % P) for k in range(6)]) == bls.f12_pow(x, 1 << n)


def test_fold_inputs():
    cases = S.table("FOLD")["cases"]
    vecs = [v for c in cases for v in c["a"]]
    vals = [g.limbs_val(v) for v in vecs]
    assert max(vals) == 32 * P - 1
    rng = random.Random(1)
    for v in [k * P + d for k in range(33) for d in (-1, 0, 1) if 0 <= k * P + d < 32 * P]:      # fold()'s own table
        carried, at_max = g.uncarried_forms(v, rng)[:2]
        assert carried in vecs and at_max in vecs                      # ... carried and with every lower limb at its maximum
        assert v < 1 << 364 or max(at_max[:13]) > 1 << 28
    assert sum(1 for v in set(vals) if vals.count(v) >= 3) >= 96       # and in a random uncarried form
    assert vecs[0][:13] == [(1 << 31) - 1] * 13                        # every lower limb at its maximum
    assert sum(1 for v in vecs if v[0] == (1 << 31) - 1) >= 2          # ... and limb 0 there in a form uncarried_forms made
    assert sum(1 for v in vecs if max(v[:13]) >= 1 << 28) > len(vecs) // 3            # uncarried forms
    hs = [x for c in S.table("CSQR")["cases"] for x in c["fold_inputs"]]               # (lane, 3 r -/+ 2 g as the device forms it)
    for sign in (0, 1):                                                # the largest 3 r + 13p - 2g (even lanes) and 3 r + 2g (odd)
        assert max((h for k, h in hs if k % 2 == sign), key=g.limbs_val) in cases[0]["a"]
    assert max(g.limbs_val(h) for _, h in hs) < 20 * P
    for c in cases:
        for src, out in zip(c["a"], c["want"]):
            assert g.limbs_val(out) % P == g.limbs_val(src) % P and g.limbs_val(out) < 2 * P + (P >> 10)


@pytest.mark.parametrize("op", ["CONJ", "FROB", "INV"])
def test_conj_frob_inv_operands(op):
    cases = S.table(op)["cases"]
    vals = parts(op)
    assert max(vals) == 5 * P - 1 and min(vals) == 0
    if op == "CONJ":
        for c in cases:
            for k in range(6):
                for q in range(2):
                    assert c["want"][2 * k + q] == (6 * P - c["a"][k][q] if k & 1 else c["a"][k][q])
    if op == "INV":
        assert [c["ok"] for c in cases].count(0) >= 2                  # zero as 0 and as multiples of p
        for c in cases:
            if c["ok"]:
                x, y = S.unmont([(re % P, im % P) for re, im in c["a"]]), S.unmont([(c["want"][2 * k], c["want"][2 * k + 1]) for k in range(6)])
                assert bls.f12_mul(x, y) == bls.F12_ONE


@pytest.mark.parametrize("op", S.OPS)
def test_positions(op):
    n_cases = len(S.table(op)["cases"])
    layouts = S.launches(n_cases)
    assert [n for n, _ in layouts] == [1, 10, 11, 21]
    seen = set()
    for n, order in layouts:
        assert len(order) == n and order[0] == 0                       # group 0
        if n >= 10:
            assert order[9] == 0                                       # the group lanes 60..63 shadow
        if n % 10 == 1:
            assert order[n - 1] == 0                                   # the lone group of a trailing wave
        for blk in range(0, n, 10):
            others = [k for k in order[blk:blk + 10] if k != 0]
            assert len(set(others)) == min(len(others), n_cases - 1)   # distinct cases in every group of a block
        seen |= set(order)
    assert seen == set(range(n_cases))                                 # the launches together run every case
    long_runs = S.launches(S.CSQR_LONG)                                # the squaring runs of 16 and 32: a handful of elements
    assert {k for _, order in long_runs for k in order} == set(range(S.CSQR_LONG)) and all(order[0] == 0 for _, order in long_runs)
