"""The six-lane engine's cyclotomic squaring with FOUR products per lane (tools/gen_six_tables.py: csqr_table, csqr_engine;
csrc/h2v_pairing_six.hpp: six_csqr_products, six_csqr_run):   re = P1 + P2 - P4,   im = P1 + P3 + P4   over three sets of column accumulators, the
second starting as a copy of the first.  The algebra of every lane kind over the integers, the generator's limb model with every
coefficient at the top of what the squaring may be handed, and the emitted header."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_six_tables as g  # noqa: E402
from plutus_halo2_verifier_gen_amd import bls12_381 as bls  # noqa: E402

P = bls.P
# lane k -> (kind, a, b): the pair of coefficients its Granger-Scott formula reads
KIND = {0: ("even", 0, 3), 3: ("odd", 0, 3), 1: ("xi_odd", 2, 5), 4: ("even", 2, 5), 2: ("even", 1, 4), 5: ("odd", 1, 4)}
V_MAX = 6          # six_csqr is handed representatives below 6p (gen_coop_program.py: check_bounds)


def kind_formula(ty, a, b):
    """the lane's Fp2 value before 3 (.) -/+ 2 g:  even a^2 + xi b^2,  odd 2 a b,  xi-odd 2 xi a b"""
    if ty == "even":
        return bls.f2_add(bls.f2_sqr(a), bls.f2_mul(bls.XI, bls.f2_sqr(b)))
    ab2 = bls.f2_scale(bls.f2_mul(a, b), 2)
    return ab2 if ty == "odd" else bls.f2_mul(bls.XI, ab2)


def staged_values(f):
    """slot -> the INTEGER the squaring's staging puts there (no reduction modulo p: the biased M = re - im + 7p as it stands)"""
    v = {g.ZERO: 0}
    for k in range(6):
        re, im = f[k]
        assert 0 <= re < V_MAX * P and 0 <= im < V_MAX * P
        v[g.A0(k)], v[g.A1(k)] = re, im
        v[g.B0(k)], v[g.B1(k)] = 2 * re, 2 * im
        v[g.C_M(k)] = re - im + 7 * P
        assert v[g.C_M(k)] > 0
    return v


def four_products(row, v):
    return [(v[x] + v[x2]) * v[y] for x, x2, y in row]


def algebra_cases():
    rng = random.Random(41)
    rf = lambda: rng.randrange(P) + rng.randrange(V_MAX) * P        # a representative anywhere below 6p
    out = []
    for _ in range(4):
        out.append([(rf(), rf()) for _ in range(6)])
    # a0 = b0 = 0 with the imaginary parts at the top: the real part at its most negative (re = P1 + P2 - P4 with the largest P4)
    out.append([(0, V_MAX * P - 1 - rng.randrange(P)) for _ in range(6)])
    out.append([(0, V_MAX * P - 1) for _ in range(6)])
    return out


@pytest.mark.parametrize("ty", ["even", "odd", "xi_odd"])
def test_four_products_give_the_lane_kinds_formula(ty):
    tab = g.csqr_table()
    lanes = [k for k in range(6) if KIND[k][0] == ty]
    assert lanes
    for f in algebra_cases():
        v = staged_values(f)
        for k in lanes:
            _, a, b = KIND[k]
            p1, p2, p3, p4 = four_products(tab[k], v)
            assert min(p1, p2, p3, p4) >= 0                       # unsigned operands: every product is a plain non-negative integer
            want = kind_formula(ty, (f[a][0] % P, f[a][1] % P), (f[b][0] % P, f[b][1] % P))
            assert ((p1 + p2 - p4) % P, (p1 + p3 + p4) % P) == want, (ty, k)
            # the value the signed reduction is handed is above -p R (it adds p once at the end)
            assert p1 + p2 - p4 > -P * g.R


def test_no_lane_has_a_null_product():
    for row in g.csqr_table():
        assert len(row) == g.N_CSQR == 4
        for x, x2, y in row:
            assert x != g.ZERO and y != g.ZERO


def cyclotomic_element():
    f = bls.miller_loop(bls.g1_mul(bls.G1_GEN, 4242), bls.g2_mul(bls.G2_GEN, 7))
    t = bls.f12_mul(bls.f12_conj(f), bls.f12_inv(f))
    return bls.f12_mul(bls.f12_frob(bls.f12_frob(t)), t)


def lift(c):
    """the representative of c just below 6p"""
    c %= P
    return c + (V_MAX - 1) * P


def run_model(tab, staged):
    """the generator's limb model on all six lanes; returns (outputs, reduced parts).  csqr_engine asserts the three column
    bounds from the limb bounds of the staged slots, reduce_cols the range of every column of the signed and the unsigned
    reduction and of the result, fold its own bounds."""
    s = g.Slots(); s.put(g.ZERO, 0); s.lam[g.ZERO] = 0
    g.stage_csqr(s, staged)
    outs, reds = [], []
    for k in range(6):
        red = []
        outs.append(g.csqr_engine(tab[k], s, None, k, reduced=red))
        reds.append(red)
        # the three column bounds, restated from the limb bounds of what was staged
        lam3 = lambda t: 14 * (s.lam[t[0]] + s.lam[t[1]]) * s.lam[t[2]]
        p1, p2, p3, p4 = (lam3(t) for t in tab[k])
        assert p1 + p2 + g.RED < (1 << 63) and p4 < (1 << 63) and p1 + p3 + p4 + g.RED < (1 << 64)
    return outs, reds


def test_limb_model_at_the_bounds_chain_of_eight():
    tab = g.csqr_table()
    t = cyclotomic_element()
    staged = [(lift(a * g.R), lift(b * g.R)) for a, b in t]          # Montgomery form, every coefficient in [5p, 6p)
    for step in range(8):
        assert all(5 * P <= c < 6 * P for pair in staged for c in pair)
        outs, reds = run_model(tab, staged)
        for (re, im), (r0, r1) in zip(outs, reds):
            assert r0 < g.CSQR_RE_BOUND and r1 < g.CSQR_IM_BOUND          # 2.2p, 1.2p: what the tail's 3 r -/+ 2 g < 20p rests on
            assert re < 2 * P + (P >> 10) and im < 2 * P + (P >> 10)      # folded
        t = bls.f12_sqr(t)
        assert g.unmont([(x % P, y % P) for x, y in outs]) == t, "squaring %d of the chain" % step
        staged = [(lift(x), lift(y)) for x, y in outs]                # the outputs feed the next squaring, lifted back to the top


def test_limb_model_with_every_limb_at_its_maximum():
    """Every staged coefficient in the carried form with ALL limbs maximal: thirteen limbs of 2^28 - 1 under the largest top limb a
    value below 6p can have.  Such an element is not in the cyclotomic subgroup, so the reference is the lane's own Granger-Scott
    formula  h = 3 (kind formula) -/+ 2 g  over the integers."""
    tab = g.csqr_table()
    top = (V_MAX * P >> 364) - 1
    c = (top << 364) + (1 << 364) - 1
    assert c < V_MAX * P and all((c >> (28 * i)) & g.MASK == g.MASK for i in range(13))
    for staged in ([(c, c)] * 6, [(c, 0)] * 6, [(0, c)] * 6):
        outs, reds = run_model(tab, staged)
        for k in range(6):
            ty, a, b = KIND[k]
            q = kind_formula(ty, (staged[a][0] % P, staged[a][1] % P), (staged[b][0] % P, staged[b][1] % P))
            sign = -2 if k % 2 == 0 else 2
            for part in range(2):
                # engine results carry the Montgomery factor: (x R)(y R) / R = (x y) R, so the formula holds on the staged integers
                # with one factor R^-1 on the products
                want = (3 * q[part] * g.RINV + sign * staged[k][part]) % P
                assert outs[k][part] % P == want, (k, part)
                assert reds[k][part] < (g.CSQR_RE_BOUND, g.CSQR_IM_BOUND)[part]
                assert outs[k][part] < 2 * P + (P >> 10)


def test_emitted_header_has_four_products_and_no_negated_slots():
    hdr = open(os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "six_tables.h")).read()
    assert "#define SIX_N_CSQR 4" in hdr
    assert "C_NA" not in hdr and "C_ND2" not in hdr
    m = re.search(r"SIX_TAB_CSQR\[6\]\[(\d+)\] = \{\n(.*?)\};", hdr, re.S)
    assert m and int(m.group(1)) == 12
    rows = [[int(x) for x in r.split(",")] for r in re.findall(r"\{([0-9, ]+)\}", m.group(2))]
    assert len(rows) == 6
    negated = set(range(12, 19))             # where NA_k (12 + k) and ND2 (18) used to be staged
    for k, row in enumerate(rows):
        assert len(row) == 12, "four products of three slot bytes"
        assert [tuple(row[3 * i:3 * i + 3]) for i in range(4)] == [tuple(t) for t in g.csqr_table()[k]]
        assert not negated & set(row)
