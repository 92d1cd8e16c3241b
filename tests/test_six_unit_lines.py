"""Miller lines with a unit coefficient (csrc/h2v_pairing_six.hpp), at value level with the package's big-integer arithmetic, and the
generator's extended self-check (two-term line rows against f * (line / c), the limb model's column and staging bounds, the
uncarried fold).

Every line l = c + ((-lambda) xP) w^2 + yP w^3 is divided by its own c (Fp2, a constant of the fixed G2 argument).  Checked
here: no c is zero; K times the normalised Miller value equals the present one COEFFICIENT BY COEFFICIENT with K in Fp2 the
product of the c along the loop's schedule (what the probe's dump relies on); and the final exponentiations are equal, for
valid and invalid pairs, so the accept bit cannot change."""
import os
import random
import sys

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = bls.P, bls.R


def embed(k):
    """an Fp2 element as an Fp12 element (coefficient w^0)"""
    return [k] + [bls.F2_ZERO] * 5


def unit_line(entry, p1):
    lam, c = entry
    ci = bls.f2_inv(c)
    xp, yp = p1
    return [bls.F2_ONE, bls.F2_ZERO, bls.f2_scale(bls.f2_mul(bls.f2_neg(lam), ci), xp), bls.f2_scale(ci, yp), bls.F2_ZERO, bls.F2_ZERO]


def miller_unit(p1, table):
    """(the loop with unit-coefficient lines, K = the product of the c along the same schedule); before the conjugation"""
    f, k, idx = list(bls.F12_ONE), bls.F2_ONE, 0
    for bit in bls.miller_bits():
        f, k = bls.f12_sqr(f), bls.f2_sqr(k)
        for _ in range(2 if bit else 1):
            f = bls.f12_mul(f, unit_line(table[idx], p1))
            k = bls.f2_mul(k, table[idx][1])
            idx += 1
    assert idx == len(table) == 68
    return f, k


def test_six_lane_tables_self_check_with_unit_lines():
    """tools/gen_six_tables.py: self_check now covers the two-term line rows (against bls.f12_mul(a, line / c), on values at the top
    of what the Miller loop stages), the own-coefficient addition inside the reduction, the bound propagation of a whole round
    (squaring + four lines inside re <= 12p, im <= 7p) and the fold on uncarried limbs; and the committed header is its output."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_six_tables as g
    assert g.self_check()
    assert g.N_LINE == 2 and all(len(row) == 2 for loop in (1, 2) for row in g.line_table(loop))
    trail = g.miller_round_bounds()
    assert len(trail) == 5 and trail[-1][0] <= g.MILLER_RE * P and trail[-1][1] <= g.MILLER_IM * P < (g.MILLER_K - 1) * P + P
    hdr = open(os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "six_tables.h")).read()
    assert "#define SIX_N_LINE 2" in hdr and "#define SIX_MILLER_K %d" % g.MILLER_K in hdr
    for loop in (1, 2):
        rows = ",\n    ".join("{" + ", ".join(str(v) for term in row for v in term) + "}" for row in g.line_table(loop))
        assert "SIX_TAB_LINE%d[6][8] = {\n    %s};" % (loop, rows) in hdr


def test_uncarried_fold_exhaustive():
    """f28_fold without the carry pass before it: every multiple of p up to 32p and its neighbours, each carried, with every lower
    limb at its maximum (2^31 - 1 where the value allows) and in random uncarried forms - same residue, below 2p + p / 1024,
    carried limbs; and the quotient estimate is never too large (asserted inside fold)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_six_tables as g
    rng = random.Random(21)
    n_maxed = 0
    for v in [k * P + d for k in range(32) for d in (-1, 0, 1) if k * P + d >= 0] + [32 * P - 1] + [rng.randrange(32 * P) for _ in range(500)]:
        forms = g.uncarried_forms(v, rng)
        n_maxed += all(x > g.FOLD_LIMB_MAX - (1 << 28) for x in forms[1][:13])
        for lim in forms:
            out = g.fold(lim)
            f = g.limbs_val(out)
            assert f % P == v % P and f < 2 * P + (P >> 10) and all(x < (1 << 28) for x in out)
    assert n_maxed > 500          # (the all-maximal form exists for every value above a few 2^364)


def test_unit_coefficient_lines_keep_the_verdict_and_differ_by_a_constant():
    rng = random.Random(22)
    s = rng.randrange(2, R)
    q1 = bls.g2_mul(bls.G2_GEN, s)
    tabs = {1: bls.g2_line_table(q1), 2: bls.g2_line_table(bls.G2_GEN)}
    for tab in tabs.values():
        assert all(c != bls.F2_ZERO for _, c in tab)
    for trial in range(3):
        a = rng.randrange(1, R)
        pa = bls.g1_mul(bls.G1_GEN, a)
        spa = bls.g1_mul(pa, s)
        for er, valid in ((spa, True), (bls.g1_add(spa, bls.G1_GEN), False)):
            pts = {1: pa, 2: bls.g1_neg(er)}
            present = bls.f12_mul(bls.miller_loop(pts[1], q1), bls.miller_loop(pts[2], bls.G2_GEN))
            f1, k1 = miller_unit(pts[1], tabs[1])
            f2, k2 = miller_unit(pts[2], tabs[2])
            # each loop: K_u times the unit-line value is the present one, coefficient by coefficient (K_u at w^0: conj leaves it)
            for f, k, loop in ((f1, k1, 1), (f2, k2, 2)):
                assert bls.f12_mul(bls.f12_conj(f), embed(k)) == bls.miller_loop(pts[loop], q1 if loop == 1 else bls.G2_GEN)
            unit = bls.f12_conj(bls.f12_mul(f1, f2))
            assert bls.f12_mul(unit, embed(bls.f2_mul(k1, k2))) == present
            # the easy part kills K: the values after it are EQUAL, and so is everything that follows
            easy = lambda f: bls.f12_mul(bls.f12_frob(bls.f12_frob(t := bls.f12_mul(bls.f12_conj(f), bls.f12_inv(f)))), t)
            assert easy(unit) == easy(present)
            if trial == 0:
                fe = bls.final_exponentiation(unit)
                assert fe == bls.final_exponentiation(present) and (fe == bls.F12_ONE) == valid
    # a skipped loop (G1 argument at infinity) has no lines and no factor: K is the other loop's alone
    f2, k2 = miller_unit(bls.g1_neg(bls.G1_GEN), tabs[2])
    assert bls.f12_mul(bls.f12_conj(f2), embed(k2)) == bls.f12_mul(bls.miller_loop(None, q1), bls.miller_loop(bls.g1_neg(bls.G1_GEN), bls.G2_GEN))
