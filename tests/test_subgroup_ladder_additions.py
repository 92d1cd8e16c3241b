"""The two additions of the subgroup ladder (csrc/h2v_curve28.hpp: g1j28_madd_complete, g1j28_add_zz as g1j28_mul_x_abs calls
them) as limb-for-limb Python models over the lazily reduced field: every statement of the device formulas, with the multiplier's
operand conditions (lam_a lam_b + lam_c lam_d <= 17, v_a v_b + v_c v_d <= 2048, the 64-bit column - tests/test_field_dot2.py's
model), the 32-bit limbs of every sum and difference, the fold's precondition and the stated (v, lam) of every intermediate
ASSERTED on operands that sit on the bounds the header states.  Then the same models on curve points, exceptional cases
included (p == q, p == -q, points outside the prime-order subgroup), against the package's affine group law."""
import os
import random
import sys

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.test_field_dot2 import MASK, P, RINV, edge_operand, model_dot2, random_operand, value

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_six_tables as six  # noqa: E402  (fold: the model of f28_fold)

RMONT = (1 << 392) % P
ZERO = [0] * 14
MUL_MADS, SQR_MADS, DOT2_MADS = 392, 301, 588


def bias(K, M):
    """tools/gen_device_consts.py: bias(K, M) - K p with every limb below the top in [M 2^28, (M + 2) 2^28)"""
    c = [(K * P >> (28 * i)) & MASK for i in range(13)] + [K * P >> 364]
    sp = M + 1
    out = [c[0] + (sp << 28)] + [c[i] + (sp << 28) - sp for i in range(1, 13)] + [c[13] - sp]
    assert value(out) == K * P
    return out


class El:
    """a field element as the device holds it: 14 limbs and the (v, lam) class the formula's comment claims for it - checked on
    construction against the data"""

    def __init__(self, limbs, v, lam):
        assert all(0 <= x < 1 << 32 for x in limbs), "a limb left 32 bits"
        assert all(x < lam << 28 for x in limbs[:13]), "limb bound (lam) violated"
        assert value(limbs) < v * P, "value bound (v) violated"
        assert lam <= 15
        self.l, self.v, self.lam = list(limbs), v, lam

    @property
    def val(self):
        return value(self.l)


class Count:
    def __init__(self):
        self.mads = 0


def f_mul(cnt, a, b):
    assert a.lam * b.lam <= 17 and a.v * b.v <= 2048
    cnt.mads += MUL_MADS
    return El(model_dot2(a.l, b.l, ZERO, ZERO), 2, 1)


def f_sqr(cnt, a):
    assert a.lam * a.lam <= 17 and a.v * a.v <= 2048
    cnt.mads += SQR_MADS
    return El(model_dot2(a.l, a.l, ZERO, ZERO), 2, 1)


def f_dot2(cnt, a, b, c, d):
    assert a.lam * b.lam + c.lam * d.lam <= 17 and a.v * b.v + c.v * d.v <= 2048
    cnt.mads += DOT2_MADS
    return El(model_dot2(a.l, b.l, c.l, d.l), 2, 1)


def f_add(a, b):
    return El([x + y for x, y in zip(a.l, b.l)], a.v + b.v, a.lam + b.lam)


def f_small(k, a):
    return El([k * x for x in a.l], k * a.v, k * a.lam)


def f_sub(a, b, K, M):
    """F28_SUB: a + (K p spread) - b, limb-wise; needs v_b <= K - 1, lam_b <= M"""
    assert b.v <= K - 1 and b.lam <= M
    bs = bias(K, M)
    assert all(x >= y for x, y in zip(bs, b.l)), "a limb of the difference went negative"
    return El([x + (s - y) for x, s, y in zip(a.l, bs, b.l)], a.v + K, a.lam + M + 2)


def f_neg(b, K, M):
    assert b.v <= K - 1 and b.lam <= M
    bs = bias(K, M)
    assert all(x >= y for x, y in zip(bs, b.l))
    return El([s - y for s, y in zip(bs, b.l)], K, M + 2)


def f_carry(a):
    out, c = [], 0
    for i in range(13):
        t = a.l[i] + c
        assert t < 1 << 32
        out.append(t & MASK)
        c = t >> 28
    assert a.l[13] + c < 1 << 32
    return El(out + [a.l[13] + c], a.v, 1)


def f_fold(a):
    """f28_fold on an uncarried element below 32 p: below 2p + p / 1024 afterwards, carried - called (3, 1) by the formulas"""
    assert a.v <= 32
    out = six.fold(a.l)
    assert value(out) < 2 * P + (P >> 10) and value(out) % P == a.val % P
    return El(out, 3, 1)


def is_zero_v5(a):
    """f28_is_zero_v5: limb patterns of 0, p .. 4p; exact for a carried element below 5p"""
    assert a.lam == 1 and a.v <= 5
    return any(a.l == [(k * P >> (28 * i)) & MASK for i in range(13)] + [k * P >> 364] for k in range(5))


def madd_complete(cnt, X1, Y1, Z1, qx, qy):
    """g1j28_madd_complete, statement for statement.  Returns (code, X3, Y3, Z3)."""
    assert (X1.v, X1.lam) <= (19, 1) and (Y1.v, Y1.lam) <= (2, 1) and (Z1.v, Z1.lam) <= (4, 2) and qx.v <= 2 and qy.v <= 2
    a = f_sqr(cnt, Z1)
    b = f_mul(cnt, qx, a)
    t = f_mul(cnt, Z1, a)
    c = f_mul(cnt, qy, t)
    b = f_sub(b, X1, 20, 1)
    assert (b.v, b.lam) == (22, 4) and all(x < 1 << 30 for x in b.l)
    b = f_fold(b)
    c = f_carry(f_sub(Y1, c, 3, 1))
    assert c.v == 5
    if is_zero_v5(b):
        return (1 if is_zero_v5(c) else 2), None, None, None
    Z3 = f_mul(cnt, Z1, b)
    a = f_sqr(cnt, b)
    t = f_neg(a, 3, 1)
    b = f_mul(cnt, b, t)
    a = f_mul(cnt, X1, t)
    X3 = f_sqr(cnt, c)
    X3 = f_add(X3, b)
    t = f_small(2, a)
    X3 = f_carry(f_add(X3, t))
    assert (X3.v, X3.lam) == (8, 1)
    t = f_add(a, X3)
    assert (t.v, t.lam) == (10, 2)
    Y3 = f_dot2(cnt, c, t, Y1, b)
    return 0, X3, Y3, Z3


def add_zz(cnt, X1, Y1, Z1, qxj, qyj, qzj, zz, zzz):
    """g1j28_add_zz (neg_q = false), statement for statement: both operands with the stored-point bounds"""
    assert X1.v <= 31 and Y1.v <= 20 and (Z1.v, Z1.lam) <= (4, 2)
    assert qxj.v <= 31 and qyj.v <= 20 and (qzj.v, qzj.lam) <= (4, 2)
    U1 = f_mul(cnt, X1, zz)
    S1 = f_mul(cnt, Y1, zzz)
    a = f_sqr(cnt, Z1)
    b = f_mul(cnt, qxj, a)
    t = f_mul(cnt, Z1, a)
    c = f_mul(cnt, qyj, t)
    b = f_carry(f_sub(b, U1, 3, 1))
    c = f_carry(f_sub(S1, c, 3, 1))
    if is_zero_v5(b):
        return (1 if is_zero_v5(c) else 2), None, None, None
    Z3 = f_mul(cnt, f_mul(cnt, Z1, qzj), b)
    a = f_sqr(cnt, b)
    t = f_neg(a, 3, 1)
    b = f_mul(cnt, b, t)
    a = f_mul(cnt, U1, t)
    X3 = f_sqr(cnt, c)
    X3 = f_add(X3, b)
    t = f_small(2, a)
    X3 = f_carry(f_add(X3, t))
    t = f_add(a, X3)
    Y3 = f_dot2(cnt, c, t, S1, b)
    return 0, X3, Y3, Z3


def formula_residues(X1, Y1, Z1, x2, y2, Z2=1):
    """the addition formulas on plain residues (Montgomery factors removed): what the limb model must agree with mod p"""
    U1, S1 = X1 * Z2 * Z2 % P, Y1 * Z2 ** 3 % P
    U2, S2 = x2 * Z1 * Z1 % P, y2 * Z1 ** 3 % P
    H, r = (U2 - U1) % P, (S2 - S1) % P
    V = U1 * H * H % P
    X3 = (r * r - H ** 3 - 2 * V) % P
    return X3, (r * (V - X3) - S1 * H ** 3) % P, Z1 * Z2 * H % P


def plain(e):
    return e.val * RINV % P


def test_mixed_complete_addition_on_the_stated_bounds():
    """every operand at the edge of its class (largest limbs, largest value), and random ones: all limb, column and value
    conditions hold, and the result is X (8,1) Y (2,1) Z (2,1) with the formulas' residues; 3843 multiply-adds"""
    rng = random.Random(11)
    cases = [(edge_operand(19, 1), edge_operand(2, 1), edge_operand(4, 2), edge_operand(2, 1), edge_operand(2, 1))]
    cases += [(random_operand(rng, 19, 1), random_operand(rng, 2, 1), random_operand(rng, 4, 2), random_operand(rng, 2, 1), random_operand(rng, 2, 1))
              for _ in range(40)]
    for x1, y1, z1, qx, qy in cases:
        cnt = Count()
        X1, Y1, Z1, QX, QY = El(x1, 19, 1), El(y1, 2, 1), El(z1, 4, 2), El(qx, 2, 1), El(qy, 2, 1)
        code, X3, Y3, Z3 = madd_complete(cnt, X1, Y1, Z1, QX, QY)
        assert code == 0 and cnt.mads == 6 * MUL_MADS + 3 * SQR_MADS + DOT2_MADS == 3843
        assert (X3.v, X3.lam, Y3.v, Y3.lam, Z3.v, Z3.lam) == (8, 1, 2, 1, 2, 1)
        assert (plain(X3), plain(Y3), plain(Z3)) == formula_residues(plain(X1), plain(Y1), plain(Z1), plain(QX), plain(QY))


def test_jacobian_addition_with_shared_zz_on_the_stated_bounds():
    """stored-point bounds X (31,1) Y (20,1) Z (4,2) on both sides, Z2^2 and Z2^3 handed in as reduced products: 5019
    multiply-adds (the complete addition's 5712 less one square and one product)"""
    rng = random.Random(12)
    # (edge operands on both sides would be the SAME point - the doubling; the second operand sits one p lower)
    pick = [lambda v, lam, d: edge_operand(v - d, lam)] + [lambda v, lam, d: random_operand(rng, v, lam)] * 30
    for f in pick:
        ops = [El(f(31, 1, 0), 31, 1), El(f(20, 1, 0), 20, 1), El(f(4, 2, 0), 4, 2), El(f(31, 1, 1), 31, 1), El(f(20, 1, 1), 20, 1), El(f(4, 2, 1), 4, 2)]
        X1, Y1, Z1, X2, Y2, Z2 = ops
        pre = Count()
        zz = f_sqr(pre, Z2)
        zzz = f_mul(pre, Z2, zz)
        assert pre.mads == SQR_MADS + MUL_MADS == 693
        cnt = Count()
        code, X3, Y3, Z3 = add_zz(cnt, X1, Y1, Z1, X2, Y2, Z2, zz, zzz)
        assert code == 0 and cnt.mads == 5712 - 693
        assert (X3.v, X3.lam, Y3.v, Y3.lam, Z3.v, Z3.lam) == (8, 1, 2, 1, 2, 1)
        assert (plain(X3), plain(Y3), plain(Z3)) == formula_residues(plain(X1), plain(Y1), plain(Z1), plain(X2), plain(Y2), plain(Z2))


def test_ladder_saving_per_point():
    """what the two forms take off the subgroup test of one point: five additions in each chain"""
    assert 5 * (5712 - 3843) + 4 * 693 == 12117


# ----------------------------------------------------------------------------- on curve points
def curve_point(rng, in_subgroup):
    """a random point of y^2 = x^3 + 4; outside the subgroup: as it comes (the cofactor is ~2^126, a random curve point is
    outside r-torsion with overwhelming probability - checked)"""
    while True:
        x = rng.randrange(P)
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is None:
            continue
        pt = (x, y)
        if in_subgroup:
            pt = bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R))
            assert bls.g1_in_subgroup(pt)
        else:
            assert not bls.g1_in_subgroup(pt)
        return pt


def lift(rng, residue, v, lam):
    """a device record of class (v, lam) for the residue (Montgomery form): the residue plus a random multiple of p below v p,
    limbs carried, then spread to lam with borrows from the limb above where lam > 1"""
    m = residue * RMONT % P + rng.randrange(v) * P
    l = [(m >> (28 * i)) & MASK for i in range(13)] + [m >> 364]
    if lam > 1:
        for i in range(13):
            k = min(lam - 1, l[i + 1]) if i < 12 else 0
            k = rng.randrange(k + 1)
            l[i + 1] -= k
            l[i] += k << 28
    assert value(l) == m
    return l


def jacobian(rng, pt, vx, vy):
    """pt as (X, Y, Z) device records with a random Z of class (4, 2)"""
    z = rng.randrange(1, P)
    return (El(lift(rng, pt[0] * z * z % P, vx, 1), vx, 1), El(lift(rng, pt[1] * z ** 3 % P, vy, 1), vy, 1), El(lift(rng, z, 4, 2), 4, 2))


def to_affine(X3, Y3, Z3):
    zi = bls.fp_inv(plain(Z3))
    return (plain(X3) * zi * zi % P, plain(Y3) * zi ** 3 % P)


@pytest.mark.parametrize("in_subgroup", [True, False])
def test_additions_match_the_group_law_with_exceptional_cases(in_subgroup):
    rng = random.Random(13 if in_subgroup else 14)
    for trial in range(6):
        base = curve_point(rng, in_subgroup)
        qx, qy = El(lift(rng, base[0], 1, 1), 2, 1), El(lift(rng, base[1], 1, 1), 2, 1)
        for k, want_code in ((rng.randrange(2, 1 << 64), 0), (1, 1), (-1, 2)):
            acc = bls.g1_mul(base, k)
            want = bls.g1_add(acc, base)
            # first chain: the base is affine
            X1, Y1, Z1 = jacobian(rng, acc, 19, 2)
            code, X3, Y3, Z3 = madd_complete(Count(), X1, Y1, Z1, qx, qy)
            assert code == want_code
            if code == 0:
                assert to_affine(X3, Y3, Z3) == want
            else:
                assert (want is None) == (code == 2)
            # second chain: the base is Jacobian, its Z^2 and Z^3 computed once
            X2, Y2, Z2 = jacobian(rng, base, 19, 2)
            cnt = Count()
            zz = f_sqr(cnt, Z2)
            zzz = f_mul(cnt, Z2, zz)
            for _ in range(2):                      # (the same zz, zzz serve every addition of the chain)
                X1, Y1, Z1 = jacobian(rng, acc, 19, 2)
                code, X3, Y3, Z3 = add_zz(cnt, X1, Y1, Z1, X2, Y2, Z2, zz, zzz)
                assert code == want_code
                if code == 0:
                    assert to_affine(X3, Y3, Z3) == want


def test_small_order_point_takes_the_exceptional_branches():
    """A point of order 3 on an a = 0 curve (x = 0): [2]P = -P, so the ladder's first addition after a doubling is P + (-P) -
    return code 2 - and a point with H == 0, R == 0 is the doubling.  The device's subgroup test runs on such inputs (proof bytes
    are adversarial); y^2 = x^3 + 4 has the points (0, +-2)."""
    rng = random.Random(15)
    pt = (0, 2)
    assert bls.g1_is_on_curve(pt) and bls.g1_mul(pt, 3) is None and bls.g1_mul(pt, 2) == bls.g1_neg(pt)
    qx, qy = El(lift(rng, pt[0], 1, 1), 2, 1), El(lift(rng, pt[1], 1, 1), 2, 1)
    X1, Y1, Z1 = jacobian(rng, bls.g1_mul(pt, 2), 19, 2)
    assert madd_complete(Count(), X1, Y1, Z1, qx, qy)[0] == 2
    X1, Y1, Z1 = jacobian(rng, pt, 19, 2)
    assert madd_complete(Count(), X1, Y1, Z1, qx, qy)[0] == 1
