"""The merged products (f28_dot2: a b + c d, W a^2 + c d with one Montgomery reduction) and the three one-lane G1 formulas built
on them, on the device, through h2v_probe_f28_dot2 (raw 14-limb records, so operands can sit ON the bounds the headers state).
Field results are compared limb for limb with the Python model of tests/test_field_dot2.py, points with bls12_381.py."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.test_field_dot2 import (MASK, P, RINV, dot2_edge_cases, model_dot2, model_dot2_sqr, random_operand, sqr_edge_cases,
                                   value)

pytestmark = pytest.mark.gpu
R392 = 1 << 392


@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


@pytest.mark.parametrize("inline", [False, True])
def test_dot2_matches_the_model_limb_for_limb(be, inline):
    rng = random.Random(41)
    cases = dot2_edge_cases()
    for _ in range(200):
        la, lb, lc, ld = rng.choice([(1, 1, 1, 1), (4, 4, 1, 1), (2, 3, 3, 3), (15, 1, 2, 1), (1, 2, 1, 15), (8, 2, 1, 1)])
        cases.append((random_operand(rng, 32, la), random_operand(rng, 32, lb), random_operand(rng, 32, lc), random_operand(rng, 32, ld)))
    got = be.probe_f28_dot2(be.DOT2_MUL | (be.DOT2_INLINE if inline else 0), *[[c[k] for c in cases] for k in range(4)])
    for (a, b, c, d), t in zip(cases, got):
        assert t == model_dot2(a, b, c, d)
        assert value(t) < 2 * P and value(t) % P == (value(a) * value(b) + value(c) * value(d)) * RINV % P


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("W", [1, 2])
def test_dot2_sqr_matches_the_model_limb_for_limb(be, inline, W):
    rng = random.Random(43 + W)
    cases = [(a, c, d) for w, a, c, d in sqr_edge_cases() if w == W]
    for _ in range(200):
        la, lc, ld = rng.choice([(1, 1, 1), (2, 3, 3), (2, 9, 1), (1, 15, 1), (3, 1, 1)] if W == 2 else [(1, 1, 1), (4, 1, 1), (3, 2, 4), (2, 13, 1)])
        cases.append((random_operand(rng, 20, la), random_operand(rng, 40, lc), random_operand(rng, 40, ld)))
    op = (be.DOT2_SQR if W == 1 else be.DOT2_SQR2) | (be.DOT2_INLINE if inline else 0)
    got = be.probe_f28_dot2(op, [c[0] for c in cases], None, [c[1] for c in cases], [c[2] for c in cases])
    for (a, c, d), t in zip(cases, got):
        assert t == model_dot2_sqr(W, a, c, d)
        assert value(t) < 2 * P and value(t) % P == (W * value(a) ** 2 + value(c) * value(d)) * RINV % P


# ------------------------------------------------------------------------------------------------ points
def record(x_mod_p, v, lam, rng=None):
    """A raw record of class (v, lam) for the field element x (Montgomery form): the representative x R + k p just below v p
    (rng: any k), limbs 0..12 pushed up to [(lam - 1) 2^28, lam 2^28) by borrowing from the limb above."""
    m = x_mod_p * R392 % P
    kmax = (v * P - 1 - m) // P
    val = m + (kmax if rng is None else rng.randrange(kmax + 1)) * P
    limbs = [(val >> (28 * i)) & MASK for i in range(13)] + [val >> 364]
    for i in range(12, -1, -1):                 # top down: each limb lends lam - 1 units to the one below
        if limbs[i + 1] >= lam - 1:
            limbs[i + 1] -= lam - 1
            limbs[i] += (lam - 1) << 28
    assert value(limbs) == val and all(x < lam << 28 for x in limbs[:13]) and limbs[13] < 1 << 32
    return limbs


def jac(pt, z, bounds, rng=None):
    """(X, Y, Z) records of the affine point with the given Z, at the (v, lam) classes in `bounds`"""
    x, y = pt
    (vx, lx), (vy, ly), (vz, lz) = bounds
    return (record(x * z * z % P, vx, lx, rng), record(y * z * z * z % P, vy, ly, rng), record(z, vz, lz, rng))


def affine(rec3):
    X, Y, Z = (value(r) * RINV % P for r in rec3)
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def in_class(rec, v, lam):
    return value(rec) < v * P and all(x < lam << 28 for x in rec[:13])


STORED = ((31, 1), (20, 1), (4, 2))          # csrc/h2v_curve28.hpp: the bounds of every stored point
DBL_IN_MAX = ((43, 1), (20, 1), (97, 2))     # the widest input g1j28_dbl_t states
AFFINE_Q = ((2, 1), (2, 1), (1, 1))


def rand_point(rng):
    return bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R))


@pytest.mark.parametrize("inline", [False, True])
def test_doubling(be, inline):
    rng = random.Random(47)
    pts, recs = [], []
    for k in range(48):
        pt = rand_point(rng)
        z = rng.randrange(1, P)
        bounds = (STORED, DBL_IN_MAX, ((1, 1), (1, 1), (1, 1)))[k % 3]
        pts.append(pt)
        recs.append(jac(pt, z, bounds, rng if k >= 24 else None))     # the first half ON the bounds, the rest anywhere below
    got = be.probe_f28_dot2(be.DOT2_DBL | (be.DOT2_INLINE if inline else 0), recs)
    for pt, (r, _) in zip(pts, got):
        assert affine(r) == bls.g1_mul(pt, 2)
        assert in_class(r[0], 19, 1) and in_class(r[1], 2, 1) and in_class(r[2], 4, 2)     # the stated output bounds


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("neg", [False, True])
def test_mixed_addition(be, inline, neg):
    rng = random.Random(53)
    want, ps, qs = [], [], []
    for k in range(48):
        p, q = rand_point(rng), rand_point(rng)
        ps.append(jac(p, rng.randrange(1, P), STORED, rng if k >= 24 else None))
        qs.append(jac(q, 1, AFFINE_Q, rng if k >= 24 else None))
        want.append(bls.g1_add(p, bls.g1_neg(q) if neg else q))
    got = be.probe_f28_dot2(be.DOT2_MADD | (be.DOT2_INLINE if inline else 0) | (be.DOT2_NEG_Q if neg else 0), ps, qs)
    for w, (r, _) in zip(want, got):
        assert affine(r) == w
        assert in_class(r[0], 8, 1) and in_class(r[1], 2, 1) and in_class(r[2], 2, 1)


@pytest.mark.parametrize("neg", [False, True])
def test_full_addition_and_its_exceptional_returns(be, neg):
    rng = random.Random(59)
    want, ps, qs = [], [], []
    for k in range(60):
        p = rand_point(rng)
        kind = k % 5                      # 0..2: generic, 3: the same point (other coordinates), 4: the opposite point
        q = p if kind == 3 else bls.g1_neg(p) if kind == 4 else rand_point(rng)
        if neg and kind >= 3:
            q = bls.g1_neg(q)             # ... as seen AFTER the subtraction flag
        ps.append(jac(p, rng.randrange(1, P), STORED, rng if k >= 30 else None))
        qs.append(jac(q, rng.randrange(1, P), STORED, rng if k >= 30 else None))
        want.append((kind, bls.g1_mul(p, 2) if kind == 3 else None if kind == 4 else bls.g1_add(p, bls.g1_neg(q) if neg else q)))
    got = be.probe_f28_dot2(be.DOT2_ADD | (be.DOT2_NEG_Q if neg else 0), ps, qs)
    for (kind, w), p_in, (r, rc) in zip(want, ps, got):
        assert rc == (1 if kind == 3 else 2 if kind == 4 else 0)
        if kind == 4:
            assert [list(x) for x in r] == [list(x) for x in p_in]      # "r untouched"
            continue
        assert affine(r) == w
        assert in_class(r[0], 19, 1) and in_class(r[1], 2, 1) and in_class(r[2], 4, 2)
        if kind < 3:
            assert in_class(r[0], 8, 1) and in_class(r[2], 2, 1)
