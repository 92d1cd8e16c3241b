"""The merged product of the lazily reduced field (csrc/h2v_field.hpp: fp_mont28_dot2, fp_mont28_dot2_sqr) as a limb-for-limb
Python model: the same product-scanning loop, with the 64-bit rolling column ASSERTED at every step, run on operands that sit on
the bounds csrc/h2v_fp28.hpp states (every limb at its maximal lam, values at their maximal v, lam_a lam_b + lam_c lam_d = 17
exactly) - a column overflow shows only there.  tests/test_field_dot2_gpu.py runs the same operands on the device and compares
limb for limb with this model."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

P = bls.P
RBITS = 392
RINV = pow(1 << RBITS, -1, P)
MASK = (1 << 28) - 1
MOD28 = [(P >> (28 * i)) & MASK for i in range(14)]
N0_28 = (-pow(P, -1, 1 << 28)) % (1 << 28)


class ColumnOverflow(AssertionError):
    pass


def _col(acc):
    if acc >= 1 << 64:
        raise ColumnOverflow("the rolling column left 64 bits")
    return acc


def value(limbs):
    return sum(x << (28 * i) for i, x in enumerate(limbs))


def model_dot2(a, b, c, d):
    """fp_mont28_dot2, statement for statement"""
    assert all(0 <= x < 1 << 32 for v in (a, b, c, d) for x in v)
    m, t, acc = [0] * 14, [0] * 14, 0
    for k in range(14):
        for i in range(k + 1):
            acc = _col(acc + a[i] * b[k - i])
        for i in range(k + 1):
            acc = _col(acc + c[i] * d[k - i])
        for i in range(k):
            acc = _col(acc + m[i] * MOD28[k - i])
        m[k] = ((acc & 0xffffffff) * N0_28) & MASK
        acc = _col(acc + m[k] * MOD28[0])
        assert acc & MASK == 0
        acc >>= 28
    for k in range(14, 27):
        for i in range(k - 13, 14):
            acc = _col(acc + a[i] * b[k - i])
        for i in range(k - 13, 14):
            acc = _col(acc + c[i] * d[k - i])
        for i in range(k - 13, 14):
            acc = _col(acc + m[i] * MOD28[k - i])
        t[k - 14] = acc & MASK
        acc >>= 28
    assert acc < 1 << 32
    t[13] = acc
    return t


def model_dot2_sqr(W, a, c, d):
    """fp_mont28_dot2_sqr<W>, statement for statement"""
    assert all(0 <= x < 1 << 32 for v in (a, c, d) for x in v)
    o = [x * 2 * W for x in a]
    assert all(x < 1 << 32 and y * W < 1 << 32 for x, y in zip(o, a)), "the scaled operand left 32 bits"
    m, t, acc = [0] * 14, [0] * 14, 0
    for k in range(27):
        lo = 0 if k < 14 else k - 13
        i = lo
        while 2 * i < k:
            acc = _col(acc + o[i] * a[k - i])
            i += 1
        if k % 2 == 0:
            acc = _col(acc + (a[k // 2] * W) * a[k // 2])
        for i in range(lo, min(k, 13) + 1):
            acc = _col(acc + c[i] * d[k - i])
        if k < 14:
            for i in range(k):
                acc = _col(acc + m[i] * MOD28[k - i])
            m[k] = ((acc & 0xffffffff) * N0_28) & MASK
            acc = _col(acc + m[k] * MOD28[0])
            assert acc & MASK == 0
        else:
            for i in range(lo, 14):
                acc = _col(acc + m[i] * MOD28[k - i])
            t[k - 14] = acc & MASK
        acc >>= 28
    assert acc < 1 << 32
    t[13] = acc
    return t


def edge_operand(v, lam):
    """The largest record of class (v, lam): limbs 0..12 at lam 2^28 - 1, the top limb as large as value < v p allows."""
    low = [(lam << 28) - 1] * 13
    top = (v * P - 1 - value(low)) >> 364
    assert top >= 0
    r = low + [top]
    assert (v - 1) * P < value(r) < v * P and top < 1 << 28
    return r


def random_operand(rng, v, lam):
    low = [rng.randrange(lam << 28) for _ in range(13)]
    top = rng.randrange(((v * P - 1 - value(low)) >> 364) + 1)
    r = low + [top]
    assert value(r) < v * P
    return r


# (v_a, lam_a, v_b, lam_b, v_c, lam_c, v_d, lam_d): lam_a lam_b + lam_c lam_d = 17 and v_a v_b + v_c v_d = 2048, both exactly
DOT2_EDGES = [
    (32, 4, 32, 4, 32, 1, 32, 1),
    (45, 1, 45, 1, 23, 4, 1, 4),
    (2047, 15, 1, 1, 1, 2, 1, 1),
    (1, 1, 2047, 15, 1, 1, 1, 2),
    (16, 8, 64, 2, 1024, 1, 1, 1),
    (64, 3, 16, 5, 32, 2, 32, 1),
    (23, 4, 10, 2, 20, 1, 2, 1),        # the mixed addition's own Y3 (lam 9, v 270): inside the bounds, for the record
]
# (W, v_a, lam_a, v_c, lam_c, v_d, lam_d): W lam_a^2 + lam_c lam_d = 17 and W v_a^2 + v_c v_d = 2048
SQR_EDGES = [
    (1, 45, 4, 23, 1, 1, 1),
    (1, 32, 1, 32, 4, 32, 4),
    (1, 32, 3, 1024, 2, 1, 4),
    (1, 2, 2, 1022, 13, 2, 1),
    (2, 31, 2, 126, 3, 1, 3),
    (2, 31, 1, 63, 15, 2, 1),
    (2, 4, 2, 6, 3, 28, 1),             # the doubling's own -Y3 (lam 11, v 200)
]


def dot2_edge_cases():
    out = []
    for va, la, vb, lb, vc, lc, vd, ld in DOT2_EDGES:
        out.append((edge_operand(va, la), edge_operand(vb, lb), edge_operand(vc, lc), edge_operand(vd, ld)))
    return out


def sqr_edge_cases():
    out = []
    for W, va, la, vc, lc, vd, ld in SQR_EDGES:
        out.append((W, edge_operand(va, la), edge_operand(vc, lc), edge_operand(vd, ld)))
    return out


def check_result(t, want_value):
    """(2, 1): limbs below 2^28 (the top limb carries the excess), value < 2p, and the right residue"""
    assert all(x <= MASK for x in t[:13])
    assert value(t) < 2 * P
    assert value(t) % P == want_value % P


def test_edge_tables_sit_on_the_stated_bounds():
    for va, la, vb, lb, vc, lc, vd, ld in DOT2_EDGES[:-1]:
        assert la * lb + lc * ld == 17 and va * vb + vc * vd == 2048 and max(la, lb, lc, ld) <= 15
    for W, va, la, vc, lc, vd, ld in SQR_EDGES[:-1]:
        assert W * va * va + vc * vd == 2048 and 2 * W * la <= 15 and max(lc, ld) <= 15
        assert W * la * la + lc * ld == 17


def test_dot2_model_at_the_bounds():
    for a, b, c, d in dot2_edge_cases():
        check_result(model_dot2(a, b, c, d), (value(a) * value(b) + value(c) * value(d)) * RINV)


def test_dot2_sqr_model_at_the_bounds():
    for W, a, c, d in sqr_edge_cases():
        check_result(model_dot2_sqr(W, a, c, d), (W * value(a) ** 2 + value(c) * value(d)) * RINV)


def test_dot2_model_random():
    rng = random.Random(2)
    for _ in range(60):
        la, lb, lc, ld = rng.choice([(1, 1, 1, 1), (4, 4, 1, 1), (2, 3, 3, 3), (15, 1, 2, 1), (1, 2, 1, 15), (8, 2, 1, 1)])
        a, b = random_operand(rng, 32, la), random_operand(rng, 32, lb)
        c, d = random_operand(rng, 32, lc), random_operand(rng, 32, ld)
        check_result(model_dot2(a, b, c, d), (value(a) * value(b) + value(c) * value(d)) * RINV)
        W = rng.choice([1, 2])
        a = random_operand(rng, 20, 2)
        check_result(model_dot2_sqr(W, a, c, d), (W * value(a) ** 2 + value(c) * value(d)) * RINV)


def test_where_the_column_overflows():
    """How far beyond the stated bound the column holds: 17 is what counting 14 full products per column proves; a column has at
    most 12 (the top limbs are small for v <= 2048), which the edge operands spend up to 19, and at 20 they DO leave 64 bits -
    the model sees an overflow where there is one, and the edge cases above sit three steps from it."""
    for lam_c, overflows in ((3, False), (4, True)):
        a, b, c, d = edge_operand(32, 4), edge_operand(32, 4), edge_operand(32, lam_c), edge_operand(32, 1)
        if overflows:
            with pytest.raises(ColumnOverflow):
                model_dot2(a, b, c, d)
        else:
            model_dot2(a, b, c, d)
    model_dot2_sqr(2, edge_operand(4, 2), edge_operand(8, 5), edge_operand(8, 2))          # 8 + 10
    with pytest.raises(ColumnOverflow):
        model_dot2_sqr(2, edge_operand(4, 2), edge_operand(8, 6), edge_operand(8, 2))      # 8 + 12


def test_multiply_add_counts():
    """588 / 497 multiply-adds, the figures the formulas' instruction counts in csrc/h2v_curve28.hpp are built from"""
    dot2 = sum(2 * (k + 1) + k + 1 for k in range(14)) + sum(3 * (27 - k) for k in range(14, 27))
    sqr_terms = sum(len([i for i in range(max(0, k - 13), 14) if 2 * i < k and k - i < 14]) + (k % 2 == 0) for k in range(27))
    assert dot2 == 588 and sqr_terms == 105 and sqr_terms + 2 * 196 == 497
    assert 2 * 392 + 3 * 301 + 497 == 2184 and 6 * 392 + 3 * 301 + 588 == 3843 and 10 * 392 + 4 * 301 + 588 == 5712
