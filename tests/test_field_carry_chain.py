"""The four product-scanning multipliers of csrc/h2v_field.hpp (fp_mont28, fp_montsqr28, fp_mont28_dot2, fp_mont28_dot2_sqr<W>)
keep each column as ONE chain of multiply-adds whose first addend is the carry of the column before (fp28_mac).  The carry
therefore sits in the 64-bit accumulator from the column's first step, not added after the products: a column that only just
fitted with the carry added last would now wrap earlier.  The CPU part replays every column with the carry FIRST and asserts
the 64-bit bound at every step, on operands whose every limb is at the bound csrc/h2v_fp28.hpp states; the GPU part runs the same
operands (and random ones) through h2v_probe_f28_dot2 - ops 3 and 4 reach the plain product and the plain squaring - and compares
limb for limb with the Python model of tests/test_field_dot2.py."""
import random

import pytest

from tests.test_field_dot2 import (MASK, MOD28, N0_28, P, RINV, dot2_edge_cases, edge_operand, model_dot2, model_dot2_sqr,
                                   random_operand, sqr_edge_cases, value)

ZERO = [0] * 14
# f28_mul: lam_a lam_b <= 17 and v_a v_b <= 2048 (limbs stay 32-bit: lam <= 15), both as far as integers allow
MUL_EDGES = [(2048, 15, 1, 1), (1, 1, 2048, 15), (45, 4, 45, 4), (32, 4, 64, 4), (128, 8, 16, 2), (512, 5, 4, 3), (4, 3, 512, 5)]
# f28_sqr: lam_a^2 <= 17 and v_a^2 <= 2048
SQR_PLAIN_EDGES = [(45, 4), (45, 1), (1, 4), (32, 3)]


def mul_edge_cases():
    return [(edge_operand(va, la), edge_operand(vb, lb)) for va, la, vb, lb in MUL_EDGES]


def sqr_plain_edge_cases():
    return [edge_operand(v, lam) for v, lam in SQR_PLAIN_EDGES]


def chain_columns(terms_of_column):
    """The column loop as the device runs it: acc starts as the carry, every term is added to it in source order and the sum
    must stay below 2^64 after EVERY step.  terms_of_column(k, m) lists column k's products; returns (result limbs, the largest
    value the accumulator reached)."""
    m, t, acc, peak = [0] * 14, [0] * 14, 0, 0
    for k in range(27):
        carry = acc
        for x, y in terms_of_column(k, m):
            assert x < 1 << 32 and y < 1 << 32
            acc += x * y
            assert acc < 1 << 64, "column %d wraps with the carry (%d) inside the chain" % (k, carry)
        if k < 14:
            m[k] = ((acc & 0xffffffff) * N0_28) & MASK
            acc += m[k] * MOD28[0]
            assert acc < 1 << 64 and acc & MASK == 0
        else:
            t[k - 14] = acc & MASK
        peak = max(peak, acc)
        acc >>= 28
    assert acc < 1 << 32
    t[13] = acc
    return t, peak


def _rng(k):
    return range(0 if k < 14 else k - 13, min(k, 13) + 1)


def _reduction(k, m):
    return [(m[i], MOD28[k - i]) for i in _rng(k) if i < k or k >= 14]


def chain_dot2(a, b, c, d):
    return chain_columns(lambda k, m: [(a[i], b[k - i]) for i in _rng(k)] + [(c[i], d[k - i]) for i in _rng(k)] + _reduction(k, m))


def chain_dot2_sqr(W, a, c, d):
    def terms(k, m):
        sq = [(a[i] * 2 * W, a[k - i]) for i in _rng(k) if 2 * i < k] + ([(a[k // 2] * W, a[k // 2])] if k % 2 == 0 else [])
        return sq + [(c[i], d[k - i]) for i in _rng(k)] + _reduction(k, m)
    return chain_columns(terms)


def test_plain_edge_tables_sit_on_the_stated_bounds():
    for va, la, vb, lb in MUL_EDGES:
        assert la * lb <= 17 and va * vb <= 2048 and max(la, lb) <= 15
        assert (la + 1) * lb > 17 or (lb + 1) * la > 17 or max(la, lb) == 15      # no limb class left to give
    assert any(va * vb == 2048 for va, _, vb, _ in MUL_EDGES) and any(la * lb == 16 for _, la, _, lb in MUL_EDGES)
    for v, lam in SQR_PLAIN_EDGES:
        assert lam * lam <= 17 and v * v <= 2048
    assert (45, 4) in SQR_PLAIN_EDGES and 46 * 46 > 2048 and 5 * 5 > 17


def test_columns_hold_64_bits_with_the_carry_first_at_the_bounds():
    """every limb at its bound: the carry rides inside the chain and no step of any column leaves 64 bits"""
    for a, b in mul_edge_cases():
        t, peak = chain_dot2(a, b, ZERO, ZERO)
        assert peak < 1 << 64 and t == model_dot2(a, b, ZERO, ZERO)
        assert value(t) < 2 * P and value(t) % P == value(a) * value(b) * RINV % P
    for a in sqr_plain_edge_cases():
        t, peak = chain_dot2_sqr(1, a, ZERO, ZERO)
        assert peak < 1 << 64 and t == model_dot2_sqr(1, a, ZERO, ZERO) == model_dot2(a, a, ZERO, ZERO)
        assert value(t) < 2 * P and value(t) % P == value(a) ** 2 * RINV % P
    for a, b, c, d in dot2_edge_cases():
        t, peak = chain_dot2(a, b, c, d)
        assert peak < 1 << 64 and t == model_dot2(a, b, c, d)
    for W, a, c, d in sqr_edge_cases():
        t, peak = chain_dot2_sqr(W, a, c, d)
        assert peak < 1 << 64 and t == model_dot2_sqr(W, a, c, d)


def test_carry_is_small_beside_the_column():
    """the header's figure: a carry-in is below 2^36 + 2^8 (a column below 2^64 shifted by 28), so the 17-unit bound
    14 x 17 x 2^56 + 14 x 2^56 + carry < 2^64 holds wherever in the chain the carry is added"""
    assert 14 * 17 * (1 << 56) + 14 * (1 << 56) + (1 << 36) < 1 << 64
    worst = 0
    for a, b, c, d in dot2_edge_cases():
        worst = max(worst, chain_dot2(a, b, c, d)[1])
    assert worst >> 28 < 1 << 36


def test_random_operands_carry_first():
    rng = random.Random(7)
    for _ in range(40):
        la, lb = rng.choice([(1, 1), (4, 4), (15, 1), (1, 15), (8, 2), (5, 3)])
        a, b = random_operand(rng, 45, la), random_operand(rng, 45, lb)
        assert chain_dot2(a, b, ZERO, ZERO)[0] == model_dot2(a, b, ZERO, ZERO)
        s = random_operand(rng, 45, rng.choice([1, 2, 4]))
        assert chain_dot2_sqr(1, s, ZERO, ZERO)[0] == model_dot2_sqr(1, s, ZERO, ZERO)


# ------------------------------------------------------------------------------------------------ device
@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


@pytest.mark.gpu
@pytest.mark.parametrize("inline", [False, True])
def test_plain_product_matches_the_model_limb_for_limb(be, inline):
    rng = random.Random(51)
    cases = mul_edge_cases()
    for _ in range(200):
        la, lb = rng.choice([(1, 1), (4, 4), (15, 1), (1, 15), (8, 2), (5, 3), (2, 8)])
        cases.append((random_operand(rng, 45, la), random_operand(rng, 45, lb)))
    got = be.probe_f28_dot2(be.DOT2_PLAIN_MUL | (be.DOT2_INLINE if inline else 0), [c[0] for c in cases], [c[1] for c in cases])
    for (a, b), t in zip(cases, got):
        assert t == model_dot2(a, b, ZERO, ZERO)
        assert value(t) < 2 * P and value(t) % P == value(a) * value(b) * RINV % P


@pytest.mark.gpu
@pytest.mark.parametrize("inline", [False, True])
def test_plain_squaring_matches_the_model_limb_for_limb(be, inline):
    rng = random.Random(53)
    cases = sqr_plain_edge_cases() + [random_operand(rng, 45, rng.choice([1, 2, 3, 4])) for _ in range(200)]
    got = be.probe_f28_dot2(be.DOT2_PLAIN_SQR | (be.DOT2_INLINE if inline else 0), cases)
    for a, t in zip(cases, got):
        assert t == model_dot2_sqr(1, a, ZERO, ZERO)
        assert value(t) < 2 * P and value(t) % P == value(a) ** 2 * RINV % P


@pytest.mark.gpu
@pytest.mark.parametrize("inline", [False, True])
def test_merged_products_at_the_bounds(be, inline):
    """the two merged multipliers on the records whose every limb is at its bound (the random ones: tests/test_field_dot2_gpu.py)"""
    flag = be.DOT2_INLINE if inline else 0
    cases = dot2_edge_cases()
    got = be.probe_f28_dot2(be.DOT2_MUL | flag, *[[c[k] for c in cases] for k in range(4)])
    assert got == [model_dot2(*c) for c in cases]
    for W, op in ((1, be.DOT2_SQR), (2, be.DOT2_SQR2)):
        cases = [(a, c, d) for w, a, c, d in sqr_edge_cases() if w == W]
        got = be.probe_f28_dot2(op | flag, [c[0] for c in cases], None, [c[1] for c in cases], [c[2] for c in cases])
        assert got == [model_dot2_sqr(W, *c) for c in cases]
