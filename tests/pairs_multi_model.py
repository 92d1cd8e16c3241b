"""Helper (not a test): the big-integer model of the batch check across several SRS (h2v_check_pairs_multi, include/h2v.h).

A call is a list of ranges; range k holds the SRS secret's G2 point s_g2_k and pairs (L, R) of affine G1 points (None = infinity).
With a coefficient r_i per position i of the CALL the check is

    FE( prod_k ML( sum_{i in k} r_i L_i ; s_g2_k ) * ML( -sum_i r_i R_i ; G2 ) ) == 1,

C + 1 Miller loops and one final exponentiation (bls.miller_loop gives one for an infinite argument: a range whose left sum is
infinity costs no loop).  The coefficients are tests/cancel.py's rule - low 128 bits of blake2b-256(seed' || LE32(i)), i counted
through the whole call, never 0."""
from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import cancel

R = bls.R


def pair_on(s, a, err=0):
    """([a]G1, [a s + err]G1): accepts under the SRS with secret s iff err == 0 (mod r), and under no other secret"""
    return bls.g1_mul(bls.G1_GEN, a % R), bls.g1_mul(bls.G1_GEN, (a * s + err) % R)


def s_g2(s):
    return bls.g2_mul(bls.G2_GEN, s % R)


def compress(pair):
    return bls.g1_compress(pair[0]) + bls.g1_compress(pair[1])


def coefficients(seed, counter, n):
    """r_0 .. r_{n-1} of a call whose seeded-call count is `counter` (cancel.coeff: one check, positions through the call)"""
    return [cancel.coeff(seed, counter, i) for i in range(n)]


def g1_sum(terms):
    """sum of r * P over (r, P); None = infinity"""
    acc = None
    for r, p in terms:
        if p is not None and r % R:
            acc = bls.g1_add(acc, bls.g1_mul(p, r % R))
    return acc


def multi_check(ranges, coeffs):
    """ranges: [(s_g2 point, [(L, R), ...]), ...]; coeffs: one per pair, by position in the call.  Returns (verdict, loops) -
    loops: the Miller loops with two finite arguments that the product holds."""
    pos, f, loops, rights = 0, list(bls.F12_ONE), 0, []
    for q, pairs in ranges:
        rs = coeffs[pos:pos + len(pairs)]
        pos += len(pairs)
        left = g1_sum((r, lr[0]) for r, lr in zip(rs, pairs))
        rights += [(r, lr[1]) for r, lr in zip(rs, pairs)]
        if left is not None:
            f = bls.f12_mul(f, bls.miller_loop(left, q))
            loops += 1
    assert pos == len(coeffs)
    right = g1_sum(rights)
    if right is not None:
        f = bls.f12_mul(f, bls.miller_loop(bls.g1_neg(right), bls.G2_GEN))
        loops += 1
    return bls.final_exponentiation(f) == bls.F12_ONE, loops


def cancelling_errors(r_a, r_b, d):
    """(err_a, err_b) with r_a err_a + r_b err_b = 0 (mod r), neither 0: the two pairs fail alone and pass together under exactly
    these two coefficients (tests/cancel.py's construction, on pairs)"""
    assert d % R and r_a % R and r_b % R
    return d * pow(r_a, -1, R) % R, -d * pow(r_b, -1, R) % R
