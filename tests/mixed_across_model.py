"""Helper (not a test): the big-integer model of a mixed call across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS).

A call is n proofs in the caller's order, proof i with the SRS label srs[i] of its key.  Classes are numbered in the order in which
the LISTED plans first carry an SRS (`listed`: the labels of the listed plans, in list order); a class without a proof is dropped.

    P(i)  = the proofs in lower classes + the rank of i within its class in the caller's order     (class-major position)

With H2V_MIXED_FOLD_MSM (Form B) the coefficient of proof i is drawn by its position in the call, r_i = coeff(i); without it
(Form A) by P(i), r_i = coeff(P(i)).  Both forms check

    prod_k e( L_k , s_g2_k ) == e( R , G2 ),      L_k = sum_{i in class k} r_i L_i,      R = sum_i r_i R_i

over the per-proof pairs (L_i, R_i) - h2v_prepare_batch's - of the proofs that were not rejected before the pairing."""
from plutus_halo2_verifier_gen_amd import bls12_381 as bls

R = bls.R


def classes(listed, srs):
    """the labels of the classes WITH proofs, in class order"""
    order = []
    for label in listed:
        if label not in order:
            order.append(label)
    assert all(s in order for s in srs)
    return [label for label in order if label in srs]


def positions(listed, srs):
    """[P(0), .., P(n - 1)]"""
    used = classes(listed, srs)
    out = []
    for i, s in enumerate(srs):
        lower = sum(1 for t in srs if used.index(t) < used.index(s))
        rank = sum(1 for t in srs[:i] if t == s)
        out.append(lower + rank)
    return out


def _sum(terms):
    acc = None
    for r, p in terms:
        if p is not None and r % R:
            acc = bls.g1_add(acc, bls.g1_mul(p, r % R))
    return acc


def sums(listed, srs, pairs, coeff, form, takes_part=None):
    """(R, [L_k per class with proofs]) of Form "A" or "B": pairs[i] = (L_i, R_i) affine points or None, coeff(position) the
    coefficient rule (tests/cancel.py: coeff with the call's seed and counter), takes_part[i] false for a proof rejected before
    the pairing (coefficient 0)"""
    assert form in ("A", "B")
    n = len(srs)
    at = positions(listed, srs) if form == "A" else list(range(n))
    r = [coeff(at[i]) if takes_part is None or takes_part[i] else 0 for i in range(n)]
    used = classes(listed, srs)
    return (_sum((r[i], pairs[i][1]) for i in range(n)),
            [_sum((r[i], pairs[i][0]) for i in range(n) if srs[i] == label) for label in used])


def check(secrets, r_sum, l_sums):
    """the multi-pairing itself: prod_k e(L_k, [s_k] G2) == e(R, G2); an infinite sum costs no Miller loop.  secrets: the SRS
    secret of every class with proofs, in class order"""
    f = list(bls.F12_ONE)
    for s, l in zip(secrets, l_sums):
        if l is not None:
            f = bls.f12_mul(f, bls.miller_loop(l, bls.g2_mul(bls.G2_GEN, s % R)))
    if r_sum is not None:
        f = bls.f12_mul(f, bls.miller_loop(bls.g1_neg(r_sum), bls.G2_GEN))
    return bls.final_exponentiation(f) == bls.F12_ONE
