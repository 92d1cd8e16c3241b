"""Helper (not a test): two proofs whose pairing errors CANCEL under chosen batch coefficients - the input the batch-accept forms
(h2v_verify_batch_rlc, H2V_RLC_FOLD_PAIRS, H2V_MIXED_RLC, H2V_MIXED_FOLD_MSM) must be sound against.

synth forges proofs whose MSM scalars do not depend on the pi point: run_plan runs with a placeholder, then pi is solved for.
For an accepting proof with pi-term scalar x3 on an SRS with trapdoor s, pi + delta G is a proof that only the pairing rejects,
and the error of its equation e(L, s_g2) == e(R, G2) has discrete log delta (s - x3).  (Recursive keys too: the accumulator part of
the folded pair satisfies the equation by itself, so the fold challenge does not enter the error.)  For proofs A, B and weights
w_A, w_B
    delta_A =  d / (w_A (s - x3_A)),    delta_B = -d / (w_B (s - x3_B))        (mod r)
make  w_A err_A + w_B err_B = 0: the pair passes a check that gives A and B exactly those coefficients, and no other except
with negligible probability.  tests/test_batch_cancellation.py holds the construction to the oracle and the big-integer model."""
import hashlib
import struct
from collections import namedtuple

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, plan as PL

R = bls.R
CHUNK_TWEAK = 0x9e3779b9          # a laned workspace's chunk c xors CHUNK_TWEAK * (c + 1) into seed word 7 (include/h2v.h: RLC mode)

# one accepting proof with everything the construction needs: the plan, the SRS trapdoor s, the proof bytes, its public inputs as
# integers, its committed instance (48 bytes or None)
Rec = namedtuple("Rec", "pl s proof ints ci")


def rec_of(entry, batch, j):
    """proof j of `batch` (a synth.Batch of accepting proofs) of the key entry = {"vk", "td", "pl", ...}"""
    return Rec(entry["pl"], entry["td"].s, batch.proof(j), batch.instance_ints(j, entry["vk"].n_public_inputs), batch.ci(j))


def x3_of(plan, proof, instance_ints, ci):
    """the scalar of the pi term among plan.terms[:n_main_terms], as synth._forge_with_plan finds it (it does not depend on pi)"""
    scalars, _r, status = PL.run_plan(plan, proof, instance_ints, ci)
    assert status is None, status
    hits = [scalars[t] for t, (kind, idx) in enumerate(plan.terms[:plan.n_main_terms]) if kind == PL.TERM_PROOF_POINT and idx == plan.pi_point]
    assert len(hits) == 1
    return hits[0] % R


def shift_pi(plan, proof, delta):
    """the proof with pi + delta G"""
    o = plan.points[plan.pi_point]
    pi = bls.g1_decompress(proof[o:o + 48])
    buf = bytearray(proof)
    buf[o:o + 48] = bls.g1_compress(bls.g1_add(pi, bls.g1_mul(bls.G1_GEN, delta % R)))
    return bytes(buf)


def cancelling(rec_a, rec_b, w_a, w_b, d):
    """(A', B'): each is rejected by the pairing alone; w_a err(A') + w_b err(B') = 0.  d != 0 is the common error."""
    assert d % R and w_a % R and w_b % R
    out = []
    for rec, w, sign in ((rec_a, w_a, 1), (rec_b, w_b, -1)):
        gap = (rec.s - x3_of(rec.pl, rec.proof, rec.ints, rec.ci)) % R
        assert gap
        out.append(shift_pi(rec.pl, rec.proof, sign * d * pow(w * gap % R, -1, R) % R))
    return tuple(out)


def coeff(seed, counter, pos, chunk=None):
    """r of position `pos` of a check: low 128 bits of blake2b-256(seed' || LE32(pos)), 1 if 0.  seed' is the given seed with the
    library's process-wide count of seeded calls mixed into words 5 and 6 (include/h2v.h: H2V_RLC_SEED_GIVEN) and - chunk c of a
    call that a LANED workspace cuts into chunks, each its own check over positions 0 .. - CHUNK_TWEAK * (c + 1) into word 7."""
    w = list(struct.unpack("<8I", seed))
    w[5] ^= counter & 0xffffffff
    w[6] ^= counter >> 32
    if chunk is not None:
        w[7] ^= (CHUNK_TWEAK * (chunk + 1)) & 0xffffffff
    r = int.from_bytes(hashlib.blake2b(struct.pack("<8I", *w) + struct.pack("<I", pos), digest_size=32).digest()[:16], "little")
    return r or 1


_floor = 0        # the count only grows: a later search starts where the last one ended


def learn_counter(be, fx, ws, seed):
    """The library's process-wide count of seeded calls, as the call made HERE mixed it in (the next seeded call of any mode
    mixes in this value + 1): one one-proof fold_msm call on ws (a workspace over fx["plans"]), whose left sum is r_0 pi_0."""
    global _floor
    from tests.test_mixed_keys_gpu import Mix
    one = Mix(fx["keys"], fx["clean"], [("simple_mul", 0)])
    acc, st, fb = be.verify_mixed(fx["plans"], one.plan_of, one.proofs, one.off, one.instances, one.committed, ws=ws, mode="rlc", seed=seed,
                                  fold_msm=True)
    assert (list(acc), st, fb) == ([1], [0], False)
    l1, _r1 = be.probe_mixed_fold_sums(ws)
    pl = fx["keys"]["simple_mul"]["pl"]
    o = pl.points[pl.pi_point]
    p0 = bls.g1_decompress(one.proofs[o:o + 48])
    _floor = next(c for c in range(_floor, _floor + (1 << 16)) if bls.g1_mul(p0, coeff(seed, c, 0)) == l1)
    return _floor
