"""The cancelling pair of tests/cancel.py, held to the CPU oracle and to the big-integer model (bls12_381.py): each altered proof
alone is rejected by the pairing and by nothing else, the sums of the oracle's (el, er) under the weights the pair was built for
satisfy the pairing equation, and under the same two weights exchanged they do not.  Same key (two distinct proofs), two keys on
one SRS, and a key with the recursive one (folded pair).  tests/test_batch_cancellation_gpu.py feeds such pairs to every
batch-accept form; this file is what makes them trustworthy.  (A Python pairing check costs about a second: nine in all.)"""
import json

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, plan as PL, synth, vk as V
from tests import cancel
from tests.test_mixed_keys import COMMON_S

PAIRINGS = [("simple_mul", 0, "simple_mul", 1), ("simple_mul", 0, "lookup_table", 0), ("lookup_table", 1, "ivc", 0)]
WEIGHTS = [(1, 1), (0x8f3c1d5e7a9b2c4d6e8f0a1b3c5d7e9f, 0x1b2a39485766758493a2b1c0dfeeddcc)]      # 128-bit, as the coefficients are
D = 987654321987654321


@pytest.fixture(scope="module")
def keys(orc):
    out = {}
    for k, name in enumerate(("simple_mul", "lookup_table", "ivc")):
        vk, td = V.on_srs(*V.BUILDERS[name](), COMMON_S)
        pl = PL.compile_plan(vk)
        e = {"vk": vk, "td": td, "pl": pl,
             "ov": orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))}
        e["clean"] = synth.forge_batch(vk, td, 2, seed=31 + k, plan=pl, workers=1)
        out[name] = e
    return out


def _traced(orc, e, rec, proof):
    ok, tr = e["ov"].verify(proof, rec.ints, rec.ci, trace=True)
    return ok, orc.STATUS[tr.status], tr


@pytest.mark.parametrize("na,ja,nb,jb", PAIRINGS)
def test_the_pair_cancels_under_its_weights_and_no_others(orc, keys, na, ja, nb, jb):
    ea, eb = keys[na], keys[nb]
    ra, rb = cancel.rec_of(ea, ea["clean"], ja), cancel.rec_of(eb, eb["clean"], jb)
    assert ra.proof != rb.proof and ra.s == rb.s == COMMON_S
    sg2 = bls.g2_mul(bls.G2_GEN, COMMON_S)
    for rec, e in ((ra, ea), (rb, eb)):
        ok, _cls, tr = _traced(orc, e, rec, rec.proof)
        assert ok
        assert tr.scalar("x3") == cancel.x3_of(rec.pl, rec.proof, rec.ints, rec.ci)       # the oracle's pi-term scalar is run_plan's
    for wa, wb in WEIGHTS:
        pa, pb = cancel.cancelling(ra, rb, wa, wb, D)
        assert pa != ra.proof and pb != rb.proof
        oka, clsa, ta = _traced(orc, ea, ra, pa)
        okb, clsb, tb = _traced(orc, eb, rb, pb)
        assert (oka, clsa, okb, clsb) == (False, "pairing", False, "pairing")
        assert cancel.x3_of(ra.pl, pa, ra.ints, ra.ci) == cancel.x3_of(ra.pl, ra.proof, ra.ints, ra.ci)      # pi does not enter x3

        def sums(u, v):
            return (bls.g1_add(bls.g1_mul(ta.point("el"), u), bls.g1_mul(tb.point("el"), v)),
                    bls.g1_add(bls.g1_mul(ta.point("er"), u), bls.g1_mul(tb.point("er"), v)))

        l, r = sums(wa, wb)
        assert l is not None and r is not None
        assert bls.pairing_check_eq(l, sg2, r, bls.G2_GEN)
        if wa != wb:
            l, r = sums(wb, wa)
            assert not bls.pairing_check_eq(l, sg2, r, bls.G2_GEN)
            assert orc.pairing_check(l, bytes.fromhex(ea["vk"].s_g2), r, orc.g2_generator_compressed()) == 0      # (the C oracle agrees)


def test_coeff_is_the_documented_hash():
    """blake2b-256(seed' || LE32(pos)), low 128 bits; the call counter in words 5 and 6, a laned chunk's tweak in word 7"""
    import hashlib
    import struct
    seed = bytes(range(100, 132))
    h = lambda s, pos: int.from_bytes(hashlib.blake2b(s + struct.pack("<I", pos), digest_size=32).digest()[:16], "little")
    assert cancel.coeff(seed, 0, 7) == h(seed, 7)
    w = list(struct.unpack("<8I", seed))
    w[5] ^= 0x01020304
    w[6] ^= 0x5
    assert cancel.coeff(seed, 0x501020304, 69) == h(struct.pack("<8I", *w), 69)
    w[7] ^= (cancel.CHUNK_TWEAK * 3) & 0xffffffff
    assert cancel.coeff(seed, 0x501020304, 69, chunk=2) == h(struct.pack("<8I", *w), 69)
    assert len({cancel.coeff(seed, 3, p, chunk=c) for p in range(140) for c in (None, 0, 1)}) == 420
