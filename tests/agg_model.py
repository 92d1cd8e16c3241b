"""Helper (not a test): the big-integer model of an aggregate call's pair (include/h2v.h: h2v_aggregate_batch / h2v_aggregate_mixed).

    pair = compress(L) || compress(R),   L = sum r_i L_i,   R = sum r_i R_i   over the included proofs

with (L_i, R_i) the pair h2v_prepare_batch returns for proof i (the oracle's el / er) and r_i the coefficient rule of the header:
the low 128 bits of blake2b-256(seed' || LE32(pos)), 1 if that is 0.  chunk = 0 (an ordinary workspace, and the mixed form):
seed' = seed_used, pos = the index in the call.  chunk > 0 (a laned workspace): proof i lies in chunk c = i // chunk, which hashes
seed_used with 0x9e3779b9 * (c + 1) xored into its last 32-bit word, at pos = i % chunk (tests/cancel.py::coeff states the same
rule from the given seed and the library's call count; seed_used already has that count mixed in)."""
import hashlib
import struct

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

CHUNK_TWEAK = 0x9e3779b9


def coeff(seed_used, i, chunk=0):
    """r_i of proof i of a call whose h2v_aggregate_info says (seed_used, chunk)"""
    w = list(struct.unpack("<8I", bytes(seed_used)))
    pos = i
    if chunk:
        w[7] ^= (CHUNK_TWEAK * (i // chunk + 1)) & 0xffffffff
        pos = i % chunk
    r = int.from_bytes(hashlib.blake2b(struct.pack("<8I", *w) + struct.pack("<I", pos), digest_size=32).digest()[:16], "little")
    return r or 1


def model_sums(pairs_i, included, seed_used, chunk=0):
    """(L, R) as affine integer points (None = infinity); pairs_i[i] = 96 bytes compress(L_i) || compress(R_i) - read only
    where included[i]"""
    L = R = None
    for i, (pr, inc) in enumerate(zip(pairs_i, included)):
        if not inc:
            continue
        r = coeff(seed_used, i, chunk)
        L = bls.g1_add(L, bls.g1_mul(bls.g1_decompress(pr[:48]), r))
        R = bls.g1_add(R, bls.g1_mul(bls.g1_decompress(pr[48:96]), r))
    return L, R


def model_pair(pairs_i, included, seed_used, chunk=0):
    """the 96 bytes an aggregate call must return"""
    L, R = model_sums(pairs_i, included, seed_used, chunk)
    return bls.g1_compress(L) + bls.g1_compress(R)


def holds(pair, s):
    """R == [s] L: what e(L, s_g2) == e(R, G2) says to whoever knows the SRS trapdoor s"""
    L, R = bls.g1_decompress(pair[:48]), bls.g1_decompress(pair[48:96])
    return bls.g1_mul(L, s % bls.R) == R if L is not None else R is None
