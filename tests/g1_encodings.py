"""One table of 48-byte G1 encodings for the decompression kernels, with what the Python model (bls12_381.g1_decompress,
g1_in_subgroup) says of each: whether the encoding is well-formed and on the curve, whether it is a point of G1, and the
decoded (x, y) whenever it is on the curve - also outside G1, where the queue launch's root wave stores the point too.
tests/test_g1_encodings.py holds the table to the oracle and asserts what it must cover; tests/test_decompress_queue_gpu.py and
test_g1_decompress (tests/test_gpu_parity.py) run it through the kernels.

Two encodings one might look for do not exist:
  * c = x^3 + 4 = 0 (y = 0, a 2-torsion point): -4 is not a cube mod p;
  * a curve point with y = (p +- 1) / 2, the two values next to the threshold of the sort flag: y^2 = 1/4 needs
    x^3 = -15/4, which is not a cube mod p either.
test_g1_encodings.py asserts both."""
import functools
import random
from dataclasses import dataclass
from typing import Optional, Tuple

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

P, R = bls.P, bls.R
COFACTOR = 0x396c8c005555e1568c00aaab0000aaab            # #E(Fp) = COFACTOR * r
# the kinds, in the order the GPU tests deal them out
KINDS = ("g1", "infinity", "bad_infinity", "no_compression_bit", "non_canonical", "off_curve", "outside_g1")
# kinds whose encoding fails before any arithmetic: the subgroup wave's verdict is 0 as well
FAILED_ENCODING = ("bad_infinity", "no_compression_bit", "non_canonical")


@dataclass(frozen=True)
class Case:
    kind: str
    name: str
    enc: bytes
    on_curve: bool                          # the encoding is well-formed AND (infinity or x is on the curve)
    in_g1: bool                             # ... and the point is in G1: the verdict
    point: Optional[Tuple[int, int]]        # (x, y) when on_curve and finite, else None


def model(enc: bytes):
    """(on_curve, in_g1, point) of an encoding from the Python model"""
    try:
        pt = bls.g1_decompress(enc, False)
    except ValueError:
        return False, False, None
    return True, pt is None or bls.g1_in_subgroup(pt), pt


def encode(x: int, sort: bool = False, flags: int = 0x80) -> bytes:
    """x (below 2^381, canonical or not) under the flag bits"""
    raw = bytearray(x.to_bytes(48, "big"))
    assert raw[0] < 0x20
    raw[0] |= flags | (0x20 if sort else 0)
    return bytes(raw)


def sort_flag(enc: bytes) -> bool:
    return bool(enc[0] & 0x20)


def stray_infinity(word: int) -> bytes:
    """the infinity encoding with exactly one more bit set, in the 32-bit word `word` of the 48 bytes (word 0 = bytes 0..3: there
    the bit lies in the low five bits of byte 0, next to the flags)"""
    raw = bytearray(bls.g1_compress(None))
    bit = 28 if word == 0 else (7 * word + 3) % 32        # (bit 31 = the top bit of the word's first byte)
    raw[4 * word + (31 - bit) // 8] |= 1 << (bit % 8)
    return bytes(raw)


def small_order_point(q: int):
    """a point of prime order q, q^2 || COFACTOR.  The q-part of E(Fp) is Z_q x Z_q (11 and 10177 alike), so [#E / q] sends
    every point to infinity; [#E / q^2] leaves the q-torsion component."""
    assert COFACTOR % (q * q) == 0 and COFACTOR % (q * q * q) != 0
    x = 1
    while x < 200:
        x += 1
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is None:
            continue
        t = bls.g1_mul((x, y), COFACTOR * R // (q * q))
        if t is not None:
            assert bls.g1_mul(t, q) is None
            return t
    raise AssertionError("no point of order %d" % q)


@functools.lru_cache(maxsize=None)
def beta() -> int:
    """the cube root of unity with (beta x, y) = [lambda](x, y) on G1, taken from the generator rather than from a constant"""
    lx, ly = bls.g1_mul(bls.G1_GEN, bls.GLV_LAMBDA)
    b = lx * bls.fp_inv(bls.G1_X) % P
    assert ly == bls.G1_Y and b != 1 and pow(b, 3, P) == 1
    return b


def phi(pt):
    return (beta() * pt[0] % P, pt[1])


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(0x6731)
    out = []

    def add(kind, name, enc):
        out.append(Case(kind, name, enc, *model(enc)))

    # ---- valid points of G1
    add("g1", "generator", bls.g1_compress(bls.G1_GEN))
    add("g1", "-generator", bls.g1_compress(bls.g1_neg(bls.G1_GEN)))
    rand = [bls.g1_mul(bls.G1_GEN, rng.randrange(1, R)) for _ in range(20)]
    for k, pt in enumerate(rand):
        add("g1", "random %d" % k, bls.g1_compress(pt))
    for k, pt in enumerate(rand[:4]):                     # the other root under the same x: the valid point -P
        enc = bls.g1_compress(pt)
        add("g1", "random %d, sort flag flipped" % k, bytes([enc[0] ^ 0x20]) + enc[1:])
    # points whose x + p still fits 381 bits (about 23 % of G1): they come back below as non-canonical encodings
    low, pt = [], bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
    while len(low) < 4 or len({sort_flag(bls.g1_compress(q)) for q in low}) < 2:
        pt = bls.g1_add(pt, bls.G1_GEN)
        if pt[0] < (1 << 381) - P:
            low.append(pt)
    for k, q in enumerate(low):
        add("g1", "low x %d" % k, bls.g1_compress(q))
    # ---- infinity
    add("infinity", "infinity", bls.g1_compress(None))
    add("bad_infinity", "infinity with the sort flag", bytes([0xE0]) + bytes(47))
    for w in range(12):
        add("bad_infinity", "infinity with a stray bit in word %d" % w, stray_infinity(w))
    # ---- compression bit clear
    for b0 in (0x00, 0x40, 0x20):
        add("no_compression_bit", "%02x 00 .." % b0, bytes([b0]) + bytes(47))
    gen = bls.g1_compress(bls.G1_GEN)
    add("no_compression_bit", "generator without bit 7", bytes([gen[0] & 0x7F]) + gen[1:])
    # ---- x >= p
    for k, q in enumerate(low):
        add("non_canonical", "low x %d + p" % k, encode(q[0] + P, sort_flag(bls.g1_compress(q))))
    add("non_canonical", "x = p", encode(P))
    add("non_canonical", "x = p + 1", encode(P + 1, True))
    add("non_canonical", "x = 2^381 - 1", encode((1 << 381) - 1))
    # ---- off the curve
    add("off_curve", "x = p - 1", encode(P - 1))          # canonical; c = 3 is a non-residue
    k = 0
    while k < 10:
        x = rng.randrange(P)
        if bls.fp_sqrt((x * x * x + 4) % P) is None:
            add("off_curve", "random non-residue %d" % k, encode(x, rng.random() < 0.5))
            k += 1
    # ---- on the curve, outside G1
    add("outside_g1", "(0, 2), order 3", bls.g1_compress((0, 2)))
    add("outside_g1", "(0, -2), order 3", bls.g1_compress((0, P - 2)))
    for q in (11, 10177):
        add("outside_g1", "order %d" % q, bls.g1_compress(small_order_point(q)))
    k = 0
    while k < 10:
        x = rng.randrange(P)
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is not None:
            add("outside_g1", "random curve point %d" % k, bls.g1_compress((x, y if rng.random() < 0.5 else P - y)))
            k += 1
    add("outside_g1", "T + Q, T of order 3, Q in G1", bls.g1_compress(bls.g1_add((0, 2), rand[5])))
    return tuple(out)


def by_kind():
    return {kind: [c for c in cases() if c.kind == kind] for kind in KINDS}
