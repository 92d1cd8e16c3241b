"""The six kinds of pairs the pairing engines are held to, the big-integer replay of each (tools/gen_coop_program.py: simulate),
and the layouts that carry every kind into every position of a wave.  Shared by tests/test_six_fetch_order_gpu.py,
tests/test_pairing_engines.py (the layouts' coverage, on the CPU) and tests/test_pairing_engines_gpu.py (the six engines).

A pair (p1, p2) is accepted under a key with s_g2 = [s]G2 exactly when e(p1, [s]G2) == e(p2, G2).  The kinds: accepting (a, [s]a);
rejecting (b, [s]b + G1) and (c, [s + 2]c); first argument at infinity; second at infinity; both.  A loop whose G1 argument is
infinity is skipped (the `keep` path: its line steps run and leave f as staged), so its Miller value is the other loop's alone.
For s = 1 the accepting pair is (a, a) and both line tables are the same; for s = r - 1 the second rejecting pair is (c, c)."""
import functools
import os
import random
import sys
from collections import namedtuple

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

ACCEPT, REJECT_A, REJECT_B, INF_1, INF_2, INF_BOTH = range(6)
N_KINDS = 6
ROTATIONS = tuple(range(N_KINDS))
ONE = [1] + [0] * 11

# c1, c2: the compressed arguments; verdict; miller, final: the value after the Miller loop and after the final exponentiation as 12
# integers (re, im of coefficient 0..5); p1, p2: the arguments as integer points (None: infinity)
Kind = namedtuple("Kind", "c1 c2 verdict miller final p1 p2")

# The engines: the probe's impl, the H2V_OPT_PAIRING_ENGINE value the probe must be given with it (0: none), lanes per proof (what the
# launcher reports) and proofs per wave G.  "coop32" is reachable only as impl 1 with the option: without it the launcher picks
# the wide engine for small batches.
Engine = namedtuple("Engine", "name impl option lanes per_wave")
ENGINES = (Engine("one_lane", 0, 0, 1, 64), Engine("coop32", 1, 32, 32, 2), Engine("narrow", 2, 0, 16, 4), Engine("wide", 3, 0, 64, 1),
           Engine("six", 5, 0, 6, 10), Engine("twelve", 6, 0, 12, 5))


def batch_sizes(per_wave: int):
    """one pair; one full wave; a full wave and a lone trailing group; two full waves and a lone trailing group"""
    out = []
    for n in (1, per_wave, per_wave + 1, 2 * per_wave + 1):
        if n not in out:
            out.append(n)
    return tuple(out)


def order(n: int, rot: int):
    """the kinds of a batch of n pairs under rotation rot"""
    return [(j + rot) % N_KINDS for j in range(n)]


def positions_seen(per_wave: int, sizes, rotations):
    """{(kind, where)} over all batches of the given sizes and rotations: where is "first" (group 0 of a wave), "last" (group
    per_wave - 1, the one the idle lanes of the packed engines shadow) or "lone" (the only live group of a trailing wave)"""
    seen = set()
    for n in sizes:
        for rot in rotations:
            for j, k in enumerate(order(n, rot)):
                if j % per_wave == 0:
                    seen.add((k, "first"))
                if j % per_wave == per_wave - 1:
                    seen.add((k, "last"))
                if j % per_wave == 0 and j == n - 1:
                    seen.add((k, "lone"))
    return seen


ALL_POSITIONS = {(k, where) for k in range(N_KINDS) for where in ("first", "last", "lone")}


@functools.lru_cache(maxsize=None)
def programs():
    """(the engines' program, its prefix up to the Miller value) - dump 0 is conj(F) after the Miller loop"""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import gen_coop_program as gp
    prog = gp.build_program()
    first_dump = [i for i, ins in enumerate(prog) if ins[0] == gp.OP_DUMP][0]
    assert prog[first_dump][1:3] == (0, gp.U) and prog[first_dump - 1][:3] == (gp.OP_CONJ, gp.U, gp.F)
    return gp, prog, prog[:first_dump - 1] + [(gp.OP_END, 0, 0, 0)]


def replay(p1, p2, q1):
    """(verdict, Miller value, final value) of the pair under s_g2 = q1, from the big-integer replay of the program"""
    gp, prog, miller_prog = programs()
    flat = lambda f: [x for pair in f for x in pair]
    final = gp.simulate(prog, p1, q1, p2, bls.G2_GEN)
    miller = bls.f12_conj(gp.simulate(miller_prog, p1, q1, p2, bls.G2_GEN))
    return (1 if final == bls.F12_ONE else 0), flat(miller), flat(final)


def build_kinds(vk, td, seed: int = 68):
    """{kind: Kind} for the key (vk, td).  Asserts what the kinds are meant to be: the verdicts, and that every rejecting kind
    carries 24 values outside {0, 1} - a non-trivial value in every lane through the whole program."""
    rng = random.Random(seed)
    q1 = bls.g2_mul(bls.G2_GEN, td.s)
    assert bls.g2_compress(q1) == bytes.fromhex(vk.s_g2)
    a, b, c = (bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R)) for _ in range(3))
    pts = {ACCEPT: (a, bls.g1_mul(a, td.s)),
           REJECT_A: (b, bls.g1_add(bls.g1_mul(b, td.s), bls.G1_GEN)),
           REJECT_B: (c, bls.g1_mul(c, (td.s + 2) % bls.R)),
           INF_1: (None, bls.g1_mul(bls.G1_GEN, 5)),
           INF_2: (bls.g1_mul(bls.G1_GEN, 7), None),
           INF_BOTH: (None, None)}
    out = {}
    for kind, (p1, p2) in pts.items():
        verdict, miller, final = replay(p1, p2, q1)
        out[kind] = Kind(bls.g1_compress(p1), bls.g1_compress(p2), verdict, miller, final, p1, p2)
    assert [out[k].verdict for k in range(N_KINDS)] == [1, 0, 0, 0, 0, 1]
    for k in (REJECT_A, REJECT_B):
        assert all(x not in (0, 1) for x in out[k].miller) and all(x not in (0, 1) for x in out[k].final)
    assert out[REJECT_A].final != out[REJECT_B].final
    return out


def off_curve_encoding() -> bytes:
    """a well-formed compressed encoding whose x is on no curve point: decompression fails"""
    x = 1
    while bls.fp_sqrt((x * x * x + 4) % bls.P) is not None:
        x += 1
    raw = bytearray(x.to_bytes(48, "big"))
    raw[0] |= 0x80
    return bytes(raw)
