"""Deterministic mixed batches of bytes that need not be proofs, for the keyed-seed tests (H2V_RLC_SEED_KEYED, form 3), and a second,
straight-line restatement of the rule that shares no code with plutus_halo2_verifier_gen_amd/seed.py."""
import hashlib
import struct

LENS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256)      # with the 64-byte header every source alignment meets every block boundary
SHAPES3 = ((0, 0), (1, 1), (3, 0))                       # (n_pi, n_ci) of three plans; a fourth, (2, 1), is listed without a proof


def stream(label: str, n: int) -> bytes:
    """n reproducible bytes"""
    out, k = bytearray(), 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (label.encode(), k)).digest()
        k += 1
    return bytes(out[:n])


def tags(k: int, label: str = "tag"):
    return [stream("%s-%d" % (label, j), 32) for j in range(k)]


class Case:
    """a flat h2v_mixed_batch: plan_of, proofs, proof_off, instances, committed - and the same per proof"""

    def __init__(self, shapes, plan_of, lens, first_off=0, label="case"):
        self.shapes, self.plan_of, n = list(shapes), list(plan_of), len(plan_of)
        self.proof = [stream("%s-p%d" % (label, i), lens[i]) for i in range(n)]
        self.inst = [stream("%s-i%d" % (label, i), 32 * self.shapes[self.plan_of[i]][0]) for i in range(n)]
        self.ci = [stream("%s-c%d" % (label, i), 48) if self.shapes[self.plan_of[i]][1] else b"" for i in range(n)]
        self.first_off = first_off
        self.flatten()

    def flatten(self):
        self.off = [self.first_off]
        for p in self.proof:
            self.off.append(self.off[-1] + len(p))
        self.proofs = stream("pad", self.first_off) + b"".join(self.proof)
        self.instances = b"".join(self.inst)
        self.committed = b"".join(self.ci)
        return self


def case3(n: int, first_off: int = 0, label: str = "c3", lens=None) -> Case:
    """n proofs over three plans interleaved i % 3 (so a proof's committed index differs from its position and the instance offsets
    are no multiple of one row length); lengths cycle through LENS with a stride that visits all of them beside every plan"""
    return Case(SHAPES3 + ((2, 1),), [i % 3 for i in range(n)], lens if lens is not None else [LENS[(7 * i + i // 10) % len(LENS)] for i in range(n)],
                first_off, "%s-%d" % (label, n))


# ---- the rule once more, from DESIGN.md section 17.1 alone: a byte stream per digest, nothing shared with seed.py
def _b(data: bytes) -> bytes:
    return hashlib.blake2b(data, digest_size=32).digest()


def _tag(s: bytes) -> bytes:
    return s + bytes(16 - len(s))


def restated_seed(key_tags, plan_of, inst, ci, proof) -> bytes:
    n = len(proof)
    level = []
    for i in range(n):
        m = bytearray(_tag(b"h2v-seed-mleaf/1"))
        m += struct.pack("<I", len(inst[i])) + struct.pack("<I", len(ci[i])) + struct.pack("<I", len(proof[i])) + bytes(4)
        m += key_tags[plan_of[i]]
        m += inst[i] + ci[i] + proof[i]
        level.append(_b(bytes(m)))
    depth = 0
    while True:
        depth += 1
        up = []
        for j in range(0, len(level), 64):
            kids = level[j:j + 64]
            up.append(_b(_tag(b"h2v-seed-node/1") + struct.pack("<I", depth) + struct.pack("<I", len(kids)) + struct.pack("<Q", j // 64) + b"".join(kids)))
        level = up
        if len(level) == 1:
            break
    return _b(_tag(b"h2v-seed-root/1") + struct.pack("<I", 3) + bytes(4) + struct.pack("<Q", n) + bytes(32) + level[0])
