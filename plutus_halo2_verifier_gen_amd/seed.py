"""The derived batch seed (H2V_RLC_SEED_TRANSCRIPT, include/h2v.h), restated with hashlib alone: what a
second party runs to re-derive the seed - and with it the coefficients and the pair - of a batch-accept call from its inputs.

B is unkeyed blake2b-256, TAG(s) the ASCII string s zero-padded to 16 bytes, integers little-endian:

    key_tag = B(TAG("h2v-seed-key/1") || plan blob bytes)
    leaf_i  = B(TAG("h2v-seed-leaf/1") || LE32(|inst_i|) || LE32(|ci_i|) || LE32(|proof_i|) || LE32(0) || inst_i || ci_i || proof_i)
    node    = B(TAG("h2v-seed-node/1") || LE32(level) || LE32(m) || LE64(index in its level) || child_0 .. child_{m-1})
              64-ary; level 1 sits over the leaves; levels are added until one node is left (n = 1: one level-1 node)
    seed    = B(TAG("h2v-seed-root/1") || LE32(form) || LE32(0) || LE64(n) || key_tag || top node)

form 1: proofs (inst_i = the proof's instance bytes, ci_i = its committed bytes, proof_i = its bytes as given, short or long);
form 2: pairs (h2v_check_pairs_rlc: |inst| = |ci| = 0, proof_i = the 96 pair bytes).  The coefficients follow from the seed as
from any other: r_i = the low 128 bits of B(seed' || LE32(pos)), 1 if that is 0 (tests/agg_model.py::coeff).

form 3, "keyed leaves" (H2V_RLC_SEED_KEYED, the mixed-key calls; frozen): every leaf binds the key of its own
proof, and the root binds none -

    mleaf_i = B(TAG("h2v-seed-mleaf/1") || LE32(|inst_i|) || LE32(|ci_i|) || LE32(|proof_i|) || LE32(0)
                || key_tag(plans[plan_of[i]]) || inst_i || ci_i || proof_i)
    seed    = B(TAG("h2v-seed-root/1") || LE32(3) || LE32(0) || LE64(n) || 32 zero bytes || top node)

with the same node and tree.  The leaves enter in the caller's order (the position the coefficients are drawn from); inst_i is the
proof's own 32 * n_pi(plan) bytes, ci_i its 48 committed bytes or empty, proof_i its bytes as given (a descending pair of offsets:
empty).  The seed does not depend on the order in which the plans are listed, on listed plans without a proof or on the call's
flags; it does depend on which key every position has; and a one-plan mixed call does NOT share its seed with the form 1 call on
the same bytes."""
import hashlib
import struct

ARITY = 64
FORM_PROOFS, FORM_PAIRS, FORM_MIXED = 1, 2, 3
MAX_N = 1 << 22


def B(data: bytes) -> bytes:
    return hashlib.blake2b(data, digest_size=32).digest()


def TAG(s: str) -> bytes:
    raw = s.encode("ascii")
    assert len(raw) <= 16
    return raw.ljust(16, b"\0")


def key_tag(plan_bytes: bytes) -> bytes:
    return B(TAG("h2v-seed-key/1") + bytes(plan_bytes))


def leaf(inst: bytes, ci: bytes, proof: bytes) -> bytes:
    return B(TAG("h2v-seed-leaf/1") + struct.pack("<IIII", len(inst), len(ci), len(proof), 0) + bytes(inst) + bytes(ci) + bytes(proof))


def node(level: int, index: int, children) -> bytes:
    assert 1 <= len(children) <= ARITY
    return B(TAG("h2v-seed-node/1") + struct.pack("<IIQ", level, len(children), index) + b"".join(children))


def level_counts(n: int):
    """nodes of level 1, 2, ... of a tree over n >= 1 leaves; the last entry is 1"""
    assert 1 <= n <= MAX_N
    out = []
    while True:
        n = (n + ARITY - 1) // ARITY
        out.append(n)
        if n == 1:
            return out


def root(leaves) -> bytes:
    """the top node over a list of leaf digests"""
    cur, level = list(leaves), 0
    while True:
        level += 1
        cur = [node(level, j, cur[ARITY * j:ARITY * j + ARITY]) for j in range((len(cur) + ARITY - 1) // ARITY)]
        if len(cur) == 1:
            return cur[0]


def seed_of_leaves(tag: bytes, form: int, leaves) -> bytes:
    assert len(tag) == 32 and form in (FORM_PROOFS, FORM_PAIRS)
    return B(TAG("h2v-seed-root/1") + struct.pack("<IIQ", form, 0, len(leaves)) + tag + root(leaves))


def batch_seed(tag: bytes, form: int, instances, committed, proofs) -> bytes:
    """tag: key_tag(plan bytes); instances / committed / proofs: one bytes object per proof (instances / committed may be None:
    every proof's is empty).  form 2: proofs = the 96-byte pairs."""
    n = len(proofs)
    inst = instances if instances is not None else [b""] * n
    ci = committed if committed is not None else [b""] * n
    assert len(inst) == n and len(ci) == n
    return seed_of_leaves(tag, form, [leaf(inst[i], ci[i], proofs[i]) for i in range(n)])


def batch_seed_flat(tag: bytes, proofs: bytes, proof_off, instances: bytes = b"", committed: bytes = b"", n_pi: int = 0, n_ci: int = 0) -> bytes:
    """form 1 from the flat buffers of an h2v_batch: proof i = proofs[proof_off[i] : proof_off[i + 1]], 32 * n_pi instance bytes and
    48 * n_ci committed bytes per proof"""
    n = len(proof_off) - 1
    return batch_seed(tag, FORM_PROOFS,
                      [bytes(instances[32 * n_pi * i:32 * n_pi * (i + 1)]) for i in range(n)],
                      [bytes(committed[48 * n_ci * i:48 * n_ci * (i + 1)]) if n_ci else b"" for i in range(n)],
                      [bytes(proofs[proof_off[i]:proof_off[i + 1]]) for i in range(n)])


def pairs_seed(tag: bytes, pairs: bytes) -> bytes:
    """form 2: n = len(pairs) / 96 pairs"""
    assert len(pairs) % 96 == 0
    return batch_seed(tag, FORM_PAIRS, None, None, [bytes(pairs[96 * i:96 * i + 96]) for i in range(len(pairs) // 96)])


# ---- form 3: keyed leaves (the mixed-key calls)
def mixed_leaf(tag: bytes, inst: bytes, ci: bytes, proof: bytes) -> bytes:
    """tag: key_tag of the proof's own plan"""
    assert len(tag) == 32
    return B(TAG("h2v-seed-mleaf/1") + struct.pack("<IIII", len(inst), len(ci), len(proof), 0) + bytes(tag) + bytes(inst) + bytes(ci) + bytes(proof))


def mixed_seed(tags, plan_of, instances, committed, proofs) -> bytes:
    """tags: key_tag per listed plan; plan_of[i]: the plan of proof i; instances / committed / proofs: one bytes object per proof in
    the caller's order (committed[i] = b"" or None for a plan without a committed instance)"""
    n = len(proofs)
    assert 1 <= n <= MAX_N and len(plan_of) == n and len(instances) == n and len(committed) == n
    leaves = [mixed_leaf(tags[plan_of[i]], instances[i], committed[i] or b"", proofs[i]) for i in range(n)]
    return B(TAG("h2v-seed-root/1") + struct.pack("<IIQ", FORM_MIXED, 0, n) + bytes(32) + root(leaves))


def mixed_seed_flat(tags, shapes, plan_of, proofs: bytes, proof_off, instances: bytes = b"", committed: bytes = b"") -> bytes:
    """form 3 from the flat buffers of an h2v_mixed_batch: shapes[k] = (n_pi, n_ci) of listed plan k; proof i =
    proofs[proof_off[i] : proof_off[i + 1]] (descending: empty), its 32 * n_pi instance bytes and - n_ci = 1 - 48 committed bytes
    follow those of the proofs before it"""
    n = len(proof_off) - 1
    inst, ci, prf, at_i, at_c = [], [], [], 0, 0
    for i in range(n):
        n_pi, n_ci = shapes[plan_of[i]]
        inst.append(bytes((instances or b"")[at_i:at_i + 32 * n_pi]))
        at_i += 32 * n_pi
        ci.append(bytes((committed or b"")[at_c:at_c + 48]) if n_ci else b"")
        at_c += 48 if n_ci else 0
        prf.append(bytes(proofs[proof_off[i]:proof_off[i + 1]]) if proof_off[i + 1] > proof_off[i] else b"")
    return mixed_seed(tags, plan_of, inst, ci, prf)
