"""Edge accumulators for the recursion (IVC) fold: a table of makers that write the accumulator fields of a proof's public
inputs from the test SRS's trapdoor, as ivc.make_accumulator does, but at the edges the random generic accumulator never
meets - coordinates whose limbs wrap past p, sums at infinity, a segmented reduction that must double or cancel, the sign
boundary of y, a small-order point, scalars at the ends, a limb that is not canonical, and an opening point at infinity.

A helper module, not a test (as tests/cancel.py and tests/pip_model.py): tests/test_ivc_edges.py pins the C oracle and the
big-integer model (ivc.fold) to this table and to each other, tests/test_ivc_edges_gpu.py the device path to the oracle.

Notation: left point [a]G with scalar il, right point [b]G with scalar ir, fixed = sum_k inst[k] dlog_k over the fixed
bases; acc_left = [il a]G, acc_right_final = [ir b + fixed]G; the accumulator is valid iff s il a == ir b + fixed.  Every
value a maker writes is below r; `post` steps (an instance limb + r, the opening point overwritten) run on the forged bytes.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Callable, List, NamedTuple, Optional

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from plutus_halo2_verifier_gen_amd import ivc
from plutus_halo2_verifier_gen_amd import plan as PL
from plutus_halo2_verifier_gen_amd import synth

P, R, B224 = bls.P, bls.R, ivc.B224
LEFT = ("left_x", "left_y", "left_scalar")
RIGHT = ("right_x", "right_y", "right_scalar")


class Kind(NamedTuple):
    name: str
    make: Callable            # (vk, td, rng, inst) -> None
    expected: str             # the oracle's reason (oracle.binding.STATUS): "accept", "pairing", "point", "scalar"
    post: Optional[Callable] = None   # (plan, vk, proof bytearray, inst list) -> None, on the forged proof


def _inv(v):
    return pow(v % R, -1, R)


def _dlogs(td):
    return [R - 1] + list(td.fixed_dlogs) + list(td.perm_dlogs) + list(td.rec_dlogs)


def _fixed(vk, td, lay, inst):
    dlogs = _dlogs(td)
    assert len(dlogs) == lay["F"]
    return sum(inst[k] * d for k, d in zip(lay["fixed_scalars"], dlogs)) % R


def _put_t(inst, lay, key, t):
    """coordinate `key` as the raw pair (t >> 224, t mod 2^224): coord = (1 + t) mod p, whatever t is"""
    inst[lay[key][0]], inst[lay[key][1]] = t >> 224, t & (B224 - 1)


def _put(inst, lay, side, dlog, scalar):
    """the canonical accumulator fields of one side, as make_accumulator writes them; returns the affine point"""
    xs, ys, sk = side
    pt = synth.fixed_base().mul(dlog)
    assert pt is not None
    _put_t(inst, lay, xs, (pt[0] - 1) % P)
    _put_t(inst, lay, ys, (pt[1] - 1) % P)
    inst[lay[sk]] = scalar
    return pt


def _maker(pick=None, tweak=None, zero_fixed=False):
    """pick(q) -> (a, b, il, ir) with b == None / a == None for `from the validity equation`; q carries s, fixed, the random
    draws a, il, ir, rng, and the fixed bases' dlogs and scalars; tweak(inst, lay, left point, right point) rewrites fields
    afterwards"""
    def make(vk, td, rng, inst):
        lay = ivc.layout(vk)
        inst[lay["vk_hash"]] = vk.transcript_repr
        if zero_fixed:
            for k in lay["fixed_scalars"]:
                inst[k] = 0
        fixed = _fixed(vk, td, lay, inst)
        a, il, ir = rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R)
        b = None
        if pick is not None:
            q = SimpleNamespace(s=td.s, fixed=fixed, a=a, il=il, ir=ir, rng=rng, dlogs=_dlogs(td),
                                scalars=[inst[k] for k in lay["fixed_scalars"]])
            a, b, il, ir = pick(q)
        if b is None:
            b = (td.s * il * a - fixed) * _inv(ir) % R
        if a is None:
            a = (ir * b + fixed) * _inv(td.s * il) % R
        assert a % R and b % R, "the accumulator's points are finite"
        lp = _put(inst, lay, LEFT, a, il)
        rp = _put(inst, lay, RIGHT, b, ir)
        if tweak is not None:
            tweak(inst, lay, lp, rp)
        assert all(0 <= v < R for v in inst)
    return make


def _wrap(key, k_of_t):
    def tweak(inst, lay, lp, rp):
        pt = lp if key.startswith("left") else rp
        t = (pt[0 if key.endswith("x") else 1] - 1) % P
        t2 = t + k_of_t(t) * P
        assert t2 >= P and P >> 224 <= (t2 >> 224) < R     # (a canonical hi is at most (p - 1) >> 224)
        _put_t(inst, lay, key, t2)
        assert ivc.coord(*[inst[i] for i in lay[key]]) == (t + 1) % P
    return tweak


def _lo_overlap(inst, lay, lp, rp):
    hi, lo = (inst[i] for i in lay["left_x"])
    assert hi > 0
    inst[lay["left_x"][0]], inst[lay["left_x"][1]] = hi - 1, lo + B224
    assert ivc.coord(hi - 1, lo + B224) == lp[0]


def _larger(y):
    return y > P - y


def _y_boundary(inst, lay, lp, rp):
    _put_t(inst, lay, "left_y", ((P + 1) // 2 if _larger(lp[1]) else (P - 1) // 2) - 1)


def _y_boundary_wrapped(inst, lay, lp, rp):
    assert _larger(lp[1])
    _put_t(inst, lay, "left_y", (P + 1) // 2 - 1 + P)   # (p + 1) / 2 through limbs that wrap: one less and the sign flips


def _a_with_sign(want_larger):
    """`a` drawn until the left point's y has the wanted sign class"""
    def pick(q):
        a = q.a
        while _larger(synth.fixed_base().mul(a)[1]) != want_larger:
            a = q.rng.randrange(1, R)
        return a, None, q.il, q.ir
    return pick


def reduction_partner(n_fixed):
    """The term of group 2 (acc_right, then the n_fixed fixed bases) whose lanes the reduction adds to acc_right's FIRST: the
    tree adds lane g + s to lane g for s = ..., 4, 2, 1 times the lanes per term, so term 0 first meets term s*, the largest
    power of two below the group's 1 + n_fixed terms - at one or two lanes per term, or a quad per half, alike."""
    j = 1
    while 2 * j < 1 + n_fixed:
        j *= 2
    return j


def _right_on_base(sign):
    """the right point is (sign = -1: the negative of) the fixed base it meets first in the reduction, with that base's scalar:
    both GLV halves of the two terms are equal (opposite) points, so whatever the lanes per term the first addition of the
    group's reduction doubles (cancels, and the tree goes on from a partial sum at infinity).  a from the validity equation."""
    def pick(q):
        k = reduction_partner(len(q.dlogs)) - 1
        assert q.scalars[k] % R
        return None, sign * q.dlogs[k] % R, q.il, q.scalars[k]
    return pick


def _y_zero(inst, lay, lp, rp):
    _put_t(inst, lay, "left_y", P - 1)          # coord == 0: "not larger", whatever the point's y is
    assert ivc.coord(*[inst[i] for i in lay["left_y"]]) == 0


def _order3(inst, lay, lp, rp):
    _put_t(inst, lay, "left_x", P - 1)          # x == 0: (0, +-2), a point of order 3 on y^2 = x^3 + 4
    assert ivc.coord(*[inst[i] for i in lay["left_x"]]) == 0


def _off_curve(inst, lay, lp, rp):
    x = 0
    while bls.fp_sqrt((x ** 3 + 4) % P) is not None:
        x += 1
    _put_t(inst, lay, "left_x", (x - 1) % P)


def _add_r(key, part=None):
    def post(pl, vk, proof, inst):
        lay = ivc.layout(vk)
        k = lay[key] if part is None else lay[key][part]
        assert inst[k] + R < 1 << 256
        inst[k] += R
    return post


def _pi_infinity(pl, vk, proof, inst):
    o = pl.points[pl.pi_point]
    proof[o:o + 48] = bls.g1_compress(None)
    assert proof[o] == 0xC0 and not any(proof[o + 1:o + 48])


_valid = _maker()
KINDS: List[Kind] = [
    Kind("plain", _valid, "accept"),
    Kind("wrap1_left_x", _maker(tweak=_wrap("left_x", lambda t: 1)), "accept"),
    Kind("wrap1_left_y", _maker(tweak=_wrap("left_y", lambda t: 1)), "accept"),
    Kind("wrap1_right_x", _maker(tweak=_wrap("right_x", lambda t: 1)), "accept"),
    Kind("wrap1_right_y", _maker(tweak=_wrap("right_y", lambda t: 1)), "accept"),
    # the largest multiple of p that keeps hi < r: hi * 2^224 + lo + 1 is about 2^98 p
    Kind("wrap_max_left_x", _maker(tweak=_wrap("left_x", lambda t: (R * B224 - 1 - t) // P)), "accept"),
    Kind("lo_overlap", _maker(tweak=_lo_overlap), "accept"),
    # il == 0 and b from the validity equation: acc_left = [0]P and acc_right + acc_fixed = O, el' = el, er' = er
    Kind("left_scalar_0", _maker(lambda q: (q.a, None, 0, q.ir)), "accept"),
    Kind("left_scalar_0_reject", _maker(lambda q: (q.a, q.rng.randrange(1, R), 0, q.ir)), "pairing"),
    Kind("left_scalar_max", _maker(lambda q: (q.a, None, R - 1, q.ir)), "accept"),
    Kind("right_scalar_0", _maker(lambda q: (None, q.rng.randrange(1, R), q.il, 0)), "accept"),
    Kind("fixed_all_0", _maker(zero_fixed=True), "accept"),
    # acc_right == acc_fixed: the reduction of group 2 must double;  acc_right == -acc_fixed: it must cancel
    Kind("right_equals_fixed", _maker(lambda q: (None, q.fixed * _inv(q.ir) % R, q.il, q.ir)), "accept"),
    Kind("right_cancels_fixed", _maker(lambda q: (q.a, -q.fixed * _inv(q.ir) % R, q.il, q.ir)), "pairing"),
    # ... which the sums above do only in the LAST addition of the tree, (sum of the even lanes) + (sum of the odd ones), where equal
    # totals are not equal summands; these two make the FIRST addition of group 2 exceptional
    Kind("right_doubles_a_base", _maker(_right_on_base(1)), "accept"),
    Kind("right_cancels_a_base", _maker(_right_on_base(-1)), "accept"),
    Kind("same_point", _maker(lambda q: (q.a, q.a, q.il, (q.s * q.il - q.fixed * _inv(q.a)) % R)), "accept"),
    # the sign class of y at its boundary: (p + 1) / 2 is the smallest "larger" value, (p - 1) / 2 the largest other one
    Kind("y_boundary_hi", _maker(_a_with_sign(True), _y_boundary), "accept"),
    Kind("y_boundary_lo", _maker(_a_with_sign(False), _y_boundary), "accept"),
    # y enters by its sign alone, so wrap1_left_y / wrap1_right_y cannot see a coordinate that is off by one: this one can
    Kind("wrap1_left_y_boundary", _maker(_a_with_sign(True), _y_boundary_wrapped), "accept"),
    # y == 0 reads as "not larger": the same point when the true y is not larger, the negated one when it is
    Kind("y_zero_accept", _maker(_a_with_sign(False), _y_zero), "accept"),
    Kind("y_zero_reject", _maker(_a_with_sign(True), _y_zero), "pairing"),
    Kind("order3", _maker(tweak=_order3), "point"),
    Kind("off_curve", _maker(tweak=_off_curve), "point"),
    Kind("limb_ge_r_coord", _valid, "scalar", _add_r("left_x", 1)),
    Kind("limb_ge_r_scalar", _valid, "scalar", _add_r("left_scalar")),
    # a valid accumulator, the proof's opening point the infinity encoding: el' = c acc_left
    Kind("pi_infinity", _valid, "pairing", _pi_infinity),
]
BY_NAME = {k.name: k for k in KINDS}
NAMES = [k.name for k in KINDS]
ACCEPTING = [k.name for k in KINDS if k.expected == "accept"]
INFINITE_SUM = ("left_scalar_0", "left_scalar_0_reject", "right_cancels_fixed")   # an accumulator sum at infinity


def placement(n: int) -> List[str]:
    """kind of each proof of the placement batch: the table cycled, pi_infinity first, right_equals_fixed in lane 63 of the
    challenge kernel's first block, an infinite-sum kind in the last place (at n = 65 alone in the second block, where the
    dead lanes shadow it)"""
    names = [NAMES[i % len(NAMES)] for i in range(n)]
    names[0] = "pi_infinity"
    if n > 63:
        names[63] = "right_equals_fixed"
    if n > 1:
        names[n - 1] = "left_scalar_0"
    return names


def forge(vk, td, pl, names, seed) -> synth.Batch:
    """one proof per name, forged in process around that kind's accumulator; expected[] from the table"""
    hook = lambda vk_, td_, rng, inst, i: BY_NAME[names[i]].make(vk_, td_, rng, inst)
    batch = synth.forge_batch(vk, td, len(names), seed=seed, plan=pl, workers=1, accumulator=hook)
    n_pi = vk.n_public_inputs
    proofs, insts = [], []
    for i, name in enumerate(names):
        proof, inst = bytearray(batch.proof(i)), batch.instance_ints(i, n_pi)
        if BY_NAME[name].post is not None:
            BY_NAME[name].post(pl, vk, proof, inst)
        proofs.append(bytes(proof))
        insts.append(b"".join(v.to_bytes(32, "little") for v in inst))
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return synth.Batch(n=batch.n, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=batch.committed,
                       expected=[int(BY_NAME[name].expected == "accept") for name in names])


def acc_sums(vk, inst: List[int]):
    """(acc_left, acc_right, acc_fixed) of the big-integer model, before acc_right + acc_fixed"""
    lay = ivc.layout(vk)
    pt = lambda xs, ys: ivc.g1_from_coords(ivc.coord(inst[lay[xs][0]], inst[lay[xs][1]]), ivc.coord(inst[lay[ys][0]], inst[lay[ys][1]]))
    left = bls.g1_mul(pt("left_x", "left_y"), inst[lay["left_scalar"]])
    right = bls.g1_mul(pt("right_x", "right_y"), inst[lay["right_scalar"]])
    fixed = None
    for h, k in zip(ivc.fixed_bases(vk), lay["fixed_scalars"]):
        fixed = bls.g1_add(fixed, bls.g1_mul(bls.g1_decompress(bytes.fromhex(h), False), inst[k]))
    return left, right, fixed


def expected_fold(vk, pl, proof: bytes, inst: List[int]):
    """The big-integer model on one proof: (el', er', c) of ivc.fold with er rebuilt from the plan's main MSM, or the
    ivc.Reject - with .reason "scalar" / "recursion" / ... from the plan interpreter, "point" from g1_from_coords - where the
    verifier stops before the pairing."""
    scal, _, status = PL.run_plan(pl, proof, inst, None)
    if status is not None:
        e = ivc.Reject("plan: %s" % status)
        e.reason = status
        return e
    pts = [bls.g1_decompress(proof[o:o + 48]) for o in pl.points]
    er = None
    for t, (k, idx) in enumerate(pl.terms[:pl.n_main_terms]):
        er = bls.g1_add(er, bls.g1_mul(pts[idx] if k == PL.TERM_PROOF_POINT else pl.vk_bases[idx], scal[t]))
    try:
        return ivc.fold(vk, inst, pts[pl.pi_point], er)
    except ivc.Reject as e:
        e.reason = "point"
        return e
