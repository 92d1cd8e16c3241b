"""Helper (not a test): verifying keys whose commitments are the point at infinity, repeated, or G / -G.

A fixed column of zeros or an unused selector commits to the identity, and two equal columns commit to the same point, so a
key's VK bases may hold the identity and repeats.  vk.BUILDERS / vk.WIDE_BUILDERS draw every commitment as [d]G with d in
[1, r); variants() edits such a key and its trapdoor TOGETHER (identity <-> dlog 0, G <-> 1, -G <-> r - 1), so that
synth.forge_batch still forges accepting proofs.  Labels:

  fixed0_inf         the first fixed commitment is the identity
  perm_last_inf      the last permutation commitment is the identity
  all_inf            every commitment of the key itself is the identity (-G1 stays: it is a constant of the verifier)
  all_equal          every commitment is the first fixed commitment
  gen_and_neg        first fixed = G, last permutation = -G (the same point as the verifier's own -G1 base)
  inner_fixed_inf    recursive keys: every fixed commitment of every inner key is the identity
  last_segment_inf   wide keys (more than 64 MSM terms): every commitment from the first all-VK-base segment on is the
                     identity, see segment_cut

The expectations of the tests that use these keys come from the CPU oracle (oracle_pairs, oracle_vk_scalars) and from the
big-integer models, never from the code under test."""
import functools
import json
from concurrent.futures import ThreadPoolExecutor
from dataclasses import replace

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, ivc, plan as PL, vk as V

R = bls.R
INF_HEX = bls.g1_compress(None).hex()
# the shapes tests/golden/msm_shape_table.txt has a row for (tests/test_msm_shape.py holds csrc/h2v_msm_shape.hpp to it)
SHAPE_N, SHAPE_HINT = 8, 1


def builder(name):
    return V.BUILDERS[name] if name in V.BUILDERS else V.WIDE_BUILDERS[name]


@functools.lru_cache(maxsize=None)
def commit(dlog: int) -> str:
    """compressed hex of [dlog]G; dlog 0 is the identity"""
    return bls.g1_compress(bls.g1_mul(bls.G1_GEN, dlog % R) if dlog % R else None).hex()


def _with_dlogs(vk, td, fixed=None, perm=None):
    """(vk', td') with the given dlog lists (None: unchanged); only the commitments whose dlog changed are recomputed"""
    def redo(old_hex, old_d, new_d):
        return [h if d == e else commit(e) for h, d, e in zip(old_hex, old_d, new_d)]
    fixed = list(td.fixed_dlogs) if fixed is None else [d % R for d in fixed]
    perm = list(td.perm_dlogs) if perm is None else [d % R for d in perm]
    assert len(fixed) == len(td.fixed_dlogs) and len(perm) == len(td.perm_dlogs)
    return (replace(vk, fixed_commitments=redo(vk.fixed_commitments, td.fixed_dlogs, fixed),
                    permutation_commitments=redo(vk.permutation_commitments, td.perm_dlogs, perm)),
            replace(td, fixed_dlogs=fixed, perm_dlogs=perm))


# ---- the launch-shape model's segments (wide keys)
def model_shape(T, n_var, n_fix, option, n=SHAPE_N, hint=SHAPE_HINT):
    """The single launch the host-only shape model (csrc/h2v_msm_shape.hpp) decides for a sum of T terms on an MI355X under
    `option` ("none=0", "lpt=1", "lpt=2", ...), read from the committed table that tests/test_msm_shape.py holds the model to:
    {lpt, bs, n_seg, seg_terms} and the split's {on, k, var_lpt, var_n_seg}."""
    from tests.test_msm_shape import _table
    head = "%d %d %d %d %d %s : " % (T, n_var, n_fix, n, hint, option)
    rows = [line for line in _table() if line.startswith(head)]
    assert len(rows) == 1, "the shape table has no row for %r" % head
    single, split = [[int(float(x)) for x in g.split()] for g in rows[0].split(" : ")[1:3]]
    return {"lpt": single[0], "bs": single[1], "n_seg": single[2], "seg_terms": single[3],
            "split": {"on": split[0], "k": split[1], "var_lpt": split[3], "var_n_seg": split[5]}}


def segments(T, shape):
    """[lo, hi) term ranges of the segments of a shape (k_g1_msm_seg: segment s = terms [s seg_terms, (s + 1) seg_terms))"""
    if shape["n_seg"] <= 1:
        return [(0, T)]
    ts = shape["seg_terms"]
    out = [(lo, min(lo + ts, T)) for lo in range(0, T, ts)]
    assert len(out) == shape["n_seg"]
    return out


def plan_counts(pl):
    """(T, per-proof terms, VK-base terms) of the proof's own sum: the VK-base terms are its tail (plan.py: a stable partition)"""
    main = pl.terms[:pl.n_main_terms]
    n_fix = sum(1 for kind, _ in main if kind == PL.TERM_VK_BASE)
    assert all(kind == PL.TERM_VK_BASE for kind, _ in main[len(main) - n_fix:])
    return len(main), len(main) - n_fix, n_fix


def segment_cut(pl):
    """The first term of the earliest segment - under the forced shapes lpt=1 and lpt=2 - that holds VK-base terms only.

    The LAST term of every main sum is the verifier's own -G1 (scalar v), which no key can make the identity, so the last
    segment's partial sum is [v](-G1), never the point at infinity.  What a key CAN do: with every commitment from this cut on
    the identity, the last segment of either shape has one live lane (-G1) beside skipped ones, and every all-VK-base segment
    before it - under lpt=2 there is at least one (asserted by the tests) - sums to the point at infinity, which
    k_g1_sum_segments must add in the middle of its fold."""
    T, n_var, n_fix = plan_counts(pl)
    cuts = []
    for opt in ("lpt=1", "lpt=2"):
        sh = model_shape(T, n_var, n_fix, opt)
        assert sh["n_seg"] > 1, (opt, sh)
        cuts.append(min(lo for lo, _hi in segments(T, sh) if lo >= n_var))
    return min(cuts)


def _commitment_of_term(pl, t):
    """("fixed" | "perm", index) of a VK-base term of the key's own commitments, None for -G1 (plan.py names the terms)"""
    name = pl.term_names[t]
    if name == "neg_g1_generator":
        return None
    assert name.endswith("_commitment") and name[0] in "fp", name
    return ("fixed" if name[0] == "f" else "perm"), int(name[1:name.index("_")]) - 1


def variants(name):
    """yields (label, vk, trapdoor) for the builder's key with edited commitments"""
    vk, td = builder(name)()
    nf, np_ = len(td.fixed_dlogs), len(td.perm_dlogs)
    assert nf >= 1 and np_ >= 1
    yield ("fixed0_inf",) + _with_dlogs(vk, td, fixed=[0] + td.fixed_dlogs[1:])
    yield ("perm_last_inf",) + _with_dlogs(vk, td, perm=td.perm_dlogs[:-1] + [0])
    yield ("all_inf",) + _with_dlogs(vk, td, fixed=[0] * nf, perm=[0] * np_)
    yield ("all_equal",) + _with_dlogs(vk, td, fixed=[td.fixed_dlogs[0]] * nf, perm=[td.fixed_dlogs[0]] * np_)
    yield ("gen_and_neg",) + _with_dlogs(vk, td, fixed=[1] + td.fixed_dlogs[1:], perm=td.perm_dlogs[:-1] + [R - 1])
    if vk.recursion_vks is not None:
        inner, dl, k = [], list(td.rec_dlogs), 0
        for v in vk.recursion_vks:                       # rec_dlogs: per inner key its fixed, then its permutation commitments
            f = len(v["fixed_commitments"])
            inner.append(dict(v, fixed_commitments=[INF_HEX] * f))
            dl[k:k + f] = [0] * f
            k += f + len(v["permutation_commitments"])
        assert k == len(dl)
        yield "inner_fixed_inf", replace(vk, recursion_vks=inner), replace(td, rec_dlogs=dl)
    if name in V.WIDE_BUILDERS and vk.recursion_vks is None:
        pl = PL.compile_plan(vk)
        cut = segment_cut(pl)
        fixed, perm = list(td.fixed_dlogs), list(td.perm_dlogs)
        for t in range(cut, pl.n_main_terms):
            c = _commitment_of_term(pl, t)
            if c is not None:
                (fixed if c[0] == "fixed" else perm)[c[1]] = 0
        yield ("last_segment_inf",) + _with_dlogs(vk, td, fixed=fixed, perm=perm)


def variant(name, label):
    for lab, vk, td in variants(name):
        if lab == label:
            return vk, td
    raise KeyError((name, label))


def expected_nones(vk):
    """identities among the plan's VK bases, counted from the key alone: -G1, the key's commitments, the inner keys' (recursive)"""
    own = list(vk.fixed_commitments) + list(vk.permutation_commitments)
    inner = [h for v in (vk.recursion_vks or []) for h in v["fixed_commitments"] + v["permutation_commitments"]]
    return sum(1 for h in own + inner if h == INF_HEX), 1 + len(own) + len(inner)


# ---- the oracle's side
def oracle_vk(orc, vk):
    return orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))


def oracle_pairs(ov, orc, batch, n_pi):
    """per proof: (accept, the pair the oracle's pairing checks - or 96 zero bytes where it stops before the pairing)"""
    def one(i):
        ok, otr = ov.verify(batch.proof(i), batch.instance_ints(i, n_pi), batch.ci(i), trace=True)
        if otr.status in (0, 1):
            return int(ok), orc.g1_compress(otr.point("el")) + orc.g1_compress(otr.point("er"))
        return int(ok), bytes(96)
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, range(batch.n)))


def oracle_vk_scalars(ov, otr):
    """{("fixed" | "perm", i): the scalar the multi-open argument gives that commitment} from the ORACLE's trace (x1, x4) and the
    oracle's own commitment map: commitment number j of the point set sorted to position s gets x4^s x1^j
    (halo2_kzg.ak:96-119; plan.py builds its terms by the same rule, which test_degenerate_keys.py cross-checks)."""
    x1, x4 = otr.scalar("x1"), otr.scalar("x4")
    seen, out = {}, {}
    for e in ov.commitment_map():
        kind, idx = e["commitment"]
        j = seen.get(e["set"], 0)
        seen[e["set"]] = j + 1
        if kind in ("fixed", "common"):
            out[("fixed" if kind == "fixed" else "perm", idx)] = pow(x4, e["sorted_set"], R) * pow(x1, j, R) % R
    return out


def identity_term_scalars(vk, ov, batch, i):
    """The scalars that multiply an identity base in proof i, from the oracle's trace and the proof's public inputs alone:
    the multi-open scalars of the key's identity commitments and - recursive keys - the accumulator's fixed-base scalars of
    every identity among ivc.fixed_bases.  [] where the oracle stops before the MSM."""
    ints = batch.instance_ints(i, vk.n_public_inputs)
    ok, otr = ov.verify(batch.proof(i), ints, batch.ci(i), trace=True)
    if otr.status not in (0, 1):
        return []
    sc = oracle_vk_scalars(ov, otr)
    out = [sc[("fixed", k)] for k, h in enumerate(vk.fixed_commitments) if h == INF_HEX]
    out += [sc[("perm", k)] for k, h in enumerate(vk.permutation_commitments) if h == INF_HEX]
    if vk.recursion_vks is not None:
        lay = ivc.layout(vk)
        out += [ints[pos] % R for h, pos in zip(ivc.fixed_bases(vk), lay["fixed_scalars"]) if h == INF_HEX]
    return out


# ---- the Python plan interpreter's side
def interpreter_pair(vk, pl, batch, i):
    """(accept-so-far, compress(el) || compress(er)) of proof i from plan.run_plan and big-integer curve arithmetic: er = the sum
    of the plan's terms with the interpreter's scalars, el = pi, folded with the accumulator for a recursive key (ivc.fold).
    None where the interpreter or the decoding of a point rejects (the pairing's own verdict is not computed here)."""
    proof, ints, ci = batch.proof(i), batch.instance_ints(i, vk.n_public_inputs), batch.ci(i)
    scalars, _regs, status = PL.run_plan(pl, proof, ints, ci)
    if status is not None:
        return None
    try:
        pts = [bls.g1_decompress(proof[o:o + 48], True) for o in pl.points]
        cip = bls.g1_decompress(ci, True) if ci is not None else None
    except ValueError:
        return None
    er = None
    for t, (kind, idx) in enumerate(pl.terms[:pl.n_main_terms]):
        base = pts[idx] if kind == PL.TERM_PROOF_POINT else pl.vk_bases[idx] if kind == PL.TERM_VK_BASE else cip
        er = bls.g1_add(er, bls.g1_mul(base, scalars[t]))
    el = pts[pl.pi_point]
    if vk.recursion_vks is not None:
        try:
            el, er, _c = ivc.fold(vk, ints, el, er)
        except ivc.Reject:
            return None
    return bls.g1_compress(el) + bls.g1_compress(er)
