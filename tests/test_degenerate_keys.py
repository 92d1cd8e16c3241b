"""Keys whose commitments are the identity, repeated, or G / -G (tests/degenerate_keys.py), what can be said without a GPU:
the plan compiler keeps such bases (None in Plan.vk_bases, 96 zero bytes in the blob), the C++ compiler behind the C-ABI writes
the same blob byte for byte, the loader's validation accepts it, the Python plan interpreter and the C oracle agree on
verdicts and on (el, er) for a small batch with rejects, and the constant files (wire.py) carry such keys both ways.

Non-vacuity, asserted per variant from the ORACLE's side alone: some proof of the batch multiplies an identity base by a
non-zero scalar.  A kernel that skips zero scalars would otherwise hide a missing skip of the identity."""
import random
from dataclasses import replace

import pytest

from plutus_halo2_verifier_gen_amd import backend, bls12_381 as bls, plan as PL, synth, vk as V, wire
from tests import agg_model, degenerate_keys as D

NARROW = ("simple_mul", "lookup_table", "ivc")
WIDE = "wide335"
LABELS = {name: ["fixed0_inf", "perm_last_inf", "all_inf", "all_equal", "gen_and_neg"] for name in NARROW + (WIDE,)}
LABELS["ivc"].append("inner_fixed_inf")
LABELS[WIDE].append("last_segment_inf")
CASES = [(name, label) for name in NARROW + (WIDE,) for label in LABELS[name]]
# identities among the plan's VK bases / VK bases: simple_mul 2 fixed + 3 permutation + -G1, lookup_table 4 + 4 + 1,
# ivc 6 + 4 + 1 and the inner key's 2 + 2, wide335 240 + 30 + 1 (last_segment_inf: the terms from 112 on but -G1)
NONES = {"simple_mul": (1, 1, 5, 6), "lookup_table": (1, 1, 8, 9), "ivc": (1, 1, 10, 15), WIDE: (1, 1, 270, 271)}
BATCH_SEED = 5          # (every variant's batch: forged with seed 5, rejects drawn with seed 6)


@pytest.fixture(scope="module")
def keys():
    """(name, label) -> (vk, trapdoor, plan); a variant is built once per module"""
    out = {}
    for name in NARROW + (WIDE,):
        got = []
        for label, vk, td in D.variants(name):
            out[(name, label)] = (vk, td, PL.compile_plan(vk))
            got.append(label)
        assert got == LABELS[name]
    return out


def _loader_accepts(blob):
    """h2v_plan_load validates the blob on the host before any device work: without a GPU a good plan ends as H2V_E_DEVICE (-3)"""
    try:
        backend.DevicePlan(blob, 0).close()
        return True
    except backend.H2VError as e:
        return "h2v error -3" in str(e)


@pytest.mark.parametrize("name,label", CASES)
def test_plan_keeps_the_bases_and_both_compilers_write_one_blob(keys, name, label):
    vk, td, pl = keys[(name, label)]
    V.validate(vk)
    nones = sum(1 for p in pl.vk_bases if p is None)
    assert (nones, len(pl.vk_bases)) == D.expected_nones(vk)
    one, one_p, every, total = NONES[name]
    want = {"fixed0_inf": one, "perm_last_inf": one_p, "all_inf": every, "all_equal": 0, "gen_and_neg": 0,
            "inner_fixed_inf": 2, "last_segment_inf": 222}[label]
    assert (nones, len(pl.vk_bases)) == (want, total)
    # no base was merged or dropped: repeated commitments stay one base per column
    own = len(vk.fixed_commitments) + len(vk.permutation_commitments)
    assert sum(1 for kind, _ in pl.terms[:pl.n_main_terms] if kind == PL.TERM_VK_BASE) == own + 1
    if label == "all_equal":
        first = bls.g1_decompress(bytes.fromhex(vk.fixed_commitments[0]))
        assert sum(1 for p in pl.vk_bases if p == first) >= own
    if label == "gen_and_neg":
        assert sum(1 for p in pl.vk_bases if p == bls.g1_neg(bls.G1_GEN)) == 2 and bls.G1_GEN in pl.vk_bases
    # the blob: the section holds what the plan holds - 96 zero bytes for the identity, Montgomery (x, y) otherwise
    blob = pl.to_bytes()
    hdr = [int.from_bytes(blob[8 + 4 * i:12 + 4 * i], "little") for i in range(PL.PLAN_HDR_WORDS)]
    assert hdr[8] == len(pl.vk_bases)
    r_inv = pow(1 << bls.MONT_BITS_FP, -1, bls.P)
    back = []
    for k in range(hdr[8]):
        rec = blob[hdr[17] + 96 * k:hdr[17] + 96 * k + 96]
        x, y = (int.from_bytes(rec[o:o + 48], "little") * r_inv % bls.P for o in (0, 48))
        back.append(None if rec == bytes(96) else (x, y))
    assert back == pl.vk_bases
    assert _loader_accepts(blob)
    # the byte-identical claim of tests/test_plan_compile.py on these keys
    assert backend.plan_compile(vk.to_json()) == blob
    # a JSON round trip of the description changes nothing
    assert PL.compile_plan(V.VerifyingKey.from_json(vk.to_json())).to_bytes() == blob


def test_the_wide_variant_follows_the_shape_model(keys):
    """last_segment_inf is cut where the host-only shape model (csrc/h2v_msm_shape.hpp, through the table tests/test_msm_shape.py
    holds it to) puts its segments: under lpt=2 one segment is all identities - its partial sum is the point at infinity - and
    under both forced shapes the last segment's only finite base is the verifier's own -G1."""
    vk, td, pl = keys[(WIDE, "last_segment_inf")]
    T, n_var, n_fix = D.plan_counts(pl)
    assert (T, n_var, n_fix) == (335, 64, 271) and D.segment_cut(pl) == 112
    finite = [pl.terms[t][0] != PL.TERM_VK_BASE or pl.vk_bases[pl.terms[t][1]] is not None for t in range(T)]
    assert pl.term_names[T - 1] == "neg_g1_generator" and finite[T - 1]
    all_inf_segments = {}
    for opt in ("none=0", "lpt=1", "lpt=2"):
        sh = D.model_shape(T, n_var, n_fix, opt)
        segs = D.segments(T, sh)
        assert sh["n_seg"] == len(segs) > 1 and segs[-1][1] == T, opt
        lo, hi = segs[-1]
        assert [t for t in range(lo, hi) if finite[t]] == [T - 1], opt
        all_inf_segments[opt] = [s for s, (lo, hi) in enumerate(segs) if not any(finite[lo:hi])]
    assert all_inf_segments == {"none=0": [1], "lpt=1": [], "lpt=2": [1]}
    # the forced split sums the per-proof terms in one unsegmented launch and leaves every VK base to the fixed-base lanes
    sp = D.model_shape(T, n_var, n_fix, "fix=1")["split"]
    assert sp["on"] == 1 and sp["k"] == 1 and sp["var_n_seg"] == 1


@pytest.mark.parametrize("name,label", CASES)
def test_interpreter_and_oracle_agree_on_a_batch_with_rejects(orc, keys, name, label):
    vk, td, pl = keys[(name, label)]
    ov = D.oracle_vk(orc, vk)
    if name == WIDE:
        # the big-integer sum of 335 terms takes seconds per proof: one accepting proof and one reject, of another kind per variant
        n = 2
        b = synth.forge_batch(vk, td, n, seed=BATCH_SEED, plan=pl, workers=1)
        kind = ["wrong_pi", "flip_last_scalar", "point_not_in_subgroup", "wrong_public_input", "infinity_commitment",
                "noncanonical_scalar"][LABELS[WIDE].index(label)]
        n_pi = vk.n_public_inputs
        p1, i1 = synth.corrupt(pl, b.proof(1), b.instances[32 * n_pi:64 * n_pi], kind, random.Random(BATCH_SEED + 1))
        b = synth.Batch(n=2, proofs=b.proof(0) + p1, proof_off=[0, len(b.proof(0)), len(b.proof(0)) + len(p1)],
                        instances=b.instances[:32 * n_pi] + i1, committed=b.committed, expected=[1, 0])
    else:
        n = 8
        b = synth.forge_batch(vk, td, n, seed=BATCH_SEED, plan=pl, workers=1)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.5, seed=BATCH_SEED + 1, kinds=list(synth.CORRUPTIONS))
    want = D.oracle_pairs(ov, orc, b, vk.n_public_inputs)
    assert [a for a, _ in want] == b.expected and 0 < sum(b.expected) < n
    for i in range(n):
        pair = D.interpreter_pair(vk, pl, b, i)
        if pair is None:                                     # rejected before the pairing by both
            assert want[i] == (0, bytes(96)), i
        else:
            assert pair == want[i][1], i
            assert int(agg_model.holds(pair, td.s)) == want[i][0], i      # the pairing's verdict, from the trapdoor
    # non-vacuity: an identity base meets a non-zero scalar (oracle's trace + public inputs), and the plan's terms agree
    n_inf = D.expected_nones(vk)[0]
    met = [D.identity_term_scalars(vk, ov, b, i) for i in range(n)]
    if n_inf:
        assert any(sc and all(sc) for sc in met), "no proof multiplies an identity base by a non-zero scalar"
        i = next(i for i, sc in enumerate(met) if sc)
        scalars, _regs, status = PL.run_plan(pl, b.proof(i), b.instance_ints(i, vk.n_public_inputs), b.ci(i))
        assert status is None
        mine = sorted(scalars[t] for t, (kind, idx) in enumerate(pl.terms) if kind == PL.TERM_VK_BASE and pl.vk_bases[idx] is None)
        assert mine == sorted(met[i]) and len(mine) >= n_inf
    else:
        assert all(sc == [] for sc in met)


# (VKConstants.check decompresses every commitment with its subgroup test: of the wide key only the variants that are mostly
#  identities, which cost nothing to decode)
@pytest.mark.parametrize("name,label", [c for c in CASES if c[0] != WIDE or c[1] in ("all_inf", "last_segment_inf")])
@pytest.mark.parametrize("flavour", ["aiken", "plinth"])
def test_constant_files_carry_the_key_both_ways(keys, name, label, flavour):
    vk, td, pl = keys[(name, label)]
    render = wire.render_vk_constants_aiken if flavour == "aiken" else wire.render_vk_constants_plinth
    c = wire.parse_vk_constants(render(vk.constants()))
    c.check(vk.k)
    assert c.fixed_commitments == vk.fixed_commitments and c.permutation_commitments == vk.permutation_commitments
    if flavour == "aiken" and vk.recursion_vks is not None:    # (only the Aiken file carries the inner keys)
        assert c.recursion_vks == vk.recursion_vks
    base, _ = D.builder(name)()                                # the circuit shape with the file's constants is this key again
    back = base.with_constants(c)
    V.validate(back)
    if flavour == "plinth" and vk.recursion_vks is not None:
        back = replace(back, recursion_vks=vk.recursion_vks)
    assert back == vk
