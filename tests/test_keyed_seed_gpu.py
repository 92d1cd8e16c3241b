"""GPU tests of the derived seed of the mixed-key calls (H2V_RLC_SEED_KEYED, include/h2v.h; DESIGN.md section 17.1: form 3, keyed
leaves).  The digest kernels alone against the public model (plutus_halo2_verifier_gen_amd/seed.py) through h2v_probe_mixed_seed,
bit for bit; then every call that takes the flag: the pair of an aggregate call is the big-integer model's (tests/agg_model.py)
over each key's own h2v_prepare_batch pairs under the MODEL's seed, the same across forms, workspaces and plan orders; the verify
forms keep their contracts, fall back with the seed they derived, and reject cancelling errors; misuse is H2V_E_ARG; a call without
the flag is what it was.  On the code before the flag existed every test here ends in H2V_E_ARG or an AttributeError.
/root/reference is NOT needed."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import seed as S, synth
from tests import agg_model, keyed_seed_cases as K
from tests.test_aggregate_gpu import REJECTS
from tests.test_batch_cancellation_gpu import _Up, _pair, cx  # noqa: F401  (cx: keys on one SRS with eight clean proofs each)
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S
from tests.test_mixed_keys_gpu import _per_key_device

pytestmark = pytest.mark.gpu
GIVEN = bytes(range(70, 102))
E_ARG = "h2v error -1"
THREE = ("simple_mul", "lookup_table", "ivc")


# ---------------------------------------------------------------------------------------------- the digest kernels alone
def _probe(be, tags, c):
    return be.probe_mixed_seed(tags, c.shapes, c.plan_of, c.proofs, c.off, c.instances or None, c.committed or None)


def _model(tags, c):
    return S.mixed_seed_flat(tags, c.shapes, c.plan_of, c.proofs, c.off, c.instances, c.committed)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097])
def test_digest_kernels_at_every_tree_shape(be, n):
    """three plans (n_pi, n_ci) = (0, 0), (1, 1), (3, 0) interleaved i % 3 and a fourth listed without a proof: the committed index
    differs from the position, the instance offsets are no multiple of one row length; lengths 0 .. 256 around every block border"""
    tags = K.tags(4, "probe")
    c = K.case3(n)
    if n >= 63:
        assert {len(p) for p in c.proof} == set(K.LENS)
    assert _probe(be, tags, c) == _model(tags, c)


@pytest.mark.parametrize("first_off", [0, 3, 48])
def test_digest_kernels_alignments_empty_and_descending(be, first_off):
    tags = K.tags(4, "align")
    c = K.case3(70, first_off)
    assert c.off[0] == first_off and {len(p) for p in c.proof} == set(K.LENS)
    assert _probe(be, tags, c) == _model(tags, c)
    # the plans listed in another order: the same seed from the kernels too
    order = [3, 1, 0, 2]
    new_of = {old: new for new, old in enumerate(order)}
    got = be.probe_mixed_seed([tags[o] for o in order], [c.shapes[o] for o in order], [new_of[k] for k in c.plan_of], c.proofs, c.off,
                              c.instances, c.committed)
    assert got == _model(tags, c)
    # every proof empty
    e = K.case3(70, first_off, lens=[0] * 70)
    assert e.off == [first_off] * 71
    assert _probe(be, tags, e) == _model(tags, e)
    # a descending pair of offsets is an empty proof: proof 3 "ends" in front of its start, proof 4 starts there
    d = K.case3(10, first_off, lens=[130, 5, 64, 0, 77, 1, 128, 200, 3, 65])
    d.off[4] = d.off[3] - 40
    want = S.mixed_seed_flat(tags, d.shapes, d.plan_of, d.proofs, d.off, d.instances, d.committed)
    proof = [d.proofs[d.off[i]:d.off[i + 1]] if d.off[i + 1] > d.off[i] else b"" for i in range(10)]
    assert proof[3] == b"" and len(proof[4]) == 77 + 40 and want == S.mixed_seed(tags, d.plan_of, d.inst, d.ci, proof)
    assert be.probe_mixed_seed(tags, d.shapes, d.plan_of, d.proofs, d.off, d.instances, d.committed) == want


# ---------------------------------------------------------------------------------------------- the calls
class KMix:
    """a mixed batch over an explicit list of plans: entries = [(plan index, proof, instance bytes, committed bytes or b"")]"""

    def __init__(self, infos, entries):
        self.infos, self.entries = list(infos), list(entries)
        self.plans = [i["dp"] for i in self.infos]
        self.plan_of = [e[0] for e in self.entries]
        self.n = len(self.entries)
        self.off = [0]
        for e in self.entries:
            self.off.append(self.off[-1] + len(e[1]))
        self.proofs = b"".join(e[1] for e in self.entries)
        self.instances = b"".join(e[2] for e in self.entries)
        self.committed = b"".join(e[3] for e in self.entries) or None

    def args(self):
        return self.plans, self.plan_of, self.proofs, self.off, self.instances, self.committed

    def seed(self):
        return S.mixed_seed([i["dp"].key_tag for i in self.infos], self.plan_of, [e[2] for e in self.entries], [e[3] for e in self.entries],
                            [e[1] for e in self.entries])

    def per_key(self):
        """every plan's own sub-batch of the call and the positions its proofs have"""
        for k, info in enumerate(self.infos):
            pos = [i for i, e in enumerate(self.entries) if e[0] == k]
            if not pos:
                continue
            off = [0]
            for i in pos:
                off.append(off[-1] + len(self.entries[i][1]))
            yield info, pos, synth.Batch(n=len(pos), proofs=b"".join(self.entries[i][1] for i in pos), proof_off=off,
                                         instances=b"".join(self.entries[i][2] for i in pos),
                                         committed=b"".join(self.entries[i][3] for i in pos) or None, expected=None)

    def prepared(self):
        """(pairs, reached, status) in the caller's order from each key's own h2v_prepare_batch"""
        pairs, st = [None] * self.n, [None] * self.n
        for info, pos, b in self.per_key():
            raw, s = info["dp"].prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
            for q, i in enumerate(pos):
                pairs[i], st[i] = raw[96 * q:96 * q + 96], s[q]
        return pairs, [int(s == 0) for s in st], st

    def verdicts(self):
        """(accept, status) in the caller's order from each key's own h2v_verify_batch_device"""
        acc, st = [None] * self.n, [None] * self.n
        for info, pos, b in self.per_key():
            a, s = _per_key_device(info["dp"], b)
            for q, i in enumerate(pos):
                acc[i], st[i] = a[q], s[q]
        return acc, st


def _info(e):
    return {"dp": e["dp"], "pl": e["pl"], "n_pi": e["vk"].n_public_inputs}


def _entry(cx, infos, name, j, names=THREE):
    b, n_pi = cx["clean"][name], cx["keys"][name]["vk"].n_public_inputs
    return (names.index(name), b.proof(j), b.instances[32 * n_pi * j:32 * n_pi * (j + 1)], b.ci(j) if b.committed is not None else b"")


@pytest.fixture(scope="module")
def kx(be, cx):
    """three keys on one SRS - simple_mul, lookup_table, the recursive key - as the cancellation tests build them, and a second
    simple_mul key of another builder seed (the same shape: a proof can be handed to the other key's tag)"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    infos = [_info(cx["keys"][name]) for name in THREE]
    for i in infos:
        assert i["dp"].key_tag == S.key_tag(i["pl"].to_bytes())
    vk, td = V.on_srs(*V.simple_mul_vk(seed=0x6b01), COMMON_S)
    pl = PL.compile_plan(vk)
    twin = {"dp": be.DevicePlan(pl.to_bytes(), 0), "pl": pl, "n_pi": vk.n_public_inputs,
            "clean": synth.forge_batch(vk, td, 4, seed=77, plan=pl, workers=1)}
    assert vk.n_public_inputs == 3
    assert twin["dp"].key_tag != infos[0]["dp"].key_tag and twin["pl"].proof_len == infos[0]["pl"].proof_len
    return {"infos": infos, "twin": twin}


def _interleaved(cx, kx, n):
    return KMix(kx["infos"], [_entry(cx, kx["infos"], THREE[i % 3], (i // 3) % 8) for i in range(n)])


def _agg_host(be, mix, ws, grouped, **kw):
    pair, inc, st, info = be.aggregate_mixed(*mix.args(), ws=ws, grouped=grouped, **kw)
    return pair, list(inc), st, info


def _agg_device(be, mix, ws, grouped, **kw):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    keep = [t(mix.proofs), torch.tensor(mix.off, dtype=torch.int64, device=dev), t(mix.instances), t(mix.committed)]
    pair = torch.full((96,), 7, dtype=torch.uint8, device=dev)
    inc = torch.full((mix.n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((mix.n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    torch.cuda.synchronize()
    info = be.aggregate_mixed_device(mix.plans, mix.plan_of, mix.n, *[ptr(x) for x in keep], pair.data_ptr(), inc.data_ptr(), st.data_ptr(), ws=ws,
                                     stream=s.cuda_stream, grouped=grouped, **kw)
    s.synchronize()
    return bytes(pair.cpu().numpy().tobytes()), inc.cpu().tolist(), [v & 0xffffffff for v in st.cpu().tolist()], info


def _laned(be, mix, cap):
    """a multi-plan workspace that cuts the call into several chunks (no ordinary workspace fits three keys of three shapes: the
    ordinary workspace has its own test over two keys of one shape, test_a_position_under_another_keys_tag)"""
    ws = be.Workspace.multi(mix.plans, cap, lanes=3, chunk=max(2, cap // 4))
    assert ws.lanes() == (3, max(2, cap // 4))
    return ws


@pytest.mark.parametrize("n", [1, 6, 65])
def test_aggregate_pair_is_the_models(be, cx, kx, n):
    mix = _interleaved(cx, kx, n)
    pairs_i, reached, pst = mix.prepared()
    assert reached == [1] * n
    want_seed = mix.seed()
    assert want_seed == S.mixed_seed_flat([i["dp"].key_tag for i in mix.infos], [(i["n_pi"], i["dp"].n_ci) for i in mix.infos], mix.plan_of, mix.proofs,
                                          mix.off, mix.instances, mix.committed or b"")
    want = agg_model.model_pair(pairs_i, reached, want_seed, 0)
    assert agg_model.holds(want, COMMON_S)
    cap = max(n, 8)
    plain, multi = _laned(be, mix, cap), be.Workspace.multi(mix.plans, cap)
    assert multi.lanes()[1] >= cap                                  # (one chunk holds the call)
    got = []
    for grouped in (False, True):
        for ws in (plain, multi, None):
            pair, inc, st, info = _agg_host(be, mix, ws, grouped, keyed_seed=True)
            assert (info.seed_source, bytes(info.seed_used), info.chunk, info.n_chunks) == (1, want_seed, 0, 1), (grouped, ws)
            assert (inc, st) == (reached, pst)
            if ws is not None:
                assert ws.seed_used() == want_seed and ws.rlc_verdict() == be.BATCH_NOT_CHECKED and ws.seed_ms() > 0
            got.append(pair)
        for ws in (plain, multi):                 # the device form: the info has no seed yet, the getter has
            pair, inc, st, info = _agg_device(be, mix, ws, grouped, keyed_seed=True)
            assert (info.seed_source, bytes(info.seed_used)) == (1, bytes(32))
            assert (inc, st) == (reached, pst) and ws.seed_used() == want_seed
            got.append(pair)
    assert got == [want] * 10, n
    # the plans listed in another order (and one more listed without a proof): the same seed, the same pair
    order = [2, 0, 1]
    new_of = {old: new for new, old in enumerate(order)}
    relisted = KMix([mix.infos[o] for o in order] + [kx["twin"]], [(new_of[e[0]],) + e[1:] for e in mix.entries])
    assert relisted.seed() == want_seed and relisted.plan_of != mix.plan_of
    wide = be.Workspace.multi(relisted.plans, cap)
    pair, _inc, _st, info = _agg_host(be, relisted, wide, False, keyed_seed=True)
    assert (pair, bytes(info.seed_used)) == (want, want_seed)
    wide.close()
    # a changed instance byte: another seed, another pair - the model's over what h2v_prepare_batch says of the changed batch
    k = n // 2
    e = mix.entries[k]
    assert e[2]
    changed = KMix(mix.infos, mix.entries[:k] + [(e[0], e[1], bytes([e[2][0] ^ 1]) + e[2][1:], e[3])] + mix.entries[k + 1:])
    pair2, inc2, _st2, info2 = _agg_host(be, changed, multi, False, keyed_seed=True)
    p2, r2, _s2 = changed.prepared()
    assert bytes(info2.seed_used) == changed.seed() != want_seed and pair2 != want
    assert inc2 == r2 and pair2 == agg_model.model_pair(p2, r2, changed.seed(), 0)
    # no flag: a given seed still gives the model's pair, as before
    pair3, inc3, _st3, info3 = _agg_host(be, mix, multi, False, seed=GIVEN)
    assert info3.seed_source == 0 and inc3 == reached and pair3 == agg_model.model_pair(pairs_i, reached, bytes(info3.seed_used), 0)
    with pytest.raises(be.H2VError, match=E_ARG):                  # ... and the getter has nothing for it
        multi.seed_used()
    plain.close()
    multi.close()


def test_a_position_under_another_keys_tag(be, cx, kx):
    """two keys of one shape: the same bytes with ONE proof handed to the other key - another seed and another pair, both the
    model's (the proof does not verify under the other key, but it reaches the pairing and is included).  Two keys of one shape also
    fit an ORDINARY workspace (no lanes: sub-batches and tail one after the other on one stream): every form there, aggregate and
    verify, with the fall-back of the fold forms."""
    infos = [kx["infos"][0], kx["twin"]]
    ent = [_entry(cx, infos, "simple_mul", j) for j in range(6)]
    a = KMix(infos, ent)
    b = KMix(infos, ent[:2] + [(1,) + ent[2][1:]] + ent[3:])
    assert a.proofs == b.proofs and a.instances == b.instances and a.plan_of != b.plan_of and a.seed() != b.seed()
    ws = be.Workspace.multi(a.plans, 8)
    out = []
    for m in (a, b):
        pairs_i, reached, _st = m.prepared()
        pair, inc, _s, info = _agg_host(be, m, ws, False, keyed_seed=True)
        assert bytes(info.seed_used) == m.seed() == ws.seed_used() and inc == reached == [1] * 6
        assert pair == agg_model.model_pair(pairs_i, reached, m.seed(), 0)
        out.append(pair)
    assert out[0] != out[1] and agg_model.holds(out[0], COMMON_S) and not agg_model.holds(out[1], COMMON_S)
    ws.close()
    for n in (1, 6, 65):
        tb = kx["twin"]["clean"]                                    # the two keys in turn, each with proofs of its own
        good = KMix(infos, [ent[(i // 2) % 6] if i % 2 == 0 else (1, tb.proof((i // 2) % 4), tb.instances[96 * ((i // 2) % 4):96 * ((i // 2) % 4) + 96], b"")
                            for i in range(n)])
        plain = be.Workspace(infos[0]["dp"], max(n, 8))
        assert plain.lanes() == (1, max(n, 8))
        for m in (good, KMix(infos, [(1,) + good.entries[0][1:]] + good.entries[1:])):
            pairs_i, reached, pst = m.prepared()
            want = agg_model.model_pair(pairs_i, reached, m.seed(), 0)
            for grouped in (False, True):
                pair, inc, st, info = _agg_host(be, m, plain, grouped, keyed_seed=True)
                assert (pair, inc, st, info.seed_source, bytes(info.seed_used)) == (want, reached, pst, 1, m.seed()), (n, grouped)
                assert plain.seed_used() == m.seed() and plain.seed_ms() > 0
                pair, inc, st, info = _agg_device(be, m, plain, grouped, keyed_seed=True)
                assert (pair, inc, st, bytes(info.seed_used)) == (want, reached, pst, bytes(32)) and plain.seed_used() == m.seed()
            want_acc, want_st = m.verdicts()
            want_fb = any(s == be.ST_PAIRING for s in want_st)
            assert want_fb == (m is not good)
            for fold, grouped in FORMS:
                assert _verify_host(be, m, plain, fold, grouped, keyed_seed=True) == (want_acc, want_st, want_fb), (n, fold, grouped)
                assert plain.seed_used() == m.seed() and plain.rlc_result(timings=False)[0] == (not want_fb) and plain.seed_ms() > 0
                assert _verify_device(be, m, plain, fold, grouped, keyed_seed=True) == (want_acc, want_st) and plain.seed_used() == m.seed()
        plain.close()


def _verify_host(be, mix, ws, fold, grouped, **kw):
    acc, st, fb = be.verify_mixed(*mix.args(), ws=ws, mode="rlc", fold_msm=fold, grouped=grouped, **kw)
    return list(acc), st, fb


def _verify_device(be, mix, ws, fold, grouped, **kw):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    keep = [t(mix.proofs), torch.tensor(mix.off, dtype=torch.int64, device=dev), t(mix.instances), t(mix.committed)]
    acc = torch.full((mix.n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((mix.n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    torch.cuda.synchronize()
    be.verify_mixed_device(mix.plans, mix.plan_of, mix.n, *[ptr(x) for x in keep], acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream,
                           mode="rlc", fold_msm=fold, grouped=grouped, **kw)
    s.synchronize()
    return acc.cpu().tolist(), [v & 0xffffffff for v in st.cpu().tolist()]


FORMS = [(False, False), (True, False), (True, True)]


def _with_rejects(mix, kinds):
    """the mix with proof positions[i] corrupted as kinds say, spread over the keys"""
    ent = list(mix.entries)
    for q, kind in enumerate(kinds):
        i = 4 + 7 * q + q % 3                                   # 4, 12, 20, 25, 33, 41: plans 1, 0, 2, 1, 0, 2
        k, proof, inst, ci = ent[i]
        proof, inst = synth.corrupt(mix.infos[k]["pl"], proof, inst, kind, random.Random(2000 + i))
        ent[i] = (k, bytes(proof), bytes(inst), ci)
    return KMix(mix.infos, ent)


def test_verify_forms(be, cx, kx):
    """H2V_MIXED_RLC alone, with _FOLD_MSM, with _FOLD_MSM | _GROUPED: accept / status are the per-key calls', fell_back as expected,
    and after a fall-back the getter still has the model's seed (derived once, the second pass copies it)"""
    clean = _interleaved(cx, kx, 48)
    kinds = sorted(set(REJECTS.values()))
    rej = _with_rejects(clean, kinds)
    assert sorted({e[0] for e, c in zip(rej.entries, clean.entries) if e != c}) == [0, 1, 2] and len(kinds) == 6
    multi = be.Workspace.multi(clean.plans, 48)
    plain = _laned(be, clean, 48)
    for mix, tag in ((clean, "clean"), (rej, "rej")):
        want_acc, want_st = mix.verdicts()
        want_fb = any(s == be.ST_PAIRING for s in want_st)
        assert (tag == "clean") == (want_acc == [1] * 48) and want_fb == (tag == "rej")
        for fold, grouped in FORMS:
            for ws in (multi, plain):
                acc, st, fb = _verify_host(be, mix, ws, fold, grouped, keyed_seed=True)
                assert (acc, st, fb) == (want_acc, want_st, want_fb), (tag, fold, grouped)
                assert ws.seed_used() == mix.seed() and ws.rlc_result(timings=False)[0] == (not want_fb) and ws.seed_ms() > 0
                assert _verify_device(be, mix, ws, fold, grouped, keyed_seed=True) == (want_acc, want_st)
                assert ws.seed_used() == mix.seed()
            acc, st, fb = _verify_host(be, mix, None, fold, grouped, keyed_seed=True)          # a temporary workspace
            assert (acc, st, fb) == (want_acc, want_st, want_fb)
    multi.close()
    plain.close()


def _put(cx, mix, at, ka, kb, names=THREE):
    """the mix with the cancelling pair (A', B') made from proofs ka, kb = (key, index) at positions `at`"""
    pa, pb = _pair(cx, ka, kb)
    ent = list(mix.entries)
    for i, (name, j), p in ((at[0], ka, pa), (at[1], kb, pb)):
        e = _entry(cx, mix.infos, name, j, names)
        ent[i] = (e[0], p, e[2], e[3])
    return KMix(mix.infos, ent)


def test_laned_tail_chunks_and_cancelling_errors(be, cx, kx):
    """chunk 64 x 3 lanes, n = 130.  The non-fold tail is cut into chunks, each a batch check of its own under the call's ONE seed
    tweaked per chunk: a pairing-only reject in chunk 1 leaves the other chunks' proofs accepted.  Two rejecting proofs of two
    DIFFERENT keys whose errors cancel under equal weights are both rejected, within one chunk and across two, in every form."""
    clean = _interleaved(cx, kx, 130)
    laned = be.Workspace.multi(clean.plans, 130, lanes=3, chunk=64)
    assert laned.lanes() == (3, 64)
    ent = list(clean.entries)
    k, proof, inst, ci = ent[70]
    proof, inst = synth.corrupt(clean.infos[k]["pl"], proof, inst, "wrong_pi", random.Random(5))
    one = KMix(clean.infos, ent[:70] + [(k, bytes(proof), bytes(inst), ci)] + ent[71:])
    want_acc, want_st = [int(i != 70) for i in range(130)], [be.ST_PAIRING if i == 70 else 0 for i in range(130)]
    for fold, grouped in FORMS:
        assert _verify_host(be, one, laned, fold, grouped, keyed_seed=True) == (want_acc, want_st, True), (fold, grouped)
        assert laned.seed_used() == one.seed()
        assert _verify_host(be, clean, laned, fold, grouped, keyed_seed=True) == ([1] * 130, [0] * 130, False)
        assert laned.seed_used() == clean.seed() != one.seed()
    for a, b in ((3, 4), (6, 70)):                                  # simple_mul at a (a % 3 == 0), lookup_table at b (b % 3 == 1)
        assert a % 3 == 0 and b % 3 == 1
        bad = _put(cx, clean, (a, b), ("simple_mul", 0), ("lookup_table", 0))
        want_acc, want_st = [int(i not in (a, b)) for i in range(130)], [be.ST_PAIRING if i in (a, b) else 0 for i in range(130)]
        for fold, grouped in FORMS:
            assert _verify_host(be, bad, laned, fold, grouped, keyed_seed=True) == (want_acc, want_st, True), (a, b, fold, grouped)
            assert _verify_device(be, bad, laned, fold, grouped, keyed_seed=True) == (want_acc, want_st)
            assert laned.seed_used() == bad.seed()
    laned.close()


def test_seventy_keys_wrap_the_record_ring(be, cx):
    """70 keys x 1 proof, grouped: the first pass takes two records, the second - after one forced reject - 71, more than the
    64-slot ring holds.  The verdicts are right and the getter answers for the call's last record with the seed derived ONCE."""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    infos, ent = [], []
    for k in range(70):
        vk, td = V.on_srs(*V.simple_mul_vk(seed=0x6c00 + k), COMMON_S)
        pl = PL.compile_plan(vk)
        infos.append({"dp": be.DevicePlan(pl.to_bytes(), 0), "pl": pl, "n_pi": vk.n_public_inputs})
        b = synth.forge_batch(vk, td, 1, seed=900 + k, plan=pl, workers=1)
        ent.append((k, b.proof(0), b.instances, b""))
    clean = KMix(infos, ent)
    k, proof, inst, ci = ent[37]
    proof, inst = synth.corrupt(infos[k]["pl"], proof, inst, "wrong_pi", random.Random(9))
    bad = KMix(infos, ent[:37] + [(k, bytes(proof), bytes(inst), ci)] + ent[38:])
    ws = be.Workspace.multi(clean.plans, 70, lanes=4, chunk=40)
    assert _verify_host(be, clean, ws, True, True, keyed_seed=True) == ([1] * 70, [0] * 70, False)
    assert ws.seed_used() == clean.seed()
    want_acc, want_st = [int(i != 37) for i in range(70)], [be.ST_PAIRING if i == 37 else 0 for i in range(70)]
    for _ in range(2):
        assert _verify_host(be, bad, ws, True, True, keyed_seed=True) == (want_acc, want_st, True)
        assert ws.seed_used() == bad.seed() != clean.seed() and ws.seed_ms() > 0
        assert not ws.rlc_result(timings=False)[0]
    assert _verify_device(be, bad, ws, True, True, keyed_seed=True) == (want_acc, want_st) and ws.seed_used() == bad.seed()
    pair, inc, _st, info = _agg_host(be, clean, ws, True, keyed_seed=True)
    assert bytes(info.seed_used) == clean.seed() and inc == [1] * 70 and agg_model.holds(pair, COMMON_S)
    ws.close()


def test_misuse(be, cx, kx):
    mix = _interleaved(cx, kx, 6)
    ws = be.Workspace.multi(mix.plans, 8)
    with pytest.raises(be.H2VError, match="H2V_MIXED_RLC"):         # a mixed call without coefficients
        be.verify_mixed(*mix.args(), ws=ws, mode="per-proof", keyed_seed=True)
    with pytest.raises(be.H2VError, match="exclude each other"):
        be.verify_mixed(*mix.args(), ws=ws, mode="rlc", seed=GIVEN, keyed_seed=True)
    with pytest.raises(be.H2VError, match="exclude each other"):
        be.aggregate_mixed(*mix.args(), ws=ws, seed=GIVEN, keyed_seed=True)
    # flag 64 in each single-key entry point
    import ctypes as C
    e = cx["keys"]["simple_mul"]
    dp, b = e["dp"], cx["clean"]["simple_mul"]
    one = be.Workspace(dp, 8)
    L = be.lib()
    flag = be.RlcOpts((C.c_uint8 * 32)(), be.RLC_SEED_KEYED)
    off = (C.c_uint64 * (b.n + 1))(*b.proof_off)
    pbuf, ibuf = C.create_string_buffer(b.proofs, len(b.proofs)), C.create_string_buffer(b.instances, len(b.instances))
    hb = be.Batch(b.n, C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p), C.cast(ibuf, C.c_void_p), None)
    acc, st, pair = (C.c_uint8 * b.n)(), (C.c_uint32 * b.n)(), C.create_string_buffer(96 * b.n)
    up = _Up(b)
    db = be.Batch(*up.args[:5])
    calls = [lambda: L.h2v_verify_batch_rlc(dp.handle, C.byref(hb), acc, one.handle, C.byref(flag), None),
             lambda: L.h2v_verify_batch_rlc_device(dp.handle, C.byref(db), up.args[5], up.args[6], one.handle, up.stream.cuda_stream, C.byref(flag)),
             lambda: L.h2v_check_pairs_rlc(dp.handle, b.n, pair, acc, st, one.handle, C.byref(flag), None),
             lambda: L.h2v_check_pairs_rlc_device(dp.handle, b.n, up.args[1], up.args[5], up.args[6], one.handle, up.stream.cuda_stream, C.byref(flag)),
             lambda: L.h2v_aggregate_batch(dp.handle, C.byref(hb), pair, acc, st, one.handle, C.byref(flag), None),
             lambda: L.h2v_aggregate_batch_device(dp.handle, C.byref(db), up.args[1], up.args[5], up.args[6], one.handle, up.stream.cuda_stream,
                                                  C.byref(flag), None)]
    for q, call in enumerate(calls):
        assert call() == -1, q
        assert "H2V_RLC_SEED_KEYED" in L.h2v_last_error().decode(), (q, L.h2v_last_error().decode())
    up.results()
    # the getter after a mixed call made without the flag
    be.verify_mixed(*mix.args(), ws=ws, mode="rlc", seed=GIVEN, fold_msm=True)
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used()
    # ... after all of which the workspaces are still usable
    acc2, _st2, fb = be.verify_mixed(*mix.args(), ws=ws, mode="rlc", fold_msm=True, keyed_seed=True)
    assert (list(acc2), fb) == ([1] * 6, False) and ws.seed_used() == mix.seed()
    with pytest.raises(be.H2VError, match=E_ARG):                   # one call back: the call with a given seed
        ws.seed_used(1)
    ws.close()
    one.close()


def test_aggregator_follows_one_rule(be, cx, kx):
    """api.Aggregator(keyed_seed=True): a single-key push goes out as a one-plan mixed call, push_mixed derives; one check over both"""
    from plutus_halo2_verifier_gen_amd import api
    e = cx["keys"]["simple_mul"]
    b = cx["clean"]["simple_mul"]
    agg = api.Aggregator(api.ParamsVerifierKZG(bytes.fromhex(e["vk"].s_g2)), keyed_seed=True)
    proofs, insts = [b.proof(i) for i in range(4)], [b.instance_ints(i, 3) for i in range(4)]
    agg.push(e["vk"], proofs, insts)
    lt, lb = cx["keys"]["lookup_table"], cx["clean"]["lookup_table"]
    n_pi = lt["vk"].n_public_inputs
    agg.push_mixed([e["vk"], lt["vk"], e["vk"]], [b.proof(4), lb.proof(0), b.proof(5)], [b.instance_ints(4, 3), lb.instance_ints(0, n_pi), b.instance_ints(5, 3)],
                   [None, lb.ci(0) if lb.committed is not None else None, None])
    one = KMix([_info(e)], [(0, proofs[i], b.instances[96 * i:96 * i + 96], b"") for i in range(4)])
    want = agg_model.model_pair(one.prepared()[0], [1] * 4, one.seed(), 0)
    assert agg._calls[0][1] == want
    accepts, reverified = agg.finish()
    assert accepts == [[True] * 4, [True] * 3] and reverified == []
