"""GPU tests of h2v_check_pairs_multi (include/h2v.h): ONE batch check over pairs on several SRS - one decoding launch, one
coefficient launch, bucket MSMs of C + 1 problems, ONE pairing kernel of C + 1 Miller loops under one final exponentiation
(k_pairing_rlc_multi), the per-pair kernels of h2v_check_pairs behind its skip flags.  Three simple_mul keys on three SRS
(vk.on_srs); the pairs need no proofs: ([a]G1, [a s]G1) accepts under s and under nothing else.  Every expectation comes from
construction and from h2v_check_pairs per range on the same bytes; verdicts and status words are compared for equality."""
import json
import os
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import cancel, pairs_multi_model as M
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import PKG, ROOT
from tests.test_pairs_multi_srs import S_A, S_B, S_C, SEED

pytestmark = pytest.mark.gpu
INF = bls.g1_compress(None)
R = bls.R


class Key:
    def __init__(self, be, name, s, seed):
        from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
        self.name, self.s = name, s
        self.vk, self.td = V.on_srs(*V.simple_mul_vk(seed=seed), s)
        self.pl = PL.compile_plan(self.vk)
        self.dp = be.DevicePlan(self.pl.to_bytes(), 0)
        # 70 valid pairs (A_i, s A_i) by running additions; computed once, never changed
        a, d = bls.g1_mul(bls.G1_GEN, 1000 + seed), bls.g1_mul(bls.G1_GEN, 77)
        sa, sd = bls.g1_mul(a, s), bls.g1_mul(d, s)
        self.pts = []
        for _ in range(70):
            self.pts.append((a, sa))
            a, sa = bls.g1_add(a, d), bls.g1_add(sa, sd)
        self.pairs = [M.compress(p) for p in self.pts]


@pytest.fixture(scope="module")
def keys(be):
    ks = {"a": Key(be, "a", S_A, 1), "b": Key(be, "b", S_B, 2), "c": Key(be, "c", S_C, 3)}
    # the construction, held to the per-pair call: a pair accepts under its own SRS and under no other
    for x in "abc":
        for y in "abc":
            acc, st = ks[y].dp.check_pairs(ks[x].pairs[0] + ks[x].pairs[69])
            assert (list(acc), st) == (([1, 1], [0, 0]) if x == y else ([0, 0], [be.ST_PAIRING] * 2)), (x, y)
    return ks


def _call(keys, layout):
    """layout: [(key name, [pair bytes, ...]), ...] -> (plans, counts, raw)"""
    return [keys[k].dp for k, _ in layout], [len(ps) for _, ps in layout], b"".join(p for _, ps in layout for p in ps)


def _per_range(keys, layout):
    """(accept, status) of h2v_check_pairs, range by range, on the same bytes"""
    acc, st = [], []
    for k, ps in layout:
        if ps:
            a, s = keys[k].dp.check_pairs(b"".join(ps))
            acc += list(a)
            st += s
    return acc, st


def _multi(be, keys, layout, ws=None, seed=SEED):
    plans, counts, raw = _call(keys, layout)
    n = sum(counts)
    own = ws is None
    ws = ws or be.Workspace(plans[0], max(n, 1))
    acc, st, fell_back = be.check_pairs_multi(plans, counts, raw, ws=ws, seed=seed)
    ok, tm = ws.rlc_result()
    assert tm.msm_terms == n and tm.transcript_combiner_ms == 0 and bool(ok) == (not fell_back)
    if own:
        ws.close()
    return list(acc), st, fell_back


def _multi_device(be, keys, layout, ws, stream=None, seed=SEED):
    import torch
    dev = torch.device("cuda", 0)
    plans, counts, raw = _call(keys, layout)
    n = sum(counts)
    s = stream or torch.cuda.Stream(device=dev)
    pairs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    be.check_pairs_multi_device(plans, counts, pairs.data_ptr(), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream, seed=seed)
    ws.join(s.cuda_stream)
    s.synchronize()
    ok, tm = ws.rlc_result()
    assert tm.msm_terms == n
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()], not ok


ACCEPTING = {
    "3_2_1": lambda k: [("a", k["a"].pairs[:3]), ("b", k["b"].pairs[:2]), ("c", k["c"].pairs[:1])],
    "65_1": lambda k: [("a", k["a"].pairs[:65]), ("b", k["b"].pairs[:1])],                      # two coefficient blocks
    "1": lambda k: [("b", k["b"].pairs[4:5])],
    "0_2_0_1": lambda k: [("a", []), ("b", k["b"].pairs[:2]), ("c", []), ("a", k["a"].pairs[:1])],    # empty ranges
    "same_plan_twice": lambda k: [("a", k["a"].pairs[:2]), ("a", k["a"].pairs[2:4])],
    "16_ranges": lambda k: [("abc"[q % 3], k["abc"[q % 3]].pairs[q:q + 1]) for q in range(16)],
}


@pytest.mark.parametrize("shape", sorted(ACCEPTING))
def test_all_accepting_is_one_pass(be, keys, shape):
    layout = ACCEPTING[shape](keys)
    n = sum(len(ps) for _, ps in layout)
    for seed in (SEED, None):
        assert _multi(be, keys, layout, seed=seed) == ([1] * n, [0] * n, False), (shape, seed)
    assert _per_range(keys, layout) == ([1] * n, [0] * n)


def _not_in_g1():
    """a point on the curve outside the prime-order subgroup, compressed"""
    x = 5
    while True:
        y = bls.fp_sqrt((x * x * x + 4) % bls.P)
        if y is not None and not bls.g1_in_subgroup((x, y)):
            return bls.g1_compress((x, y))
        x += 1


def _rejecting_layout(keys, kind):
    """(3, 66, 2) pairs over a, b, c with one altered pair in the middle range; returns (layout, position, expected status, one pass)"""
    a, b, c = list(keys["a"].pairs[:3]), list(keys["b"].pairs[:66]), list(keys["c"].pairs[:2])
    if kind == "wrong_range":
        b[64] = keys["a"].pairs[10]                    # valid under s_a, checked against s_b
    elif kind == "wrong_r":
        l, r = keys["b"].pts[64]
        b[64] = bls.g1_compress(l) + bls.g1_compress(bls.g1_add(r, bls.G1_GEN))
    elif kind == "undecodable":
        b[64] = bytes(96)
    elif kind == "not_in_g1":
        b[64] = b[64][:48] + _not_in_g1()
    return [("a", a), ("b", b), ("c", c)], 3 + 64


@pytest.mark.parametrize("kind", ["wrong_range", "wrong_r", "undecodable", "not_in_g1"])
def test_rejects_match_the_per_range_check(be, keys, kind):
    layout, pos = _rejecting_layout(keys, kind)
    n = 71
    equation = kind in ("wrong_range", "wrong_r")
    want = ([0 if i == pos else 1 for i in range(n)], [(be.ST_PAIRING if equation else be.ST_BAD_POINT) if i == pos else 0 for i in range(n)])
    assert _per_range(keys, layout) == want
    # a failed equation falls back and only that pair is rejected; an undecodable pair has coefficient 0: one pass
    assert _multi(be, keys, layout) == want + (equation,)
    assert _multi(be, keys, layout, seed=None) == want + (equation,)


def _err_pair(key, j, err):
    l, r = key.pts[j]
    return bls.g1_compress(l) + bls.g1_compress(bls.g1_add(r, bls.g1_mul(bls.G1_GEN, err % R)))


def test_errors_do_not_cancel_across_srs(be, keys):
    """R = [a1 s_a + d]G1 in range a and R = [a2 s_b - d]G1 in range b - the errors cancel under equal coefficients (the model:
    tests/test_pairs_multi_srs.py) - are both rejected: on this call, with their places in their ranges changed, on a second call"""
    ka, kb = keys["a"], keys["b"]
    d = 0x1234567
    ea, eb = _err_pair(ka, 1, d), _err_pair(kb, 1, -d)
    for layout, bad in (([("a", [ka.pairs[0], ea]), ("b", [eb, kb.pairs[2]])], [1, 2]),
                        ([("a", [ea, ka.pairs[0]]), ("b", [kb.pairs[2], eb])], [0, 3])):
        want = ([0 if i in bad else 1 for i in range(4)], [be.ST_PAIRING if i in bad else 0 for i in range(4)])
        assert _per_range(keys, layout) == want
        for seed in (SEED, SEED, None):
            assert _multi(be, keys, layout, seed=seed) == want + (True,)


def test_coefficients_are_per_position_and_per_call(be, keys):
    """H2V_RLC_SEED_GIVEN: d split by the rule's own two coefficients of THIS call (tests/cancel.py's construction) passes the one
    check - which shows the coefficients are the documented ones, by position in the call - and is rejected by the next call."""
    from plutus_halo2_verifier_gen_amd import synth
    from tests.test_mixed_keys_gpu import LISTED
    assert LISTED.index("simple_mul") == 0
    ka, kb = keys["a"], keys["b"]
    fx = {"keys": {"simple_mul": {"vk": ka.vk, "td": ka.td, "pl": ka.pl, "dp": ka.dp}},
          "clean": {"simple_mul": synth.forge_batch(ka.vk, ka.td, 1, seed=5, plan=ka.pl, workers=1)}, "plans": [ka.dp]}
    lw = be.Workspace.multi([ka.dp], 64)
    c = cancel.learn_counter(be, fx, lw, SEED)
    lw.close()
    # the next seeded call mixes in c + 1; positions: range a holds 0, 1, 2 and range b holds 3, 4 - the altered pairs sit at 1 and 4
    rs = M.coefficients(SEED, c + 1, 5)
    da, db = M.cancelling_errors(rs[1], rs[4], 0x1234567)
    layout = [("a", [ka.pairs[0], _err_pair(ka, 1, da), ka.pairs[2]]), ("b", [kb.pairs[0], _err_pair(kb, 1, db)])]
    assert _multi(be, keys, layout) == ([1] * 5, [0] * 5, False)                    # the coefficients the rule documents: it passes
    want = ([1, 0, 1, 1, 0], [0, be.ST_PAIRING, 0, 0, be.ST_PAIRING])
    assert _multi(be, keys, layout) == want + (True,)                                # the next call: other coefficients
    assert _per_range(keys, layout) == want


def test_infinity(be, keys):
    ka, kb = keys["a"], keys["b"]
    inf2 = INF + INF
    # a range holding only (inf, inf) beside a live range
    layout = [("a", [inf2, inf2]), ("b", kb.pairs[:2])]
    assert _multi(be, keys, layout) == ([1] * 4, [0] * 4, False)
    assert _per_range(keys, layout) == ([1] * 4, [0] * 4)
    # every L_k at infinity with a finite R: rejected
    layout = [("a", [INF + ka.pairs[0][48:]]), ("b", [INF + kb.pairs[0][48:], inf2])]
    want = ([0, 0, 1], [be.ST_PAIRING, be.ST_PAIRING, 0])
    assert _per_range(keys, layout) == want
    assert _multi(be, keys, layout) == want + (True,)
    # a finite L against R at infinity
    layout = [("a", [ka.pairs[0][:48] + INF]), ("b", kb.pairs[:1])]
    want = ([0, 1], [be.ST_PAIRING, 0])
    assert _per_range(keys, layout) == want
    assert _multi(be, keys, layout) == want + (True,)
    # an all-infinite call passes
    layout = [("a", [inf2]), ("b", [inf2, inf2]), ("c", [inf2])]
    assert _multi(be, keys, layout) == ([1] * 4, [0] * 4, False)


def test_calling_forms(be, keys):
    import torch
    bad, pos = _rejecting_layout(keys, "wrong_range")
    good = ACCEPTING["3_2_1"](keys)
    want_bad = ([0 if i == pos else 1 for i in range(71)], [be.ST_PAIRING if i == pos else 0 for i in range(71)])
    dp = keys["a"].dp
    forms = {"ordinary": be.Workspace(dp, 128), "laned": be.Workspace(dp, 160, lanes=4, chunk=40)}
    for form, ws in forms.items():
        # back to back: a failing call, a clean one, a failing one - every verdict is the call's own
        assert _multi(be, keys, bad, ws=ws) == want_bad + (True,), form
        assert _multi(be, keys, good, ws=ws) == ([1] * 6, [0] * 6, False), form
        assert _multi_device(be, keys, bad, ws) == want_bad + (True,), form
        assert _multi_device(be, keys, good, ws) == ([1] * 6, [0] * 6, False), form
        with pytest.raises(be.H2VError):
            ws.timings()
        # the workspace still serves the calls it served before
        acc, st = dp.check_pairs(keys["a"].pairs[0] * 50, ws=ws)
        assert list(acc) == [1] * 50, form
        ws.close()
    # a deferring workspace: a stream of its own is required, and two calls enqueued back to back on it
    ws = be.Workspace(dp, 160, lanes=4, chunk=40)
    ws.defer_joins(True)
    plans, counts, raw = _call(keys, good)
    with pytest.raises(be.H2VError, match="needs a stream of its own"):
        be.check_pairs_multi_device(plans, counts, 1, 1, None, ws=ws, stream=None, seed=SEED)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert _multi_device(be, keys, bad, ws, stream=s) == want_bad + (True,)
    assert _multi_device(be, keys, good, ws, stream=s) == ([1] * 6, [0] * 6, False)
    ws.close()
    # the host form without a workspace: a temporary one
    plans, counts, raw = _call(keys, bad)
    acc, st, fb = be.check_pairs_multi(plans, counts, raw, seed=SEED)
    assert (list(acc), st, fb) == want_bad + (True,)


def test_one_plan_is_check_pairs_rlc(be, keys):
    """n_plans = 1: accept / status of h2v_check_pairs_rlc on the same bytes with the same given seed"""
    kb = keys["b"]
    pairs = list(kb.pairs[:66])
    pairs[7] = bytes(96)
    pairs[65] = keys["c"].pairs[0]
    for ps in (pairs, kb.pairs[:66]):
        raw = b"".join(ps)
        acc, st, fb = kb.dp.check_pairs_rlc(raw, seed=SEED)
        assert _multi(be, keys, [("b", ps)]) == (list(acc), st, fb)


# ---- the surface
@pytest.fixture(scope="module")
def proofs(be, orc, keys):
    """per key a and b: 9 accepting proofs and the same with proof 4 rejecting (only the pairing sees it), the oracle's verdicts"""
    from plutus_halo2_verifier_gen_amd import synth
    out = {}
    for name in "ab":
        k = keys[name]
        ov = orc.OracleVK(orc.vk_desc(json.loads(k.vk.to_json()), k.vk.omega, k.vk.omega_inv, k.vk.barycentric_weight))
        clean = synth.forge_batch(k.vk, k.td, 9, seed=7 + ord(name), plan=k.pl, workers=1)
        plist = [clean.proof(i) for i in range(9)]
        bad = list(plist)
        bad[4] = cancel.shift_pi(k.pl, plist[4], 5)
        inst = [clean.instance_ints(i, k.vk.n_public_inputs) for i in range(9)]
        raw = b"".join(bad)
        off = [0]
        for p in bad:
            off.append(off[-1] + len(p))
        assert list(ov.verify_batch(clean.proofs, clean.proof_off, clean.instances, clean.committed, threads=2)) == [1] * 9
        assert list(ov.verify_batch(raw, off, clean.instances, clean.committed, threads=2)) == [1, 1, 1, 1, 0, 1, 1, 1, 1]
        out[name] = {"clean": plist, "bad": bad, "inst": inst}
    return out


def test_aggregator_over_two_srs(be, keys, proofs, monkeypatch):
    from plutus_halo2_verifier_gen_amd import api
    pa, pb = (api.ParamsVerifierKZG(bytes.fromhex(keys[x].vk.s_g2)) for x in "ab")
    checks = []
    real = be.check_pairs_multi
    monkeypatch.setattr(be, "check_pairs_multi", lambda *a, **kw: checks.append(list(a[1])) or real(*a, **kw))
    agg = api.Aggregator([pa, pb])
    A, B = proofs["a"], proofs["b"]
    agg.push(keys["a"].vk, A["clean"][:5], A["inst"][:5])
    agg.push(keys["b"].vk, B["bad"][:6], B["inst"][:6])              # holds the rejecting proof (index 4)
    agg.push(keys["b"].vk, B["clean"][6:], B["inst"][6:])
    agg.push(keys["a"].vk, A["clean"][5:], A["inst"][5:])
    accepts, reverified = agg.finish()
    assert checks == [[2, 2]]                                         # ONE check: two pairs per SRS, sorted by SRS
    assert reverified == [1]
    assert accepts == [[True] * 5, [True, True, True, True, False, True], [True] * 3, [True] * 4]      # push order; the oracle's verdicts
    # one SRS among the pushes: exactly what it ran before - no multi-pairing
    agg.push(keys["a"].vk, A["clean"][:2], A["inst"][:2])
    agg.push(keys["a"].vk, A["clean"][2:4], A["inst"][2:4])
    assert agg.finish() == ([[True] * 2, [True] * 2], []) and len(checks) == 1


def test_verify_mixed_across_srs(be, keys, proofs, monkeypatch):
    from plutus_halo2_verifier_gen_amd import api
    checks = []
    real = be.check_pairs_multi
    monkeypatch.setattr(be, "check_pairs_multi", lambda *a, **kw: checks.append(list(a[1])) or real(*a, **kw))
    order = [("a", i) if q % 2 == 0 else ("b", i) for i in range(9) for q in range(2)]       # interleaved: 9 proofs per SRS
    vks = [keys[x].vk for x, _ in order]
    inst = [proofs[x]["inst"][i] for x, i in order]
    for tag in ("clean", "bad"):                                                                 # bad: proof 4 of SRS b rejects
        ps = [proofs[x][tag if x == "b" else "clean"][i] for x, i in order]
        want = [not (tag == "bad" and x == "b" and i == 4) for x, i in order]
        assert api.verify_mixed(vks, ps, inst, mode="rlc") == want                           # the default route: one call per SRS
        n_before = len(checks)
        assert api.verify_mixed(vks, ps, inst, mode="rlc", across_srs=True) == want
        assert api.verify_mixed(vks, ps, inst, mode="rlc", across_srs=True, fold_msm=True) == want
        assert checks[n_before:] == [[1, 1], [1, 1]]                                         # one check over the two pairs, each time
    pa, pb = (api.ParamsVerifierKZG(bytes.fromhex(keys[x].vk.s_g2)) for x in "ab")
    ps = [proofs[x]["clean"][i] for x, i in order]
    api.batch_verify([pa, pb], vks, [proofs[x]["inst"][i] for x, i in order], ps)
    with pytest.raises(api.VerifyError):
        api.batch_verify([pa, pb], vks, [proofs[x]["inst"][i] for x, i in order], [proofs[x]["bad"][i] for x, i in order])
    with pytest.raises(ValueError, match="s_g2 differs"):                                    # one SRS given: the error of today
        api.batch_verify(pa, vks, [proofs[x]["inst"][i] for x, i in order], ps)


def test_cpp_driver(be, keys, tmp_path):
    out = str(tmp_path / "h2v_pairs_multi_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_pairs_multi_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for name in "abc":
        path = str(tmp_path / ("%s.bin" % name))
        with open(path, "wb") as f:
            f.write(keys[name].pl.to_bytes())
        paths.append(path)
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    for tag, layout, fell_back in (("good", ACCEPTING["3_2_1"](keys), 0),
                                   ("bad", [("a", keys["a"].pairs[:2]), ("b", [keys["b"].pairs[0], keys["a"].pairs[5]]), ("c", [bytes(96)])], 1)):
        _plans, counts, raw = _call(keys, layout)
        want_acc, want_st = _per_range(keys, layout)
        with open(str(tmp_path / "pairs.bin"), "wb") as f:
            f.write(len(counts).to_bytes(4, "little") + b"".join(c.to_bytes(4, "little") for c in counts) + raw)
        r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / "pairs.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = dict(line.split(" ", 1) for line in r.stdout.splitlines())
        assert lines["multi"] == "".join(str(a) for a in want_acc), tag
        assert [int(v) for v in lines["status"].split()] == want_st, tag
        assert (lines["fell_back"], lines["per_range"], lines["workspace"]) == (str(fell_back), "1", "1"), (tag, r.stdout)
