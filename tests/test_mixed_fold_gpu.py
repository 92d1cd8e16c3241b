"""GPU tests of the fold form of the mixed-key call (H2V_MIXED_FOLD_MSM: ONE bucket MSM over the per-proof terms of every key of
the call and ONE pairing; after a failed check the H2V_MIXED_RLC path on the same inputs).  The fixture is that of
tests/test_mixed_keys_gpu.py - simple_mul / lookup_table / trashcan_mix / ivc on one SRS with 70 / 65 / 9 / 1 proofs,
atms_with_lookups listed without one, shuffled: 145 proofs, which cross a 64-lane wave and a 64-proof block, hold a one-proof key
and a key without the batch form (ivc), and on 4 lanes x 40 run in chunks that are no multiples of 64.  Expectations come from
the CPU oracle, from construction, from the per-key h2v_verify_batch_device status words and, for the sums, from the big-integer
model (bls12_381.py) - never from the call under test."""
import os
import random
import struct
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, synth
from tests.cancel import coeff as _coeff
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S, MIXED_KEYS, PKG, ROOT
from tests.test_mixed_keys_gpu import LISTED, SEED, Mix, _DeviceCall, _interleaved, _per_key_device, _want_status, fx  # noqa: F401

pytestmark = pytest.mark.gpu
FOLDABLE = ("simple_mul", "lookup_table", "trashcan_mix")          # the keys with the batch form; ivc joins as one pair per proof
PRE_PAIRING = ["noncanonical_scalar", "point_not_on_curve", "point_not_in_subgroup", "bad_point_flag", "truncated"]


def _host(be, fx, mix, ws=None, plans=None, seed=SEED, fold=True):
    acc, st, fb = be.verify_mixed(plans or fx["plans"], mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, mode="rlc",
                                  seed=seed, fold_msm=fold)
    return list(acc), st, fb


class _FoldCall(_DeviceCall):
    """a device-form call with the flag set"""

    def launch(self):
        be, plans, plan_of, _mode, ws = self.args
        ptr = lambda x: x.data_ptr() if x is not None else None
        be.verify_mixed_device(plans, plan_of, self.n, *[ptr(x) for x in self.keep], self.acc.data_ptr(), self.st.data_ptr(), ws=ws,
                               stream=self.stream.cuda_stream if self.stream is not None else None, mode="rlc", seed=SEED, fold_msm=True)


def _device(be, fx, mix, ws):
    import torch
    return _FoldCall(be, fx, mix, "rlc", ws, torch.cuda.Stream(device=torch.device("cuda", 0))).results()


def _with_one_reject(fx, name, j, kind="wrong_pi", seed=7):
    """the clean batch of key `name` with proof j replaced by a variant that only the pairing rejects; checked with the oracle"""
    b, e = fx["clean"][name], fx["keys"][name]
    n_pi = e["vk"].n_public_inputs
    p, _ins = synth.corrupt(e["pl"], b.proof(j), b.instances[32 * n_pi * j:32 * n_pi * (j + 1)], kind, random.Random(seed))
    proofs = [b.proof(i) if i != j else p for i in range(b.n)]
    off = [0]
    for q in proofs:
        off.append(off[-1] + len(q))
    bad = synth.Batch(n=b.n, proofs=b"".join(proofs), proof_off=off, instances=b.instances, committed=b.committed,
                      expected=[int(i != j) for i in range(b.n)])
    assert list(e["ov"].verify_batch(bad.proofs, bad.proof_off, bad.instances, bad.committed, threads=2)) == bad.expected
    return bad


# ---- 1
def test_all_accepting_batch_is_one_msm_and_one_pairing(be, fx):
    mix = fx["mix_clean"]
    ws = be.Workspace.multi(fx["plans"], mix.n)
    acc, st, fb = _host(be, fx, mix, ws)
    assert acc == [1] * mix.n and st == [0] * mix.n and not fb
    ok, tm = ws.rlc_result()
    assert ok and tm.transcript_combiner_ms == 0
    # the term count: what a per-key h2v_verify_batch_rlc call on each key's batch alone sums, plus one pair per ivc proof
    want_terms = fx["clean"]["ivc"].n
    for name in FOLDABLE:
        b, dp = fx["clean"][name], fx["keys"][name]["dp"]
        kws = be.Workspace(dp, b.n)
        got, _fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=kws, seed=SEED)
        assert list(got) == b.expected
        want_terms += kws.rlc_result()[1].msm_terms
        kws.close()
    assert tm.msm_terms == want_terms and want_terms > mix.n
    # the device form on the same workspace, and the call without the flag after it: unchanged (msm_terms = the pairs)
    assert _device(be, fx, mix, ws) == ([1] * mix.n, [0] * mix.n)
    assert ws.rlc_result()[1].msm_terms == want_terms
    assert _host(be, fx, mix, ws, fold=False) == ([1] * mix.n, [0] * mix.n, False)
    assert ws.rlc_result()[1].msm_terms == mix.n
    ws.close()


# ---- 2
@pytest.mark.parametrize("kind", ["none", "plain", "laned", "deferring"])
def test_rejects_of_every_kind_through_every_workspace(be, fx, kind):
    mix = fx["mix"]
    want_st = _want_status(fx, "rejects", mix)
    want_fb = any(s == be.ST_PAIRING for s in want_st)
    assert 0 < sum(mix.expected) < mix.n and want_fb
    if kind == "none":
        assert _host(be, fx, mix, None) == (mix.expected, want_st, want_fb)
        return
    ws = be.Workspace.multi(fx["plans"], mix.n) if kind == "plain" else be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)
    if kind != "plain":
        assert ws.lanes() == (4, 40)
    if kind == "deferring":
        ws.defer_joins(True)
    assert _host(be, fx, mix, ws) == (mix.expected, want_st, want_fb)
    assert ws.rlc_result(timings=False)[0] == (not want_fb)
    assert _device(be, fx, mix, ws) == (mix.expected, want_st)
    assert ws.rlc_result(timings=False)[0] == (not want_fb)
    ws.close()


# ---- 3
def test_only_pre_pairing_rejects_do_not_fall_back(be, fx):
    keys = fx["keys"]
    batches, want = {}, {}
    for k, name in enumerate(MIXED_KEYS):
        e = keys[name]
        batches[name] = synth.with_rejects(e["pl"], fx["clean"][name], e["vk"].n_public_inputs, fraction=0.3, seed=71 + k, kinds=PRE_PAIRING)
        b = batches[name]
        assert list(e["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4)) == b.expected
        acc, want[name] = _per_key_device(e["dp"], b)
        assert acc == b.expected
    mix = Mix(keys, batches, _interleaved(batches, 72))
    want_st = [want[name][j] for name, j in mix.order]
    assert 0 < sum(mix.expected) < mix.n and all(s != be.ST_PAIRING for s in want_st)
    assert {bool(s & be.ST_BAD_SCALAR) for s in want_st} == {bool(s & be.ST_BAD_POINT) for s in want_st} == {True, False}
    for ws in (be.Workspace.multi(fx["plans"], mix.n), be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)):
        assert _host(be, fx, mix, ws) == (mix.expected, want_st, False)
        ok, tm = ws.rlc_result()
        assert ok and tm.msm_terms > mix.n
        assert _device(be, fx, mix, ws) == (mix.expected, want_st)
        ws.close()


# ---- 4
def _model_l(points, seed, counter):
    acc = None
    for pos, p in enumerate(points):
        acc = bls.g1_add(acc, bls.g1_mul(p, _coeff(seed, counter, pos)))
    return acc


def test_the_sums_follow_the_model(be, fx):
    keys = dict(fx["keys"])
    clean = dict(fx["clean"])
    e = keys["ivc"]
    clean["ivc"] = synth.forge_batch(e["vk"], e["td"], 3, seed=81, plan=e["pl"])          # three proofs of EVERY key
    assert list(e["ov"].verify_batch(clean["ivc"].proofs, clean["ivc"].proof_off, clean["ivc"].instances, None, threads=2)) == [1, 1, 1]
    order = [(name, j) for j in range(3) for name in MIXED_KEYS]
    random.Random(82).shuffle(order)

    def l_point(batches, name, j):
        """L_i: pi_i read from the proof bytes, or - ivc - the folded el' of the oracle's trace"""
        b, k = batches[name], keys[name]
        proof = b.proof(j)
        if name == "ivc":
            ok, tr = k["ov"].verify(proof, b.instance_ints(j, k["vk"].n_public_inputs), None, trace=True)
            assert ok
            return tr.point("el")
        o = k["pl"].points[k["pl"].pi_point]
        return bls.g1_decompress(proof[o:o + 48])

    seed = bytes(range(100, 132))
    ws = be.Workspace.multi(fx["plans"], 16, lanes=2, chunk=2)       # (a key's three proofs run as chunks of 2 + 1)
    # the count of seeded calls this process has made so far, from a one-proof call: L = r_0 pi_0
    one = Mix(keys, clean, [("simple_mul", 0)])
    assert _host(be, fx, one, ws, seed=seed) == ([1], [0], False)
    l1, r1 = be.probe_mixed_fold_sums(ws)
    p0 = l_point(clean, "simple_mul", 0)
    counter = next(c for c in range(1 << 16) if bls.g1_mul(p0, _coeff(seed, c, 0)) == l1)
    assert r1 == bls.g1_mul(l1, COMMON_S)
    # the 12-proof mix: L = sum r_i L_i with r_i keyed by the position in the CALL, R = [s] L
    mix = Mix(keys, clean, order)
    assert _host(be, fx, mix, ws, seed=seed) == ([1] * 12, [0] * 12, False)
    counter += 1
    pts = [l_point(clean, name, j) for name, j in order]
    l12, r12 = be.probe_mixed_fold_sums(ws)
    assert l12 == _model_l(pts, seed, counter) and l12 is not None
    assert r12 == bls.g1_mul(l12, COMMON_S)
    # two proofs of different keys exchanged in call order: the coefficients stay with the positions
    a = next(i for i, (name, _j) in enumerate(order) if name == "simple_mul")
    b = next(i for i, (name, _j) in enumerate(order) if name == "lookup_table")
    swapped = list(order)
    swapped[a], swapped[b] = swapped[b], swapped[a]
    assert _host(be, fx, Mix(keys, clean, swapped), ws, seed=seed) == ([1] * 12, [0] * 12, False)
    counter += 1
    pts2 = list(pts)
    pts2[a], pts2[b] = pts2[b], pts2[a]
    l_sw, r_sw = be.probe_mixed_fold_sums(ws)
    assert l_sw == _model_l(pts2, seed, counter) and l_sw != _model_l(pts, seed, counter)
    assert r_sw == bls.g1_mul(l_sw, COMMON_S)
    # one proof that only the pairing rejects: L is still the model's, R is no longer [s] L, and that proof alone is rejected
    bad = dict(clean)
    bad["lookup_table"] = _with_one_reject(fx, "lookup_table", 1)
    mix_bad = Mix(keys, bad, order)
    hit = order.index(("lookup_table", 1))
    acc, st, fb = _host(be, fx, mix_bad, ws, seed=seed)
    counter += 1
    assert acc == [int(i != hit) for i in range(12)] and st == [0 if i != hit else be.ST_PAIRING for i in range(12)] and fb
    l_bad, r_bad = be.probe_mixed_fold_sums(ws)
    assert l_bad == _model_l([l_point(bad, name, j) for name, j in order], seed, counter)
    assert r_bad != bls.g1_mul(l_bad, COMMON_S)
    ws.close()


# ---- 5
def test_rejects_in_two_keys_and_the_same_reject_twice(be, fx):
    bad = dict(fx["clean"])
    hit = [("simple_mul", 17), ("lookup_table", 64)]
    for name, j in hit:
        bad[name] = _with_one_reject(fx, name, j)
    order = list(fx["mix_clean"].order)
    ws = be.Workspace.multi(fx["plans"], len(order) + 1, lanes=4, chunk=40)
    mix = Mix(fx["keys"], bad, order)
    acc, st, fb = _host(be, fx, mix, ws)
    assert [i for i, a in enumerate(acc) if not a] == sorted(order.index(h) for h in hit) and fb
    assert acc == mix.expected and [s for s in st if s] == [be.ST_PAIRING] * 2
    assert not ws.rlc_result(timings=False)[0]
    # the same rejecting proof a second time, at another position of the call
    only = dict(fx["clean"])
    only["simple_mul"] = bad["simple_mul"]
    first = order.index(hit[0])
    at = (first + 71) % len(order)
    twice = order[:at] + [hit[0]] + order[at:]
    mix2 = Mix(fx["keys"], only, twice)
    acc, st, fb = _host(be, fx, mix2, ws)
    assert [i for i, a in enumerate(acc) if not a] == [i for i, h in enumerate(twice) if h == hit[0]] and sum(1 for a in acc if not a) == 2
    assert fb and [s for s in st if s] == [be.ST_PAIRING] * 2
    ws.close()


# ---- 6
def test_edge_shapes(be, fx):
    keys, rej, clean = fx["keys"], fx["rejects"], fx["clean"]
    ws = be.Workspace.multi(fx["plans"], 80)
    empty = Mix(keys, rej, [])
    assert _host(be, fx, empty, ws) == ([], [], False)
    assert _device(be, fx, empty, ws) == ([], [])
    for tag, batches, entry in (("clean", clean, ("simple_mul", 3)), ("clean", clean, ("ivc", 0)), ("rejects", rej, ("ivc", 0)),
                                ("rejects", rej, ("trashcan_mix", 2))):
        one = Mix(keys, batches, [entry])                      # n = 1
        acc, st, fb = _host(be, fx, one, ws)
        assert (acc, st) == (one.expected, _want_status(fx, tag, one))
        assert fb == (st == [be.ST_PAIRING])
    # a call whose only key is ivc, listed alone: one R-term per proof
    solo_ivc = Mix(keys, clean, [("ivc", 0)])
    solo_ivc.plan_of = [0]
    assert _host(be, fx, solo_ivc, ws, plans=[keys["ivc"]["dp"]]) == ([1], [0], False)
    assert ws.rlc_result()[1].msm_terms == 1
    # every proof of one key, listed alone, on an ORDINARY workspace: sub-batch and tail one after the other on one stream
    b = rej["simple_mul"]
    solo = Mix(keys, rej, [("simple_mul", j) for j in range(b.n)])
    solo.plan_of = [0] * solo.n
    plain = be.Workspace(keys["simple_mul"]["dp"], 80)
    assert plain.lanes() == (1, 80)
    want_st = fx["want"][("rejects", "simple_mul")]
    acc, st, fb = _host(be, fx, solo, plain, plans=[keys["simple_mul"]["dp"]])
    assert acc == b.expected and st == want_st and fb == any(s == be.ST_PAIRING for s in want_st)
    c = clean["simple_mul"]
    solo_clean = Mix(keys, clean, [("simple_mul", j) for j in range(c.n)])
    solo_clean.plan_of = [0] * c.n
    assert _host(be, fx, solo_clean, plain, plans=[keys["simple_mul"]["dp"]]) == ([1] * c.n, [0] * c.n, False)
    kws = be.Workspace(keys["simple_mul"]["dp"], c.n)
    keys["simple_mul"]["dp"].verify_batch_rlc(c.proofs, c.proof_off, c.instances, c.committed, ws=kws, seed=SEED)
    assert plain.rlc_result()[1].msm_terms == kws.rlc_result()[1].msm_terms
    for w in (ws, plain, kws):
        w.close()


# ---- 7
def test_seeds_and_order_do_not_change_the_verdicts(be, fx):
    mix = fx["mix"]
    want = (mix.expected, _want_status(fx, "rejects", mix))
    ws = be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)
    for seed in (bytes(range(32)), bytes(range(200, 232))):
        assert _host(be, fx, mix, ws, seed=seed)[:2] == want
    clean = fx["mix_clean"]
    for seed in (bytes(range(32)), bytes(range(200, 232)), None):
        assert _host(be, fx, clean, ws, seed=seed) == ([1] * clean.n, [0] * clean.n, False)
    perm = list(range(mix.n))
    random.Random(91).shuffle(perm)
    mix2 = Mix(fx["keys"], fx["rejects"], [mix.order[i] for i in perm])
    assert mix2.plan_of != mix.plan_of
    acc, st, _fb = _host(be, fx, mix2, ws)
    assert acc == [want[0][i] for i in perm] and st == [want[1][i] for i in perm]
    ws.close()


# ---- 8
def test_fold_and_plain_calls_back_to_back_on_one_stream(be, fx):
    import torch
    ws = be.Workspace.multi(fx["plans"], fx["mix"].n)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    first, second = fx["mix"], fx["mix_clean"]
    calls = [_FoldCall(be, fx, first, "rlc", ws, s, launch=False), _FoldCall(be, fx, second, "rlc", ws, s, launch=False),
             _DeviceCall(be, fx, first, "rlc", ws, s, launch=False)]
    for c in calls:              # every input is on the device already: nothing but the calls themselves from here on
        c.launch()
    for c, m, tag in zip(calls, (first, second, first), ("rejects", "clean", "rejects")):
        assert c.results() == (m.expected, _want_status(fx, tag, m))
    ws.close()


# ---- 9
def test_cpp_driver(be, fx, tmp_path):
    out = str(tmp_path / "h2v_mixed_fold_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_fold_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for k, name in enumerate(LISTED):
        e = fx["keys"][name]
        path = str(tmp_path / ("%s.%s" % (name, "json" if k % 2 else "bin")))      # both forms of a key
        with open(path, "wb") as f:
            f.write(e["vk"].to_json().encode() if k % 2 else e["pl"].to_bytes())
        paths.append(path)
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    bad = dict(fx["clean"])
    bad["lookup_table"] = _with_one_reject(fx, "lookup_table", 5)
    order = [(name, j) for name in MIXED_KEYS for j in range(min(6, fx["clean"][name].n))]
    random.Random(95).shuffle(order)
    for tag, batches in (("accept", fx["clean"]), ("reject", bad)):
        mix = Mix(fx["keys"], batches, order)
        assert mix.n == 19 and sum(mix.expected) == (19 if tag == "accept" else 18)
        blob = struct.pack("<I", mix.n)
        for name, j in mix.order:
            b, e = batches[name], fx["keys"][name]
            n_pi = e["vk"].n_public_inputs
            p = b.proof(j)
            blob += struct.pack("<II", LISTED.index(name), len(p)) + p + struct.pack("<I", n_pi) + b.instances[32 * n_pi * j:32 * n_pi * (j + 1)]
            blob += struct.pack("<I", 1) + b.ci(j) if b.committed is not None else struct.pack("<I", 0)
        with open(str(tmp_path / (tag + ".bin")), "wb") as f:
            f.write(blob)
        r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / (tag + ".bin"))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
        assert got["fold"] == "".join(str(a) for a in mix.expected)
        assert [int(x) for x in got["status"].split()] == [0 if a else be.ST_PAIRING for a in mix.expected]
        assert got["fold_fell_back"] == ("0" if tag == "accept" else "1")
        assert got["batch_verify"] == ("ok" if tag == "accept" else str(be.ST_PAIRING))
        assert got["workspace"] == "1"
        if tag == "accept":
            assert int(got["msm_terms"]) > mix.n
