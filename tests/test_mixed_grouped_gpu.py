"""GPU tests of H2V_MIXED_GROUPED / H2V_RLC_GROUPED (include/h2v.h: phase 1 of every groupable key of a mixed call in one launch
per kernel, up to 1024 keys).  Expectations come from the CPU oracle, from construction, from the per-key call's status words and
from the big-integer models (tests/cancel.py, tests/agg_model.py) - never from the call under test; where the ungrouped call is
run beside the grouped one it is held to the same expectation, which is how "the same results" is checked.

Keys: the shared fixture of tests/test_mixed_keys_gpu.py (simple_mul 70, lookup_table 65, trashcan_mix 9, ivc 1 - not groupable -,
atms_with_lookups listed without a proof), one blake2b-512 flavoured simple_mul key (the second transcript kind) and 66 further
simple_mul keys from other builder seeds on the common SRS, compiled through h2v_plan_compile and forged in-process.
On the code before the flag existed every test here ends in H2V_E_ARG (unknown flag), and seventy keys with proofs in one call
cannot pass in any form."""
import json
import os
import random
import struct
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, synth
from tests import agg_model, cancel
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S, MIXED_KEYS, PKG, ROOT
from tests.test_mixed_keys_gpu import LISTED, SEED, Mix, _interleaved, _per_key_device, _want_status, fx  # noqa: F401
from tests.test_mixed_fold_gpu import _with_one_reject

pytestmark = pytest.mark.gpu
PRE_PAIRING = ["noncanonical_scalar", "point_not_on_curve", "point_not_in_subgroup", "bad_point_flag", "truncated"]
N_MORE = 66


class Call:
    """a mixed batch over an explicit list of keys: order = [(key name, index in that key's batch)], names = the listed keys"""

    def __init__(self, keys, batches, names, order):
        self.order, self.names = list(order), list(names)
        self.plans = [keys[name]["dp"] for name in names]
        self.plan_of = [names.index(name) for name, _ in self.order]
        proofs, inst, ci, self.off, self.expected = [], [], [], [0], []
        for name, j in self.order:
            b, n_pi = batches[name], keys[name]["vk"].n_public_inputs
            proofs.append(b.proof(j))
            self.off.append(self.off[-1] + len(proofs[-1]))
            inst.append(b.instances[32 * n_pi * j:32 * n_pi * (j + 1)])
            if b.committed is not None:
                ci.append(b.ci(j))
            self.expected.append(b.expected[j])
        self.n = len(self.order)
        self.proofs, self.instances, self.committed = b"".join(proofs), b"".join(inst), b"".join(ci) or None


def _of_mix(fx, mix):
    c = Call(fx["keys"], {}, LISTED, [])
    c.order, c.plan_of, c.off, c.expected, c.n = mix.order, mix.plan_of, mix.off, mix.expected, mix.n
    c.proofs, c.instances, c.committed = mix.proofs, mix.instances, mix.committed
    return c


def _host(be, call, ws=None, seed=SEED, grouped=True):
    acc, st, fb = be.verify_mixed(call.plans, call.plan_of, call.proofs, call.off, call.instances, call.committed, ws=ws, mode="rlc", seed=seed,
                                  fold_msm=True, grouped=grouped)
    return list(acc), st, fb


def _on_device(call):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    keep = [t(call.proofs), torch.tensor(call.off, dtype=torch.int64, device=dev), t(call.instances), t(call.committed)]
    torch.cuda.current_stream().synchronize()
    return dev, keep, [x.data_ptr() if x is not None else None for x in keep]


def _device(be, call, ws, seed=SEED, grouped=True):
    import torch
    dev, keep, ptrs = _on_device(call)
    acc = torch.full((max(1, call.n),), 7, dtype=torch.uint8, device=dev)
    st = torch.full((max(1, call.n),), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    be.verify_mixed_device(call.plans, call.plan_of, call.n, *ptrs, acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream, mode="rlc", seed=seed,
                           fold_msm=True, grouped=grouped)
    s.synchronize()
    return list(acc.cpu().tolist())[:call.n], [v & 0xffffffff for v in st.cpu().tolist()][:call.n]


@pytest.fixture(scope="module")
def gx(be, fx, orc):
    """the further keys: one blake2b-512 flavoured simple_mul key and N_MORE simple_mul keys of other builder seeds, all on the
    common SRS; 1 or 2 forged proofs each; verdicts from the oracle (the Cardano keys) and status words from the per-key call"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    keys, clean = dict(fx["keys"]), dict(fx["clean"])
    vk, td = V.on_srs(*V.simple_mul_vk(seed=0x7000), COMMON_S)
    vk = V.with_transcript_hash(vk, "blake2b-512")
    pl = PL.compile_plan(vk)
    assert be.plan_compile(vk.to_json()) == pl.to_bytes()
    keys["b512"] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0), "ov": None}
    clean["b512"] = synth.forge_batch(vk, td, 5, seed=700, plan=pl, workers=1)
    acc, st = _per_key_device(keys["b512"]["dp"], clean["b512"])
    assert acc == [1] * 5 and st == [0] * 5                        # (the oracle replays the Cardano transcript only)
    more = ["m%02d" % k for k in range(N_MORE)]
    for k, name in enumerate(more):
        vk, td = V.on_srs(*V.simple_mul_vk(seed=0x7100 + k), COMMON_S)
        blob = be.plan_compile(vk.to_json())                       # through h2v_plan_compile
        pl = PL.compile_plan(vk)
        assert blob == pl.to_bytes()
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(blob, 0), "ov": ov}
        clean[name] = b = synth.forge_batch(vk, td, 1 + k % 2, seed=800 + k, plan=pl, workers=1)
        assert list(ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == b.expected == [1] * b.n
    assert len({keys[n]["pl"].to_bytes() for n in more}) == N_MORE
    return {"keys": keys, "clean": clean, "more": more}


def _l_point(keys, batches, name, j):
    """L_i: pi_i read from the proof bytes, or - ivc - the folded el' of the oracle's trace"""
    b, k = batches[name], keys[name]
    proof = b.proof(j)
    if k["pl"].acc_coords is not None:          # (a recursive key)
        ok, tr = k["ov"].verify(proof, b.instance_ints(j, k["vk"].n_public_inputs), None, trace=True)
        assert ok
        return tr.point("el")
    o = k["pl"].points[k["pl"].pi_point]
    return bls.g1_decompress(proof[o:o + 48])


def _model_sums(points, seed, counter):
    acc = None
    for pos, p in enumerate(points):
        acc = bls.g1_add(acc, bls.g1_mul(p, cancel.coeff(seed, counter, pos)))
    return acc, bls.g1_mul(acc, COMMON_S)


# ---- 1
@pytest.mark.parametrize("kind", ["none", "plain", "laned", "deferring"])
def test_the_fixture_through_every_workspace(be, fx, kind):
    """the 145 shuffled proofs with rejects of every kind, host and device forms: accept / status / fell_back are the oracle's
    verdicts and the per-key status words.  Lanes of 40 put range borders inside simple_mul's and lookup_table's proofs and let one
    range span lookup_table, trashcan_mix and what follows; 70 and 65 cross a 32-proof combiner block, a 64-proof terms block and
    a 64-point unit.  Then the all-accepting mix: the call's two sums are the big-integer model's under the call's coefficients -
    and so are the ungrouped call's, under its own count of seeded calls."""
    mix, clean = _of_mix(fx, fx["mix"]), _of_mix(fx, fx["mix_clean"])
    want_st = _want_status(fx, "rejects", fx["mix"])
    assert mix.n == 145 and 0 < sum(mix.expected) < mix.n and any(s == be.ST_PAIRING for s in want_st)
    if kind == "none":
        assert _host(be, mix, None) == (mix.expected, want_st, True)
        assert _host(be, clean, None) == ([1] * clean.n, [0] * clean.n, False)
        return
    ws = be.Workspace.multi(fx["plans"], mix.n) if kind == "plain" else be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)
    if kind != "plain":
        assert ws.lanes() == (4, 40)
    if kind == "deferring":
        ws.defer_joins(True)
    assert _host(be, mix, ws) == (mix.expected, want_st, True)
    assert not ws.rlc_result(timings=False)[0]
    assert _device(be, mix, ws) == (mix.expected, want_st)
    # the sums: the model's, for the grouped call and for the ungrouped call on the same workspace
    seed = bytes(range(60, 92))
    counter = cancel.learn_counter(be, fx, ws, seed)
    pts = [_l_point(fx["keys"], fx["clean"], name, j) for name, j in clean.order]
    for grouped in (True, False, True):
        assert _host(be, clean, ws, seed=seed, grouped=grouped) == ([1] * clean.n, [0] * clean.n, False)
        counter += 1
        assert be.probe_mixed_fold_sums(ws) == _model_sums(pts, seed, counter), grouped
    assert _device(be, clean, ws, seed=seed) == ([1] * clean.n, [0] * clean.n)
    counter += 1
    assert be.probe_mixed_fold_sums(ws) == _model_sums(pts, seed, counter)
    ws.close()


# ---- 2
def _replaced(keys, batch, name, changes, seed):
    """`batch` of key `name` with proof j corrupted as changes[j]; the expectation by construction"""
    e = keys[name]
    n_pi = e["vk"].n_public_inputs
    proofs, expected = [], []
    for j in range(batch.n):
        p = batch.proof(j)
        if j in changes:
            p, _ins = synth.corrupt(e["pl"], p, batch.instances[32 * n_pi * j:32 * n_pi * (j + 1)], changes[j], random.Random(seed + j))
        proofs.append(p)
        expected.append(int(j not in changes))
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return synth.Batch(n=batch.n, proofs=b"".join(proofs), proof_off=off, instances=batch.instances, committed=batch.committed, expected=expected)


@pytest.mark.parametrize("kind", PRE_PAIRING + ["wrong_pi"])
def test_rejects_at_the_edges_of_groups_and_ranges(be, fx, orc, kind):
    """one reject kind at a time, in the first and the last proof of a group (simple_mul 0 and 69 in plan order), in a one-proof
    group (a call of lookup_table x 1 among the others) and in the proofs on either side of a range border (grouped positions 39
    and 40 with lanes of 40: simple_mul 39 and 40): the verdicts are exact; after a failed check fell_back = 1"""
    keys = fx["keys"]
    bad = dict(fx["clean"])
    bad["simple_mul"] = _replaced(keys, fx["clean"]["simple_mul"], "simple_mul", {0: kind, 39: kind, 40: kind, 69: kind}, 11)
    bad["lookup_table"] = _replaced(keys, fx["clean"]["lookup_table"], "lookup_table", {0: kind}, 12)
    want = {}
    for name in ("simple_mul", "lookup_table"):
        b = bad[name]
        assert list(keys[name]["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4)) == b.expected
        acc, want[name] = _per_key_device(keys[name]["dp"], b)
        assert acc == b.expected
    # (the partition is stable: proof j of simple_mul's batch is the key's proof j in plan order, whatever lies between in the call)
    order = [("simple_mul", j) for j in range(70)] + [("lookup_table", 0)] + [("trashcan_mix", j) for j in range(9)] + [("ivc", 0)]
    call = Call(keys, bad, LISTED, _spread(order))
    want_st = [want[name][j] if name in want else 0 for name, j in call.order]
    want_fb = kind == "wrong_pi"
    ws = be.Workspace.multi(fx["plans"], call.n, lanes=4, chunk=40)
    assert _host(be, call, ws) == (call.expected, want_st, want_fb)
    assert ws.rlc_result(timings=False)[0] == (not want_fb)
    assert _device(be, call, ws) == (call.expected, want_st)
    ws.close()


def _spread(order):
    """a caller's order that keeps every key's own order (the partition is stable) but interleaves the keys"""
    by = {}
    for e in order:
        by.setdefault(e[0], []).append(e)
    names, out, rng = list(by), [], random.Random(15)
    while names:
        name = rng.choice(names)
        out.append(by[name].pop(0))
        if not by[name]:
            names.remove(name)
    return out


# ---- 3
def test_degenerate_tables(be, fx, gx):
    keys, clean = gx["keys"], gx["clean"]
    rej = fx["rejects"]
    names = LISTED + ("b512",)
    ws = be.Workspace.multi([keys[n]["dp"] for n in names], 80)
    ws4 = be.Workspace.multi([keys[n]["dp"] for n in names], 80, lanes=3, chunk=4)
    for w in (ws, ws4):
        # n = 0 and n = 1 (groupable, and not)
        assert _host(be, Call(keys, clean, names, []), w) == ([], [], False)
        for tag, batches, entry in (("clean", clean, ("simple_mul", 3)), ("rejects", rej, ("trashcan_mix", 2)), ("clean", clean, ("ivc", 0))):
            one = Call(keys, batches, names, [entry])
            acc, st, fb = _host(be, one, w)
            assert (acc, st) == (one.expected, [fx["want"][(tag, entry[0])][entry[1]]]) and fb == (st == [be.ST_PAIRING])
        # all proofs of one plan; a plan without proofs between two with proofs (lookup_table has none here)
        b = rej["simple_mul"]
        solo = Call(keys, rej, names, [("simple_mul", j) for j in range(b.n)])
        want_st = fx["want"][("rejects", "simple_mul")]
        assert _host(be, solo, w) == (b.expected, want_st, any(s == be.ST_PAIRING for s in want_st))
        gap = Call(keys, clean, names, _spread([("simple_mul", j) for j in range(7)] + [("trashcan_mix", j) for j in range(9)]))
        assert _host(be, gap, w) == ([1] * 16, [0] * 16, False)
        assert _device(be, gap, w) == ([1] * 16, [0] * 16)
        # only proofs that cannot be grouped: the group is empty
        assert _host(be, Call(keys, clean, names, [("ivc", 0)]), w) == ([1], [0], False)
        assert w.rlc_result()[1].msm_terms == 1
        # both transcript kinds in one call, and only the second
        both = Call(keys, clean, names, _spread([("b512", j) for j in range(5)] + [("simple_mul", j) for j in range(6)] + [("lookup_table", 1)]))
        assert _host(be, both, w) == ([1] * 12, [0] * 12, False)
        assert _device(be, both, w) == ([1] * 12, [0] * 12)
        second = Call(keys, clean, names, [("b512", j) for j in (4, 0, 2)])
        assert _host(be, second, w) == ([1] * 3, [0] * 3, False)
    # a proof of the second kind that only the pairing rejects, beside the first kind
    bad = dict(clean)
    bad["b512"] = _replaced(keys, clean["b512"], "b512", {2: "wrong_pi"}, 31)
    acc, st = _per_key_device(keys["b512"]["dp"], bad["b512"])
    assert acc == bad["b512"].expected and st == [0, 0, be.ST_PAIRING, 0, 0]
    mixed = Call(keys, bad, names, _spread([("b512", j) for j in range(5)] + [("simple_mul", j) for j in range(6)]))
    hit = mixed.order.index(("b512", 2))
    assert _host(be, mixed, ws4) == ([int(i != hit) for i in range(11)], [0 if i != hit else be.ST_PAIRING for i in range(11)], True)
    ws.close()
    ws4.close()


# ---- 4
def test_seventy_keys_with_proofs(be, fx, gx):
    """66 further keys + simple_mul, lookup_table, trashcan_mix + the blake2b-512 key = 70 groupable keys with proofs, plus ivc"""
    keys, clean, more = gx["keys"], gx["clean"], gx["more"]
    names = list(more[:33]) + ["simple_mul", "lookup_table", "ivc", "trashcan_mix", "atms_with_lookups", "b512"] + list(more[33:])
    take = {"simple_mul": 3, "lookup_table": 2, "trashcan_mix": 2, "ivc": 1, "b512": 2}
    order = [(name, j) for name in names if name != "atms_with_lookups" for j in range(take.get(name, clean[name].n))]
    random.Random(41).shuffle(order)
    call = Call(keys, clean, names, order)
    with_proofs = len({name for name, _ in order})
    assert with_proofs == 71 > be.MIXED_MAX_PLANS and len(names) == 72
    ws = be.Workspace.multi(call.plans, call.n, lanes=4, chunk=40)
    # the same list without the flag is H2V_E_LIMIT, as it always was
    with pytest.raises(be.H2VError, match="h2v error -4"):
        _host(be, call, ws, grouped=False)
    # all accepting: one check, msm_terms = N_R of include/h2v.h
    assert _host(be, call, ws) == ([1] * call.n, [0] * call.n, False)
    ok, tm = ws.rlc_result()
    n_r = 0
    for name in {name for name, _ in order}:
        cnt, pl = sum(1 for e in order if e[0] == name), keys[name]["pl"]
        n_fix = sum(1 for kind, _ in pl.terms if kind == 1)                  # (H2V_TERM_VK_BASE)
        n_r += cnt if pl.acc_coords is not None else cnt * (len(pl.terms) - n_fix) + n_fix
    assert ok and tm.msm_terms == n_r
    assert _device(be, call, ws) == ([1] * call.n, [0] * call.n)
    # one pairing-only reject in key 3 of the list and one in key 68: the second pass runs in slices, both are found, nothing else
    bad = dict(clean)
    hits = []
    for name in (names[3], names[68]):
        bad[name] = _replaced(keys, clean[name], name, {0: "wrong_pi"}, 43)
        b = bad[name]
        assert list(keys[name]["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == b.expected
        hits.append(order.index((name, 0)))
    call_bad = Call(keys, bad, names, order)
    want_acc = [int(i not in hits) for i in range(call.n)]
    want_st = [be.ST_PAIRING if i in hits else 0 for i in range(call.n)]
    assert call_bad.expected == want_acc
    assert _host(be, call_bad, ws) == (want_acc, want_st, True)
    assert not ws.rlc_result(timings=False)[0]
    assert _device(be, call_bad, ws) == (want_acc, want_st)
    plain = be.Workspace.multi(call.plans, call.n)
    assert _host(be, call_bad, plain) == (want_acc, want_st, True)
    assert _host(be, call, plain) == ([1] * call.n, [0] * call.n, False)
    plain.close()
    # 1024 listed plans with proofs in five of them is fine; 1025 is H2V_E_LIMIT
    five = ["simple_mul", "b512", more[0], "ivc", more[65]]
    listed = (five + [more[k % N_MORE] for k in range(be.MIXED_GROUPED_MAX_PLANS)])[:be.MIXED_GROUPED_MAX_PLANS]
    small = Call(keys, clean, listed, [(name, 0) for name in five] + [("simple_mul", 1)])
    assert small.plan_of == [0, 1, 2, 3, 4, 0] and len(small.plans) == 1024
    assert _host(be, small, ws) == ([1] * 6, [0] * 6, False)
    small.plans = small.plans + [small.plans[0]]
    with pytest.raises(be.H2VError, match="h2v error -4"):
        _host(be, small, ws)
    ws.close()


# ---- 5
def _n_records(be, ws):
    """the records a FRESH workspace has taken, through the public interface: record k calls back answers h2v_workspace_timings
    (verify / prepare / check kinds) or h2v_workspace_rlc_result (kind RLC), and beyond the first call both are H2V_E_ARG"""
    k = 0
    while k < 63:
        try:
            ws.timings(k)
        except be.H2VError:
            try:
                ws.rlc_result(k, timings=False)
            except be.H2VError:
                break
        k += 1
    return k


def test_records(be, fx):
    """an all-groupable call on a workspace whose chunk holds it takes exactly two records - the grouped part's and the tail's -
    and three with ivc present; the tail is the call's last (h2v_workspace_rlc_result(ws, 0, ..)); without the flag the same call
    takes one record per key with proofs and the tail's"""
    keys, clean = fx["keys"], fx["clean"]
    groupable = Call(keys, clean, LISTED, _spread([("simple_mul", j) for j in range(20)] + [("lookup_table", j) for j in range(9)] + [("trashcan_mix", j) for j in range(9)]))
    with_ivc = Call(keys, clean, LISTED, groupable.order + [("ivc", 0)])
    for call, grouped, want in ((groupable, True, 2), (with_ivc, True, 3), (with_ivc, False, 5)):
        ws = be.Workspace.multi(fx["plans"], 64, lanes=2, chunk=64)
        assert _n_records(be, ws) == 0
        assert _host(be, call, ws, grouped=grouped) == ([1] * call.n, [0] * call.n, False)
        ok, tm = ws.rlc_result(0)                                    # the tail: the call's last record, kind RLC, passed
        assert ok and tm.msm_terms > call.n
        with pytest.raises(be.H2VError):
            ws.rlc_result(1, timings=False)                          # (the record before it is a prepare call's)
        assert _n_records(be, ws) == want, (grouped, want)
        ws.close()
    # an ordinary workspace: the grouped part and the tail one after the other on one stream
    solo = Call(keys, clean, ["simple_mul"], [("simple_mul", j) for j in range(40)])
    plain = be.Workspace(keys["simple_mul"]["dp"], 64)
    assert plain.lanes() == (1, 64)
    assert _host(be, solo, plain) == ([1] * 40, [0] * 40, False)
    assert plain.rlc_result(0)[0] and _n_records(be, plain) == 2
    plain.close()


# ---- 6
def _aggregate_host(be, call, ws, grouped):
    pair, inc, st, info = be.aggregate_mixed(call.plans, call.plan_of, call.proofs, call.off, call.instances, call.committed, ws=ws, seed=SEED, grouped=grouped)
    return pair, list(inc), st, info


def test_aggregate_mixed_grouped(be, fx, orc):
    """the pair is tests/agg_model.py's bit for bit under the seed the call reports - for the grouped call and for the ungrouped one -
    included[] is equal, and the device form returns with its stream still busy"""
    import torch
    keys = fx["keys"]
    batches = dict(fx["clean"])
    batches["simple_mul"] = _replaced(keys, fx["clean"]["simple_mul"], "simple_mul", {1: "bad_point_flag", 5: "wrong_pi"}, 51)
    order = _spread([("simple_mul", j) for j in range(8)] + [("lookup_table", j) for j in range(5)] + [("trashcan_mix", 0), ("ivc", 0)])
    call = Call(keys, batches, LISTED, order)
    want = []
    for name, j in order:
        e, b = keys[name], batches[name]
        ok, otr = e["ov"].verify(b.proof(j), b.instance_ints(j, e["vk"].n_public_inputs), b.ci(j), trace=True)
        want.append(orc.g1_compress(otr.point("el")) + orc.g1_compress(otr.point("er")) if otr.status in (0, 1) else bytes(96))
    reached = [int(p != bytes(96)) for p in want]
    assert sum(reached) == call.n - 1
    for ws in (be.Workspace.multi(fx["plans"], 64), be.Workspace.multi(fx["plans"], 64, lanes=3, chunk=4)):
        infos = []
        for grouped in (True, False):
            pair, inc, st, info = _aggregate_host(be, call, ws, grouped)
            assert inc == reached and [int(s == 0) for s in st] == reached
            assert pair == agg_model.model_pair(want, reached, bytes(info.seed_used), info.chunk), grouped
            assert (info.chunk, info.n_chunks) == (0, 1) and not agg_model.holds(pair, COMMON_S)       # the wrong_pi proof is included
            infos.append(info.msm_terms)
        assert infos[0] == infos[1]
        assert ws.rlc_verdict() == be.BATCH_NOT_CHECKED
        # the device form: enqueued behind a spin of the stream, it returns while the stream is still busy
        dev, keep, ptrs = _on_device(call)
        pair = torch.full((96,), 7, dtype=torch.uint8, device=dev)
        inc = torch.full((call.n,), 7, dtype=torch.uint8, device=dev)
        st = torch.full((call.n,), -1, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(400_000_000)
        info = be.aggregate_mixed_device(call.plans, call.plan_of, call.n, *ptrs, pair.data_ptr(), inc.data_ptr(), st.data_ptr(), ws=ws,
                                         stream=s.cuda_stream, seed=SEED, grouped=True)
        assert not s.query()                                         # nothing synchronised the stream
        s.synchronize()
        assert inc.cpu().tolist() == reached
        assert bytes(pair.cpu().numpy().tobytes()) == agg_model.model_pair(want, reached, bytes(info.seed_used), info.chunk)
        ws.close()


# ---- 7
def test_cancelling_errors(be, fx):
    """two proofs of DIFFERENT keys built to cancel under equal weights do not pass; built for the call's coefficients under a
    given seed they pass; with their places exchanged they are rejected"""
    keys, clean = fx["keys"], fx["clean"]
    ra, rb = cancel.rec_of(keys["simple_mul"], clean["simple_mul"], 2), cancel.rec_of(keys["lookup_table"], clean["lookup_table"], 4)
    order = _spread([("simple_mul", j) for j in range(6)] + [("lookup_table", j) for j in range(6)] + [("trashcan_mix", 1)])
    pa, pb = order.index(("simple_mul", 2)), order.index(("lookup_table", 4))

    def call_with(a, b, order):
        bad = dict(clean)
        for name, j, proof in (("simple_mul", 2, a), ("lookup_table", 4, b)):
            src = clean[name]
            proofs = [src.proof(i) if i != j else proof for i in range(src.n)]
            off = [0]
            for p in proofs:
                off.append(off[-1] + len(p))
            bad[name] = synth.Batch(n=src.n, proofs=b"".join(proofs), proof_off=off, instances=src.instances, committed=src.committed,
                                    expected=[int(i != j) for i in range(src.n)])
        return Call(keys, bad, LISTED, order)

    ws = be.Workspace.multi(fx["plans"], 64, lanes=2, chunk=5)
    rejected = [int(i not in (pa, pb)) for i in range(len(order))]
    a1, b1 = cancel.cancelling(ra, rb, 1, 1, 7)
    assert _host(be, call_with(a1, b1, order), ws)[::2] == (rejected, True)
    seed = bytes(range(150, 182))
    counter = cancel.learn_counter(be, fx, ws, seed) + 1
    a2, b2 = cancel.cancelling(ra, rb, cancel.coeff(seed, counter, pa), cancel.coeff(seed, counter, pb), 7)
    assert _host(be, call_with(a2, b2, order), ws, seed=seed) == ([1] * len(order), [0] * len(order), False)      # the check is passed: that is the attack
    swapped = list(order)
    swapped[pa], swapped[pb] = swapped[pb], swapped[pa]
    counter = cancel.learn_counter(be, fx, ws, seed) + 1
    a3, b3 = cancel.cancelling(ra, rb, cancel.coeff(seed, counter, pa), cancel.coeff(seed, counter, pb), 7)
    acc, st, fb = _host(be, call_with(a3, b3, swapped), ws, seed=seed)
    assert fb and acc == rejected and [s for s in st if s] == [be.ST_PAIRING] * 2
    ws.close()


# ---- 8
def test_calls_after_a_grouped_call_are_unchanged(be, fx):
    mix = _of_mix(fx, fx["mix"])
    want = (mix.expected, _want_status(fx, "rejects", fx["mix"]))
    ws = be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)
    assert _host(be, mix, ws)[:2] == want
    assert _host(be, mix, ws, grouped=False)[:2] == want
    acc, st, _fb = be.verify_mixed(mix.plans, mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, mode="per-proof")
    assert (list(acc), st) == want
    for name in ("simple_mul", "ivc"):
        b = fx["rejects"][name]
        got = fx["keys"][name]["dp"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws)
        assert list(got) == b.expected
    assert _host(be, mix, ws)[:2] == want
    ws.close()


# ---- 9
def test_cpp_driver(be, fx, tmp_path):
    out = str(tmp_path / "h2v_mixed_grouped_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_grouped_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for k, name in enumerate(LISTED):
        e = fx["keys"][name]
        path = str(tmp_path / ("%s.%s" % (name, "json" if k % 2 else "bin")))
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
        bits = "".join(str(a) for a in mix.expected)
        assert got["grouped"] == bits
        assert [int(x) for x in got["status"].split()] == [0 if a else be.ST_PAIRING for a in mix.expected]
        assert got["grouped_fell_back"] == ("0" if tag == "accept" else "1")
        assert got["batch_verify"] == ("ok" if tag == "accept" else str(be.ST_PAIRING))
        assert got["workspace"] == "1"
        inc, holds, terms = got["aggregate"].split()
        assert inc == "1" * mix.n and holds == ("1" if tag == "accept" else "0") and int(terms) > mix.n      # (only the pairing rejects: all included)
        assert got["aggregator"] == bits + (" 0" if tag == "accept" else " 1")
        if tag == "accept":
            assert int(got["msm_terms"]) > mix.n
