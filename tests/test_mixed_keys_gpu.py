"""GPU tests of the mixed-key call (h2v_verify_mixed: proofs of several keys on one SRS, one call, one pairing launch - or
ONE pairing with H2V_MIXED_RLC).  Expectations come from the CPU oracle and from construction, as in test_end_to_end_vs_oracle;
status words are also compared with the per-key h2v_verify_batch_device call on the same proofs.

The shared fixture: simple_mul / lookup_table / trashcan_mix / ivc on one SRS (vk.on_srs) with 70 / 65 / 9 / 1 proofs - the
counts cross a 64-lane wave and a 64-proof group, and one key has a single proof -, atms_with_lookups listed without a proof,
rejects of every kind (`truncated` included: record lengths vary inside a key), interleaved by a seeded shuffle: 145 proofs."""
import json
import os
import random
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import synth
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S, MIXED_KEYS, PKG, ROOT

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
COUNTS = {"simple_mul": 70, "lookup_table": 65, "trashcan_mix": 9, "ivc": 1}
LISTED = MIXED_KEYS + ("atms_with_lookups",)          # the last one has no proof in any call


class Mix:
    """a mixed batch in the layout of h2v_mixed_batch, with the key and the index within that key's batch of every proof"""

    def __init__(self, keys, batches, order):
        self.order = list(order)                       # (key name, index in that key's batch), the caller's order
        self.plan_of = [LISTED.index(name) for name, _ in self.order]
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


def _interleaved(batches, seed):
    order = [(name, j) for name in MIXED_KEYS for j in range(batches[name].n)]
    random.Random(seed).shuffle(order)
    return order


def _per_key_device(dp, batch):
    """(accept, status) of h2v_verify_batch_device on one key's batch"""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    proofs, inst, ci = t(batch.proofs), t(batch.instances), t(batch.committed)
    off = torch.tensor(batch.proof_off, dtype=torch.int64, device=dev)
    acc = torch.full((batch.n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((batch.n,), -1, dtype=torch.int32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    dp.verify_batch_device(batch.n, ptr(proofs), ptr(off), ptr(inst), ptr(ci), acc.data_ptr(), st.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()]


@pytest.fixture(scope="module")
def fx(be, orc):
    """keys on one SRS, one batch with rejects and one without per key, the oracle's verdicts and the per-key call's status
    words for both (computed once, never changed)"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    keys = {}
    for name in LISTED:
        vk, td = V.on_srs(*V.BUILDERS[name](), COMMON_S)
        pl = PL.compile_plan(vk)
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0),
                      "ov": orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))}
    clean, rejects, want = {}, {}, {}
    for k, name in enumerate(MIXED_KEYS):
        e = keys[name]
        clean[name] = synth.forge_batch(e["vk"], e["td"], COUNTS[name], seed=41 + k, plan=e["pl"])
        rejects[name] = synth.with_rejects(e["pl"], clean[name], e["vk"].n_public_inputs, fraction=0.3, seed=51 + k,
                                           kinds=list(synth.CORRUPTIONS))
        for tag, b in (("clean", clean[name]), ("rejects", rejects[name])):
            ora = list(e["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4))
            assert ora == b.expected, (name, tag)                      # the oracle and the construction agree
            acc, st = _per_key_device(e["dp"], b)
            assert acc == ora, (name, tag)
            want[(tag, name)] = st
    assert sum(1 for name in ("simple_mul", "lookup_table") if 0 < sum(rejects[name].expected) < rejects[name].n) == 2
    assert any(len(rejects[n].proof(j)) != keys[n]["pl"].proof_len for n in MIXED_KEYS for j in range(rejects[n].n)), "no truncated proof"
    plans = [keys[name]["dp"] for name in LISTED]
    return {"keys": keys, "clean": clean, "rejects": rejects, "want": want, "plans": plans,
            "mix": Mix(keys, rejects, _interleaved(rejects, 61)), "mix_clean": Mix(keys, clean, _interleaved(clean, 62))}


def _want_status(fx, tag, mix):
    return [fx["want"][(tag, name)][j] for name, j in mix.order]


def _host(be, fx, mix, mode, ws=None, plans=None):
    acc, st, fb = be.verify_mixed(plans or fx["plans"], mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, mode=mode,
                                  seed=SEED if mode == "rlc" else None)
    return list(acc), st, fb


class _DeviceCall:
    """one device-form call: the tensors stay alive until results() has synchronised"""

    def __init__(self, be, fx, mix, mode, ws, stream, launch=True):
        import torch
        dev = torch.device("cuda", 0)
        t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
        self.keep = [t(mix.proofs), torch.tensor(mix.off, dtype=torch.int64, device=dev), t(mix.instances), t(mix.committed)]
        self.acc = torch.full((max(1, mix.n),), 7, dtype=torch.uint8, device=dev)
        self.st = torch.full((max(1, mix.n),), -1, dtype=torch.int32, device=dev)
        self.n, self.stream = mix.n, stream
        self.args = (be, fx["plans"], mix.plan_of, mode, ws)
        torch.cuda.current_stream().synchronize()          # (the uploads above)
        if launch:
            self.launch()

    def launch(self):
        be, plans, plan_of, mode, ws = self.args
        ptr = lambda x: x.data_ptr() if x is not None else None
        be.verify_mixed_device(plans, plan_of, self.n, *[ptr(x) for x in self.keep], self.acc.data_ptr(), self.st.data_ptr(), ws=ws,
                               stream=self.stream.cuda_stream if self.stream is not None else None, mode=mode,
                               seed=SEED if mode == "rlc" else None)

    def results(self):
        import torch
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()
        return list(self.acc.cpu().tolist())[:self.n], [v & 0xffffffff for v in self.st.cpu().tolist()][:self.n]


def _device(be, fx, mix, mode, ws):
    import torch
    return _DeviceCall(be, fx, mix, mode, ws, torch.cuda.Stream(device=torch.device("cuda", 0))).results()


# ---- 1
@pytest.mark.parametrize("mode", ["per-proof", "rlc"])
def test_both_modes_equal_the_oracle(be, fx, mode):
    mix = fx["mix"]
    assert mix.n == 145 and 0 < sum(mix.expected) < mix.n
    want_st = _want_status(fx, "rejects", mix)
    ws = be.Workspace.multi(fx["plans"], mix.n)
    acc, st, fb = _host(be, fx, mix, mode, ws)
    assert acc == mix.expected and st == want_st
    if mode == "rlc":
        assert fb == any(s == be.ST_PAIRING for s in want_st)
    acc, st = _device(be, fx, mix, mode, ws)
    assert acc == mix.expected and st == want_st
    acc, st, _fb = _host(be, fx, mix, mode, None)          # a temporary workspace
    assert acc == mix.expected and st == want_st
    ws.close()


# ---- 2
def test_all_accepting_batch_is_one_pairing(be, fx):
    mix = fx["mix_clean"]
    ws = be.Workspace.multi(fx["plans"], mix.n)
    acc, st, fb = _host(be, fx, mix, "rlc", ws)
    assert acc == [1] * mix.n and st == [0] * mix.n and not fb
    ok, tm = ws.rlc_result()
    assert ok and tm.msm_terms == mix.n and tm.transcript_combiner_ms == 0
    # one rejecting proof in EACH of two different keys: exactly those two are rejected
    bad = dict(fx["clean"])
    hit = []
    for name, j in (("simple_mul", 17), ("lookup_table", 64)):
        b, e = bad[name], fx["keys"][name]
        n_pi = e["vk"].n_public_inputs
        p, _ins = synth.corrupt(e["pl"], b.proof(j), b.instances[32 * n_pi * j:32 * n_pi * (j + 1)], "wrong_pi", random.Random(7))
        proofs = [b.proof(i) if i != j else p for i in range(b.n)]
        bad[name] = synth.Batch(n=b.n, proofs=b"".join(proofs), proof_off=list(b.proof_off), instances=b.instances, committed=b.committed,
                                expected=[int(i != j) for i in range(b.n)])
        assert list(e["ov"].verify_batch(bad[name].proofs, bad[name].proof_off, bad[name].instances, bad[name].committed, threads=2)) == bad[name].expected
        hit.append((name, j))
    mix2 = Mix(fx["keys"], bad, fx["mix_clean"].order)
    acc, st, fb = _host(be, fx, mix2, "rlc", ws)
    assert [i for i, a in enumerate(acc) if not a] == sorted(mix2.order.index(h) for h in hit)
    assert acc == mix2.expected and fb
    assert [s for s in st if s] == [be.ST_PAIRING] * 2
    assert not ws.rlc_result(timings=False)[0]
    ws.close()


# ---- 3
def test_edge_sizes(be, fx):
    keys, rej = fx["keys"], fx["rejects"]
    ws = be.Workspace.multi(fx["plans"], 80)
    empty = Mix(keys, rej, [])
    for mode in ("per-proof", "rlc"):
        assert _host(be, fx, empty, mode, ws) == ([], [], False)
        assert _device(be, fx, empty, mode, ws) == ([], [])
        one = Mix(keys, rej, [("ivc", 0)])
        assert _host(be, fx, one, mode, ws)[:2] == (one.expected, _want_status(fx, "rejects", one))
        # every proof of one key: the verdicts of h2v_verify_batch
        b = rej["simple_mul"]
        solo = Mix(keys, rej, [("simple_mul", j) for j in range(b.n)])
        acc, st, _fb = _host(be, fx, solo, mode, ws)
        assert acc == list(keys["simple_mul"]["dp"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed)) == b.expected
        assert st == fx["want"][("rejects", "simple_mul")]
        # ... also with that key listed alone, on an ORDINARY workspace (sub-batch and tail one after the other on one stream)
        plain = be.Workspace(keys["simple_mul"]["dp"], 80)
        assert plain.lanes() == (1, 80)
        solo.plan_of = [0] * solo.n
        acc, st, _fb = _host(be, fx, solo, mode, plain, plans=[keys["simple_mul"]["dp"]])
        assert acc == b.expected and st == fx["want"][("rejects", "simple_mul")]
        if mode == "rlc":
            assert plain.rlc_result()[1].msm_terms == solo.n
        plain.close()
        five = Mix(keys, rej, [("trashcan_mix", 2), ("simple_mul", 0), ("ivc", 0), ("lookup_table", 3), ("trashcan_mix", 0)])
        acc, st = _device(be, fx, five, mode, ws)
        assert acc == five.expected and st == _want_status(fx, "rejects", five)
    ws.close()


# ---- 4
def test_order_independence(be, fx):
    """permuting the mixed batch - plan_of with it - permutes the verdicts"""
    mix = fx["mix"]
    ws = be.Workspace.multi(fx["plans"], mix.n)
    perm = list(range(mix.n))
    random.Random(63).shuffle(perm)
    mix2 = Mix(fx["keys"], fx["rejects"], [mix.order[i] for i in perm])
    assert mix2.plan_of == [mix.plan_of[i] for i in perm] and mix2.plan_of != mix.plan_of
    for mode in ("per-proof", "rlc"):
        a1, s1, _ = _host(be, fx, mix, mode, ws)
        a2, s2, _ = _host(be, fx, mix2, mode, ws)
        assert a2 == [a1[i] for i in perm] and s2 == [s1[i] for i in perm]
    ws.close()


# ---- 5
@pytest.mark.parametrize("mode", ["per-proof", "rlc"])
def test_workspace_kinds_give_the_same_verdicts(be, fx, mode):
    import torch
    mix = fx["mix"]
    want = (mix.expected, _want_status(fx, "rejects", mix))
    plain = be.Workspace.multi(fx["plans"], mix.n)
    laned = be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)       # sub-batches and tail cut across the lanes
    assert laned.lanes() == (4, 40)
    deferring = be.Workspace.multi(fx["plans"], mix.n, lanes=4, chunk=40)
    deferring.defer_joins(True)
    for ws in (plain, laned, deferring):
        assert _device(be, fx, mix, mode, ws) == want
        assert _host(be, fx, mix, mode, ws)[:2] == want
    # on the deferring one the NULL stream is refused ...
    with pytest.raises(be.H2VError, match="h2v error -1.*NULL stream"):
        _DeviceCall(be, fx, mix, mode, deferring, None)
    # ... and a mixed call is a join point: small per-key calls gathered before it run first, and are the stream's with it
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    b = fx["rejects"]["trashcan_mix"]
    dev = torch.device("cuda", 0)
    t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    keep = [t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed)]
    acc = torch.full((b.n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fx["keys"]["trashcan_mix"]["dp"].verify_batch_device(b.n, *[x.data_ptr() for x in keep], acc.data_ptr(), None, ws=deferring, stream=s.cuda_stream)
    call = _DeviceCall(be, fx, mix, mode, deferring, s)
    assert call.results() == want
    assert list(acc.cpu().tolist()) == b.expected
    for ws in (plain, laned, deferring):
        ws.close()


# ---- 6
@pytest.mark.parametrize("mode", ["per-proof", "rlc"])
def test_two_calls_back_to_back_without_a_sync(be, fx, mode):
    """different plan_of, one stream, nothing between the calls: the second call's tables must not land in staging that the
    first call's copy or kernels still read"""
    import torch
    ws = be.Workspace.multi(fx["plans"], fx["mix"].n)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    first, second = fx["mix"], fx["mix_clean"]
    assert first.plan_of != second.plan_of
    calls = [_DeviceCall(be, fx, m, mode, ws, s, launch=False) for m in (first, second, first, second, first)]   # five: the ring of four wraps
    for c in calls:              # every input is on the device already: nothing but the calls themselves from here on
        c.launch()
    for c, m, tag in zip(calls, (first, second, first, second, first), ("rejects", "clean", "rejects", "clean", "rejects")):
        assert c.results() == (m.expected, _want_status(fx, tag, m))
    ws.close()


# ---- 7
def test_misuse_is_an_argument_error(be, fx):
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    mix = fx["mix"]
    ws = be.Workspace.multi(fx["plans"], mix.n)
    # plans on two SRS: a built-in key beside the moved ones
    own = be.DevicePlan(PL.compile_plan(V.simple_mul_vk()[0]).to_bytes(), 0)
    with pytest.raises(be.H2VError, match=r"h2v error -1.*plans\[0\] and plans\[5\].*SRS"):
        _host(be, fx, mix, "per-proof", ws, plans=fx["plans"] + [own])
    # plan_of out of range
    bad = Mix(fx["keys"], fx["rejects"], mix.order[:6])
    bad.plan_of[4] = len(LISTED)
    with pytest.raises(be.H2VError, match=r"h2v error -1.*plan_of\[4\] = 5"):
        _host(be, fx, bad, "per-proof", ws)
    # a workspace made for simple_mul alone
    small = be.Workspace(fx["keys"]["simple_mul"]["dp"], mix.n)
    with pytest.raises(be.H2VError, match=r"h2v error -1.*plans\[\d\].*workspace"):
        _host(be, fx, mix, "rlc", small)
    # a workspace smaller than the call
    tiny = be.Workspace.multi(fx["plans"], 100)
    with pytest.raises(be.H2VError, match=r"h2v error -1.*too small"):
        _host(be, fx, mix, "per-proof", tiny)
    # more plans than H2V_MIXED_MAX_PLANS
    with pytest.raises(be.H2VError, match="h2v error -4"):
        _host(be, fx, mix, "per-proof", ws, plans=[fx["plans"][0]] * (be.MIXED_MAX_PLANS + 1))
    # exactly H2V_MIXED_MAX_PLANS is fine (the same key listed again and again is one SRS)
    acc, _st, _fb = _host(be, fx, Mix(fx["keys"], fx["rejects"], [("simple_mul", 0)]), "per-proof", ws, plans=[fx["plans"][0]] * be.MIXED_MAX_PLANS)
    assert acc == [fx["rejects"]["simple_mul"].expected[0]]
    # nothing above has broken the workspace
    assert _host(be, fx, mix, "per-proof", ws)[0] == mix.expected
    for w in (ws, small, tiny):
        w.close()


# ---- 8
def test_cpp_driver(be, fx, tmp_path):
    out = str(tmp_path / "h2v_mixed_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    import struct
    mix = Mix(fx["keys"], fx["rejects"], fx["mix"].order[:24])
    assert len(set(mix.plan_of)) >= 3 and 0 < sum(mix.expected) < mix.n
    paths = []
    for k, name in enumerate(LISTED):
        e = fx["keys"][name]
        path = str(tmp_path / ("%s.%s" % (name, "json" if k % 2 else "bin")))      # both forms of a key
        with open(path, "wb") as f:
            f.write(e["vk"].to_json().encode() if k % 2 else e["pl"].to_bytes())
        paths.append(path)
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    blob = struct.pack("<I", mix.n)
    for name, j in mix.order:
        b, e = fx["rejects"][name], fx["keys"][name]
        n_pi = e["vk"].n_public_inputs
        p = b.proof(j)
        blob += struct.pack("<II", LISTED.index(name), len(p)) + p + struct.pack("<I", n_pi) + b.instances[32 * n_pi * j:32 * n_pi * (j + 1)]
        blob += struct.pack("<I", 1) + b.ci(j) if b.committed is not None else struct.pack("<I", 0)
    with open(str(tmp_path / "batch.bin"), "wb") as f:
        f.write(blob)
    r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / "batch.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    acc, st, fb = _host(be, fx, mix, "rlc")
    bits = "".join(str(a) for a in acc)
    assert got["per_proof"] == got["rlc"] == bits
    assert [int(x) for x in got["status"].split()] == st
    assert got["rlc_fell_back"] == str(int(fb))
    assert got["batch_verify"] == str(next(s for a, s in zip(acc, st) if not a))
    assert got["workspace"] == "1"
