"""What a workspace allocates and what it gives back.  The library counts, per device, the device blocks, device bytes, pinned
blocks, pinned bytes and events its owners hold (h2v_probe_device_memory); the size tables are host code
(csrc/h2v_ws_layout.hpp, asked through tests/cpp/h2v_ws_layout.cpp).  For the creation of every kind of workspace and the first
call of every set that is created on demand, the change of the five counters equals the tables' sum for that shape - and the
verdicts of the same calls equal the oracle's, so a mis-sized buffer shows as a wrong answer and not only as a wrong count.
h2v_workspace_free gives everything back, h2v_shutdown too.

profiles/workspace_memory_refactor.json holds the same changes as the parent of the owner refactor made them (its allocation
calls counted by a macro): the expected values here equal them case by case.

Keys: simple_mul, the smallest recursive key (ivc) and the smallest wide key (bls12381); capacity 65, and 260 for the group stage."""
import json
import os
import subprocess
import sys

import pytest

from plutus_halo2_verifier_gen_amd import synth
from tests.test_gpu_parity import _permute, be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 65
SEED = bytes(range(3, 35))
MEASURED = {}      # case -> the five changes as measured, in the order the cases ran (a recording run reads it)
with open(os.path.join(ROOT, "profiles", "workspace_memory_refactor.json")) as _f:
    PARENT = json.load(_f)["parent_counter_changes"]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """sum of the named sets' counter changes: tables('rlc,65,10,6', 'stats') -> (blocks, bytes, pinned blocks, pinned bytes, events)"""
    exe = str(tmp_path_factory.mktemp("wsl") / "h2v_ws_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "h2v_ws_layout.cpp"), "-o", exe])

    def ask(*specs):
        specs = [s for s in specs if s]
        if not specs:
            return (0,) * 5
        out = subprocess.run([exe] + list(specs), capture_output=True, text=True, check=True).stdout.split("\n")
        rows = [[int(v) for v in line.split()] for line in out if line]
        assert len(rows) == len(specs), out
        return tuple(sum(r[k] for r in rows) for k in range(5))
    return ask


def _facts(pl):
    """the shape facts of a plan as the loader states them: (terms, main terms, slots, ivc, fix, width, n_var, n_fix)"""
    kinds = [k for k, _ in pl.terms]
    ivc = 1 if pl.is_recursive else 0
    n_var = kinds.index(1) if 1 in kinds else len(kinds)
    tail = not ivc and n_var < len(kinds) and all(k == 1 for k in kinds[n_var:])
    n_var, n_fix = (n_var, len(kinds) - n_var) if tail else (0, 0)
    f = pl.n_terms - pl.n_main_terms - 1 if ivc and pl.n_terms > pl.n_main_terms + 1 else 0
    return {"terms": pl.n_terms, "main": pl.n_main_terms, "slots": len(pl.points) + pl.n_ci + 2 * ivc, "ivc": ivc, "fix": 1 if n_fix else 0,
            "width": max(pl.n_main_terms, f), "n_var": n_var, "n_fix": n_fix}


def _pipeline(f, cap):
    return "pipeline,%d,%d,%d,0,0,%d,%d,%d,%d" % (f["terms"], f["main"], f["slots"], f["ivc"], f["fix"], f["width"], cap)


def _union(a, b):
    u = {k: max(a[k], b[k]) for k in ("terms", "main", "slots", "ivc", "fix", "width")}
    return u


def _grown(need):
    return "grown,%d" % need


@pytest.fixture(scope="module")
def keys(be, orc):  # noqa: F811
    """name -> plan, device plan, oracle key, a batch of CAP proofs with rejects and the oracle's verdicts on it.  simple_mul and
    lookup_table are on one SRS (the mixed calls)."""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    out = {}
    for name, build, common in (("simple_mul", V.BUILDERS["simple_mul"], True), ("lookup_table", V.BUILDERS["lookup_table"], True),
                                ("ivc", V.BUILDERS["ivc"], False), ("bls12381", V.WIDE_BUILDERS["bls12381"], False)):
        vk, td = build()
        if common:
            vk, td = V.on_srs(vk, td, COMMON_S)
        pl = PL.compile_plan(vk)
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        clean = synth.forge_batch(vk, td, CAP, seed=7, plan=pl, workers=8)
        rej = synth.with_rejects(pl, clean, vk.n_public_inputs, fraction=0.2, seed=9, kinds=["flip_first_scalar", "point_not_on_curve"])
        want = list(ov.verify_batch(rej.proofs, rej.proof_off, rej.instances, rej.committed, threads=8))
        assert want == rej.expected and 0 < sum(want) < CAP, name
        out[name] = {"vk": vk, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0), "ov": ov, "clean": clean, "rej": rej, "want": want, "f": _facts(pl)}
    return out


class Dev:
    """a batch on the device and its output buffers"""

    def __init__(self, b):
        import torch
        dev = torch.device("cuda", 0)
        t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
        self.n = b.n
        self.keep = [t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed)]
        self.acc = torch.full((b.n,), 7, dtype=torch.uint8, device=dev)
        self.pair = torch.zeros(96, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()

    def ptrs(self):
        return [x.data_ptr() if x is not None else None for x in self.keep]

    def accept(self):
        self.stream.synchronize()
        return list(self.acc.cpu().tolist())


def _measure(be, case, fn):  # noqa: F811
    before = be.probe_device_memory(0)
    out = fn()
    after = be.probe_device_memory(0)
    MEASURED[case] = [a - b for a, b in zip(after, before)]
    return tuple(MEASURED[case]), out


def _hold(case, got, want):
    """the measured change is the tables' sum, and that is what the parent allocated"""
    assert got == want, (case, got, want)
    assert list(want) == PARENT[case], (case, want, PARENT[case])


def _closed(be, ws, before):  # noqa: F811
    ws.close()
    assert be.probe_device_memory(0) == before


@pytest.mark.parametrize("name", ["simple_mul", "ivc", "bls12381"])
def test_an_ordinary_workspace_is_its_pipeline_table(be, keys, tables, name):  # noqa: F811
    e = keys[name]
    before = be.probe_device_memory(0)
    got, ws = _measure(be, "create/" + name, lambda: be.Workspace(e["dp"], CAP))
    _hold("create/" + name, got, tables(_pipeline(e["f"], CAP)))
    d = Dev(e["rej"])
    e["dp"].verify_batch_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream)
    assert d.accept() == e["want"]
    _closed(be, ws, before)


def test_lanes_are_created_on_first_use(be, keys, tables):  # noqa: F811
    e = keys["simple_mul"]
    before = be.probe_device_memory(0)
    lane = ("events,1", _pipeline(e["f"], 16))
    got, ws = _measure(be, "create_lanes", lambda: be.Workspace(e["dp"], CAP, lanes=3, chunk=16))
    _hold("create_lanes", got, tables("laned,%d" % CAP, *lane))
    d = Dev(e["rej"])
    got, _ = _measure(be, "create_lanes/first_call", lambda: e["dp"].verify_batch_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream))
    assert d.accept() == e["want"]
    _hold("create_lanes/first_call", got, tables(*(lane + lane)))      # five chunks of 16 go round three lanes: two more
    _closed(be, ws, before)


def test_a_multi_plan_workspace_is_sized_for_the_union(be, keys, tables):  # noqa: F811
    a, b = keys["simple_mul"], keys["bls12381"]
    before = be.probe_device_memory(0)
    got, ws = _measure(be, "create_multi", lambda: be.Workspace.multi([a["dp"], b["dp"]], CAP, lanes=2, chunk=16))
    _hold("create_multi", got, tables("laned,%d" % CAP, "events,1", _pipeline(_union(a["f"], b["f"]), 16)))
    for e in (a, b):
        d = Dev(e["rej"])
        e["dp"].verify_batch_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream)
        assert d.accept() == e["want"], e["vk"].name
    _closed(be, ws, before)


def _rlc_call(e, d, ws, **kw):
    e["dp"].verify_batch_rlc_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream, seed=SEED, **kw)


def test_batch_accept_sets(be, keys, tables):  # noqa: F811
    """the first batch-accept call, the first aggregate call and the first batch form of the pair check on one workspace: each adds
    what the calls before it have not created"""
    e, f = keys["simple_mul"], keys["simple_mul"]["f"]
    rlc = "rlc,%d,%d,%d" % (CAP, f["n_var"], f["n_fix"])
    before = be.probe_device_memory(0)
    ws = be.Workspace(e["dp"], CAP)
    d = Dev(e["rej"])
    got, _ = _measure(be, "rlc", lambda: _rlc_call(e, d, ws))
    assert d.accept() == e["want"]
    _hold("rlc", got, tables(rlc, "stats"))
    # an aggregate call: sixteen slot events and the parts of sixteen slots of 128 parts
    d = Dev(e["clean"])
    got, _ = _measure(be, "aggregate", lambda: e["dp"].aggregate_batch_device(d.n, *d.ptrs(), d.pair.data_ptr(), d.acc.data_ptr(), None, ws=ws,
                                                                              stream=d.stream.cuda_stream, seed=SEED))
    assert d.accept() == [1] * CAP
    assert list(e["dp"].check_pairs(bytes(d.pair.cpu().tolist()))[0]) == [1]          # (a temporary workspace: nothing of it stays)
    _hold("aggregate", got, tables("events,16", _grown(16 * 128 * 72 * 4)))
    # the batch form of the pair check over every proof's pair: the two-slot view and the pair shape of the RLC set
    import torch
    pairs, _st = e["dp"].prepare_batch(e["rej"].proofs, e["rej"].proof_off, e["rej"].instances, e["rej"].committed)
    d = Dev(e["rej"])
    d_pairs = torch.frombuffer(bytearray(pairs), dtype=torch.uint8).to(d.acc.device)
    torch.cuda.synchronize()
    got, _ = _measure(be, "check_pairs_rlc", lambda: e["dp"].check_pairs_rlc_device(d.n, d_pairs.data_ptr(), d.acc.data_ptr(), None, ws=ws,
                                                                                    stream=d.stream.cuda_stream, seed=SEED))
    assert d.accept() == e["want"]
    _hold("check_pairs_rlc", got, tables("pairview,%d" % CAP, "pairs,%d" % CAP))
    _closed(be, ws, before)


def test_a_derived_seed_has_its_ring_and_digests(be, keys, tables):  # noqa: F811
    """the first call of a workspace (no estimate routes it past the batch check yet): beside the batch-accept sets the ring, the
    digests of 65 leaves + 2 + 1 nodes and the two events of the call's slot"""
    e, f = keys["simple_mul"], keys["simple_mul"]["f"]
    before = be.probe_device_memory(0)
    ws = be.Workspace(e["dp"], CAP)
    d = Dev(e["rej"])
    got, _ = _measure(be, "rlc/derived_seed", lambda: e["dp"].verify_batch_rlc_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream,
                                                                                      derive_seed=True))
    assert d.accept() == e["want"] and len(ws.seed_used()) == 32
    _hold("rlc/derived_seed", got, tables("rlc,%d,%d,%d" % (CAP, f["n_var"], f["n_fix"]), "stats", "seedring", _grown((CAP + 2 + 1) * 32), "events,2"))
    _closed(be, ws, before)


def test_the_fold_pool_of_a_recursive_key(be, keys, tables):  # noqa: F811
    e = keys["ivc"]
    before = be.probe_device_memory(0)
    ws = be.Workspace(e["dp"], CAP)
    d = Dev(e["rej"])
    got, _ = _measure(be, "rlc/fold_pairs", lambda: _rlc_call(e, d, ws, fold_pairs=True))
    assert d.accept() == e["want"]
    _hold("rlc/fold_pairs", got, tables("pairs,%d" % CAP, "pairpool,%d" % CAP, "stats", "events,12"))
    _closed(be, ws, before)


def test_the_group_stage_by_one_rejecting_proof_among_260(be, keys, tables):  # noqa: F811
    e, f = keys["simple_mul"], keys["simple_mul"]["f"]
    n, bad = 260, e["want"].index(0)
    good = [i for i, a in enumerate(e["want"]) if a]
    order = [good[i % len(good)] for i in range(n)]
    order[201] = bad
    b = _permute(e["rej"], order, e["vk"].n_public_inputs)
    before = be.probe_device_memory(0)
    ws = be.Workspace(e["dp"], n)
    d = Dev(b)
    got, _ = _measure(be, "rlc/group_stage", lambda: _rlc_call(e, d, ws))
    assert d.accept() == [0 if i == 201 else 1 for i in range(n)]
    _hold("rlc/group_stage", got, tables("rlc,%d,%d,%d" % (n, f["n_var"], f["n_fix"]), "stats", "group,%d,%d" % ((n + 63) // 64, 64 * f["n_var"] + f["n_fix"])))
    _closed(be, ws, before)


def test_a_coalesced_call_stages_in_its_lane(be, keys, tables):  # noqa: F811
    e = keys["simple_mul"]
    before = be.probe_device_memory(0)
    ws = be.Workspace(e["dp"], 128, lanes=2, chunk=64)
    ws.defer_joins(True)
    b = _permute(e["rej"], list(range(20)), e["vk"].n_public_inputs)
    d = Dev(b)
    got, _ = _measure(be, "coalesced", lambda: e["dp"].verify_batch_device(d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream))
    ws.join(d.stream.cuda_stream)
    assert d.accept() == e["want"][:20]
    _hold("coalesced", got, tables("coalesce,64,%d,%d" % (e["pl"].proof_len, e["pl"].n_pi)))
    _closed(be, ws, before)


class DevMix(Dev):
    """proofs of simple_mul and lookup_table, alternating, as one mixed batch on the device"""

    def __init__(self, keys, tag, n):
        names = ("simple_mul", "lookup_table")
        self.plan_of = [i % 2 for i in range(n)]
        self.count = [self.plan_of.count(0), self.plan_of.count(1)]
        proofs, inst, off, self.want = [], [], [0], []
        for i in range(n):
            e = keys[names[i % 2]]
            b, j, n_pi = e[tag], i // 2, e["vk"].n_public_inputs
            proofs.append(b.proof(j))
            off.append(off[-1] + len(proofs[-1]))
            inst.append(b.instances[32 * n_pi * j:32 * n_pi * (j + 1)])
            self.want.append(b.expected[j])

        class B:
            pass
        m = B()
        m.n, m.proofs, m.proof_off, m.instances, m.committed = n, b"".join(proofs), off, b"".join(inst), None
        Dev.__init__(self, m)
        pls = [keys[nm]["pl"] for nm in names]
        self.proof_cap = sum(c * pl.proof_len for c, pl in zip(self.count, pls))
        self.inst_total = sum(c * pl.n_pi * 32 for c, pl in zip(self.count, pls))
        # the fold layout of the call on an ordinary workspace: every proof's terms, every VK base, per plan the sums of its blocks of 64
        fs = [keys[nm]["f"] for nm in names]
        self.n_r = sum(c * f["n_var"] + f["n_fix"] for c, f in zip(self.count, fs))
        self.n_parts = sum((c + 63) // 64 * f["n_fix"] for c, f in zip(self.count, fs))

    def staging(self):
        return (_grown(self.proof_cap + 64), _grown(self.inst_total + 64), _grown(64))


def test_mixed_calls_and_the_fold_pool_that_grows(be, keys, tables):  # noqa: F811
    plans = [keys["simple_mul"]["dp"], keys["lookup_table"]["dp"]]
    before = be.probe_device_memory(0)
    ws = be.Workspace(keys["lookup_table"]["dp"], CAP)       # (the larger of the two in every dimension)

    def call(d, **kw):
        be.verify_mixed_device(plans, d.plan_of, d.n, *d.ptrs(), d.acc.data_ptr(), None, ws=ws, stream=d.stream.cuda_stream, **kw)

    d = DevMix(keys, "rej", 20)
    got, _ = _measure(be, "mixed", lambda: call(d))
    assert d.accept() == d.want
    _hold("mixed", got, tables("mixed,%d" % CAP, *d.staging(), "tabslot,20,0", "pairview,%d" % CAP))
    # a fold call (the second table slot), then a larger one (the third): the staging and the term pool grow
    d1 = DevMix(keys, "clean", 20)
    got, _ = _measure(be, "mixed/fold", lambda: call(d1, mode="rlc", seed=SEED, fold_msm=True))
    assert d1.accept() == [1] * 20
    _hold("mixed/fold", got, tables("stats", "fold,%d,%d,%d,0,0" % (CAP, d1.n_r, d1.n_parts), "tabslot,20,2"))
    d2 = DevMix(keys, "clean", CAP)
    got, _ = _measure(be, "mixed/fold_grows", lambda: call(d2, mode="rlc", seed=SEED, fold_msm=True))
    assert d2.accept() == [1] * CAP
    have_t, have_p = d1.n_r + d1.n_r // 4, d1.n_parts + d1.n_parts // 4 + 1
    grow = [a - b for a, b in zip(tables(*d2.staging(), "fold,%d,%d,%d,%d,%d" % (CAP, d2.n_r, d2.n_parts, have_t, have_p), "tabslot,%d,2" % CAP),
                                  tables(*d.staging(), "fold,%d,%d,%d,0,0" % (CAP, d1.n_r, d1.n_parts)))]
    _hold("mixed/fold_grows", got, tuple(grow))
    _closed(be, ws, before)


def test_shutdown_leaves_nothing_and_the_handles_free_as_empty_shells():
    """in a child process: plans and workspaces (an ordinary one with its batch-accept sets, a laned one) are live at h2v_shutdown;
    afterwards the five counters are zero, and freeing the handles changes nothing and does not fault"""
    script = (
        "import sys; sys.path.insert(0, %r)\n"
        "import torch\n"
        "from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V\n"
        "vk, td = V.simple_mul_vk()\n"
        "pl = PL.compile_plan(vk)\n"
        "b = synth.forge_batch(vk, td, 8, seed=4, plan=pl, workers=1)\n"
        "assert backend.probe_device_memory(0) == (0, 0, 0, 0, 0)\n"
        "dp = backend.DevicePlan(pl.to_bytes(), 0)\n"
        "ws, laned = backend.Workspace(dp, 8), backend.Workspace(dp, 8, lanes=2, chunk=4)\n"
        "acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws)\n"
        "assert list(acc) == b.expected and not fb\n"
        "assert list(dp.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=laned)) == b.expected\n"
        "live = backend.probe_device_memory(0)\n"
        "assert min(live) > 0, live\n"
        "backend.shutdown(0)\n"
        "assert backend.probe_device_memory(0) == (0, 0, 0, 0, 0), backend.probe_device_memory(0)\n"
        "ws.close(); laned.close(); dp.close()\n"
        "assert backend.probe_device_memory(0) == (0, 0, 0, 0, 0)\n"
        "print('nothing left')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nothing left" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
