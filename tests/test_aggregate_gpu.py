"""GPU tests of the aggregate calls (include/h2v.h: h2v_aggregate_batch / h2v_aggregate_mixed): one pair (L, R) per batch instead
of a pairing on it.  Every expected pair is the big-integer model's (tests/agg_model.py) over the CPU oracle's el / er per proof
under the seed and chunking the call's h2v_aggregate_info reports - bit for bit; included[] is the oracle's "reached the pairing",
status[] is h2v_prepare_batch's.  Every call gives its seed (H2V_RLC_SEED_GIVEN).  /root/reference is NOT needed."""
import json
import random
import types

import pytest

from plutus_halo2_verifier_gen_amd import synth
from tests import agg_model
from tests.test_batch_cancellation_gpu import _pair, _single, cx  # noqa: F401  (cx: keys on one SRS with eight clean proofs each)
from tests.test_gpu_parity import _permute, be, circuits  # noqa: F401  (module fixtures)
from tests.test_mixed_keys import COMMON_S
from tests.test_mixed_keys_gpu import Mix
from tests.test_prepare_pairs_gpu import _dev, _oracle

pytestmark = pytest.mark.gpu
GIVEN = bytes(range(100, 132))
INF_PAIR = (b"\xc0" + bytes(47)) * 2
SIZES = [1, 2, 63, 64, 65, 130]
# rejects of the 130-proof batch: every prefix in SIZES holds the wrong_pi proof at 0 (included; only the pair refuses it), and
# pre-pairing rejects sit on both sides of the 64-proof block borders of k_rlc_prepare
REJECTS = {0: "wrong_pi", 1: "bad_point_flag", 5: "noncanonical_scalar", 62: "truncated", 63: "wrong_public_input", 64: "point_not_in_subgroup",
           65: "wrong_pi", 100: "bad_point_flag", 129: "wrong_public_input"}


def _corrupted(pl, batch, n_pi, kinds):
    """batch with proof i corrupted as kinds[i] says"""
    proofs = [batch.proof(i) for i in range(batch.n)]
    insts = [batch.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(batch.n)]
    expected = list(batch.expected)
    for i, kind in kinds.items():
        proofs[i], insts[i] = synth.corrupt(pl, proofs[i], insts[i], kind, random.Random(1000 + i))
        expected[i] = 0
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return synth.Batch(n=batch.n, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=batch.committed, expected=expected)


@pytest.fixture(scope="module")
def sm(be, orc, circuits):
    """simple_mul: 130 accepting proofs, the same with REJECTS, and the oracle's (verdict, pair) of every proof of both - computed
    once, shared, never changed"""
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n_pi = vk.n_public_inputs
    clean = synth.forge_batch(vk, td, 130, seed=71, plan=pl, workers=8)
    rej = _corrupted(pl, clean, n_pi, REJECTS)
    want = {"clean": _oracle(ov, orc, clean, n_pi), "rej": _oracle(ov, orc, rej, n_pi)}
    assert [a for a, _ in want["clean"]] == [1] * 130 and [a for a, _ in want["rej"]] == rej.expected
    reached = [int(p != bytes(96)) for _, p in want["rej"]]
    assert reached[0] == 1 and reached[65] == 1 and reached[63] == 1 and sum(reached) == 130 - 5      # wrong_pi / wrong_public_input reach the pairing
    return {"vk": vk, "td": td, "pl": pl, "dp": dp, "ov": ov, "n_pi": n_pi, "clean": clean, "rej": rej, "want": want}


def _host(dp, b, ws=None, seed=GIVEN):
    pair, inc, st, info = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, seed=seed)
    return pair, list(inc), st, info


def _prep(b):
    """the batch and the outputs of one device-form call on the device (the caller synchronises before it launches)"""
    import torch
    d = _dev(b)
    dev = d["dev"]
    return {"d": d, "n": b.n, "pair": torch.full((96,), 7, dtype=torch.uint8, device=dev), "inc": torch.full((b.n,), 7, dtype=torch.uint8, device=dev),
            "st": torch.full((b.n,), -1, dtype=torch.int32, device=dev)}


def _launch(dp, p, ws, stream, seed=GIVEN):
    d = p["d"]
    ptr = lambda x: x.data_ptr() if x is not None else None
    return dp.aggregate_batch_device(p["n"], ptr(d["proofs"]), ptr(d["off"]), ptr(d["inst"]), ptr(d["ci"]), p["pair"].data_ptr(), p["inc"].data_ptr(),
                                     p["st"].data_ptr(), ws=ws, stream=stream.cuda_stream, seed=seed)


def _device(dp, b, ws, seed=GIVEN, stream=None, sync=True):
    import torch
    p = _prep(b)
    s = stream or torch.cuda.Stream(device=p["d"]["dev"])
    torch.cuda.synchronize()
    info = _launch(dp, p, ws, s, seed)
    pair, inc, st = p["pair"], p["inc"], p["st"]
    if not sync:
        return (pair, inc, st, info, p, s)
    s.synchronize()
    return bytes(pair.cpu().numpy().tobytes()), inc.cpu().tolist(), [v & 0xffffffff for v in st.cpu().tolist()], info


def _assert_model(got, want, tag):
    """got = (pair, included, status, info) of a call; want = the oracle's [(verdict, pair)] of its proofs"""
    pair, inc, st, info = got
    reached = [int(p != bytes(96)) for _, p in want]
    assert inc == reached, tag
    assert pair == agg_model.model_pair([p for _, p in want], reached, bytes(info.seed_used), info.chunk), tag
    assert [int(s == 0) for s in st] == reached, tag            # (H2V_ST_PAIRING is never set: status 0 = included)


# ---- 1
@pytest.mark.parametrize("n", SIZES)
def test_pair_is_the_models_bit_for_bit(be, sm, n):
    """an ordinary workspace, host and device forms, with rejects of both kinds mixed in and all-accepting"""
    dp, n_pi, s = sm["dp"], sm["n_pi"], sm["td"].s
    ws = be.Workspace(dp, n)
    assert ws.lanes() == (1, n)
    seeds = set()
    for tag in ("rej", "clean"):
        b, want = _permute(sm[tag], list(range(n)), n_pi), sm["want"][tag][:n]
        _raw, pst = dp.prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
        for form, got in (("host", _host(dp, b, ws)), ("device", _device(dp, b, ws)), ("host, temporary workspace", _host(dp, b))):
            pair, inc, st, info = got
            _assert_model(got, want, (tag, form, n))
            assert st == pst, (tag, form)                       # what h2v_prepare_batch reports
            assert (info.chunk, info.n_chunks) == (0, 1) and info.msm_terms > n
            assert bytes(info.seed_used)[:20] == GIVEN[:20] and bytes(info.seed_used)[28:] == GIVEN[28:]      # (the call count moves words 5 and 6 only)
            seeds.add(bytes(info.seed_used))
            acc, cst = dp.check_pairs(pair)
            if tag == "clean":
                assert agg_model.holds(pair, s) and pair != INF_PAIR
                assert (list(acc), cst) == ([1], [0])
            else:
                # the wrong_pi proof at position 0 is included and nothing but the pair's equation refuses it
                assert inc[0] == 1 and st[0] == 0 and not agg_model.holds(pair, s)
                assert (list(acc), cst) == ([0], [be.ST_PAIRING])
    assert len(seeds) == 6                                      # every seeded call draws other coefficients
    ws.close()


# ---- 2
@pytest.mark.parametrize("chunk,lanes", [(128, 2), (64, 3), (2, 4)])
def test_chunks_of_a_laned_workspace(be, sm, chunk, lanes):
    """130 proofs in 2, 3 and 65 chunks (more parts than a wave has lanes): every chunk draws its own coefficients, the export adds the parts"""
    dp, b, want = sm["dp"], sm["rej"], sm["want"]["rej"]
    ws = be.Workspace(dp, 130, lanes=lanes, chunk=chunk)
    for form, got in (("device", _device(dp, b, ws)), ("host", _host(dp, b, ws))):
        _assert_model(got, want, (chunk, form))
        info = got[3]
        assert (info.chunk, info.n_chunks) == (chunk, -(-130 // chunk))
    ws.close()


def test_chunk_edges_multi_plan_and_deferred_joins(be, sm, circuits):
    import torch
    dp, pl, n_pi, clean = sm["dp"], sm["pl"], sm["n_pi"], sm["clean"]
    # the middle chunk of three holds only pre-pairing rejects: one part is infinity on both sides
    mid = _corrupted(pl, clean, n_pi, {i: "bad_point_flag" for i in range(64, 128)})
    want_mid = [(1, p) if i < 64 or i >= 128 else (0, bytes(96)) for i, (_, p) in enumerate(sm["want"]["clean"])]
    ws = be.Workspace(dp, 130, lanes=3, chunk=64)
    got = _device(dp, mid, ws)
    _assert_model(got, want_mid, "middle chunk")
    assert got[1][64:128] == [0] * 64 and agg_model.holds(got[0], sm["td"].s) and got[0] != INF_PAIR
    # every proof rejected before the pairing: (inf, inf), nothing included - which h2v_check_pairs accepts
    none = _corrupted(pl, clean, n_pi, {i: "noncanonical_scalar" for i in range(130)})
    for w in (ws, be.Workspace(dp, 130)):
        pair, inc, st, info = _device(dp, none, w)
        assert pair == INF_PAIR and inc == [0] * 130 and all(v & be.ST_BAD_SCALAR for v in st)
        assert [list(v) for v in dp.check_pairs(pair)] == [[1], [0]]
    ws.close()
    # a multi-plan workspace
    multi = be.Workspace.multi([dp, circuits["sha256"][3]], 512, lanes=2, chunk=100)
    got = _device(dp, sm["rej"], multi)
    _assert_model(got, sm["want"]["rej"], "multi")
    assert (got[3].chunk, got[3].n_chunks) == (100, 2)
    multi.close()
    # deferred joins, small verify calls still gathered when the aggregate call arrives: their verdicts are intact, the pair is right
    ws = be.Workspace(dp, 1024, lanes=0, chunk=512)
    ws.defer_joins(True)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    held = []
    for lo in (0, 50):
        sub = _permute(sm["rej"], list(range(lo, lo + 50)), n_pi)
        db = _dev(sub)
        acc = torch.full((50,), 7, dtype=torch.uint8, device=dev)
        dp.verify_batch_device(50, db["proofs"].data_ptr(), db["off"].data_ptr(), db["inst"].data_ptr(), None, acc.data_ptr(), None, ws=ws, stream=s.cuda_stream)
        held.append((sub, db, acc))
    with pytest.raises(be.H2VError):          # the NULL-stream rule of deferred joins
        dp.aggregate_batch_device(50, db["proofs"].data_ptr(), db["off"].data_ptr(), db["inst"].data_ptr(), None, acc.data_ptr(), acc.data_ptr(), None, ws=ws, stream=None)
    pair, inc, st, info, keep, _s = _device(dp, sm["rej"], ws, stream=s, sync=False)
    ws.join(s.cuda_stream)
    s.synchronize()
    got = (bytes(pair.cpu().numpy().tobytes()), inc.cpu().tolist(), [v & 0xffffffff for v in st.cpu().tolist()], info)
    _assert_model(got, sm["want"]["rej"], "deferred")
    assert (info.chunk, info.n_chunks) == (512, 1)             # one chunk, and it is chunk 0: its tweak applies
    for sub, _db, acc in held:
        assert acc.cpu().tolist() == sub.expected
    ws.close()


def test_calls_on_several_streams_share_one_workspace(be, sm):
    """twenty calls in flight on three caller streams of one deferring laned workspace - more calls than the parts buffer has slots,
    of three geometries (1, 2 and 3 chunks) - and nothing synchronised in between: every pair is its own call's"""
    dp, n_pi = sm["dp"], sm["n_pi"]
    import torch
    ws = be.Workspace(dp, 1024, lanes=4, chunk=64)
    ws.defer_joins(True)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(3)]
    calls = []
    for k in range(20):
        lo, n = (7 * k) % 60, (64 if k % 3 else 130 - (7 * k) % 60)
        calls.append((lo, n, _prep(_permute(sm["rej"], list(range(lo, lo + n)), n_pi))))
    torch.cuda.synchronize()
    infos = [_launch(dp, p, ws, streams[k % 3]) for k, (_lo, _n, p) in enumerate(calls)]
    torch.cuda.synchronize()
    for (lo, n, p), info in zip(calls, infos):
        got = (bytes(p["pair"].cpu().numpy().tobytes()), p["inc"].cpu().tolist(), [v & 0xffffffff for v in p["st"].cpu().tolist()], info)
        _assert_model(got, sm["want"]["rej"][lo:lo + n], (lo, n))
        assert (info.chunk, info.n_chunks) == (64, -(-n // 64))
    ws.close()
    # calls of MORE parts than a slot holds (130 chunks of one proof: the whole parts buffer) between small ones (3 .. 9 parts: one
    # slot each), on three streams, nothing synchronised in between: a large call waits for every export before it and every
    # later call for the large call's
    ws = be.Workspace(dp, 130, lanes=4, chunk=1)
    ws.defer_joins(True)
    calls = []
    for k in range(9):
        lo, n = (0, 130) if k % 3 == 1 else (11 * k, 3 + k)
        calls.append((lo, n, _prep(_permute(sm["rej"], list(range(lo, lo + n)), n_pi))))
    torch.cuda.synchronize()
    infos = [_launch(dp, p, ws, streams[k % 3]) for k, (_lo, _n, p) in enumerate(calls)]
    torch.cuda.synchronize()
    for (lo, n, p), info in zip(calls, infos):
        got = (bytes(p["pair"].cpu().numpy().tobytes()), p["inc"].cpu().tolist(), [v & 0xffffffff for v in p["st"].cpu().tolist()], info)
        _assert_model(got, sm["want"]["rej"][lo:lo + n], ("one-proof chunks", lo, n))
        assert (info.chunk, info.n_chunks) == (1, n)
    ws.close()


# ---- 3
def test_every_key_kind_once(be, orc, circuits):
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    # a recursive key: the H2V_RLC_FOLD_PAIRS route, flag or not; acc_vk_hash is excluded with H2V_ST_RECURSION, acc_scalar as the oracle has it
    vk, td, pl, dp, ov = circuits["ivc"]
    n_pi = vk.n_public_inputs
    b = _corrupted(pl, synth.forge_batch(vk, td, 5, seed=72, plan=pl, workers=4), n_pi, {1: "acc_vk_hash", 3: "acc_scalar"})
    want = _oracle(ov, orc, b, n_pi)
    assert [a for a, _ in want] == b.expected and want[1][1] == bytes(96)
    _raw, pst = dp.prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
    for ws in (be.Workspace(dp, 5), be.Workspace(dp, 5, lanes=2, chunk=2)):
        for got in (_device(dp, b, ws), _host(dp, b, ws)):
            _assert_model(got, want, "ivc")
            assert got[2] == pst and got[2][1] == be.ST_RECURSION and got[1][1] == 0
            assert got[3].msm_terms == 5                        # one pair per proof
        ws.close()
    # a wide key (a main sum of more than 64 terms)
    name = sorted(V.WIDE_BUILDERS)[0]
    wvk, wtd = V.WIDE_BUILDERS[name]()
    wpl = PL.compile_plan(wvk)
    wdp = be.DevicePlan(wpl.to_bytes(), 0)
    wov = orc.OracleVK(orc.vk_desc(json.loads(wvk.to_json()), wvk.omega, wvk.omega_inv, wvk.barycentric_weight))
    wb = synth.forge_batch(wvk, wtd, 2, seed=73, plan=wpl, workers=2)
    got = _host(wdp, wb)
    _assert_model(got, _oracle(wov, orc, wb, wvk.n_public_inputs), name)
    assert agg_model.holds(got[0], wtd.s)
    # a blake2b-512 key: the oracle replays the Cardano flavour only, so the expected pairs are h2v_prepare_batch's
    kvk, ktd = V.simple_mul_vk()
    kvk = V.with_transcript_hash(kvk, "blake2b-512", None)
    kpl = PL.compile_plan(kvk)
    kdp = be.DevicePlan(kpl.to_bytes(), 0)
    kb = synth.forge_batch(kvk, ktd, 2, seed=74, plan=kpl, workers=1)
    raw, pst = kdp.prepare_batch(kb.proofs, kb.proof_off, kb.instances, kb.committed)
    assert pst == [0, 0]
    pair, inc, st, info = _host(kdp, kb)
    assert inc == [1, 1] and st == [0, 0]
    assert pair == agg_model.model_pair([raw[:96], raw[96:]], [1, 1], bytes(info.seed_used), info.chunk)
    assert agg_model.holds(pair, ktd.s)


# ---- 4
def _mixed_host(be, plans, mix, ws=None):
    pair, inc, st, info = be.aggregate_mixed(plans, mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=ws, seed=GIVEN)
    return pair, list(inc), st, info


def _mixed_device(be, plans, mix, ws):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    keep = [t(mix.proofs), torch.tensor(mix.off, dtype=torch.int64, device=dev), t(mix.instances), t(mix.committed)]
    pair = torch.full((96,), 7, dtype=torch.uint8, device=dev)
    inc = torch.full((max(1, mix.n),), 7, dtype=torch.uint8, device=dev)
    st = torch.full((max(1, mix.n),), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    torch.cuda.synchronize()
    info = be.aggregate_mixed_device(plans, mix.plan_of, mix.n, *[ptr(x) for x in keep], pair.data_ptr(), inc.data_ptr(), st.data_ptr(), ws=ws,
                                     stream=s.cuda_stream, seed=GIVEN)
    s.synchronize()
    return bytes(pair.cpu().numpy().tobytes()), inc.cpu().tolist()[:mix.n], [v & 0xffffffff for v in st.cpu().tolist()][:mix.n], info


def _oracle_mix(cx_keys, orc, batches, mix):
    out = []
    for name, j in mix.order:
        e, b = cx_keys[name], batches[name]
        ok, otr = e["ov"].verify(b.proof(j), b.instance_ints(j, e["vk"].n_public_inputs), b.ci(j), trace=True)
        out.append((int(ok), orc.g1_compress(otr.point("el")) + orc.g1_compress(otr.point("er")) if otr.status in (0, 1) else bytes(96)))
    return out


def test_mixed_three_keys_interleaved(be, orc, cx):
    """simple_mul x 3, lookup_table x 2, ivc x 1 interleaved (trashcan_mix and atms_with_lookups listed without a proof): the pair by
    call position, included / status in the caller's order, host and device forms, ordinary and multi-plan workspaces; n = 0"""
    keys, plans = cx["keys"], cx["plans"]
    batches = dict(cx["clean"])
    batches["simple_mul"] = _corrupted(keys["simple_mul"]["pl"], batches["simple_mul"], keys["simple_mul"]["vk"].n_public_inputs, {1: "bad_point_flag"})
    batches["lookup_table"] = _corrupted(keys["lookup_table"]["pl"], batches["lookup_table"], keys["lookup_table"]["vk"].n_public_inputs, {0: "wrong_pi"})
    mix = Mix(keys, batches, [("simple_mul", 0), ("lookup_table", 0), ("simple_mul", 1), ("ivc", 0), ("lookup_table", 1), ("simple_mul", 2)])
    want = _oracle_mix(keys, orc, batches, mix)
    assert [a for a, _ in want] == [1, 0, 0, 1, 1, 1] and [int(p != bytes(96)) for _, p in want] == [1, 1, 0, 1, 1, 1]
    multi = be.Workspace.multi(plans, 64)
    for tag, got in (("host", _mixed_host(be, plans, mix)), ("host, multi", _mixed_host(be, plans, mix, multi)), ("device, multi", _mixed_device(be, plans, mix, multi))):
        _assert_model(got, want, tag)
        assert got[2] == [0, 0, be.ST_BAD_POINT, 0, 0, 0], tag
        assert (got[3].chunk, got[3].n_chunks) == (0, 1), tag   # coefficients follow the position in the call
        assert not agg_model.holds(got[0], COMMON_S)            # the wrong_pi proof is included
    assert multi.rlc_verdict() == be.BATCH_NOT_CHECKED
    # without the wrong_pi proof the call's pair holds
    good = Mix(keys, batches, [("simple_mul", 0), ("simple_mul", 1), ("ivc", 0), ("lookup_table", 1)])
    got = _mixed_device(be, plans, good, multi)
    _assert_model(got, _oracle_mix(keys, orc, batches, good), "good")
    assert agg_model.holds(got[0], COMMON_S) and [list(v) for v in keys["ivc"]["dp"].check_pairs(got[0])] == [[1], [0]]
    # n = 0
    empty = Mix(keys, batches, [])
    assert _mixed_host(be, plans, empty)[:3] == (INF_PAIR, [], [])
    assert _mixed_device(be, plans, empty, multi)[:3] == (INF_PAIR, [], [])
    multi.close()


def test_mixed_sixteen_keys_by_four(be, orc):
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    keys, batches, order = {}, {}, []
    names = ["k%02d" % k for k in range(16)]
    for k, name in enumerate(names):
        vk, td = V.on_srs(*V.simple_mul_vk(seed=0x5000 + k), COMMON_S)
        pl = PL.compile_plan(vk)
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0),
                      "ov": orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))}
        batches[name] = synth.forge_batch(vk, td, 4, seed=300 + k, plan=pl, workers=1)
    order = [(names[(3 * i) % 16], i // 16) for i in range(64)]          # interleaved: every key 4 times
    assert sorted(order) == sorted((n, j) for n in names for j in range(4))
    plans = [keys[n]["dp"] for n in names]
    # (Mix indexes LISTED; this call lists its own sixteen keys)
    mix = types.SimpleNamespace(order=order, plan_of=[names.index(n) for n, _ in order], off=[0])
    proofs, inst = [], []
    for n, j in order:
        proofs.append(batches[n].proof(j))
        mix.off.append(mix.off[-1] + len(proofs[-1]))
        inst.append(batches[n].instances[32 * 3 * j:32 * 3 * (j + 1)])
    assert keys[names[0]]["vk"].n_public_inputs == 3
    mix.n, mix.proofs, mix.instances, mix.committed = 64, b"".join(proofs), b"".join(inst), None
    want = _oracle_mix(keys, orc, batches, mix)
    assert [a for a, _ in want] == [1] * 64
    ws = be.Workspace.multi(plans, 64)
    for got in (_mixed_device(be, plans, mix, ws), _mixed_host(be, plans, mix, ws)):
        _assert_model(got, want, "16 x 4")
        assert agg_model.holds(got[0], COMMON_S)
    ws.close()


# ---- 5
def test_cancelling_errors(be, cx):
    """A', B' whose errors cancel under weights (1, 1).  In one call: the pair is refused (the two positions draw different
    coefficients).  In two calls of one Aggregator: finish() scales the calls' pairs again, rejects both proofs and verifies exactly
    those two calls again."""
    from plutus_halo2_verifier_gen_amd import api
    e = cx["keys"]["simple_mul"]
    a, b = _pair(cx, ("simple_mul", 0), ("simple_mul", 1))
    one = _single(cx, "simple_mul", 6, {1: (("simple_mul", 0), a), 4: (("simple_mul", 1), b)})
    pair, inc, st, _info = _host(e["dp"], one)
    assert inc == [1] * 6 and st == [0] * 6
    assert [list(v) for v in e["dp"].check_pairs(pair)] == [[0], [be.ST_PAIRING]]
    calls = [_single(cx, "simple_mul", 3, {1: (("simple_mul", 0), a)}), _single(cx, "simple_mul", 2, {}), _single(cx, "simple_mul", 3, {2: (("simple_mul", 1), b)})]
    agg = api.Aggregator(api.ParamsVerifierKZG(bytes.fromhex(e["vk"].s_g2)))
    for c in calls:
        agg.push(e["vk"], [c.proof(i) for i in range(c.n)], [c.instance_ints(i, 3) for i in range(c.n)])
    accepts, reverified = agg.finish()
    assert accepts == [[True, False, True], [True, True], [True, True, False]]
    assert reverified == [0, 2]


# ---- 6
def test_aggregator_end_to_end(be, orc):
    from plutus_halo2_verifier_gen_amd import api
    from tests.test_aggregate_cpp import three_pushes
    pushes = three_pushes()
    agg = api.Aggregator(api.ParamsVerifierKZG(bytes.fromhex(pushes[0][1].s_g2)))
    want = []
    for name, vk, pl, b in pushes:
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        want.append([bool(v) for v in ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4)])
        agg.push(vk, [b.proof(i) for i in range(b.n)], [b.instance_ints(i, vk.n_public_inputs) for i in range(b.n)])
    assert [sum(w) for w in want] == [69, 4, 1]
    accepts, reverified = agg.finish()
    assert accepts == want
    assert reverified == [1]
    assert agg.finish() == ([], [])
    # an empty call goes through the library too: (inf, inf), nothing included, the call's seed and n_chunks = 1 in the info
    v = api.verifier_for(pushes[0][1])
    pair, inc, st, info = v.aggregate_batch([], [], seed=GIVEN)
    assert (pair, inc, st) == (INF_PAIR, [], []) and (info.chunk, info.n_chunks, info.msm_terms) == (0, 1, 0)
    assert bytes(info.seed_used)[:20] == GIVEN[:20]
    assert be.lib().h2v_plan_same_srs(v.device_plan.handle, v.device_plan.handle) == 1


# ---- 7
@pytest.mark.parametrize("laned", [False, True])
def test_records_and_the_failing_group_estimate(be, sm, laned):
    """an aggregate call's record: not checked, no pairing time; whatever its pairs would have met, the workspace's failing-group
    estimate stays where it was - the RLC call that follows runs its batch check (a routed call reports verdict 0) and gives the
    verdicts it gives on a fresh workspace"""
    dp, n_pi = sm["dp"], sm["n_pi"]
    ws = be.Workspace(dp, 130, lanes=2, chunk=64) if laned else be.Workspace(dp, 130)
    # three groups of 64 with a failing proof in two of them: as RLC calls these would switch the next call to the per-proof kernels
    for _ in range(3):
        _device(dp, sm["rej"], ws)
        assert ws.rlc_verdict() == be.BATCH_NOT_CHECKED == 2
        ok, tm = ws.rlc_result()
        assert tm.pairing_ms == 0 and tm.total_ms > 0 and tm.bucket_accumulate_ms > 0 and tm.msm_terms > 0
    with pytest.raises(be.H2VError):
        ws.timings()                                            # a record of kind RLC, as for any batch check
    acc, fb = dp.verify_batch_rlc(sm["clean"].proofs, sm["clean"].proof_off, sm["clean"].instances, None, ws=ws, seed=GIVEN)
    assert list(acc) == [1] * 130 and not fb
    assert ws.rlc_verdict() == 1                                # the batch check ran and passed: not routed
    acc, fb = dp.verify_batch_rlc(sm["rej"].proofs, sm["rej"].proof_off, sm["rej"].instances, None, ws=ws, seed=GIVEN)
    assert list(acc) == sm["rej"].expected and fb
    ws.close()


def test_argument_errors_with_a_plan(be, sm):
    import ctypes as C
    dp = sm["dp"]
    L = be.lib()
    pair, inc = C.create_string_buffer(96), (C.c_uint8 * 4)()
    big = be.Batch((1 << 22) + 1, C.cast(pair, C.c_void_p), C.cast(pair, C.c_void_p), C.cast(pair, C.c_void_p), None)
    assert L.h2v_aggregate_batch(dp.handle, C.byref(big), pair, inc, None, None, None, None) == -4          # H2V_E_LIMIT, before anything is read
    one = be.Batch(1, C.cast(pair, C.c_void_p), C.cast(pair, C.c_void_p), C.cast(pair, C.c_void_p), None)
    bad = be.RlcOpts((C.c_uint8 * 32)(), 16)
    assert L.h2v_aggregate_batch(dp.handle, C.byref(one), pair, inc, None, None, C.byref(bad), None) == -1   # an unknown flag
    assert L.h2v_aggregate_batch_device(dp.handle, C.byref(one), C.addressof(pair), C.addressof(inc), None, None, None, None, None) == -1   # ws == NULL
    # n = 0: H2V_OK and (inf, inf), both forms
    zero = be.Batch(0, None, None, None, None)
    assert L.h2v_aggregate_batch(dp.handle, C.byref(zero), pair, None, None, None, None, None) == 0 and pair.raw == INF_PAIR
    empty = synth.Batch(n=0, proofs=b"", proof_off=[0], instances=b"", committed=None, expected=[])
    ws = be.Workspace(dp, 8)
    assert _device(dp, empty, ws)[:3] == (INF_PAIR, [], [])
    ws.close()
