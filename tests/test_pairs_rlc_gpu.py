"""GPU tests of the batch-accept pair check (h2v_check_pairs_rlc: h2v_check_pairs's outputs from ONE pairing per batch, the
per-pair kernels only behind a failed check) and of H2V_RLC_FOLD_PAIRS (the batch form of recursive plans, which starts after
the fold).  Every expectation comes from the CPU oracle, from h2v_check_pairs or from the per-proof verify call; verdicts and
status words are compared for equality."""
import ctypes as C
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.test_gpu_parity import be, circuits, _permute  # noqa: F401  (module fixtures)
from tests.test_wide_keys_gpu import wide  # noqa: F401
from tests.test_prepare_pairs_gpu import _dev, _edge_pairs, PRE_PAIRING, PAIRING_ONLY, ACC

pytestmark = pytest.mark.gpu
R = bls.R
SEED = bytes(range(32))
MAX_N = 320


@pytest.fixture(scope="module")
def pool(circuits, orc):
    """MAX_N valid pairs (A_i, s A_i) of the simple_mul SRS - running additions, so one scalar multiplication in all - plus the
    points some tests perturb them with; the oracle confirms a sample of them (computed once, never changed)"""
    vk, td = circuits["simple_mul"][:2]
    rng = random.Random(81)
    s = td.s
    a, d = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R)), bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
    sa, sd = bls.g1_mul(a, s), bls.g1_mul(d, s)
    pts = []
    for _ in range(MAX_N):
        pts.append((a, sa))
        a, sa = bls.g1_add(a, d), bls.g1_add(sa, sd)
    sg2, g2 = bytes.fromhex(vk.s_g2), orc.g2_generator_compressed()
    for k in (0, 1, MAX_N - 1):
        assert orc.pairing_check(pts[k][0], sg2, pts[k][1], g2) == 1
    return {"pts": pts, "pairs": [bls.g1_compress(l) + bls.g1_compress(r) for l, r in pts], "d": d, "sg2": sg2, "g2": g2}


def _rlc_device(dp, raw, ws, seed=SEED, stream=None):
    """(accept, status) of the device form; the workspace is joined and the stream synchronised"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(raw) // 96
    s = stream or torch.cuda.Stream(device=dev)
    pairs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dp.check_pairs_rlc_device(n, pairs.data_ptr(), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream, seed=seed)
    ws.join(s.cuda_stream)
    s.synchronize()
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_all_valid_pairs(be, circuits, pool, n):
    """the edges of the 64-lane coefficient kernel, of the 64-pair groups and of GRP_MIN_N = 256; a given seed and the OS's"""
    dp = circuits["simple_mul"][3]
    raw = b"".join(pool["pairs"][:n])
    for seed in (SEED, None):
        ws = be.Workspace(dp, n)
        acc, st, fell_back = dp.check_pairs_rlc(raw, ws=ws, seed=seed)
        assert list(acc) == [1] * n and st == [0] * n and not fell_back, (n, seed)
        ok, tm = ws.rlc_result()
        assert ok and tm.msm_terms == n
        assert tm.transcript_combiner_ms == 0
        ws.close()


def test_copies_of_one_pair_meet_in_the_buckets(be, circuits, pool):
    dp = circuits["simple_mul"][3]
    acc, st, fell_back = dp.check_pairs_rlc(pool["pairs"][5] * 64, seed=SEED)
    assert list(acc) == [1] * 64 and st == [0] * 64 and not fell_back


@pytest.mark.parametrize("n", [1, 65, 300])
def test_decoding_edges_without_a_failing_equation(be, orc, circuits, n):
    vk, td, pl, dp, ov = circuits["simple_mul"]
    edges = _edge_pairs(vk, td, orc)
    inf = bls.g1_compress(None)
    keep = [e for e in edges if e[1] == 1 or e[2] == be.ST_BAD_POINT]          # good pairs, (inf, inf), every undecodable kind
    good = [e for e in keep if e[1] == 1 and e[0] != inf + inf]
    infs = [e for e in keep if e[0] == inf + inf]
    bad = [e for e in keep if e[2] == be.ST_BAD_POINT]
    assert len(good) == 2 and len(infs) == 1 and len(bad) == 10 and len(keep) == 13
    rng = random.Random(82 + n)
    mix = [rng.choice(keep) for _ in range(n)]
    if n >= 65:
        assert all(any(e in cls for e in mix) for cls in (good, infs, bad))
    raw = b"".join(e[0] for e in mix)
    ws = be.Workspace(dp, n)
    acc, st, fell_back = dp.check_pairs_rlc(raw, ws=ws, seed=SEED)
    pacc, pst = dp.check_pairs(raw)
    assert list(acc) == list(pacc) == [e[1] for e in mix]
    assert st == pst == [e[2] for e in mix]
    assert not fell_back and ws.rlc_result()[0]
    if n == 300:
        # only undecodable and (inf, inf) pairs: both sums are infinity and the check passes
        mix = [rng.choice(infs + bad) for _ in range(n)]
        assert any(e in infs for e in mix) and any(e in bad for e in mix)
        acc, st, fell_back = dp.check_pairs_rlc(b"".join(e[0] for e in mix), ws=ws, seed=SEED)
        assert list(acc) == [e[1] for e in mix] and st == [e[2] for e in mix] and not fell_back
        assert ws.rlc_result()[0]
    ws.close()


def test_coefficients_really_differ(be, orc, circuits, pool):
    """(A, sA + D), (B, sB - D): the errors cancel under equal coefficients - each pair fails alone, their plain sum passes"""
    dp = circuits["simple_mul"][3]
    (a, sa), (b, sb) = pool["pts"][0], pool["pts"][1]
    d, sg2, g2 = pool["d"], pool["sg2"], pool["g2"]
    r0, r1 = bls.g1_add(sa, d), bls.g1_add(sb, bls.g1_neg(d))
    assert orc.pairing_check(a, sg2, r0, g2) == 0 and orc.pairing_check(b, sg2, r1, g2) == 0
    assert orc.pairing_check(bls.g1_add(a, b), sg2, bls.g1_add(r0, r1), g2) == 1
    two = [bls.g1_compress(a) + bls.g1_compress(r0), bls.g1_compress(b) + bls.g1_compress(r1)]
    for pad in (0, 62):
        raw = b"".join(two + pool["pairs"][2:2 + pad])
        for seed in (SEED, None):
            acc, st, fell_back = dp.check_pairs_rlc(raw, seed=seed)
            assert list(acc) == [0, 0] + [1] * pad and st == [be.ST_PAIRING] * 2 + [0] * pad and fell_back, (pad, seed)


def _localise_batch(pool, n):
    """valid pairs with one failing equation in group 3, one at the last index, one (inf, P) and one (P, inf)"""
    inf = bls.g1_compress(None)
    pairs = list(pool["pairs"][:n])
    for k in (3 * 64 + 5, n - 1):
        l, r = pool["pts"][k]
        pairs[k] = bls.g1_compress(l) + bls.g1_compress(bls.g1_add(r, pool["d"]))
    pairs[10] = inf + pairs[10][48:]
    pairs[70] = pairs[70][:48] + inf
    return b"".join(pairs), [3 * 64 + 5, n - 1, 10, 70]


@pytest.fixture(scope="module")
def localise(be, circuits, pool):
    """n -> (pairs, h2v_check_pairs's accept, status): the reference every form below is compared with"""
    dp = circuits["simple_mul"][3]
    out = {}
    for n in (200, 300, 320):
        raw, bad = _localise_batch(pool, n)
        acc, st = dp.check_pairs(raw)
        assert list(acc) == [0 if k in bad else 1 for k in range(n)]
        assert st == [be.ST_PAIRING if k in bad else 0 for k in range(n)]
        out[n] = (raw, list(acc), st)
    return out


def test_the_fall_back_localises(be, circuits, localise):
    """n = 320: five groups, the group stage on - and the same outputs with the stage switched off, and below GRP_MIN_N"""
    dp = circuits["simple_mul"][3]
    for n, group_stage in ((320, 0), (320, -1), (200, 0)):
        raw, want_acc, want_st = localise[n]
        ws = be.Workspace(dp, n)
        if group_stage:
            ws.set_option(be.OPT_RLC_GROUP_STAGE, group_stage)
        acc, st, fell_back = dp.check_pairs_rlc(raw, ws=ws, seed=SEED)
        assert list(acc) == want_acc and st == want_st and fell_back, (n, group_stage)
        ok, tm = ws.rlc_result()
        assert not ok and tm.msm_terms == n
        ws.close()


def test_calling_forms(be, circuits, localise):
    import torch
    vk, td, pl, dp, ov = circuits["simple_mul"]
    dp2 = circuits["sha256"][3]
    n = 300
    raw, want_acc, want_st = localise[n]
    forms = {
        "ordinary": be.Workspace(dp, n),
        "laned": be.Workspace(dp, n, lanes=3, chunk=128),       # a chunk that does not divide n
        "multi": be.Workspace.multi([dp, dp2], 512, lanes=2, chunk=200),
    }
    for form, ws in forms.items():
        acc, st, fell_back = dp.check_pairs_rlc(raw, ws=ws, seed=SEED)
        assert list(acc) == want_acc and st == want_st and fell_back, form
        assert _rlc_device(dp, raw, ws) == (want_acc, want_st), form
        with pytest.raises(be.H2VError):
            ws.timings()
        ok, tm = ws.rlc_result()
        assert not ok and tm.msm_terms > 0 and tm.pairing_ms > 0, form
        # a clean batch on the same workspace afterwards: the verdict is the call's own
        acc, st, fell_back = dp.check_pairs_rlc(raw[:96 * 10], ws=ws, seed=SEED)
        assert list(acc) == [1] * 10 and not fell_back and ws.rlc_result()[0], form
        ws.close()
    # deferred joins: small verify calls still gathered in an open group when the pair check arrives
    from plutus_halo2_verifier_gen_amd import synth
    batch = synth.forge_batch(vk, td, 150, seed=41, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.3, seed=42, kinds=PRE_PAIRING + PAIRING_ONLY)
    ws = be.Workspace(dp, 1024, lanes=0, chunk=512)
    ws.defer_joins(True)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    held = []
    for lo in (0, 50, 100):
        db = _dev(_permute(batch, list(range(lo, lo + 50)), vk.n_public_inputs))
        acc = torch.zeros(50, dtype=torch.uint8, device=dev)
        dp.verify_batch_device(50, db["proofs"].data_ptr(), db["off"].data_ptr(), db["inst"].data_ptr(), None, acc.data_ptr(),
                               None, ws=ws, stream=s.cuda_stream)
        held.append((lo, db, acc))
    assert _rlc_device(dp, raw, ws, stream=s) == (want_acc, want_st)
    for lo, _db, acc in held:
        assert acc.cpu().tolist() == batch.expected[lo:lo + 50]
    assert any(batch.expected[:150]) and not all(batch.expected[:150])
    ok, _tm = ws.rlc_result()
    assert not ok
    # the NULL stream is refused under deferred joins
    pairs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)
    with pytest.raises(be.H2VError):
        dp.check_pairs_rlc_device(n, pairs.data_ptr(), out.data_ptr(), None, ws=ws, stream=None)
    ws.close()


def _reject_batch(circuits, name, n=96):
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits[name]
    kinds = PRE_PAIRING + PAIRING_ONLY + (ACC if pl.is_recursive else [])
    batch = synth.forge_batch(vk, td, n, seed=31, plan=pl, workers=8, ci_identity=(name == "sha256"))
    return synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.4, seed=32, kinds=kinds)


@pytest.mark.parametrize("name", ["simple_mul", "sha256", "ivc"])
def test_prepare_then_check_pairs_rlc_is_verify(be, circuits, name):
    vk, td, pl, dp, ov = circuits[name]
    batch = _reject_batch(circuits, name)
    args = (batch.proofs, batch.proof_off, batch.instances, batch.committed)
    want = list(dp.verify_batch(*args))
    assert want == batch.expected
    raw, pst = dp.prepare_batch(*args)
    pre = [i for i in range(batch.n) if pst[i]]
    late = [i for i in range(batch.n) if not pst[i] and not want[i]]
    assert pre and late and any(want)                  # both classes of reject, and accepts
    acc, st, fell_back = dp.check_pairs_rlc(raw, seed=SEED)
    assert list(acc) == want and fell_back
    assert all(st[i] == be.ST_BAD_POINT for i in pre) and all(st[i] == be.ST_PAIRING for i in late)
    assert (list(acc), st) == tuple(map(list, dp.check_pairs(raw)))


def _verify_device(dp, batch, ws, rlc=False, fold_pairs=False):
    import torch
    d = _dev(batch)
    dev = d["dev"]
    s = torch.cuda.Stream(device=dev)
    acc = torch.full((batch.n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((batch.n,), -1, dtype=torch.int32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    args = (batch.n, ptr(d["proofs"]), ptr(d["off"]), ptr(d["inst"]), ptr(d["ci"]), acc.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    if rlc:
        dp.verify_batch_rlc_device(*args, ws=ws, stream=s.cuda_stream, seed=SEED, fold_pairs=fold_pairs)
    else:
        dp.verify_batch_device(*args, ws=ws, stream=s.cuda_stream)
    ws.join(s.cuda_stream)
    s.synchronize()
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()]


def test_fold_pairs_clean_batches(be, circuits, wide):
    from plutus_halo2_verifier_gen_amd import synth
    for (vk, td, pl, dp, ov), n in ((circuits["ivc"], 96), (wide["ivc_wide"], 32)):
        batch = synth.forge_batch(vk, td, n, seed=33, plan=pl, workers=8)
        ws = be.Workspace(dp, n)
        acc, fell_back = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws, seed=SEED,
                                             fold_pairs=True)
        assert list(acc) == [1] * n and not fell_back
        ok, tm = ws.rlc_result()
        assert ok and tm.msm_terms == n
        ws.close()


def test_fold_pairs_with_rejects_matches_the_per_proof_call(be, circuits):
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["ivc"]
    batch = _reject_batch(circuits, "ivc")
    n = batch.n
    args = (batch.proofs, batch.proof_off, batch.instances, batch.committed)
    ws = be.Workspace(dp, n)
    want = _verify_device(dp, batch, ws)
    assert want[0] == batch.expected
    assert any(s == be.ST_PAIRING for s in want[1]) and any(s and not s & be.ST_PAIRING for s in want[1]) and any(want[0])
    assert _verify_device(dp, batch, ws, rlc=True, fold_pairs=True) == want        # bit for bit
    ok, tm = ws.rlc_result()
    assert not ok and tm.msm_terms == n
    with pytest.raises(be.H2VError):
        ws.timings()
    acc, fell_back = dp.verify_batch_rlc(*args, ws=ws, seed=SEED, fold_pairs=True)
    assert list(acc) == want[0] and fell_back
    # without the flag: today's behaviour - per proof behind the RLC entry point
    acc, fell_back = dp.verify_batch_rlc(*args, ws=ws, seed=SEED)
    assert list(acc) == want[0] and not fell_back
    assert _verify_device(dp, batch, ws, rlc=True) == want
    ws.close()
    # laned, every chunk its own check (a chunk that does not divide n), device and host form, and submit / wait
    laned = be.Workspace(dp, n, lanes=2, chunk=40)
    assert _verify_device(dp, batch, laned, rlc=True, fold_pairs=True) == want
    assert not laned.rlc_result()[0]
    acc, fell_back = dp.verify_batch_rlc(*args, ws=laned, seed=SEED, fold_pairs=True)
    assert list(acc) == want[0] and fell_back
    hb, keep = dp.host_batch(*args)
    for ws in (laned, be.Workspace(dp, n)):
        dp.submit(hb, ws, rlc=True, seed=SEED, fold_pairs=True)
        acc, fell_back = ws.wait(n)
        assert list(acc) == want[0] and fell_back
        dp.submit(hb, ws, rlc=True, seed=SEED)
        acc, fell_back = ws.wait(n)
        assert list(acc) == want[0] and not fell_back
        ws.close()
    del keep
    # only pre-pairing and H2V_ST_RECURSION rejects: they take no part, the check passes
    clean = synth.forge_batch(vk, td, n, seed=35, plan=pl, workers=8)
    early = synth.with_rejects(pl, clean, vk.n_public_inputs, fraction=0.4, seed=36, kinds=PRE_PAIRING + ["acc_vk_hash"])
    ws = be.Workspace(dp, n)
    want = _verify_device(dp, early, ws)
    assert want[0] == early.expected and any(want[0]) and not all(want[0])
    assert not any(s & be.ST_PAIRING for s in want[1])
    assert any(s & be.ST_RECURSION for s in want[1]) and any(s and not s & be.ST_RECURSION for s in want[1])
    assert _verify_device(dp, early, ws, rlc=True, fold_pairs=True) == want
    assert ws.rlc_result()[0]
    ws.close()


def test_fold_pairs_is_ignored_by_a_plan_that_is_not_recursive(be, circuits):
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    batch = synth.forge_batch(vk, td, 96, seed=37, plan=pl, workers=8)
    args = (batch.proofs, batch.proof_off, batch.instances, batch.committed)
    terms = []
    for flag in (False, True):
        ws = be.Workspace(dp, 96)
        acc, fell_back = dp.verify_batch_rlc(*args, ws=ws, seed=SEED, fold_pairs=flag)
        assert list(acc) == [1] * 96 and not fell_back
        ok, tm = ws.rlc_result()
        assert ok
        terms.append(tm.msm_terms)
        ws.close()
    assert terms[0] == terms[1] > 96           # the verify form's right-hand sum: every per-proof term and the VK bases


def test_misuse(be, circuits, pool):
    dp = circuits["simple_mul"][3]
    L = be.lib()
    raw = b"".join(pool["pairs"][:4])
    acc = (C.c_uint8 * 4)(9, 9, 9, 9)
    E_ARG = -1
    assert L.h2v_check_pairs_rlc(dp.handle, 4, None, acc, None, None, None, None) == E_ARG
    assert L.h2v_check_pairs_rlc(dp.handle, 4, raw, None, None, None, None, None) == E_ARG
    assert L.h2v_check_pairs_rlc_device(dp.handle, 4, None, C.addressof(acc), None, None, None, None) == E_ARG
    assert L.h2v_check_pairs_rlc_device(dp.handle, 4, C.addressof(acc), C.addressof(acc), None, None, None, None) == E_ARG   # no workspace
    ws = be.Workspace(dp, 2)
    assert L.h2v_check_pairs_rlc(dp.handle, 4, raw, acc, None, ws.handle, None, None) == E_ARG       # n > max_batch
    assert L.h2v_check_pairs_rlc(dp.handle, 0, raw, acc, None, ws.handle, None, None) == 0
    assert list(acc) == [9, 9, 9, 9]                                                                   # nothing written
    assert L.h2v_check_pairs_rlc(dp.handle, (1 << 22) + 1, raw, acc, None, ws.handle, None, None) == -4   # H2V_E_LIMIT
    ws.close()


def test_after_shutdown_the_call_is_refused(be):
    import os
    import subprocess
    import sys
    script = (
        "import sys; sys.path.insert(0, %r)\n"
        "import ctypes as C\n"
        "from plutus_halo2_verifier_gen_amd import backend, plan as PL, vk as V\n"
        "vk, td = V.simple_mul_vk()\n"
        "dp = backend.DevicePlan(PL.compile_plan(vk).to_bytes(), 0)\n"
        "ws = backend.Workspace(dp, 8)\n"
        "acc, st, fb = dp.check_pairs_rlc((b'\\xc0' + bytes(47)) * 2, ws=ws)\n"
        "assert list(acc) == [1] and st == [0] and not fb\n"
        "backend.shutdown(0)\n"
        "L = backend.lib()\n"
        "out = (C.c_uint8 * 1)()\n"
        "assert L.h2v_check_pairs_rlc(dp.handle, 1, bytes(96), out, None, ws.handle, None, None) == -3\n"
        "assert L.h2v_check_pairs_rlc(dp.handle, 1, bytes(96), out, None, None, None, None) == -3\n"
        "assert L.h2v_check_pairs_rlc_device(dp.handle, 1, C.addressof(out), C.addressof(out), None, ws.handle, None, None) == -3\n"
        "backend.shutdown(-1)\n"
        "ws.close(); dp.close()\n"
        "print('shutdown ok')\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shutdown ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_python_api(be, circuits):
    """the three-proof case of test_python_api_dual_msm: an accept, a pairing-only reject, a pre-pairing reject"""
    from plutus_halo2_verifier_gen_amd import api, synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    batch = synth.forge_batch(vk, td, 3, seed=61, plan=pl, workers=1)
    proofs = [batch.proof(i) for i in range(3)]
    pubs = [batch.instance_ints(i, vk.n_public_inputs) for i in range(3)]
    rng = random.Random(62)
    proofs[1] = synth.corrupt(pl, proofs[1], b"", "wrong_pi", rng)[0]
    proofs[2] = synth.corrupt(pl, proofs[2], b"", "bad_point_flag", rng)[0]
    v = api.verifier_for(vk)
    pairs, _st = v.prepare_batch(proofs, pubs)
    want = v.check_pairs(pairs)
    assert want == ([True, False, False], [0, be.ST_PAIRING, be.ST_BAD_POINT])
    assert v.check_pairs(pairs, mode="rlc") == want
    assert v.check_pairs(pairs, mode="rlc", seed=SEED) == want
    assert v.check_pairs(pairs[:1], mode="rlc") == ([True], [0])
    assert v.check_pairs([], mode="rlc") == ([], [])
    with pytest.raises(ValueError):
        v.check_pairs(pairs, mode="batch")
