"""GPU tests of prepare (the verify pipeline up to the pairing, returning each proof's pair compress(L) || compress(R)) and
the pair check (the pairing alone on pairs from anywhere), include/h2v.h.  Every key against the CPU oracle's el / er, the
calling forms (host / device, laned, multi-plan, deferred joins with open coalesced groups), the pair check's decoding
edges and sizes, the Python API and points at infinity.  /root/reference is NOT needed."""
import json
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.degenerate_keys import oracle_pairs
from tests.test_gpu_parity import be, circuits, _permute  # noqa: F401  (module fixtures)
from tests.test_wide_keys_gpu import wide  # noqa: F401

pytestmark = pytest.mark.gpu
P, R = bls.P, bls.R
PRE_PAIRING = ["bad_point_flag", "point_not_in_subgroup", "noncanonical_scalar", "truncated"]
PAIRING_ONLY = ["wrong_pi", "wrong_public_input"]
ACC = ["acc_limb", "acc_scalar", "acc_fixed_scalar", "acc_sign", "acc_vk_hash"]


_oracle = oracle_pairs   # (shared with the tests of degenerate keys: tests/degenerate_keys.py)


def _dev(batch):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    return {"proofs": t(batch.proofs), "off": torch.tensor(batch.proof_off, dtype=torch.int64, device=dev),
            "inst": t(batch.instances), "ci": t(batch.committed), "dev": dev}


def _device_run(dp, batch, ws=None, stream=None):
    """(verify accept, verify status, prepare pairs, prepare status, check accept, check status), all device forms"""
    import torch
    d = _dev(batch)
    n, dev = batch.n, d["dev"]
    s = stream or torch.cuda.Stream(device=dev)
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    vst = torch.zeros(n, dtype=torch.int32, device=dev)
    pairs = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    pst = torch.zeros(n, dtype=torch.int32, device=dev)
    cacc = torch.zeros(n, dtype=torch.uint8, device=dev)
    cst = torch.zeros(n, dtype=torch.int32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    args = (n, ptr(d["proofs"]), ptr(d["off"]), ptr(d["inst"]), ptr(d["ci"]))
    torch.cuda.synchronize()
    dp.verify_batch_device(*args, acc.data_ptr(), vst.data_ptr(), ws=ws, stream=s.cuda_stream)
    dp.prepare_batch_device(*args, pairs.data_ptr(), pst.data_ptr(), ws=ws, stream=s.cuda_stream)
    if ws is not None:
        ws.join(s.cuda_stream)
    dp.check_pairs_device(n, pairs.data_ptr(), cacc.data_ptr(), cst.data_ptr(), ws=ws, stream=s.cuda_stream)
    if ws is not None:
        ws.join(s.cuda_stream)
    s.synchronize()
    raw = bytes(pairs.cpu().numpy().tobytes())
    return (list(acc.cpu().tolist()), [v & 0xffffffff for v in vst.cpu().tolist()], raw,
            [v & 0xffffffff for v in pst.cpu().tolist()], list(cacc.cpu().tolist()), [v & 0xffffffff for v in cst.cpu().tolist()])


def _all_keys(circuits, wide):
    from plutus_halo2_verifier_gen_amd import vk as V
    keys = [(name, circuits[name]) for name in V.BUILDERS] + [(name, wide[name]) for name in V.WIDE_BUILDERS]
    return keys


def test_every_key_against_the_oracle(be, orc, circuits, wide):
    """pairs == the oracle's compress(el) || compress(er) where it reaches the pairing, 96 zero bytes elsewhere; prepare's status
    == verify's without ST_PAIRING; check_pairs(pairs) == verify == the oracle - host and device forms"""
    from plutus_halo2_verifier_gen_amd import synth
    for name, (vk, td, pl, dp, ov) in _all_keys(circuits, wide):
        n = 200
        kinds = PRE_PAIRING + PAIRING_ONLY + (ACC if pl.is_recursive else [])
        batch = synth.forge_batch(vk, td, n, seed=31, plan=pl, workers=8, ci_identity=(name == "sha256"))
        batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.4, seed=32, kinds=kinds)
        want = _oracle(ov, orc, batch, vk.n_public_inputs)
        assert [a for a, _ in want] == batch.expected, name
        acc, vst, raw, pst, cacc, cst = _device_run(dp, batch)
        assert acc == batch.expected, name
        for i in range(n):
            assert raw[96 * i:96 * i + 96] == want[i][1], (name, i)
        assert pst == [v & ~be.ST_PAIRING for v in vst], name
        assert cacc == acc, name
        hraw, hst = dp.prepare_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)
        assert hraw == raw and hst == pst, name
        hacc, hcst = dp.check_pairs(hraw)
        assert list(hacc) == acc and hcst == cst, name
        # pre-pairing rejects: zero pair, checked as a bad point; pairing-only rejects: a valid pair the pairing refuses
        for i in range(n):
            if pst[i]:
                assert cst[i] == be.ST_BAD_POINT
            elif not acc[i]:
                assert cst[i] == be.ST_PAIRING and vst[i] == be.ST_PAIRING
        assert any(pst) and any(not a and not s for a, s in zip(acc, pst)) and any(acc), name


def test_calling_forms_and_chunking(be, orc, circuits):
    """laned workspace (a chunk that does not divide n), multi-plan workspace, deferred joins with small verify calls still
    gathered when a prepare call arrives: every form gives the same pairs, status and verdicts"""
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n = 300
    batch = synth.forge_batch(vk, td, n, seed=41, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.3, seed=42, kinds=PRE_PAIRING + PAIRING_ONLY)
    ref = _device_run(dp, batch)
    assert ref[0] == batch.expected and ref[4] == ref[0]
    dp2 = circuits["sha256"][3]
    forms = {
        "ordinary": be.Workspace(dp, n),
        "laned": be.Workspace(dp, n, lanes=3, chunk=128),
        "multi": be.Workspace.multi([dp, dp2], 512, lanes=2, chunk=200),
    }
    for form, ws in forms.items():
        got = _device_run(dp, batch, ws=ws)
        assert got == ref, form
        hraw, hst = dp.prepare_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
        assert hraw == ref[2] and hst == ref[3], form
        hacc, hcst = dp.check_pairs(hraw, ws=ws)
        assert list(hacc) == ref[4] and hcst == ref[5], form
        tm = ws.timings()
        assert tm.pairing_ms > 0                   # (the check call ran the pairing)
    # deferred joins: small verify calls gathered into an open group when a prepare call arrives
    ws = be.Workspace(dp, 1024, lanes=0, chunk=512)
    ws.defer_joins(True)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    d = _dev(batch)
    held = []
    for lo in (0, 50, 100):
        b = _permute(batch, list(range(lo, lo + 50)), vk.n_public_inputs)
        db = _dev(b)
        acc = torch.zeros(50, dtype=torch.uint8, device=dev)
        st = torch.zeros(50, dtype=torch.int32, device=dev)
        dp.verify_batch_device(50, db["proofs"].data_ptr(), db["off"].data_ptr(), db["inst"].data_ptr(), None, acc.data_ptr(),
                               st.data_ptr(), ws=ws, stream=s.cuda_stream)
        held.append((lo, db, acc, st))
    pairs = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    pst = torch.zeros(n, dtype=torch.int32, device=dev)
    dp.prepare_batch_device(n, d["proofs"].data_ptr(), d["off"].data_ptr(), d["inst"].data_ptr(), None, pairs.data_ptr(),
                            pst.data_ptr(), ws=ws, stream=s.cuda_stream)
    ws.join(s.cuda_stream)
    s.synchronize()
    tm = ws.timings()
    assert tm.pairing_ms == 0                      # a prepare call runs no pairing
    assert bytes(pairs.cpu().numpy().tobytes()) == ref[2]
    assert [v & 0xffffffff for v in pst.cpu().tolist()] == ref[3]
    for lo, _db, acc, st in held:
        assert acc.cpu().tolist() == ref[0][lo:lo + 50]
        assert [v & 0xffffffff for v in st.cpu().tolist()] == ref[1][lo:lo + 50]
    ws.close()
    # the NULL-stream rule of deferred joins holds for the new device forms too
    ws = be.Workspace(dp, 1024, lanes=2, chunk=256)
    ws.defer_joins(True)
    with pytest.raises(be.H2VError):
        dp.prepare_batch_device(n, d["proofs"].data_ptr(), d["off"].data_ptr(), d["inst"].data_ptr(), None, pairs.data_ptr(),
                                None, ws=ws, stream=None)
    with pytest.raises(be.H2VError):
        dp.check_pairs_device(n, pairs.data_ptr(), pairs.data_ptr(), None, ws=ws, stream=None)
    ws.close()


def _edge_pairs(vk, td, orc):
    """(pair bytes, expected accept, expected status) - the oracle decides every expectation"""
    rng = random.Random(51)
    s = td.s
    sg2, g2 = bytes.fromhex(vk.s_g2), orc.g2_generator_compressed()
    A = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
    B = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
    good = [(bls.g1_compress(A), bls.g1_compress(bls.g1_mul(A, s))), (bls.g1_compress(B), bls.g1_compress(bls.g1_mul(B, s)))]
    bad_eq = (bls.g1_compress(A), bls.g1_compress(bls.g1_mul(A, s + 1)))
    inf = bls.g1_compress(None)
    flag = bytearray(bls.g1_compress(A)); flag[0] &= 0x7F
    big = bytearray((P + 1).to_bytes(48, "big")); big[0] |= 0x80
    while True:
        x = rng.randrange(P)
        if bls.fp_sqrt(x * x * x + 4) is None:
            break
    off = bytearray(x.to_bytes(48, "big")); off[0] |= 0x80
    while True:
        x = rng.randrange(P)
        yy = bls.fp_sqrt(x * x * x + 4)
        if yy is not None and not bls.g1_in_subgroup((x, yy)):
            break
    nosub = bls.g1_compress((x, yy))
    cases = good + [bad_eq, (inf, inf), (inf, bls.g1_compress(A)), (bls.g1_compress(A), inf)]
    for badp in (bytes(flag), bytes(big), bytes(off), nosub, bytes(48)):
        cases += [(badp, good[0][1]), (good[0][0], badp)]
    out = []
    for l, r in cases:
        okl, pl_ = orc.g1_decompress(l)
        okr, pr_ = orc.g1_decompress(r)
        okl = okl and (pl_ is None or orc.g1_in_subgroup(pl_) == 1)
        okr = okr and (pr_ is None or orc.g1_in_subgroup(pr_) == 1)
        if not (okl and okr):
            out.append((l + r, 0, 8))
        else:
            e = orc.pairing_check(pl_, sg2, pr_, g2)
            assert e in (0, 1)
            out.append((l + r, e, 0 if e else 16))
    return out


def test_pair_check_edges_and_sizes(be, orc, circuits):
    vk, td, pl, dp, ov = circuits["simple_mul"]
    edges = _edge_pairs(vk, td, orc)
    want_acc = [a for _, a, _ in edges]
    assert want_acc[:6] == [1, 1, 0, 1, 0, 0]           # (P, sP) x2, (P, (s+1)P), (inf, inf), (inf, P), (P, inf)
    assert all(st == be.ST_BAD_POINT for _, _, st in edges[6:])
    acc, st = dp.check_pairs(b"".join(p for p, _, _ in edges))
    assert list(acc) == want_acc and st == [s for _, _, s in edges]
    rng = random.Random(52)
    laned = be.Workspace(dp, 8192, lanes=3, chunk=1500)
    for n, ws in ((1, None), (63, None), (64, None), (65, None), (4096, None), (4097, laned)):
        idx = [rng.randrange(len(edges)) for _ in range(n)]
        acc, st = dp.check_pairs(b"".join(edges[k][0] for k in idx), ws=ws)
        assert list(acc) == [edges[k][1] for k in idx], n
        assert st == [edges[k][2] for k in idx], n


def test_python_api_dual_msm(be, circuits):
    from plutus_halo2_verifier_gen_amd import api, synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    batch = synth.forge_batch(vk, td, 3, seed=61, plan=pl, workers=1)
    proofs = [batch.proof(i) for i in range(3)]
    pubs = [batch.instance_ints(i, vk.n_public_inputs) for i in range(3)]
    rng = random.Random(62)
    proofs[1] = synth.corrupt(pl, proofs[1], b"", "wrong_pi", rng)[0]                  # rejected by the pairing only
    proofs[2] = synth.corrupt(pl, proofs[2], b"", "bad_point_flag", rng)[0]            # rejected before the pairing
    v = api.verifier_for(vk)
    pairs, st = v.prepare_batch(proofs, pubs)
    assert st[0] == 0 and st[1] == 0 and st[2] == be.ST_BAD_POINT and pairs[2] == bytes(96)
    acc, cst = v.check_pairs(pairs)
    assert acc == [True, False, False] == v.verify_batch(proofs, pubs)

    def guard(i):
        return api.prepare(vk, [[]], [[pubs[i]]], api.CircuitTranscript.init_from_bytes(proofs[i]))

    for i in (0, 1):
        m = guard(i).dual_msm()
        assert m.left + m.right == pairs[i]
        assert m.check() == guard(i).check() == (i == 0)
    with pytest.raises(api.VerifyError):
        guard(2).dual_msm()


def test_infinity_in_the_export(be, orc, circuits):
    """L at infinity: a proof whose pi is the infinity encoding (pi is never hashed, so the transcript is unchanged and the
    proof reaches the pairing) exports 0xc0 || 0..., as the oracle's el.  (R at infinity would need an MSM that sums to
    infinity; the forger cannot make one.)"""
    from plutus_halo2_verifier_gen_amd import synth
    for name in ("simple_mul", "sha256"):
        vk, td, pl, dp, ov = circuits[name]
        batch = synth.forge_batch(vk, td, 2, seed=71, plan=pl, workers=1, ci_identity=(name == "sha256"))
        proofs = [bytearray(batch.proof(i)) for i in range(2)]
        o = pl.points[pl.pi_point]
        proofs[1][o:o + 48] = bls.g1_compress(None)
        b2 = synth.Batch(n=2, proofs=b"".join(bytes(p) for p in proofs), proof_off=[0, len(proofs[0]), len(proofs[0]) + len(proofs[1])],
                         instances=batch.instances, committed=batch.committed, expected=[1, 0])
        raw, st = dp.prepare_batch(b2.proofs, b2.proof_off, b2.instances, b2.committed)
        want = _oracle(ov, orc, b2, vk.n_public_inputs)
        assert st == [0, 0], name
        assert raw[96:144] == b"\xc0" + bytes(47), name
        assert raw == want[0][1] + want[1][1], name
        acc, cst = dp.check_pairs(raw)
        assert list(acc) == [w for w, _ in want] == list(dp.verify_batch(b2.proofs, b2.proof_off, b2.instances, b2.committed))
