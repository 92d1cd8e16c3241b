"""GPU tests of keys whose final MSM has more than 64 terms in one sum (vk.WIDE_BUILDERS): segmented sums (k_g1_msm_seg and
its kin, folded by k_g1_sum_segments) against the CPU oracle - the probe MSM up to H2V_MAX_MSM_TERMS terms under every
forced shape, every wide key in every calling form and forced shape, the wide recursion key, and bls12381 at 1024 proofs.
/root/reference is NOT needed."""
import json
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.test_gpu_parity import TRACE_NAMES, _permute, be  # noqa: F401  (be: the module's backend fixture)

pytestmark = pytest.mark.gpu
R = bls.R
WIDE_T = (65, 69, 128, 257, 513, 1000, 4096)


@pytest.fixture(scope="module")
def wide():
    """name -> (vk, trapdoor, plan, device plan, oracle vk)"""
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, vk as V
    from oracle import binding as orc
    out = {}
    for name, build in V.WIDE_BUILDERS.items():
        vk, td = build()
        pl = PL.compile_plan(vk)
        dp = backend.DevicePlan(pl.to_bytes(), 0)
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        out[name] = (vk, td, pl, dp, ov)
    return out


def _msm_groups(T, chain, rng):
    """test_g1_msm's five groups at width T - random scalars; zero and R - 1 scalars; equal bases; opposite bases; an
    infinity base with GLV / window-border scalars - and two whose SEGMENT sums meet the exceptional cases of the fold
    (k_g1_sum_segments): every term the same base and scalar, so that segments of equal width have equal sums under any
    segmentation and the fold must double; and every scalar but the last zero, so that every segment but the last sums to
    the point at infinity"""
    lam = bls.GLV_LAMBDA
    edge = [1, 2, 7, 8, 9, 15, 16, 17, lam - 1, lam, lam + 1, 2 * lam, R - lam, (1 << 128) - 1, 1 << 128,
            (1 << 255) % R, 0x8888888888888888888888888888888888888888888888888888888888888888 % R]
    groups = []
    for g in range(7):
        ps = chain[g:g + T]
        ss = [rng.randrange(R) for _ in range(T)]
        if g == 1:
            ss[0], ss[-1] = 0, R - 1
        if g == 2:
            ps[1], ss[1] = ps[0], ss[0]           # equal terms: the reduction inside a block must double
            ps[T // 2], ss[T // 2] = ps[0], ss[0]
        if g == 3:
            ps[1] = bls.g1_neg(ps[0])             # opposite bases with equal scalars: lane sums cancel inside a block
            ss[1] = ss[0]
            ps[T - 1], ss[T - 1] = bls.g1_neg(ps[0]), ss[0]
        if g == 4:
            ps[0] = None
            for t in range(1, T):
                ss[t] = edge[(t - 1) % len(edge)]
        if g == 5:
            ps = [chain[0]] * T                   # equal segment sums: the fold doubles
            ss = [ss[0]] * T
        if g == 6:
            ss = [0] * (T - 1) + [ss[-1]]          # infinite segment sums: the fold starts from and adds infinity
        groups.append((ss, ps))
    return groups


@pytest.fixture(scope="module")
def msm_cases(orc):
    """per T the seven groups and the oracle's sums (computed once: orc_g1_msm takes seconds at 4096 terms)"""
    rng = random.Random(44)
    n = max(WIDE_T) + 7
    q, d = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R)), bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
    chain = [q]
    for _ in range(n - 1):                        # running additions: thousands of bases without a scalar multiplication each
        chain.append(bls.g1_add(chain[-1], d))
    comp = {}
    out = {}
    for T in WIDE_T:
        groups = _msm_groups(T, list(chain), rng)
        for _, ps in groups:
            for p in ps:
                if p not in comp:
                    comp[p] = bls.g1_compress(p)
        out[T] = ([ss for ss, _ in groups], [[comp[p] for p in ps] for _, ps in groups], [orc.g1_msm(ss, ps) for ss, ps in groups])
    return out


_SHAPES = [None, ("lpt", 1), ("lpt", 2), ("lpt", 8), ("tpl", 2), ("tpl", 3), ("tpl", 4)] + [("bs", b) for b in range(64, 513, 64)]


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "auto" if s is None else "%s%d" % s)
def test_wide_probe_msm_matches_oracle(be, msm_cases, shape):  # noqa: F811
    opt = None
    if shape is not None:
        opt = {"lpt": be.OPT_MSM_LANES_PER_TERM, "tpl": be.OPT_MSM_TERMS_PER_LANE, "bs": be.OPT_MSM_BLOCK_SIZE}[shape[0]]
        be.probe_set_option(opt, shape[1])
    try:
        for T in WIDE_T:
            ss, bs, want = msm_cases[T]
            assert be.probe_g1_msm(ss, bs) == want, (shape, T)
    finally:
        if opt is not None:
            be.probe_set_option(opt, 0)


def test_probe_msm_above_the_cap_is_refused(be):  # noqa: F811
    g = bls.g1_compress(bls.G1_GEN)
    with pytest.raises(be.H2VError, match="H2V_MAX_MSM_TERMS"):
        be.probe_g1_msm([[1] * 4097], [[g] * 4097])


def _mixed(vk, td, pl, n, seed, fraction=0.4):
    from plutus_halo2_verifier_gen_amd import synth
    b = synth.forge_batch(vk, td, n, seed=seed, plan=pl, workers=16)
    return b, synth.with_rejects(pl, b, vk.n_public_inputs, fraction=fraction, seed=seed + 1, kinds=list(synth.CORRUPTIONS))


def _device_call(dp, b, ws, stream, rlc=False):
    import torch
    dev = torch.device("cuda", 0)
    dpr = torch.frombuffer(bytearray(b.proofs), dtype=torch.uint8).to(dev)
    dof = torch.tensor(b.proof_off, dtype=torch.int64).to(dev)
    din = torch.frombuffer(bytearray(b.instances), dtype=torch.uint8).to(dev) if b.instances else None
    dci = torch.frombuffer(bytearray(b.committed), dtype=torch.uint8).to(dev) if b.committed else None
    acc = torch.full((b.n,), 7, dtype=torch.uint8, device=dev)
    args = (b.n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr() if din is not None else None,
            dci.data_ptr() if dci is not None else None, acc.data_ptr(), None)
    if rlc:
        dp.verify_batch_rlc_device(*args, ws=ws, stream=stream, seed=bytes(range(32)))
    else:
        dp.verify_batch_device(*args, ws=ws, stream=stream)
    return acc, (dpr, dof, din, dci)


@pytest.mark.parametrize("name", ["bls12381", "composite", "wide335", "wide677", "ivc_wide"])
def test_wide_key_every_form_matches_oracle(be, wide, name):  # noqa: F811
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = wide[name]
    n, n_pi = 48, vk.n_public_inputs
    clean, batch = _mixed(vk, td, pl, n, seed=21)
    want = list(ov.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, threads=16))
    assert want == batch.expected and 0 < sum(want) < n
    # a plain workspace
    ws = be.Workspace(dp, n)
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == want
    # trace slots and el / er of one accepting and one rejecting proof
    for i in (want.index(1), want.index(0)):
        ok, otr = ov.verify(batch.proof(i), batch.instance_ints(i, n_pi), batch.ci(i), trace=True)
        tr = dp.trace(batch.proof(i), batch.instances[32 * n_pi * i:32 * n_pi * (i + 1)], batch.ci(i))
        assert tr["accept"] == int(ok)
        if otr.status in (0, 1):
            for slot, val in tr["scalars"].items():
                assert val == (otr.scalar(TRACE_NAMES[slot]) if slot < 32 else otr.expression(slot - 32)), slot
            assert tr["el"] == otr.point("el") and tr["er"] == otr.point("er")
    # forced shapes: fixed-base split, lanes per term, terms per lane
    W = be.Workspace
    for opt, vals in ((be.OPT_MSM_FIXED_SPLIT, (-1, 1, 4)), (be.OPT_MSM_LANES_PER_TERM, (1, 2, 8)), (be.OPT_MSM_TERMS_PER_LANE, (2, 3, 4))):
        for v in vals:
            ws.set_option(opt, v)
            assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == want, (opt, v)
        ws.set_option(opt, 0)
    ws.close()
    # host-buffer submit / wait
    hws = be.Workspace(dp, n)
    hb, _keep = dp.host_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)
    dp.submit(hb, hws)
    acc, _ = hws.wait(n)
    assert list(acc) == want
    hws.close()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    # the device form
    dws = be.Workspace(dp, n)
    acc, _keep = _device_call(dp, batch, dws, s.cuda_stream)
    s.synchronize()
    assert acc.cpu().tolist() == want
    dws.close()
    # a laned workspace with deferred joins: small calls coalesced into one launch per kernel
    lw = W(dp, 1024, lanes=0, chunk=512)
    lw.defer_joins(True)
    held = []
    for k, idx in enumerate([range(0, 7), range(7, 20), range(20, 21), range(21, 48), range(0, 48)]):
        sub = _permute(batch, list(idx), n_pi)
        held.append((sub.expected, _device_call(dp, sub, lw, s.cuda_stream, rlc=(k == 3))))
    lw.join(s.cuda_stream)
    s.synchronize()
    for exp, (acc, _keep) in held:
        assert acc.cpu().tolist() == exp
    lw.close()
    # RLC: an all-valid batch passes the batch check; a batch with one pairing-only reject is localised by the fall-back
    rws = be.Workspace(dp, n)
    acc, fell_back = dp.verify_batch_rlc(clean.proofs, clean.proof_off, clean.instances, clean.committed, ws=rws)
    assert list(acc) == [1] * n and (not fell_back or pl.is_recursive)
    rws.close()
    k = 5
    p2, i2 = synth.corrupt(pl, clean.proof(k), clean.instances[32 * n_pi * k:32 * n_pi * (k + 1)], "flip_first_scalar", random.Random(5))
    proofs = [p2 if i == k else clean.proof(i) for i in range(n)]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    one = synth.Batch(n=n, proofs=b"".join(proofs), proof_off=off,
                      instances=clean.instances[:32 * n_pi * k] + i2 + clean.instances[32 * n_pi * (k + 1):],
                      committed=clean.committed, expected=[int(i != k) for i in range(n)])
    rws = be.Workspace(dp, n)
    acc, fell_back = dp.verify_batch_rlc(one.proofs, one.proof_off, one.instances, one.committed, ws=rws)
    assert list(acc) == one.expected and (fell_back or pl.is_recursive)
    rws.close()


def test_rlc_fall_back_with_passing_and_failing_groups(be, wide):  # noqa: F811
    """wide677 under RLC at 256 proofs (four groups of 64, the group stage on): one pairing-only reject in group 2 only.  The
    batch check fails, groups 0, 1 and 3 pass their group checks, and the fall-back's segmented MSM and its fold
    (k_g1_msm_cond_seg / k_g1_msm_merged_cond_seg, k_g1_sum_segments with skip) must still give group 2's other 63 proofs
    their sums: the verdicts equal the construction, under both segmented ladder forms."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = wide["wide677"]
    n, n_pi, k = 256, vk.n_public_inputs, 150
    clean = synth.forge_batch(vk, td, n, seed=31, plan=pl, workers=16)
    p2, i2 = synth.corrupt(pl, clean.proof(k), clean.instances[32 * n_pi * k:32 * n_pi * (k + 1)], "flip_first_scalar", random.Random(7))
    proofs = [p2 if i == k else clean.proof(i) for i in range(n)]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    one = synth.Batch(n=n, proofs=b"".join(proofs), proof_off=off,
                      instances=clean.instances[:32 * n_pi * k] + i2 + clean.instances[32 * n_pi * (k + 1):],
                      committed=clean.committed, expected=[int(i != k) for i in range(n)])
    for lpt in (0, 1, 2):
        ws = be.Workspace(dp, n)
        ws.set_option(be.OPT_MSM_LANES_PER_TERM, lpt)
        acc, fell_back = dp.verify_batch_rlc(one.proofs, one.proof_off, one.instances, one.committed, ws=ws)
        assert fell_back and list(acc) == one.expected, lpt
        ws.close()


def _with_one_reject(pl, clean, n_pi, k, seed):
    from plutus_halo2_verifier_gen_amd import synth
    p2, i2 = synth.corrupt(pl, clean.proof(k), clean.instances[32 * n_pi * k:32 * n_pi * (k + 1)], "flip_first_scalar", random.Random(seed))
    proofs = [p2 if i == k else clean.proof(i) for i in range(clean.n)]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return synth.Batch(n=clean.n, proofs=b"".join(proofs), proof_off=off,
                       instances=clean.instances[:32 * n_pi * k] + i2 + clean.instances[32 * n_pi * (k + 1):],
                       committed=clean.committed, expected=[int(i != k) for i in range(clean.n)])


@pytest.fixture(scope="module")
def narrow_rejects():
    """simple_mul x 256 (four groups of 64): its device plan and three batches with one pairing-only reject each - the first
    proof of group 2, an inner one, its last"""
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    clean = synth.forge_batch(vk, td, 256, seed=37, plan=pl, workers=16)
    return backend.DevicePlan(pl.to_bytes(), 0), [_with_one_reject(pl, clean, vk.n_public_inputs, k, 9 + k) for k in (128, 150, 191)]


@pytest.mark.parametrize("lpt, bs", [(1, 64), (1, 256), (2, 64), (2, 256), (1, 192), (2, 192)])
def test_rlc_fall_back_with_passing_and_failing_groups_narrow(be, narrow_rejects, lpt, bs):  # noqa: F811
    """The narrow twin of the test above: the UNSEGMENTED conditional ladders (k_g1_msm_cond / k_g1_msm_merged_cond) with
    passing and failing groups, under both lane forms.  simple_mul under RLC at 256 proofs, always the batch check first
    (OPT_RLC_ROUTE = -1): the batch check fails, groups 0, 1 and 3 pass their group checks and their logical blocks are
    skipped, group 2's other 63 proofs still need their sums.  The fall-back sums the key's 16 terms per proof in one launch:
    2, 4, 8 or 16 proofs per block at 64 / 256 threads, which divide the groups of 64; 192-thread blocks hold 6 or 12
    proofs, so that a block straddles each border of group 2 (skipped only when BOTH groups it touches passed)."""
    dp, batches = narrow_rejects
    for one in batches:
        ws = be.Workspace(dp, one.n)
        ws.set_option(be.OPT_RLC_ROUTE, -1)
        ws.set_option(be.OPT_MSM_LANES_PER_TERM, lpt)
        ws.set_option(be.OPT_MSM_BLOCK_SIZE, bs)
        acc, fell_back = dp.verify_batch_rlc(one.proofs, one.proof_off, one.instances, one.committed, ws=ws)
        assert fell_back and list(acc) == one.expected, one.expected.index(0)
        ws.close()


def test_wide_ivc_fold_and_separate_ranges(be, wide):  # noqa: F811
    """ivc_wide: F = 113 fixed bases.  At two lanes per term the three sums fill 392 lanes of one block; forcing 256-thread
    blocks makes them run as three separate ranges (segmented where they must be).  el / er after the fold equal the
    oracle's, the accumulator corruptions set their status bits, and every pairing engine gives the same verdicts."""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth
    vk, td, pl, dp, ov = wide["ivc_wide"]
    n_pi = vk.n_public_inputs
    assert pl.n_main_terms == 81 and pl.n_terms - pl.n_main_terms - 1 == 114
    big, mixed = _mixed(vk, td, pl, 64, seed=8, fraction=0.5)
    want = list(ov.verify_batch(mixed.proofs, mixed.proof_off, mixed.instances, None, threads=16))
    assert want == mixed.expected and 0 < sum(want) < mixed.n
    ws = be.Workspace(dp, mixed.n)
    for lpt, bsz, tpl in ((0, 0, 0), (2, 0, 0), (2, 256, 0), (1, 64, 0), (2, 64, 0), (2, 256, 2), (2, 256, 4)):
        ws.set_option(be.OPT_MSM_LANES_PER_TERM, lpt)
        ws.set_option(be.OPT_MSM_BLOCK_SIZE, bsz)
        ws.set_option(be.OPT_MSM_TERMS_PER_LANE, tpl)     # (separate ranges: several terms per lane where the form applies)
        assert list(dp.verify_batch(mixed.proofs, mixed.proof_off, mixed.instances, None, ws=ws)) == want, (lpt, bsz, tpl)
    ws.set_option(be.OPT_MSM_LANES_PER_TERM, 0)
    ws.set_option(be.OPT_MSM_BLOCK_SIZE, 0)
    ws.set_option(be.OPT_MSM_TERMS_PER_LANE, 0)
    hw = be.Workspace(dp, mixed.n)                        # a caller that keeps batches in flight: the hint reaches every range
    hw.hint_in_flight(8)
    hw.set_option(be.OPT_MSM_LANES_PER_TERM, 2)
    hw.set_option(be.OPT_MSM_BLOCK_SIZE, 256)
    assert list(dp.verify_batch(mixed.proofs, mixed.proof_off, mixed.instances, None, ws=hw)) == want
    hw.close()
    for engine in (6, 12, 16, 32, 64):
        ws.set_option(be.OPT_PAIRING_ENGINE, engine)
        assert list(dp.verify_batch(mixed.proofs, mixed.proof_off, mixed.instances, None, ws=ws)) == want, engine
        assert ws.timings().pairing_lanes_per_proof == engine
    ws.close()
    for i in (want.index(1), 0):
        proof = big.proof(i)
        inst = big.instances[32 * n_pi * i:32 * n_pi * (i + 1)]
        ok, otr = ov.verify(proof, big.instance_ints(i, n_pi), None, trace=True)
        tr = dp.trace(proof, inst, None)
        assert ok and tr["accept"] == 1 and tr["el"] == otr.point("el") and tr["er"] == otr.point("er")
        assert tr["msm_scalars"][pl.n_main_terms:] == PL.run_plan(pl, proof, big.instance_ints(i, n_pi), None)[0][pl.n_main_terms:]
    rng = random.Random(6)
    for kind, bit in (("acc_vk_hash", 32), ("acc_limb", 8 | 16), ("acc_sign", 16)):
        p, ins = synth.corrupt(pl, big.proof(1), big.instances[32 * n_pi:64 * n_pi], kind, rng)
        tr = dp.trace(p, ins, None)
        assert tr["accept"] == 0 and tr["status"] & bit, (kind, tr["status"])


def test_bls12381_at_1024(be, wide):  # noqa: F811
    """bls12381 x 1024, as test_baseline_config_sizes checks the existing shapes: the verdict vector equals the construction
    (8 % corruptions of every kind), does not depend on the order of the batch, equals the oracle's on a 64-proof sample, and
    the RLC mode gives the same vector."""
    vk, td, pl, dp, ov = wide["bls12381"]
    n, n_pi = 1024, vk.n_public_inputs
    _, batch = _mixed(vk, td, pl, n, seed=90, fraction=0.08)
    ws = be.Workspace(dp, n)
    got = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
    assert list(got) == batch.expected and 0 < sum(got) < n
    order = list(range(n))
    random.Random(15).shuffle(order)
    perm = _permute(batch, order, n_pi)
    assert list(dp.verify_batch(perm.proofs, perm.proof_off, perm.instances, perm.committed, ws=ws)) == [got[i] for i in order]
    sample = sorted(random.Random(16).sample(range(n), 64))
    sb = _permute(batch, sample, n_pi)
    assert list(ov.verify_batch(sb.proofs, sb.proof_off, sb.instances, sb.committed, threads=16)) == [got[i] for i in sample]
    got_rlc, fell_back = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
    assert list(got_rlc) == list(got) and fell_back
    ws.close()
