"""GPU tests of derived batch seeds (H2V_RLC_SEED_TRANSCRIPT, include/h2v.h).  The digest kernels alone
against the public model (plutus_halo2_verifier_gen_amd/seed.py) through h2v_probe_batch_seed, bit for bit; then every call that
takes the flag: the pair of an aggregate call is the big-integer model's (tests/agg_model.py) under the MODEL's seed, the same
across calls, workspaces and forms; the verify and pair-check forms keep their contracts; misuse is H2V_E_ARG; a call without the
flag is what it was.  /root/reference is NOT needed."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import seed as S, synth
from tests import agg_model, cancel
from tests.test_aggregate_gpu import REJECTS, _corrupted
from tests.test_batch_cancellation_gpu import _Up
from tests.test_gpu_parity import _permute, be  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
GIVEN = bytes(range(40, 72))
E_ARG = "h2v error -1"


# ---------------------------------------------------------------------------------------------- the digest kernels alone
def _random_batch(rng, n, n_pi, n_ci, off0, lengths):
    proofs = [rng.randbytes(rng.choice(lengths)) for _ in range(n)]
    off = [off0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return rng.randbytes(off0) + b"".join(proofs), off, rng.randbytes(32 * n_pi * n), rng.randbytes(48 * n_ci * n)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097])
def test_digest_kernels_at_every_tree_shape(be, n):
    """one level (1 .. 64), two (65 .. 4096), three with a lone child at the top (4097); proofs of every length mod 128"""
    rng = random.Random(1000 + n)
    tag = rng.randbytes(32)
    proofs, off, inst, ci = _random_batch(rng, n, 1, 1, 0, list(range(0, 400)))
    got = be.probe_batch_seed(1, tag, proofs, off, inst, ci, n_pi=1, n_ci=1)
    assert got == S.batch_seed_flat(tag, proofs, off, inst, ci, n_pi=1, n_ci=1)
    pairs = rng.randbytes(96 * n)
    assert be.probe_batch_seed(2, tag, pairs) == S.pairs_seed(tag, pairs)


def test_digest_kernels_four_levels(be):
    """n = 262145 pairs (25 MB): 4097 / 65 / 2 / 1 nodes"""
    n = 262145
    assert S.level_counts(n) == [4097, 65, 2, 1]
    rng = random.Random(4)
    tag = rng.randbytes(32)
    pairs = rng.randbytes(96 * n)
    assert be.probe_batch_seed(2, tag, pairs) == S.pairs_seed(tag, pairs)


@pytest.mark.parametrize("off0", [0, 3, 48])
def test_digest_kernels_ragged_proofs_and_alignments(be, off0):
    """proofs of 0, 1, 127, 128, 129, 255 and 256 bytes mixed in one batch - so that every source alignment meets every block
    boundary -, behind a first offset of 0, 3 and 48; n_pi = 0, 1, 3 and n_ci = 0, 1"""
    rng = random.Random(77 + off0)
    tag = rng.randbytes(32)
    for n_pi in (0, 1, 3):
        for n_ci in (0, 1):
            proofs, off, inst, ci = _random_batch(rng, 70, n_pi, n_ci, off0, [0, 1, 127, 128, 129, 255, 256])
            assert {b - a for a, b in zip(off, off[1:])} == {0, 1, 127, 128, 129, 255, 256}
            got = be.probe_batch_seed(1, tag, proofs, off, inst or None, ci or None, n_pi=n_pi, n_ci=n_ci)
            assert got == S.batch_seed_flat(tag, proofs, off, inst, ci, n_pi=n_pi, n_ci=n_ci), (n_pi, n_ci)
    # every proof empty; one proof of one byte at an odd address
    assert be.probe_batch_seed(1, tag, b"x" * 8, [off0 % 8] * 6, None, None) == S.batch_seed_flat(tag, b"x" * 8, [off0 % 8] * 6)
    assert be.probe_batch_seed(1, tag, b"abcdefgh", [off0 % 8, off0 % 8 + 1], None, None) == S.batch_seed_flat(tag, b"abcdefgh", [off0 % 8, off0 % 8 + 1])


# ---------------------------------------------------------------------------------------------- the calls
@pytest.fixture(scope="module")
def sm(be):
    """simple_mul: 130 accepting proofs, the same with rejects of every kind, and of both the pair of every proof from
    h2v_prepare_batch - computed once, shared, never changed"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    blob = pl.to_bytes()
    dp = be.DevicePlan(blob, 0)
    assert dp.key_tag == S.key_tag(blob)                           # the host blake2b of h2v_plan_load
    n_pi = vk.n_public_inputs
    clean = synth.forge_batch(vk, td, 130, seed=71, plan=pl, workers=8)
    rej = _corrupted(pl, clean, n_pi, REJECTS)
    out = {"vk": vk, "td": td, "pl": pl, "dp": dp, "n_pi": n_pi, "clean": clean, "rej": rej, "pairs": {}}
    for tag in ("clean", "rej"):
        b = out[tag]
        raw, st = dp.prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
        out["pairs"][tag] = ([raw[96 * i:96 * i + 96] for i in range(b.n)], [int(s == 0) for s in st], st)
    assert out["pairs"]["clean"][1] == [1] * 130 and sum(out["pairs"]["rej"][1]) == 130 - 5
    return out


def _model_seed(fx, b):
    return S.batch_seed_flat(fx["dp"].key_tag, b.proofs, b.proof_off, b.instances, b.committed or b"", n_pi=fx["n_pi"], n_ci=1 if b.committed else 0)


def _agg_device(dp, b, ws, **kw):
    """(pair, included, status, info) of the device form on a stream of its own"""
    import torch
    up = _Up(b)
    pair = torch.full((96,), 7, dtype=torch.uint8, device=up.acc.device)
    info = dp.aggregate_batch_device(*up.args[:5], pair.data_ptr(), up.acc.data_ptr(), up.st.data_ptr(), ws=ws, stream=up.stream.cuda_stream, **kw)
    inc, st = up.results()
    return bytes(pair.cpu().numpy().tobytes()), inc, st, info


@pytest.mark.parametrize("n", [1, 2, 65, 130])
def test_aggregate_is_reproducible(be, sm, n):
    dp, n_pi = sm["dp"], sm["n_pi"]
    for tag in ("rej", "clean"):
        b = _permute(sm[tag], list(range(n)), n_pi)
        pairs_i, reached, pst = (x[:n] for x in sm["pairs"][tag])
        want_seed = _model_seed(sm, b)
        want = agg_model.model_pair(pairs_i, reached, want_seed)
        ws, ws2 = be.Workspace(dp, n), be.Workspace(dp, max(n, 200))
        assert ws.lanes() == (1, n)
        got = []
        for w in (ws, ws, ws2, None):                               # two calls, two workspaces, a temporary one
            pair, inc, st, info = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=w, derive_seed=True)
            assert (info.seed_source, bytes(info.seed_used), info.chunk, info.n_chunks) == (1, want_seed, 0, 1), tag
            assert (list(inc), st) == (reached, pst)
            if w is not None:
                assert w.seed_used() == want_seed and w.rlc_verdict() == be.BATCH_NOT_CHECKED
            got.append(pair)
        for w in (ws, ws2):                                         # the device form: the info has no seed yet, the getter has
            pair, inc, st, info = _agg_device(dp, b, w, derive_seed=True)
            assert (info.seed_source, bytes(info.seed_used)) == (1, bytes(32))
            assert (inc, st) == (reached, pst) and w.seed_used() == want_seed
            got.append(pair)
        assert got == [want] * 6, (tag, n)
        # one instance byte of one proof: another seed, another pair (the proof itself now fails its own equation or not - the
        # pair is still the model's over what h2v_prepare_batch says of the changed batch)
        k = n // 2
        inst = bytearray(b.instances)
        inst[32 * n_pi * k] ^= 1
        pair2, inc2, _st2, info2 = dp.aggregate_batch(b.proofs, b.proof_off, bytes(inst), b.committed, ws=ws, derive_seed=True)
        seed2 = S.batch_seed_flat(dp.key_tag, b.proofs, b.proof_off, bytes(inst), b.committed or b"", n_pi=n_pi)
        assert bytes(info2.seed_used) == seed2 != want_seed and pair2 != want
        raw2, st2 = dp.prepare_batch(b.proofs, b.proof_off, bytes(inst), b.committed)
        assert pair2 == agg_model.model_pair([raw2[96 * i:96 * i + 96] for i in range(n)], [int(s == 0) for s in st2], seed2)
        ws.close()
        ws2.close()


def test_laned_workspace_whole_call_seed_per_chunk_tweak(be, sm):
    """chunk 64 x 3 lanes, n = 130: two full chunks and a two-proof tail; ONE seed over the whole call, tweaked per chunk"""
    dp, b = sm["dp"], sm["rej"]
    pairs_i, reached, pst = sm["pairs"]["rej"]
    want_seed = _model_seed(sm, b)
    ws = be.Workspace(dp, 130, lanes=3, chunk=64)
    assert ws.lanes() == (3, 64)
    want = agg_model.model_pair(pairs_i, reached, want_seed, 64)
    for form in ("host", "device", "host"):
        if form == "host":
            pair, inc, st, info = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, derive_seed=True)
            assert bytes(info.seed_used) == want_seed
        else:
            pair, inc, st, info = _agg_device(dp, b, ws, derive_seed=True)
        assert (info.seed_source, info.chunk, info.n_chunks) == (1, 64, 3)
        assert pair == want and (list(inc), st) == (reached, pst) and ws.seed_used() == want_seed, form
    plain = be.Workspace(dp, 130)
    pair0, _inc, _st, info0 = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=plain, derive_seed=True)
    assert bytes(info0.seed_used) == want_seed and pair0 != want and pair0 == agg_model.model_pair(pairs_i, reached, want_seed)
    plain.close()
    ws.close()


def _verify_device(dp, b, ws, **kw):
    up = _Up(b)
    dp.verify_batch_rlc_device(*up.args, ws=ws, stream=up.stream.cuda_stream, **kw)
    return up.results()


def test_verify_form(be, sm):
    """accept[] / status[] are the per-proof call's with rejects of every kind; the getter has the model's seed; an all-accepting
    batch passes its check; a pair built to cancel under equal weights is rejected"""
    dp, n_pi = sm["dp"], sm["n_pi"]
    ws = be.Workspace(dp, 130)
    ws.set_option(be.OPT_RLC_ROUTE, -1)                             # (every call here runs its batch check: test_routed_call.. has the rest)
    b = sm["rej"]
    up = _Up(b)
    dp.verify_batch_device(*up.args, ws=ws, stream=up.stream.cuda_stream)
    per_proof = up.results()
    assert per_proof[0] == b.expected
    assert _verify_device(dp, b, ws, derive_seed=True) == per_proof
    assert ws.seed_used() == _model_seed(sm, b) and ws.rlc_result(timings=False)[0] is False
    acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, derive_seed=True)      # the host form
    assert (list(acc), fb) == (b.expected, True) and ws.seed_used() == _model_seed(sm, b)
    laned = be.Workspace(dp, 130, lanes=3, chunk=64)
    assert _verify_device(dp, b, laned, derive_seed=True) == per_proof and laned.seed_used() == _model_seed(sm, b)
    laned.close()
    c = sm["clean"]
    assert _verify_device(dp, c, ws, derive_seed=True) == ([1] * 130, [0] * 130)
    assert ws.rlc_result(timings=False)[0] is True and ws.seed_used() == _model_seed(sm, c)
    # two proofs whose errors cancel under EQUAL weights, at positions in two 64-proof blocks
    recs = [cancel.rec_of(sm, c, j) for j in (0, 1)]
    pa, pb = cancel.cancelling(recs[0], recs[1], 1, 1, 0x1d2c3b4a5968778695a4b3c2d1e0f)
    proofs = [c.proof(i) for i in range(130)]
    proofs[5], proofs[69] = pa, pb
    insts = [c.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(130)]
    insts[5], insts[69] = insts[0], insts[1]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    x = synth.Batch(n=130, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=c.committed, expected=None)
    acc, st = _verify_device(dp, x, ws, derive_seed=True)
    assert [i for i, a in enumerate(acc) if a != 1] == [5, 69] and [i for i, s in enumerate(st) if s] == [5, 69]
    assert st[5] == st[69] == be.ST_PAIRING and ws.rlc_result(timings=False)[0] is False
    ws.close()


def test_routed_call_derives_nothing(be, sm):
    """every group of the first call fails, so routing sends the second straight to the per-proof kernels: the same verdicts,
    no seed; the estimate moved as for any RLC call"""
    dp, b = sm["dp"], sm["rej"]
    ws = be.Workspace(dp, 130)
    first = _verify_device(dp, b, ws, derive_seed=True)
    assert ws.seed_used() == _model_seed(sm, b)
    assert _verify_device(dp, b, ws, derive_seed=True) == first == (b.expected, first[1])
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used()
    assert ws.seed_used(1) == _model_seed(sm, b)                    # the first call's is still there
    ws.close()


@pytest.mark.parametrize("n", [1, 65])
def test_pair_check(be, sm, n):
    """h2v_check_pairs_rlc with the flag: form 2 of the rule; one bad pair among n"""
    dp = sm["dp"]
    pairs_i = sm["pairs"]["clean"][0][:n]
    ws = be.Workspace(dp, 130)
    good = b"".join(pairs_i)
    for form in ("host", "device"):
        for raw, want_acc in ((good, [1] * n), (good[:96 * (n - 1)] + pairs_i[-1][:48] + sm["pairs"]["clean"][0][100][48:], [1] * (n - 1) + [0])):
            if form == "host":
                acc, st, fb = dp.check_pairs_rlc(raw, ws=ws, derive_seed=True)
                acc = list(acc)
            else:
                up = _Up(pairs=raw)
                dp.check_pairs_rlc_device(*up.args, ws=ws, stream=up.stream.cuda_stream, derive_seed=True)
                acc, st = up.results()
                fb = not ws.rlc_result(timings=False)[0]
            assert (acc, fb) == (want_acc, want_acc[-1] == 0), form
            assert st == [0 if a else be.ST_PAIRING for a in want_acc]
            assert ws.seed_used() == S.pairs_seed(dp.key_tag, raw)
            assert (acc, st) == tuple(map(list, dp.check_pairs(raw, ws=ws)))
    ws.close()


def test_recursive_key_on_its_fold_pairs_route(be):
    """the ivc circuit, n = 3, through h2v_aggregate_batch: the leaf binds the INPUTS, the pair is the model's on the folded pairs"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td = V.BUILDERS["ivc"]()
    pl = PL.compile_plan(vk)
    dp = be.DevicePlan(pl.to_bytes(), 0)
    n_pi = vk.n_public_inputs
    b = synth.forge_batch(vk, td, 3, seed=5, plan=pl)
    raw, st = dp.prepare_batch(b.proofs, b.proof_off, b.instances, b.committed)
    assert st == [0, 0, 0]
    want_seed = S.batch_seed_flat(dp.key_tag, b.proofs, b.proof_off, b.instances, b.committed or b"", n_pi=n_pi, n_ci=dp.n_ci)
    want = agg_model.model_pair([raw[96 * i:96 * i + 96] for i in range(3)], [1, 1, 1], want_seed)
    ws = be.Workspace(dp, 8)
    for _ in range(2):
        pair, inc, _st, info = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, derive_seed=True)
        assert (pair, list(inc), info.seed_source, bytes(info.seed_used)) == (want, [1, 1, 1], 1, want_seed)
    acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, fold_pairs=True, derive_seed=True)
    assert (list(acc), fb) == ([1, 1, 1], False) and ws.seed_used() == want_seed
    # without fold_pairs a recursive plan runs per proof: nothing is derived
    acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, derive_seed=True)
    assert list(acc) == [1, 1, 1]
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used()
    ws.close()


def test_misuse(be, sm):
    dp, b = sm["dp"], _permute(sm["clean"], [0, 1, 2, 3], sm["n_pi"])
    ws = be.Workspace(dp, 16)
    args = (b.proofs, b.proof_off, b.instances, b.committed)
    with pytest.raises(be.H2VError, match=E_ARG):                   # the flag beside a given seed, every form
        dp.aggregate_batch(*args, ws=ws, seed=GIVEN, derive_seed=True)
    with pytest.raises(be.H2VError, match=E_ARG):
        dp.verify_batch_rlc(*args, ws=ws, seed=GIVEN, derive_seed=True)
    with pytest.raises(be.H2VError, match=E_ARG):
        dp.check_pairs_rlc(bytes(96), ws=ws, seed=GIVEN, derive_seed=True)
    up = _Up(b)
    with pytest.raises(be.H2VError, match=E_ARG):
        dp.verify_batch_rlc_device(*up.args, ws=ws, stream=up.stream.cuda_stream, seed=GIVEN, derive_seed=True)
    # the mixed calls
    import ctypes as C
    flag = be.RlcOpts((C.c_uint8 * 32)(), be.RLC_SEED_TRANSCRIPT)
    mws = be.Workspace.multi([dp], 16)
    n = b.n
    off = (C.c_uint64 * (n + 1))(*b.proof_off)
    po = (C.c_uint32 * n)()
    pbuf, ibuf = C.create_string_buffer(b.proofs, len(b.proofs)), C.create_string_buffer(b.instances, len(b.instances))
    mb = be.MixedBatch(n, C.cast(po, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p), C.cast(ibuf, C.c_void_p), None)
    plans = (C.c_void_p * 1)(dp.handle)
    acc, st, pair = (C.c_uint8 * n)(), (C.c_uint32 * n)(), C.create_string_buffer(96)
    L = be.lib()
    for mflags in (0, be.MIXED_RLC, be.MIXED_RLC | be.MIXED_FOLD_MSM):
        assert L.h2v_verify_mixed(plans, 1, C.byref(mb), acc, st, mws.handle, mflags, C.byref(flag), None) == -1
        assert L.h2v_verify_mixed_device(plans, 1, C.byref(mb), acc, st, mws.handle, None, mflags, C.byref(flag)) == -1
    assert L.h2v_aggregate_mixed(plans, 1, C.byref(mb), pair, acc, st, mws.handle, C.byref(flag), None) == -1
    assert L.h2v_aggregate_mixed_device(plans, 1, C.byref(mb), C.addressof(pair), acc, st, mws.handle, None, C.byref(flag), None) == -1
    # the getter on calls without the flag
    dp.aggregate_batch(*args, ws=ws, seed=GIVEN)
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used()
    dp.verify_batch(*args, ws=ws)
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used()
    with pytest.raises(be.H2VError, match=E_ARG):
        ws.seed_used(63)
    # ... after all of which the workspaces are still usable
    pair, inc, _st, info = dp.aggregate_batch(*args, ws=ws, derive_seed=True)
    assert list(inc) == [1] * 4 and ws.seed_used() == bytes(info.seed_used) == _model_seed(sm, b)
    with pytest.raises(be.H2VError, match=E_ARG):                   # one call back: the call with a given seed
        ws.seed_used(1)
    acc2, st2, fb = be.verify_mixed([dp], [0] * n, *args, ws=mws, mode="rlc")
    assert (list(acc2), fb) == ([1] * 4, False)
    mws.close()
    ws.close()


def test_a_call_without_the_flag_is_what_it_was(be, sm):
    """the seed_dev == NULL path: a given seed, and the pair agg_model predicts from info.seed_used, on both kinds of workspace"""
    dp, b = sm["dp"], sm["rej"]
    pairs_i, reached, pst = sm["pairs"]["rej"]
    for ws, chunk in ((be.Workspace(dp, 130), 0), (be.Workspace(dp, 130, lanes=3, chunk=64), 64)):
        pair, inc, st, info = dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, seed=GIVEN)
        assert info.seed_source == 0 and bytes(info.seed_used)[:20] == GIVEN[:20] and bytes(info.seed_used)[28:] == GIVEN[28:]
        assert info.chunk == chunk and (list(inc), st) == (reached, pst)
        assert pair == agg_model.model_pair(pairs_i, reached, bytes(info.seed_used), chunk)
        # a derived call in between leaves the next given-seed call alone
        dp.aggregate_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, derive_seed=True)
        pair, inc, st, info = _agg_device(dp, b, ws, seed=GIVEN)
        assert info.seed_source == 0 and pair == agg_model.model_pair(pairs_i, reached, bytes(info.seed_used), chunk)
        acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, seed=GIVEN)
        assert (list(acc), fb) == (b.expected, True)
        ws.close()
