"""GPU tests of the keyed blake2b-512 transcript flavour (vk.transcript_hash = {"kind": "blake2b-512"}), all through the
C-ABI.  The hash code itself against hashlib (h2v_probe_blake2b_ex), the combiner's replay against plan.run_plan register by
register on every kernel and schedule, verdicts and status words against the construction (synth.forge_batch / corrupt work
through run_plan, which models the flavour; the CPU oracle knows the Cardano transcript only and is not consulted here),
proofs of one hash under the other's plan, both flavours on one workspace, and the API's tag check."""
import hashlib
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests.test_gpu_parity import be, _permute  # noqa: F401  (module fixture, helper)
from tests.test_prepare_pairs_gpu import _device_run

pytestmark = pytest.mark.gpu
R = bls.R
PAIRING_ONLY = ("flip_first_scalar", "flip_last_scalar", "wrong_pi")
REQUIRED_BIT = {"bad_point_flag": "ST_BAD_POINT", "point_not_on_curve": "ST_BAD_POINT", "point_not_in_subgroup": "ST_BAD_POINT",
                "noncanonical_scalar": "ST_BAD_SCALAR", "noncanonical_instance": "ST_BAD_SCALAR", "truncated": "ST_SHORT_PROOF",
                "acc_vk_hash": "ST_RECURSION"}


@pytest.fixture(scope="module")
def keys(be):
    """name -> (flavoured vk, trapdoor, plan, device plan), made on demand and kept; "<name>/cardano" the key as built"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    made = {}

    def get(name, key=None):
        tag = (name, key)
        if tag not in made:
            base, _, what = name.partition("/")
            vk, td = V.BUILDERS[base]()
            if what != "cardano":
                vk = V.with_transcript_hash(vk, "blake2b-512", key)
            pl = PL.compile_plan(vk)
            made[tag] = (vk, td, pl, be.DevicePlan(pl.to_bytes(), 0))
        return made[tag]
    return get


@pytest.fixture(scope="module")
def pools(keys):
    """name -> 65 accepting proofs forged for that key (forged once, shared, never changed)"""
    from plutus_halo2_verifier_gen_amd import synth
    made = {}

    def get(name, n=65):
        if name not in made:
            vk, td, pl, dp = keys(name)
            made[name] = synth.forge_batch(vk, td, n, seed=91, plan=pl, workers=8, ci_identity=(name.startswith("sha256")))
        return made[name]
    return get


def _with_one_of_each_kind(pl, batch, n_pi, seed):
    """`batch` with one proof of every applicable synth.CORRUPTIONS kind (as many as fit, spread over the batch): the
    batch, and index -> kind"""
    from plutus_halo2_verifier_gen_amd import synth
    rng = random.Random(seed)
    proofs = [batch.proof(i) for i in range(batch.n)]
    insts = [batch.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(batch.n)]
    expected, where = list(batch.expected), {}
    slots = list(range(batch.n))
    rng.shuffle(slots)
    for kind in synth.CORRUPTIONS:
        if not slots:
            break
        res = synth.corrupt(pl, proofs[slots[-1]], insts[slots[-1]], kind, rng)
        if res is None:
            continue
        i = slots.pop()
        proofs[i], insts[i] = res
        expected[i], where[i] = 0, kind
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    return synth.Batch(n=batch.n, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=batch.committed,
                       expected=expected), where


def test_probe_against_hashlib(be):
    """tr_put / tr_digest behind a host-computed state, with a key block in front: every block boundary, both widths, keys
    of 0, 1, 31 and 64 bytes, 65 messages per call (two waves, the second ragged)"""
    rng = random.Random(5)
    keys_ = [b"", b"\x80", b"Domain separator for transcript", bytes(rng.randrange(256) for _ in range(64))]
    for ln in (0, 1, 127, 128, 129, 255, 256, 257):
        msgs = [bytes(rng.randrange(256) for _ in range(ln)) for _ in range(65)]
        for key in keys_:
            for dl in (32, 64):
                got = be.probe_blake2b_ex(msgs, digest_len=dl, key=key)
                assert got == [hashlib.blake2b(m, key=key, digest_size=dl).digest() for m in msgs], (ln, len(key), dl)
    # the unkeyed 32-byte form is the older probe's hash
    msgs = [bytes(rng.randrange(256) for _ in range(77)) for _ in range(3)]
    assert be.probe_blake2b_ex(msgs, digest_len=32) == be.probe_blake2b(msgs)
    with pytest.raises(be.H2VError):
        be.probe_blake2b_ex(msgs, digest_len=48)
    with pytest.raises(be.H2VError):
        be.probe_blake2b_ex(msgs, key=bytes(65))


def _assert_trace_is_run_plan(dp, pl, batch, i, n_pi):
    from plutus_halo2_verifier_gen_amd import plan as PL
    proof = batch.proof(i)
    _sc, regs, status = PL.run_plan(pl, proof, batch.instance_ints(i, n_pi), batch.ci(i))
    assert status is None
    tr = dp.trace(proof, batch.instances[32 * n_pi * i:32 * n_pi * (i + 1)], batch.ci(i))
    assert set(tr["scalars"]) == {slot for slot, _ in pl.trace} and len(pl.trace) > 19
    for slot, reg in pl.trace:
        assert tr["scalars"][slot] == regs[reg], slot
    assert tr["msm_scalars"] == _sc
    return tr


def test_replay_equals_run_plan_on_every_kernel_and_schedule(be, keys, pools):
    """every h2v_trace slot == the run_plan register the plan's trace table names: simple_mul (two lanes per proof), the
    sha256 shape on its narrow schedule, the same with H2V_OPT_COMBINER_SCHEDULE = 2, and a plan whose register file does
    not fit LDS (k_transcript_combiner, the global-register-file kernel: one lane per proof, 885 registers)"""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    for name in ("simple_mul", "sha256"):
        vk, td, pl, dp = keys(name)
        assert pl.vm_lanes == (2 if name == "simple_mul" else 4) and pl.wide is not None
        batch = pools(name)
        for i in (0, 64):
            tr = _assert_trace_is_run_plan(dp, pl, batch, i, vk.n_public_inputs)
            assert tr["accept"] == 1 and tr["status"] == 0
    # the wide schedule: forced for the probes (the trace itself always names the narrow schedule's registers) and for a
    # workspace, where it is what runs - same verdicts as the construction
    vk, td, pl, dp = keys("sha256")
    batch, where = _with_one_of_each_kind(pl, _permute(pools("sha256"), list(range(40)), vk.n_public_inputs), vk.n_public_inputs, 7)
    try:
        be.probe_set_option(be.OPT_COMBINER_SCHEDULE, 2)
        _assert_trace_is_run_plan(dp, pl, pools("sha256"), 1, vk.n_public_inputs)
    finally:
        be.probe_set_option(be.OPT_COMBINER_SCHEDULE, 0)
    for schedule in (2, 1):
        ws = be.Workspace(dp, batch.n)
        ws.set_option(be.OPT_COMBINER_SCHEDULE, schedule)
        assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == batch.expected, schedule
        ws.close()
    # one lane per proof and a register file too large for LDS
    wvk, wtd = V.WIDE_BUILDERS["wide677"]()
    wvk = V.with_transcript_hash(wvk, "blake2b-512")
    wpl = PL.compile_plan(wvk, lanes=1)
    assert wpl.vm_lanes == 1 and wpl.n_regs * 32 * 8 > PL.VM_LDS_BYTES
    wdp = be.DevicePlan(wpl.to_bytes(), 0)
    wb = synth.forge_batch(wvk, wtd, 3, seed=92, plan=wpl, workers=1)
    for i in range(3):
        _assert_trace_is_run_plan(wdp, wpl, wb, i, wvk.n_public_inputs)
    bad = synth.corrupt(wpl, wb.proof(1), wb.instances[32 * wvk.n_public_inputs:64 * wvk.n_public_inputs], "flip_first_scalar", random.Random(1))
    proofs = wb.proof(0) + bad[0] + wb.proof(2)
    off = [0, len(wb.proof(0)), len(wb.proof(0)) + len(bad[0]), len(proofs)]
    got = wdp.verify_batch(proofs, off, wb.instances[:32 * wvk.n_public_inputs] + bad[1] + wb.instances[64 * wvk.n_public_inputs:], wb.committed)
    assert list(got) == [1, 0, 1]


@pytest.mark.parametrize("name,n", [("simple_mul", 1), ("simple_mul", 63), ("simple_mul", 65), ("lookup_table", 65), ("ivc", 33)])
def test_end_to_end_against_the_construction(be, keys, pools, name, n):
    """all valid, and one of each applicable corruption kind; per proof, mode "rlc" and prepare_batch -> check_pairs; accept
    and status vectors as constructed"""
    vk, td, pl, dp = keys(name)
    n_pi = vk.n_public_inputs
    good = _permute(pools(name), list(range(n)), n_pi)
    mixed, where = _with_one_of_each_kind(pl, good, n_pi, seed=n)
    assert len(where) == min(n, len(where)) >= 1 and (n == 1 or (len(where) >= 10 and sum(mixed.expected) > 0))
    for batch, kinds in ((good, {}), (mixed, where)):
        acc, vst, raw, pst, cacc, cst = _device_run(dp, batch)
        assert acc == batch.expected, (name, n)
        assert [int(s == 0) for s in vst] == batch.expected
        for i, kind in kinds.items():
            if kind in PAIRING_ONLY or (kind == "wrong_public_input" and not pl.is_recursive):
                assert vst[i] == be.ST_PAIRING, (kind, vst[i])
            elif kind in REQUIRED_BIT:
                assert vst[i] & getattr(be, REQUIRED_BIT[kind]), (kind, vst[i])
        # prepare -> check_pairs: the same verdicts; prepare's status is verify's without the pairing bit
        assert pst == [v & ~be.ST_PAIRING for v in vst] and cacc == acc
        hraw, hst = dp.prepare_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)
        assert hraw == raw and hst == pst
        hacc, hcst = dp.check_pairs(hraw)
        assert list(hacc) == batch.expected and hcst == cst
        # host forms: per proof and the batch-accept mode
        assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)) == batch.expected
        got, fell_back = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=be.Workspace(dp, max(n, 64)),
                                             seed=bytes(range(32)))
        assert list(got) == batch.expected
        if pl.is_recursive:      # (recursive plans run per proof in this mode unless asked for the form that starts after the fold)
            got, _fb = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=be.Workspace(dp, max(n, 64)),
                                           seed=bytes(range(32)), fold_pairs=True)
            assert list(got) == batch.expected
        elif not kinds:
            assert not fell_back


def test_a_proof_made_under_another_hash_is_rejected_by_the_pairing(be, keys, pools):
    import torch
    cvk, _, cpl, cdp = keys("simple_mul/cardano")
    fvk, _, fpl, fdp = keys("simple_mul")
    _, _, opl, odp = keys("simple_mul", key=b"Domain separator for transcripT")     # the default key with its last byte changed
    assert cpl.proof_len == fpl.proof_len == opl.proof_len
    assert (cdp.transcript_kind, cdp.transcript_key) == (be.TRANSCRIPT_CARDANO_BLAKE2B_256, b"")
    assert (fdp.transcript_kind, fdp.transcript_key) == (be.TRANSCRIPT_BLAKE2B_512, b"Domain separator for transcript")
    assert odp.transcript_key == b"Domain separator for transcripT"
    cb, fb = pools("simple_mul/cardano"), pools("simple_mul")
    for dp, batch, ok in ((cdp, cb, True), (fdp, fb, True), (fdp, cb, False), (cdp, fb, False), (odp, fb, False), (odp, cb, False)):
        acc, vst, raw, pst, cacc, cst = _device_run(dp, batch)
        assert acc == [int(ok)] * batch.n and cacc == acc
        assert vst == [0 if ok else be.ST_PAIRING] * batch.n       # a reject like any forged proof: nothing else is wrong with it
        assert pst == [0] * batch.n
        got, fell_back = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=be.Workspace(dp, batch.n),
                                             seed=bytes(32))
        assert list(got) == acc and fell_back == (not ok)
    torch.cuda.synchronize()


def test_one_workspace_serves_both_flavours(be, keys, pools):
    """h2v_workspace_create_multi over the Cardano plan and the flavoured plan of one circuit; interleaved 64-proof device
    calls with deferred joins (small enough to be coalesced): each call gets its own plan's verdicts.  The proofs of either
    batch all reject under the other plan, so a call replayed under the wrong instantiation cannot pass."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    parts = []
    for name in ("simple_mul/cardano", "simple_mul"):
        vk, td, pl, dp = keys(name)
        b, _ = _with_one_of_each_kind(pl, _permute(pools(name), list(range(64)), vk.n_public_inputs), vk.n_public_inputs, seed=len(name))
        assert 0 < sum(b.expected) < 64
        parts.append((name, dp, b, (up(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64).to(dev), up(b.instances))))
    ws = be.Workspace.multi([p[1] for p in parts], 1024, lanes=2, chunk=256)
    ws.defer_joins(True)
    s = torch.cuda.Stream(device=dev)
    for rlc in (False, True):
        held = []
        for r in range(3):
            for name, dp, b, d in parts:
                acc = torch.full((64,), 7, dtype=torch.uint8, device=dev)
                st = torch.full((64,), -1, dtype=torch.int32, device=dev)
                args = (64, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, acc.data_ptr(), st.data_ptr())
                if rlc:
                    dp.verify_batch_rlc_device(*args, ws=ws, stream=s.cuda_stream, seed=bytes(range(32)))
                else:
                    dp.verify_batch_device(*args, ws=ws, stream=s.cuda_stream)
                held.append((name, b, acc, st))
        ws.join(s.cuda_stream)
        s.synchronize()
        for name, b, acc, st in held:
            assert acc.cpu().tolist() == b.expected, (name, rlc)
            assert [int(x == 0) for x in st.cpu().tolist()] == b.expected, (name, rlc)
    ws.close()


def test_api_tags(be, keys, pools):
    from plutus_halo2_verifier_gen_amd import api
    fvk, _, fpl, _ = keys("simple_mul")
    cvk = keys("simple_mul/cardano")[0]
    fb, cb = pools("simple_mul"), pools("simple_mul/cardano")
    pubs = fb.instance_ints(0, fvk.n_public_inputs)
    before = set(api._VERIFIERS)
    with pytest.raises(ValueError, match="transcript hash mismatch"):     # misuse: nothing is compiled, loaded or launched
        api.prepare(fvk, [[]], [[pubs]], api.CircuitTranscript.init_from_bytes(fb.proof(0)))
    assert set(api._VERIFIERS) == before
    api.prepare(fvk, [[]], [[pubs]], api.CircuitTranscript.init_from_bytes(fb.proof(0), hash=api.BLAKE2B_512)).verify()
    assert api.verifier_for(fvk).device_plan.transcript_kind == be.TRANSCRIPT_BLAKE2B_512
    with pytest.raises(ValueError, match="transcript hash mismatch"):
        api.prepare(cvk, [[]], [[pubs]], api.CircuitTranscript.init_from_bytes(cb.proof(0), hash=api.BLAKE2B_512))
    # the right tag on a proof that was made under the other hash: a reject, not an error
    wrong = lambda: api.prepare(fvk, [[]], [[cb.instance_ints(0, cvk.n_public_inputs)]],
                                api.CircuitTranscript.init_from_bytes(cb.proof(0), hash=api.BLAKE2B_512))
    assert wrong().check() is False
    assert api.Verifier(fvk, plan=fpl).verify_batch([fb.proof(i) for i in range(3)], [fb.instance_ints(i, fvk.n_public_inputs) for i in range(3)],
                                                     mode="rlc") == [True] * 3
