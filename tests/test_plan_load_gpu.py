"""h2v_plan_load on the device: every table the loader builds - the VK window tables, the fixed-base tables at each window width,
the six-lane line constants, the fold terms of a recursive plan, the keyed transcript's midstate - is used by a batch of 4 proofs
(3 valid, 1 with a flipped scalar) on the per-proof path and on the batch-accept path, and what the plan's own entry points answer
is the Python plan's.  Then the plan is freed, loaded again and verified again: the same answers.  The oracle knows the Cardano
transcript only; for the keyed plan the construction (synth) says what to expect, as in tests/test_transcript_hash_gpu.py.
Failures of device allocation are not provoked."""
import json
import random

import pytest

from plutus_halo2_verifier_gen_amd import plan as PL, seed as SEED, synth
from plutus_halo2_verifier_gen_amd import vk as V
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
CASES = [("simple_mul", None, 0), ("ivc", None, 0), ("simple_mul", "blake2b-512", 0), ("simple_mul", None, 4), ("simple_mul", None, 8),
         ("simple_mul", None, 12)]


@pytest.fixture(scope="module")
def material(orc):
    """(name, flavour) -> (plan, batch of 4 with proof 2 corrupted, accept[] and the reject reasons by the oracle or the construction)"""
    made = {}

    def get(name, flavour):
        if (name, flavour) not in made:
            vk, td = V.BUILDERS[name]()
            if flavour:
                vk = V.with_transcript_hash(vk, flavour)
            pl = PL.compile_plan(vk)
            good = synth.forge_batch(vk, td, 4, seed=61, plan=pl, workers=1)
            n_pi = vk.n_public_inputs
            proofs = [good.proof(i) for i in range(4)]
            insts = [good.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(4)]
            proofs[2], insts[2] = synth.corrupt(pl, proofs[2], insts[2], "flip_first_scalar", random.Random(7))
            off = [0]
            for p in proofs:
                off.append(off[-1] + len(p))
            batch = synth.Batch(n=4, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=good.committed,
                                expected=[1, 1, 0, 1])
            if flavour:
                reasons = ["accept", "accept", "pairing", "accept"]
            else:
                ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
                reasons = [orc.STATUS[ov.verify(batch.proof(i), batch.instance_ints(i, n_pi), batch.ci(i), trace=True)[1].status] for i in range(4)]
                assert list(ov.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, threads=2)) == batch.expected
            assert reasons == ["accept", "accept", "pairing", "accept"]
            made[(name, flavour)] = (pl, batch, reasons)
        return made[(name, flavour)]
    return get


def _answers(be, dp, batch):
    """accept[] and status[] of the per-proof path and of the batch-accept path (host forms for accept, device forms for both)"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    ws = be.Workspace(dp, batch.n)
    ws.set_option(be.OPT_RLC_ROUTE, -1)            # the batch check first, whatever the call before it met
    args = (batch.proofs, batch.proof_off, batch.instances, batch.committed)
    out = {"verify": list(dp.verify_batch(*args, ws=ws)), "rlc": list(dp.verify_batch_rlc(*args, ws=ws, seed=bytes(range(32)), fold_pairs=True)[0])}
    d_p, d_i, d_c = up(batch.proofs), up(batch.instances), up(batch.committed)
    d_off = torch.tensor(batch.proof_off, dtype=torch.int64).to(dev)
    s = torch.cuda.Stream(device=dev)
    for form, call in (("verify", dp.verify_batch_device), ("rlc", lambda *a, **k: dp.verify_batch_rlc_device(*a, seed=bytes(range(32)), fold_pairs=True, **k))):
        acc = torch.zeros(batch.n, dtype=torch.uint8, device=dev)
        st = torch.zeros(batch.n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call(batch.n, ptr(d_p), ptr(d_off), ptr(d_i), ptr(d_c), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream)
        ws.join(s.cuda_stream)
        s.synchronize()
        out[form + "_device"] = acc.cpu().tolist()
        out[form + "_status"] = [v & 0xffffffff for v in st.cpu().tolist()]
    ws.close()
    return out


@pytest.mark.parametrize("name,flavour,bits", CASES, ids=lambda v: str(v))
def test_load_verify_free_load_verify(be, material, name, flavour, bits):
    pl, batch, reasons = material(name, flavour)
    blob = pl.to_bytes()
    seen = []
    for _round in range(2):
        dp = be.DevicePlan(blob, 0, fixed_base_window_bits=bits)
        # what the plan's own entry points answer
        assert (dp.proof_len, dp.n_pi, dp.n_ci, dp.n_terms) == (pl.proof_len, pl.n_pi, pl.n_ci, pl.n_terms)
        assert (dp.transcript_kind, dp.transcript_key) == (pl.transcript_kind, bytes(pl.transcript_key))
        assert dp.key_tag == SEED.key_tag(blob) and dp.trace_slots == [slot for slot, _ in pl.trace]
        other = be.DevicePlan(blob, 0)
        assert be.lib().h2v_plan_same_srs(dp.handle, other.handle) == 1
        other.close()
        got = _answers(be, dp, batch)
        want_acc = [int(r == "accept") for r in reasons]
        assert got["verify"] == got["verify_device"] == got["rlc"] == got["rlc_device"] == want_acc == batch.expected
        assert got["verify_status"] == [0 if r == "accept" else be.ST_PAIRING for r in reasons]
        assert [int(s == 0) for s in got["rlc_status"]] == want_acc and all(s == 0 or s & be.ST_PAIRING for s in got["rlc_status"])
        seen.append(got)
        dp.close()
    assert seen[0] == seen[1]
