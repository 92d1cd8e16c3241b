"""The records a mixed call takes (include/h2v.h: h2v_verify_mixed), counted through the public interface on a fresh workspace:
one per phase-1 unit - the grouped unit if the call has one, then every key that runs a sub-batch of its own - and the tail's,
which is the call's last.  A fold call whose check fails runs a second pass, which takes its own.  The counts are what the
schedule implies, for an ordinary and for a laned workspace and for every flag set; the verdicts are by construction (forged
proofs, one of them with public inputs that only the pairing rejects, checked with the oracle).

Keys: simple_mul of the shared fixture (tests/test_mixed_keys_gpu.py) and two simple_mul keys of other builder seeds on the
common SRS - three different keys of one shape, so that an ORDINARY workspace of one of them fits the call (a workspace over
several plans, h2v_workspace_create_multi, is always laned)."""
import json

import pytest

from plutus_halo2_verifier_gen_amd import synth
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S
from tests.test_mixed_keys_gpu import SEED, fx  # noqa: F401
from tests.test_mixed_fold_gpu import _with_one_reject
from tests.test_mixed_grouped_gpu import Call, _n_records, _spread

pytestmark = pytest.mark.gpu
KEYS = ("simple_mul", "m00", "m01")                              # all three groupable
P = len(KEYS)
FLAG_SETS = {"none": dict(mode="per-proof"), "rlc": dict(mode="rlc"), "fold": dict(mode="rlc", fold_msm=True),
             "grouped": dict(mode="rlc", fold_msm=True, grouped=True)}


@pytest.fixture(scope="module")
def kx(be, fx, orc):
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    keys, clean = {"simple_mul": fx["keys"]["simple_mul"]}, {"simple_mul": fx["clean"]["simple_mul"]}
    for k, name in enumerate(KEYS[1:]):
        vk, td = V.on_srs(*V.simple_mul_vk(seed=0x7100 + k), COMMON_S)
        pl = PL.compile_plan(vk)
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0), "ov": ov}
        clean[name] = b = synth.forge_batch(vk, td, 8, seed=800 + k, plan=pl, workers=1)
        assert list(ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == b.expected == [1] * 8
    assert len({keys[name]["pl"].to_bytes() for name in KEYS}) == P
    bad = dict(clean)
    bad["m00"] = _with_one_reject({"keys": keys, "clean": clean}, "m00", 5)
    return {"keys": keys, "clean": clean, "bad": bad, "order": _spread([(name, j) for name in KEYS for j in range(8)])}


def _ws(be, kx, laned):
    plans = [kx["keys"][name]["dp"] for name in KEYS]
    ws = be.Workspace.multi(plans, 64, lanes=2, chunk=8) if laned else be.Workspace(plans[0], 64)
    assert ws.lanes() == ((2, 8) if laned else (1, 64))
    assert _n_records(be, ws) == 0
    return ws


def _run(be, call, ws, flags):
    acc, st, fb = be.verify_mixed(call.plans, call.plan_of, call.proofs, call.off, call.instances, call.committed, ws=ws,
                                  seed=SEED if flags["mode"] == "rlc" else None, **flags)
    return list(acc), st, fb


@pytest.mark.parametrize("laned", [False, True], ids=["ordinary", "lanes2x8"])
@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_all_accepting_call_takes_one_record_per_unit_and_the_tails(be, kx, laned, flags):
    """three keys, 8 proofs each, all accepting: P + 1 = 4 records, or 2 with H2V_MIXED_GROUPED (every key is groupable: ONE
    phase-1 unit); the last record is the tail's - h2v_workspace_rlc_result(0) answers for the RLC kinds and says "passed",
    h2v_workspace_timings(0) answers for the plain form (a pairing ran: pairing_ms > 0; in the sub-batch's record before it none)"""
    call = Call(kx["keys"], kx["clean"], KEYS, kx["order"])
    assert call.n == 24 and len(set(call.plan_of)) == P
    ws = _ws(be, kx, laned)
    assert _run(be, call, ws, FLAG_SETS[flags]) == ([1] * 24, [0] * 24, False)
    if flags == "none":
        assert ws.timings(0).pairing_ms > 0 and ws.timings(1).pairing_ms == 0
        with pytest.raises(be.H2VError):
            ws.rlc_result(0, timings=False)
    else:
        assert ws.rlc_result(0, timings=False)[0]
        with pytest.raises(be.H2VError):
            ws.rlc_result(1, timings=False)                      # (the record before the tail's is a prepare call's)
    assert _n_records(be, ws) == (2 if flags == "grouped" else P + 1)
    ws.close()


@pytest.mark.parametrize("laned", [False, True], ids=["ordinary", "lanes2x8"])
@pytest.mark.parametrize("flags", ["fold", "grouped"])
def test_a_failed_fold_check_takes_the_records_of_two_passes(be, kx, laned, flags):
    """one proof that only the pairing rejects: the fold form's check fails and the H2V_MIXED_RLC path runs on the same inputs.
    The fold form takes 2 x (P + 1) records - the first pass plus the second; the grouped form 2 + (P + 1): its first pass has ONE
    phase-1 unit, its second pass is ungrouped.  The last record is the second pass's tail: kind RLC, check failed; so is the
    first pass's tail, P + 1 records back."""
    call = Call(kx["keys"], kx["bad"], KEYS, kx["order"])
    hit = call.order.index(("m00", 5))
    ws = _ws(be, kx, laned)
    assert _run(be, call, ws, FLAG_SETS[flags]) == ([int(i != hit) for i in range(24)], [be.ST_PAIRING if i == hit else 0 for i in range(24)], True)
    assert not ws.rlc_result(0, timings=False)[0]
    with pytest.raises(be.H2VError):
        ws.rlc_result(1, timings=False)
    assert not ws.rlc_result(P + 1, timings=False)[0]
    first = 2 if flags == "grouped" else P + 1
    assert _n_records(be, ws) == first + P + 1
    ws.close()
