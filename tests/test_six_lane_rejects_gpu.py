"""The headline shape with the six-lanes-per-proof pairing engine FORCED (the launcher itself takes it only for callers that keep
the chip full): simple_mul x 4096 holding every way a proof can be turned away - a wrong pi (only the pairing sees it), byte
flips, the pi point at infinity (the engine skips that loop's lines), points that are on the curve but outside the prime-order
subgroup, both of SMALL order (the subgroup ladder's additions meet P + (-P), P + P and infinity) and random curve points (a
large cofactor component: the generic branch) - against the CPU oracle: accept[] proof by proof, status[] by its class."""
import json
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

pytestmark = pytest.mark.gpu
P, R = bls.P, bls.R
H_COFACTOR = 0x396c8c005555e1568c00aaab0000aaab            # #E(Fp) = h r,  h = 3 * 11^2 * 10177^2 * ...
# the oracle's status class -> the device's status bit (include/h2v.h)
CLASS_BIT = {"pairing": 16, "point": 8, "scalar": 1, "short": 4, "inverse": 2, "recursion": 32}


def small_order_points():
    """points of order 3, 11 and 10177 on y^2 = x^3 + 4"""
    out, x = [], 1
    while len(out) < 6:
        x += 1
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is None:
            continue
        for q in (3, 11, 10177):
            t = bls.g1_mul((x, y), H_COFACTOR * R // q)
            if t is not None:
                assert bls.g1_mul(t, q) is None and not bls.g1_in_subgroup(t)
                out.append(t)
    return out


def random_curve_point(rng):
    while True:
        x = rng.randrange(P)
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is not None and not bls.g1_in_subgroup((x, y)):
            return (x, y)


def test_six_lane_engine_full_batch_rejects_match_the_oracle(orc):
    import torch
    from plutus_halo2_verifier_gen_amd import backend as be, plan as PL, synth, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    dp = be.DevicePlan(pl.to_bytes(), 0)
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    n, n_pi = 4096, vk.n_public_inputs
    good = synth.forge_batch(vk, td, n, seed=91, plan=pl, workers=8)
    rng = random.Random(92)
    proofs = [good.proof(i) for i in range(n)]
    insts = [good.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(n)]
    victims = rng.sample(range(n), 700)
    small = small_order_points()
    made = {}
    for j, i in enumerate(victims):
        kind = ("wrong_pi", "flip_first_scalar", "flip_last_scalar", "pi_infinity", "small_order", "large_cofactor", "point_not_on_curve")[j % 7]
        buf = bytearray(proofs[i])
        if kind == "pi_infinity":
            o = pl.points[pl.pi_point]
            buf[o:o + 48] = bls.g1_compress(None)
        elif kind in ("small_order", "large_cofactor"):
            # every slot in turn, the pi point included (its decompression is the same kernel's work)
            o = pl.points[(j // 7) % len(pl.points)]
            buf[o:o + 48] = bls.g1_compress(small[(j // 7) % len(small)] if kind == "small_order" else random_curve_point(rng))
        else:
            buf, insts[i] = synth.corrupt(pl, bytes(buf), insts[i], kind, rng)
        proofs[i] = bytes(buf)
        made[i] = kind
    off = [0]
    for p_ in proofs:
        off.append(off[-1] + len(p_))
    pb, ib = b"".join(proofs), b"".join(insts)

    ws = be.Workspace(dp, n)
    ws.set_option(be.Workspace.OPT_PAIRING_ENGINE, 6)
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    d_p, d_i, d_c = up(pb), up(ib), up(good.committed)
    d_off = torch.tensor(off, dtype=torch.int64).to(dev)
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    dp.verify_batch_device(n, d_p.data_ptr(), d_off.data_ptr(), d_i.data_ptr(), d_c.data_ptr() if d_c is not None else None,
                           acc.data_ptr(), st.data_ptr(), ws=ws)
    torch.cuda.synchronize()
    assert ws.timings().pairing_lanes_per_proof == 6
    got, status = acc.cpu().tolist(), st.cpu().tolist()
    # the host entry point on the same workspace: the same vector
    assert list(dp.verify_batch(pb, off, ib, good.committed, ws=ws)) == got
    ws.close()

    want = list(ov.verify_batch(pb, off, ib, good.committed, threads=16))
    assert got == want
    assert [int(s == 0) for s in status] == want
    assert sum(want) == n - len(victims), "every corruption rejects, nothing else does"
    seen = set()
    for i in victims:
        ok, tr = ov.verify(proofs[i], [int.from_bytes(insts[i][32 * k:32 * k + 32], "little") for k in range(n_pi)], None, trace=True)
        cls = orc.STATUS[tr.status]
        assert not ok and status[i] & CLASS_BIT[cls], (i, made[i], cls, status[i])
        if cls == "pairing":
            assert status[i] == 16, (i, made[i], status[i])      # reached the pairing clean, failed there
        seen.add((made[i], cls))
    # the cases the test is about did occur, with the class they are meant to have
    assert {("wrong_pi", "pairing"), ("pi_infinity", "pairing"), ("small_order", "point"), ("large_cofactor", "point")} <= seen
