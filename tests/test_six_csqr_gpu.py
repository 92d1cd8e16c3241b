"""The six-lane pairing engine's FINAL value - after all 315 cyclotomic squarings of the hard part (four products per lane:
csrc/h2v_pairing_six.hpp: six_csqr_products, six_csqr_run) - coefficient by coefficient against the big-integer replay of the generated program
(tools/gen_coop_program.py: simulate), on accepting and on rejecting pairs: a rejecting pair carries twelve non-trivial
coefficients through every squaring.  The one-lane kernel is held to the same replay.  And the verdicts of a small simple_mul batch
with the engine forced, against the oracle."""
import json
import os
import random
import sys

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
IMPL_ONE_LANE, IMPL_SIX = 0, 5          # h2v_probe_pairing_ex: the kernel choices


@pytest.fixture(scope="module")
def simple_mul():
    from plutus_halo2_verifier_gen_amd import backend as be, plan as PL, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    return vk, td, pl, be.DevicePlan(pl.to_bytes(), 0)


@pytest.fixture(scope="module")
def pairs_and_replay(simple_mul):
    """14 pairs (one full wave of ten and a wave with six idle groups): accept <=> e(p1, [s]G2) == e(p2, G2).  Returns the compressed
    arguments, the verdicts as constructed, and the replay's final value per pair as 12 integers (re, im of coefficient 0..5)."""
    import gen_coop_program as gp
    vk, td, pl, dp = simple_mul
    rng = random.Random(315)
    q1 = bls.g2_mul(bls.G2_GEN, td.s)
    assert bls.g2_compress(q1) == bytes.fromhex(vk.s_g2)
    pts, want = [], []
    for k in range(11):
        A = bls.g1_mul(bls.G1_GEN, rng.randrange(1, bls.R))
        sA = bls.g1_mul(A, td.s)
        if k % 2:                                        # off by one generator: rejects
            sA = bls.g1_add(sA, bls.G1_GEN)
        pts.append((A, sA))
        want.append(0 if k % 2 else 1)
    pts += [(None, None), (bls.G1_GEN, None), (None, bls.G1_GEN)]      # each argument at infinity
    want += [1, 0, 0]
    assert len(pts) == 14
    prog = gp.build_program()
    replay = []
    for (a, b), w in zip(pts, want):
        f = gp.simulate(prog, a, q1, b, bls.G2_GEN)
        assert (f == bls.F12_ONE) == bool(w)
        replay.append([c for pair in f for c in pair])
    p1 = [bls.g1_compress(a) for a, _ in pts]
    p2 = [bls.g1_compress(b) for _, b in pts]
    return p1, p2, want, replay


@pytest.mark.parametrize("impl", [IMPL_SIX, IMPL_ONE_LANE])
def test_final_value_equals_the_big_integer_replay(simple_mul, pairs_and_replay, impl):
    from plutus_halo2_verifier_gen_amd import backend as be
    vk, td, pl, dp = simple_mul
    p1, p2, want, replay = pairs_and_replay
    acc, dump = be.probe_pairing_ex(dp, p1, p2, impl=impl)
    assert acc == want
    for i in range(len(p1)):
        assert dump[i][1] == replay[i], "final value of pair %d" % i
    # the rejecting pairs with both arguments finite exercise every lane: no coefficient of their final value is trivial
    for i in (1, 3, 5, 7, 9):
        assert all(c not in (0, 1) for c in replay[i])


def test_forced_six_lane_engine_verdicts_match_the_oracle(simple_mul, orc):
    from plutus_halo2_verifier_gen_amd import backend as be, synth
    vk, td, pl, dp = simple_mul
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    n, n_pi = 24, vk.n_public_inputs                    # three waves of the engine: ten, ten and four proofs
    good = synth.forge_batch(vk, td, n, seed=61, plan=pl, workers=1)
    rng = random.Random(62)
    proofs = [good.proof(i) for i in range(n)]
    insts = [good.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(n)]
    victims = sorted(rng.sample(range(n), 5))
    for i in victims:                                   # only the pairing sees a wrong pi
        proofs[i], insts[i] = synth.corrupt(pl, proofs[i], insts[i], "wrong_pi", rng)
        proofs[i], insts[i] = bytes(proofs[i]), bytes(insts[i])
    off = [0]
    for p_ in proofs:
        off.append(off[-1] + len(p_))
    pb, ib = b"".join(proofs), b"".join(insts)
    ws = be.Workspace(dp, n)
    ws.set_option(be.Workspace.OPT_PAIRING_ENGINE, 6)
    got = list(dp.verify_batch(pb, off, ib, good.committed, ws=ws))
    assert ws.timings().pairing_lanes_per_proof == 6
    ws.close()
    want = list(ov.verify_batch(pb, off, ib, good.committed, threads=4))
    assert got == want
    assert want == [0 if i in victims else 1 for i in range(n)]
