"""Every pairing engine against the big-integer replay (tools/gen_coop_program.py: simulate), value by value, in every position of a
wave and from every entry state a pipeline can hand it.  The six engines: k_pairing_check (one lane per proof), k_pairing_coop (32
lanes, reachable from the probe only as impl 1 with H2V_OPT_PAIRING_ENGINE = 32), k_pairing_coop_narrow, k_pairing_coop_wide,
k_pairing_six and k_pairing_coop_twelve.  h2v_probe_pairing_states presets every output to 0xA5 and brings back 64 proofs' worth
of guard records behind the batch: what a dead group of the last wave writes shows there.

 a  values in every position: the six kinds (tests/pairing_kinds.py) rotated through batches of {1, G, G + 1, 2G + 1} pairs, G the
    engine's proofs per wave - verdicts, status words, Miller and final value of every pair, the engine that ran, the guard;
 b  the same at 2G + 1 under s_g2 = G2 (identical line tables, accepting pair (a, a)) and s_g2 = -G2;
 c  entry states: proofs that arrive rejected, a failed subgroup verdict, an undecodable argument - next to live neighbours;
 d  the first argument in Jacobian form (el_jac: recursion, the fold-pairs batch form) with Z = 1, a random Z, Z = p - 1, infinity.

Every comparison is exact.  The conditional launch (k_pairing_coop behind skip flags) needs the batch check's flags buffer and is
not reached from here; test_the_fall_back_localises holds its verdicts."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import pairing_kinds as K

pytestmark = pytest.mark.gpu
EDGE_SECRETS = {"s_g2_is_g2": 1, "s_g2_is_minus_g2": bls.R - 1}


@pytest.fixture(scope="module")
def keys():
    """{name: (device plan, {kind: Kind})} for simple_mul's key and the two edge keys; the replays run once per key"""
    from plutus_halo2_verifier_gen_amd import backend as be, plan as PL, vk as V
    vk, td = V.simple_mul_vk()
    named = {"simple_mul": (vk, td)}
    for name, s in EDGE_SECRETS.items():
        named[name] = V.on_srs(vk, td, s)
    return {name: (be.DevicePlan(PL.compile_plan(v).to_bytes(), 0), K.build_kinds(v, t)) for name, (v, t) in named.items()}


def run(dp, engine, p1, p2, **states):
    from plutus_halo2_verifier_gen_amd import backend as be
    if engine.option:
        be.probe_set_option(be.OPT_PAIRING_ENGINE, engine.option)
    try:
        return be.probe_pairing_states(dp, p1, p2, impl=engine.impl, **states)
    finally:
        if engine.option:
            be.probe_set_option(be.OPT_PAIRING_ENGINE, 0)


def check_pair(r, j, want, where):
    """proof j of the result against a Kind: verdict, status word, all 24 coefficients"""
    from plutus_halo2_verifier_gen_amd import backend as be
    assert r.accept[j] == want.verdict, "verdict: " + where
    assert r.status[j] == (0 if want.verdict else be.ST_PAIRING), "status: " + where
    assert r.values[j] is not None, "no value was written: " + where
    for q in range(12):
        assert r.values[j][0][q] == want.miller[q], "Miller value, coefficient %d: %s" % (q, where)
        assert r.values[j][1][q] == want.final[q], "final value, coefficient %d: %s" % (q, where)


def check_positions(dp, kinds, engine, n):
    for rot in K.ROTATIONS:
        order = K.order(n, rot)
        r = run(dp, engine, [kinds[k].c1 for k in order], [kinds[k].c2 for k in order])
        assert r.lanes == engine.lanes, "the engine that ran: batch %d rotation %d" % (n, rot)
        assert r.accept == [kinds[k].verdict for k in order], "verdicts, batch %d rotation %d" % (n, rot)
        for j, k in enumerate(order):
            check_pair(r, j, kinds[k], "batch %d rotation %d pair %d kind %d" % (n, rot, j, k))
        assert r.guard_clean, "something was written behind the last proof: batch %d rotation %d" % (n, rot)


POSITION_CASES = [pytest.param(e, n, id="%s-%d" % (e.name, n)) for e in K.ENGINES for n in K.batch_sizes(e.per_wave)]


@pytest.mark.parametrize("engine,n", POSITION_CASES)
def test_values_and_verdicts_in_every_position(keys, engine, n):
    dp, kinds = keys["simple_mul"]
    check_positions(dp, kinds, engine, n)


@pytest.mark.parametrize("key", sorted(EDGE_SECRETS))
@pytest.mark.parametrize("engine", K.ENGINES, ids=lambda e: e.name)
def test_values_and_verdicts_under_the_edge_keys(keys, engine, key):
    dp, kinds = keys[key]
    check_positions(dp, kinds, engine, 2 * engine.per_wave + 1)


@pytest.mark.parametrize("engine", K.ENGINES, ids=lambda e: e.name)
def test_entry_states(keys, engine):
    """Two proofs arrive rejected (first and last group of the first wave), one has a failed subgroup verdict on slot 1, one an
    argument that does not decode; everything around them keeps its values.  The dump of a proof rejected on entry is not
    asserted: the one-lane kernel writes none, the others run the program on infinity."""
    from plutus_halo2_verifier_gen_amd import backend as be
    dp, kinds = keys["simple_mul"]
    G = engine.per_wave
    n = 2 * G + 1
    order = [(K.ACCEPT, K.REJECT_A, K.REJECT_B)[j % 3] for j in range(n)]
    arrived = sorted({0, G - 1})
    bad_sub, bad_enc = (1, 2) if G == 1 else (G, G + 1)
    assert len({bad_sub, bad_enc} | set(arrived)) == 2 + len(arrived) and max(bad_sub, bad_enc) < n
    p1 = [kinds[k].c1 for k in order]
    p2 = [kinds[k].c2 for k in order]
    p1[bad_enc] = K.off_curve_encoding()
    status_in = [be.ST_BAD_SCALAR if j in arrived else 0 for j in range(n)]
    valid_sub = [(1, 0) if j == bad_sub else (1, 1) for j in range(n)]
    r = run(dp, engine, p1, p2, status_in=status_in, valid_sub_in=valid_sub)
    assert r.lanes == engine.lanes
    for j, k in enumerate(order):
        where = "pair %d kind %d" % (j, k)
        if j in arrived:
            assert (r.status[j], r.accept[j]) == (be.ST_BAD_SCALAR, 0), where
        elif j in (bad_sub, bad_enc):
            assert (r.status[j], r.accept[j]) == (be.ST_BAD_POINT, 0), where
        else:
            check_pair(r, j, kinds[k], where)
    assert r.guard_clean


@pytest.mark.parametrize("engine", K.ENGINES, ids=lambda e: e.name)
def test_first_argument_in_jacobian_form(keys, engine):
    """el_jac given: slot p1 holds ANOTHER valid point, so an engine that took the slot shows in values and verdicts.  The kinds'
    own first arguments go in as (x Z^2, y Z^3, Z); the kinds at infinity as g1j_set_inf's encoding.  Each Z with an accepting and a
    rejecting pair in group 0 and in group G - 1; a proof that arrives rejected stays so whatever el_jac holds."""
    from plutus_halo2_verifier_gen_amd import backend as be
    dp, kinds = keys["simple_mul"]
    G = engine.per_wave
    n = 2 * G + 1
    decoy = bls.g1_compress(bls.g1_mul(bls.G1_GEN, 0xdec0))
    assert all(kinds[k].p1 != bls.g1_mul(bls.G1_GEN, 0xdec0) for k in kinds)
    rng = random.Random(36)
    zs = {"one": 1, "random": rng.randrange(2, bls.P - 1), "p_minus_1": bls.P - 1}
    launches = [(name, z, first, last) for name, z in zs.items() for first, last in ((K.ACCEPT, K.REJECT_A), (K.REJECT_B, K.ACCEPT))]
    launches.append(("infinity", 1, K.INF_1, K.INF_BOTH))
    arrived = G                                            # group 0 of the second wave
    for name, z, first, last in launches:
        order = K.order(n, 0)
        order[G - 1] = last
        order[0] = first
        if G == 1:                                         # group 0 is group G - 1: the second wave's takes the other kind
            order[2] = last
        el = [be.g1_jacobian_limbs(kinds[k].p1, z) for k in order]
        status_in = [be.ST_BAD_SCALAR if j == arrived else 0 for j in range(n)]
        r = run(dp, engine, [decoy] * n, [kinds[k].c2 for k in order], status_in=status_in, el_jac_in=el)
        assert r.lanes == engine.lanes
        for j, k in enumerate(order):
            where = "Z %s pair %d kind %d" % (name, j, k)
            if j == arrived:
                assert (r.status[j], r.accept[j]) == (be.ST_BAD_SCALAR, 0), where
            else:
                check_pair(r, j, kinds[k], where)
        assert r.guard_clean, "Z %s" % name
