"""The layouts tests/test_pairing_engines_gpu.py runs cover every position of every pairing engine: with G proofs per wave (64 for
the one-lane kernel, 1 wide, 2 for the 32-lane engine, 4 narrow, 5 twelve-lane, 10 six-lane), batches of {1, G, G + 1, 2G + 1} pairs
under the six rotations bring each of the six kinds (tests/pairing_kinds.py) into group 0 of a wave, into group G - 1 - the one the
idle lanes 60..63 of the packed engines shadow - and into the lone live group of a trailing wave.  A condition on the table, checked
without a GPU; the kinds themselves and the probe's input encodings are checked here too."""
import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import pairing_kinds as K


def test_the_engine_table_is_the_launchers():
    assert [(e.name, e.lanes, e.per_wave) for e in K.ENGINES] == [("one_lane", 1, 64), ("coop32", 32, 2), ("narrow", 16, 4), ("wide", 64, 1),
                                                                   ("six", 6, 10), ("twelve", 12, 5)]
    assert sorted(e.impl for e in K.ENGINES) == [0, 1, 2, 3, 5, 6]
    # only the 32-lane engine needs the option: impl 1 alone is the launcher's rule, which takes the wide engine for a small batch
    assert [(e.impl, e.option) for e in K.ENGINES if e.option] == [(1, 32)]
    for e in K.ENGINES:
        assert e.lanes * e.per_wave <= 64 < e.lanes * (e.per_wave + 1), e.name


@pytest.mark.parametrize("engine", K.ENGINES, ids=lambda e: e.name)
def test_every_kind_visits_the_first_group_the_last_group_and_a_lone_trailing_group(engine):
    G = engine.per_wave
    sizes = K.batch_sizes(G)
    assert sizes == ((1, 2, 3) if G == 1 else (1, G, G + 1, 2 * G + 1))
    assert K.ROTATIONS == (0, 1, 2, 3, 4, 5)
    assert max(sizes) == (129 if engine.name == "one_lane" else 2 * G + 1) and (engine.name == "one_lane" or max(sizes) <= 21)
    assert K.positions_seen(G, sizes, K.ROTATIONS) == K.ALL_POSITIONS
    # the edge keys run the largest size alone: it covers the first and the last group and a lone trailing one by itself
    assert K.positions_seen(G, (2 * G + 1,), K.ROTATIONS) == K.ALL_POSITIONS


def test_the_coverage_condition_notices_a_layout_that_is_too_small():
    # no rotations: only six consecutive kinds from 0; a wave of ten never shows kind 5 in group 0 without them
    assert K.positions_seen(10, K.batch_sizes(10), (0,)) != K.ALL_POSITIONS
    # no trailing wave: nothing is ever alone
    assert not any(where == "lone" for _, where in K.positions_seen(10, (10, 20), K.ROTATIONS))
    # (a single pair IS a lone trailing group, and of a one-proof wave every group is first, last and alone)
    assert K.positions_seen(1, (1,), K.ROTATIONS) == K.ALL_POSITIONS


def test_order_is_the_rotation_the_six_lane_test_has_always_used():
    assert K.order(8, 0) == [0, 1, 2, 3, 4, 5, 0, 1] and K.order(3, 5) == [5, 0, 1]


def test_jacobian_limbs_are_montgomery_form_of_the_scaled_point():
    from plutus_halo2_verifier_gen_amd import backend as be
    RM = 1 << 392                                             # the kernels' Montgomery radix (csrc/h2v_field.hpp)
    assert bls.to_mont_fp(1) == RM % bls.P
    rinv = pow(RM, -1, bls.P)
    words = lambda raw: [int.from_bytes(raw[48 * i:48 * i + 48], "little") for i in range(3)]
    pt = bls.g1_mul(bls.G1_GEN, 11)
    for z in (1, 0x1234567 << 300 | 5, bls.P - 1):
        X, Y, Z = (w * rinv % bls.P for w in words(be.g1_jacobian_limbs(pt, z)))
        assert all(w < bls.P for w in words(be.g1_jacobian_limbs(pt, z)))
        assert Z == z % bls.P
        zi = pow(Z, -1, bls.P)
        assert (X * zi * zi % bls.P, Y * zi * zi * zi % bls.P) == pt
    # infinity as g1j_set_inf writes it: X = Y = 1 (Montgomery form: R mod p), Z = 0
    assert words(be.g1_jacobian_limbs(None)) == [RM % bls.P, RM % bls.P, 0]
    with pytest.raises(ValueError):
        be.g1_jacobian_limbs(pt, bls.P)


def test_the_off_curve_encoding_does_not_decode():
    enc = K.off_curve_encoding()
    assert len(enc) == 48 and enc[0] & 0xe0 == 0x80
    with pytest.raises(ValueError):
        bls.g1_decompress(enc, False)


@pytest.fixture(scope="module")
def edge_key_kinds():
    """the six kinds under the two edge keys: s_g2 = G2 and s_g2 = -G2"""
    from plutus_halo2_verifier_gen_amd import vk as V
    vk, td = V.simple_mul_vk()
    return {s: (V.on_srs(vk, td, s), K.build_kinds(*V.on_srs(vk, td, s))) for s in (1, bls.R - 1)}


def test_the_edge_keys_give_the_same_six_kinds(edge_key_kinds):
    from plutus_halo2_verifier_gen_amd import plan as PL
    for s, ((vk, td), kinds) in edge_key_kinds.items():
        assert td.s == s
        PL.compile_plan(vk)                                   # the plan compiler takes the key
        # (s = +-1: the accepting pair's two loops run the same lines at +-y, and the odd powers of w cancel in its Miller value)
        assert kinds[K.ACCEPT].final == K.ONE and kinds[K.ACCEPT].miller != K.ONE
        assert kinds[K.INF_BOTH].miller == K.ONE and kinds[K.INF_BOTH].final == K.ONE
        for k in (K.INF_1, K.INF_2):
            assert kinds[k].miller != K.ONE and kinds[k].final != K.ONE
    (vk1, _), k1 = edge_key_kinds[1]
    (vkm, _), km = edge_key_kinds[bls.R - 1]
    assert bytes.fromhex(vk1.s_g2) == bls.g2_compress(bls.G2_GEN) and bytes.fromhex(vkm.s_g2) == bls.g2_compress(bls.g2_neg(bls.G2_GEN))
    assert k1[K.ACCEPT].p1 == k1[K.ACCEPT].p2                 # s = 1: the accepting pair is (a, a)
    assert km[K.ACCEPT].p2 == bls.g1_neg(km[K.ACCEPT].p1)     # s = r - 1: (a, -a)
    assert km[K.REJECT_B].p1 == km[K.REJECT_B].p2             # ... and (c, [s + 2]c) is (c, c)
