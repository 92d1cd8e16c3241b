"""The table of G1 encodings (tests/g1_encodings.py) held to the oracle case by case, and the conditions it must keep covering -
so that the table the GPU tests run cannot thin out unnoticed.  CPU only."""
from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import g1_encodings as G

P, R = bls.P, bls.R


def test_model_equals_the_oracle_on_every_case(orc):
    for c in G.cases():
        ok, pt = orc.g1_decompress(c.enc)
        assert ok == c.in_g1, (c.name, c.enc.hex())
        if ok:
            assert pt == c.point, (c.name, c.enc.hex())
        # the table's own consistency: the verdicts nest, a stored point is on the curve, has the encoded x and the flagged root
        assert c.on_curve or not c.in_g1, c.name
        assert (c.point is not None) == (c.on_curve and c.kind != "infinity"), c.name
        if c.point is not None:
            x, y = c.point
            assert bls.g1_is_on_curve(c.point) and x == int.from_bytes(bytes([c.enc[0] & 0x1F]) + c.enc[1:], "big") and x < P
            assert (y > P - y) == G.sort_flag(c.enc), c.name


def test_verdict_of_every_kind():
    want = {"g1": (True, True), "infinity": (True, True), "bad_infinity": (False, False), "no_compression_bit": (False, False),
            "non_canonical": (False, False), "off_curve": (False, False), "outside_g1": (True, False)}
    assert set(want) == set(G.KINDS) == {c.kind for c in G.cases()}
    for c in G.cases():
        assert (c.on_curve, c.in_g1) == want[c.kind], c.name
    assert len({c.enc for c in G.cases()}) == len(G.cases())
    assert all(len(c.enc) == 48 for c in G.cases())


def test_valid_points_cover_both_roots(orc):
    by = G.by_kind()
    g1 = {c.name: c for c in by["g1"]}
    assert g1["generator"].point == bls.G1_GEN and g1["-generator"].point == bls.g1_neg(bls.G1_GEN)
    rand = [c for c in by["g1"] if c.name.startswith("random") and "flipped" not in c.name]
    assert len(rand) >= 20 and {G.sort_flag(c.enc) for c in rand} == {True, False}
    flipped = [c for c in by["g1"] if "flipped" in c.name]
    assert len(flipped) >= 4
    for c in flipped:
        twin = g1[c.name.split(",")[0]]
        assert c.enc[1:] == twin.enc[1:] and c.enc[0] == twin.enc[0] ^ 0x20
        assert c.point == bls.g1_neg(twin.point) and c.point != twin.point


def test_infinity_cases_touch_every_word():
    by = G.by_kind()
    assert [c.enc for c in by["infinity"]] == [bytes([0xC0]) + bytes(47)]
    bad = {c.enc for c in by["bad_infinity"]}
    assert bytes([0xE0]) + bytes(47) in bad
    words = {}
    for enc in bad - {bytes([0xE0]) + bytes(47)}:
        v = int.from_bytes(enc, "big") ^ (0xC0 << 376)
        assert v and v & (v - 1) == 0, enc.hex()             # exactly one stray bit
        words.setdefault((383 - (v.bit_length() - 1)) // 32, []).append(enc)
    assert sorted(words) == list(range(12)) and all(len(e) == 1 for e in words.values())
    assert 0 < words[0][0][0] & 0x1F                          # word 0's bit: beside the flags, in the low five bits of byte 0


def test_compression_bit_cases():
    encs = {c.enc for c in G.by_kind()["no_compression_bit"]}
    assert {bytes([b]) + bytes(47) for b in (0x00, 0x40, 0x20)} <= encs
    gen = bls.g1_compress(bls.G1_GEN)
    assert bytes([gen[0] & 0x7F]) + gen[1:] in encs
    assert all(not e[0] & 0x80 for e in encs)


def test_non_canonical_cases(orc):
    by = G.by_kind()
    g1 = {c.name: c for c in by["g1"]}
    plus_p = [c for c in by["non_canonical"] if c.name.startswith("low x")]
    assert len(plus_p) >= 4 and {G.sort_flag(c.enc) for c in plus_p} == {True, False}
    for c in plus_p:
        twin = g1[c.name[:-len(" + p")]]
        x0 = twin.point[0]
        assert x0 < (1 << 381) - P and c.enc == G.encode(x0 + P, G.sort_flag(twin.enc))
        assert orc.g1_decompress(twin.enc) == (True, twin.point) and orc.g1_decompress(c.enc) == (False, None)
    xs = {int.from_bytes(bytes([c.enc[0] & 0x1F]) + c.enc[1:], "big") for c in by["non_canonical"]}
    assert {P, P + 1, (1 << 381) - 1} <= xs and all(x >= P for x in xs)
    assert all(c.enc[0] & 0xC0 == 0x80 for c in by["non_canonical"])
    # x = p - 1: canonical, and off the curve for being off the curve
    assert G.encode(P - 1) in {c.enc for c in by["off_curve"]} and bls.fp_sqrt(((P - 1) ** 3 + 4) % P) is None


def test_curve_points_outside_g1_and_points_off_the_curve():
    by = G.by_kind()
    out = {c.name: c for c in by["outside_g1"]}
    assert out["(0, 2), order 3"].point == (0, 2) and out["(0, -2), order 3"].point == (0, P - 2)
    assert bls.g1_mul((0, 2), 3) is None
    for q in (11, 10177):
        pt = out["order %d" % q].point
        assert pt is not None and bls.g1_mul(pt, q) is None
    assert len([n for n in out if n.startswith("random curve point")]) >= 10
    tq = out["T + Q, T of order 3, Q in G1"].point
    q3 = bls.g1_mul(tq, 3)                                    # 3 (T + Q) = 3 Q is in G1, T + Q is not
    assert bls.g1_in_subgroup(q3) and q3 is not None and not bls.g1_in_subgroup(tq)
    assert {G.sort_flag(c.enc) for c in by["outside_g1"]} == {True, False}
    off = [c for c in by["off_curve"] if c.name.startswith("random")]
    assert len(off) >= 10 and {G.sort_flag(c.enc) for c in off} == {True, False}
    for c in by["off_curve"]:
        x = int.from_bytes(bytes([c.enc[0] & 0x1F]) + c.enc[1:], "big")
        assert x < P and pow((x * x * x + 4) % P, (P - 1) // 2, P) == P - 1, c.name


def test_the_two_cases_that_do_not_exist():
    assert P % 3 == 1
    assert pow(P - 4, (P - 1) // 3, P) != 1                   # c = 0 needs x^3 = -4
    assert pow((P - 15) * bls.fp_inv(4) % P, (P - 1) // 3, P) != 1   # y = (p +- 1) / 2 = +-1/2 needs x^3 = 1/4 - 4
    assert (2 * ((P + 1) // 2)) % P == 1 and (2 * ((P - 1) // 2)) % P == P - 1


def test_endomorphism_of_the_window_tables():
    """(beta x, y) = [lambda] (x, y) on every G1 case: what the GPU test holds the second window table to"""
    for c in G.by_kind()["g1"]:
        assert G.phi(c.point) == bls.g1_mul(c.point, bls.GLV_LAMBDA), c.name
