"""The division-step inverter (csrc/h2v_modinv.hpp) on operands chosen by the way they leave it, CPU side.

tests/golden/inverter_paths.json (tools/gen_inverter_paths.py) holds, per field, operands of every class - (sign of f at exit,
+M repairs, final -M, batches) - a seeded search of 25 000 uniform operands met; tests/safegcd_model.structured adds the
chosen integers: powers of two and their neighbours from both ends, the truncated modulus, low limbs zero, high limbs zero.
Here the integer model runs all of them with its range assertions, the labels and the coverage of the class table are checked,
and the header itself - compiled as a host program with ASan + UBSan - inverts all of them and 50 000 random operands per field
against h2v_hostmath.hpp.  The same operands on the device: tests/test_inverter_paths_gpu.py."""
import json
import os
import subprocess

import pytest

from tests import safegcd_model as S

ROOT = S.ROOT
FIELDS = ("FP", "FR")
N_RANDOM = 50000


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


@pytest.fixture(scope="module")
def modelled(fixture):
    """name -> {operand: (inverse, class, zeta range)} of every fixture and structured operand, worked out once"""
    return {name: {x: S.inverse(x, name) for x in [x for x, _ in fixture[name]] + S.structured(name)} for name in FIELDS}


@pytest.mark.parametrize("name", FIELDS)
def test_model_inverts_every_operand_inside_its_ranges(modelled, name):
    """every fixture and structured operand: all range assertions of the model hold (matrix entries within +-2^30, md / me and
    the top limbs in 32 bits, the carries in 64, exact divisions, f = +-1, d in (-2M, M)) and the result is the inverse.  The
    structured operands do reach what random ones do not: whole batches of halvings, where a matrix entry is 2^30 and zeta
    falls far below the -30 of random operands (to minus the bit length for 2^(bits - 1)).  Batch counts stay far inside the
    kernel's limit of 48"""
    mod = S.field(name).mod
    for x, (inv, cls, _z) in modelled[name].items():
        assert inv == pow(x, mod - 2, mod), hex(x)
        assert cls[3] <= 32, hex(x)
    assert min(z[0] for _i, _c, z in modelled[name].values()) <= -(mod.bit_length() - 1)


@pytest.mark.parametrize("name", FIELDS)
def test_structured_operands_hold_what_they_promise(name):
    fld = S.field(name)
    m, bits = fld.mod, fld.mod.bit_length()
    xs = S.structured(name)
    have = set(xs)
    assert len(have) == len(xs) and all(0 < x < m for x in xs)
    for k in range(bits):
        p2 = 1 << k
        assert all(v in have for v in (p2, p2 + 1, p2 - 1, m - p2, m - p2 + 1, m - p2 - 1, m >> k, (m >> k) << k) if 0 < v < m)
    assert {1, 2, 3, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2} <= have
    for j in range(1, fld.limbs):
        low = 30 * j
        if low < bits - 1:       # low 30 j bits zero under a high part that is no power of two
            assert sum(1 for x in xs if x % (1 << low) == 0 and x & (x - 1)) >= 3
        assert sum(1 for x in xs if x < (1 << low) and x >= (1 << (low - 30)) and x & (x + 1) and x & (x - 1)) >= 3


@pytest.mark.parametrize("name", FIELDS)
def test_fixture_operands_take_the_class_of_their_label(fixture, modelled, name):
    assert len({x for x, _ in fixture[name]}) == len(fixture[name])
    for x, cls in fixture[name]:
        assert modelled[name][x][1] == cls, (hex(x), S.label(cls))


@pytest.mark.parametrize("name", FIELDS)
def test_fixture_covers_the_class_table(fixture, name):
    """a condition, not a measurement: at least 8 operands with two +M repairs, with the final -M, with f = -1 and one repair,
    with f = +1 and none, and of every batch count beside the usual one - except FP in 25 batches, of which the search of
    25 000 met three, all stored.  Every class holds 8 operands or all that were met."""
    with open(S.FIXTURE) as f:
        doc = json.load(f)[name]
    assert set(doc["classes"]) == set(doc["counts"]) and doc["draws"] >= 25000 == sum(doc["counts"].values())
    for lab, ops in doc["classes"].items():
        assert len(ops) == min(8, doc["counts"][lab]), lab
    classes = [c for _x, c in fixture[name]]
    for what, pick in S.RARE.items():
        assert sum(1 for c in classes if pick(c)) >= 8, what
    for b in S.RARE_BATCHES[name] + (S.COMMON_BATCHES[name],):
        n = sum(1 for c in classes if c[3] == b)
        assert n >= 8 or (name, b, n) == ("FP", 25, 3), (b, n)


@pytest.mark.parametrize("name", FIELDS)
def test_lane_arrangements_are_what_they_say(fixture, modelled, name):
    """the batches tests/test_inverter_paths_gpu.py launches, by the model's classes: exactly one lane of every full wave runs
    one batch longer (shorter) than all others; a zero sits beside a long-running lane; the rare tails sit in lane 0, lane 63
    and the last lane"""
    batches = lambda x: modelled[name][x][1][3]   # noqa: E731
    long_b = max(S.COMMON_BATCHES[name], *S.RARE_BATCHES[name])
    arr = S.lane_arrangements(name, fixture)
    assert {len(xs) for _w, xs in arr} == set(S.LANE_SIZES)
    seen = set()
    for what, xs in arr:
        n = len(xs)
        kind = what.split(",")[0]
        seen.add((kind, n))
        waves = [xs[w:w + 64] for w in range(0, n - 63, 64)]
        if kind in ("one long among short", "one short among long"):
            odd, rest = (long_b, long_b - 1) if kind.startswith("one long") else (long_b - 1, long_b)
            assert all(sorted(batches(x) for x in w) == sorted([odd] + [rest] * 63) for w in waves), what
            assert all(batches(x) == rest for x in xs[64 * len(waves):])
            spot = int(what.rsplit(" ", 1)[1])
            assert batches(xs[spot]) == odd and (n < 128 or batches(xs[64 + 63 - spot]) == odd)
        elif kind == "zero beside a long one":
            for w in waves:
                z = w.index(0)
                assert w.count(0) == 1 and long_b in [batches(w[k]) for k in (z - 1, z + 1) if 0 <= k < 64], what
        elif kind == "one long among zeros":
            assert all(w.count(0) == 63 and batches(max(w)) == long_b for w in waves), what
        else:
            pick = S.RARE[kind.split(" in lanes")[0]]
            assert [i for i, x in enumerate(xs) if pick(modelled[name][x][1])] == sorted({0, 63, n - 1}), what
    assert len(seen) == 6 * len(S.LANE_SIZES)


def test_probe_mapping_reaches_the_intended_integer():
    for name in FIELDS:
        fld = S.field(name)
        for x in (1, 2, fld.mod - 1, 1 << 90):
            assert S.to_probe(x, name) * (1 << fld.mont_bits) % fld.mod == x


def test_header_as_a_host_program_under_sanitizers(tmp_path, fixture):
    """tests/cpp/h2v_modinv_host.cpp: host code only, its own main, csrc/h2v_modinv.hpp itself with the device qualifiers defined
    away, built with ASan + UBSan and run as a program on every fixture and structured operand plus 50 000 random ones per field;
    each result checked inside the program by h2v_hostmath.hpp's Montgomery product"""
    out = str(tmp_path / "h2v_modinv_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_modinv_host.cpp"), "-o", out])
    sent = {name: [x for x, _ in fixture[name]] + S.structured(name) for name in FIELDS}
    text = "".join("%s %x\n" % (name, x) for name in FIELDS for x in sent[name])
    r = subprocess.run([out, str(N_RANDOM)], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines() == ["%s stdin %d random %d ok %d" % (name, len(sent[name]), N_RANDOM, len(sent[name]) + N_RANDOM)
                                     for name in FIELDS]
