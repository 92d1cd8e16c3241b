"""Integer model of csrc/h2v_modinv.hpp (30 division steps per batch on the low words, transition matrix applied to (f, g)
and, modulo M with exact division by 2^30, to (d, e)) with the constants the device header carries, and the operand sets the
inverter tests share.  Every intermediate is asserted to stay inside the 64-bit / 32-bit ranges the kernel code assumes, the
loop to end within the kernel's batch limit and f to end as +-1.

`inverse` also says which way an operand leaves the inverter - its class: (sign of f at exit, number of +M repairs the `rep`
loop makes: 0, 1 or 2, whether the final conditional -M is taken, number of batches).  tools/gen_inverter_paths.py searches
operands by class into tests/golden/inverter_paths.json; tests/test_inverter_paths.py and tests/test_inverter_paths_gpu.py
read them.  Plain integers; nothing here touches a device."""
import collections
import json
import os
import random
import re

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "inverter_paths.json")
M30 = (1 << 30) - 1
BATCH_LIMIT = 48        # the kernel's loop bound

Field = collections.namedtuple("Field", "name mod mod30 minv30 limbs mont_bits")
_hdr = None


def _header():
    global _hdr
    if _hdr is None:
        with open(os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "bls_consts.h")) as f:
            _hdr = f.read()
    return _hdr


def arr(name):
    return [int(x.rstrip("u"), 16) for x in re.search(name + r"\[\d+\] = \{([^}]*)\}", _header()).group(1).split(", ")]


def const(name):
    return int(re.search(name + r" = (0x[0-9a-f]+)u", _header()).group(1), 16)


_fields = {}


def field(name):
    """"FP" / "FR": modulus, its 30-bit limbs and -M^-1 mod 2^30 as bls_consts.h has them, and the Montgomery exponent"""
    if name not in _fields:
        mod, bits = {"FP": (bls.P, bls.MONT_BITS_FP), "FR": (bls.R, bls.MONT_BITS_FR)}[name]
        _fields[name] = Field(name, mod, arr(name + "_MOD30"), const(name + "_MINV30"), len(arr(name + "_MOD30")), bits)
    return _fields[name]


def divsteps(zeta, f, g, zrange):
    u, v, q, r = 1, 0, 0, 1
    for _ in range(30):
        c1 = -1 if zeta < 0 else 0
        c2 = -(g & 1)
        x = ((f ^ (c1 & 0xFFFFFFFF)) - c1) & 0xFFFFFFFF
        y, z = (u ^ c1) - c1, (v ^ c1) - c1
        g = (g + (x & (c2 & 0xFFFFFFFF))) & 0xFFFFFFFF
        q += y & c2
        r += z & c2
        c1 &= c2
        zeta = (zeta ^ c1) - 1
        f = (f + (g & (c1 & 0xFFFFFFFF))) & 0xFFFFFFFF
        u += q & c1
        v += r & c1
        g >>= 1
        u <<= 1
        v <<= 1
        assert all(-(1 << 30) <= t <= (1 << 30) for t in (u, v, q, r))
        zrange[0], zrange[1] = min(zrange[0], zeta), max(zrange[1], zeta)
    return zeta, (u, v, q, r)


def inverse(x, fld):
    """(x^-1 mod M, class, (lowest, highest zeta)) of 0 < x < M; fld: "FP", "FR" or a Field"""
    if isinstance(fld, str):
        fld = field(fld)
    mod30, minv30, L = fld.mod30, fld.minv30, fld.limbs
    assert 0 < x < fld.mod
    f, g = list(mod30), [(x >> (30 * i)) & M30 for i in range(L)]
    d, e = [0] * L, [1] + [0] * (L - 1)
    zeta = -1
    zrange = [zeta, zeta]
    for n in range(BATCH_LIMIT):
        zeta, (u, v, q, r) = divsteps(zeta, (f[0] | (f[1] << 30)) & 0xFFFFFFFF, (g[0] | (g[1] << 30)) & 0xFFFFFFFF, zrange)
        sd, se = (-1 if d[-1] < 0 else 0), (-1 if e[-1] < 0 else 0)
        md, me = (u & sd) + (v & se), (q & sd) + (r & se)
        cd, ce = u * d[0] + v * e[0], q * d[0] + r * e[0]
        md -= (minv30 * (cd & 0xFFFFFFFF) + md) & M30
        me -= (minv30 * (ce & 0xFFFFFFFF) + me) & M30
        assert -(1 << 31) <= md < (1 << 31) and -(1 << 31) <= me < (1 << 31)
        cd += mod30[0] * md
        ce += mod30[0] * me
        assert cd & M30 == 0 and ce & M30 == 0
        cd >>= 30
        ce >>= 30
        cf, cg = u * f[0] + v * g[0], q * f[0] + r * g[0]
        assert cf & M30 == 0 and cg & M30 == 0
        cf >>= 30
        cg >>= 30
        for i in range(1, L):
            cd += u * d[i] + v * e[i] + mod30[i] * md
            ce += q * d[i] + r * e[i] + mod30[i] * me
            cf += u * f[i] + v * g[i]
            cg += q * f[i] + r * g[i]
            assert all(-(1 << 63) <= t < (1 << 63) for t in (cd, ce, cf, cg))
            d[i - 1], e[i - 1], f[i - 1], g[i - 1] = cd & M30, ce & M30, cf & M30, cg & M30
            cd >>= 30
            ce >>= 30
            cf >>= 30
            cg >>= 30
        assert all(-(1 << 31) <= t < (1 << 31) for t in (cd, ce, cf, cg))
        d[-1], e[-1], f[-1], g[-1] = cd, ce, cf, cg
        if not any(g):
            break
    else:
        raise AssertionError("no convergence within the kernel's batch limit")
    fv = sum(t << (30 * i) for i, t in enumerate(f))
    dv = sum(t << (30 * i) for i, t in enumerate(d))
    m = fld.mod
    assert sum(t << (30 * i) for i, t in enumerate(mod30)) == m
    assert fv in (1, -1) and -2 * m < dv < m
    # the tail as the kernel runs it: sign(f) * d, M added while negative (at most twice), M taken off once if it fits
    w, repairs = dv * fv, 0
    for _ in range(2):
        if w < 0:
            w, repairs = w + m, repairs + 1
    assert 0 <= w < 2 * m
    final = w >= m
    if final:
        w -= m
    assert w == dv * fv % m
    return w, (fv, repairs, final, n + 1), (zrange[0], zrange[1])


def label(cls):
    """a class as the fixture's key: "f=-1 repairs=2 final=0 batches=26\""""
    return "f=%+d repairs=%d final=%d batches=%d" % (cls[0], cls[1], int(cls[2]), cls[3])


def parse_label(text):
    m = re.fullmatch(r"f=([+-]1) repairs=([012]) final=([01]) batches=(\d+)", text)
    return int(m.group(1)), int(m.group(2)), bool(int(m.group(3))), int(m.group(4))


# what the class table of DESIGN.md 4.5 lists: every one of these has to be among a field's fixture classes
RARE = {
    "two repairs": lambda c: c[1] == 2,
    "final subtraction": lambda c: c[2],
    "f = -1, one repair": lambda c: c[0] == -1 and c[1] == 1,
    "f = +1, no repair": lambda c: c[0] == 1 and c[1] == 0,
}
RARE_BATCHES = {"FP": (25, 27), "FR": (17,)}     # beside the usual 26 and 18
COMMON_BATCHES = {"FP": 26, "FR": 18}


def load_fixture():
    """{"FP": [(operand, class), ...], "FR": [...]} from tests/golden/inverter_paths.json"""
    with open(FIXTURE) as f:
        doc = json.load(f)
    return {name: [(int(h, 16), parse_label(lab)) for lab, ops in sorted(doc[name]["classes"].items()) for h in ops]
            for name in ("FP", "FR")}


def structured(name, seed=21):
    """The chosen integers of one field, without duplicates and all in (0, M): powers of two and their neighbours from both
    ends, the modulus with its low bits cut off, the small and the near-modulus values, operands whose low 30 j bits are zero
    under a random high part, and operands below 2^(30 j)."""
    fld = field(name)
    m, bits = fld.mod, fld.mod.bit_length()
    rng = random.Random(seed)
    out = []
    for k in range(bits):
        out += [1 << k, (1 << k) + 1, (1 << k) - 1, m - (1 << k), m - (1 << k) + 1, m - (1 << k) - 1]
        out += [m >> k, (m >> k) << k]
    out += [1, 2, 3, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2]
    for j in range(1, fld.limbs):
        low = 30 * j
        if low < bits - 1:
            out += [(rng.randrange(1, (m >> low)) << low) for _ in range(3)]
            out += [((m >> low) - 1) << low, 1 << low]
        top = min(1 << low, m)
        out += [rng.randrange(1, top) for _ in range(3)] + [top - 1]
    seen, uniq = set(), []
    for x in out:
        if 0 < x < m and x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq


def to_probe(x, fld):
    """the canonical value a field probe has to be given so that the inverter (which sees the Montgomery residue) works on x"""
    if isinstance(fld, str):
        fld = field(fld)
    return x * pow(1 << fld.mont_bits, -1, fld.mod) % fld.mod


LANE_SIZES = (64, 65, 128)      # the probe launches blocks of 64: one full wave, a ragged second block of one lane, two waves
LANE_SPOTS = (0, 31, 63)


def _cycle(pool, n, start=0):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def lane_arrangements(name, fixture=None):
    """(what, operands) lists for the per-lane exit of the batch loop and of the tail, from the fixture's operands of one field
    (0 stands for the zero operand, which the callers of the inverter answer with 0 without entering it):
      one long-running operand (27 batches for FP, 18 for FR) among short ones (26 / 17) in lane 0, 31, 63 of every wave;
      the converse; a zero next to a long-running one among short ones, and a long-running one alone among zeros;
      the two-repair and final-subtraction operands in lane 0, lane 63 and the last lane of the batch among common ones."""
    ops = (fixture or load_fixture())[name]
    long_b = COMMON_BATCHES[name] + (1 if name == "FP" else 0)
    short_b = long_b - 1
    longs, shorts = [x for x, c in ops if c[3] == long_b], [x for x, c in ops if c[3] == short_b]
    rare = {what: [x for x, c in ops if RARE[what](c)] for what in ("two repairs", "final subtraction")}
    common = [x for x, c in ops if c[3] == COMMON_BATCHES[name] and not c[2] and c[1] < 2]
    out, turn = [], 0
    for n in LANE_SIZES:
        waves = range(0, n - 63, 64)      # first lane of every full wave
        for spot in LANE_SPOTS:
            for what, few, many in (("one long among short", longs, shorts), ("one short among long", shorts, longs)):
                xs = _cycle(many, n, turn)
                for w in waves:
                    xs[w + (spot if w == 0 else 63 - spot)] = few[turn % len(few)]
                    turn += 1
                out.append(("%s, n=%d, lane %d" % (what, n, spot), xs))
            xs, alone = _cycle(shorts, n, turn), [0] * n
            for w in waves:
                at = w + spot
                xs[at], xs[at + 1 if spot < 63 else at - 1] = 0, longs[turn % len(longs)]
                alone[at] = longs[(turn + 1) % len(longs)]
                turn += 2
            out.append(("zero beside a long one, n=%d, lane %d" % (n, spot), xs))
            out.append(("one long among zeros, n=%d, lane %d" % (n, spot), alone))
        for what, pool in rare.items():
            xs = _cycle(common, n, turn)
            for k, at in enumerate(sorted({0, 63, n - 1})):
                xs[at] = pool[(turn + k) % len(pool)]
            turn += 3
            out.append(("%s in lanes 0, 63 and %d, n=%d" % (what, n - 1, n), xs))
    return out
