"""Limb model of ONE call of the cooperative Fp12 engine (csrc/h2v_pairing_coop.hpp) in each of its shapes:
  normal  two lanes per coefficient   (nq = 2)          wide    four lanes per coefficient (nq = 4)
  narrow  one lane per coefficient    (nq = 1, `both`)  twelve  the narrow engine packed, five proofs per wave
The slot map and the term tables are those of tools/gen_coop_tables.py (which checks them mod p only); the bias tables and the
constants +-2/3 are read from csrc/bls_consts.h; the fold is tools/gen_six_tables.py's.  Staging goes limb by limb as the device
does it and asserts that no limb goes negative; an engine call is then stated on the integers the 14-dword vectors spell (the top
limb holds everything from bit 364 up):

    lane q of a coefficient takes the terms t = q, q + nq, ... of its table row, T_q = sum x y, and leaves
        (w T_q + m p) / 2^392,   m = -w T_q / p mod 2^392        (w = 3: cyclotomic squaring with nq >= 2; else 1)
    which is exactly what the operand-scanning reduction leaves (replay() runs that reduction column by column and is held to the
    formula); the call returns the SUM over q, carried.  The reduction is per lane, so the integer differs between the shapes -
    only the residue is shared.

Column fill (the largest value a 64-bit column of a lane can take - products, tripling and the reduction's worst case - over 2^64)
with every slot at the limb maxima of its stated (v, lam) - see SLOT_BOUNDS; tests/test_coop_engine_model.py recomputes the table and holds it to these
figures.  Value bounds: VALUE_BOUND, in p / 1000, from the slots' value bounds (lane: w sum(v_x v_y) p^2 / R + p)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_coop_tables as ct  # noqa: E402
from gen_six_tables import bias_13_2, fold, limbs_val  # noqa: E402
from plutus_halo2_verifier_gen_amd import bls12_381 as bls  # noqa: E402

P = bls.P
R = 1 << 392
MASK = (1 << 28) - 1
PINV = pow(P, -1, R)
RINV = pow(R, -1, P)
MONT1 = R % P
N0 = (-pow(P, -1, 1 << 28)) % (1 << 28)
SHAPES = {"normal": 2, "wide": 4, "narrow": 1, "twelve": 1}        # shape -> lanes per coefficient (nq)
GROUPS_PER_WAVE = {"normal": 2, "wide": 1, "narrow": 4, "twelve": 5}
MT, ST, CT = ct.mul_table(), ct.sqr_table(), ct.csqr_table()
LT = {1: ct.line_table(1), 2: ct.line_table(2)}
V_OPERAND, V_CONJ = 6, 5               # what every staged operand may reach; CONJ and INV (F28_NEG(.., 6, 1))

# column fill per (op, shape): column_fill()'s figure, rounded up (test_column_headroom recomputes and compares)
COLUMN_FILL = {
    ("MUL", "narrow"): 0.643, ("MUL", "normal"): 0.338, ("MUL", "wide"): 0.186,
    ("SQR", "narrow"): 0.643, ("SQR", "normal"): 0.389, ("SQR", "wide"): 0.237,
    ("CSQR", "narrow"): 0.288, ("CSQR", "normal"): 0.643, ("CSQR", "wide"): 0.338,
    ("LINE", "narrow"): 0.338, ("LINE", "normal"): 0.186, ("LINE", "wide"): 0.135,
    ("PROD", "twelve"): 0.084,
}
# (the twelve shape runs the narrow engine: its fills and bounds are the narrow ones, and PROD is its own)
# value bound of a call's result per (op, shape) in units of p: what value_bound() yields from the slots' value bounds, rounded up
# to three places (test_value_bounds recomputes), and STATED_BOUND: what the header of h2v_pairing_coop.hpp states for the shape
VALUE_BOUND = {
    ("MUL", "narrow"): 1.367, ("MUL", "normal"): 2.367, ("MUL", "wide"): 4.367,
    ("SQR", "narrow"): 1.356, ("SQR", "normal"): 2.356, ("SQR", "wide"): 4.356,
    ("CSQR", "narrow"): 2.001, ("CSQR", "normal"): 2.510, ("CSQR", "wide"): 4.510,
    ("LINE", "narrow"): 1.021, ("LINE", "normal"): 2.021, ("LINE", "wide"): 4.021,
    ("PROD", "twelve"): 1.001,
}
STATED_BOUND = {
    ("MUL", "narrow"): 1.43, ("SQR", "narrow"): 1.56, ("CSQR", "narrow"): 2.001, ("LINE", "narrow"): 1.03, ("PROD", "twelve"): 2.0,
    "normal": 3.0, "wide": 4.8,
}


def stated_bound(op, shape):
    """the header's bound for a call's result, as an integer"""
    shape = "narrow" if shape == "twelve" and op != "PROD" else shape
    b = STATED_BOUND.get((op, shape), STATED_BOUND.get(shape))
    return int(b * 1000) * P // 1000


def _consts():
    text = open(os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "bls_consts.h")).read()
    arr = lambda body: [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
    bias = {(int(k), int(m)): arr(body) for k, m, body in re.findall(r"F28_BIAS_(\d+)_(\d+)\[14\] = \{([^}]*)\}", text)}
    named = {n: arr(body) for n, body in re.findall(r"(FP_C23P28|FP_C23N28|FP_MOD28|FP_ONE28)\[14\] = \{([^}]*)\}", text)}
    return bias, named


BIAS, _NAMED = _consts()
C23P_L, C23N_L, P_L = _NAMED["FP_C23P28"], _NAMED["FP_C23N28"], _NAMED["FP_MOD28"]
assert limbs_val(P_L) == P and limbs_val(_NAMED["FP_ONE28"]) == MONT1
assert limbs_val(C23P_L) == ct.C23 * R % P and limbs_val(C23N_L) == (P - ct.C23) * R % P
assert BIAS[(13, 2)] == bias_13_2()
for (_k, _m), _b in BIAS.items():
    assert limbs_val(_b) == _k * P


# ------------------------------------------------------------------------------------------------ limb vectors
def limbs(v):
    """the carried limb vector of v: 13 limbs of 28 bits, the top limb holds the rest (one dword)"""
    assert 0 <= v and (v >> 364) < (1 << 32)
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]


def is_carried(l):
    return all(0 <= x <= MASK for x in l[:13]) and 0 <= l[13] < (1 << 32)


def neg(b, K, M):
    """F28_NEG: K p - b limb by limb against bls_consts.h's bias; no limb may go negative"""
    out = [x - y for x, y in zip(BIAS[(K, M)], b)]
    assert all(0 <= x < (1 << 32) for x in out), "F28_NEG(%d, %d): a limb left its dword" % (K, M)
    return out


def add(a, b):
    out = [x + y for x, y in zip(a, b)]
    assert all(x < (1 << 32) for x in out)
    return out


def scale(a, k):
    out = [k * x for x in a]
    assert all(x < (1 << 32) for x in out)
    return out


def carry(l):
    """f28_carry"""
    out, c = [], 0
    for i in range(13):
        t = l[i] + c
        assert t < (1 << 32)
        out.append(t & MASK)
        c = t >> 28
    assert l[13] + c < (1 << 32)
    return out + [l[13] + c]


def limbs_all_max(bound):
    """the largest value below `bound` whose thirteen lower limbs are all 2^28 - 1"""
    low = (1 << 364) - 1
    v = (((bound - 1 - low) >> 364) << 364) | low
    assert low <= v < bound
    return v


# ------------------------------------------------------------------------------------------------ staging (slot -> limb vector)
def new_slots():
    return {ct.SLOT_ZERO: [0] * 14, ct.SLOT_C23P: list(C23P_L), ct.SLOT_C23N: list(C23N_L)}


def stage_a(s, a):
    """coop_stage_a: A = a, NA = 7p - a_im carried"""
    for g in range(12):
        s[ct.SLOT_A + g] = list(a[g])
        if g & 1:
            s[ct.SLOT_NA + (g >> 1)] = carry(neg(a[g], 7, 1))


def xi_of(own, partner, g, K, M):
    """(xi z)_part for z = (re, im): re - im + K p on the real lane, re + im on the imaginary one, carried"""
    return carry(add(own, partner if g & 1 else neg(partner, K, M)))


def stage_b(s, b):
    for g in range(12):
        s[ct.SLOT_B + g] = list(b[g])
        s[ct.SLOT_XB + g] = xi_of(b[g], b[g ^ 1], g, 7, 1)


def stage_sqr(s, a):
    stage_a(s, a)
    for g in range(12):
        d2, pd2 = scale(a[g], 2), scale(a[g ^ 1], 2)          # D = 2a, UNCARRIED
        s[ct.SLOT_D + g] = d2
        s[ct.SLOT_XD + g] = xi_of(d2, pd2, g, 13, 2)
        if g >= 6:
            s[ct.SLOT_XA + (g - 6)] = xi_of(a[g], a[g ^ 1], g, 7, 1)


def stage_csqr(s, a):
    """coop_csqr_stage, both roles: A, NA, ND2 = 2 NA_2 uncarried; D = 2a uncarried, S = re + im, M = re + 7p - im"""
    for g in range(12):
        n = neg(a[g], 7, 1)
        s[ct.SLOT_A + g] = list(a[g])
        if g & 1:
            s[ct.SLOT_NA + (g >> 1)] = carry(n)
            if g == 5:
                s[ct.SLOT_ND2] = scale(carry(n), 2)
        s[ct.SLOT_D + g] = scale(a[g], 2)
        s[ct.SLOT_SM + g] = carry(add(a[g ^ 1], n if g & 1 else a[g]))


# (v, lam) of every staged slot kind, as the header of h2v_pairing_coop.hpp states them
SLOT_BOUNDS = {
    "MUL": {ct.SLOT_A: (12, 6, 1), ct.SLOT_NA: (6, 7, 1), ct.SLOT_B: (12, 6, 1), ct.SLOT_XB: (12, 13, 1)},
    "SQR": {ct.SLOT_A: (12, 6, 1), ct.SLOT_NA: (6, 7, 1), ct.SLOT_D: (12, 12, 2), ct.SLOT_XD: (12, 25, 1), ct.SLOT_XA: (6, 13, 1)},
    "CSQR": {ct.SLOT_A: (12, 6, 1), ct.SLOT_NA: (6, 7, 1), ct.SLOT_D: (12, 12, 2), ct.SLOT_SM: (12, 13, 1), ct.SLOT_C23P: (2, 1, 1)},
    "LINE": {ct.SLOT_A: (12, 6, 1), ct.SLOT_NA: (6, 7, 1), ct.SLOT_T1: (8, 2, 1), ct.SLOT_PX1: (4, 1, 1), ct.SLOT_LN1: (16, 1, 1)},
}
ND2_BOUND = (14, 2)      # overwrites slot XA + 0 in the cyclotomic squaring's staging


def bound_slots(op):
    """slot -> (v, lam) for every slot an op's table reads"""
    out = {ct.SLOT_ZERO: (0, 0)}
    for base, (count, v, lam) in SLOT_BOUNDS[op].items():
        for j in range(count):
            out[base + j] = (v, lam)
    if op == "CSQR":
        out[ct.SLOT_ND2] = ND2_BOUND
    return out


def max_vector(v, lam):
    """every limb at the maximum (v, lam) allows: lower limbs lam (2^28 - 1), the top limb that of v p - 1"""
    return [lam * MASK] * 13 + [(v * P - 1) >> 364] if v else [0] * 14


def within(l, v, lam):
    """the limb vector respects (v, lam): value at most v p (7p - 0 is 7p itself), lower limbs at most lam (2^28 - 1)"""
    if v == 0:
        return not any(l)
    return all(0 <= x <= lam * MASK for x in l[:13]) and limbs_val(l) <= v * P


# ------------------------------------------------------------------------------------------------ the engine
def lane_value(terms, s, w):
    T = sum(limbs_val(s[x]) * limbs_val(s[y]) for x, y in terms)
    m = (-w * T * PINV) % R
    v = w * T + m * P
    assert v % R == 0
    v >>= 392
    assert (v >> 364) < (1 << 32)
    return v


def lane_terms(row, q, nq, triple):
    nte = len(row) - 1 if (nq == 1 and triple) else len(row)        # one lane per coefficient: the constant term is left out
    return [row[t] for t in range(q, nte, nq)]


def engine(row, s, nq, triple=False):
    """the call's result for one coefficient: the sum of its lanes' reduced parts (an integer; the device returns limbs(.))"""
    w = 3 if triple and nq >= 2 else 1
    total = sum(lane_value(lane_terms(row, q, nq, triple), s, w) for q in range(nq))
    assert (total >> 364) < (1 << 32)
    return total


# what the reduction and the carries add to a column at most, whatever the data: 14 products m p_j with m below 2^28, the carry
# of the column below and the extraction's running carry (each below 2^36)
RED_MAX = MASK * sum(P_L) + (1 << 37)


def replay(terms, s, w):
    """coop_accumulate for one lane, column by column on true integers: products, tripling, the 14 reduction steps, extraction.
    Returns (result limbs, largest column value met)."""
    acc = [0] * 28
    for x, y in terms:
        for i in range(14):
            for j in range(14):
                acc[i + j] += s[x][i] * s[y][j]
    acc = [w * c for c in acc]
    top = max(acc)
    for k in range(14):
        m = ((acc[k] & 0xffffffff) * N0) & MASK
        for j in range(14):
            acc[k + j] += m * P_L[j]
        assert acc[k] & MASK == 0
        acc[k + 1] += acc[k] >> 28
        top = max(top, max(acc[k:min(k + 15, 28)]))
    out, c = [], 0
    for k in range(13):
        c += acc[14 + k]
        top = max(top, c)
        out.append(c & MASK)
        c >>= 28
    out.append(c + acc[27])
    return out, top



def product_columns_top(terms, s, w):
    acc = [0] * 28
    for x, y in terms:
        for i in range(14):
            for j in range(14):
                acc[i + j] += s[x][i] * s[y][j]
    return w * max(acc)


def column_fill(op, shape):
    """the largest value a column can take, over 2^64, over every row and lane of op's tables: the product columns with every slot
    at its limb maxima (they are monotone in the limbs), tripled where the engine triples, plus RED_MAX (the reduction's m depend
    on the data, so no single operand shows its maximum); the replay's result is held to lane_value on the way"""
    nq = SHAPES[shape]
    if op == "PROD":
        s = {0: max_vector(1, 1), 1: max_vector(1, 1)}
        out, top = replay([(0, 1)], s, 1)
        assert out == limbs(lane_value([(0, 1)], s, 1))
        return (product_columns_top([(0, 1)], s, 1) + RED_MAX) / 2.0 ** 64
    s = {slot: max_vector(v, lam) for slot, (v, lam) in bound_slots(op).items()}
    for j in range(16 if op == "LINE" else 0):                       # the line tables name both loops' slots
        s[ct.SLOT_LN1 + j] = max_vector(1, 1)
    tables = {"MUL": [MT], "SQR": [ST], "CSQR": [CT], "LINE": [LT[1], LT[2]]}[op]
    triple = op == "CSQR"
    w = 3 if triple and nq >= 2 else 1
    worst = 0
    for tab in tables:
        rows = range(12) if (op != "LINE" or shape == "twelve") else range(16)
        for g in rows:
            for q in range(nq):
                terms = lane_terms(tab[g], q, nq, triple)
                out, top = replay(terms, s, w)
                assert out == limbs(lane_value(terms, s, w)), "the replay and the formula disagree"
                worst = max(worst, product_columns_top(terms, s, w))
    return (worst + RED_MAX) / 2.0 ** 64


def value_bound(op, shape):
    """analytic bound of a call's result, as an integer: lanes below w sum(v_x v_y) p^2 / R + p, summed over a coefficient's lanes,
    the largest over the rows; the narrow cyclotomic squaring ends in the fold (below 2p + p / 1024)"""
    nq = SHAPES[shape]
    if op == "PROD":
        return P * P // R + 1 + P
    if op == "CSQR" and nq == 1:
        r = max(sum(vb_prod("CSQR", x, y) for x, y in lane_terms(CT[g], 0, 1, True)) // R + 1 + P for g in range(12))
        assert 3 * r + 13 * P < 32 * P, "the fold takes values below 32p"
        return 2 * P + (P >> 10)
    tables = {"MUL": [MT], "SQR": [ST], "CSQR": [CT], "LINE": [LT[1], LT[2]]}[op]
    triple = op == "CSQR"
    w = 3 if triple else 1
    worst = 0
    for tab in tables:
        for g in range(12):
            worst = max(worst, sum(w * sum(vb_prod(op, x, y) for x, y in lane_terms(tab[g], q, nq, triple)) // R + 1 + P for q in range(nq)))
    return worst


def vb_prod(op, x, y):
    b = bound_slots(op)
    if op == "LINE":
        for j in range(16):
            b[ct.SLOT_LN1 + j] = (1, 1)
    return b[x][0] * P * b[y][0] * P


# ------------------------------------------------------------------------------------------------ one call each
def vecs(ints):
    return [limbs(v) for v in ints]


def model_mul(a, b, nq):
    """a, b: 12 integers (flat order 2k + part), carried on the device.  Returns 12 integers."""
    s = new_slots()
    stage_a(s, vecs(a))
    stage_b(s, vecs(b))
    return [engine(MT[g], s, nq) for g in range(12)]


def model_sqr(a, nq):
    s = new_slots()
    stage_sqr(s, vecs(a))
    return [engine(ST[g], s, nq) for g in range(12)]


def model_csqr(a, nq):
    s = new_slots()
    av = vecs(a)
    stage_csqr(s, av)
    out = []
    for g in range(12):
        r = engine(CT[g], s, nq, triple=True)
        if nq == 1:        # 3 r + (13p - 2a) on even k, 3 r + 2a on odd k, limb by limb; carry; fold
            rl, g2 = limbs(r), scale(av[g], 2)
            minus = ((g >> 1) & 1) == 0
            h = [3 * rl[i] + (BIAS[(13, 2)][i] - g2[i] if minus else g2[i]) for i in range(14)]
            assert all(0 <= x < (1 << 32) for x in h)
            r = limbs_val(fold(carry(h)))
        out.append(r)
    return out


def model_csqr_run(a, nq, n):
    for _ in range(n):
        a = model_csqr(a, nq)
    return a


def line_slots(s, lines1, lines2, pts):
    for j in range(8):
        s[ct.SLOT_LN1 + j] = limbs(lines1[j])
        s[ct.SLOT_LN2 + j] = limbs(lines2[j])
    for slot, v in zip((ct.SLOT_PX1, ct.SLOT_PY1, ct.SLOT_PX2, ct.SLOT_PY2), pts):
        s[slot] = limbs(v)


def model_line(loop, a, T, lines1, lines2, pts, nq, spare=True):
    """coop_line<loop>: T are the loop's own four T slots.  Returns (12 results, the other loop's four T slots as the spare lanes
    leave them - None where the shape has no spare lanes)."""
    s = new_slots()
    stage_a(s, vecs(a))
    line_slots(s, lines1, lines2, pts)
    tt = ct.SLOT_T1 if loop == 1 else ct.SLOT_T2
    for j in range(4):
        s[tt + j] = limbs(T[j])
    out = [engine(LT[loop][g], s, nq) for g in range(12)]
    return out, ([engine(LT[loop][g], s, nq) for g in range(12, 16)] if spare else None)


def model_prod(lines1, lines2, pts):
    """the twelve shape's pass of eight coop_prod products: T1 then T2"""
    s = new_slots()
    line_slots(s, lines1, lines2, pts)
    return ([lane_value([(ct.SLOT_LN1 + j, ct.SLOT_PX1)], s, 1) for j in range(4)] +
            [lane_value([(ct.SLOT_LN2 + j, ct.SLOT_PX2)], s, 1) for j in range(4)])


def model_round(a, lines1_0, lines1_1, lines2_0, pts, flags, shape):
    """the Miller loop's first round (ln = 0) with its warm-up: returns (f, T1 of line 1 or None)"""
    nq = SHAPES[shape]
    skip1, skip2 = flags & 1, flags & 2
    if shape == "twelve":
        f = model_sqr(a, nq)
        T = model_prod(lines1_0, lines2_0, pts)
        r1, _ = model_line(1, f, T[:4], lines1_0, lines2_0, pts, nq, spare=False)
        f = f if skip1 else r1
        r2, _ = model_line(2, f, T[4:], lines1_0, lines2_0, pts, nq, spare=False)
        return (f if skip2 else r2), None
    _, T1 = model_line(2, a, [0] * 4, lines1_0, lines2_0, pts, nq)         # warm-up: only its spare lanes matter
    f = model_sqr(a, nq)
    r1, T2 = model_line(1, f, T1, lines1_0, lines2_0, pts, nq)
    f = f if skip1 else r1
    r2, T1n = model_line(2, f, T2, lines1_1, lines2_0, pts, nq)              # (LN1 holds the next line of loop 1 by now)
    return (f if skip2 else r2), T1n


def model_conj(a):
    """coop_conj: 6p - a on the odd coefficients (F28_NEG(.., 6, 1), carried)"""
    return [limbs_val(carry(neg(limbs(v), 6, 1))) if (g >> 1) & 1 else v for g, v in enumerate(a)]


# ------------------------------------------------------------------------------------------------ residues
def unmont(ints):
    """12 representatives -> the Fp12 element they spell (6 pairs, plain residues)"""
    return [(ints[2 * k] * RINV % P, ints[2 * k + 1] * RINV % P) for k in range(6)]


def mont(f):
    return [c * R % P for pair in f for c in pair]


def line_element(lines, xp_t, yp):
    """the sparse line c + b w^2 + yP w^3 from the line's constants and b = (b0, b1) (plain residues)"""
    return [(lines[ct.LN_C0], lines[ct.LN_C1]), bls.F2_ZERO, xp_t, (yp, 0), bls.F2_ZERO, bls.F2_ZERO]
