#!/usr/bin/env python3
"""Generates plutus_halo2_verifier_gen_amd/csrc/six_tables.h: the operand tables of the SIX-LANES-PER-PROOF Fp12 engine
of the pairing kernel (h2v_pairing_six.hpp: ten proofs per wave), after checking them twice:
  * at VALUE level against the package's big-integer Fp12 arithmetic (every table, random operands), and
  * at LIMB level against a model of the device code (28-bit limbs, 64-bit column accumulators that wrap, the signed /
    unsigned Montgomery reductions) on operands at their declared bounds - the headroom argument of the header, executed.

Model.  Fp12 = Fp2[w]/(w^6 - xi), element = 6 Fp2 coefficients; lane k < 6 of a group owns coefficient k WHOLE (re, im).
A Karatsuba term is an Fp2 product x * y computed as three Fp products into three sets of column accumulators,
      U += x0 y0        V += x1 y1        W += (x0 + x1)(y0 + y1),
and an engine call (MUL: 6 terms, SQR: 4, LINE: 2 and the lane's own coefficient added) ends with   re = U - V  (signed columns),  im = W - U - V  (column-wise
equal to sum(x0 y1 + x1 y0) because the engine forms the sums LIMB-WISE in registers, so unsigned), one Montgomery reduction each: 3 NT + 2 products
of 196 multiply-adds where the one-coefficient-per-lane engine spends 2 (2 NT + 1) on the same Fp2 coefficient.
Wrapped terms (x xi) take the xi on the A side: XA = xi a = (a0 - a1, a0 + a1).
The cyclotomic squaring is four products P1..P4 into three sets (operands S = re + im - formed by the engine -, M = re - im,
D = 2a; no negated operand): re = P1 + P2 - P4, im = P1 + P3 + P4, the set of P1 + P2 starting as a copy of P1's through the
addend of its first multiply-adds (csqr_table); the lane forms h = 3 (reduced) -/+ 2 g itself and folds it below 2p by a quotient
estimate from the top limb (the +-2/3 constant products of the other engines cost two products more).
A group's operand slots are 56 bytes (14 limbs, no padding) and 38 in number: 2.1 KB per proof, 23 KB per wave of ten.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plutus_halo2_verifier_gen_amd import bls12_381 as bls  # noqa: E402

P = bls.P
R = 1 << 392
MASK = (1 << 28) - 1
M64 = (1 << 64) - 1
N0 = (-pow(P, -1, 1 << 28)) % (1 << 28)
P_L = [(P >> (28 * i)) & MASK for i in range(14)]

# ---- slot map: group-local slots < 64 (38 used, 56 bytes each), wave-shared >= 64
A0 = lambda k: 2 * k
A1 = lambda k: 2 * k + 1
XA0 = lambda k: 12 + 2 * (k - 1)        # k = 1..5 (MUL); the Miller loop stages k = 3..5 only
XA1 = lambda k: 13 + 2 * (k - 1)
B0 = lambda k: 22 + 2 * k               # MUL: b ; SQR / CSQR: D = 2a ; between the squaring and the lines of a Miller round the
B1 = lambda k: 23 + 2 * k               # line products: a = A xP of loop 1 at 22, 23, of loop 2 at 24, 25; b = B yP at 26, 27 and 28, 29
TA1, TA2, TB1, TB2 = (22, 23), (24, 25), (26, 27), (28, 29)
# cyclotomic squaring: M = re - im in the XA area and in the P area; S = re + im is formed by the engine (A0 + A1)
C_M = lambda k: 19 + k if k < 3 else 31 + k     # 19..21, 34..36 over the points
PX1, PY1, PX2, PY2 = 34, 35, 36, 37
N_GROUP_SLOTS = 38
SH = 64
# Lines with a UNIT coefficient.  The plan's line is l = c + ((-lambda) xP) w^2 + yP w^3 with c in Fp2 a constant of the fixed G2
# argument; a factor in Fp2* of the Miller value is killed by the easy part of the final exponentiation, so every line is divided
# by its own c:   l / c = 1 + (A xP) w^2 + (B yP) w^3,   A = -lambda / c,  B = 1 / c   (derived once at plan load), and
# f (l / c) = f + f (a w^2 + b w^3): two Karatsuba terms and the lane's own staged coefficient added after the reduction.
LN1, LN2 = SH, SH + 4                   # per line and loop 4 slots [A0, A1, B0, B1] (the plan-load table of the six-lane engine)
LN_A0, LN_A1, LN_B0, LN_B1 = 0, 1, 2, 3
C23P, C23N, ZERO = SH + 16, SH + 17, SH + 18
N_SHARED_SLOTS = 19
C23 = 2 * pow(3, -1, P) % P
N_MUL, N_SQR, N_LINE, N_CSQR = 6, 4, 2, 4
ZT = (ZERO, ZERO, ZERO, ZERO)


def a_side(i, wrapped):
    return (XA0(i), XA1(i)) if wrapped else (A0(i), A1(i))


def kterm(xs, ys):
    return (xs[0], ys[0], xs[1], ys[1])


def mul_table():
    tab = []
    for k in range(6):
        terms = []
        for i in range(6):
            j = (k - i) % 6
            terms.append(kterm(a_side(i, i > k), (B0(j), B1(j))))
        tab.append(terms)
    return tab


def sqr_table():
    """c_k = sum over unordered pairs {i, j}, i + j = k mod 6, of a_i a_j (x 2 when i != j, x xi when i + j >= 6).
    i < j unwrapped: a_i x D_j ; wrapped: D_i x XA_j (j in {4, 5}) ; squares: a_i x a_i, wrapped a_i x XA_i (i >= 3)."""
    D = lambda k: (B0(k), B1(k))
    tab = []
    for k in range(6):
        terms = []
        for i in range(6):
            for j in range(i, 6):
                if (i + j) % 6 != k:
                    continue
                wrapped = i + j >= 6
                if i < j:
                    terms.append(kterm(D(i), a_side(j, True)) if wrapped else kterm(a_side(i, False), D(j)))
                else:
                    terms.append(kterm(a_side(i, False), a_side(i, wrapped)))
        assert len(terms) <= N_SQR
        while len(terms) < N_SQR:
            terms.append(ZT)
        tab.append(terms)
    return tab


def line_table(loop):
    """coefficient k of f (a w^2 + b w^3) = f_(k-2) a + f_(k-3) b (indices mod 6, x xi when they wrap); f_k itself is added by the
    engine from the lane's own A slots (kara_engine: add_self)"""
    ta, tb = (TA1, TB1) if loop == 1 else (TA2, TB2)
    tab = []
    for k in range(6):
        i2, i3 = (k - 2) % 6, (k - 3) % 6
        tab.append([kterm(a_side(i2, i2 > k), ta),
                    kterm(a_side(i3, i3 > k), tb)])
    return tab


def csqr_table():
    """Per lane FOUR products (x + x2) * y, P1..P4, into three sets of column accumulators
           A = P1      B = A + P2 (B starts as a copy of A: the addend of P2's first multiply-add per column)      A += P3      C = P4
       and the engine ends with re = B - C = P1 + P2 - P4 (signed columns), im = A + C = P1 + P3 + P4, one reduction each
       (x2 = ZERO except where a sum is formed limb-wise by the engine: S = re + im from A0, A1; 2 S from B0, B1; 2 M from M, M).
       Granger-Scott with the pair (a, b) of the lane's kind, D = 2 (re, im), M = re - im (+ 7p), S = re + im:
       kind                      P1 (both parts)    P2                 P3                   P4
       even    a^2 + xi b^2      S_b M_b            S_a M_a            a0 D_a1              b0 D_b1
       odd     2 a b             a0 D_b1            D_a0 M_b           D_a1 M_b             a1 D_b1
       xi-odd  2 xi a b          M_a D_b1           (M_a + M_a) M_b    (D_a0 + D_a1) M_b    (a0 + a1) D_b1        (xi a = (M_a, S_a))
       odd:  re = 2 a0 b1 + 2 a0 (b0 - b1) - 2 a1 b1,  im = 2 a0 b1 + 2 a1 (b0 - b1) + 2 a1 b1.  No lane has a null product, and no
       negated operand is staged.  The lane then forms h = 3 (reduced) -/+ 2 g_k itself and folds it below 2p (h2v_pairing_six.hpp: six_csqr_run)."""
    kind = {0: ("even", 0, 3), 3: ("odd", 0, 3), 1: ("xi_odd", 2, 5), 4: ("even", 2, 5), 2: ("even", 1, 4), 5: ("odd", 1, 4)}
    one = lambda x, y: (x, ZERO, y)
    SxM = lambda k: (A0(k), A1(k), C_M(k))
    tab = []
    for k in range(6):
        ty, a, b = kind[k]
        if ty == "even":
            sets = [SxM(b), SxM(a), one(A0(a), B1(a)), one(A0(b), B1(b))]
        elif ty == "odd":
            sets = [one(A0(a), B1(b)), one(B0(a), C_M(b)), one(B1(a), C_M(b)), one(A1(a), B1(b))]
        else:
            sets = [one(C_M(a), B1(b)), (C_M(a), C_M(a), C_M(b)), (B0(a), B1(a), C_M(b)), (A0(a), A1(a), B1(b))]
        assert len(sets) == N_CSQR
        tab.append(sets)
    return tab


# ----------------------------------------------------------------------------- staging (value, limb bound) models
class Slots(dict):
    """slot -> list of 14 limbs (limbs may exceed 28 bits where the device stores them uncarried)"""

    def __init__(self):
        super().__init__()
        self.lam = {}                   # slot -> bound on its limbs (the analytic headroom check uses these, not the data)

    def put(self, s, value):            # carried
        self[s] = [(value >> (28 * i)) & MASK for i in range(13)] + [value >> (28 * 13)]
        assert self[s][13] < (1 << 28)
        self.lam[s] = 1 << 28

    def put_sum(self, s, *src):         # limb-wise sum of staged slots (uncarried)
        self[s] = [sum(self[q][i] for q in src) for i in range(14)]
        self.lam[s] = sum(self.lam[q] for q in src)

    def put_scaled(self, s, src, f):    # limb-wise multiple (uncarried)
        self[s] = [f * v for v in self[src]]
        self.lam[s] = f * self.lam[src]

    def val(self, s):
        return sum(v << (28 * i) for i, v in enumerate(self[s]))


def stage_a(s, f, xa_from, K=7):
    """f: list of 6 (re, im) integer representatives (any multiple of p allowed; im below (K - 1) p: XA0 = re - im + K p)"""
    for k in range(6):
        assert f[k][1] <= (K - 1) * P
        s.put(A0(k), f[k][0]); s.put(A1(k), f[k][1])
        if k >= xa_from:
            s.put(XA0(k), f[k][0] + K * P - f[k][1]); s.put(XA1(k), f[k][0] + f[k][1])


def stage_b(s, f):
    for k in range(6):
        s.put(B0(k), f[k][0]); s.put(B1(k), f[k][1])


def stage_d(s, f):
    for k in range(6):
        s.put(A0(k), f[k][0]); s.put(A1(k), f[k][1])
        s.put_scaled(B0(k), A0(k), 2); s.put_scaled(B1(k), A1(k), 2)


def stage_csqr(s, g):
    s.put(C23P, C23 * R % P); s.put(C23N, (-C23) % P * R % P)     # Montgomery forms of +-2/3
    for k in range(6):
        s.put(A0(k), g[k][0]); s.put(A1(k), g[k][1])
        s.put_scaled(B0(k), A0(k), 2); s.put_scaled(B1(k), A1(k), 2)
        s.put(C_M(k), g[k][0] + 7 * P - g[k][1])


# ----------------------------------------------------------------------------- the device engine, limb for limb
def mac(acc, x, y):
    for i in range(14):
        for j in range(14):
            acc[i + j] = (acc[i + j] + x[i] * y[j]) & M64
            assert x[i] < (1 << 32) and y[j] < (1 << 32)


def to_signed(v):
    return v - (1 << 64) if v >> 63 else v


def reduce_cols(acc, signed, add=None):
    """Montgomery reduction of 28 columns (mod 2^64 registers); signed: columns are two's complement, p is added at the
    end.  add: 14 carried limbs added to columns 14..27 first (the value add R: the result is the reduced value + add).
    Returns the 14 result limbs (carried) - asserts that no column left its register."""
    a = [to_signed(v) if signed else v for v in acc]
    lo, hi = (-(1 << 63), 1 << 63) if signed else (0, 1 << 64)
    if add is not None:
        assert all(0 <= v < (1 << 28) for v in add)
        for k in range(14):
            a[14 + k] += add[k]
            assert lo <= a[14 + k] < hi
    for k in range(14):
        m = ((a[k] & 0xffffffff) * N0) & MASK
        for j in range(14):
            a[k + j] += m * P_L[j]
            assert lo <= a[k + j] < hi, "column overflow in the reduction"
        assert a[k] & MASK == 0
        a[k + 1] += a[k] >> 28
        assert lo <= a[k + 1] < hi
    out, carry = [], 0
    for k in range(13):
        carry += a[14 + k] + (P_L[k] if signed else 0)
        out.append(carry & MASK)
        carry >>= 28
    top = carry + a[27] + (P_L[13] if signed else 0)
    assert 0 <= top < (1 << 32), "negative or oversized result"
    return out + [top]


def limbs_val(l):
    return sum(v << (28 * i) for i, v in enumerate(l))


RED = 15 << 56      # what the reduction adds to a column at most: 14 products m p_j and a carry


def kara_engine(terms, s, add_self=None):
    """add_self = k: the lane's own staged coefficient (slots A0(k), A1(k)) is added to the reduced parts (line steps)"""
    # analytic headroom from the limb bounds of the staged slots (whatever the data)
    col = lambda x, y: 14 * s.lam[x] * s.lam[y]
    assert sum(col(t[0], t[1]) for t in terms) + RED < (1 << 63) and sum(col(t[2], t[3]) for t in terms) < (1 << 63), "re columns"
    assert sum(col(t[0], t[3]) + col(t[2], t[1]) for t in terms) + RED < (1 << 64), "im columns"
    U, V, W = [0] * 28, [0] * 28, [0] * 28
    for (x0, y0, x1, y1) in terms:
        mac(U, s[x0], s[y0]); mac(V, s[x1], s[y1])
        mac(W, [a + b for a, b in zip(s[x0], s[x1])], [a + b for a, b in zip(s[y0], s[y1])])     # the sums, limb-wise, in registers
    for acc in (U, V):
        assert max(acc) < (1 << 63), "U / V must not wrap (signed difference)"
    im = [(W[i] - U[i] - V[i]) & M64 for i in range(28)]
    re = [(U[i] - V[i]) & M64 for i in range(28)]
    # the column-wise identity: im columns are the true (non-negative) cross sums
    chk = [0] * 28
    for (x0, y0, x1, y1) in terms:
        for i in range(14):
            for j in range(14):
                chk[i + j] += s[x0][i] * s[y1][j] + s[x1][i] * s[y0][j]
    assert chk == im and max(chk) < (1 << 64)
    if add_self is not None:
        return limbs_val(reduce_cols(re, True, s[A0(add_self)])), limbs_val(reduce_cols(im, False, s[A1(add_self)]))
    return limbs_val(reduce_cols(re, True)), limbs_val(reduce_cols(im, False))


# ----------------------------------------------------------------------------- value bounds of a Miller round
# An engine result is (columns + m p) / R (+ p for the signed part) with m < R: below  sum(v_x v_y) p^2 / R + p  (+ p).  A line step
# adds the staged coefficient, so the value GROWS from the squaring to the last line of a round (up to four lines: two steps of
# two loops) and falls back with the next squaring.  MILLER_RE / MILLER_IM are what the loop's staging accepts; the
# propagation below proves that a round started inside them ends inside them, with XA0 = re - im + MILLER_K p.
MILLER_K = 11                      # the bias of XA0 in the Miller loop's staging (F28_BIAS_11_1): im <= 10 p
MILLER_RE, MILLER_IM = 12, 7       # multiples of p


def engine_bound(table, vb):
    """(re, im) bounds, as integers, of every lane's result for slot value bounds vb (slot -> integer bound)"""
    out = []
    for terms in table:
        re = sum(vb[t[0]] * vb[t[1]] for t in terms) // R + 1 + 2 * P
        im = sum(vb[t[0]] * vb[t[3]] + vb[t[2]] * vb[t[1]] for t in terms) // R + 1 + P
        out.append((re, im))
    return max(o[0] for o in out), max(o[1] for o in out)


def miller_round_bounds():
    """worst case of one round: squaring of a value at the staging bound, then four line steps; returns the (re, im) after each"""
    def staged(re, im, with_d):
        vb = {ZERO: 0}
        for k in range(6):
            vb[A0(k)], vb[A1(k)] = re, im
            vb[XA0(k)], vb[XA1(k)] = re + MILLER_K * P, re + im
            if with_d:
                vb[B0(k)], vb[B1(k)] = 2 * re, 2 * im
        for t in (TA1, TA2, TB1, TB2):
            if not with_d:
                vb[t[0]] = vb[t[1]] = 2 * P              # reduced products
        return vb
    re, im = MILLER_RE * P, MILLER_IM * P
    assert im <= (MILLER_K - 1) * P
    re, im = engine_bound(sqr_table(), staged(re, im, True))
    trail = [(re, im)]
    for step in range(4):
        assert re <= MILLER_RE * P and im <= MILLER_IM * P, "a line step would be staged outside the loop's bounds"
        dre, dim = engine_bound(line_table(1 + step % 2), staged(re, im, False))
        re, im = re + dre, im + dim
        trail.append((re, im))
    assert re <= MILLER_RE * P and im <= MILLER_IM * P, "the next squaring would be staged outside the loop's bounds"
    assert re < 32 * P and im < 32 * P                   # what the fold after the loop is handed
    return trail


FOLD_M = (1 << 32) // ((P >> 364) + 1)
BIAS_13_2 = None


def bias_13_2():
    """13 p written with every limb below the top >= 2 * 2^28 (tools/gen_device_consts.py: bias(13, 2))"""
    c = [(13 * P >> (28 * i)) & MASK for i in range(13)] + [13 * P >> 364]
    sp = 3
    out = [c[0] + (sp << 28)] + [c[i] + (sp << 28) - sp for i in range(1, 13)] + [c[13] - sp]
    assert sum(x << (28 * i) for i, x in enumerate(out)) == 13 * P
    return out


FOLD_LIMB_MAX = (1 << 31) - 1       # what the squaring's tail hands the fold at most: 3 (2^28 - 1) + a bias limb below 2^30 (or 2 g, below 2^29)


def fold(l):
    """the device's f28_fold: limbs of a value below 32 p, UNCARRIED (every limb below 2^31) -> the same residue below 2p (and a
    hair), carried.  The quotient is estimated from the top limb as it stands: the lower limbs only add to the value, so q is
    never too large; against the carried top limb it misses the carry the lower limbs send up (below 8), which moves the
    estimate by less than 8 / (p >> 364) < 2^-21 - the "at most one too small" of the carried form stands, the hair grows by
    that much.  The signed carry chain that subtracts q p normalises the limbs on the way."""
    assert all(0 <= v <= FOLD_LIMB_MAX for v in l[:13]) and 0 <= l[13] < (1 << 22)
    assert limbs_val(l) < 32 * P
    q = (l[13] * FOLD_M) >> 32
    assert q * P <= limbs_val(l), "quotient estimate too large"
    out, t = [], 0
    for i in range(14):
        t += l[i] - q * P_L[i]
        assert -(1 << 63) <= t < (1 << 63)
        out.append(t & MASK if i < 13 else t)
        t >>= 28
    assert t == 0 and 0 <= out[13] < (1 << 28)
    return out


def uncarried_forms(v, rng):
    """limb vectors of the value v with limbs up to FOLD_LIMB_MAX: the carried form, the form with EVERY lower limb at its
    maximum that v allows (each limb borrows from the one above, lowest first), and random forms in between"""
    base = [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]
    forms = [list(base)]
    for mode in ("max", "rnd", "rnd"):
        l = list(base)
        for i in range(13):               # move as much as allowed from limb i + 1 down into limb i
            room = (FOLD_LIMB_MAX - l[i]) >> 28
            k = min(room, l[i + 1])
            if mode == "rnd":
                k = rng.randrange(k + 1)
            l[i + 1] -= k
            l[i] += k << 28
        assert limbs_val(l) == v and all(0 <= x <= FOLD_LIMB_MAX for x in l[:13])
        forms.append(l)
    return forms


CSQR_RE_BOUND, CSQR_IM_BOUND = 22 * P // 10, 12 * P // 10      # the reduced parts of a squaring (operands staged by stage_csqr: v <= 6)


def csqr_engine(sets, s, g, k, reduced=None):
    """sets: the lane's four products P1..P4; g = (re, im) limbs of the lane's own coefficient as staged in A0(k), A1(k).
    reduced: a list that receives the two reduced parts (before 3 r -/+ 2 g), for the tests"""
    lam3 = lambda t: 14 * (s.lam[t[0]] + s.lam[t[1]]) * s.lam[t[2]]
    assert lam3(sets[0]) + lam3(sets[1]) + RED < (1 << 63) and lam3(sets[3]) < (1 << 63), "re columns"
    assert lam3(sets[0]) + lam3(sets[2]) + lam3(sets[3]) + RED < (1 << 64), "im columns"
    prod = lambda t: ([a + b for a, b in zip(s[t[0]], s[t[1]])], s[t[2]])
    A, C = [0] * 28, [0] * 28
    mac(A, *prod(sets[0]))
    B = list(A)                         # (the device: A's column is the addend of the first multiply-add into B's)
    mac(B, *prod(sets[1]))
    mac(A, *prod(sets[2]))
    mac(C, *prod(sets[3]))
    assert max(B) < (1 << 63) and max(C) < (1 << 63)
    re = [(B[i] - C[i]) & M64 for i in range(28)]
    im = [(A[i] + C[i]) & M64 for i in range(28)]
    r = [reduce_cols(re, True), reduce_cols(im, False)]
    assert limbs_val(r[0]) < CSQR_RE_BOUND and limbs_val(r[1]) < CSQR_IM_BOUND
    if reduced is not None:
        reduced.extend(limbs_val(v) for v in r)
    bias = bias_13_2()
    out = []
    for part in range(2):
        two_g = [2 * v for v in s[(A0 if part == 0 else A1)(k)]]
        h = [3 * r[part][i] + (bias[i] - two_g[i] if k % 2 == 0 else two_g[i]) for i in range(14)]
        assert all(0 <= v <= FOLD_LIMB_MAX for v in h)
        f = fold(h)                     # uncarried: the fold's carry chain is the only one
        assert limbs_val(f) < 2 * P + (P >> 10)
        out.append(limbs_val(f))
    return out[0], out[1]


def prod_engine(s, x, y):
    acc = [0] * 28
    mac(acc, s[x], s[y])
    return limbs_val(reduce_cols(acc, False))


# ----------------------------------------------------------------------------- checks
RINV = pow(R, -1, P)


def mont(f):        # value -> Montgomery representative
    return [(a * R % P, b * R % P) for a, b in f]


def unmont(f):
    return [(a * RINV % P, b * RINV % P) for a, b in f]


def spread(rng, f, vmax):
    """random representatives: value + t p below vmax p"""
    return [tuple(c + rng.randrange(vmax) * P for c in pair) for pair in f]


def self_check():
    rng = random.Random(7)
    rf2 = lambda: (rng.randrange(P), rng.randrange(P))
    mt, st, ct = mul_table(), sqr_table(), csqr_table()
    for trial in range(6):
        vmax = 6 if trial else 1
        a = [rf2() for _ in range(6)]
        b = [rf2() for _ in range(6)]
        s = Slots(); s.put(ZERO, 0); s.lam[ZERO] = 0
        am, bm = spread(rng, mont(a), vmax), spread(rng, mont(b), vmax)
        stage_a(s, am, 1); stage_b(s, bm)
        got = [kara_engine(mt[k], s) for k in range(6)]
        assert all(v < 3 * P for pair in got for v in pair)
        assert unmont([(x % P, y % P) for x, y in got]) == bls.f12_mul(a, b)
        # squaring
        s = Slots(); s.put(ZERO, 0); s.lam[ZERO] = 0
        stage_d(s, am); stage_a(s, am, 3)
        got = [kara_engine(st[k], s) for k in range(6)]
        assert all(v < 3 * P for pair in got for v in pair)
        assert unmont([(x % P, y % P) for x, y in got]) == bls.f12_sqr(a)
        # lines (unit coefficient): f + f (a w^2 + b w^3) against f * (line / c), on a value at the top of what the loop stages
        fm = spread(rng, mont(a), 1)
        if trial:
            fm = [(c0 + rng.randrange(MILLER_RE - 4, MILLER_RE) * P, c1 + rng.randrange(MILLER_IM - 3, MILLER_IM) * P) for c0, c1 in fm]
        for loop in (1, 2):
            lt = line_table(loop)
            lam, cc = rf2(), rf2()
            xp, yp = rng.randrange(P), rng.randrange(P)
            s = Slots(); s.put(ZERO, 0); s.lam[ZERO] = 0
            stage_a(s, fm, 3, MILLER_K)
            ln = LN1 if loop == 1 else LN2
            ci = bls.f2_inv(cc)
            ca, cb = bls.f2_mul(bls.f2_neg(lam), ci), ci                       # A = -lambda / c, B = 1 / c
            s.put(ln + LN_A0, ca[0] * R % P); s.put(ln + LN_A1, ca[1] * R % P)
            s.put(ln + LN_B0, cb[0] * R % P); s.put(ln + LN_B1, cb[1] * R % P)
            px, py = (PX1, PY1) if loop == 1 else (PX2, PY2)
            s.put(px, xp * R % P); s.put(py, yp * R % P)
            ta, tb = (TA1, TB1) if loop == 1 else (TA2, TB2)
            prods = [prod_engine(s, ln + LN_A0, px), prod_engine(s, ln + LN_A1, px), prod_engine(s, ln + LN_B0, py), prod_engine(s, ln + LN_B1, py)]
            assert all(v < 2 * P for v in prods)
            s.put(ta[0], prods[0]); s.put(ta[1], prods[1]); s.put(tb[0], prods[2]); s.put(tb[1], prods[3])
            got = [kara_engine(lt[k], s, add_self=k) for k in range(6)]
            # the step adds at most (2p, p) and a little to the staged coefficient (miller_round_bounds takes the exact figure)
            assert all(x < fm[k][0] + 2 * P + (P >> 3) and y < fm[k][1] + P + (P >> 3) for k, (x, y) in enumerate(got))
            line = [cc, bls.F2_ZERO, bls.f2_scale(bls.f2_neg(lam), xp), (yp, 0), bls.F2_ZERO, bls.F2_ZERO]
            unit = [bls.F2_ONE, bls.F2_ZERO, bls.f2_scale(ca, xp), bls.f2_scale(cb, yp), bls.F2_ZERO, bls.F2_ZERO]
            assert [bls.f2_mul(t, cc) for t in unit] == line                   # line / c
            assert unmont([(x % P, y % P) for x, y in got]) == bls.f12_mul(a, unit)
            # and a squaring staged the same way (the loop's squaring takes what the lines leave)
            s = Slots(); s.put(ZERO, 0); s.lam[ZERO] = 0
            stage_d(s, fm); stage_a(s, fm, 3, MILLER_K)
            got = [kara_engine(st[k], s) for k in range(6)]
            assert all(v < 3 * P for pair in got for v in pair)
            assert unmont([(x % P, y % P) for x, y in got]) == bls.f12_sqr(a)
    trail = miller_round_bounds()
    assert trail[0][0] < 3 * P and trail[0][1] < 2 * P
    # the fold on its own: every multiple of p up to 32 p and its neighbours, random values, the largest value it is handed -
    # each in its carried form, with every lower limb at its maximum, and in random uncarried forms
    for v in [k * P + d for k in range(32) for d in (-1, 0, 1) if k * P + d >= 0] + [rng.randrange(32 * P) for _ in range(2000)] + [32 * P - 1]:
        for lim in uncarried_forms(v, rng):
            out = fold(lim)
            f = limbs_val(out)
            assert f % P == v % P and f < 2 * P + (P >> 10)
            assert all(x < (1 << 28) for x in out)      # carried: what six_stage_a, six_mul and six_conj accept (v <= 6)
    # cyclotomic squaring on an element of the cyclotomic subgroup
    f = bls.miller_loop(bls.g1_mul(bls.G1_GEN, 777), bls.g2_mul(bls.G2_GEN, 3))
    t = bls.f12_mul(bls.f12_conj(f), bls.f12_inv(f))
    t = bls.f12_mul(bls.f12_frob(bls.f12_frob(t)), t)
    for trial in range(4):
        s = Slots(); s.put(ZERO, 0); s.lam[ZERO] = 0
        stage_csqr(s, spread(rng, mont(t), 6))
        got = [csqr_engine(ct[k], s, None, k) for k in range(6)]
        assert all(v < 3 * P for pair in got for v in pair)
        assert unmont([(x % P, y % P) for x, y in got]) == bls.f12_sqr(t)
        t = bls.f12_mul(bls.f12_sqr(t), t)
    return True


def emit():
    assert self_check()
    o = ["// GENERATED by tools/gen_six_tables.py (tables checked against big-integer Fp12 arithmetic and a limb-level model of the",
         "// engine) - do not edit.", "#pragma once", "#include <stdint.h>"]
    for name, val in (("A", 0), ("XA", 12), ("T", TA1[0]), ("B", 22), ("PX1", PX1),
                      ("PY1", PY1), ("PX2", PX2), ("PY2", PY2), ("ZERO", ZERO), ("LN1", LN1), ("LN2", LN2), ("C23P", C23P), ("C23N", C23N)):
        o.append("#define SIX_SLOT_%s %d" % (name, val))
    for name, val in (("N_GROUP_SLOTS", N_GROUP_SLOTS), ("N_SHARED_SLOTS", N_SHARED_SLOTS), ("SHARED_BASE", SH), ("N_MUL", N_MUL), ("N_SQR", N_SQR),
                      ("N_LINE", N_LINE), ("N_CSQR", N_CSQR), ("MILLER_K", MILLER_K)):
        o.append("#define SIX_%s %d" % (name, val))

    def arr(name, tab, width):
        rows = ["{" + ", ".join(str(v) for term in tab[k] for v in term) + "}" for k in range(6)]
        o.append("__device__ alignas(4) static constexpr uint8_t %s[6][%d] = {\n    %s};" % (name, width, ",\n    ".join(rows)))

    arr("SIX_TAB_MUL", mul_table(), 4 * N_MUL)
    arr("SIX_TAB_SQR", sqr_table(), 4 * N_SQR)
    arr("SIX_TAB_LINE1", line_table(1), 4 * N_LINE)
    arr("SIX_TAB_LINE2", line_table(2), 4 * N_LINE)
    arr("SIX_TAB_CSQR", csqr_table(), 3 * N_CSQR)
    path = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "six_tables.h")
    with open(path, "w") as f:
        f.write("\n".join(o) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    emit()
