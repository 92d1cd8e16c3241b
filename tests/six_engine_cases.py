"""Case tables for single calls of the six-lane pairing engine (csrc/h2v_pairing_six.hpp; device probe h2v_probe_six_call): operands
that sit ON the bounds the engine's headroom argument states, and for each what the limb model of tools/gen_six_tables.py yields -
the model alone must stay inside its own assertions on every case, which is the condition on the inputs.  Shared by the device test
(tests/test_six_engine_calls_gpu.py: exact comparison, limb for limb) and the host test (tests/test_six_engine_cases.py: the tables
hold what they are meant to hold).

A table is {"cases": [...], "lines": the launch's eight line constants or None}; case 0 is the op's hardest.  A case is a dict:
  a      6 pairs (re, im) of integer representatives (FOLD: 12 raw limb vectors)          b      6 pairs (MUL)
  T      8 integers, slots 22..29 (LINE1 / LINE2)        pts    4 integers PX1, PY1, PX2, PY2       flags  bit 0 skip1, bit 1 skip2
  want   12 integers re0, im0, re1, ... (PROD2: the 8 T slots; FOLD: 12 limb vectors); FROB / INV: residues, `ok` beside them
A result is carried, so its limb vector and its integer determine each other: limbs(want) is what the device must return."""
import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_six_tables as g  # noqa: E402
from plutus_halo2_verifier_gen_amd import bls12_381 as bls  # noqa: E402

P, R, MASK = g.P, g.R, g.MASK
OPS = ("MUL", "SQR", "LINE1", "LINE2", "PROD2", "ROUND", "CSQR", "CONJ", "FROB", "INV", "FOLD")
SIZES = (1, 10, 11, 21)              # groups per launch: one, a full wave, a lone group in a trailing wave, two waves and one
CSQR_RUNS = (1, 2, 3, 9, 16, 32)     # the run lengths of x^|x|
CSQR_LONG = 4                        # elements that take the runs of 16 and 32
V_MUL = 6                            # MUL, CSQR: representatives below 6p
V_CONJ = 5                           # CONJ, FROB, INV: below 5p (the header: v <= 5)
RE_MAX, IM_MAX = g.MILLER_RE * P, g.MILLER_IM * P      # what the Miller loop's staging accepts, inclusive
MONT1 = R % P
EDGE_FP = (0, MONT1, P - MONT1, P - 1)                 # 0, 1, p - 1 in Montgomery form, and the largest canonical limb vector
MT, ST, CT = g.mul_table(), g.sqr_table(), g.csqr_table()
LT = {1: g.line_table(1), 2: g.line_table(2)}


def limbs(v):
    """the carried limb vector of v (below 2^392)"""
    assert 0 <= v < 1 << 392
    return [(v >> (28 * i)) & MASK for i in range(13)] + [v >> 364]


def flat(pairs):
    return [v for pair in pairs for v in pair]


def limbs_all_max(bound):
    """the largest value below `bound` whose thirteen lower limbs are all 2^28 - 1"""
    low = (1 << 364) - 1
    v = (((bound - 1 - low) >> 364) << 364) | low
    assert low <= v < bound
    return v


def slots():
    s = g.Slots()
    s.put(g.ZERO, 0)
    s.lam[g.ZERO] = 0
    return s


# ------------------------------------------------------------------------------------------------ the model, one engine call each
def model_mul(a, b):
    s = slots()
    g.stage_a(s, a, 1)
    g.stage_b(s, b)
    return [g.kara_engine(MT[k], s) for k in range(6)]


def stage_miller(s, a):
    assert all(re <= RE_MAX and im <= IM_MAX for re, im in a)
    g.stage_a(s, a, 3, g.MILLER_K)


def model_sqr(a):
    s = slots()
    g.stage_d(s, a)
    stage_miller(s, a)
    return [g.kara_engine(ST[k], s) for k in range(6)]


def model_line(loop, a, T, skip):
    if skip:
        return [tuple(c) for c in a]
    s = slots()
    stage_miller(s, a)
    for j, v in enumerate(T):
        assert v < 2 * P
        s.put(g.TA1[0] + j, v)
    return [g.kara_engine(LT[loop][k], s, add_self=k) for k in range(6)]


def model_prod2(lines, pts):
    """slots 22..29 as six_prod2 leaves them: a = A xP of loop 1, of loop 2, b = B yP of loop 1, of loop 2 (two parts each)"""
    s = slots()
    for j, v in enumerate(lines):
        assert v < P
        s.put(g.LN1 + j, v)
    for slot, v in zip((g.PX1, g.PY1, g.PX2, g.PY2), pts):
        assert v < P
        s.put(slot, v)
    A, B = (g.LN_A0, g.LN_A1), (g.LN_B0, g.LN_B1)
    T = ([g.prod_engine(s, g.LN1 + q, g.PX1) for q in A] + [g.prod_engine(s, g.LN2 + q, g.PX2) for q in A] +
         [g.prod_engine(s, g.LN1 + q, g.PY1) for q in B] + [g.prod_engine(s, g.LN2 + q, g.PY2) for q in B])
    assert all(v < 2 * P for v in T)
    return T


def model_round(a, lines, pts, flags):
    f = model_sqr(a)
    T = model_prod2(lines, pts)
    f = model_line(1, f, T, flags & 1)
    return model_line(2, f, T, flags & 2)


def csqr_step(x, trace=None):
    """one squaring of a run: restaged as six_csqr_run does (M = re - im + 7p carried, D = 2x uncarried).  trace: receives, per
    lane and part, the uncarried limb vector 3 r -/+ 2 g the lane hands the fold"""
    s = slots()
    g.stage_csqr(s, x)
    out = []
    for k in range(6):
        red = []
        out.append(g.csqr_engine(CT[k], s, None, k, reduced=red))
        if trace is not None:
            bias = g.bias_13_2()
            for part in range(2):
                r, two_g = limbs(red[part]), [2 * v for v in limbs(x[k][part])]
                trace.append((k, [3 * r[i] + (bias[i] - two_g[i] if k % 2 == 0 else two_g[i]) for i in range(14)]))
    return out


def model_conj(a):
    """six_conj: 6p - a on the odd coefficients (F28_NEG with the 6p bias, carried), a itself on the even ones"""
    return [(6 * P - re, 6 * P - im) if k & 1 else (re, im) for k, (re, im) in enumerate(a)]


def unmont(pairs):
    return [tuple(v * g.RINV % P for v in pair) for pair in pairs]


def mont(pairs):
    return [tuple(v * R % P for v in pair) for pair in pairs]


# ------------------------------------------------------------------------------------------------ operands
def rf(rng, vmax):
    """a representative anywhere below vmax p"""
    return rng.randrange(P) + rng.randrange(vmax) * P


def elem(rng, vmax):
    return [(rf(rng, vmax), rf(rng, vmax)) for _ in range(6)]


def const_elem(re, im):
    return [(re, im)] * 6


def with_value(rng, vmax, at, v):
    """a random element with part `at` (0..11) set to v"""
    e = flat(elem(rng, vmax))
    e[at] = v
    return [(e[2 * k], e[2 * k + 1]) for k in range(6)]


def mul_operands(rng, vmax):
    """(a, b) pairs: the corners, single coefficients on the special values, limbs at their maximum, random representatives"""
    top = vmax * P - 1
    out = [(const_elem(top, top), const_elem(top, top)),
           (const_elem(top, 0), const_elem(0, top)),                 # re = 0, the largest im
           (const_elem(0, top), const_elem(0, top)),                 # U = 0: the most negative re columns
           (const_elem(0, 0), const_elem(0, 0)),
           (const_elem(*[limbs_all_max(vmax * P)] * 2), const_elem(*[limbs_all_max(vmax * P)] * 2))]     # W's middle columns wrap
    for j, v in enumerate((0, 1, P - 1, P, P + 1, top)):
        out.append((with_value(rng, vmax, (5 * j) % 12, v), with_value(rng, vmax, (7 * j + 3) % 12, v)))
    for t in range(vmax):
        out.append(([(rng.randrange(P) + t * P, rng.randrange(P) + (vmax - 1 - t) * P) for _ in range(6)], elem(rng, vmax)))
    out += [(elem(rng, vmax), elem(rng, vmax)) for _ in range(4)]
    return out


def miller_operands(rng):
    """values the Miller loop's staging takes: re <= 12p, im <= 7p, the bounds themselves included"""
    rre, rim = lambda: rng.randrange(RE_MAX + 1), lambda: rng.randrange(IM_MAX + 1)
    out = [const_elem(RE_MAX, IM_MAX), const_elem(RE_MAX, 0), const_elem(0, IM_MAX), const_elem(0, 0),
           const_elem(limbs_all_max(RE_MAX), limbs_all_max(IM_MAX))]
    out += [[(v, rim()) for _ in range(6)] for v in (RE_MAX - 1, RE_MAX)]
    out += [[(rre(), v) for _ in range(6)] for v in (IM_MAX - 1, IM_MAX)]
    for k in range(6):                                                 # one coefficient on the bounds, the others anywhere
        e = [(rre(), rim()) for _ in range(6)]
        e[k] = (RE_MAX, IM_MAX)
        out.append(e)
    out += [[(rre(), rim()) for _ in range(6)] for _ in range(6)]
    return out


def point_sets(rng):
    rp = lambda: rng.randrange(P)
    out = [(P - 1,) * 4, (0,) * 4, (MONT1,) * 4, (P - MONT1,) * 4]
    out += [tuple(rp() for _ in range(4)) for _ in range(4)]
    out += [(0, rp(), rp(), P - 1), (P - 1, 0, MONT1, rp()), (rp(), P - 1, 0, P - MONT1), (P - MONT1, MONT1, P - 1, 0)]
    return out


def line_constants(rng):
    """the launch's eight constants [A0, A1, B0, B1] of loop 1, then of loop 2: every slot kind meets 0, 1, p - 1 or a random value"""
    rp = lambda: rng.randrange(P)
    return [rp(), P - 1, 0, MONT1, P - MONT1, rp(), P - 1, rp()]


# ------------------------------------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def table(op):
    rng = random.Random(0x51c + OPS.index(op))
    cases, lines = [], None
    if op == "MUL":
        for a, b in mul_operands(rng, V_MUL):
            cases.append({"a": a, "b": b, "want": flat(model_mul(a, b))})
    elif op == "SQR":
        for a in miller_operands(rng):
            cases.append({"a": a, "want": flat(model_sqr(a))})
    elif op in ("LINE1", "LINE2"):
        loop = 1 if op == "LINE1" else 2
        lines_c, pts = line_constants(rng), point_sets(rng)
        t_sets = [[2 * P - 1] * 8, [0] * 8, [P] * 8] + [model_prod2(lines_c, p) for p in pts[:3]]
        # flags: bit 0 skips loop 1's line, bit 1 loop 2's.  EVERY operand of miller_operands and every T set RUNS the line under
        # test (its own bit clear; the other loop's bit, which the op must ignore, set in every second case); the skipped cases
        # are duplicates of a running operand with T slots of their own, placed behind every third case so that a block holds
        # skipped groups between running neighbours.
        own, other = loop, 3 - loop
        ops_a = miller_operands(rng)
        for j, a in enumerate(ops_a):
            T = t_sets[j] if j < len(t_sets) else [rng.randrange(2 * P) for _ in range(8)]
            flags = other if j % 2 else 0
            cases.append({"a": a, "T": T, "flags": flags, "want": flat(model_line(loop, a, T, False))})
            if j % 3 == 1:
                dup, flags = ops_a[j - 1], own | (other if j % 2 == 0 else 0)
                cases.append({"a": dup, "T": [rng.randrange(2 * P) for _ in range(8)], "flags": flags, "want": flat(dup)})
    elif op == "PROD2":
        lines = line_constants(rng)
        for pts in point_sets(rng):
            cases.append({"a": const_elem(0, 0), "pts": pts, "want": model_prod2(lines, pts)})
    elif op == "ROUND":
        lines = line_constants(rng)
        trail = g.miller_round_bounds()[-1]                            # what a round's last line leaves the next squaring at most
        assert trail[0] <= RE_MAX and trail[1] <= IM_MAX
        ops_a = [const_elem(RE_MAX, IM_MAX), const_elem(*trail)] + miller_operands(rng)[1:11]
        for j, (a, pts) in enumerate(zip(ops_a, point_sets(rng))):
            flags = j % 4                                              # all four (skip1, skip2), case 0 runs both lines
            cases.append({"a": a, "pts": pts, "flags": flags, "want": flat(model_round(a, lines, pts, flags))})
    elif op == "CSQR":
        f = bls.miller_loop(bls.g1_mul(bls.G1_GEN, 777), bls.g2_mul(bls.G2_GEN, 3))          # as gen_six_tables.self_check
        t = bls.f12_mul(bls.f12_conj(f), bls.f12_inv(f))
        t = bls.f12_mul(bls.f12_frob(bls.f12_frob(t)), t)
        top = V_MUL * P - 1
        elems = [a for a, _ in mul_operands(rng, V_MUL)[:5]]
        elems.insert(CSQR_LONG - 1, [(c0 + (V_MUL - 1) * P, c1 + (V_MUL - 1) * P) for c0, c1 in mont(t)])    # cyclotomic, just below 6p
        elems += [g.spread(rng, mont(t), V_MUL), g.spread(rng, mont(bls.f12_sqr(t)), V_MUL)]
        elems += [with_value(rng, V_MUL, (5 * j) % 12, v) for j, v in enumerate((0, P, top))]
        elems += [elem(rng, V_MUL) for _ in range(8)]
        for j, a in enumerate(elems):
            x, chain, trace = a, {}, []
            for n in range(1, (CSQR_RUNS[-1] if j < CSQR_LONG else CSQR_RUNS[3]) + 1):
                x = csqr_step(x, trace)                                # every squaring of the run hands the fold its inputs
                if n in CSQR_RUNS:
                    chain[n] = flat(x)
            cases.append({"a": a, "want": chain, "fold_inputs": trace})
    elif op == "CONJ":
        top = V_CONJ * P - 1
        ops_a = [const_elem(top, top), const_elem(0, 0), const_elem(top, 0), const_elem(0, top)] + [elem(rng, V_CONJ) for _ in range(8)]
        for a in ops_a:
            cases.append({"a": a, "want": flat(model_conj(a))})
    elif op in ("FROB", "INV"):
        top = V_CONJ * P - 1
        ops_a = [const_elem(top, top), const_elem(0, 0), const_elem(P, 2 * P), const_elem(top, 0), [(MONT1, 0)] + [(0, 0)] * 5]
        ops_a += [with_value(rng, V_CONJ, (5 * j) % 12, v) for j, v in enumerate((0, 1, P - 1, P + 1, top))]
        ops_a += [elem(rng, V_CONJ) for _ in range(8)]
        for a in ops_a:
            x = unmont(a)
            zero = all(v == 0 for v in flat(x))
            if op == "FROB":
                cases.append({"a": a, "want": flat(mont(bls.f12_frob(x)))})
            else:
                cases.append({"a": a, "ok": 0 if zero else 1, "want": [0] * 12 if zero else flat(mont(bls.f12_inv(x)))})
    elif op == "FOLD":
        low = sum(g.FOLD_LIMB_MAX << (28 * i) for i in range(13))
        vecs = [[g.FOLD_LIMB_MAX] * 13 + [(32 * P - 1 - low) >> 364]]                       # every lower limb at 2^31 - 1
        vecs += g.uncarried_forms(32 * P - 1, rng)
        vecs += g.uncarried_forms(limbs_all_max(32 * P), rng)[:2]                            # max form: limb 0 = 2^31 - 1
        by_sign = {0: [], 1: []}
        for c in table("CSQR")["cases"]:
            for k, h in c["fold_inputs"]:
                by_sign[k & 1].append(h)
        vecs += [max(by_sign[0], key=g.limbs_val), max(by_sign[1], key=g.limbs_val)]        # the squaring's largest 3 r + 13p - 2g, 3 r + 2g
        for v in [k * P + d for k in range(33) for d in (-1, 0, 1) if 0 <= k * P + d < 32 * P]:
            vecs += g.uncarried_forms(v, rng)[:3]                                            # carried, every lower limb at its maximum, random
        while len(vecs) % 12 or len(vecs) < 12 * 34:
            vecs.append(g.uncarried_forms(rng.randrange(32 * P), rng)[rng.randrange(4)])
        for j in range(0, len(vecs), 12):
            cases.append({"a": vecs[j:j + 12], "want": [g.fold(l) for l in vecs[j:j + 12]]})
    else:
        raise KeyError(op)
    return {"cases": cases, "lines": lines}


# ------------------------------------------------------------------------------------------------ positions
def launches(n_cases, sizes=SIZES):
    """[(n_groups, [case per group])]: case 0 - the hardest - in group 0, in group 9 (the one lanes 60..63 shadow) and in the lone group
    of a trailing wave; every other group takes the next case of the table, so that the groups of a block hold distinct cases
    (a table shorter than a block's free groups repeats) and the launches together run every case"""
    out, nxt = [], 0
    for n in sizes:
        order = []
        for grp in range(n):
            if grp in (0, 9) or (grp == n - 1 and n % 10 == 1) or n_cases == 1:
                order.append(0)
            else:
                order.append(1 + nxt % (n_cases - 1))
                nxt += 1
        out.append((n, order))
    return out


def kara_columns(terms, s):
    """the exact integer columns of a Karatsuba call before they meet a 64-bit register: (U - V, W) - for the host test's claims
    that some real part's columns go negative and some W column passes 2^64"""
    U, V, W = [0] * 28, [0] * 28, [0] * 28
    for x0, y0, x1, y1 in terms:
        for i in range(14):
            for j in range(14):
                U[i + j] += s[x0][i] * s[y0][j]
                V[i + j] += s[x1][i] * s[y1][j]
                W[i + j] += (s[x0][i] + s[x1][i]) * (s[y0][j] + s[y1][j])
    return [u - v for u, v in zip(U, V)], W
