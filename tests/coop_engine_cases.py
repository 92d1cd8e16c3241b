"""Case tables for single calls of the cooperative pairing engine (csrc/h2v_pairing_coop.hpp; device probe h2v_probe_coop_call) in
its four shapes: operands that sit ON the bounds the engine's headroom note states, and for each what the limb model of
tests/coop_engine_model.py yields - the model alone must stay inside its own assertions on every case, which is the condition on the
inputs.  Shared by the device test (tests/test_coop_engine_calls_gpu.py: exact comparison, limb for limb) and the host test
(tests/test_coop_engine_model.py: residues and bounds of the same cases).

cases(op) is the op's list of inputs, the same for every shape, case 0 the hardest; a case is a dict:
  a      12 integer representatives, flat order 2k + part                       b      12 integers (MUL)
  T      4 integers, the loop's own T slots (LINE1 / LINE2)     pts    4 integers PX1, PY1, PX2, PY2     flags  bit 0 skip1, bit 1 skip2
expected(op, shape, case index, line set, run length) is what the model returns for it: (12 integers - PROD: the 8 T slots; FROB / INV:
residues -, the spare lanes' four T slots or None, ok).  A result is carried, so its limb vector and its integer determine each other:
limbs(want) is what the device must return.  LINE_SETS are the launch's line constants: (loop 1's line 0, line 1, loop 2's line 0)."""
import functools
import random

from tests import coop_engine_model as M
from plutus_halo2_verifier_gen_amd import bls12_381 as bls

P, R, MONT1 = M.P, M.R, M.MONT1
ct = M.ct
OPS = ("MUL", "SQR", "CSQR", "LINE1", "LINE2", "PROD", "ROUND", "CONJ", "FROB", "INV")
SHAPES = ("normal", "wide", "narrow", "twelve")
CSQR_RUNS = (1, 2, 3, 9, 16, 32)
CSQR_LONG = 4                        # elements that take the runs of 16 and 32 (the last of them cyclotomic)
TOP6, TOP5 = 6 * P - 1, 5 * P - 1
PMAX = M.limbs_all_max(P)            # the largest canonical value whose lower limbs are all 2^28 - 1


def cyclotomic():
    """an element of the cyclotomic subgroup (plain residues), as tools/gen_coop_tables.py's self check builds it"""
    f = bls.miller_loop(bls.g1_mul(bls.G1_GEN, 777), bls.g2_mul(bls.G2_GEN, 3))
    t = bls.f12_mul(bls.f12_conj(f), bls.f12_inv(f))
    return bls.f12_mul(bls.f12_frob(bls.f12_frob(t)), t)


def operands(rng, v):
    """every coefficient at v p - 1; at all-lower-limbs-max below v p; 0, the Montgomery one, p - 1; the twelve spikes; random"""
    top = v * P - 1
    out = [[top] * 12, [M.limbs_all_max(v * P)] * 12, [0] * 12, [MONT1] * 12, [P - 1] * 12]
    out += [[top if g == j else 0 for g in range(12)] for j in range(12)]
    out += [[rng.randrange(v * P) for _ in range(12)] for _ in range(4)]
    return out


@functools.lru_cache(maxsize=None)
def line_sets():
    rng = random.Random(0xc00b)
    rp = lambda: rng.randrange(P)
    consistent = lambda: ct.line_consts((rp(), rp()), (rp(), rp()))            # [nl0, nl1, nxl0, nxl1, c0, c1, xc0, xc1], linear: holds on Montgomery forms
    return (([P - 1] * 8, [P - 1] * 8, [P - 1] * 8), ([PMAX] * 8, [PMAX] * 8, [PMAX] * 8), (consistent(), consistent(), consistent()),
            ([0, MONT1, P - 1, rp(), PMAX, 0, MONT1, rp()], [rp() for _ in range(8)], [MONT1, rp(), 0, P - 1, rp(), PMAX, rp(), 0]))


def point_sets(rng):
    rp = lambda: rng.randrange(P)
    out = [(P - 1,) * 4, (PMAX,) * 4, (0,) * 4, (MONT1,) * 4]
    out += [tuple(rp() for _ in range(4)) for _ in range(4)]
    out += [(0, rp(), rp(), P - 1), (P - 1, 0, MONT1, rp()), (rp(), PMAX, 0, P - MONT1), (P - MONT1, MONT1, P - 1, 0)]
    return out


def t_max():
    """the largest value a T slot takes from the model's own products, over the shapes: one reduced product of canonical operands"""
    s = {0: M.limbs(P - 1), 1: M.limbs(PMAX)}
    return max(M.lane_value([(x, y)], s, 1) for x in (0, 1) for y in (0, 1))


@functools.lru_cache(maxsize=None)
def cases(op):
    rng = random.Random(0xc0 + OPS.index(op))
    out = []
    if op == "MUL":
        ops = operands(rng, 6)
        pairs = [(x, x) for x in ops[:5]] + [(ops[0], ops[1]), (ops[2], ops[0])]
        pairs += [(ops[5 + j], ops[5 + (7 * j + 3) % 12]) for j in range(12)]                 # a spike against another coefficient's spike
        pairs += [(ops[5 + j], ops[j % 2]) for j in range(0, 12, 3)] + [(ops[j % 2], ops[5 + j]) for j in range(1, 12, 3)]
        pairs += [(ops[17 + j], ops[17 + (j + 1) % 4]) for j in range(4)]
        out = [{"a": a, "b": b} for a, b in pairs]
    elif op == "SQR":
        out = [{"a": a} for a in operands(rng, 6)]
    elif op == "CSQR":
        t = M.mont(cyclotomic())
        ops = operands(rng, 6)
        elems = ops[:CSQR_LONG - 1] + [[c + 5 * P for c in t]] + ops[CSQR_LONG - 1:]           # cyclotomic, just below 6p
        elems.append([c + rng.randrange(6) * P for c in M.mont(bls.f12_sqr(cyclotomic()))])
        out = [{"a": a} for a in elems]
    elif op in ("LINE1", "LINE2", "ROUND"):
        pts, tm = point_sets(rng), t_max()
        t_sets = [[tm] * 4, [0] * 4, [2 * P - 1] * 4, [P] * 4]
        for j, a in enumerate(operands(rng, 6)):
            c = {"a": a, "pts": pts[j % len(pts)], "flags": j % 4}                           # all four (skip1, skip2); case 0 runs both lines
            if op != "ROUND":
                c["T"] = t_sets[j] if j < len(t_sets) else [rng.randrange(2 * P) for _ in range(4)]
            out.append(c)
    elif op == "PROD":
        out = [{"a": [0] * 12, "pts": p} for p in point_sets(rng)]
    elif op == "CONJ":
        out = [{"a": a} for a in operands(rng, 5)]
    elif op == "FROB":
        out = [{"a": a} for a in operands(rng, 6)]
    elif op == "INV":
        ops = operands(rng, 5)
        ops.insert(3, [P, 2 * P, 0, 4 * P] * 3)                                                # zero, spelled with multiples of p
        ops.append([MONT1] + [0] * 11)                                                         # one
        out = [{"a": a} for a in ops]
    else:
        raise KeyError(op)
    return out


@functools.lru_cache(maxsize=None)
def _csqr_chain(nq, k):
    """the model's squaring run of case k: {run length: 12 integers}"""
    x, chain = cases("CSQR")[k]["a"], {}
    for n in range(1, (CSQR_RUNS[-1] if k < CSQR_LONG else CSQR_RUNS[3]) + 1):
        x = M.model_csqr(x, nq)
        if n in CSQR_RUNS:
            chain[n] = x
    return chain


@functools.lru_cache(maxsize=None)
def _expected(op, nq, twelve, k, ls, run):
    c = cases(op)[k]
    l1_0, l1_1, l2_0 = line_sets()[ls] if ls is not None else (None, None, None)
    shape = "twelve" if twelve else {1: "narrow", 2: "normal", 4: "wide"}[nq]
    if op == "MUL":
        return M.model_mul(c["a"], c["b"], nq), None, 1
    if op == "SQR":
        return M.model_sqr(c["a"], nq), None, 1
    if op == "CSQR":
        return _csqr_chain(nq, k)[run], None, 1
    if op in ("LINE1", "LINE2"):
        loop = 1 if op == "LINE1" else 2
        r, spare = M.model_line(loop, c["a"], c["T"], l1_0, l2_0, c["pts"], nq, spare=not twelve)
        return (list(c["a"]) if c["flags"] & loop else r), spare, 1
    if op == "PROD":
        return M.model_prod(l1_0, l2_0, c["pts"]), None, 1
    if op == "ROUND":
        r, spare = M.model_round(c["a"], l1_0, l1_1, l2_0, c["pts"], c["flags"], shape)
        return r, spare, 1
    if op == "CONJ":
        return M.model_conj(c["a"]), None, 1
    x = M.unmont(c["a"])
    if op == "FROB":
        return M.mont(bls.f12_frob(x)), None, 1
    zero = all(v == 0 for pair in x for v in pair)
    return (None if zero else M.mont(bls.f12_inv(x))), None, 0 if zero else 1


def expected(op, shape, k, ls=None, run=0):
    if op not in ("LINE1", "LINE2", "PROD", "ROUND"):
        ls = None
    return _expected(op, M.SHAPES[shape], shape == "twelve", k, ls, run if op == "CSQR" else 0)


def launches(shape, n_cases):
    """[(n_groups, [case per group], line set)]: 1, G, G + 1 and 2G + 1 groups (G groups per wave), then launches of 2G + 1 (wide: 9) until every
    case has run.  Case 0 - the hardest - sits in group 0, in the last group of a full first wave and in the lone group of a trailing
    wave; every other group takes the next case of the table, so that the groups of a launch hold distinct cases.  The line sets take
    turns."""
    G = M.GROUPS_PER_WAVE[shape]
    out, nxt, sizes = [], 0, [1, G, G + 1, 2 * G + 1]
    while True:
        n = sizes[len(out)] if len(out) < len(sizes) else (2 * G + 1 if G > 1 else 9)
        order = []
        for grp in range(n):
            if grp == 0 or (grp == G - 1 and n >= G) or (grp == n - 1 and grp % G == 0) or n_cases == 1:
                order.append(0)
            else:
                order.append(1 + nxt % (n_cases - 1))
                nxt += 1
        out.append((n, order, len(out) % len(line_sets())))
        if len(out) >= len(sizes) and nxt >= n_cases - 1:
            return out
