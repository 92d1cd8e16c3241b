"""A host model of the multi-term MSM ladder (csrc/h2v_msm.hpp: msm_multi_body, msm_multi_ladder) in plain Python integers.

What it mirrors, as the kernel stands:
  * the deal: half hh = 2 term + glv_half of a proof goes to lane hh // hpl, slot hh % hpl;
  * halves at term >= T, with a zero scalar or with an infinity base are unused - all their digits are zero;
  * bls12_381.glv_split (k = k1 + k2 lambda) and the signed 4-bit recoding of msm_recode4: 33 digits in [-8, 8], least significant
    first, the carry as digit 32;
  * the walk: windows 32 down to 0, four doublings between windows once the accumulator is set, the slots in order; the first
    non-zero digit sets the accumulator, every later one is an addition.

Bases are given by their discrete logs (B_t = [b_t] G, None: the point at infinity), so the accumulator is a number modulo r and
an addition of the entry e is a DOUBLING event when acc == e and an INVERSE event when acc == -e: the two cases the unchecked
addition of the kernel gets wrong (Z = 0), which the Z test at the end of the ladder has to catch and the complete redo to repair.
phi(P) = [lambda] P, so the entry of digit d in a slot of half h of term t is d lambda^h b_t.

craft() puts such an event where a test wants it: with the other logs known, the accumulator in front of slot (window, slot) is
c + sum_u x_u b_u, linear in the logs b_u still to be chosen, and each wanted event is one linear equation in them modulo r.

What cannot be built, and why (craft raises, cases() never asks for it): an event needs two DIFFERENT terms in the accumulator and
the entry.  With one term alone the equation is (a -+ d) + b lambda = 0 mod r in the signed prefixes, which the GLV lattice
excludes - the argument the one-term ladders rest on.  So there is no event in a lane that holds halves of one term only (at
T = 11 the partly filled last lane of 3, 4, 5 and 7 halves per lane), none in window 32 at slot 1 of a lane that starts on a k1
half (slots 0 and 1 are one term; the earliest is slot 2), and where a lane holds fewer than three terms (3 and 4 halves per
lane) neither an unused slot 0 in front of an event nor two events in one lane: two crafted logs with no known term beside them
make the two equations homogeneous."""
import random
from dataclasses import dataclass, field

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

R = bls.R
LAM = bls.GLV_LAMBDA
MAX_HALVES = 8
WINDOWS = 33
assert (LAM * LAM + LAM + 1) % R == 0


# ----------------------------------------------------------------------------- the deal
def shape(T, tpl, forced):
    """(halves per lane, lanes per proof) of the multi-term launch: csrc/h2v_msm_shape.hpp, msm_multi_shape"""
    lpp0 = -(-T // tpl)
    hpl = 2 * tpl if forced else -(-2 * T // lpp0)
    return hpl, -(-2 * T // hpl)


def lanes_per_proof(T, hpl):
    return -(-2 * T // hpl)


def lane_slots(T, hpl, lane):
    """[(term, glv_half)] of the lane's hpl slots; term >= T: a slot behind the proof's last half"""
    return [((lane * hpl + j) >> 1, (lane * hpl + j) & 1) for j in range(hpl)]


def lane_terms(T, hpl, lane):
    """the different terms (< T) a lane holds halves of, in slot order"""
    out = []
    for t, _ in lane_slots(T, hpl, lane):
        if t < T and t not in out:
            out.append(t)
    return out


def last_used_slot(T, hpl, lane):
    return max(j for j, (t, _) in enumerate(lane_slots(T, hpl, lane)) if t < T)


def recode4(k):
    """msm_recode4 on a 128-bit half: 33 signed digits, least significant first"""
    assert 0 <= k < 1 << 128
    dg, carry = [], 0
    for q in range(32):
        d = ((k >> (4 * q)) & 15) + carry
        carry = 1 if d > 8 else 0
        dg.append(d - 16 if carry else d)
    dg.append(carry)
    assert sum(d << (4 * q) for q, d in enumerate(dg)) == k
    return dg


def lane_digits(scalars, logs, hpl, lane):
    """per slot (term, glv_half, digits); unused slots carry 33 zeros"""
    T = len(scalars)
    out = []
    for t, h in lane_slots(T, hpl, lane):
        use = t < T and scalars[t] % R != 0 and logs[t] is not None
        out.append((t, h, recode4(bls.glv_split(scalars[t])[h]) if use else [0] * WINDOWS))
    return out


def _walk(digits):
    """(window, slot, digit) of every non-zero digit in the order the ladder meets them"""
    for q in range(WINDOWS - 1, -1, -1):
        for j, (_, _, dg) in enumerate(digits):
            if dg[q]:
                yield q, j, dg[q]


# ----------------------------------------------------------------------------- the events of a lane
def events(scalars, logs, hpl, lane):
    """([(window, slot, "dbl" | "inv")], the lane's true sum as a multiple of G).  The first event is what the unchecked ladder
    meets; all of them are what the complete redo meets (after an "inv" the accumulator is the point at infinity: the next
    non-zero digit restarts it, which is no event)."""
    digits = lane_digits(scalars, logs, hpl, lane)
    acc, is_set, last_q, found = 0, False, WINDOWS - 1, []
    for q, j, d in _walk(digits):
        t, h, _ = digits[j]
        if is_set:
            acc = acc * pow(16, last_q - q, R) % R
        last_q = q
        e = d * (LAM if h else 1) * logs[t] % R
        assert e != 0
        if not is_set:
            acc, is_set = e, True
            continue
        if acc == e:
            found.append((q, j, "dbl"))
        elif (acc + e) % R == 0:
            found.append((q, j, "inv"))
        acc = (acc + e) % R
    if is_set:
        acc = acc * pow(16, last_q, R) % R
    return found, acc


def _solve(rows, rhs):
    """x with rows x = rhs modulo r (Gauss-Jordan); None: singular"""
    k = len(rows)
    m = [list(r) + [v] for r, v in zip(rows, rhs)]
    for c in range(k):
        p = next((i for i in range(c, k) if m[i][c] % R), None)
        if p is None:
            return None
        m[c], m[p] = m[p], m[c]
        inv = pow(m[c][c], R - 2, R)
        m[c] = [v * inv % R for v in m[c]]
        for i in range(k):
            if i != c and m[i][c]:
                f = m[i][c]
                m[i] = [(a - f * b) % R for a, b in zip(m[i], m[c])]
    return [m[i][k] for i in range(k)]


def _equations(scalars, logs, hpl, targets, unknown):
    """the linear system of `targets` in the logs of the terms `unknown`; None where a target has a zero digit or meets an
    accumulator that is not yet set"""
    rows, rhs = [], []
    for lane in sorted({t[0] for t in targets}):
        mine = {(q, j): kind for ln, q, j, kind in targets if ln == lane}
        digits = lane_digits(scalars, [1 if t in unknown else b for t, b in enumerate(logs)], hpl, lane)
        c, x, is_set, last_q = 0, [0] * len(unknown), False, WINDOWS - 1
        for q, j, d in _walk(digits):
            t, h, _ = digits[j]
            if is_set:
                f = pow(16, last_q - q, R)
                c, x = c * f % R, [v * f % R for v in x]
            last_q = q
            m = d * (LAM if h else 1) % R
            kind = mine.pop((q, j), None)
            if kind is not None:
                if not is_set:
                    return None
                # acc = +m b_t (dbl) or -m b_t (inv)
                row = list(x)
                row[unknown.index(t)] = (row[unknown.index(t)] - (m if kind == "dbl" else -m)) % R
                rows.append(row)
                rhs.append(-c % R)
            if t in unknown:
                x[unknown.index(t)] = (x[unknown.index(t)] + m) % R
            else:
                c = (c + m * logs[t]) % R
            is_set = True
        if mine:
            return None     # a target on a zero digit
    return rows, rhs


def craft(scalars, logs, hpl, targets, rng, pinned=None, tries=20000):
    """(scalars, logs) with the logs of the target slots' terms chosen so that every target (lane, window, slot, kind) is an event
    of its lane.  Where a target's digit is zero, the accumulator is still unset there or the system is singular, the scalars of
    the targets' lanes are drawn again (those of `pinned` terms, {term: draw(rng)}, by their own rule; never zero scalars or those
    of infinity bases), at most `tries` times; then it raises: a target is never skipped."""
    T = len(scalars)
    pinned = pinned or {}
    scalars, logs = list(scalars), list(logs)
    unknown = []
    for lane, q, j, kind in targets:
        t = lane_slots(T, hpl, lane)[j][0]
        if t >= T or t in unknown or kind not in ("dbl", "inv") or not 0 <= q < WINDOWS:
            raise ValueError("bad target %r" % ((lane, q, j, kind),))
        if logs[t] is None or scalars[t] % R == 0:
            raise ValueError("the term of target %r is not free" % ((lane, q, j, kind),))
        unknown.append(t)
    free = sorted({t for lane, _, _, _ in targets for t in lane_terms(T, hpl, lane)
                   if logs[t] is not None and scalars[t] % R != 0 and t not in pinned})
    for _ in range(tries):
        eq = _equations(scalars, logs, hpl, targets, unknown)
        sol = _solve(*eq) if eq else None
        known = {b for t, b in enumerate(logs) if t not in unknown}
        if sol is not None and all(sol) and len(set(sol)) == len(sol) and not set(sol) & known:
            for t, b in zip(unknown, sol):
                logs[t] = b
            for lane, q, j, kind in targets:
                assert (q, j, kind) in events(scalars, logs, hpl, lane)[0]
            return scalars, logs
        for t in free:
            scalars[t] = rng.randrange(1, R)
        for t, draw in pinned.items():
            scalars[t] = draw(rng)
    raise ValueError("no scalars found for the targets %r at %d halves per lane, %d terms" % (targets, hpl, T))


# ----------------------------------------------------------------------------- the cases
# honest bases: a chain of running additions with a known step, the same for every case (term t takes POOL_LOGS[t])
POOL_B0 = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R
POOL_STEP = 0x0123456789ABCDEFFEDCBA98765432100123456789ABCDEFFEDCBA9876543211 % R
POOL_SIZE = 16
POOL_LOGS = [(POOL_B0 + i * POOL_STEP) % R for i in range(POOL_SIZE)]
_pool_points = []


def pool_points():
    if not _pool_points:
        p, step = bls.g1_mul(bls.G1_GEN, POOL_B0), bls.g1_mul(bls.G1_GEN, POOL_STEP)
        for _ in range(POOL_SIZE):
            _pool_points.append(p)
            p = bls.g1_add(p, step)
    return _pool_points


@dataclass
class Case:
    name: str
    hpl: int
    scalars: list
    logs: list                                    # None: the point at infinity
    targets: list = field(default_factory=list)   # (lane, window, slot, kind); empty: an honest case
    control_of: str = None                        # an honest control: the crafted case whose scalars it shares

    @property
    def T(self):
        return len(self.scalars)

    @property
    def honest(self):
        return not self.targets

    def events(self, lane):
        return events(self.scalars, self.logs, self.hpl, lane)

    def crafted_lanes(self):
        return sorted({t[0] for t in self.targets})

    def sum_log(self):
        return sum(s * b for s, b in zip(self.scalars, self.logs) if b is not None) % R

    @property
    def sum_is_infinity(self):
        return self.sum_log() == 0

    def points(self):
        """the bases: pool points where the log is the pool's, one scalar multiplication per crafted base"""
        pool = pool_points()
        return [None if b is None else pool[t] if b == POOL_LOGS[t] else bls.g1_mul(bls.G1_GEN, b) for t, b in enumerate(self.logs)]


FULL_T = 11
FULL_WINDOWS = (32, 31, 16, 1, 0)
OTHER_WINDOWS = (32, 16, 0)


def eventful_lanes(T, hpl):
    """lanes in which two different terms meet: the only ones that can hold an event"""
    return [ln for ln in range(lanes_per_proof(T, hpl)) if len(lane_terms(T, hpl, ln)) >= 2]


def earliest_slot(T, hpl, lane, window):
    """the first slot an event can fall on: slot 1, but in window 32 - where nothing older is in the accumulator - the first
    slot whose term differs from slot 0's"""
    slots = lane_slots(T, hpl, lane)
    if window < WINDOWS - 1:
        return 1
    return next(j for j, (t, _) in enumerate(slots) if t != slots[0][0])


def single_targets(T, hpl):
    """(lane, window, slot, kind) of the single-event cases.  Lanes: the first, a middle one (for odd hpl one that starts on a k2
    half, so that its slot 1 follows a k2 half in slot 0) and the last in which two terms meet (the partly filled last lane where
    it holds two terms).  Slots: the earliest, a middle one, the last used one."""
    ev = eventful_lanes(T, hpl)
    if not ev:
        return []
    lanes = [ev[0]]
    if T == FULL_T:
        mid = [ln for ln in ev[1:-1] if (ln * hpl) & 1 == hpl & 1] or ev[1:-1]
        lanes.append(mid[len(mid) // 2])
    if ev[-1] not in lanes:
        lanes.append(ev[-1])
    out = []
    for kind in ("dbl", "inv"):
        for q in (FULL_WINDOWS if T == FULL_T else OTHER_WINDOWS):
            for ln in lanes:
                first, last = earliest_slot(T, hpl, ln, q), last_used_slot(T, hpl, ln)
                slots = [first, last] if T != FULL_T else [first, (first + last) // 2, last]
                for j in sorted(set(slots)):
                    out.append((ln, q, j, kind))
    return out


def _lonely_lane_scalars(T, hpl, scalars, rng):
    """for a proof whose every lane is to sum to infinity: a lane with halves of one term only cannot cancel, so its halves are
    made to vanish - a term wholly inside it gets the scalar 0, a term whose k2 half alone is in it a scalar below lambda.
    Returns {term: how to draw its scalar again}."""
    pinned = {}
    for ln in range(lanes_per_proof(T, hpl)):
        terms = lane_terms(T, hpl, ln)
        if len(terms) != 1:
            continue
        t = terms[0]
        halves = [h for tt, h in lane_slots(T, hpl, ln) if tt == t]
        if halves == [0, 1]:
            pinned[t] = lambda rng: 0
        elif halves == [1]:
            pinned[t] = lambda rng: rng.randrange(1, LAM)
        else:
            raise ValueError("a lane that holds a k1 half alone")
        scalars[t] = pinned[t](rng)
    return pinned


def _unused_case(T, hpl, scalars, logs):
    """zero scalars and infinity bases in the slots in front of an event, slot 0 among them: in lanes of three or more terms all
    but the last two become unused, alternately by a zero scalar and by an infinity base, until both kinds occur; the event falls
    on the first slot of the lane's last term.  None where no lane has the room for both kinds."""
    targets, crafted, kinds = [], set(), []
    for ln in range(lanes_per_proof(T, hpl)):
        terms = lane_terms(T, hpl, ln)
        if len(terms) < 3 or set(terms) & crafted or set(kinds) == {"zero", "inf"}:
            continue
        if any(scalars[t] == 0 or logs[t] is None for t in terms):
            continue
        for t in terms[:-2]:
            kind = "inf" if kinds and kinds[-1] == "zero" else "zero"
            kinds.append(kind)
            if kind == "zero":
                scalars[t] = 0
            else:
                logs[t] = None
        slot = next(j for j, (t, _) in enumerate(lane_slots(T, hpl, ln)) if t == terms[-1])
        targets.append((ln, 16, slot, "inv" if len(targets) & 1 else "dbl"))
        crafted.add(terms[-1])
    return targets if set(kinds) == {"zero", "inf"} else None


def cases(hpl, T):
    """The crafted cases of (hpl, T), each followed at the end of the list by its honest control (the same scalars, pool logs),
    and three plain honest cases.  T = 11 gets the whole list; another T the single events in windows 32, 16 and 0 at the earliest
    and the last slot of the first and the last eventful lane, and the two last-addition cases."""
    assert 3 <= hpl <= MAX_HALVES and 1 <= T <= POOL_SIZE
    out = []

    def add(name, targets, prepare=None):
        rng = random.Random("multi-ladder/%d/%d/%s" % (hpl, T, name))
        scalars, logs, pinned = [rng.randrange(1, R) for _ in range(T)], list(POOL_LOGS[:T]), {}
        if prepare:
            got = prepare(scalars, logs, rng)
            if got is None:
                return
            targets, pinned = got
        scalars, logs = craft(scalars, logs, hpl, targets, rng, pinned)
        out.append(Case(name, hpl, scalars, logs, list(targets)))

    for ln, q, j, kind in single_targets(T, hpl):
        add("%s-w%d-lane%d-slot%d" % (kind, q, ln, j), [(ln, q, j, kind)])
    ev = eventful_lanes(T, hpl)
    if ev:
        mid = ev[len(ev) // 2]
        # the event on the very last addition: the lane's sum is the point at infinity, and Z = 0 has nothing left to inherit it
        add("inv-last-addition-lane%d" % mid, [(mid, 0, last_used_slot(T, hpl, mid), "inv")])
        add("inv-last-addition-every-lane", None,
            lambda s, b, rng: ([(ln, 0, last_used_slot(T, hpl, ln), "inv") for ln in ev], _lonely_lane_scalars(T, hpl, s, rng)))
    if ev and T == FULL_T:
        mid = ev[len(ev) // 2]
        last = last_used_slot(T, hpl, mid)
        # through the true point at infinity in the middle of the ladder: the redo restarts from an entry and goes on
        add("restart-w16-lane%d" % mid, [(mid, 16, last, "inv")])
        # two events in one lane need two crafted terms and a third, known one (with two terms alone the two equations are
        # homogeneous in the two logs): the first slot of the lane's second term and the last used slot, in a lane of three terms
        wide = [ln for ln in ev if len(lane_terms(T, hpl, ln)) >= 3]
        if wide:
            ln = wide[len(wide) // 2]
            second = lane_terms(T, hpl, ln)[1]
            first = next(j for j, (t, _) in enumerate(lane_slots(T, hpl, ln)) if t == second)
            add("two-events-lane%d" % ln, [(ln, 20, first, "dbl"), (ln, 5, last_used_slot(T, hpl, ln), "inv")])
        add("unused-slots-before-the-event", None,
            lambda s, b, rng: (lambda tg: None if tg is None else (tg, {}))(_unused_case(T, hpl, s, b)))
    controls = [Case("honest:" + c.name, hpl, list(c.scalars), [None if b is None else POOL_LOGS[t] for t, b in enumerate(c.logs)],
                     control_of=c.name) for c in out]
    rng = random.Random("multi-ladder/%d/%d/plain" % (hpl, T))
    plain = [Case("honest-plain", hpl, [rng.randrange(1, R) for _ in range(T)], list(POOL_LOGS[:T])),
             Case("honest-zero-scalar", hpl, [0] + [rng.randrange(1, R) for _ in range(T - 1)], list(POOL_LOGS[:T])),
             Case("honest-infinity-base", hpl, [rng.randrange(1, R) for _ in range(T)], list(POOL_LOGS[:T - 1]) + [None])]
    return out + controls + plain


def gpu_shapes(hpl):
    """the term counts the device test runs at `hpl` halves per lane: 11 (three or more lanes, a partly filled last one; for odd
    hpl terms that straddle two lanes), the full-last-lane shape, and the one-lane-per-proof shape (the largest T with 2 T <= hpl)"""
    full = {3: 12, 4: 12, 5: 10, 6: 12, 7: 7, 8: 12}[hpl]
    assert 2 * full % hpl == 0 and 2 * FULL_T % hpl != 0 and lanes_per_proof(FULL_T, hpl) >= 3
    return [FULL_T, full, hpl // 2]
