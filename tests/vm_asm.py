"""A small assembler for hand-written programs of the transcript + Fr-combiner VM, and the programs and batches the VM tests
share (tests/test_vm_programs.py checks them on the CPU, tests/test_vm_programs_gpu.py runs them through h2v_probe_vm).

The programs are data: `assemble` pads the bundles it is given with OP_NOP, appends the END bundle, runs plan.check_bundles
and returns a copy of a skeleton plan (compile_plan(simple_mul_vk()): proof_len 1120, 3 public inputs, 10 points, 16 terms)
with the program swapped in.  The tests choose which lane executes which record - the project's scheduler is not used: lane
placement is what is being tested.  Everything here is plain integers and hashlib; nothing touches a device."""
import dataclasses
import random

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from plutus_halo2_verifier_gen_amd import plan as PL

R = bls.R
NOP = (PL.OP_NOP, 0, 0, 0)
END = (PL.OP_END, 0, 0, 0)
# the status bits the interpreter sets (include/h2v.h) by run_plan's reason
ST_BAD_SCALAR, ST_INVERSE_OF_ZERO, ST_SHORT_PROOF, ST_RECURSION = 1, 2, 4, 32
ST_OF = {"scalar": ST_BAD_SCALAR, "inverse": ST_INVERSE_OF_ZERO, "short": ST_SHORT_PROOF, "recursion": ST_RECURSION}
PROOF_LEN, N_PI, N_TERMS = 1120, 3, 16
BLAKE_KEY = b"vm program tests"

_skeleton = None


def skeleton():
    global _skeleton
    if _skeleton is None:
        from plutus_halo2_verifier_gen_amd import vk as V
        _skeleton = PL.compile_plan(V.simple_mul_vk()[0])
        assert (_skeleton.proof_len, _skeleton.n_pi, len(_skeleton.points), _skeleton.n_terms) == (PROOF_LEN, N_PI, 10, N_TERMS)
    return _skeleton


def _pad(bundles, L):
    out = []
    for bun in list(bundles) + [[END]]:
        assert 1 <= len(bun) <= L, "a bundle has at most L records"
        out.extend(list(bun) + [NOP] * (L - len(bun)))
    PL.check_bundles(out, L)
    return out


def _regs_used(instrs):
    top = 0
    for rec in instrs:
        for reg in PL._uses(*rec):
            top = max(top, reg)
        if PL._defines(rec[0]):
            top = max(top, rec[1])
    return top + 1


def assemble(bundles, L, consts=(), n_regs=None, trace=(), wide=None, transcript_kind=PL.TR_CARDANO_BLAKE2B_256,
             transcript_key=b"", n_ci=0):
    """bundles: lists of at most L records (op, dst, a, b), record j of a bundle runs on lane j (NOP = that lane idles).
    wide: (lanes, bundles[, n_regs]) of a second schedule.  trace: (slot id, register) pairs of the narrow schedule."""
    instrs = _pad(bundles, L)
    n_regs = n_regs or _regs_used(instrs)
    assert n_regs >= _regs_used(instrs)
    wide_out = None
    if wide is not None:
        w_instrs = _pad(wide[1], wide[0])
        wide_out = (wide[0], wide[2] if len(wide) > 2 else _regs_used(w_instrs), w_instrs)
    n_sq = sum(1 for rec in instrs if rec[0] == PL.OP_SQUEEZE)
    return dataclasses.replace(skeleton(), instrs=instrs, consts=list(consts) or [0], n_regs=n_regs, vm_lanes=L, wide=wide_out,
                               trace=list(trace), transcript_kind=transcript_kind, transcript_key=bytes(transcript_key),
                               n_ci=n_ci, n_squeezes=n_sq, stream_len=sum(stream_steps(instrs)), commitment_map=None)


class Lanes:
    """Places records on lanes: `serial` puts a transcript operation alone on lane 0, `stage` spreads records that do not
    depend on each other over bundles of at most `width` records, starting at a lane that moves on with every bundle."""

    def __init__(self, L, width=None, first=0):
        self.L, self.width, self.rot, self.bundles = L, min(width or L, L), first, []

    def serial(self, rec):
        self.bundles.append([rec])

    def stage(self, recs):
        for s in range(0, len(recs), self.width):
            bun = [NOP] * self.L
            for j, rec in enumerate(recs[s:s + self.width]):
                bun[(self.rot + j) % self.L] = rec
            self.bundles.append(bun)
            self.rot = (self.rot + ((self.L // 2 - 1) | 1)) % self.L   # an odd step: every lane gets its turn

    def at(self, lane, rec):
        self.bundles.append([NOP] * lane + [rec])


def stream_steps(instrs):
    """bytes each record adds to the hashed stream (a scalar 33, a point 49, the squeeze's own byte 1)"""
    add = {PL.OP_ABSORB_REG: 33, PL.OP_READ_SCALAR: 33, PL.OP_ABSORB_CI: 49, PL.OP_READ_POINT: 49, PL.OP_SQUEEZE: 1}
    out = []
    for rec in instrs:
        if rec[0] == PL.OP_END:
            break
        out.append(add.get(rec[0], 0))
    return out


def squeeze_lengths(instrs):
    """length of the hashed stream at every SQUEEZE, its own 0x00 included (the same in both flavours: the Cardano one hashes
    the whole stream again, the blake2b-512 one keeps one running state)"""
    total, out = 0, []
    for rec, step in zip(instrs, stream_steps(instrs)):
        total += step
        if rec[0] == PL.OP_SQUEEZE:
            out.append(total)
    return out


# ------------------------------------------------------------------------------------------------ operands
def mont_image(v):
    """the plain value whose Montgomery form (what the kernel's carry chains see) is the 256-bit pattern v"""
    assert 0 <= v < R
    return v * pow(1 << 256, -1, R) % R


EDGE = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 2 ** 32 - 1, 2 ** 32, 2 ** 224, 2 ** 254, 2 ** 255 % R, 2 ** 256 % R,
        R - 2 ** 256 % R]
# register patterns: one, r - 1, a low limb of ones, all ones below r, 0xffffffff in each single limb (the top limb of r is
# 0x73eda753: there the largest value with the limbs below it zero)
MONT_PATTERNS = [1, R - 1, 2 ** 32 - 1, 2 ** 254 - 1] + [0xffffffff << (32 * i) for i in range(7)] + [0x73eda752 << 224]
MONT_EDGE = [mont_image(v) for v in MONT_PATTERNS]
OPERANDS = EDGE + [v for v in MONT_EDGE if v not in EDGE]
NON_CANONICAL = [R, R + 1, 2 * R, 2 * R + 1, 2 ** 256 - 1]


@dataclasses.dataclass
class VmBatch:
    proofs: list       # bytes per proof
    instances: list    # N_PI integers per proof (any 256-bit value)
    committed: list    # 48 bytes per proof, or None when the plan has no committed instance

    @property
    def n(self):
        return len(self.proofs)

    def take(self, idx):
        return VmBatch([self.proofs[i] for i in idx], [self.instances[i] for i in idx],
                       None if self.committed is None else [self.committed[i] for i in idx])

    def wire(self):
        """(proofs, proof_off, instances, committed) as the C-ABI takes them"""
        off = [0]
        for p in self.proofs:
            off.append(off[-1] + len(p))
        inst = b"".join(v.to_bytes(32, "little") for row in self.instances for v in row)
        return b"".join(self.proofs), off, inst, None if self.committed is None else b"".join(self.committed)


def expected(plan, batch, use_wide=False):
    """run_plan on every proof: (status words - the OR of every reject reason -, term scalars, registers)"""
    st, sc, regs = [], [], []
    for i in range(batch.n):
        why = set()
        s, r, _first = PL.run_plan(plan, batch.proofs[i], batch.instances[i], None if batch.committed is None else batch.committed[i],
                                   use_wide=use_wide, reasons=why)
        st.append(sum(ST_OF[w] for w in why))
        sc.append(s)
        regs.append(r)
    return st, sc, regs


# ------------------------------------------------------------------------------------------------ (a) the opcode table
OFF_A, OFF_B = 64, 1120 - 32          # where the two scalars of a proof sit (the second ends with the proof)
TABLE_NAMES = ["a+b", "a-b", "b-a", "a*b", "-a", "-b", "1/a", "1/b", "a+a", "a*a", "c*k", "c-k", "1/(a-b)", "-(a*b)", "c", "challenge"]


def spread_regs(n_logical, n_regs):
    """n_logical distinct registers of a file of n_regs: register 0, the highest, and the rest evenly between"""
    assert n_regs >= n_logical
    return [i * (n_regs - 1) // (n_logical - 1) for i in range(n_logical)]


def table_program(L, k_const, n_regs=None, width=None, pi_index=1, first_lane=0, **kw):
    """Reads a, b (READ_SCALAR), c (LOAD_INSTANCE pi_index), k (CONST), squeezes one challenge, and sends the sixteen values of
    TABLE_NAMES to the sixteen term slots and - with a, b, k - to the trace (slot ids 0 .. 18)."""
    O = PL
    n_logical = 19
    rg = spread_regs(n_logical, n_regs or n_logical)
    a, b, c, k, ch = rg[0], rg[1], rg[2], rg[3], rg[4]
    v = rg[5:19]       # the fourteen computed values, in TABLE_NAMES order
    ln = Lanes(L, width, first_lane)
    ln.serial((O.OP_READ_SCALAR, a, OFF_A & 0xffff, OFF_A >> 16))
    ln.stage([(O.OP_LOAD_INSTANCE, c, pi_index, 0), (O.OP_CONST, k, 0, 0)])
    ln.serial((O.OP_READ_SCALAR, b, OFF_B & 0xffff, OFF_B >> 16))
    ln.serial((O.OP_SQUEEZE, ch, 0, 0))
    ln.stage([(O.OP_ADD, v[0], a, b), (O.OP_SUB, v[1], a, b), (O.OP_SUB, v[2], b, a), (O.OP_MUL, v[3], a, b), (O.OP_NEG, v[4], a, 0),
              (O.OP_NEG, v[5], b, 0), (O.OP_INV, v[6], a, 0), (O.OP_INV, v[7], b, 0), (O.OP_ADD, v[8], a, a), (O.OP_MUL, v[9], a, a),
              (O.OP_MUL, v[10], c, k), (O.OP_SUB, v[11], c, k)])
    ln.stage([(O.OP_INV, v[12], v[1], 0), (O.OP_NEG, v[13], v[3], 0)])
    outs = list(v) + [c, ch]
    first_out = ln.rot
    ln.stage([(O.OP_OUT_SCALAR, t, reg, 0) for t, reg in enumerate(outs)])
    if L > 16:      # the lanes the sixteen records above left out write the same values once more: every lane stores
        ln.rot = (first_out + 16) % L
        ln.stage([(O.OP_OUT_SCALAR, t, reg, 0) for t, reg in enumerate(outs)])
    trace = [(t, reg) for t, reg in enumerate(outs)] + [(16, a), (17, b), (18, k)]
    return ln.bundles, dict(consts=[k_const], n_regs=n_regs, trace=trace, **kw)


def table_plan(L, k_const, **kw):
    bundles, args = table_program(L, k_const, **kw)
    return assemble(bundles, L, **args)


WIDE_PI_INDEX = 0


def two_schedule_plan(k_const, **kw):
    """the table program as a narrow schedule of 2 lanes with an 8-lane wide one beside it.  The wide one loads public input
    WIDE_PI_INDEX where the narrow one loads input 1 - otherwise the same program -, so the results tell which schedule ran."""
    narrow, args = table_program(2, k_const, **kw)
    wide, _ = table_program(8, k_const, first_lane=3, pi_index=WIDE_PI_INDEX)
    return assemble(narrow, 2, wide=(8, wide), **args)


def table_model(a, b, c, k):
    """the sixteen values by hand (everything but the challenge), for the CPU test that pins run_plan itself"""
    inv = lambda x: pow(x, R - 2, R) if x % R else 0   # noqa: E731
    a, b, c = a % R, b % R, c % R
    return [(a + b) % R, (a - b) % R, (b - a) % R, a * b % R, -a % R, -b % R, inv(a), inv(b), 2 * a % R, a * a % R, c * k % R,
            (c - k) % R, inv(a - b), -(a * b) % R, c]


def make_proof(rng, a, b):
    p = bytearray(rng.randrange(256) for _ in range(PROOF_LEN))
    p[OFF_A:OFF_A + 32] = a.to_bytes(32, "little")
    p[OFF_B:OFF_B + 32] = b.to_bytes(32, "little")
    return bytes(p)


def _batch_of(triples, seed):
    """(a, b, c) -> proofs; c: the public inputs, one value for all N_PI of them or a list"""
    rng = random.Random(seed)
    return VmBatch([make_proof(rng, a, b) for a, b, _ in triples], [list(c) if isinstance(c, list) else [c] * N_PI for _, _, c in triples], None)


def edge_pairs():
    """every (a, b) of (a): EDGE x EDGE, (x, r - x) and (x, x) for every operand, 60 random pairs"""
    rng = random.Random(1)
    pairs = [(x, y) for x in EDGE for y in EDGE]
    pairs += [(x, (R - x) % R) for x in OPERANDS] + [(x, x) for x in OPERANDS]
    pairs += [(x, y) for x, y in zip(MONT_EDGE, reversed(MONT_EDGE))]
    pairs += [(rng.randrange(R), rng.randrange(R)) for _ in range(60)]
    return pairs


def edge_batch():
    pairs = edge_pairs()
    m = len(OPERANDS)      # (the three public inputs of a proof differ: which one a program loads shows in its results)
    return _batch_of([(a, b, [OPERANDS[(i + 5) % m], OPERANDS[i % m], OPERANDS[(i + 11) % m]]) for i, (a, b) in enumerate(pairs)], seed=2)


def non_canonical_program(L, n_regs=None, **kw):
    """(b): a, b (READ_SCALAR) and c (LOAD_INSTANCE 2) as the VM stores them, and a + b, a * c, c - b, to terms and trace 0 .. 5.
    No inversion: a clean proof has status 0 whatever its values."""
    O = PL
    rg = spread_regs(6, n_regs or 6)
    ln = Lanes(L, first=L - 1)
    ln.serial((O.OP_READ_SCALAR, rg[0], OFF_A, 0))
    ln.serial((O.OP_READ_SCALAR, rg[1], OFF_B, 0))
    ln.stage([(O.OP_LOAD_INSTANCE, rg[2], 2, 0)])
    ln.stage([(O.OP_ADD, rg[3], rg[0], rg[1]), (O.OP_MUL, rg[4], rg[0], rg[2]), (O.OP_SUB, rg[5], rg[2], rg[1])])
    ln.stage([(O.OP_OUT_SCALAR, t, reg, 0) for t, reg in enumerate(rg)])
    return assemble(ln.bundles, L, n_regs=n_regs, trace=list(enumerate(rg)), **kw)


def non_canonical_batch():
    """(b): every non-canonical value in a, in b and in the public input, each between the canonical neighbours r - 1 and 0"""
    triples = []
    for where in range(3):
        for v in NON_CANONICAL:
            for x in (R - 1, v, 0):
                t = [5, 7, 11]
                t[where] = x
                triples.append(tuple(t))
    return _batch_of(triples, seed=3)


# ------------------------------------------------------------------------------------------------ (c) status bits per lane
STATUS_SLOTS = lambda P: sorted({0, 1, P - 1, P, 2 * P})   # noqa: E731


def status_program(L, inv_lane=None, assert_lane=None):
    """x, y from the proof; INV x on inv_lane, ASSERT_ZERO y on assert_lane (None: the program has no such record);
    term 0 and trace slot 0 = the inverse, trace slots 1, 2 = x, y"""
    O = PL
    ln = Lanes(L)
    ln.serial((O.OP_READ_SCALAR, 0, OFF_A, 0))
    ln.serial((O.OP_READ_SCALAR, 1, OFF_B, 0))
    if inv_lane is not None:
        ln.at(inv_lane, (O.OP_INV, 2, 0, 0))
    else:
        ln.at(L - 1, (O.OP_ADD, 2, 0, 0))
    if assert_lane is not None:
        ln.at(assert_lane, (O.OP_ASSERT_ZERO, 0, 1, 0))
    ln.at((L - 1) // 2, (O.OP_OUT_SCALAR, 0, 2, 0))
    return assemble(ln.bundles, L, trace=[(0, 2), (1, 0), (2, 1)])


def status_batch(P, marked=None, seed=4):
    """2P + 1 proofs; the marked ones (default: slots 0, 1, P-1, P, 2P) carry x = 0 and y != 0, the others x != 0 and y = 0"""
    rng = random.Random(seed)
    marked = set(STATUS_SLOTS(P) if marked is None else marked)
    return _batch_of([(0, 1 + rng.randrange(R - 1), 0) if i in marked else (1 + rng.randrange(R - 1), 0, 0) for i in range(2 * P + 1)], seed)


def status_p_choices(L):
    """proofs per block: the launcher's 64 / L, one, and - wherever one exists (64 / L >= 4) - a value strictly between: half
    of 64 / L, the geometry in which the slot mask and the shadow lanes act together"""
    full = 64 // L
    return sorted({full, 1, full // 2 if full >= 4 else 1})


# ------------------------------------------------------------------------------------------------ (d) register-file sizes
def lds_slots(n_regs, L=1):
    """proofs per block the launcher gives a plan (h2v_capi.hip: vm_lds_slots); 0 = the global-register-file kernel"""
    if L > 1:
        return 64 // L
    P = 64
    while P >= 8 and n_regs * 32 * P > PL.VM_LDS_BYTES:
        P >>= 1
    return P if P >= 8 else 0


# one register more than fits 64 / 32 / 16 / 8 proofs of a block in LDS: 32, 16, 8 proofs per block, then global memory
FALLBACK_REGS = {P: PL.VM_LDS_BYTES // (32 * 2 * P) + 1 for P in (32, 16, 8)}
GLOBAL_REGS = PL.VM_LDS_BYTES // (32 * 8) + 1


# ------------------------------------------------------------------------------------------------ (e) transcript operations
SQUEEZE_TARGETS = [127, 0, 1, 127, 0, 1, 64, 0]     # stream length mod 128 at the successive squeezes


def transcript_segments():
    """For every squeeze, how many scalars and points to absorb since the last one so that the stream (the squeeze's 0x00
    included) ends on SQUEEZE_TARGETS: the fewest absorbs that do, found by search"""
    total, out = 0, []
    for want in SQUEEZE_TARGETS:
        best = min((s + p, s, p) for s in range(0, 40) for p in range(0, 40)
                   if s + p >= 1 and (total + 33 * s + 49 * p + 1) % 128 == want)
        out.append((best[1], best[2]))
        total += 33 * best[1] + 49 * best[2] + 1
    return out


def transcript_program(L, kind, key=b"", n_regs=None):
    """READ_POINT / READ_SCALAR / ABSORB_REG (of 0, r - 1 and a computed sum) / ABSORB_CI / SQUEEZE interleaved; challenge j goes
    to term slot j (and trace slot j); the arithmetic between the transcript operations moves over the lanes"""
    O = PL
    ln = Lanes(L)
    zero, top, acc, spare, x = 0, 1, 2, 3, 4     # (acc and spare swap: no record may read a register its bundle writes)
    ln.stage([(O.OP_CONST, zero, 0, 0), (O.OP_CONST, top, 1, 0)])
    ln.stage([(O.OP_ADD, acc, zero, top)])
    n_s = n_p = 0
    trace = []
    for j, (s, p) in enumerate(transcript_segments()):
        ops = ["s"] * s + ["p"] * p
        random.Random(j).shuffle(ops)
        for o in ops:
            if o == "s":
                pick = n_s % 5
                if pick in (0, 3):
                    ln.serial((O.OP_READ_SCALAR, x, 32 * ((7 * n_s) % (PROOF_LEN // 32)), 0))
                    ln.stage([(O.OP_ADD, spare, acc, x)])      # the computed value: r - 1, everything read so far, the challenges
                    acc, spare = spare, acc
                else:
                    ln.serial((O.OP_ABSORB_REG, 0, {1: zero, 2: top, 4: acc}[pick], 0))
                n_s += 1
            else:
                if n_p % 3 == 2:
                    ln.serial((O.OP_ABSORB_CI, 0, 0, 0))
                else:
                    ln.serial((O.OP_READ_POINT, 0, (48 * n_p + 5 * j) % (PROOF_LEN - 48), 0))
                n_p += 1
        ch = 5 + j
        ln.serial((O.OP_SQUEEZE, ch, 0, 0))
        ln.stage([(O.OP_OUT_SCALAR, j, ch, 0), (O.OP_MUL, spare, acc, ch)])
        acc, spare = spare, acc
        trace.append((j, ch))
    trace.append((100, acc))
    return assemble(ln.bundles, L, consts=[0, R - 1], trace=trace, transcript_kind=kind, transcript_key=key, n_ci=1, n_regs=n_regs)


def transcript_batch(n=150, seed=6):
    """random proofs whose scalar slots are canonical (top byte cleared to < r's), a committed instance each"""
    rng = random.Random(seed)
    proofs = []
    for _ in range(n):
        p = bytearray(rng.randrange(256) for _ in range(PROOF_LEN))
        for o in range(31, PROOF_LEN, 32):
            p[o] &= 0x3f
        proofs.append(bytes(p))
    return VmBatch(proofs, [[rng.randrange(R) for _ in range(N_PI)] for _ in range(n)],
                   [bytes(rng.randrange(256) for _ in range(48)) for _ in range(n)])


def squeeze_halves(plan, batch):
    """the 256-bit halves (lo, hi) from_uniform_bytes reduces, of every squeeze of every proof"""
    out = []
    for i in range(batch.n):
        halves = []
        PL.run_plan(plan, batch.proofs[i], batch.instances[i], batch.committed[i], squeezed=halves)
        out.extend(halves)
    return out


# ------------------------------------------------------------------------------------------------ what the GPU tests load
KINDS = ((PL.TR_CARDANO_BLAKE2B_256, b""), (PL.TR_BLAKE2B_512, BLAKE_KEY))
LANE_COUNTS = (1, 2, 4, 8, 16, 32)
# (a): lanes, constant, transcript, declared registers
TABLE_RUNS = ((2, R - 1, KINDS[0], None), (4, (R + 1) // 2, KINDS[1], None), (16, 2 ** 256 % R, KINDS[0], None),
              (1, MONT_EDGE[3], KINDS[0], GLOBAL_REGS))
NON_CANONICAL_LAYOUTS = ((4, None), (32, None), (1, GLOBAL_REGS))       # (b): lanes, declared registers
TRANSCRIPT_LAYOUTS = ((4, None), (1, GLOBAL_REGS))                      # (e)
FALLBACK_K, TWO_SCHEDULE_K = R - 2, 2 ** 32


def geometry_k(L):
    return EDGE[3 + L % 5]


def status_programs(L, k):
    """(c): (inv lane, assert lane, status bits of a marked proof) of the three programs of lane k"""
    return ((k, None, ST_INVERSE_OF_ZERO), (None, k, ST_RECURSION), (k, (k + L // 2) % L, ST_INVERSE_OF_ZERO | ST_RECURSION))


def empty_program():
    """no record but END, no trace table: what h2v_probe_vm refuses to trace"""
    return assemble([[NOP]], 1)


def all_programs():
    """(name, plan) of every program tests/test_vm_programs_gpu.py loads, built from the same tables its tests read"""
    out = [("empty", empty_program()), ("table L=2 k=1", table_plan(2, 1))]
    for L, k, (kind, key), n_regs in TABLE_RUNS:
        out.append(("(a) table L=%d kind=%d n_regs=%s" % (L, kind, n_regs), table_plan(L, k, n_regs=n_regs, transcript_kind=kind, transcript_key=key)))
    for L, n_regs in NON_CANONICAL_LAYOUTS:
        out.append(("(b) non-canonical L=%d n_regs=%s" % (L, n_regs), non_canonical_program(L, n_regs=n_regs)))
    for L in LANE_COUNTS[1:]:
        for k in range(L):
            for inv_lane, assert_lane, _bits in status_programs(L, k):
                out.append(("(c) L=%d inv on %s assert on %s" % (L, inv_lane, assert_lane), status_program(L, inv_lane, assert_lane)))
    for kind, key in KINDS:
        for L in LANE_COUNTS:
            out.append(("(d) table L=%d kind=%d" % (L, kind), table_plan(L, geometry_k(L), transcript_kind=kind, transcript_key=key)))
        for n_regs in list(FALLBACK_REGS.values()) + [GLOBAL_REGS]:
            out.append(("(d) table L=1 n_regs=%d kind=%d" % (n_regs, kind), table_plan(1, FALLBACK_K, n_regs=n_regs, transcript_kind=kind, transcript_key=key)))
        out.append(("(d) two schedules kind=%d" % kind, two_schedule_plan(TWO_SCHEDULE_K, transcript_kind=kind, transcript_key=key)))
        for L, n_regs in TRANSCRIPT_LAYOUTS:
            out.append(("(e) transcript L=%d kind=%d n_regs=%s" % (L, kind, n_regs), transcript_program(L, kind, key, n_regs=n_regs)))
    return out
