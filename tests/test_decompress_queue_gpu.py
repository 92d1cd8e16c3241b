"""The decompression launch of the pipelines (launch_decompress -> k_g1_decompress_queue: subgroup waves in dec_group mode 2,
root waves in mode 1) through h2v_probe_decompress, held point by point to the table of tests/g1_encodings.py: the affine
point, `valid`, `valid_sub` and the 448-dword window tables of every slot of every proof.  Bit-exact, no tolerance.
The table itself is held to the oracle on the CPU (tests/test_g1_encodings.py)."""
import random
import struct
from collections import namedtuple

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, ivc, synth
from tests import g1_encodings as G
from tests.test_gpu_parity import be, circuits  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu
P, R = bls.P, bls.R
RINV = pow(1 << bls.MONT_BITS_FP, -1, P)
FILL = b"\xa5" * 1792
ZERO = bytes(96)
# what one point slot must come out as: valid, valid_sub (None: unspecified, only valid && valid_sub is), x || y, and the tables:
# a point (both tables are checked), "fill" (not written) or None (unspecified)
Exp = namedtuple("Exp", "valid sub xy tab")
DEALT = G.KINDS + ("honest",)
STRIDE = 7
RUNS = len(DEALT)


def _xy(pt):
    return ZERO if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def exp_of_case(c):
    sub = 1 if c.in_g1 else (None if c.kind == "off_curve" else 0)
    tab = c.point if c.in_g1 and c.point is not None else ("fill" if not c.on_curve else None)
    return Exp(int(c.on_curve), sub, _xy(c.point), tab)


def exp_of_encoding(enc):
    """an encoding that is not in the table (the honest points, the accumulator slots), through the same model"""
    on_curve, in_g1, pt = G.model(enc)
    return exp_of_case(G.Case("outside_g1" if on_curve and not in_g1 else "g1" if in_g1 else "off_curve", "", enc, on_curve, in_g1, pt))


def exp_honest(enc):
    """a point the forger made as a multiple of the generator: in G1 by construction, no subgroup test on the host"""
    pt = bls.g1_decompress(enc, False)
    return Exp(1, 1, _xy(pt), pt)


class Layout:
    def __init__(self, vk, pl):
        self.pl, self.n_pi = pl, vk.n_public_inputs
        self.n_points, self.n_ci, self.n_acc = len(pl.points), vk.n_committed_instances, 2 if pl.is_recursive else 0
        self.slots = self.n_points + self.n_ci + self.n_acc
        assert pl.pi_point == self.n_points - 1

    def kind(self, j):
        return "pi" if j == self.pl.pi_point else "proof" if j < self.n_points else "committed" if j < self.n_points + self.n_ci else "acc"


class Work:
    """a batch as lists that can be overwritten slot by slot, and the expectation of every slot beside it"""

    def __init__(self, lay, batch):
        self.lay = lay
        self.proofs = [bytearray(batch.proof(i)) for i in range(batch.n)]
        self.inst = [bytearray(batch.instances[32 * lay.n_pi * i:32 * lay.n_pi * (i + 1)]) for i in range(batch.n)]
        self.ci = [bytearray(batch.ci(i)) for i in range(batch.n)] if lay.n_ci else None
        self.exp = [None] * (batch.n * lay.slots)
        for i in range(batch.n):
            for j in range(lay.slots):
                self.exp[i * lay.slots + j] = self.acc_exp(i, j) if lay.kind(j) == "acc" else exp_honest(self.get(i, j))

    @property
    def n(self):
        return len(self.proofs)

    def get(self, i, j):
        o = self.lay.pl.points[j] if j < self.lay.n_points else 0
        return bytes(self.proofs[i][o:o + 48]) if j < self.lay.n_points else bytes(self.ci[i])

    def put(self, i, j, enc, exp):
        if j < self.lay.n_points:
            o = self.lay.pl.points[j]
            self.proofs[i][o:o + 48] = enc
        else:
            assert self.lay.kind(j) == "committed"
            self.ci[i][:] = enc
        self.exp[i * self.lay.slots + j] = exp

    def acc_encoding(self, i, j):
        """the encoding g1_from_coords builds for an accumulator slot from the public inputs (ivc.py)"""
        c = self.lay.pl.acc_coords[4 * (j - self.lay.n_points - self.lay.n_ci):][:4]
        v = [int.from_bytes(self.inst[i][32 * k:32 * k + 32], "little") for k in c]
        x, y = ivc.coord(v[0], v[1]), ivc.coord(v[2], v[3])
        return G.encode(x, y > P - y), (x, y)

    def acc_exp(self, i, j, honest=True):
        enc, (x, y) = self.acc_encoding(i, j)
        if honest:                              # make_accumulator wrote the coordinates of a multiple of the generator
            e = exp_honest(enc)
            assert e.xy == _xy((x, y))
            return e
        return exp_of_encoding(enc)

    def wire(self):
        off = [0]
        for p in self.proofs:
            off.append(off[-1] + len(p))
        return b"".join(bytes(p) for p in self.proofs), off, b"".join(bytes(b) for b in self.inst), b"".join(bytes(c) for c in self.ci) if self.ci else None


@pytest.fixture(scope="module")
def honest(circuits):   # noqa: F811
    """per key: the layout and a small honest batch whose n * slots points fill three 64-point groups and part of a fourth;
    forged once, never changed (every test copies it into a Work)"""
    out = {}
    for k, name in enumerate(("simple_mul", "trashcan_mix", "ivc")):
        vk, td, pl, dp, ov = circuits[name]
        lay = Layout(vk, pl)
        n = 192 // lay.slots + 1
        while n * lay.slots % 64 == 0:
            n += 1
        assert n * lay.slots > 192 and n * lay.slots % 64
        out[name] = (lay, synth.forge_batch(vk, td, n, seed=131 + k, plan=pl, workers=1, ci_identity=False))
    return out


_MULTIPLES = {}


def multiples(pt):
    """[1..8]P and [1..8]phi(P); phi(P) = [lambda]P by tests/test_g1_encodings.py, so entry m of the second table is [m lambda]P"""
    if pt not in _MULTIPLES:
        row = []
        for base in (pt, G.phi(pt)):
            q = None
            for _ in range(8):
                q = bls.g1_add(q, base)
                row.append(q)
        _MULTIPLES[pt] = row
    return _MULTIPLES[pt]


_TABLES_OK = set()


def check_tables(pt, raw, what):
    if (pt, raw) in _TABLES_OK:
        return
    dw = struct.unpack("<448I", raw)
    for m, want in enumerate(multiples(pt)):
        for c in range(2):
            limbs = dw[28 * m + 14 * c:28 * m + 14 * c + 14]
            assert all(v < 1 << 28 for v in limbs[:13]), (what, m, c, "limbs")
            val = sum(v << (28 * k) for k, v in enumerate(limbs))
            assert val < 2 * P, (what, m, c, "value above 2p")
            assert val * RINV % P == want[c], (what, "table", m // 8, "entry", m % 8 + 1, "xy"[c])
    _TABLES_OK.add((pt, raw))


def check(out, exps, what, tables=True):
    xy, valid, sub, tab, _blocks = out
    assert len(valid) == len(sub) == len(exps) and len(xy) == 96 * len(exps)
    assert (tab is not None) == tables
    for g, e in enumerate(exps):
        w = (what, "point", g)
        assert valid[g] == e.valid, w
        assert sub[g] in (0, 1), w
        if e.sub is None:
            assert not (valid[g] and sub[g]), w
        else:
            assert sub[g] == e.sub, w
        assert xy[96 * g:96 * g + 96] == (e.xy if e.valid else ZERO), w
        if tables and e.tab is not None:
            raw = tab[1792 * g:1792 * g + 1792]
            if e.tab == "fill":
                assert raw == FILL, w
            else:
                check_tables(e.tab, raw, w)


def deal(work, r):
    """run r of RUNS: slot g of the batch gets entry (STRIDE g + 31 r) of the round of kinds (the seven kinds and `honest`, each
    kind's cases in turn); accumulator slots and `honest` entries stay.  Returns the {(kind, slot kind)} and {(kind, lane)} hit
    and the cases dealt."""
    by = G.by_kind()
    L = len(DEALT) * max(len(v) for v in by.values())
    lay = work.lay
    where, lanes, dealt = set(), set(), set()
    for g in range(work.n * lay.slots):
        i, j = divmod(g, lay.slots)
        e = (STRIDE * g + 31 * r) % L
        kind = DEALT[e % len(DEALT)]
        if lay.kind(j) == "acc":
            continue
        where.add((kind, lay.kind(j)))
        lanes.add((kind, g % 64))
        if kind == "honest":
            continue
        c = by[kind][(e // len(DEALT)) % len(by[kind])]
        work.put(i, j, c.enc, exp_of_case(c))
        dealt.add(c.enc)
    return where, lanes, dealt


@pytest.mark.parametrize("name", ["simple_mul", "trashcan_mix", "ivc"])
def test_every_kind_in_every_slot_kind_and_lane(be, circuits, honest, name):   # noqa: F811
    """Every kind of the table - and untouched honest points between them - in a proof-point slot, the pi slot, the committed
    slot where the key has one, and lanes 0 and 63 of a 64-point group; every case of the table at least once.  With the
    window tables and without: the same points and verdicts."""
    from math import gcd
    dp = circuits[name][3]
    lay, batch = honest[name]
    assert gcd(STRIDE, 64) == 1 and gcd(STRIDE, lay.slots) == 1
    where, lanes, dealt = set(), set(), set()
    for r in range(RUNS):
        work = Work(lay, batch)
        w, ln, d = deal(work, r)
        where |= w
        lanes |= ln
        dealt |= d
        groups = (work.n * lay.slots + 63) // 64
        assert groups >= 4 and work.n * lay.slots % 64
        full = be.probe_decompress(dp, lay.slots, *work.wire(), tables=True)
        bare = be.probe_decompress(dp, lay.slots, *work.wire(), tables=False)
        check(full, work.exp, (name, r))
        assert bare[:3] == full[:3] and bare[3] is None and bare[4] == full[4], (name, r)
        assert full[4] == (2 * groups + 3) // 4            # fewer units than the chip has waves: one wave each
    slot_kinds = {"proof", "pi"} | ({"committed"} if lay.n_ci else set())
    assert where == {(k, s) for k in DEALT for s in slot_kinds}
    assert {(k, ln) for k in DEALT for ln in (0, 63)} <= lanes
    assert dealt == {c.enc for c in G.cases()}


def test_short_proof(be, circuits, honest):   # noqa: F811
    """one proof a byte short: its proof-point slots are all invalid (the kernel reads nothing of it), its committed instance
    still decodes, and the proofs around it - which start a byte earlier in the buffer - are what they were"""
    dp = circuits["trashcan_mix"][3]
    lay, batch = honest["trashcan_mix"]
    work = Work(lay, batch)
    mid = work.n // 2
    work.proofs[mid] = work.proofs[mid][:-1]
    for j in range(lay.n_points):
        work.exp[mid * lay.slots + j] = Exp(0, 0, ZERO, "fill")
    assert work.exp[mid * lay.slots + lay.n_points].valid == 1 and lay.kind(lay.n_points) == "committed"
    check(be.probe_decompress(dp, lay.slots, *work.wire()), work.exp, "short proof")


def test_accumulator_slots(be, circuits, honest):   # noqa: F811
    """the two slots rebuilt from public inputs: honest accumulators give the points make_accumulator wrote; acc_sign (y -> p - y
    on the right accumulator) the negated point; acc_limb (another x on the left) whatever the model says of the new x"""
    vk, td, pl, dp, ov = circuits["ivc"]
    lay, batch = honest["ivc"]
    work = Work(lay, batch)
    left, right = lay.n_points + lay.n_ci, lay.n_points + lay.n_ci + 1
    assert lay.kind(left) == lay.kind(right) == "acc" and right == lay.slots - 1
    check(be.probe_decompress(dp, lay.slots, *work.wire()), work.exp, "honest accumulators")
    rng = random.Random(77)
    verdicts = set()
    for i in range(work.n):
        before = work.exp[i * lay.slots + (right if i % 2 else left)]
        _, inst = synth.corrupt(pl, bytes(work.proofs[i]), bytes(work.inst[i]), "acc_sign" if i % 2 else "acc_limb", rng)
        work.inst[i] = bytearray(inst)
        if i % 2:
            e = work.acc_exp(i, right, honest=False)
            x, y = int.from_bytes(before.xy[:48], "big"), int.from_bytes(before.xy[48:], "big")
            assert e.xy == _xy((x, P - y)) and (e.valid, e.sub) == (1, 1)
            work.exp[i * lay.slots + right] = e
        else:
            e = work.acc_exp(i, left, honest=False)
            assert e.xy[:48] != before.xy[:48]
            verdicts.add((e.valid, e.sub))
            work.exp[i * lay.slots + left] = e
    assert len(verdicts) >= 2                               # (new x values off the curve and on it)
    check(be.probe_decompress(dp, lay.slots, *work.wire()), work.exp, "damaged accumulators")


def test_queue_walk(be, circuits, honest):   # noqa: F811
    """more units than the launch has waves, so that waves go round the queue: the dealt simple_mul batch repeated until
    2 ceil(n slots / 64) exceeds four times the grid - the grid as the probe reports it.  Every repetition must come out as the
    first (the lanes a point sits in move on with every repetition).  And a batch of one proof: two units for a block's four waves."""
    dp = circuits["simple_mul"][3]
    lay, batch = honest["simple_mul"]
    work = Work(lay, batch)
    deal(work, 3)
    proofs, off, inst, ci = work.wire()
    reps, out = 16, None
    while reps <= 1024:
        n = work.n * reps
        offs = [k * (off[-1] // work.n) for k in range(n + 1)]
        units = 2 * ((n * lay.slots + 63) // 64)
        out = be.probe_decompress(dp, lay.slots, proofs * reps, offs, inst * reps, None, tables=False)
        if units > 4 * out[4]:
            break
        reps *= 2
    out = be.probe_decompress(dp, lay.slots, proofs * reps, offs, inst * reps, None, tables=True)
    print("queue walk: %d points, %d units, %d blocks" % (n * lay.slots, units, out[4]))
    assert units > 4 * out[4]
    check(out, work.exp * reps, ("queue walk", reps))
    one = Work(lay, batch)
    one.proofs, one.inst, one.exp = one.proofs[:1], one.inst[:1], one.exp[:lay.slots]
    one.put(0, 0, G.by_kind()["outside_g1"][0].enc, exp_of_case(G.by_kind()["outside_g1"][0]))
    tiny = be.probe_decompress(dp, lay.slots, *one.wire())
    assert tiny[4] == 1 and 2 * ((lay.slots + 63) // 64) < 4 * tiny[4]
    check(tiny, one.exp, "one proof")


def test_probe_refuses_bad_arguments(be, circuits, honest):   # noqa: F811
    dp = circuits["trashcan_mix"][3]
    lay, batch = honest["trashcan_mix"]
    with pytest.raises(be.H2VError):
        be.probe_decompress(dp, lay.slots, b"", [0], b"", None)                         # an empty batch
    import ctypes as C
    n, b, _keep = dp._host_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)
    m = n * lay.slots
    xy, v, s, blocks = C.create_string_buffer(96 * m), C.create_string_buffer(m), C.create_string_buffer(m), C.c_uint32()
    tab = C.create_string_buffer(1792 * m)
    L = be.lib()
    assert L.h2v_probe_decompress(dp.handle, C.byref(b), 0, xy, v, s, tab, C.byref(blocks)) != 0    # tables asked for, none built
    assert L.h2v_probe_decompress(dp.handle, C.byref(b), 1, xy, None, s, None, C.byref(blocks)) != 0
    b.committed = None
    assert L.h2v_probe_decompress(dp.handle, C.byref(b), 1, xy, v, s, None, C.byref(blocks)) != 0  # the key has a committed instance


def _device_verdicts(be, dp, w, rlc):   # noqa: F811
    """(accept, status) of the device form of verify_batch / verify_batch_rlc (the batch check's results live in a workspace)"""
    import torch
    dev = torch.device("cuda", 0)
    proofs, off, inst, ci = w
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    d_proofs, d_inst, d_ci = t(proofs), t(inst), t(ci)
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    n = len(off) - 1
    acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run = dp.verify_batch_rlc_device if rlc else dp.verify_batch_device
    ws = be.Workspace(dp, n)
    run(n, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream)
    s.synchronize()
    ws.close()
    return list(acc.cpu().tolist()), [v & 0xffffffff for v in st.cpu().tolist()]


def test_through_whole_pipelines(be, circuits, honest):   # noqa: F811
    """a damaged committed instance (off the curve, outside G1, bit 7 clear: one proof each) and a proof point re-encoded as
    x + p, through verify_batch, verify_batch_rlc and prepare_batch: the oracle's verdicts, ST_BAD_POINT on each damaged proof"""
    vk, td, pl, dp, ov = circuits["trashcan_mix"]
    lay, batch = honest["trashcan_mix"]
    work = Work(lay, batch)
    by = G.by_kind()
    ci_slot = lay.n_points
    damage = {1: by["off_curve"][1], 3: by["outside_g1"][4], 4: by["no_compression_bit"][3]}
    for i, c in damage.items():
        work.put(i, ci_slot, c.enc, exp_of_case(c))
    low = [(i, j) for i in range(work.n) if i not in damage and i != 0 for j in range(lay.n_points)
           if int.from_bytes(work.get(i, j), "big") & ((1 << 381) - 1) < (1 << 381) - P]
    assert low, "no proof point with x + p below 2^381 in the batch"
    i, j = low[0]
    enc = work.get(i, j)
    x0 = int.from_bytes(enc, "big") & ((1 << 381) - 1)
    work.put(i, j, G.encode(x0 + P, G.sort_flag(enc)), Exp(0, 0, ZERO, "fill"))
    damaged = sorted(list(damage) + [i])
    w = work.wire()
    want = list(ov.verify_batch(*w, threads=4))
    assert want == [0 if k in damaged else 1 for k in range(work.n)]
    check(be.probe_decompress(dp, lay.slots, *w), work.exp, "pipeline batch")
    assert list(dp.verify_batch(*w)) == want
    acc, _fell_back = dp.verify_batch_rlc(*w)
    assert list(acc) == want
    pairs, pst = dp.prepare_batch(*w)
    assert [int(s == 0) for s in pst] == want
    for rlc in (False, True):
        acc, st = _device_verdicts(be, dp, w, rlc)
        assert acc == want, rlc
        assert [bool(v & be.ST_BAD_POINT) for v in st] == [k in damaged for k in range(work.n)], (rlc, st)
        assert [v == 0 for v in st] == [k not in damaged for k in range(work.n)], (rlc, st)
    for k in range(work.n):
        assert (pst[k] == be.ST_BAD_POINT) == (k in damaged) and (pairs[96 * k:96 * k + 96] == bytes(96)) == (k in damaged), k
