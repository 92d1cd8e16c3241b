"""CPU side of the hand-assembled VM programs (tests/vm_asm.py): every program and batch the GPU tests of
tests/test_vm_programs_gpu.py run is built here, passes plan.check_bundles and the loader's validation, the big-integer model
plan.run_plan is pinned on hand-computed records, and the coverage the batches are meant to have is asserted, not assumed."""
import os

import pytest

from plutus_halo2_verifier_gen_amd import plan as PL
from tests import vm_asm as A
from tests.plan_loading import plan_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = A.R
E_PLAN, E_DEVICE = -2, -3


def test_programs_pass_check_bundles_and_the_loader():
    """every program: plan.check_bundles (inside the assembler, again here for both schedules), and h2v_plan_load's own
    validation of the blob - which ends with H2V_E_DEVICE on a machine without a GPU (H2V_E_PLAN would be a refusal)"""
    from plutus_halo2_verifier_gen_amd import backend
    load = plan_loader()
    ok_rc = 0 if backend.device_count() >= 1 else E_DEVICE
    plans = A.all_programs()      # every program the GPU tests load: both files read the same tables of tests/vm_asm.py
    assert len(plans) == 2 + 4 + 3 + 3 * 62 + 2 * (6 + 4 + 1 + 2)
    for name, pl in plans:
        PL.check_bundles(pl.instrs, pl.vm_lanes)
        assert pl.instrs[-pl.vm_lanes][0] == PL.OP_END and all(r[0] != PL.OP_END for r in pl.instrs[:-pl.vm_lanes]), name
        if pl.wide:
            PL.check_bundles(pl.wide[2], pl.wide[0])
        rc, _msg = load(pl.to_bytes())
        assert rc == ok_rc, (name, rc)
    # the assembler refuses what the device relies on not happening
    with pytest.raises(AssertionError):
        A.assemble([[A.NOP, (PL.OP_SQUEEZE, 0, 0, 0)]], 2)                          # transcript operation off lane 0
    with pytest.raises(AssertionError):
        A.assemble([[(PL.OP_CONST, 0, 0, 0), (PL.OP_NEG, 1, 0, 0)]], 2)              # reads what its bundle writes
    with pytest.raises(AssertionError):
        A.assemble([[(PL.OP_CONST, 0, 0, 0)] * 3], 2)                               # more records than lanes


def test_lane_placement_covers_every_lane():
    """the table program's arithmetic sits on every lane of every lane count at least once, and its transcript operations on
    lane 0 only: the placement moves on between bundles"""
    for L in (2, 4, 8, 16, 32):
        pl = A.table_plan(L, 1)
        busy = {k % L for k, rec in enumerate(pl.instrs) if rec[0] not in (PL.OP_NOP, PL.OP_END)}
        assert busy == set(range(L)), (L, busy)
        # some bundle holds more than one record (lanes really run side by side), unless the program is one lane wide
        assert max(sum(1 for rec in pl.instrs[s:s + L] if rec[0] != PL.OP_NOP) for s in range(0, len(pl.instrs), L)) == min(L, 16)
    assert len(A.TABLE_NAMES) == A.N_TERMS


def test_run_plan_on_hand_computed_records():
    """the model itself, on records worked out by hand"""
    pl = A.table_plan(4, 7)
    names = A.TABLE_NAMES

    def run(a, b, c):
        batch = A._batch_of([(a, b, c)], seed=9)
        why = set()
        sc, regs, first = PL.run_plan(pl, batch.proofs[0], batch.instances[0], reasons=why)
        return dict(zip(names, sc)), first, why

    v, first, why = run(R - 1, 1, 0)
    assert v["a+b"] == 0 and v["a-b"] == R - 2 and v["b-a"] == 2 and v["a*b"] == R - 1 and v["-a"] == 1 and v["-b"] == R - 1
    assert v["1/a"] == R - 1 and v["1/b"] == 1 and v["a+a"] == R - 2 and v["a*a"] == 1 and v["-(a*b)"] == 1
    assert v["c*k"] == 0 and v["c-k"] == R - 7 and v["c"] == 0 and v["1/(a-b)"] * (R - 2) % R == 1
    assert first is None and why == set()
    v, first, why = run(0, 1, 8)
    assert v["a-b"] == R - 1 and v["-a"] == 0 and v["1/a"] == 0 and v["c*k"] == 56 and v["c-k"] == 1
    assert first == "inverse" and why == {"inverse"}
    v, first, why = run(R + 5, 5, 3)                       # READ_SCALAR of r + 5: register 5, and then a - b = 0 has no inverse
    assert v["a+b"] == 10 and v["a-b"] == 0 and v["1/(a-b)"] == 0 and v["a*a"] == 25
    assert first == "scalar" and why == {"scalar", "inverse"}
    v, first, why = run(2, 3, 2 * R + 1)                   # LOAD_INSTANCE of 2r + 1: register 1
    assert v["c"] == 1 and v["c*k"] == 7 and first == "scalar" and why == {"scalar"}
    # ASSERT_ZERO and a short proof
    sp = A.status_program(4, inv_lane=1, assert_lane=3)
    b = A.status_batch(2)
    st, sc, regs = A.expected(sp, b)
    assert st == [A.ST_INVERSE_OF_ZERO | A.ST_RECURSION if i in (0, 1, 2, 4) else 0 for i in range(5)]
    assert all(sc[i][0] == 0 for i in (0, 1, 2, 4)) and all(sc[i][0] * regs[i][0] % R == 1 for i in (3,))
    why = set()
    assert PL.run_plan(sp, b.proofs[0][:-1], b.instances[0], reasons=why)[2] == "short" and why == {"short"}
    # every existing caller's view is unchanged: three values, the first reason
    assert len(PL.run_plan(sp, b.proofs[0], b.instances[0])) == 3
    # the whole table against the formulas, on the edge batch
    eb = A.edge_batch()
    k = 7
    st, sc, regs = A.expected(pl, eb)
    for i in range(eb.n):
        a = int.from_bytes(eb.proofs[i][A.OFF_A:A.OFF_A + 32], "little")
        b_ = int.from_bytes(eb.proofs[i][A.OFF_B:A.OFF_B + 32], "little")
        assert sc[i][:15] == A.table_model(a, b_, eb.instances[i][1], k), i
        assert st[i] == (A.ST_INVERSE_OF_ZERO if 0 in (a, b_, (a - b_) % R) else 0), i


def test_edge_batch_covers_the_boundaries():
    """(a): the pairs the opcode table runs on hold each boundary at least once - in the plain domain, and the Montgomery
    patterns as register contents"""
    pairs = A.edge_pairs()
    assert 300 <= len(pairs) <= 400 and len(set(A.EDGE)) == 14
    assert all(0 <= a < R and 0 <= b < R for a, b in pairs)
    have = lambda f: any(f(a, b) for a, b in pairs)   # noqa: E731
    assert have(lambda a, b: a + b == R) and have(lambda a, b: a + b == R - 1) and have(lambda a, b: a + b == R + 1)
    assert have(lambda a, b: a == b and a) and have(lambda a, b: a < b) and have(lambda a, b: a > b)
    assert have(lambda a, b: a * b % R == 1 and a != 1) and have(lambda a, b: a == 0 and b) and have(lambda a, b: b == 0 and a)
    assert have(lambda a, b: a == 0 and b == 0)
    assert all((x, y) in set(pairs) for x in A.EDGE for y in A.EDGE)
    assert all((x, (R - x) % R) in set(pairs) and (x, x) in set(pairs) for x in A.OPERANDS)
    mont = lambda v: v * (1 << 256) % R   # noqa: E731
    seen = {mont(a) for a, _ in pairs} | {mont(b) for _, b in pairs}
    assert set(A.MONT_PATTERNS) <= seen
    assert 0x73eda752 << 224 in seen and all(0xffffffff << (32 * limb) in seen for limb in range(7))
    eb = A.edge_batch()
    assert {row[1] for row in eb.instances} == set(A.OPERANDS)
    # (b): every non-canonical value in every position, between clean canonical neighbours
    nb = A.non_canonical_batch()
    st, sc, regs = A.expected(A.non_canonical_program(2), nb)
    assert st == [0, A.ST_BAD_SCALAR, 0] * 15
    assert [s[:3] for s in sc[:6]] == [[R - 1, 7, 11], [0, 7, 11], [0, 7, 11], [R - 1, 7, 11], [1, 7, 11], [0, 7, 11]]
    assert sc[-2][:3] == [5, 7, (2 ** 256 - 1) % R]
    assert all(v >= R and v < 2 ** 256 for v in A.NON_CANONICAL)


def test_register_file_sizes_reach_every_fallback():
    """(d): the register counts that make the launcher run 32, 16 and 8 proofs per block and then the global register file
    (h2v_capi.hip: vm_lds_slots), each one register past the boundary"""
    assert A.lds_slots(20) == 64
    for P, n_regs in A.FALLBACK_REGS.items():
        assert A.lds_slots(n_regs) == P and A.lds_slots(n_regs - 1) == 2 * P, (P, n_regs)
        pl = A.table_plan(1, 1, n_regs=n_regs)
        used = {r[1] for r in pl.instrs if PL._defines(r[0])}
        assert 0 in used and n_regs - 1 in used
    assert A.lds_slots(A.GLOBAL_REGS) == 0 and A.lds_slots(A.GLOBAL_REGS - 1) == 8
    for L in (2, 4, 8, 16, 32):
        assert A.table_plan(L, 1).n_regs * 32 * (64 // L) <= PL.VM_LDS_BYTES
        # (c): the launcher's 64 / L, one, and a value strictly between wherever there is one
        ps, full = A.status_p_choices(L), 64 // L
        assert 1 in ps and full in ps and all(p & (p - 1) == 0 for p in ps)
        assert full < 4 or any(1 < p < full for p in ps), (L, ps)
    assert A.status_p_choices(16) == [1, 2, 4]


def test_transcript_program_hits_the_block_boundaries_and_every_reduction_range():
    """(e): the hashed stream ends 127, 0 and 1 bytes into a 128-byte block at a squeeze, in each flavour; and over the batch
    both halves that from_uniform_bytes reduces fall in [0, r), [r, 2r) and [2r, 2^256)"""
    for kind, key in ((PL.TR_CARDANO_BLAKE2B_256, b""), (PL.TR_BLAKE2B_512, A.BLAKE_KEY)):
        pl = A.transcript_program(4, kind, key)
        lens = A.squeeze_lengths(pl.instrs)
        assert [n % 128 for n in lens] == A.SQUEEZE_TARGETS and {127, 0, 1} <= {n % 128 for n in lens}
        assert len(lens) == 8 and lens[-1] > 4 * 128
        ops = {r[0] for r in pl.instrs}
        assert {PL.OP_READ_POINT, PL.OP_READ_SCALAR, PL.OP_ABSORB_REG, PL.OP_ABSORB_CI, PL.OP_SQUEEZE} <= ops and pl.n_ci == 1
        absorbed = {r[2] for r in pl.instrs if r[0] == PL.OP_ABSORB_REG}
        assert {0, 1} < absorbed            # the constants 0 and r - 1, and the computed accumulator
        batch = A.transcript_batch()
        halves = A.squeeze_halves(pl, batch)
        assert len(halves) == 8 * batch.n
        band = lambda v: 0 if v < R else 1 if v < 2 * R else 2   # noqa: E731
        assert {band(lo) for lo, _ in halves} == {0, 1, 2} and {band(hi) for _, hi in halves} == {0, 1, 2}
        st, sc, regs = A.expected(pl, batch)
        assert st == [0] * batch.n          # canonical scalars throughout: the only status in the GPU run is the short proof's
        assert len({s[j] for s in sc for j in range(8)}) == 8 * batch.n
    # the same program gives other challenges under the other hash
    b3 = A.transcript_batch(3)
    assert A.expected(A.transcript_program(2, 0), b3)[1] != A.expected(A.transcript_program(2, 1, A.BLAKE_KEY), b3)[1]
