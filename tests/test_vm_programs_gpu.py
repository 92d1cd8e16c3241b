"""The transcript + Fr-combiner interpreter (csrc/h2v_kernels.hip: vm_run and its four kernels, launched by launch_vm) driven
with hand-assembled programs (tests/vm_asm.py) through h2v_probe_vm, and held to plan.run_plan bit for bit: trace registers,
the sixteen term scalars and the status word of EVERY proof of a batch.  No tolerance anywhere.

Which kernel a combination reaches (launch_vm picks by lane count, register count and the plan's transcript kind):
  k_transcript_combiner_lds        any lane count whose register file fits LDS, Cardano transcript - (a) to (e)
  k_transcript_combiner_lds_b512   the same under the keyed blake2b-512 transcript               - (a), (d), (e)
  k_transcript_combiner            one lane per proof and more than 604 registers, Cardano       - (a), (b), (d), (e)
  k_transcript_combiner_b512       the same under the keyed blake2b-512 transcript               - (d), (e)
The CPU side of the same programs and batches (coverage conditions, the model on hand-computed records) is
tests/test_vm_programs.py."""
import contextlib

import pytest

from plutus_halo2_verifier_gen_amd import plan as PL
from tests import vm_asm as A
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
R = A.R
KINDS = A.KINDS


def load(be, pl):   # noqa: F811
    # (the narrowest fixed-base tables: nothing here runs an MSM)
    return be.DevicePlan(pl.to_bytes(), 0, fixed_base_window_bits=4)


@contextlib.contextmanager
def loaded(be, pl):   # noqa: F811
    """the plan on the device for the length of a `with` block: its tables are freed when the block ends, pass or fail"""
    dp = load(be, pl)
    try:
        yield dp
    finally:
        dp.close()


def probe(be, dp, batch, P=0, schedule=0, trace=True):   # noqa: F811
    be.probe_set_option(be.OPT_COMBINER_PROOFS_PER_BLOCK, P)
    be.probe_set_option(be.OPT_COMBINER_SCHEDULE, schedule)
    try:
        return be.probe_vm(dp, *batch.wire(), want_trace=trace)
    finally:
        be.probe_set_option(be.OPT_COMBINER_PROOFS_PER_BLOCK, 0)
        be.probe_set_option(be.OPT_COMBINER_SCHEDULE, 0)


def model(pl, batch, use_wide=False):
    """(status, scalars, trace dict) per proof from run_plan; the trace by slot id, so that it does not depend on which
    registers a layout of the program uses"""
    st, sc, regs = A.expected(pl, batch, use_wide)
    return [(st[i], sc[i], {slot: regs[i][reg] for slot, reg in pl.trace}) for i in range(batch.n)]


def assert_equal(got, want, what, trace=True, skip=()):
    st, sc, tr = got
    assert len(st) == len(want), what
    assert st == [w[0] for w in want], (what, "status", [(i, hex(s), hex(w[0])) for i, (s, w) in enumerate(zip(st, want)) if s != w[0]][:8])
    for i, w in enumerate(want):
        if i in skip:
            continue
        assert sc[i] == w[1], (what, "term scalars of proof", i, [k for k in range(len(w[1])) if sc[i][k] != w[1][k]])
        if trace:
            assert tr[i] == w[2], (what, "trace of proof", i, [k for k in w[2] if tr[i].get(k) != w[2][k]])
    assert trace or tr is None


@pytest.fixture(scope="module")
def table(be):   # noqa: F811
    """The opcode-table program's expected values on the whole edge batch, worked out once per (constant, transcript, public
    input) - they do not depend on lanes or registers - and the loaded plans, kept for the module and closed after it"""
    batch = A.edge_batch()
    models, plans = {}, {}

    def want(k, kind, key, idx, pi_index=1):
        tag = (k, kind, pi_index)
        if tag not in models:
            models[tag] = model(A.table_plan(1, k, transcript_kind=kind, transcript_key=key, pi_index=pi_index), batch)
        return [models[tag][i] for i in idx]

    def plan(tag, make):
        if tag not in plans:
            pl = make()
            plans[tag] = (pl, load(be, pl))
        return plans[tag]
    yield batch, want, plan
    for _pl, dp in plans.values():
        dp.close()


def test_probe_refuses_bad_arguments(be):   # noqa: F811
    proofs, off, inst, ci = A.edge_batch().take([0]).wire()
    with loaded(be, A.table_plan(2, 1)) as dp:
        with pytest.raises(be.H2VError):
            be.probe_vm(dp, b"", [0], b"", None)                      # an empty batch
        st, sc, tr = be.probe_vm(dp, proofs, off, inst, ci, want_trace=False)
        assert tr is None and st == [A.ST_INVERSE_OF_ZERO] and sc[0][0] == 0     # (proof 0 of the edge batch is a = b = 0)
    with loaded(be, A.empty_program()) as dp:
        with pytest.raises(be.H2VError):
            be.probe_vm(dp, proofs, off, inst, ci, want_trace=True)   # no trace table to read


def test_opcode_table_on_edge_operands(be, table):   # noqa: F811
    """(a): the whole edge batch (320 proofs: several blocks, the last one ragged) through the table program, with four
    constants from the edge set, on 2, 4 and 16 lanes in LDS and on the global-register-file kernel, under both transcripts"""
    batch, want, plan = table
    idx = list(range(batch.n))
    for L, k, (kind, key), n_regs in A.TABLE_RUNS:
        pl, dp = plan(("a", L, k, kind, n_regs), lambda: A.table_plan(L, k, n_regs=n_regs, transcript_kind=kind, transcript_key=key))
        assert_equal(probe(be, dp, batch), want(k, kind, key, idx), (L, hex(k), kind, n_regs))


def test_non_canonical_input(be):   # noqa: F811
    """(b): r, r + 1, 2r, 2r + 1 and 2^256 - 1 as READ_SCALAR and LOAD_INSTANCE input: ST_BAD_SCALAR, the register holds the
    value mod r (fr_to_mont above the modulus), and the canonical neighbours r - 1 and 0 in the adjacent slots stay clean"""
    batch = A.non_canonical_batch()
    for L, n_regs in A.NON_CANONICAL_LAYOUTS:
        pl = A.non_canonical_program(L, n_regs=n_regs)
        want = model(pl, batch)
        with loaded(be, pl) as dp:
            got = probe(be, dp, batch)
        assert got[0] == [0, A.ST_BAD_SCALAR, 0] * 15, L
        assert_equal(got, want, ("non-canonical", L))
        for j, v in enumerate(A.NON_CANONICAL * 3):
            assert got[1][3 * j + 1][j // 5] == v % R and got[1][3 * j][j // 5] == R - 1 and got[1][3 * j + 2][j // 5] == 0


@pytest.mark.parametrize("L", [2, 4, 8, 16, 32])
def test_status_bits_per_lane(be, L):   # noqa: F811
    """(c): the cross-lane status reduction.  For every lane k of L: a program whose only INV of a proof-supplied value sits on
    lane k, one whose only ASSERT_ZERO does, and one with both on different lanes; batches of 2P + 1 proofs of which exactly
    those at slots 0, 1, P-1, P, 2P carry the zero / non-zero value; P = 64 / L, 1 and - for L <= 16 - half of 64 / L, where the
    slot mask and the shadow lanes act together (L = 32 has no value between).  The status vector
    is exactly the constructed one - H2V_ST_INVERSE_OF_ZERO and / or H2V_ST_RECURSION on those proofs and on no other - and
    the inverse register of a zero is zero.  Control: every proof clean gives an all-zero status."""
    batches = {P: A.status_batch(P) for P in A.status_p_choices(L)}
    for k in range(L):
        for inv_lane, assert_lane, bits in A.status_programs(L, k):
            pl = A.status_program(L, inv_lane, assert_lane)
            with loaded(be, pl) as dp:
                for P, batch in batches.items():
                    got = probe(be, dp, batch, P=P)
                    marked = A.STATUS_SLOTS(P)
                    assert got[0] == [bits if i in marked else 0 for i in range(2 * P + 1)], (L, k, inv_lane, assert_lane, P)
                    assert_equal(got, model(pl, batch), (L, k, inv_lane, assert_lane, P))
                    if inv_lane is not None:
                        assert all(got[1][i][0] == 0 and got[2][i][0] == 0 for i in marked)
                if k == L - 1 and assert_lane is not None and inv_lane is not None:
                    for P in batches:
                        clean = A.status_batch(P, marked=[])
                        got = probe(be, dp, clean, P=P)
                        assert got[0] == [0] * (2 * P + 1)
                        assert_equal(got, model(pl, clean), (L, "clean", P))


def _sizes(P):
    return sorted({n for n in (1, P - 1, P, P + 1, 2 * P + 3) if n >= 1})


def _geometry_runs(be, table, L, n_regs, k, kinds, forced):   # noqa: F811
    """the table program at one lane count and register-file size: every P of `forced` (0 = the launcher's choice) x every
    batch size around it.  The proofs move through the edge batch from run to run; in the 2P + 3 run the last proof - the one
    the dead slots of the last block shadow - is the only one with a status bit."""
    batch, want, plan = table
    auto = A.lds_slots(n_regs or 20, L) or 64
    clean = [i for i, w in enumerate(want(k, KINDS[0][0], b"", range(batch.n))) if w[0] == 0]
    run = 0
    for kind, key in kinds:
        pl, dp = plan(("d", L, n_regs, k, kind), lambda: A.table_plan(L, k, n_regs=n_regs, transcript_kind=kind, transcript_key=key))
        for P in forced:
            for n in _sizes(P or auto):
                run += 1
                if n == 2 * (P or auto) + 3:
                    idx = [clean[(41 * run + j) % len(clean)] for j in range(n - 1)] + [0]    # proof 0: a = b = 0
                else:
                    idx = [(53 * run + j) % batch.n for j in range(n)]
                w = want(k, kind, key, idx)
                assert n != 2 * (P or auto) + 3 or [x[0] for x in w] == [0] * (n - 1) + [A.ST_INVERSE_OF_ZERO]
                assert_equal(probe(be, dp, batch.take(idx), P=P), w, (L, n_regs, kind, "P", P, "n", n))


@pytest.mark.parametrize("L", A.LANE_COUNTS)
def test_geometry_matrix(be, table, L):   # noqa: F811
    """(d): the opcode-table program laid out for L lanes (which lane gets which record moves on between bundles), under both
    transcripts, with the launcher's choice of proofs per block and every forced power of two from 1 to 64 / L, at
    n = 1, P-1, P, P+1 and 2P+3 proofs.  L = 32 is reached by no compiled key; it runs here like the others."""
    forced = [0] + [1 << s for s in range(7) if (1 << s) <= 64 // L]
    _geometry_runs(be, table, L, None, A.geometry_k(L), KINDS, forced)


@pytest.mark.parametrize("slots", [32, 16, 8, 0])
def test_geometry_one_lane_register_file_sizes(be, table, slots):   # noqa: F811
    """(d), L = 1: register counts one past what fits 64, 32 and 16 proofs of a block in LDS - the launcher's fallbacks to 32,
    16 and 8 proofs per block with the other lanes idle, each with the launcher's choice and every forced power of two up to it -
    and one past 8: the global-register-file kernels (64 proofs per block whatever is asked).  The program uses register 0 and
    the highest one."""
    n_regs = A.FALLBACK_REGS[slots] if slots else A.GLOBAL_REGS
    assert A.lds_slots(n_regs) == slots
    _geometry_runs(be, table, 1, n_regs, A.FALLBACK_K, KINDS, [0] + [1 << s for s in range(6) if (1 << s) <= slots])


def test_both_schedules_of_one_plan(be, table):   # noqa: F811
    """(d): a plan with the 2-lane program as its narrow schedule and the 8-lane one as `wide`, H2V_OPT_COMBINER_SCHEDULE forced
    both ways.  The wide program loads another public input than the narrow one, so the scalars show which one ran; there is no
    trace on the wide schedule, and asking for the trace runs the narrow one whatever the option says."""
    batch, want, plan = table
    k = A.TWO_SCHEDULE_K
    for kind, key in KINDS:
        pl, dp = plan(("two", kind), lambda: A.two_schedule_plan(k, transcript_kind=kind, transcript_key=key))
        for n in (1, 9, 67):
            idx = [(7 * n + j) % batch.n for j in range(n)]
            sub = batch.take(idx)
            narrow, wide = want(k, kind, key, idx), want(k, kind, key, idx, pi_index=A.WIDE_PI_INDEX)
            assert [w[1] for w in narrow] != [w[1] for w in wide]
            assert [m[:2] for m in model(pl, sub, use_wide=True)] == [w[:2] for w in wide]     # run_plan on the plan's own wide schedule
            assert_equal(probe(be, dp, sub, schedule=1), narrow, ("narrow", kind, n))
            assert_equal(probe(be, dp, sub, schedule=1, trace=False), narrow, ("narrow, no trace", kind, n), trace=False)
            assert_equal(probe(be, dp, sub, schedule=2, trace=False), wide, ("wide", kind, n), trace=False)
            assert_equal(probe(be, dp, sub, schedule=2, trace=False, P=2), wide, ("wide, P = 2", kind, n), trace=False)
            assert_equal(probe(be, dp, sub, schedule=2, trace=True), narrow, ("wide asked for, with trace", kind, n))


@pytest.mark.parametrize("kind,key", KINDS)
def test_transcript_ops_inside_the_vm(be, kind, key):   # noqa: F811
    """(e): READ_POINT, READ_SCALAR, ABSORB_REG (of 0, r - 1 and a computed value), ABSORB_CI and SQUEEZE interleaved; the hashed
    stream ends 127, 0 and 1 bytes into a block at a squeeze, the halves from_uniform_bytes reduces fall in all three ranges
    (tests/test_vm_programs.py asserts both); 150 proofs, on 4 lanes in LDS and on the global-register-file kernel.  Then the same
    batch with the proof in the middle one byte short: it has exactly H2V_ST_SHORT_PROOF, and every other proof's challenges
    are what they were."""
    batch = A.transcript_batch()
    mid = batch.n // 2
    short = A.VmBatch(list(batch.proofs), batch.instances, batch.committed)
    short.proofs[mid] = short.proofs[mid][:-1]
    want = None
    for L, n_regs in A.TRANSCRIPT_LAYOUTS:
        pl = A.transcript_program(L, kind, key, n_regs=n_regs)
        want = want or model(pl, batch)          # (the same registers in both layouts)
        with loaded(be, pl) as dp:
            full = probe(be, dp, batch)
            cut = probe(be, dp, short)
        assert_equal(full, want, ("transcript", L, kind))
        assert cut[0] == [A.ST_SHORT_PROOF if i == mid else 0 for i in range(batch.n)]
        want_cut = list(want)
        want_cut[mid] = (A.ST_SHORT_PROOF,) + want[mid][1:]
        assert_equal(cut, want_cut, ("transcript, one short proof", L, kind), skip=(mid,))
        for i in range(batch.n):
            if i != mid:
                assert cut[1][i] == full[1][i] and cut[2][i] == full[2][i], i
