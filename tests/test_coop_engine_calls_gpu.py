"""Single calls of the cooperative pairing engine on the device (h2v_probe_coop_call -> k_probe_coop*, csrc/h2v_pairing_coop.hpp: the
functions the pairing kernels themselves call, behind the same set-up helpers) against the limb model of tests/coop_engine_model.py,
on the tables of tests/coop_engine_cases.py, in all four engine shapes: normal (two lanes per coefficient), wide (four - the engine
of the single pairing every batch-accept form rests on), narrow (one) and twelve (the narrow engine, five proofs per wave).
Operands sit ON the bounds of the headroom note - every coefficient at 6p - 1 (CONJ, INV: 5p - 1), at all lower limbs 2^28 - 1, 0, the
Montgomery one, p - 1, one coefficient on the bound and the rest zero (a term taken by the wrong lane shows), line constants and points
at p - 1 and at all-limbs-max below p.  A whole pairing's ~550 calls see only what its chain happens to produce.

Exact comparison, limb for limb, for MUL, SQR, CSQR runs, LINE1 / LINE2, PROD, ROUND and CONJ: results are carried, so limbs and
integer determine each other.  FROB and INV are held to bls12_381's residues, carried, inside the shape's bound.  Every op runs at
1, G, G + 1 and 2G + 1 groups (G groups per wave) with its hardest case in group 0, in the last group of a full wave and in the lone
group of a trailing wave, a distinct case in every other group; the probe's outputs are preset to 0xA5 with a block's worth of guard
records, so what a dead group, a spare lane or lanes 60..63 of the twelve shape wrote would show."""
import ctypes as C

import pytest

from tests import coop_engine_cases as S
from tests import coop_engine_model as M

pytestmark = pytest.mark.gpu
P = M.P
E_ARG = -1


@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


def launch(be, shape, op, order, ls, csqr_n=0):
    """one probe launch: group j runs case order[j]"""
    cases = [S.cases(op)[k] for k in order]
    a = [M.vecs(c["a"]) for c in cases]
    b = pts = flags = lines = None
    if op == "MUL":
        b = [M.vecs(c["b"]) for c in cases]
    if op in ("LINE1", "LINE2"):
        b = [M.vecs(c["T"]) + [[0] * 14] * 8 for c in cases]
    if op in ("LINE1", "LINE2", "PROD", "ROUND"):
        pts = [M.vecs(c["pts"]) for c in cases]
        l1_0, l1_1, l2_0 = S.line_sets()[ls]
        lines = [M.vecs(l1_0), M.vecs(l1_1), M.vecs(l2_0), [[0] * 14] * 8]
    if op in ("LINE1", "LINE2", "ROUND"):
        flags = [c["flags"] for c in cases]
    return be.probe_coop_call(shape, getattr(be, "COOP_" + op), a, b=b, pts=pts, flags=flags, lines=lines, csqr_n=csqr_n)


def check_exact(be, shape, op, n_cases=None, csqr_n=0):
    for n, order, ls in S.launches(shape, n_cases or len(S.cases(op))):
        r = launch(be, shape, op, order, ls, csqr_n)
        for j, k in enumerate(order):
            where = "%s %s, %d groups, group %d (case %d, line set %d)" % (shape, op, n, j, k, ls)
            want, spare, _ = S.expected(op, shape, k, ls, csqr_n)
            for q, (got, w) in enumerate(zip(r.parts[j], M.vecs(want))):
                assert got == w, "%s, part %d: %x against the model's %x" % (where, q, M.limbs_val(got), M.limbs_val(w))
            assert len(r.parts[j]) == len(want)
            if spare is not None:
                assert r.spare[j] == M.vecs(spare), "the spare lanes' T slots: " + where
            else:
                assert r.spare is None
            assert r.lanes_agree[j], "the lanes of a pair or quad returned different limbs: " + where
            assert r.ok[j] == 1
        assert r.guard_clean, "%s %s, %d groups: something was written outside the live groups' records" % (shape, op, n)


@pytest.mark.parametrize("op", ["MUL", "SQR", "LINE1", "LINE2", "ROUND", "CONJ"])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_call_equals_the_limb_model(be, shape, op):
    check_exact(be, shape, op)


def test_twelve_product_pass_equals_the_limb_model(be):
    check_exact(be, "twelve", "PROD")


@pytest.mark.parametrize("n_sqr", S.CSQR_RUNS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_squaring_run_equals_the_limb_model(be, shape, n_sqr):
    """coop_csqr n times, the value in registers between the calls as COOP_OP_CSQR and EXPX keep it, against the model chained n times
    through its own restaging.  The two long runs take the first CSQR_LONG elements alone - the corners and a cyclotomic element,
    which tests/test_coop_engine_model.py holds to f12_sqr as well."""
    check_exact(be, shape, "CSQR", n_cases=S.CSQR_LONG if n_sqr > S.CSQR_RUNS[3] else None, csqr_n=n_sqr)


@pytest.mark.parametrize("op", ["FROB", "INV"])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_frobenius_and_inverse_residues_and_bounds(be, shape, op):
    """FROB: v <= 5; INV: an engine product's bound for the shape (csrc/h2v_pairing_coop.hpp); both carried.  INV of zero: ok = 0."""
    bound = 5 * P if op == "FROB" else M.stated_bound("MUL", shape)
    for n, order, ls in S.launches(shape, len(S.cases(op))):
        r = launch(be, shape, op, order, ls)
        for j, k in enumerate(order):
            where = "%s %s, %d groups, group %d (case %d)" % (shape, op, n, j, k)
            want, _, ok = S.expected(op, shape, k)
            assert r.ok[j] == ok, "ok: " + where
            assert r.lanes_agree[j], where
            for q, got in enumerate(r.parts[j]):
                assert max(got[:13]) < 1 << 28, "not carried: %s part %d" % (where, q)
                assert M.limbs_val(got) < bound, "outside the stated bound: %s part %d" % (where, q)
                if ok:
                    assert M.limbs_val(got) % P == want[q], "residue: %s part %d" % (where, q)
        assert r.guard_clean, "%s %s, %d groups" % (shape, op, n)


def test_bad_arguments_are_refused(be):
    L = be.lib()
    buf = (C.c_uint32 * (12 * 14))()
    small = (C.c_uint32 * (32 * 14))()
    out = (C.c_uint32 * ((1 + be.PROBE_COOP_GUARD) * 224))()
    ok = (C.c_uint32 * ((1 + be.PROBE_COOP_GUARD) * 2))()
    flags = (C.c_uint32 * 1)()

    def call(op, engine=0, n=1, csqr_n=0, a=buf, b=None, pts=None, fl=None, lines=None, o=out, k=ok):
        return L.h2v_probe_coop_call(0, engine, op, n, csqr_n, a, b, pts, fl, lines, o, k)
    assert call(be.COOP_CONJ) == 0                                     # (the same call with nothing missing runs)
    assert call(be.COOP_CONJ, engine=4) == E_ARG and call(be.COOP_CONJ, engine=-1) == E_ARG
    assert call(be.COOP_CONJ, n=0) == E_ARG
    assert call(be.COOP_INV + 1) == E_ARG and call(-1) == E_ARG        # unknown op
    assert call(be.COOP_CSQR, csqr_n=0) == E_ARG and call(be.COOP_CSQR, csqr_n=65) == E_ARG
    for engine in (0, 1, 2):
        assert call(be.COOP_PROD, engine=engine, pts=small, lines=small) == E_ARG          # the twelve shape alone
    assert b"twelve" in L.h2v_last_error()
    assert call(be.COOP_CONJ, a=None) == E_ARG and call(be.COOP_CONJ, o=None) == E_ARG and call(be.COOP_INV, k=None) == E_ARG
    assert call(be.COOP_MUL) == E_ARG                                  # no b
    assert call(be.COOP_LINE1, b=buf, pts=small, lines=small) == E_ARG                     # no flags
    assert call(be.COOP_LINE2, pts=small, lines=small, fl=flags) == E_ARG                  # no T slots
    assert call(be.COOP_LINE1, b=buf, lines=small, fl=flags) == E_ARG and call(be.COOP_LINE1, b=buf, pts=small, fl=flags) == E_ARG
    assert call(be.COOP_PROD, engine=3, pts=small) == E_ARG and call(be.COOP_PROD, engine=3, lines=small) == E_ARG
    assert call(be.COOP_ROUND, pts=small, lines=small) == E_ARG        # no flags
    assert b"missing" in L.h2v_last_error()
