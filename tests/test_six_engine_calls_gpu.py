"""Single calls of the six-lane pairing engine on the device (h2v_probe_six_call -> k_probe_six, csrc/h2v_pairing_six.hpp: the
out-of-line functions the pairing itself calls) against the limb model of tools/gen_six_tables.py, on the tables of
tests/six_engine_cases.py: operands ON the bounds of the headroom argument - MUL at 6p - 1, the Miller loop's squaring and lines at
(12p, 7p) with products at 2p - 1, the squaring's fold inputs uncarried up to 2^31 - 1 and 32p - 1.  A whole pairing's ~550 calls see
only what its chain happens to produce; here every call is held to the model where the argument is tight.

Exact comparison, limb for limb: results are carried, so limbs and integer determine each other.  FROB and INV are held to
bls12_381's residues, and every part must be carried and inside the bound the header states.  Every op runs at 1, 10, 11 and 21
groups with its hardest case in group 0, in group 9 (the group lanes 60..63 shadow) and in the lone group of a trailing wave, a
distinct case in every other group of a block; the probe's outputs are preset to 0xA5 with a block's worth of guard records."""
import ctypes as C

import pytest

from tests import six_engine_cases as S

pytestmark = pytest.mark.gpu
P, g = S.P, S.g
E_ARG = -1


@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


def vecs(pairs):
    return [S.limbs(v) for v in S.flat(pairs)]


def launch(be, op, table, order, csqr_n=0):
    """one probe launch: group j runs case order[j]"""
    cases = [table["cases"][k] for k in order]
    code = getattr(be, "SIX_" + op)
    a = [c["a"] if op == "FOLD" else vecs(c["a"]) for c in cases]
    b = pts = flags = lines = None
    if op == "MUL":
        b = [vecs(c["b"]) for c in cases]
    if op in ("LINE1", "LINE2"):
        b = [[S.limbs(v) for v in c["T"]] + [[0] * 14] * 4 for c in cases]
    if op in ("PROD2", "ROUND"):
        pts = [[S.limbs(v) for v in c["pts"]] for c in cases]
        lines = [S.limbs(v) for v in table["lines"]]
    if op in ("LINE1", "LINE2", "ROUND"):
        flags = [c["flags"] for c in cases]
    return cases, be.probe_six_call(code, a, b=b, pts=pts, flags=flags, lines=lines, csqr_n=csqr_n)


def check_exact(be, op, table, sizes=S.SIZES, csqr_n=0):
    for n, order in S.launches(len(table["cases"]), sizes):
        cases, r = launch(be, op, table, order, csqr_n)
        for j, c in enumerate(cases):
            want = c["want"][csqr_n] if op == "CSQR" else c["want"]
            want = want if op == "FOLD" else [S.limbs(v) for v in want]
            for q, (got, w) in enumerate(zip(r.parts[j], want)):
                assert got == w, "%s, %d groups, group %d (case %d), part %d: %x against the model's %x" % (
                    op, n, j, order[j], q, g.limbs_val(got), g.limbs_val(w))
        assert r.guard_clean, "%s, %d groups: something was written outside the live groups' records" % (op, n)


@pytest.mark.parametrize("op", ["MUL", "SQR", "LINE1", "LINE2", "PROD2", "ROUND", "CONJ", "FOLD"])
def test_call_equals_the_limb_model(be, op):
    check_exact(be, op, S.table(op))


@pytest.mark.parametrize("n_sqr", S.CSQR_RUNS)
def test_squaring_run_equals_the_limb_model(be, n_sqr):
    """six_csqr_run: n squarings as one call, against the model's csqr_engine chained n times through the integer forms of the run's
    restaging.  The two long runs take the first CSQR_LONG elements (the corners and a cyclotomic element) alone, so their blocks
    repeat elements."""
    t = S.table("CSQR")
    if n_sqr > S.CSQR_RUNS[3]:
        check_exact(be, "CSQR", {"cases": t["cases"][:S.CSQR_LONG], "lines": None}, csqr_n=n_sqr)
    else:
        check_exact(be, "CSQR", t, csqr_n=n_sqr)


@pytest.mark.parametrize("op", ["FROB", "INV"])
def test_frobenius_and_inverse_residues_and_bounds(be, op):
    """FROB: v <= 5; INV: the engine products' below 3p (csrc/h2v_pairing_six.hpp); both carried.  INV of zero: ok = 0."""
    table = S.table(op)
    bound = 5 * P if op == "FROB" else 3 * P
    for n, order in S.launches(len(table["cases"])):
        cases, r = launch(be, op, table, order)
        for j, c in enumerate(cases):
            where = "%s, %d groups, group %d (case %d)" % (op, n, j, order[j])
            for q, (got, w) in enumerate(zip(r.parts[j], c["want"])):
                assert max(got) < 1 << 28, "not carried: %s part %d" % (where, q)
                assert g.limbs_val(got) < bound, "outside the stated bound: %s part %d" % (where, q)
                assert g.limbs_val(got) % P == w, "residue: %s part %d" % (where, q)
            if op == "INV":
                assert r.ok[j] == c["ok"], "ok: " + where
        assert r.guard_clean, "%s, %d groups" % (op, n)


def test_bad_arguments_are_refused(be):
    L = be.lib()
    buf = (C.c_uint32 * (12 * 14))()
    small = (C.c_uint32 * (8 * 14))()
    out = (C.c_uint32 * ((1 + be.PROBE_SIX_GUARD) * 168))()
    ok = (C.c_uint32 * (1 + be.PROBE_SIX_GUARD))()
    flags = (C.c_uint32 * 1)()

    def call(op, n=1, csqr_n=0, a=buf, b=None, pts=None, fl=None, lines=None, o=out, k=ok):
        return L.h2v_probe_six_call(0, op, n, csqr_n, a, b, pts, fl, lines, o, k)
    assert call(be.SIX_CONJ) == 0                                      # (the same call with nothing missing runs)
    assert call(be.SIX_CONJ, n=0) == E_ARG
    assert call(be.SIX_FOLD + 1) == E_ARG and call(-1) == E_ARG        # unknown op
    assert call(be.SIX_CSQR, csqr_n=0) == E_ARG
    assert call(be.SIX_CONJ, a=None) == E_ARG and call(be.SIX_CONJ, o=None) == E_ARG
    assert call(be.SIX_MUL) == E_ARG                                   # no b
    assert call(be.SIX_LINE1, b=buf) == E_ARG and call(be.SIX_LINE2, fl=flags) == E_ARG      # no flags / no T slots
    assert call(be.SIX_PROD2, pts=small) == E_ARG and call(be.SIX_PROD2, lines=small) == E_ARG
    assert call(be.SIX_ROUND, pts=small, lines=small) == E_ARG         # no flags
    assert call(be.SIX_INV, k=None) == E_ARG
    assert b"missing" in L.h2v_last_error()
