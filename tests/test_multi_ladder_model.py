"""The multi-term MSM ladder (k_g1_msm_multi), what can be said without a GPU.

  * The lane shape of its launch (csrc/h2v_msm_shape.hpp: msm_multi_shape) over everything the launcher admits, printed by a host
    program under ASan + UBSan: the bounds the kernel's arrays and its block rely on, and the dealing of tests/multi_ladder_model.py.
  * The model's crafted cases - the inputs of tests/test_msm_multi_ladder_gpu.py - are what they claim: every targeted exceptional
    addition is an event of its lane, the honest controls have none, and the oracle's sum over the actual points is
    [sum s_t b_t] G.
  * Why test_gpu_parity.py::test_g1_msm[_forced_shape] is not enough: on its inputs the unchecked ladder meets an exceptional
    addition only in windows 32 and 31, on the second term's slots."""
import os
import random
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import multi_ladder_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bls.R
SHAPES = [(hpl, T) for hpl in range(3, M.MAX_HALVES + 1) for T in M.gpu_shapes(hpl)]


def test_multi_shape_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_msm_multi_shape.cpp: host code only, its own main, built with ASan + UBSan and run as a program"""
    out = str(tmp_path / "h2v_msm_multi_shape")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_msm_multi_shape.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == "max_halves"
    max_halves = int(lines[0].split()[1])
    assert max_halves == M.MAX_HALVES
    seen, want_lines = set(), 0
    for T in range(2, 1025):
        for tpl in (2, 3, 4):
            want_lines += 2 * (tpl <= T <= 256 * tpl)
    assert len(lines) - 1 == want_lines
    for line in lines[1:]:
        (T, tpl, forced), (hpl, lpp) = (tuple(int(v) for v in part.split()) for part in line.split(" : "))
        assert tpl <= T <= 256 * tpl, line
        assert 3 <= hpl <= max_halves, line
        assert lpp * hpl >= 2 * T > (lpp - 1) * hpl, line           # no lane is empty
        assert lpp <= 256, line
        assert not forced or hpl == 2 * tpl, line
        assert (hpl, lpp) == M.shape(T, tpl, bool(forced)) and lpp == M.lanes_per_proof(T, hpl), line
        # the model's deal of that shape: every half in exactly one slot, the last lane not empty
        if T <= 64:
            dealt = [s for ln in range(lpp) for s in M.lane_slots(T, hpl, ln) if s[0] < T]
            assert dealt == [(t, h) for t in range(T) for h in (0, 1)] and M.lane_terms(T, hpl, lpp - 1), line
        seen.add(hpl)
    assert seen == {3, 4, 5, 6, 7, 8}
    # the examples of the odd shapes
    assert M.shape(10, 3, False)[0] == 5 and M.shape(13, 4, False)[0] == 7 and M.shape(17, 4, False)[0] == 7


def test_recoding_and_split_are_the_kernels():
    rng = random.Random(1)
    lam = bls.GLV_LAMBDA
    for k in [0, 1, 8, 9, 15, 16, lam - 1, lam, lam + 1, R - 1, (1 << 128) - 1] + [rng.randrange(R) for _ in range(200)]:
        k1, k2 = bls.glv_split(k % R)
        for half in (k1, k2):
            dg = M.recode4(half)
            assert len(dg) == 33 and all(-8 <= d <= 8 for d in dg) and dg[32] in (0, 1)
        assert (k1 + k2 * lam) % R == k % R
    assert M.recode4(9)[:2] == [-7, 1] and M.recode4(8)[:2] == [8, 0] and M.recode4((1 << 128) - 1)[32] == 1


@pytest.fixture(scope="module")
def all_cases():
    return {(hpl, T): M.cases(hpl, T) for hpl, T in SHAPES}


def test_the_shapes_are_the_ones_asked_for():
    for hpl in range(3, 9):
        T11, full, one = M.gpu_shapes(hpl)
        assert T11 == 11 and M.lanes_per_proof(11, hpl) >= 3 and 22 % hpl != 0
        assert 2 * full % hpl == 0 and M.lanes_per_proof(one, hpl) == 1 and 2 * (one + 1) > hpl
        if hpl & 1:   # terms that straddle two lanes, lanes that begin on a k2 half
            assert any(M.lane_slots(11, hpl, ln)[0][1] == 1 for ln in range(1, M.lanes_per_proof(11, hpl)))


@pytest.mark.parametrize("hpl", range(3, 9))
def test_case_list_holds_what_the_device_test_needs(all_cases, hpl):
    cs = all_cases[(hpl, 11)]
    names = {c.name for c in cs}
    assert len(names) == len(cs)
    crafted = [c for c in cs if c.targets]
    single = [c for c in crafted if c.name[:4] in ("dbl-", "inv-") and "-w" in c.name and len(c.targets) == 1]
    ev = M.eventful_lanes(11, hpl)
    for kind in ("dbl", "inv"):
        for q in (32, 31, 16, 1, 0):
            mine = [c.targets[0] for c in single if c.targets[0][3] == kind and c.targets[0][1] == q]
            lanes = {t[0] for t in mine}
            # the first lane, a middle one, the last lane that two terms share (the partly filled last lane where it has two)
            assert ev[0] in lanes and ev[-1] in lanes and len(lanes) == 3
            for ln in lanes:
                slots = {t[2] for t in mine if t[0] == ln}
                assert M.earliest_slot(11, hpl, ln, q) in slots and M.last_used_slot(11, hpl, ln) in slots
                assert q == 32 or 1 in slots
            if hpl & 1:    # slot 1 of a lane whose slot 0 is a k2 half
                assert any(t[2] == 1 and M.lane_slots(11, hpl, t[0])[0][1] == 1 for t in mine)
    if M.lanes_per_proof(11, hpl) - 1 in ev:
        assert hpl in (6, 8)
    assert "inv-last-addition-every-lane" in names and any(n.startswith("inv-last-addition-lane") for n in names)
    assert any(n.startswith("restart-w16") for n in names)
    # two events in one lane and unused slots in front of an event need a lane of three terms (the model's docstring)
    assert any(n.startswith("two-events") for n in names) == (hpl >= 5)
    assert ("unused-slots-before-the-event" in names) == (hpl >= 5)
    for c in crafted:
        if c.name.startswith("unused"):
            kinds = set()
            for ln in c.crafted_lanes():
                first = min(j for _, q, j, _ in [t for t in c.targets if t[0] == ln])
                before = [t for t, _ in M.lane_slots(11, hpl, ln)[:first]]
                kinds |= {"zero" for t in before if c.scalars[t] == 0} | {"inf" for t in before if c.logs[t] is None}
                t0 = M.lane_slots(11, hpl, ln)[0][0]
                assert c.scalars[t0] == 0 or c.logs[t0] is None      # slot 0 itself is unused: the ladder starts later
            assert kinds == {"zero", "inf"}
        if c.name.startswith("two-events"):
            assert len(c.targets) == 2 and len(c.crafted_lanes()) == 1
        if c.name.startswith("restart"):
            ln, q, j, kind = c.targets[0]
            digits = M.lane_digits(c.scalars, c.logs, hpl, ln)
            assert kind == "inv" and q == 16 and any(dg[w] for _, _, dg in digits for w in range(16)) and c.events(ln)[1] != 0
    # every crafted case has its control
    assert {c.control_of for c in cs if c.control_of} == {c.name for c in crafted}


@pytest.mark.parametrize("hpl,T", SHAPES)
def test_cases_are_what_they_claim(all_cases, orc, hpl, T):
    lanes = range(M.lanes_per_proof(T, hpl))
    for c in all_cases[(hpl, T)]:
        assert c.T == T and c.hpl == hpl
        found = {ln: c.events(ln) for ln in lanes}
        if c.honest:
            assert not any(ev for ev, _ in found.values()), c.name
        for ln, q, j, kind in c.targets:
            assert (q, j, kind) in found[ln][0], c.name
            if c.name.startswith("inv-last-addition"):
                assert found[ln][1] == 0 and found[ln][0][-1] == (0, M.last_used_slot(T, hpl, ln), "inv"), c.name
        # lanes beside the crafted ones are honest
        assert all(not found[ln][0] for ln in lanes if ln not in c.crafted_lanes()), c.name
        assert sum(s for _, s in found.values()) % R == c.sum_log(), c.name
        if c.name == "inv-last-addition-every-lane":
            assert all(s == 0 for _, s in found.values()) and c.sum_is_infinity
        # the data are what they claim: the oracle's sum over the actual points is [sum s_t b_t] G
        want = bls.g1_mul(bls.G1_GEN, c.sum_log())
        assert orc.g1_msm(c.scalars, c.points()) == want, c.name
        assert (want is None) == c.sum_is_infinity


def test_an_event_needs_two_terms():
    """what the model's docstring says cannot be built: craft raises instead of skipping"""
    rng = random.Random(2)
    scalars, logs = [rng.randrange(1, R) for _ in range(11)], list(M.POOL_LOGS[:11])
    with pytest.raises(ValueError):      # hpl = 4, last lane of T = 11: term 10 alone
        M.craft(scalars, logs, 4, [(5, 16, 1, "inv")], rng, tries=50)
    with pytest.raises(ValueError):      # window 32, slot 1 of a lane that starts on a k1 half: slots 0 and 1 are one term
        M.craft(scalars, logs, 4, [(0, 32, 1, "dbl")], rng, tries=300)
    assert M.earliest_slot(11, 4, 0, 32) == 2 and M.earliest_slot(11, 3, 1, 32) == 1


def _parity_inputs():
    """the scalars and the discrete logs of test_gpu_parity.py::test_g1_msm: the same random.Random(4) draws in the same order"""
    rng = random.Random(4)
    lam = bls.GLV_LAMBDA
    for T in (1, 2, 5, 16, 34, 58, 64):
        for g in range(5):
            logs = [rng.randrange(1, R) for _ in range(T)]
            ss = [rng.randrange(R) for _ in range(T)]
            if g == 1:
                ss[0] = 0
                ss[-1] = R - 1
            if g == 2 and T >= 2:
                logs[1], ss[1] = logs[0], ss[0]
            if g == 3 and T >= 2:
                logs[1], ss[1] = R - logs[0], ss[0]
            if g == 4:
                logs[0] = None
                edge = [1, 2, 7, 8, 9, 15, 16, 17, lam - 1, lam, lam + 1, 2 * lam, R - lam, (1 << 128) - 1, 1 << 128,
                        (1 << 255) % R, 0x8888888888888888888888888888888888888888888888888888888888888888 % R]
                for t in range(1, T):
                    ss[t] = edge[(t - 1) % len(edge)]
            yield T, g, ss, logs


def test_parity_inputs_reach_only_the_top_windows_of_the_second_term():
    """test_g1_msm under tpl2 / tpl3 / tpl4 (test_g1_msm_forced_shape): the exceptional additions the unchecked ladder runs - the
    FIRST event of a lane - lie in windows 32 and 31, in lane 0, on slots 2 and 3 (the second term's); doublings come from the
    equal-bases group alone, only for T = 58 and 64, in window 32, where the accumulator is an entry just loaded (Z = 1); no
    other group has an event at all.  Nothing there reaches an event deep in the ladder, on the last addition, on a third or fourth
    term's slot or in an odd lane shape: tests/test_msm_multi_ladder_gpu.py does."""
    first_events, dbl_T = [], set()
    for T, g, ss, logs in _parity_inputs():
        for tpl in (2, 3, 4):
            if T < tpl:
                continue
            hpl = 2 * tpl
            for ln in range(M.lanes_per_proof(T, hpl)):
                ev, _ = M.events(ss, logs, hpl, ln)
                if not ev:
                    continue
                assert g in (2, 3) and ln == 0, (T, g, tpl, ln, ev)
                assert all(j in (2, 3) for _, j, _ in ev), (T, g, tpl, ev)
                assert all(kind == ("dbl" if g == 2 else "inv") for _, _, kind in ev)
                first_events.append((T, g, tpl, ev[0]))
                if g == 2:
                    dbl_T.add(T)
                    assert all(q == 32 for q, _, _ in ev), (T, tpl, ev)
    assert first_events
    assert all(ev[0] in (32, 31) for _, _, _, ev in first_events), first_events
    assert dbl_T == {58, 64}
    assert {T for T, g, _, _ in first_events if g == 3} >= {2, 5, 16, 34, 58, 64}
