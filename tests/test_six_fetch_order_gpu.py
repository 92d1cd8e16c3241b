"""The six-lane pairing engine fetches the NEXT operands while the current product runs (csrc/h2v_pairing_six.hpp: six_issue /
six_arrive): a swapped or stale operand register, or a fetch that stands above a store to its slot, changes the values of a rejecting
pair in all twelve coefficients.  Six kinds of pairs - accepting, two different rejecting ones, first argument at infinity, second at
infinity, both - are replayed ONCE each with big integers (tools/gen_coop_program.py: simulate) and laid out, rotated, in batches of
1, 10, 11 and 21 pairs, so that every kind visits group 0 of a wave, group 9 (the one lanes 60..63 shadow) and the lone live group of a
trailing wave (nine dead groups shadowing it).  Both values the probe dumps - after the Miller loop and after the final
exponentiation - are compared coefficient by coefficient; a loop whose G1 argument is infinity is skipped (the `keep` path: its line
steps run and leave f as staged), so its Miller value is the other loop's alone."""
import pytest

from tests import pairing_kinds as K
from tests.pairing_kinds import ACCEPT, REJECT_A, REJECT_B, INF_1, INF_2, INF_BOTH, N_KINDS

pytestmark = pytest.mark.gpu
IMPL_SIX = 5                              # h2v_probe_pairing_ex: the six-lane kernel
BATCHES = (1, 10, 11, 21)


@pytest.fixture(scope="module")
def simple_mul():
    from plutus_halo2_verifier_gen_amd import backend as be, plan as PL, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    return vk, td, be.DevicePlan(pl.to_bytes(), 0)


@pytest.fixture(scope="module")
def kinds(simple_mul):
    """Per kind: (compressed p1, compressed p2, verdict, Miller value, final value, ...), the values as 12 integers (re, im of
    coefficient 0..5) from the replay: accept <=> e(p1, [s]G2) == e(p2, G2).  tests/pairing_kinds.py builds them."""
    vk, td, dp = simple_mul
    return K.build_kinds(vk, td)


def test_the_six_kinds_are_what_they_are_meant_to_be(kinds):
    one = [1] + [0] * 11
    for k in (REJECT_A, REJECT_B):                      # every lane carries a non-trivial value through the whole program
        assert all(x not in (0, 1) for x in kinds[k][3]) and all(x not in (0, 1) for x in kinds[k][4])
    assert kinds[REJECT_A][4] != kinds[REJECT_B][4]
    assert kinds[ACCEPT][4] == one and all(x not in (0, 1) for x in kinds[ACCEPT][3])
    assert kinds[INF_BOTH][3] == one and kinds[INF_BOTH][4] == one      # both loops skipped: f stays as staged
    for k in (INF_1, INF_2):                            # one loop skipped: the other loop's lines alone
        assert kinds[k][3] != one and kinds[k][4] != one


def test_every_kind_visits_group_0_group_9_and_a_lone_trailing_group():
    seen = {(k, where): False for k in range(N_KINDS) for where in ("group0", "group9", "lone")}
    for n in BATCHES:
        for rot in range(N_KINDS):
            for j in range(n):
                k = (j + rot) % N_KINDS
                if j % 10 == 0:
                    seen[(k, "group0")] = True
                if j % 10 == 9:
                    seen[(k, "group9")] = True
                if j % 10 == 0 and j == n - 1:
                    seen[(k, "lone")] = True
    assert all(seen.values())


@pytest.mark.parametrize("n", BATCHES)
def test_values_and_verdicts_in_every_position(simple_mul, kinds, n):
    from plutus_halo2_verifier_gen_amd import backend as be
    vk, td, dp = simple_mul
    for rot in range(N_KINDS):
        order = [(j + rot) % N_KINDS for j in range(n)]
        acc, dump = be.probe_pairing_ex(dp, [kinds[k][0] for k in order], [kinds[k][1] for k in order], impl=IMPL_SIX)
        assert acc == [kinds[k][2] for k in order], "verdicts, batch %d rotation %d" % (n, rot)
        for j, k in enumerate(order):
            for q in range(12):
                assert dump[j][0][q] == kinds[k][3][q], "Miller value: batch %d rotation %d pair %d kind %d coefficient %d" % (n, rot, j, k, q)
                assert dump[j][1][q] == kinds[k][4][q], "final value: batch %d rotation %d pair %d kind %d coefficient %d" % (n, rot, j, k, q)
