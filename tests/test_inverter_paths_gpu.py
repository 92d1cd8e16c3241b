"""The division-step inverter (csrc/h2v_modinv.hpp) on the device, on operands chosen by the way they leave it.

k_probe_field and READ_SCALAR bring their canonical input to Montgomery form before fp_inv / fr_inv run, so the inverter works on
a 2^k mod M (k = 392 for Fp, 256 for Fr).  To put a chosen integer X into it, the tests pass a = X 2^-k mod M - and assert that
mapping - and expect pow(a, M - 2, M), exactly.  The operands: tests/golden/inverter_paths.json (every exit class a seeded search
met: sign of f, +M repairs, final -M, batches) and safegcd_model.structured (powers of two and their neighbours from both ends,
the truncated modulus, zero low limbs, zero high limbs).  The CPU side - the model on the same operands, the labels, the
coverage condition, what the lane arrangements hold - is tests/test_inverter_paths.py.

What these tests cannot see: fp_inv / fr_inv multiply the inverter's output by R^3 at once, and that Montgomery product reduces an
operand in [M, 2M) like one in [0, M) - a missing final -M inside the inverter gives the same field element.  The range [0, M) of
the header's own output is held by the host program of tests/test_inverter_paths.py."""
import pytest

from tests import safegcd_model as S
from tests import vm_asm as A
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_vm_programs_gpu import assert_equal, loaded, model, probe

pytestmark = pytest.mark.gpu
OPS = {"FP": 3, "FR": 5}      # h2v_probe_field: fp_inv, fr_inv
PER_LAUNCH = 512


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


def mapped(xs, name):
    """the probe's inputs for the integers xs (0 stays 0) and the inverses it has to return"""
    fld = S.field(name)
    a = [S.to_probe(x, fld) if x else 0 for x in xs]
    assert all(v * (1 << fld.mont_bits) % fld.mod == x and 0 <= v < fld.mod for v, x in zip(a, xs))
    return a, [pow(v, fld.mod - 2, fld.mod) for v in a]


def run(be, name, xs):   # noqa: F811
    """(index, operand) of every wrong result of one launch"""
    a, want = mapped(xs, name)
    got = be.probe_field(OPS[name], a, [0] * len(a))
    return [(i, hex(xs[i])) for i in range(len(xs)) if got[i] != want[i]]


@pytest.mark.parametrize("name", ["FP", "FR"])
def test_every_fixture_and_structured_operand(be, fixture, name):   # noqa: F811
    """all of them (about 3000 for Fp, 2000 for Fr), a few hundred per launch: the inverse, exactly"""
    xs = [x for x, _ in fixture[name]] + S.structured(name)
    for s in range(0, len(xs), PER_LAUNCH):
        assert run(be, name, xs[s:s + PER_LAUNCH]) == [], (name, "operands from", s)


@pytest.mark.parametrize("name", ["FP", "FR"])
def test_lanes_that_leave_the_loop_at_different_batches(be, fixture, name):   # noqa: F811
    """batches of 64, 65 and 128 (the probe launches blocks of 64): one long-running operand among short ones in lane 0, 31, 63,
    the converse, a zero beside a long-running one and a long-running one alone among zeros, the two-repair and final-subtraction
    operands in lane 0, lane 63 and the lone lane of a ragged last block - every lane's result exact, the zero's 0"""
    for what, xs in S.lane_arrangements(name, fixture):
        assert run(be, name, xs) == [], (name, what)


@pytest.mark.parametrize("L,inv_lane", [(1, 0), (4, 2)])
def test_combiner_inv_on_the_rare_classes(be, fixture, L, inv_lane):   # noqa: F811
    """the production call site: OP_INV of the combiner VM on the proof scalar x (READ_SCALAR converts to Montgomery form, so the
    same mapping holds), every Fr fixture operand and one proof with x = 0 in their middle, at the launcher's proofs per block
    (64 and 16: more than one block, the last one ragged).  Term 0 is the inverse and the status 0; the zero carries
    H2V_ST_INVERSE_OF_ZERO, answers 0 and leaves its neighbours clean."""
    xs = [x for x, _ in fixture["FR"]]
    assert sum(1 for _, c in fixture["FR"] if c[1] == 2) >= 8 and sum(1 for _, c in fixture["FR"] if c[2]) >= 8
    zero_at = len(xs) // 2
    xs.insert(zero_at, 0)
    a, want = mapped(xs, "FR")
    batch = A._batch_of([(v, 0, 0) for v in a], seed=9)
    pl = A.status_program(L, inv_lane=inv_lane)
    with loaded(be, pl) as dp:
        got = probe(be, dp, batch)
    st, sc, _tr = got
    assert st == [A.ST_INVERSE_OF_ZERO if i == zero_at else 0 for i in range(len(xs))]
    assert [s[0] for s in sc] == want and want[zero_at] == 0
    assert_equal(got, model(pl, batch), ("inverse of the rare classes", L))
