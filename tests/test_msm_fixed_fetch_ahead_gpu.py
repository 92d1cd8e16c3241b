"""The window walk of k_g1_msm_fixed (csrc/h2v_msm.hpp: msm_body, FIX) at its edges - written for a form of the loop that fetches
the table entry of window q - 1 before the addition of window q (built, measured, not shipped): an entry fetched for the
wrong window or digit, one used for a zero digit, or a fetch carried from one base's last window into the next base's first changes
the sum.  The simple_mul plan's six VK bases, sixteen rows of scalars at the edges of the window walk, against
the fold with bls12_381.g1_mul / g1_add; one base per lane and three (a lane walks from one base's last window into the next base's
first), with the shipped 12-bit windows (22 per scalar) and with 4-bit ones (65)."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

pytestmark = pytest.mark.gpu
R = bls.R


def from_digits(digits, c):
    """sum d_q 2^(c q), least significant first: the scalar whose signed c-bit recoding is `digits`"""
    s = sum(d << (c * q) for q, d in enumerate(digits))
    assert 0 <= s < R
    return s


@pytest.fixture(scope="module")
def simple_mul():
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    bases = [pl.vk_bases[idx] for kind, idx in pl.terms if kind == PL.TERM_VK_BASE]
    assert len(bases) == 6
    return pl, bases


@pytest.fixture(scope="module")
def rows_and_sums(simple_mul):
    pl, bases = simple_mul
    rng = random.Random(9)
    rnd = lambda: rng.randrange(1, R)
    top12, top4 = 3 << 252, 5 << 252                      # only the top window: window 21 of 22 (12 bits), 63 of 65 (4 bits)
    alt12 = from_digits([(q % 2) * (1 + q) for q in range(21)], 12)          # zero and non-zero windows in turn
    alt12b = from_digits([((q + 1) % 2) * (2047 - q) for q in range(21)], 12)
    alt4 = from_digits([(q % 2) * (1 + q % 7) for q in range(63)], 4)
    max12, min12 = int("800" * 21, 16), int("800" * 20 + "801", 16)          # every digit + 2048 / every digit - 2047 (and the carry on top)
    max4, min4 = int("8" * 63, 16), int("8" * 62 + "9", 16)
    rows = [
        [0, 1, R - 1, R - 2, rnd(), rnd()],               # r - 2: the last window is a doubling (digit -1 onto the prefix r - 1)
        [R - 2] * 6,
        [0] * 6,
        [rnd(), R - 2, 0, 1, R - 1, rnd()],
        [top12, top4, top12, rnd(), top4, top12],
        [5, 2048, 2047, 8, 7, 1],                         # only window 0
        [2049, 9, 4095, 15, 16, 4096],                    # ... and window 0 with a carry into window 1 alone
        [alt12, alt12b, alt4, alt12, alt4, alt12b],
        [alt12b, rnd(), alt12, alt4, rnd(), alt12],
        [max12, min12, max4, min4, max12, min4],
        [min12, max12, min4, max4, min12, max4],
        [rnd(), 0, rnd(), rnd(), 0, rnd()],               # a zero scalar between two non-zero ones on one lane (three bases per lane)
        [0, rnd(), 0, 0, rnd(), 0],
        [rnd(), rnd(), 0, 0, rnd(), rnd()],
        [top12, 0, 1, R - 2, 0, top4],
        [rnd() for _ in range(6)],
    ]
    assert len(rows) == 16 and all(0 <= s < R for row in rows for s in row)
    sums = []
    for row in rows:
        acc = None
        for s, b in zip(row, bases):
            acc = bls.g1_add(acc, bls.g1_mul(b, s))
        sums.append(acc)
    assert sums[2] is None
    return rows, sums


@pytest.mark.parametrize("window_bits", [0, 4])           # 0: the library's choice (12 bits for this plan)
@pytest.mark.parametrize("bases_per_lane", [1, 3])
def test_fixed_base_sums_equal_the_fold(simple_mul, rows_and_sums, bases_per_lane, window_bits):
    from plutus_halo2_verifier_gen_amd import backend as be
    pl, bases = simple_mul
    rows, sums = rows_and_sums
    dp = be.DevicePlan(pl.to_bytes(), 0, fixed_base_window_bits=window_bits)
    assert be.probe_g1_msm_fixed(dp, None) == 6
    got = be.probe_g1_msm_fixed(dp, rows, bases_per_lane=bases_per_lane)
    for j, (row, r, want) in enumerate(zip(rows, got, sums)):
        assert r == want, "row %d: %s" % (j, [hex(x) for x in row])
