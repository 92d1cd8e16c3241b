"""The integer model of the bucket MSM's bookkeeping (tests/pip_model.py) against the rules the comments of
csrc/h2v_pippenger.hpp promise: the launcher's shape, the signed-digit recoding, and above all the size classes - every
non-empty bucket gets enough lanes for chains of at most T entries, empty buckets get none, and the lane ranges of the classes
are disjoint and 256-aligned.  No GPU: tests/test_bucket_msm_shapes_gpu.py compares the device's tables with the same model."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import pip_model as M

R = bls.R


def test_shape_model():
    """pip_shape: at least 24 entries per bucket on average, widths below 7 widened until the windows fit, forced values."""
    assert M.shape(3000, 2) == (8, 17, 128, 20)          # the two problems of a mixed launch in the GPU tests
    assert M.shape(40, 1) == (7, 19, 64, 20)
    assert M.shape(1, 2) == (7, 19, 64, 20)
    assert M.shape(600000, 2) == (10, 13, 512, 20)
    assert M.shape(24 * 256 // 2, 2)[0] == 9 and M.shape(24 * 256 // 2 - 1, 2)[0] == 8      # the border of the average
    for forced, want in ((3, 7), (4, 7), (5, 7), (6, 7), (7, 7), (8, 8), (9, 9), (10, 10), (2, 10), (11, 10), (0, 10)):
        c, W, NB, chain = M.shape(10 ** 6, 2, forced_c=forced)
        assert (c, W, NB) == (want, 128 // want + 1, 1 << (want - 1)) and W <= M.MAX_W and W * c > 128 and chain == 20
    assert M.shape(300, 2, forced_c=8)[1] == 17 and 128 - 16 * 8 == 0     # the top window of c = 8 holds the carry alone
    for forced, want in ((0, 20), (1, 20), (2, 2), (64, 64), (1024, 1024), (1025, 20)):
        assert M.shape(300, 2, forced_chain=forced)[3] == want


def test_recoding_model_digits_and_counts():
    lam = bls.GLV_LAMBDA
    edge = [0, 1, R - 1, lam, lam - 1, lam + 1, (1 << 128) - 1, 1 << 128, (1 << 255) % R, R - lam]
    rng = random.Random(3)
    scalars = edge + [rng.randrange(R) for _ in range(100)]
    for c in (7, 8, 9, 10):
        W, NB = 128 // c + 1, 1 << (c - 1)
        for s in scalars:
            rows = M.digits(s, 2, c, W)
            k1, k2 = (sum(d << (w * c) for w, d in enumerate(row)) for row in rows)
            assert (k1 + k2 * lam - s) % R == 0
            # the recoding never produces -NB: raw > NB turns into raw - 2 NB >= -(NB - 1)
            assert all(-(NB - 1) <= d <= NB for row in rows for d in row)
        # a small scalar is one entry of bucket (window 0, d): what the size-class tests build their counts from
        for d in range(1, NB + 1):
            assert bls.glv_split(d) == (d, 0)
            for halves in (1, 2):
                assert M.digits(d, halves, c, W) == [[d] + [0] * (W - 1)] + [[0] * W] * (halves - 1)
        # 2^128 - 1 as one half: -1, zeros, and the carry in the top window
        top = M.recode((1 << 128) - 1, c, W)
        assert top[0] == -1 and not any(top[1:-1]) and top[-1] == (1 << (128 - c * (W - 1)))
        # zero scalars and infinity bases are skipped; everything else counts one entry per non-zero digit
        live = [i % 7 != 3 for i in range(len(scalars))]
        cnts = M.counts(scalars, live, 2, c, W)
        assert len(cnts) == W * NB
        assert sum(cnts) == sum(1 for s, a in zip(scalars, live) if a and s for row in M.digits(s, 2, c, W) for d in row if d)
        assert M.counts([0, 5, 5], [True, False, True], 1, c, W) == [0] * 4 + [1] + [0] * (W * NB - 5)


def _lanes(cnts, cls):
    return [None if k is None else 1 << k for k in M.bucket_class(cnts, cls)]


def _check_layout(cnts, cls):
    """empty buckets get no lane, every other bucket is in exactly one class, and the classes' lane ranges are 256-aligned,
    disjoint, laid out from k = 8 down and wide enough for their members"""
    nonempty = sum(1 for cv in cnts if cv)
    assert cls[0] <= cls[1] == nonempty                      # class 0 ends the ranks: exactly the non-empty buckets
    lane, first = 0, 0
    for k in range(M.N_CLASSES - 1, -1, -1):
        f, e, base = cls[3 * k:3 * k + 3]
        assert f == first and e >= f and base == lane and base % 256 == 0
        lane = base + ((((e - f) << k) + 255) & ~255)
        first = e
    assert cls[3 * M.N_CLASSES] == lane
    kinds = M.bucket_class(cnts, cls)
    assert all((k is None) == (cv == 0) for k, cv in zip(kinds, cnts))
    for k in range(M.N_CLASSES):
        assert sum(1 for q in kinds if q == k) == cls[3 * k + 1] - cls[3 * k]
    assert len(M.block_classes(cls)) * 256 == lane


@pytest.mark.parametrize("chain", [2, 3, 20, 31])
def test_size_classes_give_every_lane_a_chain_of_at_most_T(chain):
    """Chains up to 31 (T 2^7 < 4095, so the histogram resolves every border): a bucket of at most 256 T entries has
    lanes x T >= count, and exactly the class the comment states: count in (T 2^(k-1), T 2^k] -> 2^k lanes."""
    T = chain
    rng = random.Random(chain)
    borders = [0, 1] + [v for k in range(9) for v in (T << k, (T << k) + 1, (T << k) - 1)] + [4094, 4095, 4096, 5000, 256 * T, 256 * T + 1]
    for trial in range(4):
        cnts = borders + [rng.randrange(0, 300 * T) for _ in range(200)] + [0] * 50 + [rng.randrange(0, 2 * T) for _ in range(300)]
        cnts = [max(cv, 0) for cv in cnts]
        rng.shuffle(cnts)
        cls = M.classes(cnts, T)
        _check_layout(cnts, cls)
        for cv, lanes in zip(cnts, _lanes(cnts, cls)):
            if cv == 0:
                assert lanes is None
                continue
            if cv <= 256 * T:
                assert lanes * T >= cv
            want = next((k for k in range(8) if cv <= T << k), 8)
            assert lanes == 1 << want, (cv, lanes)


@pytest.mark.parametrize("chain", [32, 64, 1024])
def test_size_classes_beyond_the_histogram(chain):
    """A forced chain above 31 puts T 2^(k-1) beyond the histogram for the top classes: they start at 4095 entries instead -
    longer chains than T, never a bucket without a lane - and the borders below 4095 hold as stated."""
    T = chain
    cnts = [0, 1, 2048, 2049, 4094, 4095, 4096, 9000, 0, T, T + 1, 2 * T, 2 * T + 1, 40000]
    cls = M.classes(cnts, T)
    _check_layout(cnts, cls)
    for cv, lanes in zip(cnts, _lanes(cnts, cls)):
        if cv == 0:
            assert lanes is None
            continue
        if cv >= 4095:
            assert lanes == 256
        # the largest class whose lower border - T 2^(k-1), read as 4094 where it is beyond the histogram - the count exceeds
        want = max(k for k in range(9) if cv > min(0 if k == 0 else T << (k - 1), 4094))
        assert lanes == 1 << want, (cv, lanes)
        if cv <= 2048:
            assert lanes * T >= cv


def test_size_classes_of_an_empty_and_a_uniform_table():
    assert M.classes([0] * 1216, 20) == [0] * M.CLS_DW
    cls = M.classes([7] * 1216, 20)                           # the usual case: everything in class 0
    assert cls[0:3] == [0, 1216, 0] and cls[27] == 1280 and M.block_classes(cls) == [0] * 5
    cls = M.classes([21] * 3, 20)
    assert cls[3:6] == [0, 3, 0] and cls[0:3] == [3, 3, 256] and cls[27] == 256
