"""The bucket (Pippenger) G1 MSM of csrc/h2v_pippenger.hpp on the device, at the inputs where its data-dependent parts go
wrong: every size class and class border of k_pip_scan, forced window widths and chains, skewed and degenerate digit
distributions, two problems of different shape in one launch, an index map over two pools, and the logical-block walk of
k_pip_accumulate.  All through h2v_probe_g1_msm_pippenger_ex, i.e. the production pip_alloc / pip_launch path.

Reference: the oracle's fold orc.g1_msm over the scalars grouped per distinct base (exact, mod r), as tests/test_rlc.py does it;
the device's tables (shape, bucket counts, order, size classes) against the integer model tests/pip_model.py.  Every comparison
is equality of affine coordinates or of integers.

Bases: P_i = P_0 + i D with P_0 = m_0 G, D = d G (one affine addition each), so the multiplier of P_i is m_0 + i d; the case with
5000 distinct bases uses that identity for its expected sum - one multiplication of G by sum s_i (m_0 + i d) mod r -, which the
fixture checks against the oracle at both ends of the pool."""
import contextlib
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import pip_model as M

pytestmark = pytest.mark.gpu
R = bls.R
INF = bls.g1_compress(None)
LAM = bls.GLV_LAMBDA
EDGE = [0, 1, R - 1, LAM, LAM - 1, LAM + 1, (1 << 128) - 1, 1 << 128, (1 << 255) % R, R - LAM]   # (test_rlc.py's list)


@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


class Pool:
    """k distinct points P_i = (m0 + i d) G as affine pairs and compressed, and their multipliers"""

    def __init__(self, orc, k, seed):
        rng = random.Random(seed)
        m0, d = rng.randrange(1, R), rng.randrange(1, R)
        p, step = orc.g1_msm([m0], [bls.G1_GEN]), orc.g1_msm([d], [bls.G1_GEN])
        self.aff, self.mult = [], []
        for i in range(k):
            self.aff.append(p)
            self.mult.append((m0 + i * d) % R)
            p = bls.g1_add(p, step)
        self.comp = [bls.g1_compress(q) for q in self.aff]
        for i in (0, k // 2, k - 1):
            assert orc.g1_msm([self.mult[i]], [bls.G1_GEN]) == self.aff[i]


@pytest.fixture(scope="module")
def pool(orc):
    return Pool(orc, 300, 1)


def fold(orc, aff, scalars, idx):
    """the oracle's fold after grouping the scalars per distinct base; idx[i] is None for a base at infinity"""
    sums = {}
    for s, j in zip(scalars, idx):
        if j is not None:
            sums[j] = (sums.get(j, 0) + s) % R
    keys = sorted(sums)
    return orc.g1_msm([sums[j] for j in keys], [aff[j] for j in keys]) if keys else None


@contextlib.contextmanager
def forced(be, c=0, chain=0):
    """H2V_OPT_RLC_WINDOW_BITS / H2V_OPT_RLC_CHAIN for the probes of this thread, reset to 0 whatever happens"""
    try:
        be.probe_set_option(be.OPT_RLC_WINDOW_BITS, c)
        be.probe_set_option(be.OPT_RLC_CHAIN, chain)
        yield
    finally:
        be.probe_set_option(be.OPT_RLC_WINDOW_BITS, 0)
        be.probe_set_option(be.OPT_RLC_CHAIN, 0)


def check_tables(dump, scalars, live, halves, forced_c=0, forced_chain=0):
    """the dumped shape, bucket counts, order and size classes against the model; returns the model's counts and classes"""
    c, W, NB, chain = M.shape(len(scalars), halves, forced_c, forced_chain)
    assert (dump["c"], dump["W"], dump["NB"], dump["chain"]) == (c, W, NB, chain)
    cnts = M.counts(scalars, live, halves, c, W)
    off = dump["off"]
    assert off[0] == 0 and [off[b + 1] - off[b] for b in range(W * NB)] == cnts
    order = dump["order"]
    assert sorted(order) == list(range(W * NB))
    clamped = [min(cnts[b], 4095) for b in order]
    assert all(clamped[i] >= clamped[i + 1] for i in range(len(clamped) - 1))
    cls = M.classes(cnts, chain)
    assert dump["cls"] == cls
    return cnts, cls


def run1(be, scalars, points, halves=2, pidx=None, n_pool0=None, cap=0):
    return be.probe_g1_msm_pippenger_ex([{"scalars": scalars, "points": points, "halves": halves, "pidx": pidx, "n_pool0": n_pool0}],
                                        acc_grid_cap=cap, dump=True)[0]


# ------------------------------------------------------------------------------------------------ (a) forced window widths
@pytest.mark.parametrize("n", [300, 3000])
@pytest.mark.parametrize("c", [3, 5, 7, 8, 9, 10])
def test_forced_window_widths(be, orc, pool, c, n):
    """Every width the option takes: 3 and 5 come back as 7 with 19 windows (pip_shape widens until the windows fit), 8 has a
    top window of 128 - 16 x 8 = 0 bits that holds the carry alone.  Random and edge scalars, bases mixed with infinity."""
    rng = random.Random(1000 * c + n)
    scalars = [rng.randrange(R) if rng.random() < 0.8 else rng.choice(EDGE) for _ in range(n)]
    idx = [None if i % 29 == 7 else rng.randrange(len(pool.comp)) for i in range(n)]
    points = [INF if j is None else pool.comp[j] for j in idx]
    with forced(be, c=c):
        got, dump = run1(be, scalars, points)
    assert got == fold(orc, pool.aff, scalars, idx)
    want_c = max(c, 7)
    assert (dump["c"], dump["W"], dump["NB"]) == (want_c, 128 // want_c + 1, 1 << (want_c - 1))
    check_tables(dump, scalars, [j is not None for j in idx], 2, forced_c=c)


# ------------------------------------------------------------------------------------------------ (b) size classes and borders
def border_input(pool, bucket_counts, seed):
    """Scalars d in 1 .. NB are one entry of bucket (window 0, d) each (glv_split(d) == (d, 0)): bucket_counts[i] entries for the
    i-th of a set of digits that includes 1 and NB, the terms shuffled, bases drawn from the pool through an index map."""
    rng = random.Random(seed)
    n = sum(bucket_counts)
    NB = M.shape(n, 2)[2]
    assert len(bucket_counts) <= NB
    ds = [1, NB] + rng.sample(range(2, NB), len(bucket_counts) - 2)
    scalars = [d for d, cv in zip(ds, bucket_counts) for _ in range(cv)]
    rng.shuffle(scalars)
    assert all(bls.glv_split(d) == (d, 0) for d in ds)
    pidx = [rng.randrange(len(pool.comp)) for _ in range(n)]
    return scalars, pidx


def default_chain_counts():
    T = M.DEFAULT_CHAIN
    return [1] + [v for k in range(8) for v in (T << k, (T << k) + 1)] + [4094, 4095, 4096, 5003]


@pytest.fixture(scope="module")
def border_case(orc, pool):
    """the input of the default chain T = 20 (about 27 k terms), its fold and its model tables: shared with the block walk"""
    counts = default_chain_counts()
    scalars, pidx = border_input(pool, counts, 20)
    return {"scalars": scalars, "pidx": pidx, "counts": counts, "want": fold(orc, pool.aff, scalars, pidx)}


def check_border_tables(dump, scalars, bucket_counts, forced_chain=0):
    cnts, cls = check_tables(dump, scalars, [True] * len(scalars), 2, forced_chain=forced_chain)
    assert sorted(cv for cv in cnts if cv) == sorted(bucket_counts)       # the prescribed counts, in window 0 and nowhere else
    assert not any(cnts[dump["NB"]:])
    return cnts, cls


def test_size_class_borders_default_chain(be, pool, border_case):
    """Buckets of 1, T, T + 1, 2 T, 2 T + 1, ... 128 T, 128 T + 1, 4094, 4095, 4096 and 5003 entries with T = 20: both sides of
    every class border, and the three counts around the histogram's last bin."""
    got, dump = run1(be, border_case["scalars"], pool.comp, pidx=border_case["pidx"])
    assert got == border_case["want"]
    cnts, cls = check_border_tables(dump, border_case["scalars"], border_case["counts"])
    T = 20
    lanes = {cv: 1 << k for cv, k in zip(cnts, M.bucket_class(cnts, cls)) if cv}
    assert all(lanes[T << k] == 1 << k and lanes[(T << k) + 1] == 2 << k for k in range(8))
    assert lanes[1] == 1 and lanes[4094] == lanes[4095] == lanes[4096] == lanes[5003] == 256


def test_size_class_borders_chain_2(be, orc, pool):
    """T = 2: the 256-lane class starts above 256 entries, and a lane's slice is one or two entries long."""
    counts = [1] + [v for k in range(8) for v in (2 << k, (2 << k) + 1)] + [1000, 2500]
    scalars, pidx = border_input(pool, counts, 2)
    with forced(be, chain=2):
        got, dump = run1(be, scalars, pool.comp, pidx=pidx)
    assert got == fold(orc, pool.aff, scalars, pidx)
    cnts, cls = check_border_tables(dump, scalars, counts, forced_chain=2)
    lanes = {cv: 1 << k for cv, k in zip(cnts, M.bucket_class(cnts, cls)) if cv}
    assert lanes[256] == 128 and lanes[257] == lanes[1000] == lanes[2500] == 256


@pytest.mark.parametrize("chain", [64, 1024])
def test_size_classes_beyond_the_histogram(be, orc, pool, chain):
    """Chains above 31: T 2^(k-1) lies beyond the histogram for the top classes, which then start at 4095 entries."""
    counts = [1, 2048, 2049, 4094, 4095, 4096, 9001]
    scalars, pidx = border_input(pool, counts, chain)
    with forced(be, chain=chain):
        got, dump = run1(be, scalars, pool.comp, pidx=pidx)
    assert got == fold(orc, pool.aff, scalars, pidx)
    cnts, cls = check_border_tables(dump, scalars, counts, forced_chain=chain)
    lanes = {cv: 1 << k for cv, k in zip(cnts, M.bucket_class(cnts, cls)) if cv}
    assert lanes[4095] == lanes[4096] == lanes[9001] == 256
    assert (lanes[2048], lanes[2049], lanes[4094]) == ((32, 64, 64) if chain == 64 else (2, 4, 4))


# ------------------------------------------------------------------------------------------------ (c) skewed scalars
def test_one_scalar_for_every_term(be, orc):
    """5000 distinct bases, all with the same random 255-bit scalar: every window of either half has one bucket of 5000 entries
    (or one of 10000 where the halves' digits agree) and nothing else."""
    big = Pool(orc, 5000, 2)
    s = random.Random(5).randrange(1 << 254, R)
    scalars = [s] * 5000
    got, dump = run1(be, scalars, big.comp)
    assert got == orc.g1_msm([s * sum(big.mult) % R], [bls.G1_GEN])
    cnts, _ = check_tables(dump, scalars, [True] * 5000, 2)
    assert set(cnts) <= {0, 5000, 10000} and sum(cnts) == 5000 * sum(1 for row in M.digits(s, 2, dump["c"], dump["W"]) for d in row if d)


@pytest.mark.parametrize("c", [0, 8, 9, 10])
def test_one_window_at_a_time(be, orc, pool, c):
    """halves = 1, scalars d 2^(c w) for each window w in turn: every other window sum is infinity in k_pip_reduce and
    k_pip_combine, and the doublings of the window's weight run for every c w there is, the top window included (c = 0: the
    launcher's choice for a small batch, 7).  The top window of c = 8 holds no scalar bit: it is reached by the carry of
    window 15, which is then not empty either."""
    n = 256
    cc, W, NB, _ = M.shape(n, 1, forced_c=c)
    rng = random.Random(c)
    with forced(be, c=c):
        for w in range(W):
            top_bits = 128 - cc * w
            if top_bits > 0:
                dmax = min(NB, (1 << top_bits) - 1)
                ds = [1, dmax] + [rng.randrange(1, dmax + 1) for _ in range(n - 2)]
                scalars = [d << (cc * w) for d in ds]
            else:
                ds = None
                scalars = [(NB + 1 + i % (NB - 1)) << (cc * (w - 1)) for i in range(n)]      # window w - 1 above NB: it carries
            pidx = [rng.randrange(32) for _ in range(n)]              # (few bases: the fold runs once per window)
            got, dump = run1(be, scalars, pool.comp, halves=1, pidx=pidx)
            assert got == fold(orc, pool.aff, scalars, pidx), (c, w)
            cnts, _ = check_tables(dump, scalars, [True] * n, 1, forced_c=c)
            if ds is not None:
                assert [b // NB for b, cv in enumerate(cnts) if cv] == [w] * len(set(ds))
            else:
                assert {b // NB for b, cv in enumerate(cnts) if cv} == {w - 1, w} and cnts[w * NB] == n


@pytest.mark.parametrize("c", [0, 8, 10])
def test_all_ones_half_carries_into_the_top_window(be, orc, pool, c):
    """2^128 - 1 with halves = 1: digits -1, 0, ... 0 and the carry in the top window."""
    n = 200
    cc, W, NB, _ = M.shape(n, 1, forced_c=c)
    scalars = [(1 << 128) - 1] * n
    row = M.digits(scalars[0], 1, cc, W)[0]
    assert row[0] == -1 and not any(row[1:-1]) and row[-1] == 1 << (128 - cc * (W - 1))
    pidx = [i % len(pool.comp) for i in range(n)]
    with forced(be, c=c):
        got, dump = run1(be, scalars, pool.comp, halves=1, pidx=pidx)
    assert got == fold(orc, pool.aff, scalars, pidx)
    cnts, _ = check_tables(dump, scalars, [True] * n, 1, forced_c=c)
    assert cnts[0] == n and cnts[(W - 1) * NB + row[-1] - 1] == n and sum(cnts) == 2 * n


@pytest.mark.parametrize("c", [0, 8, 10])
def test_digits_at_the_border_of_the_recoding(be, orc, pool, c):
    """The border raw > NB of the recoding: window bits NB everywhere (raw == NB stays +NB, no carry), and window bits
    NB + 1, NB - 1 alternating (raw == NB + 1 becomes -(NB - 1) and carries; the carry lifts NB - 1 to raw == NB, which stays
    +NB).  -NB itself is no digit of this recoding."""
    n = 300
    cc, W, NB, _ = M.shape(n, 1, forced_c=c)
    full = 128 // cc                                   # windows that lie below bit 128 entirely
    a = sum(NB << (cc * w) for w in range(full))
    b = sum((NB + 1 if w % 2 == 0 else NB - 1) << (cc * w) for w in range(full - full % 2))
    assert M.digits(a, 1, cc, W)[0][:full] == [NB] * full
    assert M.digits(b, 1, cc, W)[0][:full - full % 2] == [-(NB - 1), NB] * (full // 2)
    scalars = [a if i % 2 else b for i in range(n)]
    pidx = [i % len(pool.comp) for i in range(n)]
    with forced(be, c=c):
        got, dump = run1(be, scalars, pool.comp, halves=1, pidx=pidx)
    assert got == fold(orc, pool.aff, scalars, pidx)
    cnts, _ = check_tables(dump, scalars, [True] * n, 1, forced_c=c)
    assert all(cnts[w * NB + NB - 1] >= n // 2 for w in range(full - full % 2))


# ------------------------------------------------------------------------------------------------ (d) equal and opposite points
def test_equal_and_opposite_points_everywhere(be, orc, pool):
    """One base for all of 2000 terms; the two bases P and -P; P with scalars that sum to 0 mod r.  Nearly every lane of
    k_pip_accumulate redoes its slice with the complete law, and the LDS trees meet equal, opposite and infinite partial sums."""
    rng = random.Random(4)
    n = 2000
    p = pool.aff[3]
    neg = (p[0], bls.P - p[1])
    scalars = [rng.randrange(R) for _ in range(n)]
    got, dump = run1(be, scalars, [pool.comp[3]], pidx=[0] * n)
    assert got == orc.g1_msm([sum(scalars) % R], [p])
    check_tables(dump, scalars, [True] * n, 2)
    pidx = [rng.randrange(2) for _ in range(n)]
    got, _ = run1(be, scalars, [pool.comp[3], bls.g1_compress(neg)], pidx=pidx)
    assert got == fold(orc, [p, neg], scalars, pidx)
    assert got == orc.g1_msm([sum(s if j == 0 else R - s for s, j in zip(scalars, pidx)) % R], [p])
    zero = scalars[:-1] + [(-sum(scalars[:-1])) % R]
    got, _ = run1(be, zero, [pool.comp[3]], pidx=[0] * n)
    assert got is None
    same = [scalars[0]] * n                                # and equal scalars on P and -P in equal numbers
    got, _ = run1(be, same, [pool.comp[3], bls.g1_compress(neg)], pidx=[i % 2 for i in range(n)])
    assert got is None


# ------------------------------------------------------------------------------------------------ (e) two problems, one launch
def test_two_problems_of_different_shape_in_one_launch(be, orc, pool):
    """A: 3000 terms, halves = 2 -> c = 8, W = 17, NB = 128.  B: 40 terms, halves = 1 -> c = 7, W = 19, NB = 64.  The launches
    are 19 windows and 128 threads wide, so either problem has blocks and threads that belong to the other's shape."""
    rng = random.Random(6)
    sa = [rng.randrange(R) if rng.random() < 0.9 else rng.choice(EDGE) for _ in range(3000)]
    ia = [rng.randrange(len(pool.comp)) for _ in range(3000)]
    sb = [rng.randrange(1 << 128) for _ in range(38)] + [(1 << 128) - 1, 1]
    ib = [rng.randrange(len(pool.comp)) for _ in range(40)]
    A = {"scalars": sa, "points": pool.comp, "pidx": ia, "halves": 2}
    B = {"scalars": sb, "points": pool.comp, "pidx": ib, "halves": 1}
    want_a, want_b = fold(orc, pool.aff, sa, ia), fold(orc, pool.aff, sb, ib)
    (alone_a, dump_a), = be.probe_g1_msm_pippenger_ex([A], dump=True)
    (alone_b, dump_b), = be.probe_g1_msm_pippenger_ex([B], dump=True)
    assert (dump_a["c"], dump_a["W"], dump_a["NB"]) == (8, 17, 128) and (dump_b["c"], dump_b["W"], dump_b["NB"]) == (7, 19, 64)
    assert alone_a == want_a and alone_b == want_b
    for order in ((A, B), (B, A)):
        res = be.probe_g1_msm_pippenger_ex(list(order), dump=True)
        (got_a, da), (got_b, db) = res if order[0] is A else res[::-1]
        assert got_a == want_a == alone_a and got_b == want_b == alone_b
        check_tables(da, sa, [True] * 3000, 2)
        check_tables(db, sb, [True] * 40, 1)
        assert da["acc_blocks"] == db["acc_blocks"] == max(dump_a["acc_blocks"], dump_b["acc_blocks"])


# ------------------------------------------------------------------------------------------------ (f) index map over two pools
def _not_a_point():
    """a compressed encoding whose x is on no curve point"""
    x = 5
    while bls.fp_sqrt((x * x * x + 4) % bls.P) is not None:
        x += 1
    return bytes([0x80]) + x.to_bytes(48, "big")[1:]


@pytest.mark.parametrize("n_pool0", [152, 0, 304])
def test_index_map_over_two_pools(be, orc, pool, n_pool0):
    """pidx with repeats over pool0 = records [0, n_pool0) and pool1 = the rest (separate allocations on the device), an
    infinity and an encoding that does not decompress in either part; n_pool0 = 0 and = the pool size: one part is empty."""
    bad = _not_a_point()
    ok, _ = orc.g1_decompress(bad)
    assert not ok
    points = pool.comp[:150] + [INF, bad] + pool.comp[150:] + [INF, bad]
    assert len(points) == 304
    src = list(range(150)) + [None, None] + list(range(150, 300)) + [None, None]     # record -> base of the pool
    rng = random.Random(n_pool0)
    n = 2000
    pidx = [0, 149, 150, 151, 152, 153, 301, 302, 303, 152, 152, 0] + [rng.randrange(304) for _ in range(n - 12)]
    scalars = [rng.randrange(1, R) for _ in range(n)]
    got, dump = run1(be, scalars, points, pidx=pidx, n_pool0=n_pool0)
    idx = [src[j] for j in pidx]
    assert got == fold(orc, pool.aff, scalars, idx)
    check_tables(dump, scalars, [j is not None for j in idx], 2)


def test_probe_rejects_bad_arguments(be, pool):
    with pytest.raises(be.H2VError, match="error -1"):
        run1(be, [1, 1 << 128], pool.comp[:2], halves=1)                 # halves = 1 takes scalars below 2^128
    with pytest.raises(be.H2VError, match="error -1"):
        run1(be, [1, 2], pool.comp[:2], pidx=[0, 2])                     # an index outside the pool
    with pytest.raises(be.H2VError, match="error -1"):
        run1(be, [1, 2, 3], pool.comp[:2])                               # the identity map needs one point per term
    with pytest.raises(be.H2VError, match="error -1"):
        run1(be, [1, 2], pool.comp[:2], n_pool0=3)
    assert run1(be, [1, 2], pool.comp[:2], halves=1)[0] == bls.g1_add(pool.aff[0], bls.g1_add(pool.aff[1], pool.aff[1]))


# ------------------------------------------------------------------------------------------------ (g) the logical-block walk
@pytest.mark.parametrize("cap", [1, 3])
def test_accumulate_walks_the_logical_blocks(be, pool, border_case, cap):
    """The input of the default-chain border test with the grid of k_pip_accumulate capped at 1 and at 3 blocks: every block
    walks several logical blocks of different classes (red[] reused, the trailing barrier), and nothing changes."""
    free, dump0 = run1(be, border_case["scalars"], pool.comp, pidx=border_case["pidx"])
    got, dump = run1(be, border_case["scalars"], pool.comp, pidx=border_case["pidx"], cap=cap)
    assert got == free == border_case["want"]
    assert dump["acc_blocks"] == cap < dump0["acc_blocks"]
    assert (dump["cls"], dump["off"]) == (dump0["cls"], dump0["off"])
    _, cls = check_border_tables(dump, border_case["scalars"], border_case["counts"])
    blocks = M.block_classes(cls)
    assert len(blocks) > cap and len(blocks) <= dump0["acc_blocks"]
    assert len(set(blocks)) >= 4
    for first in range(cap):                                   # what each physical block walks: more than one class
        assert len(blocks[first::cap]) >= 2 and len(set(blocks[first::cap])) >= 2
