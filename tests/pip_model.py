"""Integer model of the bucket (Pippenger) G1 MSM's bookkeeping, restated from the comments of csrc/h2v_pippenger.hpp and
csrc/h2v_capi.hip (pip_shape): the shape the launcher picks, the signed-digit recoding of k_pip_digits, the bucket counts, and
the size-class table k_pip_scan writes.  Plain Python, no GPU; tests/test_bucket_msm_model.py ties it to the rules the kernel
comments promise, tests/test_bucket_msm_shapes_gpu.py compares the device's tables with it."""
from plutus_halo2_verifier_gen_amd import bls12_381 as bls

MAX_W, MAX_C = 20, 10          # PIP_MAX_W, PIP_MAX_C
N_CLASSES = 9                  # a bucket gets 2^0 .. 2^8 lanes
CLS_DW = 3 * N_CLASSES + 1     # per class: first rank, end rank, first lane; then the lane total
HIST = 4096                    # k_pip_scan's histogram: counts of 4095 and more share the last bin
DEFAULT_CHAIN = 20


def shape(n, halves, forced_c=0, forced_chain=0):
    """(c, W, NB, chain) as pip_shape picks them: the widest window with at least 24 entries per bucket on average, a forced
    width of 3 .. 10 instead, and either widened until W = 128 // c + 1 windows fit PIP_MAX_W."""
    c = MAX_C
    while c > 4 and n * halves < 24 * (1 << (c - 1)):
        c -= 1
    if 3 <= forced_c <= MAX_C:
        c = forced_c
    while 128 // c + 1 > MAX_W:
        c += 1
    chain = forced_chain if 2 <= forced_chain <= 1024 else DEFAULT_CHAIN
    return c, 128 // c + 1, 1 << (c - 1), chain


def recode(half, c, W):
    """W signed c-bit digits of a value below 2^128: raw = window bits + carry; raw > 2^(c-1) becomes raw - 2^c and carries."""
    assert 0 <= half < (1 << 128)
    NB, carry, out = 1 << (c - 1), 0, []
    for w in range(W):
        raw = ((half >> (w * c)) & ((1 << c) - 1)) + carry
        if raw > NB:
            d, carry = raw - (1 << c), 1
        else:
            d, carry = raw, 0
        out.append(d)
    assert carry == 0, "W c > 128 and the top window holds fewer than c - 1 bits: no carry leaves it"
    return out


def digits(scalar, halves, c, W):
    """the digit rows of one scalar, one per half: (k1, k2) of the GLV split for halves = 2, the scalar itself for halves = 1"""
    if halves == 2:
        parts = bls.glv_split(scalar)
    else:
        assert scalar < (1 << 128)
        parts = (scalar,)
    return [recode(p, c, W) for p in parts]


def counts(scalars, live, halves, c, W):
    """entries per bucket, bucket (window w, |digit| j) at w NB + j - 1; live[i] is False for a base at infinity, which like a
    zero scalar contributes nothing"""
    NB = 1 << (c - 1)
    out = [0] * (W * NB)
    for s, alive in zip(scalars, live):
        if not alive or s == 0:
            continue
        for row in digits(s, halves, c, W):
            for w, d in enumerate(row):
                if d:
                    out[w * NB + abs(d) - 1] += 1
    return out


def _first_rank(cnts):
    """first_rank[v] = number of buckets whose clamped count exceeds v = the first rank of count v in descending order"""
    hist = [0] * HIST
    for cv in cnts:
        hist[min(cv, HIST - 1)] += 1
    first, acc = [0] * HIST, 0
    for v in range(HIST - 1, -1, -1):
        first[v] = acc
        acc += hist[v]
    return first


def classes(cnts, chain):
    """The cls[] table of k_pip_scan: class k holds the buckets with count in (T 2^(k-1), T 2^k] (k = 8: all above T 2^7, k = 0:
    1 .. T) as ranks [first, end) of the descending order, its lanes start at a multiple of 256, and the last dword is the lane
    total.  A border T 2^(k-1) of 4095 or more is beyond the histogram and reads as 4094: such a class starts at 4095 entries."""
    first_rank = _first_rank(cnts)
    cls, lane, first = [0] * CLS_DW, 0, 0
    for k in range(N_CLASSES - 1, -1, -1):
        low = 0 if k == 0 else chain << (k - 1)
        end = first_rank[low if low < HIST - 1 else HIST - 2]
        cls[3 * k:3 * k + 3] = [first, end, lane]
        lane += (((end - first) << k) + 255) & ~255
        first = end
    cls[3 * N_CLASSES] = lane
    return cls


def bucket_class(cnts, cls):
    """per bucket the class k whose rank range holds it, None for a bucket without a lane.  Buckets of equal clamped count are
    neighbours in the descending order and every class border is a count, so the first rank of its count decides."""
    first_rank = _first_rank(cnts)
    out = []
    for cv in cnts:
        rank = first_rank[min(cv, HIST - 1)]
        ks = [k for k in range(N_CLASSES) if cls[3 * k] <= rank < cls[3 * k + 1]]
        assert len(ks) <= 1
        out.append(ks[0] if ks else None)
    return out


def block_classes(cls):
    """the class of every logical 256-lane block of k_pip_accumulate, in launch order (k = 8 first)"""
    out = []
    for k in range(N_CLASSES - 1, -1, -1):
        lanes = (cls[3 * k + 1] - cls[3 * k]) << k
        assert cls[3 * k + 2] == 256 * len(out)
        out += [k] * ((lanes + 255) // 256)
    assert 256 * len(out) == cls[3 * N_CLASSES]
    return out
