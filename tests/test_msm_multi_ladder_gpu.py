"""The multi-term MSM ladder (k_g1_msm_multi: msm_multi_body, msm_multi_ladder) against the oracle, in every lane shape and on every
exceptional addition that can be built on purpose.

Several terms share one accumulator there, so a crafted proof can make the unchecked addition meet acc == entry or acc == -entry;
that leaves Z = 0, the lane is judged once at the end by fp_is_zero on the converted Z, and a lane that fails redoes its ladder
with the complete law.  tests/multi_ladder_model.py builds the inputs - bases with known discrete logs, the log of one term solved
so that the event falls on a chosen (lane, window, slot) - and tests/test_multi_ladder_model.py proves on the CPU that they are
what they claim.  Here h2v_probe_g1_msm_multi launches the kernel with 3 .. 8 halves per lane (the odd shapes, where a term's two
halves sit in two lanes, are otherwise reached only unforced in large batches) and every proof's sum is compared with
oracle.binding.g1_msm.

Per hpl one probe call per T, all cases of that T as the proofs of one batch:
  T = 11                   three or more lanes per proof, a partly filled last lane; for odd hpl straddling terms, lanes that begin
                           on a k2 half.  The whole case list: single doubling / inverse events in windows 32, 31, 16, 1 and 0 at
                           the earliest, a middle and the last used slot of the first, a middle and the last eventful lane; the
                           inverse on the very last addition (one lane; every lane: the proof's sum is infinity); a restart behind
                           the true point at infinity; two events in one lane; unused slots in front of the event; the honest
                           control of each.
  the full-last-lane T     (12, 12, 10, 12, 7, 12) and the one-lane-per-proof T (hpl // 2: the reduction loop does not run): the
                           single events in windows 32, 16 and 0 and the two last-addition cases.
The T = 11 batch is laid out so that block 0 holds exactly one crafted lane among honest proofs, another block only crafted
proofs, and the last block is partly filled.

No pipeline case: with the launcher's rule (msm_terms_per_lane, msm_multi_shape) at in-flight hint 8 no key of vk.BUILDERS runs
an odd number of halves per lane unforced in a batch of at most 2048 proofs - three terms per lane need n ceil(T / 3) >= 16384 and
give an odd shape only for T = 5, 7 and 10, four need n ceil(T / 4) >= 16384 and give 7 only up to T = 21."""
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import multi_ladder_model as M
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
BLOCK = 256
E_ARG = "h2v error -1"


def arrange(cs, hpl, T):
    """the batch order: block 0 = honest proofs around ONE proof with one crafted lane, then every other crafted proof (at least one
    block of nothing else), then the remaining honest ones; one more honest proof if that would fill the last block"""
    per_block = BLOCK // M.lanes_per_proof(T, hpl)
    crafted, honest = [c for c in cs if c.targets], [c for c in cs if c.honest]
    order = list(cs)
    if T == M.FULL_T:
        lone = next(c for c in crafted if len(c.targets) == 1 and c.targets[0][1] == 16)
        head = honest[:per_block - 1]
        head.insert(per_block // 2, lone)
        order = head + [c for c in crafted if c is not lone] + honest[per_block - 1:]
    if len(order) % per_block == 0:
        rng = random.Random("multi-ladder/%d/%d/pad" % (hpl, T))
        order.append(M.Case("honest-pad", hpl, [rng.randrange(1, bls.R) for _ in range(T)], list(M.POOL_LOGS[:T])))
    return order, per_block


def check_layout(order, per_block):
    blocks = [order[k:k + per_block] for k in range(0, len(order), per_block)]
    assert len(blocks) >= 2 and len(blocks[-1]) < per_block
    assert sum(len(c.crafted_lanes()) for c in blocks[0]) == 1 and sum(1 for c in blocks[0] if c.honest) == per_block - 1
    assert any(len(b) == per_block and all(c.targets for c in b) for b in blocks)


@pytest.mark.parametrize("hpl", range(3, 9))
def test_every_lane_shape_and_every_exceptional_addition(be, orc, hpl):   # noqa: F811
    for T in M.gpu_shapes(hpl):
        order, per_block = arrange(M.cases(hpl, T), hpl, T)
        if T == M.FULL_T:
            check_layout(order, per_block)
        points = [c.points() for c in order]
        want = [orc.g1_msm(c.scalars, ps) for c, ps in zip(order, points)]
        assert all((w is None) == c.sum_is_infinity for c, w in zip(order, want))
        got = be.probe_g1_msm_multi([c.scalars for c in order], [[bls.g1_compress(p) for p in ps] for ps in points], hpl)
        wrong = [c.name for c, g, w in zip(order, got, want) if g != w]
        print("hpl %d T %d: %d proofs, %d per block, wrong: %d crafted, %d honest" %
              (hpl, T, len(order), per_block, sum(1 for c in order if c.targets and c.name in wrong), sum(1 for c in order if c.honest and c.name in wrong)))
        assert not wrong, "hpl %d, T %d: %d of %d proofs differ from the oracle: %s" % (hpl, T, len(wrong), len(order), wrong[:12])


def test_probe_refuses_other_lane_shapes(be):   # noqa: F811
    g = bls.g1_compress(bls.G1_GEN)
    for hpl in (2, 9):
        with pytest.raises(be.H2VError, match=E_ARG):
            be.probe_g1_msm_multi([[1, 2, 3]], [[g, g, g]], hpl)
