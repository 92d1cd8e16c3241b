"""GPU tests of the batch coefficients of every batch-accept form (h2v_verify_batch_rlc, H2V_RLC_FOLD_PAIRS, h2v_check_pairs_rlc,
H2V_MIXED_RLC, H2V_MIXED_FOLD_MSM, coalesced RLC groups) against inputs built to defeat them: two proofs whose pairing errors cancel
under chosen weights (tests/cancel.py; the construction itself is held to the oracle in tests/test_batch_cancellation.py).

Part A - equal weights must never pass.  The pair is built for w = (1, 1): a form that gave the two positions the SAME coefficient
(keyed by the lane, by the index within a key, a chunk or a gathered call instead of the position in the check) would accept both.
Part B - the documented weights, and only those, pass.  With a given seed (H2V_RLC_SEED_GIVEN is test-only for exactly this
reason) the pair is built for the coefficients include/h2v.h documents for positions (a, b): the check passes, so each position
really got that coefficient; the same bytes on the next call (the call counter has moved) and the pair placed at (b, a) are rejected.

Every expectation is exact and comes from the construction: verdict bytes, status words, the batch verdict.  Batches are small
(eight forged proofs per key, repeated: duplicates are legal) and every altered proof is checked with the CPU oracle."""
import json

import pytest

from plutus_halo2_verifier_gen_amd import synth
from tests import cancel
from tests.test_gpu_parity import be  # noqa: F401  (module fixture)
from tests.test_mixed_keys import COMMON_S, MIXED_KEYS
from tests.test_mixed_keys_gpu import LISTED, Mix, _DeviceCall

pytestmark = pytest.mark.gpu
GIVEN = bytes(range(60, 92))
PER_KEY = 8
N = 130                                   # holds every position pair below; three 64-proof blocks, the last one ragged
POSITIONS = [(0, 1), (63, 64), (5, 69), (0, N - 1)]          # (5, 69): the same lane of two 64-proof blocks
N_GROUPS = 258                            # >= GRP_MIN_N (256, h2v_capi.hip: rlc_groups_on) + 2: the 64-proof group stage runs after a failed check
GROUP_POSITIONS = [(70, 75), (5, 69)]     # inside one group; the same lane of two groups
D = 0x1d2c3b4a5968778695a4b3c2d1e0f


@pytest.fixture(scope="module")
def cx(be, orc):
    """keys on one SRS, PER_KEY accepting proofs of each (oracle-checked), the device plans in LISTED order"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    keys, clean = {}, {}
    for k, name in enumerate(LISTED):
        vk, td = V.on_srs(*V.BUILDERS[name](), COMMON_S)
        pl = PL.compile_plan(vk)
        keys[name] = {"vk": vk, "td": td, "pl": pl, "dp": be.DevicePlan(pl.to_bytes(), 0),
                      "ov": orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))}
        if name in MIXED_KEYS:
            b = clean[name] = synth.forge_batch(vk, td, PER_KEY, seed=141 + k, plan=pl)
            assert list(keys[name]["ov"].verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4)) == [1] * PER_KEY
            assert len({b.proof(j) for j in range(PER_KEY)}) == PER_KEY
    return {"keys": keys, "clean": clean, "plans": [keys[name]["dp"] for name in LISTED], "orc": orc}


@pytest.fixture(scope="module")
def lw(be, cx):
    """the workspace of cancel.learn_counter's one-proof calls"""
    ws = be.Workspace.multi(cx["plans"], 16)
    yield ws
    ws.close()


def _pair(cx, ka, kb, wa=1, wb=1):
    """(A', B') of the accepting proofs ka = (key, index), kb for the weights; each is rejected by the oracle, by the pairing alone"""
    recs = [cancel.rec_of(cx["keys"][name], cx["clean"][name], j) for name, j in (ka, kb)]
    assert recs[0].proof != recs[1].proof
    out = cancel.cancelling(recs[0], recs[1], wa, wb, D)
    for (name, _j), rec, p in zip((ka, kb), recs, out):
        ok, tr = cx["keys"][name]["ov"].verify(p, rec.ints, rec.ci, trace=True)
        assert not ok and cx["orc"].STATUS[tr.status] == "pairing"
    return out


def _with_altered(cx, put):
    """per key: the clean batch with the altered proofs of `put` = {position: ((key, index), proof)} appended (public inputs and
    committed instance of the proof they were made from); {position: (key, index in that batch)}"""
    parts = {name: ([b.proof(j) for j in range(b.n)], [j for j in range(b.n)]) for name, b in cx["clean"].items()}
    at = {}
    for pos, ((name, j), proof) in sorted(put.items()):
        at[pos] = (name, len(parts[name][0]))
        parts[name][0].append(proof)
        parts[name][1].append(j)
    batches = {}
    for name, (proofs, src) in parts.items():
        b, n_pi = cx["clean"][name], cx["keys"][name]["vk"].n_public_inputs
        off = [0]
        for p in proofs:
            off.append(off[-1] + len(p))
        batches[name] = synth.Batch(n=len(proofs), proofs=b"".join(proofs), proof_off=off,
                                    instances=b"".join(b.instances[32 * n_pi * j:32 * n_pi * (j + 1)] for j in src),
                                    committed=None if b.committed is None else b"".join(b.ci(j) for j in src),
                                    expected=[1] * b.n + [0] * (len(proofs) - b.n))
    return batches, at


def _mix(cx, names, put):
    """the mixed batch with key names[i] at position i (clean proofs, repeated in turn) and the altered proofs of `put` in place"""
    batches, at = _with_altered(cx, put)
    seen, order = {}, []
    for i, name in enumerate(names):
        if i in at:
            assert at[i][0] == name
            order.append(at[i])
        else:
            order.append((name, seen.get(name, 0) % PER_KEY))
            seen[name] = seen.get(name, 0) + 1
    return Mix(cx["keys"], batches, order)


def _single(cx, name, n, put):
    """n proofs of one key as a synth.Batch"""
    mix = _mix(cx, [name] * n, put)
    return synth.Batch(n=n, proofs=mix.proofs, proof_off=mix.off, instances=mix.instances, committed=mix.committed, expected=mix.expected)


class _Up:
    """a single-key batch (or n pairs) on the device with accept / status tensors; alive until results() has synchronised"""

    def __init__(self, batch=None, pairs=None):
        import torch
        dev = torch.device("cuda", 0)
        t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
        ptr = lambda x: x.data_ptr() if x is not None else None
        if pairs is not None:
            self.n, self.keep = len(pairs) // 96, [t(pairs)]
        else:
            self.n = batch.n
            self.keep = [t(batch.proofs), torch.tensor(batch.proof_off, dtype=torch.int64, device=dev), t(batch.instances), t(batch.committed)]
        self.acc = torch.full((self.n,), 7, dtype=torch.uint8, device=dev)
        self.st = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        torch.cuda.current_stream().synchronize()
        self.args = (self.n, *[ptr(x) for x in self.keep], self.acc.data_ptr(), self.st.data_ptr())

    def results(self):
        self.stream.synchronize()
        return list(self.acc.cpu().tolist()), [v & 0xffffffff for v in self.st.cpu().tolist()]


class _MixedCall(_DeviceCall):
    """h2v_verify_mixed_device with H2V_MIXED_RLC, a seed (None: the OS's) and optionally H2V_MIXED_FOLD_MSM"""

    def __init__(self, be, cx, mix, ws, seed, fold):
        import torch
        self.seed, self.fold = seed, fold
        super().__init__(be, cx, mix, "rlc", ws, torch.cuda.Stream(device=torch.device("cuda", 0)))

    def launch(self):
        be, plans, plan_of, _mode, ws = self.args
        ptr = lambda x: x.data_ptr() if x is not None else None
        be.verify_mixed_device(plans, plan_of, self.n, *[ptr(x) for x in self.keep], self.acc.data_ptr(), self.st.data_ptr(), ws=ws,
                               stream=self.stream.cuda_stream, mode="rlc", seed=self.seed, fold_msm=self.fold)


# ---- the forms.  run(n or names, put, seed) -> (accept list, status list or None where the form has none, the batch verdict);
# weight(counter, p): the coefficient include/h2v.h documents for position p of the check when the form's (first) seeded call
# mixes `counter` in.  An ordinary workspace's call is ONE check over positions 0 .. n - 1; chunk 0 of a laned workspace carries
# that chunk's tweak (cancel.coeff).
class _Form:
    chunk = None

    def __init__(self, be, cx, ws):
        self.be, self.cx, self.ws = be, cx, ws
        ws.set_option(be.OPT_RLC_ROUTE, -1)            # always the batch check first, whatever earlier calls on ws met

    def weight(self, counter, p):
        return cancel.coeff(GIVEN, counter, p, chunk=self.chunk)

    def close(self):
        self.ws.close()


class RlcProofs(_Form):
    """h2v_verify_batch_rlc(_device) on an ordinary workspace; fold_pairs: H2V_RLC_FOLD_PAIRS on the recursive key"""

    def __init__(self, be, cx, name, device, cap=N, fold_pairs=False):
        super().__init__(be, cx, be.Workspace(cx["keys"][name]["dp"], cap))
        assert self.ws.lanes() == (1, cap)
        self.name, self.device, self.fold_pairs = name, device, fold_pairs
        self.ka, self.kb = (name, 0), (name, 1)

    def run(self, n, put, seed):
        dp, b = self.cx["keys"][self.name]["dp"], _single(self.cx, self.name, n, put)
        if self.device:
            up = _Up(b)
            dp.verify_batch_rlc_device(*up.args, ws=self.ws, stream=up.stream.cuda_stream, seed=seed, fold_pairs=self.fold_pairs)
            acc, st = up.results()
            return acc, st, self.ws.rlc_result(timings=False)[0]
        acc, fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=self.ws, seed=seed, fold_pairs=self.fold_pairs)
        assert self.ws.rlc_result(timings=False)[0] == (not fb)
        return list(acc), None, not fb


class PairsRlc(_Form):
    """h2v_check_pairs_rlc(_device) over the pairs h2v_prepare_batch makes of the batch"""

    def __init__(self, be, cx, name, device, cap=N):
        super().__init__(be, cx, be.Workspace(cx["keys"][name]["dp"], cap))
        assert self.ws.lanes() == (1, cap)
        self.name, self.device = name, device
        self.ka, self.kb = (name, 0), (name, 1)

    def run(self, n, put, seed):
        dp, b = self.cx["keys"][self.name]["dp"], _single(self.cx, self.name, n, put)
        pairs, st0 = dp.prepare_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=self.ws)
        assert st0 == [0] * n and len(pairs) == 96 * n
        if self.device:
            up = _Up(pairs=pairs)
            dp.check_pairs_rlc_device(*up.args, ws=self.ws, stream=up.stream.cuda_stream, seed=seed)
            acc, st = up.results()
            return acc, st, self.ws.rlc_result(timings=False)[0]
        acc, st, fb = dp.check_pairs_rlc(pairs, ws=self.ws, seed=seed)
        assert self.ws.rlc_result(timings=False)[0] == (not fb)
        return list(acc), st, not fb


class Mixed(_Form):
    """h2v_verify_mixed(_device) with H2V_MIXED_RLC (fold: and H2V_MIXED_FOLD_MSM); laned: 4 lanes x 40 proofs, else a workspace
    whose one chunk holds the call - a laned workspace all the same (h2v_workspace_create_multi), so without the fold flag the
    tail is chunk 0 of a laned call"""

    def __init__(self, be, cx, fold, device, laned, cap=N):
        super().__init__(be, cx, be.Workspace.multi(cx["plans"], cap, lanes=4, chunk=40) if laned else be.Workspace.multi(cx["plans"], cap))
        assert self.ws.lanes() == (4, 40) if laned else self.ws.lanes()[1] >= cap
        self.fold, self.device, self.laned = fold, device, laned
        self.chunk = None if fold else 0

    def run(self, names, put, seed):
        be, mix = self.be, _mix(self.cx, names, put)
        if self.device:
            acc, st = _MixedCall(be, self.cx, mix, self.ws, seed, self.fold).results()
            return acc, st, self.ws.rlc_result(timings=False)[0]
        acc, st, fb = be.verify_mixed(self.cx["plans"], mix.plan_of, mix.proofs, mix.off, mix.instances, mix.committed, ws=self.ws, mode="rlc",
                                      seed=seed, fold_msm=self.fold)
        assert self.ws.rlc_result(timings=False)[0] == (not fb)
        return list(acc), st, not fb


class Coalesced(_Form):
    """two h2v_verify_batch_rlc_device calls of HALF proofs each on a deferring workspace, gathered into ONE group (include/h2v.h,
    COALESCING): position HALF * k + j of the batch is proof j of call k, and of the group's one check"""
    HALF = 64

    def __init__(self, be, cx, name):
        super().__init__(be, cx, be.Workspace(cx["keys"][name]["dp"], 512, lanes=4, chunk=160))
        assert self.ws.lanes() == (4, 160)
        self.ws.defer_joins(True)
        self.name = name
        self.ka, self.kb = (name, 0), (name, 1)

    def run(self, n, put, seed):
        import torch
        assert n == 2 * self.HALF
        be, dp = self.be, self.cx["keys"][self.name]["dp"]
        s = torch.cuda.Stream(device=torch.device("cuda", 0))
        ups = []
        for k in range(2):
            lo = k * self.HALF
            up = _Up(_single(self.cx, self.name, self.HALF, {p - lo: v for p, v in put.items() if lo <= p < lo + self.HALF}))
            up.stream = s
            dp.verify_batch_rlc_device(*up.args, ws=self.ws, stream=s.cuda_stream, seed=seed)
            ups.append(up)
        with pytest.raises(be.H2VError, match="has not run yet"):          # both calls are in the open group
            self.ws.rlc_result(1, timings=False)
        self.ws.join(s.cuda_stream)
        (acc0, st0), (acc1, st1) = ups[0].results(), ups[1].results()
        ok = [self.ws.rlc_result(back, timings=False)[0] for back in (1, 0)]
        assert ok[0] == ok[1]                                               # each call reports the GROUP's verdict
        return acc0 + acc1, st0 + st1, ok[0]


# ---- the two parts
def _rejected(be, got, n, a, b):
    acc, st, passed = got
    assert [i for i, v in enumerate(acc) if v != 1] == sorted((a, b)) and acc[a] == acc[b] == 0 and len(acc) == n
    if st is not None:
        assert st == [be.ST_PAIRING if i in (a, b) else 0 for i in range(n)]
    assert not passed


def _part_a(be, cx, form, shape, a, b, ka, kb):
    """the pair for w = (1, 1) at (a, b): both rejected, every other proof accepted, the batch check failed - given and OS seed"""
    n = shape if isinstance(shape, int) else len(shape)
    pa, pb = _pair(cx, ka, kb)
    for seed in (GIVEN, None):
        _rejected(be, form.run(shape, {a: (ka, pa), b: (kb, pb)}, seed), n, a, b)


def _part_b(be, cx, lw, form, shape, a, b, ka, kb):
    n = shape if isinstance(shape, int) else len(shape)
    c = cancel.learn_counter(be, cx, lw, GIVEN)
    pa, pb = _pair(cx, ka, kb, form.weight(c + 1, a), form.weight(c + 1, b))
    put = {a: (ka, pa), b: (kb, pb)}
    acc, st, passed = form.run(shape, put, GIVEN)
    assert passed, "the documented coefficients of positions (%d, %d) are not the ones the check used" % (a, b)
    assert acc == [1] * n and (st is None or st == [0] * n)
    _rejected(be, form.run(shape, put, GIVEN), n, a, b)                 # the same bytes: the call counter has moved
    c = cancel.learn_counter(be, cx, lw, GIVEN)
    pa, pb = _pair(cx, ka, kb, form.weight(c + 1, a), form.weight(c + 1, b))
    if not isinstance(shape, int):                                      # (a mixed call: the two keys change places with their proofs)
        shape = list(shape)
        shape[a], shape[b] = shape[b], shape[a]
    _rejected(be, form.run(shape, {b: (ka, pa), a: (kb, pb)}, GIVEN), n, a, b)     # right weights, exchanged places


SINGLE_CASES = [(N, a, b) for a, b in POSITIONS]


# ---- h2v_verify_batch_rlc: k_rlc_prepare; after a failed check at n >= GRP_MIN_N the group stage (k_rlc_group_terms)
@pytest.mark.parametrize("part", ["A", "B"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["simple_mul", "lookup_table"])
def test_verify_batch_rlc(be, cx, lw, name, device, part):
    form = RlcProofs(be, cx, name, device, cap=N_GROUPS)
    for n, a, b in SINGLE_CASES + [(N_GROUPS, a, b) for a, b in GROUP_POSITIONS]:
        if part == "A":
            _part_a(be, cx, form, n, a, b, form.ka, form.kb)
        else:
            _part_b(be, cx, lw, form, n, a, b, form.ka, form.kb)
    form.close()


# ---- H2V_RLC_FOLD_PAIRS on the recursive key: k_fold_pairs_affine + k_rlc_pairs_prepare
@pytest.mark.parametrize("part", ["A", "B"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_fold_pairs_of_the_recursive_key(be, cx, lw, device, part):
    form = RlcProofs(be, cx, "ivc", device, fold_pairs=True)
    for n, a, b in SINGLE_CASES:
        if part == "A":
            _part_a(be, cx, form, n, a, b, form.ka, form.kb)
        else:
            _part_b(be, cx, lw, form, n, a, b, form.ka, form.kb)
    form.close()


# ---- h2v_check_pairs_rlc: k_rlc_pairs_prepare; at n >= GRP_MIN_N + 2 the 64-pair group checks
@pytest.mark.parametrize("part", ["A", "B"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_check_pairs_rlc(be, cx, lw, device, part):
    form = PairsRlc(be, cx, "simple_mul", device, cap=N_GROUPS)
    for n, a, b in SINGLE_CASES + [(N_GROUPS, 70, 75)]:
        if part == "A":
            _part_a(be, cx, form, n, a, b, form.ka, form.kb)
        else:
            _part_b(be, cx, lw, form, n, a, b, form.ka, form.kb)
    form.close()


# ---- h2v_verify_mixed with H2V_MIXED_RLC, and with H2V_MIXED_FOLD_MSM (mixed_coeff: k_mixed_terms, k_mixed_pair_terms)
def _names(n):
    """the keys of a mixed call: simple_mul / lookup_table in turn, a trashcan_mix and an ivc proof now and then"""
    return ["ivc" if i % 29 == 28 else "trashcan_mix" if i % 13 == 12 else ("simple_mul", "lookup_table")[i % 2] for i in range(n)]


def _mixed_cases():
    """(names, a, b, ka, kb): A and B are always proofs of two DIFFERENT keys"""
    sm, lt, ivc = ("simple_mul", 0), ("lookup_table", 0), ("ivc", 0)
    out = []
    # the same index within their keys (45: on 4 x 40 also the same index, 5, within the second chunk of either key's sub-batch)
    names = _names(N)
    nth = lambda key, k: [i for i, x in enumerate(names) if x == key][k]
    out.append((names, nth("simple_mul", 45), nth("lookup_table", 45), sm, lt))
    # call positions p and p + chunk, then the position pairs of every form
    for a, b in [(7, 47)] + POSITIONS:
        names = _names(N)
        names[a], names[b] = "simple_mul", "lookup_table"
        out.append((names, a, b, sm, lt))
    # a foldable key's proof against the recursive key's (R-term against pair term)
    names = _names(N)
    names[5], names[69] = "simple_mul", "ivc"
    out.append((names, 5, 69, sm, ivc))
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("laned", [False, True], ids=["plain", "laned"])
@pytest.mark.parametrize("fold", [False, True], ids=["rlc", "fold_msm"])
def test_mixed_equal_weights_never_pass(be, cx, fold, laned, device):
    form = Mixed(be, cx, fold, device, laned)
    for names, a, b, ka, kb in _mixed_cases():
        _part_a(be, cx, form, names, a, b, ka, kb)
    form.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fold,laned", [(False, False), (True, False), (True, True)], ids=["rlc-plain", "fold_msm-plain", "fold_msm-laned"])
def test_mixed_documented_weights_and_only_those_pass(be, cx, lw, fold, laned, device):
    """(H2V_MIXED_RLC on 4 x 40 is not here: its tail is cut into chunks, each a check of its own, so no pair spans the call)"""
    form = Mixed(be, cx, fold, device, laned)
    for names, a, b, ka, kb in _mixed_cases():
        _part_b(be, cx, lw, form, names, a, b, ka, kb)
    form.close()


# ---- coalesced RLC calls: ONE check over the group, the first call's seed, positions counted through the group
COALESCED_POSITIONS = [(5, 69), (63, 64), (69, 70), (0, 127)]       # index 5 of both calls; across the seam; in one call; the ends


@pytest.mark.parametrize("part", ["A", "B"])
def test_coalesced_rlc_group(be, cx, lw, part):
    form = Coalesced(be, cx, "simple_mul")
    for a, b in COALESCED_POSITIONS:
        if part == "A":
            _part_a(be, cx, form, 2 * Coalesced.HALF, a, b, form.ka, form.kb)
        else:
            _part_b(be, cx, lw, form, 2 * Coalesced.HALF, a, b, form.ka, form.kb)
    form.close()
