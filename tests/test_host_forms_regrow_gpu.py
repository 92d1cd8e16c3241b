"""The blocking host-buffer forms on ONE workspace whose blocks grow, shrink and are shared: every form of h2v_prepare_batch,
h2v_check_pairs(_rlc), h2v_aggregate_batch, h2v_verify_batch_rlc, h2v_verify_mixed and h2v_aggregate_mixed returns, bit for bit,
what its *_device form returns on the same bytes on a second workspace of the same kind.

The host forms share one packer (stage_batch), one result block per workspace (hostcall::result_block) and one download tail;
the sizes 1, 17, 3, 16, 15, 40, 2 - growth, shrink, the three sizes around a 16-byte region boundary, growth, shrink - are run
in that order with the forms interleaved inside every size, once on an ordinary workspace and once on a laned one whose chunks
of 3 make 40 proofs 14 chunks.  Batches are prefixes of one pool of 40 proofs per module; every batch of two or more holds a
rejecting proof, so no accept[] / included[] is constant.  (Sizes of blocks are checked on the CPU: tests/test_hostcall_layout.py.)

One output cannot be equal on the two sides: an aggregate call's pair.  The library mixes a process-wide call counter into a
given seed (rlc_seed: no two calls get the same coefficients), so the host call and the device call combine the same per-proof
pairs with different r_i.  Each side's pair is therefore held to the big-integer model (tests/agg_model.py) under the seed its
own h2v_aggregate_info reports, over the per-proof pairs of h2v_prepare_batch_device - which says more than equality would -
and the seeds must be the given one outside the two counter words."""
import ctypes as C
import struct

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls, synth
from tests import agg_model
from tests.test_gpu_parity import be, circuits  # noqa: F401  (module fixtures)
from tests.test_mixed_keys import COMMON_S

pytestmark = pytest.mark.gpu
SIZES = [1, 17, 3, 16, 15, 40, 2]
SEED = bytes(range(7, 39))
KINDS = ["flip_first_scalar", "point_not_on_curve"]     # rejected by the pairing / before it: fell_back takes both values
REJECT_SEED, MIXED_REJECT_SEEDS = 4, (2, 1)               # with_rejects seeds that accept proof 0 and reject proof 1 (the fixture asserts it)


class Pool:
    """proofs of one or several keys in call order; prefix(m) is the batch of the first m in the layout of h2v_(mixed_)batch"""

    def __init__(self, parts):
        """parts: (plan index, proof bytes, instance bytes, expected) per proof"""
        self.plan_of = [p[0] for p in parts]
        self.expected = [p[3] for p in parts]
        self.off, self.ioff = [0], [0]
        for _k, pr, ins, _e in parts:
            self.off.append(self.off[-1] + len(pr))
            self.ioff.append(self.ioff[-1] + len(ins))
        self.proofs, self.inst = b"".join(p[1] for p in parts), b"".join(p[2] for p in parts)

    def set_pairs(self, pairs):
        """pairs: 96 bytes compress(L_i) || compress(R_i) per proof (zero: rejected before the pairing); kept as points"""
        cut = [pairs[96 * i:96 * i + 96] for i in range(len(self.expected))]
        self.points = [(bls.g1_decompress(c[:48]), bls.g1_decompress(c[48:])) if any(c) else None for c in cut]

    def model_pair(self, included, seed_used, chunk):
        """agg_model.model_pair over the first len(included) proofs, on the points decompressed once"""
        L = R = None
        for i, inc in enumerate(included):
            if inc:
                r = agg_model.coeff(seed_used, i, chunk)
                L, R = bls.g1_add(L, bls.g1_mul(self.points[i][0], r)), bls.g1_add(R, bls.g1_mul(self.points[i][1], r))
        return bls.g1_compress(L) + bls.g1_compress(R)

    def prefix(self, m, shift=0):
        """(proofs, offsets, instances) of the first m proofs; shift: that many junk bytes in front, every offset moved by it"""
        return b"\xee" * shift + self.proofs[:self.off[m]], [o + shift for o in self.off[:m + 1]], self.inst[:self.ioff[m]]


def _parts(k, batch, n_pi):
    return [(k, batch.proof(j), batch.instances[32 * n_pi * j:32 * n_pi * (j + 1)], batch.expected[j]) for j in range(batch.n)]


def _device_pairs(dp, batch):
    """n x 96 bytes: h2v_prepare_batch_device on one key's batch, a temporary workspace"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    proofs, inst, off = up(batch.proofs), up(batch.instances), torch.tensor(batch.proof_off, dtype=torch.int64, device=dev)
    pairs = torch.zeros(96 * batch.n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.current_stream().synchronize()
    dp.prepare_batch_device(batch.n, proofs.data_ptr(), off.data_ptr(), inst.data_ptr(), None, pairs.data_ptr(), None, stream=stream.cuda_stream)
    stream.synchronize()
    return bytes(pairs.cpu().tolist())


@pytest.fixture(scope="module")
def fx(be, circuits):
    """the single-key pool (simple_mul, 40 proofs), the mixed pool (simple_mul and lookup_table on one SRS, 20 each, alternating),
    every proof's pair (h2v_prepare_batch_device, a temporary workspace) and the plans; made once, never changed"""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td, pl, dp, _ov = circuits["simple_mul"]
    assert vk.n_committed_instances == 0
    b = synth.with_rejects(pl, synth.forge_batch(vk, td, 40, seed=81, plan=pl), vk.n_public_inputs, fraction=0.2, seed=REJECT_SEED, kinds=KINDS)
    single = Pool(_parts(0, b, vk.n_public_inputs))
    single.set_pairs(_device_pairs(dp, b))
    plans, per_key, key_pairs = [], [], []
    for k, name in enumerate(("simple_mul", "lookup_table")):
        vk_k, td_k = V.on_srs(circuits[name][0], circuits[name][1], COMMON_S)
        pl_k = PL.compile_plan(vk_k)
        assert vk_k.n_committed_instances == 0
        plans.append(be.DevicePlan(pl_k.to_bytes(), 0))
        bk = synth.with_rejects(pl_k, synth.forge_batch(vk_k, td_k, 20, seed=91 + k, plan=pl_k), vk_k.n_public_inputs, fraction=0.2,
                                seed=MIXED_REJECT_SEEDS[k], kinds=KINDS)
        per_key.append(_parts(k, bk, vk_k.n_public_inputs))
        key_pairs.append(_device_pairs(plans[k], bk))
    mixed = Pool([p for pair in zip(*per_key) for p in pair])
    mixed.set_pairs(b"".join(kp[96 * j:96 * j + 96] for j in range(20) for kp in key_pairs))
    for pool in (single, mixed):
        assert all(0 < sum(pool.expected[:m]) < m for m in SIZES if m >= 2), pool.expected
    return {"dp": dp, "plans": plans, "single": single, "mixed": mixed}


def _workspaces(be, fx, kind):
    """two workspaces of one kind that serve both plans of the mixed pool (and simple_mul's own plan: the same shape): an ordinary
    one of 64 proofs, or lanes=2, chunk=3.  Routing off: every RLC call takes the batch check first on both."""
    wide = max(fx["plans"], key=lambda p: p.n_terms)
    out = []
    for _ in range(2):
        ws = be.Workspace(wide, 64) if kind == "ordinary" else be.Workspace.multi(fx["plans"], 64, lanes=2, chunk=3)
        assert ws.lanes() == ((1, 64) if kind == "ordinary" else (2, 3))
        ws.set_option(be.OPT_RLC_ROUTE, -1)
        out.append(ws)
    return out


class Dev:
    """the *_device forms on torch tensors, on a stream of its own; every call returns host values after synchronising"""

    def __init__(self, be, fx, ws):
        import torch
        self.t, self.be, self.fx, self.ws = torch, be, fx, ws
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(device=self.dev)

    def _in(self, proofs, off, inst):
        t = self.t
        up = lambda b: t.frombuffer(bytearray(b), dtype=t.uint8).to(self.dev) if b else None
        keep = [up(proofs), t.tensor(off, dtype=t.int64, device=self.dev), up(inst)]
        t.cuda.current_stream().synchronize()
        return keep, [x.data_ptr() if x is not None else None for x in keep] + [None]

    def _out(self, n, dtype, fill):
        return self.t.full((max(1, n),), fill, dtype=dtype, device=self.dev)

    def _words(self, st, n):
        self.stream.synchronize()
        return [v & 0xffffffff for v in st.cpu().tolist()][:n]

    def _fell_back(self):
        return self.ws.rlc_verdict() == 0

    def prepare(self, proofs, off, inst):
        n = len(off) - 1
        _keep, ptrs = self._in(proofs, off, inst)
        pairs, st = self._out(96 * n, self.t.uint8, 0x5a), self._out(n, self.t.int32, -1)
        self.fx["dp"].prepare_batch_device(n, *ptrs, pairs.data_ptr(), st.data_ptr(), ws=self.ws, stream=self.stream.cuda_stream)
        words = self._words(st, n)
        return bytes(pairs.cpu().tolist()), words

    def check(self, pairs, rlc):
        n = len(pairs) // 96
        d_pairs = self.t.frombuffer(bytearray(pairs), dtype=self.t.uint8).to(self.dev)
        self.t.cuda.current_stream().synchronize()
        acc, st = self._out(n, self.t.uint8, 7), self._out(n, self.t.int32, -1)
        if rlc:
            self.fx["dp"].check_pairs_rlc_device(n, d_pairs.data_ptr(), acc.data_ptr(), st.data_ptr(), ws=self.ws, stream=self.stream.cuda_stream, seed=SEED)
        else:
            self.fx["dp"].check_pairs_device(n, d_pairs.data_ptr(), acc.data_ptr(), st.data_ptr(), ws=self.ws, stream=self.stream.cuda_stream)
        words = self._words(st, n)
        return (bytes(acc.cpu().tolist()[:n]), words) + ((self._fell_back(),) if rlc else ())

    def verify_rlc(self, proofs, off, inst):
        n = len(off) - 1
        _keep, ptrs = self._in(proofs, off, inst)
        acc = self._out(n, self.t.uint8, 7)
        self.fx["dp"].verify_batch_rlc_device(n, *ptrs, acc.data_ptr(), None, ws=self.ws, stream=self.stream.cuda_stream, seed=SEED)
        self.stream.synchronize()
        return bytes(acc.cpu().tolist()[:n]), self._fell_back()

    def aggregate(self, proofs, off, inst, plan_of=None):
        n = len(off) - 1
        _keep, ptrs = self._in(proofs, off, inst)
        pair, inc, st = self._out(96, self.t.uint8, 0x5a), self._out(n, self.t.uint8, 7), self._out(n, self.t.int32, -1)
        if plan_of is None:
            info = self.fx["dp"].aggregate_batch_device(n, *ptrs, pair.data_ptr(), inc.data_ptr(), st.data_ptr(), ws=self.ws,
                                                        stream=self.stream.cuda_stream, seed=SEED)
        else:
            info = self.be.aggregate_mixed_device(self.fx["plans"], plan_of, n, *ptrs, pair.data_ptr(), inc.data_ptr(), st.data_ptr(), ws=self.ws,
                                                  stream=self.stream.cuda_stream, seed=SEED)
        words = self._words(st, n)
        return _agg(self.fx["single" if plan_of is None else "mixed"], bytes(pair.cpu().tolist()), bytes(inc.cpu().tolist()[:n]), words, info)

    def mixed(self, plan_of, proofs, off, inst, mode, fold):
        n = len(off) - 1
        _keep, ptrs = self._in(proofs, off, inst)
        acc, st = self._out(n, self.t.uint8, 7), self._out(n, self.t.int32, -1)
        self.be.verify_mixed_device(self.fx["plans"], plan_of, n, *ptrs, acc.data_ptr(), st.data_ptr(), ws=self.ws, stream=self.stream.cuda_stream,
                                    mode=mode, seed=SEED if mode == "rlc" else None, fold_msm=fold)
        words = self._words(st, n)
        return bytes(acc.cpu().tolist()[:n]), words, (self._fell_back() if mode == "rlc" else False)


def _agg(pool, pair, included, status, info):
    """an aggregate call's outputs with the two that depend on the call counter replaced: the pair by whether it is the model's
    under the seed the call reports, that seed by its words outside the counter's (rlc_seed: words 5 and 6)"""
    seed = struct.unpack("<8I", bytes(info.seed_used))
    return (pair == pool.model_pair(included, bytes(info.seed_used), info.chunk), included, status,
            (seed[:5] + seed[7:], info.chunk, info.n_chunks, info.msm_terms))


MIXED_MODES = [("per-proof", False), ("rlc", False), ("rlc", True)]     # plain, H2V_MIXED_RLC, H2V_MIXED_FOLD_MSM


def _host_forms(be, fx, ws, m, shift=0):
    """every host form on the first m proofs, interleaved on ws: prepare, check, aggregate, mixed.  name -> result"""
    dp, single, mixed = fx["dp"], fx["single"], fx["mixed"]
    pr, off, ins = single.prefix(m, shift)
    mp, moff, mins = mixed.prefix(m, shift)
    plan_of = mixed.plan_of[:m]
    out = {"prepare": dp.prepare_batch(pr, off, ins, None, ws=ws)}
    pairs = out["prepare"][0]
    out["check"] = dp.check_pairs(pairs, ws=ws)
    out["check_rlc"] = dp.check_pairs_rlc(pairs, ws=ws, seed=SEED)
    out["aggregate"] = _agg(single, *dp.aggregate_batch(pr, off, ins, None, ws=ws, seed=SEED))
    out["verify_rlc"] = dp.verify_batch_rlc(pr, off, ins, None, ws=ws, seed=SEED)
    for mode, fold in MIXED_MODES:
        out["mixed", mode, fold] = be.verify_mixed(fx["plans"], plan_of, mp, moff, mins, None, ws=ws, mode=mode,
                                                   seed=SEED if mode == "rlc" else None, fold_msm=fold)
    out["aggregate_mixed"] = _agg(mixed, *be.aggregate_mixed(fx["plans"], plan_of, mp, moff, mins, None, ws=ws, seed=SEED))
    return out


def _device_forms(dev, fx, m):
    single, mixed = fx["single"], fx["mixed"]
    pr, off, ins = single.prefix(m)
    mp, moff, mins = mixed.prefix(m)
    plan_of = mixed.plan_of[:m]
    out = {"prepare": dev.prepare(pr, off, ins)}
    pairs = out["prepare"][0]
    out["check"] = dev.check(pairs, False)
    out["check_rlc"] = dev.check(pairs, True)
    out["aggregate"] = dev.aggregate(pr, off, ins)
    out["verify_rlc"] = dev.verify_rlc(pr, off, ins)
    for mode, fold in MIXED_MODES:
        out["mixed", mode, fold] = dev.mixed(plan_of, mp, moff, mins, mode, fold)
    out["aggregate_mixed"] = dev.aggregate(mp, moff, mins, plan_of)
    return out


@pytest.mark.parametrize("kind", ["ordinary", "laned"])
def test_host_forms_equal_device_forms_while_blocks_regrow(be, fx, kind):
    ws, ref_ws = _workspaces(be, fx, kind)
    dev = Dev(be, fx, ref_ws)
    fell_back = set()
    for m in SIZES:
        got, want = _host_forms(be, fx, ws, m), _device_forms(dev, fx, m)
        for name in want:
            assert tuple(got[name]) == tuple(want[name]), (kind, m, name)
        # ... and both are right, not merely equal: the verdicts by construction, included[] = "reached the pairing"
        exp, mexp = bytes(fx["single"].expected[:m]), bytes(fx["mixed"].expected[:m])
        assert got["check"][0] == got["check_rlc"][0] == got["verify_rlc"][0] == exp, (kind, m)
        assert all(got["mixed", mode, fold][0] == mexp for mode, fold in MIXED_MODES), (kind, m)
        assert got["aggregate"][1] == bytes(int(s == 0) for s in got["prepare"][1]), (kind, m)
        given = struct.unpack("<8I", SEED)
        for name in ("aggregate", "aggregate_mixed"):      # the pair is the model's, the seed the given one
            assert got[name][0] is True and want[name][0] is True and got[name][3][0] == given[:5] + given[7:], (kind, m, name)
        assert got["check_rlc"][2] == got["verify_rlc"][1] == any(s == be.ST_PAIRING for s in got["check"][1]), (kind, m)
        fell_back.add(got["verify_rlc"][1])
    assert fell_back == {False, True}
    ws.close()
    ref_ws.close()


def _null_status_calls(be, fx, ws, m):
    """every form that takes status[], called through the library directly with status = NULL: name -> what it still returns"""
    L, dp = be.lib(), fx["dp"]
    pr, off, ins = fx["single"].prefix(m)
    _n, b, _keep = dp._host_batch(pr, off, ins, None)
    opts = be._rlc_opts(SEED)
    pairs, acc, pair, fb = C.create_string_buffer(96 * m), (C.c_uint8 * m)(), C.create_string_buffer(96), C.c_int(0)
    out = {}
    be.check(L.h2v_prepare_batch(dp.handle, C.byref(b), pairs, None, ws.handle))
    out["prepare"] = pairs.raw
    be.check(L.h2v_check_pairs(dp.handle, m, pairs.raw, acc, None, ws.handle))
    out["check"] = bytes(acc)
    be.check(L.h2v_check_pairs_rlc(dp.handle, m, pairs.raw, acc, None, ws.handle, C.byref(opts), C.byref(fb)))
    out["check_rlc"] = (bytes(acc), bool(fb.value))
    info = be.AggregateInfo()
    be.check(L.h2v_aggregate_batch(dp.handle, C.byref(b), pair, acc, None, ws.handle, C.byref(opts), C.byref(info)))
    out["aggregate"] = (pair.raw == fx["single"].model_pair(bytes(acc), bytes(info.seed_used), info.chunk), bytes(acc))
    mp, moff, mins = fx["mixed"].prefix(m)
    arr = (C.c_void_p * 2)(*[p.handle for p in fx["plans"]])
    po, moffs = (C.c_uint32 * m)(*fx["mixed"].plan_of[:m]), (C.c_uint64 * (m + 1))(*moff)
    pbuf, ibuf = C.create_string_buffer(mp, len(mp)), C.create_string_buffer(mins, len(mins))
    mb = be.MixedBatch(m, C.cast(po, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(moffs, C.c_void_p), C.cast(ibuf, C.c_void_p), None)
    for mode, fold in MIXED_MODES:
        be.check(L.h2v_verify_mixed(arr, 2, C.byref(mb), acc, None, ws.handle, be._mixed_mode(mode, fold), C.byref(opts) if mode == "rlc" else None,
                                    C.byref(fb)))
        out["mixed", mode, fold] = (bytes(acc), bool(fb.value))
    be.check(L.h2v_aggregate_mixed(arr, 2, C.byref(mb), pair, acc, None, ws.handle, C.byref(opts), C.byref(info)))
    out["aggregate_mixed"] = (pair.raw == fx["mixed"].model_pair(bytes(acc), bytes(info.seed_used), info.chunk), bytes(acc))
    return out


@pytest.mark.parametrize("kind", ["ordinary", "laned"])
def test_optional_status_and_a_nonzero_first_offset(be, fx, kind):
    """status = NULL: the same pairs / accept / included / fell_back come back, and the aggregate pair is the model's.
    proof_off[0] = 48 - junk bytes in front of the first proof, every offset moved: the same results as the unshifted call (the
    packer rebases, no kernel reads the junk)."""
    ws, _other = _workspaces(be, fx, kind)
    _other.close()
    m = 17
    base = _host_forms(be, fx, ws, m)
    assert base["aggregate"][0] is True and base["aggregate_mixed"][0] is True
    assert {name: tuple(v) for name, v in _host_forms(be, fx, ws, m, shift=48).items()} == {name: tuple(v) for name, v in base.items()}
    got = _null_status_calls(be, fx, ws, m)
    assert got["prepare"] == base["prepare"][0] and got["check"] == base["check"][0]
    assert got["check_rlc"] == (base["check_rlc"][0], base["check_rlc"][2])
    assert got["aggregate"] == base["aggregate"][:2] and got["aggregate_mixed"] == base["aggregate_mixed"][:2]
    for mode, fold in MIXED_MODES:
        assert got["mixed", mode, fold] == (base["mixed", mode, fold][0], base["mixed", mode, fold][2]), (mode, fold)
    ws.close()
