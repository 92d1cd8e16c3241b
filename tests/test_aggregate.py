"""Aggregate calls (include/h2v.h: h2v_aggregate_batch / h2v_aggregate_mixed), what can be said without a GPU: the header declares
the entry points, the info struct and H2V_BATCH_NOT_CHECKED, the library exports them and the binding matches; the argument rules
that can be reached without a plan come back before any device call (NO plan or workspace exists without a device, so no aggregate
entry point can be driven as far as H2V_E_DEVICE here: the C++ leg's "error -3" is h2v_plan_load's, in VerifyingKey's constructor);
the big-integer model of the pair (tests/agg_model.py) satisfies the pairing equation exactly when every included proof does; aggregate_sharded gathers pairs and included bytes on rank 0.  GPU legs: tests/test_aggregate_gpu.py."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import agg_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["h2v_aggregate_batch", "h2v_aggregate_batch_device", "h2v_aggregate_mixed", "h2v_aggregate_mixed_device"]
E_ARG, E_DEVICE, E_LIMIT = -1, -3, -4
INF_PAIR = (b"\xc0" + bytes(47)) * 2


def _header():
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        return f.read()


def _arg_count(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, _header(), re.S)
    assert m, name
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


def test_header_library_and_binding_agree():
    """fails on a tree without the feature: nothing declares, exports or binds these names"""
    from plutus_halo2_verifier_gen_amd import backend
    h = _header()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in backend.EXPORTS, name
    m = re.search(r"#define\s+H2V_BATCH_NOT_CHECKED\s+(\d+)u", h)
    assert m and int(m.group(1)) == 2 == backend.BATCH_NOT_CHECKED
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2v_aggregate_info;", h)
    assert m
    fields = re.findall(r"(uint8_t|uint32_t)\s+(\w+)(\[32\])?;", m.group(1))
    assert [(t, n, bool(a)) for t, n, a in fields] == [("uint8_t", "seed_used", True), ("uint32_t", "chunk", False), ("uint32_t", "n_chunks", False),
                                                      ("uint32_t", "msm_terms", False), ("uint32_t", "reserved", False)]
    assert [n for n, _ in backend.AggregateInfo._fields_] == [n for _, n, _ in fields]
    assert C.sizeof(backend.AggregateInfo) == 48
    L = backend.lib()
    for name, nargs in zip(ENTRY_POINTS, (8, 9, 9, 10)):
        assert len(getattr(L, name).argtypes) == _arg_count(name) == nargs, name
    # the entry points of the Python layers
    from plutus_halo2_verifier_gen_amd import api, shard
    assert callable(backend.DevicePlan.aggregate_batch) and callable(backend.DevicePlan.aggregate_batch_device)
    assert callable(backend.aggregate_mixed) and callable(backend.aggregate_mixed_device)
    assert callable(api.Verifier.aggregate_batch) and callable(api.Aggregator) and callable(shard.aggregate_sharded)


def test_argument_rules_come_back_before_any_device_call():
    """what can be reached without a plan (no plan loads without a GPU): null arguments and unknown flags are H2V_E_ARG, too
    many plans H2V_E_LIMIT; an empty mixed call is H2V_OK and writes (inf, inf) and the info without touching a device"""
    from plutus_halo2_verifier_gen_amd import backend
    L = backend.lib()
    pair = C.create_string_buffer(96)
    inc = (C.c_uint8 * 4)()
    b = backend.Batch(1, None, None, None, None)
    info = backend.AggregateInfo()
    assert L.h2v_aggregate_batch(None, C.byref(b), pair, inc, None, None, None, None) == E_ARG
    assert L.h2v_aggregate_batch_device(None, C.byref(b), C.addressof(pair), C.addressof(inc), None, None, None, None, None) == E_ARG
    mb = backend.MixedBatch(0, None, None, None, None, None)
    plans = (C.c_void_p * 1)()
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), None, inc, None, None, None, None) == E_ARG            # pair == NULL
    assert L.h2v_aggregate_mixed(None, 0, C.byref(mb), pair, inc, None, None, None, None) == E_ARG             # plans == NULL
    assert L.h2v_aggregate_mixed_device(plans, 0, None, C.addressof(pair), None, None, None, None, None, None) == E_ARG   # batch == NULL
    bad = backend.RlcOpts((C.c_uint8 * 32)(), 8)
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, inc, None, None, C.byref(bad), None) == E_ARG    # an unknown flag
    many = (C.c_void_p * 65)()
    assert L.h2v_aggregate_mixed(many, 65, C.byref(mb), pair, inc, None, None, None, None) == E_LIMIT
    assert L.h2v_aggregate_mixed_device(plans, 0, C.byref(mb), C.addressof(pair), None, None, None, None, None, None) == E_ARG   # ws == NULL
    # n = 0, host form: H2V_OK, (inf, inf), the given seed (with the call count mixed into words 5 and 6) in the info
    seed = bytes(range(32))
    ok = backend.RlcOpts((C.c_uint8 * 32)(*seed), backend.RLC_SEED_GIVEN | backend.RLC_FOLD_PAIRS | backend.RLC_ONE_STREAM)
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, None, None, None, C.byref(ok), C.byref(info)) == 0
    assert pair.raw == INF_PAIR
    assert bytes(info.seed_used)[:20] == seed[:20] and bytes(info.seed_used)[28:] == seed[28:]
    assert (info.chunk, info.n_chunks, info.msm_terms) == (0, 1, 0)
    p, inc2, st, info2 = backend.aggregate_mixed([], [], b"", [0], None, None)
    assert (p, inc2, st) == (INF_PAIR, b"", [])
    assert "h2v_plan_same_srs" in backend.EXPORTS and L.h2v_plan_same_srs(None, None) == E_ARG


def test_api_refuses_a_key_of_another_srs():
    from plutus_halo2_verifier_gen_amd import api, vk as V
    vk, _td = V.simple_mul_vk()
    other = bytearray(bytes.fromhex(vk.s_g2))
    other[-1] ^= 1
    agg = api.Aggregator(api.ParamsVerifierKZG(bytes(other)))
    with pytest.raises(ValueError):
        agg.push(vk, [], [])
    assert api.Aggregator(api.ParamsVerifierKZG(bytes.fromhex(vk.s_g2))).finish() == ([], [])


def _oracle_pairs(orc, vk, batch):
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    pairs, oks = [], []
    for i in range(batch.n):
        ok, otr = ov.verify(batch.proof(i), batch.instance_ints(i, vk.n_public_inputs), batch.ci(i), trace=True)
        assert otr.status in (0, 1)
        pairs.append(orc.g1_compress(otr.point("el")) + orc.g1_compress(otr.point("er")))
        oks.append(int(ok))
    return pairs, oks


def test_model_pair_satisfies_the_equation_iff_every_included_proof_does(orc):
    """a forged accepting simple_mul batch of 5 proofs: the model's pair from the oracle's el / er has R = [s] L (s: the SRS
    trapdoor) on an ordinary workspace's coefficients and on a laned one's; with one wrong_pi proof it does not - and with that
    proof excluded it does again"""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    batch = synth.forge_batch(vk, td, 5, seed=17, plan=pl, workers=1)
    pairs, oks = _oracle_pairs(orc, vk, batch)
    assert oks == [1] * 5
    seed = bytes(random.Random(3).randrange(256) for _ in range(32))
    for chunk in (0, 2):
        pair = agg_model.model_pair(pairs, [1] * 5, seed, chunk)
        assert agg_model.holds(pair, td.s) and pair != INF_PAIR
    assert agg_model.model_pair(pairs, [1] * 5, seed, 0) != agg_model.model_pair(pairs, [1] * 5, seed, 2)      # (the chunk tweak moves the coefficients)
    assert agg_model.coeff(seed, 3, 2) != agg_model.coeff(seed, 1, 0)                                            # (position 1 of chunk 1 is not position 1 of the call)
    assert agg_model.model_pair(pairs, [0] * 5, seed) == INF_PAIR
    proofs = [batch.proof(i) for i in range(5)]
    proofs[3] = synth.corrupt(pl, proofs[3], b"", "wrong_pi", random.Random(4))[0]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    bad = synth.Batch(n=5, proofs=b"".join(proofs), proof_off=off, instances=batch.instances, committed=batch.committed, expected=[1, 1, 1, 0, 1])
    pairs_bad, oks_bad = _oracle_pairs(orc, vk, bad)
    assert oks_bad == bad.expected
    assert not agg_model.holds(agg_model.model_pair(pairs_bad, [1] * 5, seed), td.s)
    assert agg_model.holds(agg_model.model_pair(pairs_bad, [1, 1, 1, 0, 1], seed), td.s)


GLOO_WORKER = r'''
import json, os, random, sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from plutus_halo2_verifier_gen_amd import plan as PL, shard, synth, vk as V
from oracle import binding as orc
from tests import agg_model
orc.build()
dist.init_process_group(backend="gloo")
vk, td = V.simple_mul_vk()
pl = PL.compile_plan(vk)
n_pi = vk.n_public_inputs
b = synth.forge_batch(vk, td, 7, seed=4, plan=pl, workers=1)
proofs = [b.proof(i) for i in range(7)]
proofs[1] = synth.corrupt(pl, proofs[1], b"", "bad_point_flag", random.Random(1))[0]      # rank 0's range: excluded, its pair passes
proofs[5] = synth.corrupt(pl, proofs[5], b"", "wrong_pi", random.Random(2))[0]            # rank 1's range: included, its pair fails
off = [0]
for p in proofs:
    off.append(off[-1] + len(p))
raw = b"".join(proofs)
ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
seed = bytes([dist.get_rank() + 1]) * 32
def aggregate(proofs, off, inst, ci):       # the model stands in for h2v_aggregate_batch
    pairs, inc = [], []
    for i in range(len(off) - 1):
        ints = [int.from_bytes(inst[32 * (n_pi * i + k):32 * (n_pi * i + k + 1)], "little") for k in range(n_pi)]
        ok, otr = ov.verify(proofs[off[i]:off[i + 1]], ints, None, trace=True)
        reached = otr.status in (0, 1)
        inc.append(1 if reached else 0)
        pairs.append(orc.g1_compress(otr.point("el")) + orc.g1_compress(otr.point("er")) if reached else bytes(96))
    return agg_model.model_pair(pairs, inc, seed), bytes(inc)
calls = []
def check(pairs):                            # a trapdoor check stands in for h2v_check_pairs_rlc
    calls.append(len(pairs))
    return [agg_model.holds(p, td.s) for p in pairs]
out = shard.aggregate_sharded(aggregate, check, raw, off, b.instances, b.committed, n_pi)
if dist.get_rank() == 0:
    verdicts, included = out
    assert calls == [2], calls               # ONE check over the node's pairs
    assert verdicts == [True, False], verdicts
    assert list(included) == [1, 0, 1, 1, 1, 1, 1], list(included)
    print("AGG_GLOO_OK", verdicts, list(included))
else:
    assert out is None and calls == []
dist.destroy_process_group()
'''


def test_aggregate_sharded_two_ranks_gloo(tmp_path):
    """world_size 2 over gloo: every rank aggregates its range, 96-byte pairs and included bytes are gathered on rank 0, which
    checks once; the rank whose range holds a wrong_pi proof is the one whose verdict is False"""
    script = tmp_path / "worker.py"
    script.write_text(GLOO_WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29547", str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "AGG_GLOO_OK" in res.stdout


def test_aggregate_sharded_single_process():
    from plutus_halo2_verifier_gen_amd import shard
    seen = []

    def aggregate(proofs, off, inst, ci):
        seen.append((proofs, off))
        return INF_PAIR, bytes([1] * (len(off) - 1))

    verdicts, included = shard.aggregate_sharded(aggregate, lambda pairs: [p == INF_PAIR for p in pairs], b"abcdef", [0, 2, 6], b"", None, 0)
    assert verdicts == [True] and included == b"\x01\x01" and seen == [(b"abcdef", [0, 2, 6])]
    with pytest.raises(ValueError):
        shard.aggregate_sharded(lambda *a: (b"short", b""), lambda p: [], b"ab", [0, 2], b"", None, 0)
