"""CPU tests (no GPU): plan compiler vs the oracle on forged proofs, the big-integer plan interpreter, host logic,
the C-ABI library's exported symbols, and the multi-process sharding path over gloo."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from plutus_halo2_verifier_gen_amd import plan as PL
from plutus_halo2_verifier_gen_amd import shard, synth
from plutus_halo2_verifier_gen_amd import vk as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bls.R


def _oracle_vk(orc, vk):
    return orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))


@pytest.fixture(scope="module")
def simple(orc):
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    return vk, td, pl, _oracle_vk(orc, vk)


def test_domain_constants(kats):
    # omega / omega^-1 of the reference's n = 2^14 KAT (omega_rotations.ak:48-81) come out of the domain derivation
    k = kats["rotations"]
    assert V.domain_omega(14) == int(k["omega"], 16)
    assert bls.fr_inv(V.domain_omega(14)) == int(k["omega_inv"], 16)
    assert int(kats["lagrange_basis"]["barycentric_weight"], 16) == bls.fr_inv(1 << 14)


def test_simple_mul_layout(simple):
    vk, td, pl, ov = simple
    # 10 G1 + 20 Fr = 1120 bytes (transcript.ak:246), 16 MSM terms, 3 point sets (ProofData.hs:176-197)
    assert pl.proof_len == 1120 == ov.proof_len
    assert len(pl.points) == 10 and pl.n_terms == 16 == ov.n_msm_terms
    assert ov.n_point_sets == 3
    assert pl.point_names[-1] == "pi" and pl.pi_point == 9
    assert pl.n_squeezes == 10  # theta beta gamma trash y x x1 x2 x3 x4


@pytest.mark.parametrize("name", sorted(V.BUILDERS))
def test_forged_proofs_accept_and_corruptions_reject(orc, name):
    """Plan compiler + forger (Python, product host side) against the independent C oracle."""
    vk, td = V.BUILDERS[name]()
    pl = PL.compile_plan(vk)
    ov = _oracle_vk(orc, vk)
    assert pl.proof_len == ov.proof_len and pl.n_main_terms == ov.n_msm_terms
    b = synth.forge_batch(vk, td, 3, seed=5, plan=pl, workers=1, ci_identity=(name == "sha256"))
    for i in range(b.n):
        assert ov.verify(b.proof(i), b.instance_ints(i, vk.n_public_inputs), b.ci(i))
    rng = random.Random(2)
    n_pi = vk.n_public_inputs
    expected_status = {"flip_first_scalar": "pairing", "flip_last_scalar": "pairing", "bad_point_flag": "point",
                       "point_not_on_curve": "point", "point_not_in_subgroup": "point", "noncanonical_scalar": "scalar",
                       "noncanonical_instance": "scalar",
                       "wrong_public_input": "pairing", "wrong_pi": "pairing", "truncated": "short",
                       "infinity_commitment": "pairing", "acc_limb": "point", "acc_scalar": "pairing",
                       "acc_fixed_scalar": "pairing", "acc_sign": "pairing", "acc_vk_hash": "recursion"}
    if vk.recursion_vks is not None:
        expected_status["wrong_public_input"] = "recursion"   # input 0 of a recursive circuit is the verifying-key hash
    for kind in synth.CORRUPTIONS:
        res = synth.corrupt(pl, b.proof(1), b.instances[32 * n_pi:64 * n_pi], kind, rng)
        if res is None:
            continue
        p2, i2 = res
        inst = [int.from_bytes(i2[32 * k:32 * k + 32], "little") for k in range(n_pi)]
        ok, tr = ov.verify(p2, inst, b.ci(1), trace=True)
        assert not ok
        assert orc.STATUS[tr.status] == expected_status[kind] or (kind == "acc_limb" and orc.STATUS[tr.status] == "pairing"), kind


def test_plan_interpreter_matches_oracle_trace(simple, orc):
    """Every named intermediate value of the compiled program equals the oracle's (the reference's plutus_debug
    trace surface: theta..v and every expression_i)."""
    vk, td, pl, ov = simple
    b = synth.forge_batch(vk, td, 2, seed=9, plan=pl, workers=1)
    for i in range(2):
        scal, regs, status = PL.run_plan(pl, b.proof(i), b.instance_ints(i, 3), None)
        assert status is None
        ok, tr = ov.verify(b.proof(i), b.instance_ints(i, 3), None, trace=True)
        assert ok
        for slot, reg in pl.trace:
            if slot < PL.TRACE_EXPR0:
                assert regs[reg] == tr.scalar(PL.TRACE_NAMES[slot]), PL.TRACE_NAMES[slot]
            else:
                assert regs[reg] == tr.expression(slot - PL.TRACE_EXPR0)
        # the flattened MSM reproduces er
        bases = []
        pts = [bls.g1_decompress(b.proof(i)[o:o + 48]) for o in pl.points]
        for kind, idx in pl.terms:
            bases.append(pts[idx] if kind == PL.TERM_PROOF_POINT else pl.vk_bases[idx])
        assert orc.g1_msm(scal, bases) == tr.point("er")


def test_legacy_layout_replays_the_golden_proof(simple, kats):
    """compile_plan(legacy_no_trash_squeeze=True) is the layout of the reference's in-tree proof (transcript.ak:241-382):
    the plan interpreter reproduces every value of that vector (the GPU test replays the same plan on the device)."""
    vk, td, pl, ov = simple
    k = kats["simple_mul_full"]
    pl2 = PL.compile_plan(vk, legacy_no_trash_squeeze=True)
    assert pl2.proof_len == 1120 and pl2.n_squeezes == pl.n_squeezes - 1
    scal, regs, status = PL.run_plan(pl2, bytes.fromhex(k["proof"]), [42, 42, 42], None)
    assert status is None
    got = {PL.TRACE_NAMES[s]: regs[r] for s, r in pl2.trace if s < PL.TRACE_EXPR0}
    for name in ("gamma", "y", "x", "advice_eval_1", "advice_eval_2", "advice_eval_3", "x1", "x2", "x3", "x4"):
        assert got[name] == int(k[name], 16), name
    assert pl2.points[pl2.pi_point] == 1120 - 48 and bytes.fromhex(k["proof"])[-48:] == bytes.fromhex(k["pi"])


def test_plan_rejects_in_interpreter(simple):
    vk, td, pl, ov = simple
    b = synth.forge_batch(vk, td, 1, seed=3, plan=pl, workers=1)
    rng = random.Random(1)
    p2, i2 = synth.corrupt(pl, b.proof(0), b.instances, "noncanonical_scalar", rng)
    assert PL.run_plan(pl, p2, b.instance_ints(0, 3), None)[2] == "scalar"
    assert PL.run_plan(pl, b.proof(0)[:-1], b.instance_ints(0, 3), None)[2] == "short"


def test_plan_blob_layout(simple):
    vk, td, pl, ov = simple
    blob = pl.to_bytes()
    assert blob[:8] == PL.PLAN_MAGIC
    hdr = [int.from_bytes(blob[8 + 4 * i:12 + 4 * i], "little") for i in range(PL.PLAN_HDR_WORDS)]
    assert hdr[0] == PL.PLAN_VERSION and hdr[1] == 1120 and hdr[22] == len(blob)
    assert all(o % 16 == 0 for o in hdr[14:22] + hdr[23:25])
    # committed-instance circuits carry exactly one kind-2 term
    vk2, _ = V.sha256_vk()
    pl2 = PL.compile_plan(vk2)
    assert sum(1 for k, _ in pl2.terms if k == PL.TERM_COMMITTED_INSTANCE) == 1
    assert pl2.n_terms == 60


# rotation sets in the BTreeMap order of the reference's RotationSet (stats/chips/types/rotation_set.rs:2-11: Ord over the
# flags first, prev, curr, next, next2, next3, last; false < true) - the order docs/chip_profiles.json lists the sets in
_PROFILE_SET_ORDER = [(0,), (0, 1), (PL.ROT_LAST, 0, 1), (-1, 0), (-1, 0, 1)]


def _set_sizes(pl):
    sizes = {}
    for e in pl.commitment_map:
        key = tuple(r for r, _ in e["pairs"])
        sizes[key] = sizes.get(key, 0) + 1
    assert set(sizes) <= set(_PROFILE_SET_ORDER)
    return [[len(k), sizes[k]] for k in _PROFILE_SET_ORDER if k in sizes]


@pytest.mark.parametrize("name", ["sha256", "secp256k1"])
def test_chip_shapes_match_reference_profile(kats, name):
    """BASELINE configs[3] / [4] are built on /root/reference/docs/chip_profiles.json (fixture "chip_profiles", extracted by
    tests/golden/make_reference_fixtures.py).  The chip-alone variant of the synthetic key (pi = 1, ci = 0, the profile's
    own setting) compiles to EXACTLY the profile's numbers; the example-wrapper variant differs from it by the deltas
    asserted one by one below."""
    prof = kats["chip_profiles"][name]
    mine = {"sha256": V.SHA256_PROFILE, "secp256k1": V.SECP256K1_PROFILE}[name]
    for k, v in mine.items():
        assert prof[k] == v, k                      # the literals in vk.py are the reference's
    vk, _ = V.BUILDERS[name](chip_alone=True)
    V.validate(vk)
    pl = PL.compile_plan(vk)
    d = prof["degree"]
    assert vk.cs_degree == d and vk.num_advice_columns == prof["advice_cols"] and vk.num_fixed_columns == prof["fixed_cols"]
    assert len(vk.permutation_columns) == prof["copy_constraints"] and vk.n_public_inputs == 1 and vk.n_committed_instances == 0
    assert len(vk.gates) == prof["gate_expressions"]
    assert sum(len(i) for i, _ in vk.lookups) == prof["lookups"]
    # commitments: the proof's G1 count and the VK's
    assert len(pl.points) == prof["proof_commitments"]
    assert len(vk.fixed_commitments) + len(vk.permutation_commitments) == prof["vk_commitments"]
    # the commitment map, set by set in the profile's order (stats/estimate/build.rs:252-273 / profile.rs:121-132)
    assert _set_sizes(pl) == prof["commitment_map_sets"]
    n_map = sum(c for _, c in prof["commitment_map_sets"])
    assert len(pl.commitment_map) == n_map
    # MSM width: every commitment of the map, vanishing_g expanded over its degree - 1 splits, + F, -G1, pi (App. A.3)
    assert pl.n_terms == (n_map - 1) + (d - 1) + 3 == 57
    # gate / lookup op counts: the profile's figures are the expressions' own plus one add + one mul per batched
    # expression (ScalarExpression::batch_expressions, stats/chips/types/expression.rs:52-66)
    own = {"neg": 0, "add": 0, "mul": 0, "const": 0}
    for g in vk.gates:
        V.expr_op_counts(g, own)
    batching = prof["gate_expressions"] - prof["gates"]
    assert own == {"neg": prof["gate_ops"]["neg"], "add": prof["gate_ops"]["add"] - batching,
                   "mul": prof["gate_ops"]["mul"] - batching, "const": prof["gate_ops"]["from_int"]}
    assert max(V.expr_degree(g) for g in vk.gates) <= d
    lk = {"neg": 0, "add": 0, "mul": 0, "const": 0}
    for ins, tabs in vk.lookups:
        for e in list(ins) + list(tabs):
            V.expr_op_counts(e, lk)
    lbatch = prof["lookups"] - len(vk.lookups)
    assert lk == {"neg": prof["lookup_ops"]["neg"], "add": prof["lookup_ops"]["add"] - lbatch,
                  "mul": prof["lookup_ops"]["mul"] - lbatch, "const": prof["lookup_ops"]["from_int"]}
    # evaluations and proof bytes.  The profile passes the number of advice + fixed COLUMNS as `nb_evaluations`
    # (profile.rs:112), the estimator proper counts one evaluation per QUERY (estimate/build.rs:186-188) and so does a
    # proof: the difference is exactly (#advice queries - #advice columns) scalars (fixed columns are queried once)
    n_fr = (pl.proof_len - 48 * len(pl.points)) // 32
    per_query_extra = len(vk.advice_queries) - vk.num_advice_columns
    assert len(vk.fixed_queries) == vk.num_fixed_columns
    assert n_fr == prof["evals"] + per_query_extra
    assert pl.proof_len == prof["proof_size"] + 32 * per_query_extra
    assert pl.proof_len == {"sha256": 3712, "secp256k1": 3632}[name]
    # App. A.1 closed form with this key's counts
    L, cc, S = len(vk.lookups), len(vk.permutation_columns), len(prof["commitment_map_sets"])
    chunks = -(-cc // (d - 2))
    assert len(pl.points) == vk.num_advice_columns + 3 * L + chunks + 1 + (d - 1) + 2
    assert n_fr == len(vk.advice_queries) + len(vk.fixed_queries) + 1 + cc + (3 * chunks - 1) + 5 * L + S

    # ---- the example wrapper (examples/sha256.rs:42,131-137: 32 public inputs + one committed instance column)
    wk, _ = V.BUILDERS[name]()
    wp = PL.compile_plan(wk)
    assert wk.n_committed_instances == 1 and wk.n_public_inputs == {"sha256": 32, "secp256k1": 4}[name]
    assert wk.gates == vk.gates and wk.lookups == vk.lookups and wk.advice_queries == vk.advice_queries
    # both instance columns are copy-constrained (estimate/build.rs:166-177): two more sigma commitments, same chunk count
    assert wk.permutation_columns == vk.permutation_columns + [("instance", 0), ("instance", 1)]
    assert -(-len(wk.permutation_columns) // (d - 2)) == chunks and len(wp.points) == len(pl.points)
    assert len(wk.permutation_commitments) == len(vk.permutation_commitments) + 2
    # the committed column is opened at x: {cur} grows by the two sigmas + that column, nothing else moves
    want = [list(x) for x in prof["commitment_map_sets"]]
    want[0][1] += 3
    assert _set_sizes(wp) == want
    assert wp.n_terms == pl.n_terms + 3 and sum(1 for k, _ in wp.terms if k == PL.TERM_COMMITTED_INSTANCE) == 1
    # three more evaluations in the proof (the committed column's and the two sigmas'): 96 bytes
    assert wp.proof_len == pl.proof_len + 96
    assert wp.stream_len == pl.stream_len + 96 + 3 + 49 + 33 * (wk.n_public_inputs - 1)


def test_vk_json_roundtrip():
    vk, _ = V.atms_with_lookups_vk()
    vk2 = V.VerifyingKey.from_json(vk.to_json())
    assert vk2 == vk
    assert PL.compile_plan(vk2).to_bytes() == PL.compile_plan(vk).to_bytes()


def test_coop_tables_self_check():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_coop_tables
    assert gen_coop_tables.self_check()


def test_six_lane_tables_self_check():
    """The six-lanes-per-proof pairing engine (csrc/h2v_pairing_six.hpp): its operand tables against big-integer Fp12 arithmetic,
    and a limb-for-limb model of the device engine (28-bit limbs, wrapping 64-bit columns, signed / unsigned Montgomery reduction)
    with the column headroom asserted from the staged slots' limb bounds."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_six_tables
    assert gen_six_tables.self_check()


def test_g2_line_table_matches_pairing():
    """The precomputed line tables shipped in the plan reproduce the big-integer pairing (bilinearity)."""
    rng = random.Random(8)
    a, b_ = rng.randrange(1, R), rng.randrange(1, R)
    q = bls.g2_mul(bls.G2_GEN, b_)
    assert len(bls.g2_line_table(q)) == PL.MILLER_LINES
    assert bls.pairing_check_eq(bls.g1_mul(bls.G1_GEN, a), q, bls.g1_mul(bls.G1_GEN, a * b_ % R), bls.G2_GEN)


def test_c_abi_library_exports_every_declared_symbol():
    """include/h2v.h <-> libh2v_hip.so: every declared entry point is exported (no compute calls without a GPU)."""
    import __graft_entry__ as ge
    lib_path = ge.build_hip()
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(h2v_[a-z0-9_]+)\s*\(", header))
    declared -= {"h2v_verify_batch_ex"}  # mentioned in a comment only
    lib = ctypes.CDLL(lib_path)
    for name in sorted(declared):
        assert hasattr(lib, name), name
    from plutus_halo2_verifier_gen_amd import backend
    assert declared == set(backend.EXPORTS)


def test_shutdown_is_exported_and_idempotent_without_a_gpu():
    """h2v_shutdown (include/h2v.h: library lifecycle) is exported, succeeds with nothing to release (no GPU needed), is
    idempotent, rejects a bad device index, and the process still exits 0 afterwards.  Child process: the call marks the
    devices shut for the rest of the process."""
    import subprocess
    import sys
    import __graft_entry__ as ge
    script = ("import ctypes\n"
              "L = ctypes.CDLL(%r)\n"
              "L.h2v_shutdown.argtypes = [ctypes.c_int]\n"
              "assert L.h2v_shutdown(-1) == 0 and L.h2v_shutdown(-1) == 0 and L.h2v_shutdown(0) == 0\n"
              "assert L.h2v_shutdown(99) == -1 and L.h2v_shutdown(-2) == -1\n"
              "print('shutdown ok')\n" % ge.build_hip())
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shutdown ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_retired_option_ids_are_refused_without_a_gpu():
    """Option ids 9 and 10 (the retired decompression forms and sub-pipelines, include/h2v.h) are not reused: the option
    check refuses them with H2V_E_ARG before anything touches a device."""
    L = ctypes.CDLL(os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "libh2v_hip.so"))
    L.h2v_probe_set_option.argtypes = [ctypes.c_uint32, ctypes.c_int32]
    L.h2v_probe_set_option.restype = ctypes.c_int
    E_ARG = -1
    assert L.h2v_probe_set_option(9, 0) == E_ARG
    assert L.h2v_probe_set_option(10, 0) == E_ARG


def test_no_cpu_fallback_without_gpu():
    """Without a GPU the product path fails loudly instead of detouring through a CPU implementation."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from plutus_halo2_verifier_gen_amd import backend
    vk, td = V.simple_mul_vk()
    with pytest.raises(backend.H2VError):
        backend.DevicePlan(PL.compile_plan(vk).to_bytes(), 0)


def test_shard_ranges():
    for n in (0, 1, 7, 4096, 4097):
        for world in (1, 2, 3, 8):
            ranges = [shard.shard_range(n, r, world) for r in range(world)]
            assert ranges[0][0] == 0 and ranges[-1][1] == n
            assert all(ranges[i][1] == ranges[i + 1][0] for i in range(world - 1))


GLOO_WORKER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from plutus_halo2_verifier_gen_amd import plan as PL, shard, synth, vk as V
from oracle import binding as orc   # CPU test: the oracle stands in for the per-rank GPU call
dist.init_process_group(backend="gloo")
vk, td = V.simple_mul_vk()
pl = PL.compile_plan(vk)
b = synth.forge_batch(vk, td, 7, seed=4, plan=pl, workers=1)
b = synth.with_rejects(pl, b, 3, fraction=0.5, seed=2, kinds=["flip_first_scalar", "bad_point_flag"])
ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
def verify(proofs, off, inst, ci):
    return ov.verify_batch(proofs, off, inst, ci, threads=1)
out = shard.verify_sharded(verify, b.proofs, b.proof_off, b.instances, b.committed, 3)
if dist.get_rank() == 0:
    assert list(out) == b.expected, (list(out), b.expected)
    assert 0 < sum(out) < 7
    print("GLOO_OK", list(out))
else:
    assert out is None
dist.destroy_process_group()
'''


def test_sharded_verify_two_ranks_gloo(tmp_path):
    """world_size 2 over gloo: contiguous shards, no data-path collective, accept bytes gathered on rank 0."""
    script = tmp_path / "worker.py"
    script.write_text(GLOO_WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29531", str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "GLOO_OK" in res.stdout


def test_safegcd_model():
    """Integer model of csrc/h2v_modinv.hpp (tests/safegcd_model.py: 30 division steps per batch on the low words, transition
    matrix applied to (f, g) and, modulo M with exact division by 2^30, to (d, e)) with the constants the device header carries:
    every intermediate stays inside the 64-bit / 32-bit ranges the kernel code assumes (the model asserts them), the loop ends
    within the kernel's batch limit and the result is the modular inverse."""
    from tests import safegcd_model as S
    rng = random.Random(8)
    for mod, name, L in ((bls.P, "FP", 13), (bls.R, "FR", 9)):
        fld = S.field(name)
        mod30, minv30 = S.arr(name + "_MOD30"), S.const(name + "_MINV30")
        assert (fld.mod, fld.mod30, fld.minv30, fld.limbs) == (mod, mod30, minv30, L)
        assert len(mod30) == L and sum(t << (30 * i) for i, t in enumerate(mod30)) == mod
        assert minv30 * mod % (1 << 30) == 1
        worst = 0
        for x in [1, 2, 3, mod - 1, mod - 2, (mod - 1) // 2, 1 << (mod.bit_length() - 1)] + [rng.randrange(1, mod) for _ in range(150)]:
            inv, cls, _zeta = S.inverse(x, fld)
            assert inv * x % mod == 1
            worst = max(worst, cls[3])
        assert worst <= 32
    assert S.arr("FP_R3") == [(pow(2, 3 * bls.MONT_BITS_FP, bls.P) >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def test_plan_loader_rejects_mutated_blobs_without_a_gpu():
    """h2v_plan_load validates a blob completely on the host before any device work (an out-of-range register, offset or
    term index would become an out-of-bounds access inside a kernel).  Mutated blobs must come back as H2V_E_PLAN /
    H2V_E_LIMIT - or, when the mutation happens to leave a valid plan, as H2V_E_DEVICE on this GPU-less box - and never
    crash the process."""
    import struct
    from plutus_halo2_verifier_gen_amd import backend
    from tests.plan_loading import plan_loader
    load_plan = plan_loader()
    have_gpu = backend.device_count() >= 1
    E_ARG, E_PLAN, E_DEVICE, E_LIMIT = -1, -2, -3, -4

    def load(blob):
        return load_plan(blob)[0]

    rng = random.Random(11)
    for name in ("simple_mul", "ivc"):
        vk, _ = V.BUILDERS[name]()
        blob = PL.compile_plan(vk).to_bytes()
        ok_rc = 0 if have_gpu else E_DEVICE
        assert load(blob) == ok_rc
        hdr_words = PL.PLAN_HDR_WORDS
        w = list(struct.unpack_from("<%dI" % hdr_words, blob, 8))
        # every header word set to hostile values
        for k in range(hdr_words):
            for val in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF, w[k] + 1, w[k] + 16, max(0, w[k] - 1)):
                if val == w[k]:
                    continue
                m = bytearray(blob)
                struct.pack_into("<I", m, 8 + 4 * k, val & 0xFFFFFFFF)
                assert load(m) in (E_PLAN, E_LIMIT, ok_rc), (name, k, val)
        # instruction stream: every field of random instructions
        off_instr, n_instr = w[14], w[5]
        for _ in range(400):
            m = bytearray(blob)
            pos = off_instr + 8 * rng.randrange(n_instr) + rng.randrange(8)
            m[pos] = rng.randrange(256)
            assert load(m) in (E_PLAN, E_LIMIT, ok_rc)
        # term table and point offsets
        for sec_word, count_word, rec in ((18, 9, 8), (16, 7, 4), (21, 10, 8)):
            for _ in range(100):
                m = bytearray(blob)
                if w[count_word] == 0:
                    break
                pos = w[sec_word] + rec * rng.randrange(w[count_word]) + rng.randrange(rec)
                m[pos] = rng.randrange(256)
                assert load(m) in (E_PLAN, E_LIMIT, ok_rc)
        # truncations and garbage
        for cut in (0, 7, 8, 100, len(blob) // 2, len(blob) - 1):
            assert load(blob[:cut]) in (E_PLAN, E_ARG)
        assert load(bytes(rng.randrange(256) for _ in range(4096))) == E_PLAN


def test_generated_headers_are_current(tmp_path):
    """csrc/bls_consts.h, coop_tables.h, six_tables.h and coop_program.h are generated (and self-checked against big-integer
    arithmetic) by tools/gen_*.py; the committed copies must be what the generators produce today."""
    import shutil
    csrc = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
    names = {"gen_device_consts.py": "bls_consts.h", "gen_coop_tables.py": "coop_tables.h", "gen_coop_program.py": "coop_program.h",
             "gen_six_tables.py": "six_tables.h"}
    backup = {h: open(os.path.join(csrc, h)).read() for h in names.values()}
    stamps = {h: os.stat(os.path.join(csrc, h)) for h in names.values()}
    try:
        for script, header in names.items():
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", script)], stdout=subprocess.DEVNULL)
            assert open(os.path.join(csrc, header)).read() == backup[header], "%s is stale: run tools/%s" % (header, script)
    finally:
        for h, text in backup.items():
            with open(os.path.join(csrc, h), "w") as f:
                f.write(text)
            os.utime(os.path.join(csrc, h), ns=(stamps[h].st_atime_ns, stamps[h].st_mtime_ns))   # no spurious rebuild
    # the program generator also checks statically the value bounds the kernel's lazy field arithmetic relies on
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_coop_program
    assert gen_coop_program.check_bounds(gen_coop_program.build_program())


@pytest.mark.parametrize("name", ["simple_mul", "lookup_table", "sha256", "ivc"])
def test_scheduled_programs_are_equivalent(name):
    """The combiner program is list-scheduled into bundles of L records (plan.py: _schedule); every schedule of a plan -
    one lane per proof, the narrow one, the wide one - must compute the same MSM scalars and the same reject reason, on a
    valid proof and on corrupted ones, and respect the bundle discipline the device interpreter relies on."""
    vk, td = V.BUILDERS[name]()
    pl = PL.compile_plan(vk)
    pl1 = PL.compile_plan(vk, lanes=1)
    assert pl1.vm_lanes == 1 and pl1.wide is None
    assert pl.vm_lanes in PL.VM_LANE_CHOICES and pl.n_regs * 32 * (64 // pl.vm_lanes) <= PL.VM_LDS_BYTES
    PL.check_bundles(pl.instrs, pl.vm_lanes)
    assert pl.wide is not None and pl.wide[0] > pl.vm_lanes
    PL.check_bundles(pl.wide[2], pl.wide[0])
    assert pl.wide[1] * 32 * (64 // pl.wide[0]) <= PL.VM_LDS_BYTES
    # same multiset of real instructions in every schedule
    def ops(instrs):
        return sorted(op for op, *_ in instrs if op not in (PL.OP_NOP, PL.OP_END))
    assert ops(pl.instrs) == ops(pl.wide[2]) == ops(pl1.instrs)
    b = synth.forge_batch(vk, td, 3, seed=21, plan=pl, workers=1)
    b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.7, seed=5, kinds=["flip_first_scalar", "noncanonical_scalar", "wrong_pi"])
    for i in range(3):
        inst = b.instance_ints(i, vk.n_public_inputs)
        ci = b.committed[48 * i:48 * i + 48] if b.committed else None
        ref = PL.run_plan(pl1, b.proof(i), inst, ci)
        for got in (PL.run_plan(pl, b.proof(i), inst, ci), PL.run_plan(pl, b.proof(i), inst, ci, use_wide=True)):
            assert got[0] == ref[0] and got[2] == ref[2]


def test_plan_loader_rejects_broken_bundles():
    """A bundle whose records depend on each other, or a transcript operation that is not alone on lane 0, must be refused
    by h2v_plan_load on the host (the interpreter's lanes run the records of a bundle in no particular order)."""
    import struct
    from tests.plan_loading import plan_loader
    load = plan_loader()

    vk, _ = V.BUILDERS["simple_mul"]()
    pl = PL.compile_plan(vk)
    lanes = pl.vm_lanes
    assert lanes >= 2
    blob = pl.to_bytes()
    off_instr = struct.unpack_from("<I", blob, 8 + 4 * 14)[0]
    recs = pl.instrs
    # a bundle with two arithmetic records
    k = next(s for s in range(0, len(recs), lanes) if recs[s][0] == PL.OP_MUL and recs[s + 1][0] in (PL.OP_MUL, PL.OP_ADD, PL.OP_SUB))
    op0, d0, a0, b0 = recs[k]
    op1, d1, a1, b1 = recs[k + 1]
    m = bytearray(blob)
    struct.pack_into("<BBHHH", m, off_instr + 8 * (k + 1), op1, 0, d1, d0, b1)       # lane 1 reads what lane 0 writes
    rc, msg = load(m)
    assert rc == -2 and "reads a register it writes" in msg
    m = bytearray(blob)
    struct.pack_into("<BBHHH", m, off_instr + 8 * (k + 1), op1, 0, d0, a1, b1)       # both lanes write one register
    rc, msg = load(m)
    assert rc == -2 and "write one register" in msg
    # a transcript operation on lane 1 / sharing its bundle
    t = next(s for s in range(0, len(recs), lanes) if recs[s][0] == PL.OP_SQUEEZE)
    m = bytearray(blob)
    struct.pack_into("<BBHHH", m, off_instr + 8 * (t + 1), PL.OP_CONST, 0, 0, 0, 0)
    rc, msg = load(m)
    assert rc == -2 and "shares its bundle" in msg
    m = bytearray(blob)
    struct.pack_into("<BBHHH", m, off_instr + 8 * (k + 1), PL.OP_SQUEEZE, 0, d1, 0, 0)
    rc, msg = load(m)
    assert rc == -2 and "off lane 0" in msg
    # lane count that does not divide the stream / is not a power of two
    for bad in (3, 0, 64):
        m = bytearray(blob)
        struct.pack_into("<I", m, 8 + 4 * 35, bad)
        assert load(m)[0] == -2


def test_bucket_msm_recoding_model():
    """The scalar recoding of the bucket MSM (csrc/h2v_pippenger.hpp: k_pip_digits) restated on integers: GLV split into two
    halves below 2^128, then signed c-bit digits in [-2^(c-1), 2^(c-1)] over W = 128 // c + 1 windows.  For every window
    width the launcher can pick (7..10) the digits reconstruct the half exactly, stay in range, and no carry leaves the top
    window - the property that lets the kernel address 2^(c-1) buckets per window without an overflow bucket."""
    rng = random.Random(77)
    lam = bls.GLV_LAMBDA
    edge = [0, 1, bls.R - 1, lam, lam - 1, lam + 1, (1 << 128) - 1, 1 << 128, (1 << 255) % bls.R, bls.R - lam, bls.R // 2]
    scalars = edge + [rng.randrange(bls.R) for _ in range(300)]
    for k in scalars:
        k1, k2 = bls.glv_split(k)
        assert 0 <= k1 < (1 << 128) and 0 <= k2 < (1 << 128) and (k1 + k2 * lam - k) % bls.R == 0
        for c in (7, 8, 9, 10):
            W, NB = 128 // c + 1, 1 << (c - 1)
            for half in (k1, k2, (1 << 128) - 1):          # (any value below 2^128 must recode: the left-hand scalars r_i)
                carry, digits = 0, []
                for w in range(W):
                    raw = ((half >> (w * c)) & ((1 << c) - 1)) + carry
                    if raw > NB:
                        d, carry = raw - (1 << c), 1
                    else:
                        d, carry = raw, 0
                    digits.append(d)
                assert carry == 0
                assert all(-NB <= d <= NB for d in digits)
                assert sum(d << (w * c) for w, d in enumerate(digits)) == half


def test_bucket_msm_lane_estimate_covers_the_size_classes():
    """Integer model of the bucket MSM's size classes (csrc/h2v_pippenger.hpp: k_pip_scan) against the host's grid estimate
    (csrc/h2v_capi.hip: pip_launch): a bucket of more than T 2^(k-1) entries gets 2^k lanes (k <= 8), every class is padded
    to whole 256-lane blocks, and the launch has 2 n halves W / T + nb + 256 x 9 lanes.  Round 2's histogram stopped at
    2047 entries, so for T = 20 the 256-lane class began at 2047 instead of 2560 and the estimate fell short for
    530-625 k terms; with the histogram at 4096 it holds up to the API's limit (and the kernel now walks every logical
    block whatever the grid is)."""
    import math
    T, HIST = 20, 4096

    def shape(n, halves):
        c = 10
        while c > 4 and n * halves / (1 << (c - 1)) < 24.0:
            c -= 1
        return c, 1 << (c - 1), 128 // c + 1

    def lanes_used(counts, hist_cap):
        used = 0
        for k in range(8, -1, -1):
            low = 0 if k == 0 else T << (k - 1)
            low_eff = min(low, hist_cap - 2) if low >= hist_cap - 1 else low
            high = None if k == 8 else min(T << k, hist_cap - 2) if (T << k) >= hist_cap - 1 else (T << k)
            members = sum(1 for cv in counts if cv > low_eff and (high is None or cv <= high))
            used += ((members << k) + 255) & ~255
        return used

    rng = random.Random(5)
    for n in (1000, 40966, 300000, 560000, 600000, 1 << 20, 3_000_000):
        for halves in (1, 2):
            c, NB, W = shape(n, halves)
            entries = n * halves
            counts = []
            for w in range(W):
                bits = min(c, 128 - w * c) if w * c < 128 else 0
                live = NB if bits >= c else max(1, 1 << max(bits - 1, 0))      # the top window holds 128 mod c bits
                mean = entries * (1 - 2.0 ** -bits if bits else 0) / live
                for b in range(NB):
                    counts.append(max(0, int(rng.gauss(mean, math.sqrt(mean) + 1))) if b < live else 0)
            estimate = 2 * entries * W // T + W * NB + 256 * 9
            estimate = (estimate + 255) // 256 * 256
            assert lanes_used(counts, HIST) <= estimate, (n, halves)
            if n in (560000, 600000) and halves == 2:
                assert lanes_used(counts, 2048) > estimate       # the round-2 clamp: short by a few hundred blocks
