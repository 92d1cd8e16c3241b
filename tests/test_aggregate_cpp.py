"""h2v::aggregate_batch and h2v::Aggregator (include/h2v.hpp) through tests/cpp/h2v_aggregate_driver.cpp, built the way
tests/test_cpp_host.py builds its driver.  CPU leg: it compiles against the header with -Wall -Werror, links against the C-ABI
library and fails loudly with H2V_E_DEVICE without a GPU.  GPU leg: three pushes of two keys of one SRS against the oracle."""
import json
import os
import random
import struct
import subprocess

import pytest

from tests.test_cpp_host import _gpu_present, _write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build_hip()
    out = str(tmp_path_factory.mktemp("cpp") / "h2v_aggregate_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_aggregate_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_driver_builds_against_the_header(driver):
    assert os.access(driver, os.X_OK)


def test_driver_fails_loudly_without_gpu(driver, tmp_path):
    if _gpu_present():
        pytest.skip("a GPU is present: covered by the gpu leg")
    plan, batch, _ = _write_case(tmp_path, n=2, corrupt=())
    r = subprocess.run([driver, plan, batch], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stdout + r.stderr
    assert r.stdout.startswith("error -3 ")          # H2V_E_DEVICE: no CPU fallback


def three_pushes():
    """The three calls of the end-to-end test (tests/test_aggregate_gpu.py runs the same through api.Aggregator): (key name, batch)
    x 3 - 70 simple_mul proofs with one noncanonical_scalar reject (excluded before the pairing: its call's pair still passes), 5
    lookup_table proofs with one wrong_pi (included, and it fails its call's pair), 1 simple_mul proof."""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    from tests.test_mixed_keys import COMMON_S
    out = []
    for name, n, seed, (bad, kind) in (("simple_mul", 70, 81, (33, "noncanonical_scalar")), ("lookup_table", 5, 82, (2, "wrong_pi")),
                                       ("simple_mul", 1, 83, (None, None))):
        vk, td = V.on_srs(*V.BUILDERS[name](), COMMON_S)      # two keys of ONE SRS
        pl = PL.compile_plan(vk)
        b = synth.forge_batch(vk, td, n, seed=seed, plan=pl, workers=4)
        n_pi = vk.n_public_inputs
        proofs = [b.proof(i) for i in range(n)]
        insts = [b.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in range(n)]
        expected = [1] * n
        if bad is not None:
            proofs[bad], insts[bad] = synth.corrupt(pl, proofs[bad], insts[bad], kind, random.Random(seed))
            expected[bad] = 0
        off = [0]
        for p in proofs:
            off.append(off[-1] + len(p))
        out.append((name, vk, pl, synth.Batch(n=n, proofs=b"".join(proofs), proof_off=off, instances=b"".join(insts), committed=b.committed,
                                              expected=expected)))
    return out


@pytest.mark.gpu
def test_cpp_aggregator_three_pushes(driver, tmp_path, orc):
    args, want = [], []
    for k, (name, vk, pl, b) in enumerate(three_pushes()):
        n_pi = vk.n_public_inputs
        assert b.committed is None
        blob = struct.pack("<III", b.n, n_pi, 0)
        for i in range(b.n):
            blob += struct.pack("<I", len(b.proof(i))) + b.proof(i) + b.instances[32 * n_pi * i:32 * n_pi * (i + 1)]
        (tmp_path / ("%s.plan" % name)).write_bytes(pl.to_bytes())
        (tmp_path / ("batch%d.bin" % k)).write_bytes(blob)
        args += [str(tmp_path / ("%s.plan" % name)), str(tmp_path / ("batch%d.bin" % k))]
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        verdicts = list(ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4))
        assert verdicts == b.expected
        want.append("".join(str(v) for v in verdicts))
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    (tmp_path / "foreign.plan").write_bytes(PL.compile_plan(V.simple_mul_vk()[0]).to_bytes())      # simple_mul on its OWN SRS
    r = subprocess.run([driver] + args + [str(tmp_path / "foreign.plan")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split(" ") for l in r.stdout.strip().splitlines()]
    assert [l[1] for l in lines if l[0] == "foreign_refused"] == ["1"]      # as api.Aggregator: a key of another SRS is refused
    calls = {int(l[1]): l[2] for l in lines if l[0] == "call"}
    assert [calls[k] for k in range(3)] == want
    assert [l[1] for l in lines if l[0] == "reverified"] == ["1"]
    pair_ok = {int(l[1]): l[2] for l in lines if l[0] == "pair_ok"}
    assert pair_ok == {0: "1", 1: "0", 2: "1"}
    included = {int(l[1]): l[2] for l in lines if l[0] == "included"}
    assert included[0] == want[0] and included[1] == "11111" and included[2] == "1"      # wrong_pi is included: only the pair refuses it
