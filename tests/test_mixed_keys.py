"""Mixed-key batches (include/h2v.h: h2v_verify_mixed), what can be said without a GPU: the host side of the partition as a
stand-alone sanitized program, the agreement of header, binding and C++ wrapper on the two new exports, and the built-in keys
moved to one common SRS (vk.on_srs) - the fixtures of tests/test_mixed_keys_gpu.py - against the CPU oracle."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd")
NEW = ("h2v_verify_mixed", "h2v_verify_mixed_device")
MIXED_KEYS = ("simple_mul", "lookup_table", "trashcan_mix", "ivc")
COMMON_S = 0x6d697865645f6b6579735f6f6e655f535253      # the common SRS secret of the mixed-key fixtures


@pytest.fixture(scope="module")
def be():
    import __graft_entry__ as ge
    ge.build_hip()
    from plutus_halo2_verifier_gen_amd import backend
    return backend


def test_partition_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_partition.cpp: host code only, its own main, built with ASan + UBSan and run as a program - the
    permutation is stable, instance / committed offsets are right for the (3, 0), (1, 0), (5, 1), (28, 0) shapes, a listed key
    without a proof, n = 0, n = 1, H2V_MIXED_MAX_PLANS keys of one proof each, and an out-of-range plan_of is refused"""
    out = str(tmp_path / "h2v_mixed_partition")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_partition.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
    assert r.stderr == ""


def test_partition_header_has_no_hip_in_it():
    with open(os.path.join(PKG, "csrc", "h2v_mixed.hpp")) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()


def test_exports_are_declared_and_bound(be):
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in be.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
        getattr(be.lib(), name)
    assert re.search(r"#define H2V_MIXED_MAX_PLANS (\d+)u", header).group(1) == str(be.MIXED_MAX_PLANS)
    assert be.MIXED_MAX_PLANS >= 64
    assert re.search(r"#define H2V_MIXED_RLC (\d+)u", header).group(1) == str(be.MIXED_RLC)


def test_cpp_driver_builds_against_the_header(be, tmp_path):
    out = str(tmp_path / "h2v_mixed_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.access(out, os.X_OK)


def test_argument_errors_that_need_no_device(be):
    """checked before anything touches a device: null arguments, and more plans than H2V_MIXED_MAX_PLANS (a stand-in plan
    list is never dereferenced before its length has been checked)"""
    L = be.lib()
    acc = (C.c_uint8 * 4)()
    b = be.MixedBatch(0, None, None, None, None, None)
    many = (C.c_void_p * (be.MIXED_MAX_PLANS + 1))()
    assert L.h2v_verify_mixed(None, 0, C.byref(b), acc, None, None, 0, None, None) == -1
    assert L.h2v_verify_mixed(many, 1, None, acc, None, None, 0, None, None) == -1
    assert L.h2v_verify_mixed(many, 1, C.byref(b), None, None, None, 0, None, None) == -1
    assert L.h2v_verify_mixed(many, be.MIXED_MAX_PLANS + 1, C.byref(b), acc, None, None, 0, None, None) == -4
    assert str(be.MIXED_MAX_PLANS) in L.h2v_last_error().decode()
    assert L.h2v_verify_mixed_device(many, be.MIXED_MAX_PLANS + 1, C.byref(b), acc, None, None, None, 0, None) == -4
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, 2, None, None) == -1           # an unknown flag
    fb = C.c_int(7)
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, 0, None, C.byref(fb)) == 0    # n = 0
    assert fb.value == 0


@pytest.mark.parametrize("name", MIXED_KEYS)
def test_keys_on_a_common_srs(orc, name):
    """vk.on_srs: three forged proofs are accepted by the oracle under the moved key and rejected under the key's own SRS"""
    vk, td = V.BUILDERS[name]()
    vk2, td2 = V.on_srs(vk, td, COMMON_S)
    assert td2.s == COMMON_S and vk2.s_g2 != vk.s_g2
    assert (td2.fixed_dlogs, td2.perm_dlogs, td2.rec_dlogs) == (td.fixed_dlogs, td.perm_dlogs, td.rec_dlogs)
    moved = json.loads(vk2.to_json())
    own = json.loads(vk.to_json())
    assert {k for k in own if own[k] != moved[k]} == {"s_g2"}
    b = synth.forge_batch(vk2, td2, 3, seed=31, workers=1)
    ov2 = orc.OracleVK(orc.vk_desc(moved, vk2.omega, vk2.omega_inv, vk2.barycentric_weight))
    ov = orc.OracleVK(orc.vk_desc(own, vk.omega, vk.omega_inv, vk.barycentric_weight))
    assert list(ov2.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == [1, 1, 1]
    assert list(ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=2)) == [0, 0, 0]


def test_on_srs_refuses_a_zero_secret():
    vk, td = V.simple_mul_vk()
    with pytest.raises(ValueError):
        V.on_srs(vk, td, 0)
    from plutus_halo2_verifier_gen_amd import bls12_381 as bls
    with pytest.raises(ValueError):
        V.on_srs(vk, td, bls.R)


def test_plan_digests_of_the_built_in_keys_are_unchanged():
    with open(os.path.join(ROOT, "tests", "golden", "plan_digests.json")) as f:
        gold = json.load(f)
    for name, build in V.BUILDERS.items():
        vk, _ = build()
        assert hashlib.sha256(PL.compile_plan(vk).to_bytes()).hexdigest() == gold["BUILDERS"][name], name
