"""H2V_MIXED_GROUPED (include/h2v.h: phase 1 of every groupable key of a mixed call in one launch per kernel, up to 1024 keys),
what can be said without a GPU: the group tables as a stand-alone sanitized program against a brute-force enumeration, the
agreement of header, binding, Python API and C++ wrapper on the new constants, and the flag rules and limits that are decided
before a device is touched.  No plan or workspace exists without a device, so what lies behind the argument rules is
H2V_E_DEVICE in every layer.  GPU legs: tests/test_mixed_grouped_gpu.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from tests.test_mixed_keys import PKG, ROOT, be  # noqa: F401  (module fixture)

E_ARG, E_DEVICE, E_LIMIT = -1, -3, -4


def _header(name="h2v.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_group_table_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_group.cpp: host code only, its own main, built with ASan + UBSan and run as a program - every grouped
    position in exactly one block of exactly one group in each prefix array, no decompression unit across two groups, ranges that
    start and end inside a plan / hold one proof / skip plans without proofs, 1024 plans of one proof each, and the block
    ownership of the VK-base sums equal to fold_layout's for ranges that are whole plans"""
    out = str(tmp_path / "h2v_mixed_group")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_group.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout
    assert r.stderr == ""


def test_layout_header_has_no_hip_in_it():
    with open(os.path.join(PKG, "csrc", "h2v_mixed_group.hpp")) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()


def test_constants_agree_in_header_binding_and_wrapper(be):
    h, hpp = _header(), _header("h2v.hpp")
    for name, value, bound in (("H2V_MIXED_GROUPED", 4, be.MIXED_GROUPED), ("H2V_MIXED_GROUPED_MAX_PLANS", 1024, be.MIXED_GROUPED_MAX_PLANS),
                               ("H2V_MIXED_GROUPED_MAX_OTHER", 62, be.MIXED_GROUPED_MAX_OTHER), ("H2V_RLC_GROUPED", 16, be.RLC_GROUPED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, h).group(1)) == value == bound, name
    assert be.MIXED_GROUPED & (be.MIXED_RLC | be.MIXED_FOLD_MSM) == 0
    assert be.RLC_GROUPED & (be.RLC_SEED_GIVEN | be.RLC_ONE_STREAM | be.RLC_FOLD_PAIRS) == 0
    assert be.MIXED_MAX_PLANS == 64                                   # the limit of every call without the flag stays
    assert "H2V_MIXED_GROUPED" in hpp and "H2V_RLC_GROUPED" in hpp
    # the header states the contract: records, limits, the fall-back in slices, the options that do not apply
    for phrase in ("RECORDS: the grouped part takes ONE record", "H2V_MIXED_GROUPED_MAX_OTHER", "slices of at most 62 plans",
                   "H2V_OPT_COMBINER_PROOFS_PER_BLOCK shape per-plan launches and do not apply"):
        assert phrase in h, phrase
    from plutus_halo2_verifier_gen_amd import api
    for f in (api.verify_mixed, api.batch_verify, api.Aggregator.__init__, be.verify_mixed, be.verify_mixed_device, be.aggregate_mixed,
              be.aggregate_mixed_device):
        assert inspect.signature(f).parameters["grouped"].default is False, f


def test_flag_rules_that_need_no_device(be):
    L = be.lib()
    acc = (C.c_uint8 * 4)()
    b = be.MixedBatch(0, None, None, None, None, None)
    many = (C.c_void_p * (be.MIXED_GROUPED_MAX_PLANS + 1))()
    full = be.MIXED_RLC | be.MIXED_FOLD_MSM | be.MIXED_GROUPED
    # the flag without both others: H2V_E_ARG in both forms, in the wording of the FOLD_MSM rule
    for flags in (be.MIXED_GROUPED | be.MIXED_FOLD_MSM, be.MIXED_GROUPED, be.MIXED_GROUPED | be.MIXED_RLC):
        assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, flags, None, None) == E_ARG
        assert "is valid only together with H2V_MIXED_RLC" in L.h2v_last_error().decode()
        assert L.h2v_verify_mixed_device(many, 1, C.byref(b), acc, None, None, None, flags, None) == E_ARG
    assert "H2V_MIXED_GROUPED is valid only together with H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM" in L.h2v_last_error().decode()
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, full | 8, None, None) == E_ARG          # an unknown flag beside it
    # the limits: 1024 plans listed is fine (n = 0: H2V_OK), 1025 is H2V_E_LIMIT - before anything looks at a plan or a device;
    # without the flag 65 stays H2V_E_LIMIT
    assert L.h2v_verify_mixed(many, be.MIXED_GROUPED_MAX_PLANS, C.byref(b), acc, None, None, full, None, None) == 0
    assert L.h2v_verify_mixed_device(many, be.MIXED_GROUPED_MAX_PLANS, C.byref(b), acc, None, None, None, full, None) == 0
    assert L.h2v_verify_mixed(many, be.MIXED_GROUPED_MAX_PLANS + 1, C.byref(b), acc, None, None, full, None, None) == E_LIMIT
    assert "1024" in L.h2v_last_error().decode()
    assert L.h2v_verify_mixed_device(many, be.MIXED_GROUPED_MAX_PLANS + 1, C.byref(b), acc, None, None, None, full, None) == E_LIMIT
    assert L.h2v_verify_mixed(many, be.MIXED_MAX_PLANS + 1, C.byref(b), acc, None, None, be.MIXED_RLC | be.MIXED_FOLD_MSM, None, None) == E_LIMIT
    one = be.MixedBatch(1, None, None, None, None, None)
    assert L.h2v_verify_mixed(many, be.MIXED_GROUPED_MAX_PLANS + 1, C.byref(one), acc, None, None, full, None, None) == E_LIMIT   # (n > 0: still the limit first)
    # the aggregate side: H2V_RLC_GROUPED is known to the mixed forms alone
    pair = C.create_string_buffer(96)
    grouped = be.RlcOpts((C.c_uint8 * 32)(), be.RLC_GROUPED)
    assert L.h2v_aggregate_mixed(many, be.MIXED_GROUPED_MAX_PLANS, C.byref(b), pair, acc, None, None, C.byref(grouped), None) == 0
    assert pair.raw == (b"\xc0" + bytes(47)) * 2
    assert L.h2v_aggregate_mixed(many, be.MIXED_GROUPED_MAX_PLANS + 1, C.byref(b), pair, acc, None, None, C.byref(grouped), None) == E_LIMIT
    assert L.h2v_aggregate_mixed(many, be.MIXED_MAX_PLANS + 1, C.byref(b), pair, acc, None, None, None, None) == E_LIMIT
    sb = be.Batch(0, None, None, None, None)
    assert L.h2v_aggregate_batch(many, C.byref(sb), pair, acc, None, None, C.byref(grouped), None) == E_ARG       # any other call: unknown
    assert "unknown flag" in L.h2v_last_error().decode()
    assert L.h2v_aggregate_batch_device(many, C.byref(sb), C.addressof(pair), C.addressof(acc), None, None, None, C.byref(grouped), None) == E_ARG
    # the Python surfaces: grouped without fold_msm reaches the library and comes back as H2V_E_ARG; api refuses it before any call
    with pytest.raises(be.H2VError, match="H2V_MIXED_GROUPED is valid only together"):
        be.verify_mixed([], [], b"", [0], None, None, mode="rlc", grouped=True)
    with pytest.raises(be.H2VError, match="H2V_MIXED_GROUPED is valid only together"):
        be.verify_mixed_device([], [], 0, None, None, None, None, C.addressof(acc), mode="rlc", grouped=True)
    assert be.verify_mixed([], [], b"", [0], None, None, mode="rlc", fold_msm=True, grouped=True) == (b"", [], False)
    assert be.aggregate_mixed([], [], b"", [0], None, None, grouped=True)[0] == (b"\xc0" + bytes(47)) * 2
    from plutus_halo2_verifier_gen_amd import api
    with pytest.raises(ValueError, match="grouped"):
        api.verify_mixed([], [], [], mode="rlc", grouped=True)
    assert api.verify_mixed([], [], [], mode="rlc", fold_msm=True, grouped=True) == []


def test_no_device_is_an_error_in_every_layer(be, tmp_path):
    """without a GPU nothing loads a plan: the Python layers raise H2V_E_DEVICE from the key's upload, and the C++ wrapper's driver
    ends with error -3 - never a detour around the device"""
    if be.device_count() >= 1:
        return                  # (a machine with a GPU: tests/test_mixed_grouped_gpu.py drives the same layers to their results)
    from plutus_halo2_verifier_gen_amd import api, plan as PL, synth, vk as V
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    with pytest.raises(be.H2VError) as e:
        be.DevicePlan(pl.to_bytes(), 0)
    assert "h2v error %d" % E_DEVICE in str(e.value)
    batch = synth.forge_batch(vk, td, 2, seed=3, plan=pl, workers=1)
    proofs = [batch.proof(i) for i in range(2)]
    inst = [batch.instance_ints(i, vk.n_public_inputs) for i in range(2)]
    with pytest.raises(be.H2VError) as e:
        api.verify_mixed([vk, vk], proofs, inst, mode="rlc", fold_msm=True, grouped=True)
    assert "h2v error %d" % E_DEVICE in str(e.value)
    with pytest.raises(be.H2VError) as e:
        api.Aggregator(api.ParamsVerifierKZG(bytes.fromhex(vk.s_g2)), grouped=True).push_mixed([vk, vk], proofs, inst)
    assert "h2v error %d" % E_DEVICE in str(e.value)
    out = str(tmp_path / "h2v_mixed_grouped_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_grouped_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    key = str(tmp_path / "simple_mul.bin")
    with open(key, "wb") as f:
        f.write(pl.to_bytes())
    with open(str(tmp_path / "plans.txt"), "w") as f:
        f.write(key + "\n")
    with open(str(tmp_path / "empty.bin"), "wb") as f:
        f.write(bytes(4))
    r = subprocess.run([out, str(tmp_path / "plans.txt"), str(tmp_path / "empty.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout.startswith("error -3 "), r.stdout + r.stderr
