"""The fold form of mixed-key batches (include/h2v.h: H2V_MIXED_FOLD_MSM - one bucket MSM and one pairing for a call over several
keys), what can be said without a GPU: the layout of the call's term pool as a stand-alone sanitized program, the argument
errors that are decided before a device is touched, and the agreement of header, binding, Python API and C++ wrapper on the
flag and on the test probe."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from tests.test_mixed_keys import PKG, ROOT, be  # noqa: F401  (module fixture)


def test_term_layout_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_terms.cpp: host code only, its own main, built with ASan + UBSan and run as a program - counts
    70 / 65 / 9 / 1 / 0, chunk sizes 40, 64 and 4096 (and one piece), an all-non-foldable call, a single-proof call: term ranges
    disjoint and covering [0, N_R), block ranges disjoint, N_R by the header's formula, the limit exactly 2^22"""
    out = str(tmp_path / "h2v_mixed_terms")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_terms.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
    assert r.stderr == ""


def test_layout_header_has_no_hip_in_it():
    with open(os.path.join(PKG, "csrc", "h2v_mixed_fold.hpp")) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()


def test_flag_and_probe_are_declared_and_bound(be):
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        header = f.read()
    assert re.search(r"#define H2V_MIXED_FOLD_MSM (\d+)u", header).group(1) == str(be.MIXED_FOLD_MSM) == "2"
    assert be.MIXED_FOLD_MSM & be.MIXED_RLC == 0
    assert "h2v_probe_mixed_fold_sums" in be.EXPORTS
    assert re.search(r"\bint h2v_probe_mixed_fold_sums\(h2v_workspace \*ws, uint8_t out_xy_be\[192\]\)", header)
    getattr(be.lib(), "h2v_probe_mixed_fold_sums")
    # the header states the term count, its limit, the fall-back and the synchronisation of the device form
    for phrase in ("TERM COUNT", "N_R > 2^22 is H2V_E_LIMIT", "FALL-BACK", "return only after the batch verdict is known"):
        assert phrase in header, phrase
    with open(os.path.join(ROOT, "include", "h2v.hpp")) as f:
        assert "H2V_MIXED_FOLD_MSM" in f.read()


def test_argument_errors_that_need_no_device(be):
    L = be.lib()
    acc = (C.c_uint8 * 4)()
    b = be.MixedBatch(0, None, None, None, None, None)
    many = (C.c_void_p * 2)()
    # the flag alone is H2V_E_ARG in both forms, whatever n is; with H2V_MIXED_RLC an empty call is H2V_OK
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, be.MIXED_FOLD_MSM, None, None) == -1
    assert "H2V_MIXED_RLC" in L.h2v_last_error().decode()
    assert L.h2v_verify_mixed_device(many, 1, C.byref(b), acc, None, None, None, be.MIXED_FOLD_MSM, None) == -1
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, be.MIXED_FOLD_MSM | be.MIXED_RLC, None, None) == 0
    assert L.h2v_verify_mixed_device(many, 1, C.byref(b), acc, None, None, None, be.MIXED_FOLD_MSM | be.MIXED_RLC, None) == 0
    assert L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, 4, None, None) == -1           # an unknown flag
    assert L.h2v_probe_mixed_fold_sums(None, None) == -1
    # the Python surface refuses the combination before any call
    with pytest.raises(ValueError, match="fold_msm"):
        be.verify_mixed([], [], b"", [0], None, None, mode="per-proof", fold_msm=True)
    with pytest.raises(ValueError, match="fold_msm"):
        be.verify_mixed_device([], [], 0, None, None, None, None, None, mode="per-proof", fold_msm=True)
    from plutus_halo2_verifier_gen_amd import api
    with pytest.raises(ValueError, match="fold_msm"):
        api.verify_mixed([], [], [], mode="per-proof", fold_msm=True)
    for f in (api.verify_mixed, api.batch_verify, be.verify_mixed, be.verify_mixed_device):
        assert inspect.signature(f).parameters["fold_msm"].default is False, f


def test_cpp_driver_builds_against_the_header(be, tmp_path):
    out = str(tmp_path / "h2v_mixed_fold_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_fold_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.access(out, os.X_OK)
