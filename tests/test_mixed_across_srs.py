"""Mixed-key calls across several SRS (include/h2v.h: H2V_MIXED_ACROSS_SRS - one call and ONE multi-pairing for proofs whose keys
sit on several SRS), what can be said without a GPU: header, binding and C++ wrapper agree on the flag and the probe; the flag
rules that are decided before a device is touched; the Python API's own refusals; the SRS classes as a stand-alone sanitized
program; and the class-major position rule of tests/mixed_across_model.py.  GPU legs: tests/test_mixed_across_srs_gpu.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls
from tests import mixed_across_model as AM
from tests.test_mixed_keys import PKG, ROOT, be  # noqa: F401  (module fixture)

E_ARG = -1


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flag_and_probe_agree_in_header_binding_and_wrapper(be):
    h, hpp = _text("include", "h2v.h"), _text("include", "h2v.hpp")
    assert re.search(r"#define H2V_MIXED_ACROSS_SRS (\d+)u", h).group(1) == str(be.MIXED_ACROSS_SRS) == "16"
    assert be.MIXED_ACROSS_SRS & (be.MIXED_RLC | be.MIXED_FOLD_MSM | be.MIXED_GROUPED | 8) == 0      # bit 8 stays unassigned
    assert "h2v_probe_mixed_fold_sums_multi" in be.EXPORTS
    assert re.search(r"\bint h2v_probe_mixed_fold_sums_multi\(h2v_workspace \*ws, uint32_t cap, uint8_t \*out_xy_be[^,]*, uint32_t \*n_classes\)", h)
    getattr(be.lib(), "h2v_probe_mixed_fold_sums_multi")
    assert re.search(r"\bint h2v_probe_mixed_fold_sums\(h2v_workspace \*ws, uint8_t out_xy_be\[192\]\)", h)      # unchanged
    assert "H2V_MIXED_ACROSS_SRS" in hpp
    assert len(re.findall(r"bool across_srs = false\) \{", hpp)) == 2                                # verify_mixed and batch_verify, trailing
    for phrase in ("SRS CLASSES", "ARGUMENT RULES", "CLASS-MAJOR position", "more than H2V_MULTI_SRS_MAX classes WITH proofs is H2V_E_LIMIT",
                   "does not count against the limit", "one pair cannot span SRS"):
        assert phrase in h, phrase
    for f in (be.verify_mixed, be.verify_mixed_device):
        assert inspect.signature(f).parameters["across_srs"].default is False, f
    assert list(inspect.signature(be.probe_mixed_fold_sums_multi).parameters)[0] == "ws"
    # the new HIP lives in a file of its own, the host side in a header without HIP
    dev = _text("plutus_halo2_verifier_gen_amd", "csrc", "h2v_mixed_srs_dev.hpp")
    for k in ("k_across_lterms", "k_across_coeff", "k_across_gather", "k_across_scatter"):
        assert k in dev, k
    host = _text("plutus_halo2_verifier_gen_amd", "csrc", "h2v_mixed_srs.hpp")
    assert "hip" not in "\n".join(line.split("//")[0] for line in host.splitlines()).lower()


def test_flag_rules_that_need_no_device(be):
    L = be.lib()
    acc = (C.c_uint8 * 4)()
    b = be.MixedBatch(0, None, None, None, None, None)
    many = (C.c_void_p * 2)()
    A, RLC = be.MIXED_ACROSS_SRS, be.MIXED_RLC
    host = lambda flags: L.h2v_verify_mixed(many, 1, C.byref(b), acc, None, None, flags, None, None)
    dev = lambda flags: L.h2v_verify_mixed_device(many, 1, C.byref(b), acc, None, None, None, flags, None)
    for call in (host, dev):
        assert call(A | RLC) == 0                                   # n = 0 is H2V_OK
        assert call(A | RLC | be.MIXED_FOLD_MSM) == 0
        assert call(A | RLC | be.MIXED_FOLD_MSM | be.MIXED_GROUPED) == 0
        assert call(A) == E_ARG
        assert L.h2v_last_error().decode() == "H2V_MIXED_ACROSS_SRS is valid only together with H2V_MIXED_RLC"
        assert call(A | RLC | 8) == E_ARG and "unknown flag" in L.h2v_last_error().decode()
        assert call(A | be.MIXED_FOLD_MSM) == E_ARG and "H2V_MIXED_FOLD_MSM" in L.h2v_last_error().decode()      # the older rule first
        assert call(32 | RLC) == E_ARG and "unknown flag" in L.h2v_last_error().decode()
    nc = C.c_uint32(0)
    assert L.h2v_probe_mixed_fold_sums_multi(None, 16, None, C.byref(nc)) == E_ARG
    # the binding refuses the flag without the batch-accept mode before any call
    with pytest.raises(ValueError, match="across_srs"):
        be.verify_mixed([], [], b"", [0], None, None, mode="per-proof", across_srs=True)
    with pytest.raises(ValueError, match="across_srs"):
        be.verify_mixed_device([], [], 0, None, None, None, None, None, mode="per-proof", across_srs=True)
    assert be.verify_mixed([], [], b"", [0], None, None, mode="rlc", across_srs=True) == (b"", [], False)


def test_api_refuses_one_call_without_its_form():
    from plutus_halo2_verifier_gen_amd import api
    for f in (api.verify_mixed, api.batch_verify):
        assert inspect.signature(f).parameters["one_call"].default is False, f
    with pytest.raises(ValueError, match="one_call"):
        api.verify_mixed([], [], [], mode="rlc", one_call=True)                      # without across_srs
    with pytest.raises(ValueError, match="one_call"):
        api.verify_mixed([], [], [], one_call=True)
    with pytest.raises(ValueError):
        api.verify_mixed([], [], [], mode="per-proof", across_srs=True, one_call=True)      # without mode="rlc"
    params = api.ParamsVerifierKZG(bls.g2_compress(bls.g2_mul(bls.G2_GEN, 5)))
    with pytest.raises(ValueError, match="one_call"):
        api.batch_verify(params, [], [], [], one_call=True)                           # one SRS: not the across form
    assert api.verify_mixed([], [], [], mode="rlc", across_srs=True, one_call=True) == []
    api.batch_verify([params], [], [], [], one_call=True)


def test_srs_classes_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_srs.cpp: host code only, its own main, built with ASan + UBSan and run as a program - interleaved
    classes, one class (P is the identity), a class without proofs (front, middle, end, and one whose first listed plan has none),
    listed plans repeating an SRS, 16 and 17 classes with proofs, a 17th listed without one; P is a permutation, stable within a
    class, and pos its inverse - every value restated from the rule by a count of its own"""
    out = str(tmp_path / "h2v_mixed_srs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_srs.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
    assert r.stderr == ""


def test_model_positions_and_sums():
    listed = ["a", "b", "b", "c", "c", "d"]                         # "d" is listed without a proof
    srs = ["c", "a", "b", "a", "c", "b", "a"]
    assert AM.classes(listed, srs) == ["a", "b", "c"]
    P = AM.positions(listed, srs)
    assert P == [5, 0, 3, 1, 6, 4, 2] and sorted(P) == list(range(7))
    assert AM.positions(["x", "y"], ["y", "y", "y"]) == [0, 1, 2]   # one class among the proofs: P(i) = i
    assert AM.positions(["y", "x"], ["x", "y"]) == [1, 0]           # the LIST orders the classes, not the call
    # sums over pairs ([a_i] G, [a_i s_i] G): both forms pass the check, under their own coefficients
    secrets = {"a": 11, "b": 13, "c": 17}
    pairs = [(bls.g1_mul(bls.G1_GEN, 3 + i), bls.g1_mul(bls.G1_GEN, (3 + i) * secrets[s])) for i, s in enumerate(srs)]
    coeff = lambda pos: 1000003 * (pos + 1) + 7
    for form in "AB":
        r_sum, l_sums = AM.sums(listed, srs, pairs, coeff, form)
        assert len(l_sums) == 3 and AM.check([11, 13, 17], r_sum, l_sums)
        at = P if form == "A" else list(range(7))
        want_a = sum(coeff(at[i]) * (3 + i) for i, s in enumerate(srs) if s == "a") % bls.R
        assert l_sums[0] == bls.g1_mul(bls.G1_GEN, want_a)
    assert AM.sums(listed, srs, pairs, coeff, "A") != AM.sums(listed, srs, pairs, coeff, "B")
    # a proof that takes no part has coefficient 0; a class of such proofs alone has an infinite sum and costs no loop
    part = [s != "b" for s in srs]
    r_sum, l_sums = AM.sums(listed, srs, pairs, coeff, "B", part)
    assert l_sums[1] is None and AM.check([11, 13, 17], r_sum, l_sums)
    # a pair on the wrong SRS fails it
    bad = list(pairs)
    bad[2] = (pairs[2][0], bls.g1_mul(pairs[2][0], 11))             # class b's pair made under a's secret
    r_sum, l_sums = AM.sums(listed, srs, bad, coeff, "B")
    assert not AM.check([11, 13, 17], r_sum, l_sums)


def test_cpp_driver_builds_against_the_header(be, tmp_path):
    out = str(tmp_path / "h2v_mixed_across_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_mixed_across_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.access(out, os.X_OK)
