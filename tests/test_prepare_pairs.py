"""CPU tests of the prepare / pair-check surface (include/h2v.h: h2v_prepare_batch(_device), h2v_check_pairs(_device)): the
exports are declared and bound, the h2v.hpp wrappers compile and link, every entry point refuses a NULL plan or output
before it touches a device, and the fail-closed encoding of a rejected proof (96 zero bytes) decodes nowhere."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd")
NEW = ["h2v_prepare_batch", "h2v_prepare_batch_device", "h2v_check_pairs", "h2v_check_pairs_device"]


@pytest.fixture(scope="module")
def be():
    import __graft_entry__ as ge
    ge.build_hip()
    from plutus_halo2_verifier_gen_amd import backend
    return backend


def test_exports_are_declared_and_bound(be):
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in be.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
        getattr(be.lib(), name)


def test_cpp_wrappers_compile_and_link(be, tmp_path):
    out = str(tmp_path / "h2v_prepare_pairs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_prepare_pairs.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(out)


def _err(be):
    return (be.lib().h2v_last_error() or b"").decode()


def test_null_plan_or_output_is_an_argument_error(be):
    """Checked before anything else: no device is needed.  (A stand-in plan handle is never dereferenced before the
    output pointer has been checked.)"""
    L = be.lib()
    b = be.Batch(1, None, None, None, None)
    out = C.create_string_buffer(96)
    st = (C.c_uint32 * 1)()
    fake = C.create_string_buffer(4096)
    fake_plan = C.cast(fake, C.c_void_p)
    cases = [
        (lambda: L.h2v_prepare_batch(None, C.byref(b), out, st, None), "plan"),
        (lambda: L.h2v_prepare_batch(fake_plan, C.byref(b), None, st, None), "pairs"),
        (lambda: L.h2v_prepare_batch_device(None, C.byref(b), out, st, None, None), "plan"),
        (lambda: L.h2v_prepare_batch_device(fake_plan, C.byref(b), None, st, None, None), "pairs"),
        (lambda: L.h2v_check_pairs(None, 1, bytes(96), out, st, None), "plan"),
        (lambda: L.h2v_check_pairs(fake_plan, 1, bytes(96), None, st, None), "accept"),
        (lambda: L.h2v_check_pairs(fake_plan, 1, None, out, st, None), "pairs"),
        (lambda: L.h2v_check_pairs_device(None, 1, out, out, st, None, None), "plan"),
        (lambda: L.h2v_check_pairs_device(fake_plan, 1, out, None, st, None, None), "accept"),
        (lambda: L.h2v_check_pairs_device(fake_plan, 1, None, out, st, None, None), "pairs"),
    ]
    for call, arg in cases:
        assert call() == -1                     # H2V_E_ARG
        assert arg in _err(be), (arg, _err(be))


def test_zero_pair_is_not_an_encoding(orc):
    """A proof rejected before the pairing gets 96 zero bytes: neither half decodes (compression flag unset), so the pair
    check rejects it as a bad point - unlike (inf, inf), which is a valid pair that passes the pairing."""
    from plutus_halo2_verifier_gen_amd import bls12_381 as bls
    with pytest.raises(ValueError):
        bls.g1_decompress(bytes(48))
    ok, _ = orc.g1_decompress(bytes(48))
    assert not ok
    inf = bls.g1_compress(None)
    assert inf == b"\xc0" + bytes(47)
    assert bls.g1_decompress(inf) is None and orc.g1_decompress(inf) == (True, None)
