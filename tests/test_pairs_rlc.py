"""The batch-accept pair check (h2v_check_pairs_rlc) and H2V_RLC_FOLD_PAIRS: what can be said without a GPU - the header
declares the entry points and the flag, the Python binding matches them, and the API validates its mode before it touches a
device.  The GPU legs are in tests/test_pairs_rlc_gpu.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_flag():
    h = _header()
    assert re.search(r"\bint\s+h2v_check_pairs_rlc\s*\(\s*const h2v_plan \*plan,\s*uint64_t n,\s*const uint8_t \*pairs", h)
    assert re.search(r"\bint\s+h2v_check_pairs_rlc_device\s*\(\s*const h2v_plan \*plan,\s*uint64_t n,\s*const uint8_t \*pairs", h)
    m = re.search(r"#define\s+H2V_RLC_FOLD_PAIRS\s+(\d+)u", h)
    assert m and int(m.group(1)) == 4
    # the flag shares h2v_rlc_opts.flags with the two older ones: distinct bits
    older = [int(re.search(r"#define\s+%s\s+(\d+)u" % name, h).group(1)) for name in ("H2V_RLC_SEED_GIVEN", "H2V_RLC_ONE_STREAM")]
    assert all(v & 4 == 0 for v in older)


def _arg_count(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, _header(), re.S)
    assert m, name
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


def test_backend_binds_both_entry_points_with_matching_argtypes():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.RLC_FOLD_PAIRS == 4
    assert "h2v_check_pairs_rlc" in backend.EXPORTS and "h2v_check_pairs_rlc_device" in backend.EXPORTS
    L = backend.lib()
    host, dev = L.h2v_check_pairs_rlc.argtypes, L.h2v_check_pairs_rlc_device.argtypes
    assert len(host) == _arg_count("h2v_check_pairs_rlc") == 8
    assert len(dev) == _arg_count("h2v_check_pairs_rlc_device") == 8
    # plan, n, pairs, accept, status, ws, then (opts, fell_back) / (stream, opts)
    assert host[1] is C.c_uint64 and dev[1] is C.c_uint64
    assert host[6] is C.POINTER(backend.RlcOpts) and host[7] is C.POINTER(C.c_int)
    assert dev[6] is C.c_void_p and dev[7] is C.POINTER(backend.RlcOpts)


def test_rlc_opts_carry_the_fold_flag():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend._rlc_opts(None) is None
    o = backend._rlc_opts(None, fold_pairs=True)
    assert o.flags == backend.RLC_FOLD_PAIRS
    o = backend._rlc_opts(bytes(32), one_stream=True, fold_pairs=True)
    assert o.flags == backend.RLC_FOLD_PAIRS | backend.RLC_ONE_STREAM | backend.RLC_SEED_GIVEN


def test_null_arguments_are_refused_before_any_device_work():
    from plutus_halo2_verifier_gen_amd import backend
    L = backend.lib()
    H2V_E_ARG = -1
    acc = (C.c_uint8 * 1)()
    assert L.h2v_check_pairs_rlc(None, 1, bytes(96), acc, None, None, None, None) == H2V_E_ARG
    assert L.h2v_check_pairs_rlc_device(None, 1, None, None, None, None, None, None) == H2V_E_ARG


def test_verifier_check_pairs_rejects_an_unknown_mode():
    from plutus_halo2_verifier_gen_amd import api
    v = api.Verifier.__new__(api.Verifier)      # (no device: the mode is validated before anything else is looked at)
    with pytest.raises(ValueError):
        api.Verifier.check_pairs(v, [bytes(96)], mode="batch")
    with pytest.raises(ValueError):
        api.Verifier.check_pairs(v, [], mode="")
