"""h2v::check_pairs_rlc (include/h2v.hpp) through tests/cpp/h2v_pairs_rlc_driver.cpp, built the way tests/test_cpp_host.py
builds its driver: check_pairs_rlc(vk, prepare_batch(vk, b).pairs).accept == verify_batch(vk, b)."""
import os
import subprocess

import pytest

from tests.test_cpp_host import _write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build_hip()
    out = str(tmp_path_factory.mktemp("cpp") / "h2v_pairs_rlc_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_pairs_rlc_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_driver_builds_against_the_header(driver):
    """no GPU needed: the wrapper compiles with -Wall -Werror and links against the C-ABI library"""
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("corrupt", [(), (1, 4)])
def test_cpp_check_pairs_rlc_is_verify(driver, tmp_path, corrupt):
    plan, batch, want = _write_case(tmp_path, corrupt=corrupt)
    r = subprocess.run([driver, plan, batch], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    assert lines["batch"] == want and lines["pairs_rlc"] == want and lines["pairs"] == want
    assert lines["same_status"] == "1"
    assert lines["fell_back"] == ("1" if corrupt else "0")    # flip_last_scalar: caught only by the pairing
