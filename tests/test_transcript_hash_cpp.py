"""The transcript hash through include/h2v.hpp (tests/cpp/h2v_transcript_driver.cpp, built the way tests/test_cpp_host.py
builds its driver): a key description naming blake2b-512 compiles behind the C-ABI to a version-5 plan, the wrapper reports
its kind and key, proofs forged for that key verify under the Blake2b512 tag and reject (by the pairing) when they were
forged for the Cardano key, and prepare() under the other tag is refused as misuse."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build_hip()
    out = str(tmp_path_factory.mktemp("cpp") / "h2v_transcript_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "h2v_transcript_driver.cpp"), "-o", out,
                           "-L", PKG, "-lh2v_hip", "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_driver_builds_against_the_header(driver):
    """no GPU needed: both instantiations of h2v::Transcript and h2v::prepare compile with -Wall -Werror"""
    assert os.access(driver, os.X_OK)


def _case(tmp_path, key_vk, forge_vk, n=5, corrupt=(2,)):
    """vk.json of key_vk and a batch forged for forge_vk (the layout of tests/test_cpp_host.py: _write_case)"""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    _vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(forge_vk)
    b = synth.forge_batch(forge_vk, td, n, seed=71, plan=pl, workers=1)
    proofs = [b.proof(i) for i in range(n)]
    for i in corrupt:
        proofs[i] = synth.corrupt(pl, proofs[i], b.instances[96 * i:96 * i + 96], "flip_last_scalar", None)[0]
    blob = struct.pack("<III", n, forge_vk.n_public_inputs, 0)
    for i in range(n):
        blob += struct.pack("<I", len(proofs[i])) + proofs[i] + b.instances[96 * i:96 * i + 96]
    (tmp_path / "vk.json").write_text(key_vk.to_json())
    (tmp_path / "batch.bin").write_bytes(blob)
    return str(tmp_path / "vk.json"), str(tmp_path / "batch.bin"), "".join("0" if i in corrupt else "1" for i in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["flavoured", "cardano", "wrong_hash"])
def test_cpp_transcript_tags_on_gpu(driver, tmp_path, case):
    from plutus_halo2_verifier_gen_amd import vk as V
    vk, _ = V.simple_mul_vk()
    fv = V.with_transcript_hash(vk, "blake2b-512")
    key_vk, forge_vk = {"flavoured": (fv, fv), "cardano": (vk, vk), "wrong_hash": (fv, vk)}[case]
    vk_json, batch, want = _case(tmp_path, key_vk, forge_vk)
    r = subprocess.run([driver, vk_json, batch], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) if " " in l else (l, "") for l in r.stdout.strip().splitlines())
    flav = key_vk is fv
    assert lines["plan_version"] == ("5" if flav else "4") and lines["kind"] == ("1" if flav else "0")
    assert lines["key"] == (V.DEFAULT_BLAKE2B_512_KEY.hex() if flav else "")
    if case == "wrong_hash":     # a proof made under another hash is a reject by the pairing, never an API error
        want = "0" * len(want)
    assert lines["single"] == want and lines["batch"] == want
    assert lines["status"].split() == ["0" if c == "1" else "16" for c in want]      # H2V_ST_PAIRING
    assert lines["mismatch_refused"] == "1"
