"""The layouts of the host-buffer calls (csrc/h2v_hostcall_layout.hpp), what can be said without a GPU: the input block, the
result block of every call kind, the download block's verdict word and the packer, checked by a stand-alone program under
ASan + UBSan.  The sizes are checked HERE and nowhere on a GPU: a layout that is too small is an out-of-bounds write there."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
HEADER = os.path.join(CSRC, "h2v_hostcall_layout.hpp")


def test_layout_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_hostcall_layout.cpp: host code only, its own main.  Result blocks: every call kind, n = 0..300, 4095, 4096,
    4097, 2^22 - regions disjoint, 16-byte aligned, inside the extent; the verdict word inside accept_extent(n); extents monotone.
    Input blocks: n = 0..40 x instance / committed / proof sizes - sections disjoint and aligned, the 64 zero bytes inside `need`,
    n + 1 offsets.  The packer into a vector of exactly `need` bytes, first offset 0 and 48: offsets rebased, the proof bytes
    those from proof_off[0] on.  The old formulas beside the new extents go to the log."""
    out = str(tmp_path / "h2v_hostcall_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_hostcall_layout.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    old = [ln for ln in lines if ln.startswith("old ")]
    assert len(old) == 4 * 5                                  # n = 1, 100, 186, 4096: four call kinds and the download block
    for ln in old:
        m = re.fullmatch(r"old n=\d+ (\w+): addressed (\d+) of a block of \d+; now extent (\d+)", ln)
        if m:                                                 # no form's block ends before the last byte the form addressed
            assert int(m.group(3)) >= int(m.group(2)), ln


def test_layout_header_has_no_hip_in_it():
    with open(HEADER) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()
    for inc in re.findall(r"#include\s*(\S+)", code):
        assert inc in ("<stddef.h>", "<stdint.h>", "<string.h>"), inc


def test_no_call_site_lays_a_block_out_by_hand():
    """h2v_capi.hip finds a region of a host-buffer block through the header alone: none of the old formulas is left in it"""
    with open(os.path.join(CSRC, "h2v_capi.hip")) as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    for old in ("n * 100", "n * (96 + 4 + 1)", "up16(n)", "96 + (size_t)n * 4", "(n + 7) & ~"):
        assert old not in code, old
    assert code.count("hostcall::result_block(") == 1 and code.count("hostcall::input_block(") == 1
