"""The table block of a mixed-key call with keyed leaves (H2V_RLC_SEED_KEYED; csrc/h2v_mixed_tables.hpp), without a GPU: the plan
index per position and the key tags lie behind every other region, every region is disjoint from the others, 16-byte aligned and
inside the extent, and the packer stays inside a buffer of exactly the extent - a stand-alone program under ASan + UBSan.  The sizes
are checked HERE and nowhere on a GPU: a block that is too small is an out-of-bounds write into pinned memory there."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyed_tables_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_tables_keyed.cpp: host code only, its own main.  n = 0, 1, 64, 65 x 1, 3, 1024 listed plans, with and
    without a fold table and grouped ranges; real Partitions packed into a vector of exactly the extent and read back."""
    out = str(tmp_path / "h2v_mixed_tables_keyed")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_tables_keyed.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]) and int(lines[-1].split()[1]) > 1000 and not [ln for ln in lines if ln.startswith("FAIL")]
