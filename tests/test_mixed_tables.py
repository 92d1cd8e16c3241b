"""The table block of the mixed-key calls (csrc/h2v_mixed_tables.hpp), what can be said without a GPU: the layout is the one the
hand-written offsets produced (tests/golden/mixed_table_layout.txt, recorded from them), its regions are disjoint, aligned and
inside the extent, and the packer stays inside a buffer of exactly the extent - checked by a stand-alone program under
ASan + UBSan.  The sizes are checked HERE and nowhere on a GPU: a block that is too small is an out-of-bounds write into pinned
memory there."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
HEADER = os.path.join(CSRC, "h2v_mixed_tables.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mixed_table_layout.txt")


def test_tables_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_mixed_tables.cpp: host code only, its own main.  The grid - n = 0..40, 63, 64, 65, 4095, 4096, 4097, 2^22;
    fold-plan tables of 0, 1, 3, 64 plans; lists of 0..3 ranges of 0, 1, 5, 64 groups - line for line as the golden file has it;
    real Partitions (1..5 plans, n up to 40, with and without host offsets) and real GroupTables packed into a vector of exactly
    the extent and read back."""
    out = str(tmp_path / "h2v_mixed_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_mixed_tables.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]) and not [ln for ln in lines if ln.startswith("FAIL")]
    with open(GOLDEN) as f:
        golden = f.read().splitlines()
    assert 100 < len(golden) < 1000
    assert lines[:-1] == golden


def test_tables_header_has_no_hip_in_it():
    with open(HEADER) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()
    for inc in re.findall(r"#include\s*(\S+)", code):
        assert inc in ("<stddef.h>", "<stdint.h>", "<string.h>", "<vector>", '"h2v_mixed.hpp"', '"h2v_mixed_group.hpp"'), inc


def test_no_call_site_lays_the_table_block_out_by_hand():
    """h2v_capi.hip finds a region of the mixed table block through the header alone"""
    with open(os.path.join(CSRC, "h2v_capi.hip")) as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    for old in ("up16(", "o_isrc", "o_perm", "o_grp"):
        assert old not in code, old
    assert code.count("mixedtab::table_block(") == 1 and code.count("mixedtab::pack_tables(") == 1
