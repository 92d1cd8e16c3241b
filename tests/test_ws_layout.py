"""The size tables of a workspace's memory (csrc/h2v_ws_layout.hpp), what can be said without a GPU: every buffer of every set
has the bytes the allocation sites computed before the tables existed (tests/golden/workspace_layout.txt, recorded from those
expressions), the group stage's pool binds inside a block of exactly its total with no two regions overlapping, Shape's fit
rule is the one ws_fits had, and shape_union is the smallest shape both fit - checked by a stand-alone program under
ASan + UBSan.  tests/test_workspace_memory_gpu.py holds the same tables against what the library really allocates."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
HEADER = os.path.join(CSRC, "h2v_ws_layout.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_layout.txt")


def _code(path):
    with open(path) as f:
        return "\n".join(line.split("//")[0] for line in f.read().splitlines())


def test_layout_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_ws_layout.cpp: host code only, its own main.  The grid - capacities 1, 63, 64, 65, 4096, 2^24; the pipeline set
    for the facts of every built-in key, one of them and a synthetic one also with a trace, with recursion flipped and with the
    fixed-base sum flipped, MSM widths 64, 65, 96, a global register file; the three RLC shapes; the group stage of 256, 260, 4096,
    32768 proofs of a plan and of pairs - line for line as the golden file has it."""
    out = str(tmp_path / "h2v_ws_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_ws_layout.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]) and not [ln for ln in lines if ln.startswith("FAIL")]
    with open(GOLDEN) as f:
        golden = f.read().splitlines()
    assert 200 < len(golden) < 400
    assert lines[:-1] == golden


def test_layout_header_has_no_hip_in_it():
    for path in (HEADER, os.path.join(CSRC, "h2v_pip_sizes.hpp")):
        code = _code(path)
        assert "hip" not in code.lower(), path
        for inc in re.findall(r"#include\s*(\S+)", code):
            assert inc in ("<stddef.h>", "<stdint.h>", '"h2v_mixed_fold.hpp"', '"h2v_msm_shape.hpp"', '"h2v_pip_sizes.hpp"', '"h2v_plan.h"'), inc


def test_every_block_and_event_goes_through_the_owner():
    """h2v_capi.hip allocates, frees, creates and destroys in ONE place, and keeps no hand-written list of what to free"""
    code = _code(os.path.join(CSRC, "h2v_capi.hip"))
    begin, end = code.index("struct Owner {"), code.index("template <bool PINNED> struct GrowBuf")
    outside = re.sub(r'"(?:[^"\\]|\\.)*"', '""', code[:begin] + code[end:])        # (error messages name the calls)
    for call in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipEventCreate(", "hipEventCreateWithFlags(", "hipEventDestroy(",
                 "ptrs[]", "old[]"):
        assert call not in outside, call
    for call in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipEventCreateWithFlags(", "hipEventDestroy("):
        assert code[begin:end].count(call) == 1, call


def test_bucket_msm_constants_have_one_definition():
    for name in ("PIP_PT_DW", "PIP_PART_DW", "PIP_MAX_W", "PIP_MAX_C", "PIP_N_CLASSES", "PIP_CLS_DW"):
        hits = [f for f in sorted(os.listdir(CSRC)) if re.search(r"#define\s+%s\b" % name, open(os.path.join(CSRC, f)).read())]
        assert hits == ["h2v_pip_sizes.hpp"], (name, hits)
