"""The launch-shape model of the per-proof G1 MSM (csrc/h2v_msm_shape.hpp), what can be said without a GPU: the decisions over
a grid of sums, batch sizes, in-flight hints and forced options equal a committed table.

tests/golden/msm_shape_table.txt records the decisions of the model as it stood inside h2v_capi.hip, before it became a header:
it was printed once by a program made of those functions' text verbatim, a stub for the launch options and one for the SIMD
count (1024), and the case loop of tests/cpp/h2v_msm_shape.cpp; its 5616 lines are stored as 432, each option's outcome as its
difference from the outcome without options (_table below expands them).  A change of a rule or a constant of the model changes the
table on purpose, and says so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "h2v_msm_shape.hpp")


OPTS = ["none=0", "lpt=1", "lpt=2", "lpt=8", "bs=64", "bs=256", "bs=512", "tpl=2", "tpl=3", "tpl=4", "fix=-1", "fix=1", "fix=4"]


def _table():
    """The program's lines from the table's.  A table line is one (T, n_var, n_fix, n, hint) and thirteen outcomes, one per
    option setting in the order of OPTS; an outcome is the four groups of a program line joined by "/" with "," for " ", "-" for
    a split that is off; from the second outcome on a group that equals the first outcome's is left empty, "=" if all four do."""
    lines = []
    with open(os.path.join(ROOT, "tests", "golden", "msm_shape_table.txt")) as f:
        for row in f.read().splitlines():
            case, outcomes = row.split(" ")[:5], row.split(" ")[5:]
            assert len(outcomes) == len(OPTS)
            base = outcomes[0].split("/")
            for opt, o in zip(OPTS, outcomes):
                groups = base if o == "=" else [g or b for g, b in zip(o.split("/"), base)]
                groups = ["0,0,0,0,0,0,0" if g == "-" else g for g in groups]
                lines.append(" : ".join([" ".join(case + [opt])] + [g.replace(",", " ") for g in groups]))
    return lines


def test_shape_model_program_under_sanitizers_matches_the_table(tmp_path):
    """tests/cpp/h2v_msm_shape.cpp: host code only, its own main, built with ASan + UBSan and run as a program; one line per
    case, every line equal to the table's"""
    out = str(tmp_path / "h2v_msm_shape")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_msm_shape.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    want = _table()
    got = r.stdout.splitlines()
    # 16 sums x 9 batch sizes x 3 hints x 13 option settings
    assert len(want) == 16 * 9 * 3 * 13
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d cases differ, the first: got %r, the table has %r" % (len(wrong), wrong[0][0], wrong[0][1])
    # the grid is wide enough to tell shapes apart: every lane form, every block size, segments and splits all occur
    singles = {tuple(line.split(" : ")[1].split()[:3]) for line in want}
    assert {s[0] for s in singles} == {"1", "2", "8"} and {s[1] for s in singles} >= {"64", "256", "512"}
    assert any(int(s[2]) > 1 for s in singles) and any(line.split(" : ")[2].startswith("1 ") for line in want)


def test_shape_model_header_has_no_hip_in_it():
    with open(HEADER) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()
    assert "#include" not in code.replace("#include <stdint.h>", "")
