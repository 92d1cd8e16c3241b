"""The per-proof pairing's engine table and selection rule (csrc/h2v_pairing_engine.hpp), what can be said without a GPU: the
engine, grid and reported lanes over a grid of batch sizes, in-flight hints, forced options, probe impl numbers and plans with and
without the six-lane line table equal a committed table.

tests/golden/pairing_engine_table.txt records what the launcher did while the choice was a chain of conditions inside h2v_capi.hip,
before it became a header.  It was printed once by a scratch program made of the text of launch_pairing_impl, launch_pairing and the
conditional launch (launch_pairing_behind) verbatim, with every launch line replaced by a print of (kernel, grid), stubs for the
launch options and the SIMD count (1024), the tuner's three candidate lists as they stood, and the case loop of
tests/cpp/h2v_pairing_engine.cpp; the "engine" lines state the kernels' group counts and the numbers include/h2v.h and the probes
document.  A replay of the same chain in Python gave the same 4784 lines.  They are stored as 734: the seven option settings of a
case on one line, an outcome that equals the first one as "=" (_table below expands them).  A change of the rule, a threshold or
the engine table changes this table on purpose, and says so."""
import os
import subprocess

import pytest

from tests import pairing_kinds as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc", "h2v_pairing_engine.hpp")
SOURCE = os.path.join(ROOT, "tests", "cpp", "h2v_pairing_engine.cpp")

NS = 26
HINTS = [1, 3, 4, 7, 8, 16]
OPTIONS = [0, 1, 6, 12, 16, 32, 64]
IMPLS = [-1, 0, 1, 2, 3, 5, 6]


def build_model_program(out_dir, sanitizers: bool) -> str:
    """tests/cpp/h2v_pairing_engine.cpp; under ASan + UBSan for the tests of this file, which run without a GPU, and a plain build
    for tests/test_pairing_engine_rule_gpu.py, which only asks it for answers: no sanitizer runs where the GPU is"""
    out = os.path.join(str(out_dir), "h2v_pairing_engine")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitizers else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [SOURCE, "-o", out])
    return out


def _table():
    """The program's lines from the table's.  "engine" lines are the program's own.  A pipe / probe line is (n, hint or impl,
    six-lane table present) and seven outcomes "engine,grid", one per option in the order of OPTIONS, "=" for one that equals the
    first; the lanes an outcome reports are its engine's option value."""
    lines, lanes = [], {}
    with open(os.path.join(ROOT, "tests", "golden", "pairing_engine_table.txt")) as f:
        for row in f.read().splitlines():
            w = row.split(" ")
            if w[0] == "engine":
                lanes[w[1]] = w[2]
                lines.append(row)
            elif w[0] == "tune":
                lines.append("tune %s : %s" % (w[1], w[2].replace(",", " ")))
            else:
                case, outcomes = (w[:4], w[4:]) if w[0] != "behind" else (w[:2], w[2:])
                assert len(outcomes) == (len(OPTIONS) if w[0] != "behind" else 1)
                for opt, o in zip(OPTIONS, outcomes):
                    name, grid = (outcomes[0] if o == "=" else o).split(",")
                    lines.append("%s : %s %s %s" % (" ".join(case + ([str(opt)] if w[0] != "behind" else [])), name, grid, lanes[name]))
    return lines


@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    r = subprocess.run([build_model_program(tmp_path_factory.mktemp("pairing_engine"), sanitizers=True)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_engine_model_program_under_sanitizers_matches_the_table(program_lines):
    """host code only, its own main, built with ASan + UBSan and run as a program; one line per case, every line equal to the
    table's"""
    want, got = _table(), program_lines
    # the engine table; pipelines: sizes x hints x table present / absent x options; probes: sizes x impls x the same; the conditional
    # launch and the tuner's candidates per size
    assert len(want) == 6 + NS * len(HINTS) * 2 * len(OPTIONS) + NS * len(IMPLS) * 2 * len(OPTIONS) + NS + NS
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d cases differ: got / the table has\n%s" % (len(wrong), "\n".join("%s / %s" % gw for gw in wrong))
    # the grid is wide enough to tell the rule's branches apart: every engine the rule can choose is its own choice somewhere - all
    # but the one-lane cross-check kernel, which runs only when asked for - and every engine is a forced one somewhere
    engine = lambda line: line.split(" : ")[1].split()[0]
    pipes = [line for line in want if line.startswith("pipe ")]
    names = {e.name for e in pk.ENGINES}
    assert {engine(line) for line in pipes if line.split(" : ")[0].endswith(" 0")} == names - {"one_lane"}
    assert {engine(line) for line in pipes if not line.split(" : ")[0].endswith(" 0")} == names
    # the two recorded oddities (h2v_pairing_engine.hpp: pairing_engine).  (1) option 1, eight batches in flight: the twelve-lane
    # engine from 3/8 of 1024 SIMDs up, the one-lane kernel below
    assert "pipe 383 8 1 1 : one_lane 6 1" in want and "pipe 384 8 1 1 : twelve 77 12" in want and "pipe 8192 16 0 1 : twelve 1639 12" in want
    assert "pipe 8192 7 1 1 : one_lane 128 1" in want
    # (2) option 6 without the line table: the rule's answer for that size and hint - wide, coop 32, narrow or twelve
    for case, answer in (("512 4", "wide 512 64"), ("513 4", "coop32 257 32"), ("4096 4", "narrow 1024 16"), ("4096 8", "twelve 820 12")):
        assert "pipe %s 0 6 : %s" % (case, answer) in want and "pipe %s 0 0 : %s" % (case, answer) in want
    assert "pipe 4096 4 1 6 : six 410 6" in want


def test_engine_model_header_has_no_hip_in_it():
    with open(HEADER) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower()
    assert "#include" not in code.replace("#include <stdint.h>", "")


def test_pairing_kinds_engines_are_the_engine_table(program_lines):
    """tests/pairing_kinds.py keeps its own tuples (the GPU suite imports it where nothing is compiled): they are the header's
    table.  An engine that pairing_kinds reaches as impl 1 (the rule) under an option is reached by that engine's option value."""
    table = {}
    for line in program_lines:
        w = line.split()
        if w[0] == "engine":
            table[w[1]] = (int(w[2]), int(w[3]), int(w[4]))
    assert len(table) == 6 and set(table) == {e.name for e in pk.ENGINES} and len(pk.ENGINES) == 6
    for e in pk.ENGINES:
        option, impl, per_wave = table[e.name]
        assert (e.lanes, e.per_wave) == (option, per_wave), e
        assert (e.impl, e.option) == ((1, option) if e.option else (impl, 0)), e
