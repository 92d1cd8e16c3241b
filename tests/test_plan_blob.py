"""Plan loading, what can be said without a GPU.  csrc/h2v_planblob.hpp reads the untrusted blob on the host: a stand-alone program
under ASan + UBSan (tests/cpp/h2v_planblob.cpp) runs it over the recorded corpus of tests/plan_loading.py with every blob in a heap
block of exactly its length, and its verdicts - and the library's - must be those of tests/golden/plan_load_verdicts.txt, recorded
from the loader as it was before the parser left h2v_capi.hip.  Beside that: the six-lane unit-line constants and the 28-bit slot
codec against big-integer arithmetic, the opcode table of h2v_plan.h against plan.py's own lists, the plan compiler's blobs against
digests recorded before it read that table, and the structure the consolidation leaves behind."""
import hashlib
import os
import random
import re
import struct
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import backend, bls12_381 as bls, plan as PL
from plutus_halo2_verifier_gen_amd import vk as V
from tests import plan_loading as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_load_verdicts.txt")
P = bls.P


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("planblob") / "h2v_planblob")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "h2v_planblob.cpp"), "-o", out])

    def run(*args):
        r = subprocess.run([out] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def plans():
    return C.corpus_plans()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return f.read().splitlines()


def test_corpus_is_the_recorded_one(plans, golden):
    cases = C.corpus(plans)
    assert [ln.split("\t")[0] for ln in golden] == [c[0] for c in cases] and 1500 <= len(cases) <= 2000
    said = {ln.split("\t", 2)[2] for ln in golden if not ln.endswith("\tvalid")}
    # every refusal of the parser is in the recording at least once (the numbers in a message aside)
    with open(os.path.join(CSRC, "h2v_planblob.hpp")) as f:
        for msg in re.findall(r'fail\((?:H2V_E_\w+, )?(?:std::string\()?"([^"]+)"', f.read()):
            assert any(msg in s for s in said), msg
    assert sum(ln.endswith("\tvalid") for ln in golden) > 500


def test_parser_program_under_sanitizers_gives_the_recorded_verdicts(driver, plans, golden, tmp_path):
    """parse on a heap block of exactly len bytes per case, then - accepted blobs - device_terms, fixed_tables, six_line_tables, the
    digests: no sanitizer report, and line by line what the loader said before the parser moved"""
    for name, blob in plans.items():
        (tmp_path / (name + ".bin")).write_bytes(blob)
    cases = C.corpus(plans)
    with open(tmp_path / "cases.txt", "w") as f:
        for cid, name, cut, patches in cases:
            f.write("%s %s %d %d%s\n" % (cid, name, -1 if cut is None else cut, len(patches),
                                         "".join(" %d %s" % (off, data.hex()) for off, data in patches)))
    assert driver("corpus", tmp_path / "cases.txt", tmp_path) == golden


def test_library_gives_the_recorded_verdicts(plans, golden):
    """the same corpus through h2v_plan_load: codes and h2v_last_error texts; `valid` is H2V_E_DEVICE without a GPU and 0 with one"""
    load = C.plan_loader()
    ok_rc = 0 if backend.device_count() >= 1 else C.E_DEVICE
    for case, want in zip(C.corpus(plans), golden):
        rc, msg = load(C.case_blob(plans, case))
        assert C.verdict_line(case[0], rc, msg) == want
        assert rc == ok_rc or not want.endswith("\tvalid"), (case[0], rc, msg)


def _six_tables_by_bigint(pl):
    """[line][loop][A0, A1, B0, B1] as operand slots, then [1, K1, K2, K1 K2] as 2 x 48 Montgomery bytes: A = -lambda / c, B = 1 / c,
    K_u the product of loop u's c along the Miller schedule (k <- k^2 per bit, k <- k c per line)"""
    tabs = (pl.lines_sg2, pl.lines_g2)
    out = b""
    for ln in range(PL.MILLER_LINES):
        for tab in tabs:
            lam, c = tab[ln]
            b = bls.f2_inv(c)
            a = bls.f2_mul(bls.f2_neg(lam), b)
            out += b"".join(bls.fp_mont28_slot(x) for x in (a[0], a[1], b[0], b[1]))
    ks = []
    for tab in tabs:
        k, idx = bls.F2_ONE, 0
        for bit in bls.miller_bits():
            k = bls.f2_sqr(k)
            for _ in range(2 if bit else 1):
                k = bls.f2_mul(k, tab[idx][1])
                idx += 1
        assert idx == PL.MILLER_LINES
        ks.append(k)
    for k in (bls.F2_ONE, ks[0], ks[1], bls.f2_mul(ks[0], ks[1])):
        out += bls.f2_mont_bytes(k)
    return out


@pytest.mark.parametrize("name", ["simple_mul", "ivc"])
def test_unit_line_constants_against_big_integers(driver, name, tmp_path):
    pl = PL.compile_plan(V.BUILDERS[name]()[0])
    blob = pl.to_bytes()
    (tmp_path / "plan.bin").write_bytes(blob)
    got = b"".join(struct.pack("<I", int(ln, 16)) for ln in driver("six", tmp_path / "plan.bin"))
    want = _six_tables_by_bigint(pl)
    assert len(want) == 4 * (PL.MILLER_LINES * 2 * 4 * 16 + 4 * 24)
    assert [got[k:k + 4] for k in range(0, len(got), 4)] == [want[k:k + 4] for k in range(0, len(want), 4)]
    # some c = 0: no table (the loader then does not offer the engine)
    w = struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, blob, 8)
    for off_word, line in ((23, 0), (24, 67), (23, 41)):
        m = bytearray(blob)
        at = w[off_word] + 512 * line + 4 * 64
        m[at:at + 128] = bytes(128)
        (tmp_path / "zero.bin").write_bytes(m)
        assert driver("six", tmp_path / "zero.bin") == ["no table"]


def test_slot_codec_round_trips_and_is_fp_mont28_slot(driver, tmp_path):
    rng = random.Random(28)
    vals = [0, 1, P - 1] + [rng.randrange(P) for _ in range(200)]
    (tmp_path / "vals.txt").write_text("".join("%096x\n" % v for v in vals))
    got = driver("slots", tmp_path / "vals.txt")      # (the program itself requires unpack(pack(x)) == x)
    assert got == [bls.fp_mont28_slot(v).hex() for v in vals]


def _model_facts(op):
    """(reads a, reads b, writes dst, transcript, serial) of an opcode as plan.py has them: _uses / _defines, TRANSCRIPT_OPS, and
    check_bundles put to the question with a two-lane bundle; then run_plan on a one-record program, by what it does"""
    uses = PL._uses(op, "dst", "a", "b")
    assert "dst" not in uses
    facts = ["a" in uses, "b" in uses, PL._defines(op), op in PL.TRANSCRIPT_OPS]
    try:
        PL.check_bundles([(op, 7, 8, 9), (PL.OP_CONST, 1, 0, 0)], 2)
        facts.append(False)
    except AssertionError as e:
        assert "shares its bundle" in str(e)
        facts.append(True)
    try:
        PL.check_bundles([(PL.OP_NOP, 0, 0, 0), (op, 7, 8, 9)], 2)
        assert not facts[4]
    except AssertionError as e:
        assert "off lane 0" in str(e) and facts[4]
    return tuple(facts)


def _run_plan_facts(op):
    """(reads a, reads b, writes dst) of an opcode by what plan.run_plan does with it: r0 and r1 are set to constants, the record
    (op, 2, 0, 1) runs, a SQUEEZE into r3 makes what it absorbed visible; a register is read if changing it changes the outcome"""
    base = PL.compile_plan(V.simple_mul_vk()[0], lanes=1)
    proof = bytes(range(1, 200)) * 8

    def outcome(x, y):
        pl = PL.Plan(**{**base.__dict__, "consts": [999, 12345, x, y], "n_regs": 4, "wide": None,
                        "instrs": [(PL.OP_CONST, 0, 2, 0), (PL.OP_CONST, 1, 3, 0), (PL.OP_CONST, 2, 1, 0), (op, 2, 0, 1),
                                   (PL.OP_SQUEEZE, 3, 0, 0), (PL.OP_END, 0, 0, 0)]})
        scalars, regs, status = PL.run_plan(pl, proof, [77, 78, 79], bytes(48))
        return scalars, regs[2:], status              # (r0 and r1 themselves aside)
    ref = outcome(7, 9)
    return outcome(0, 9) != ref, outcome(7, 0) != ref, ref[1][0] != 12345


def test_opcode_table_is_plan_py_s(driver):
    rows = [tuple(int(x) for x in ln.split()) for ln in driver("ops")]
    assert [r[0] for r in rows] == list(range(len(PL.OP_NAMES))) and PL.OP_NOP == len(rows) - 1
    for op, *facts in rows:
        assert tuple(bool(x) for x in facts) == _model_facts(op), PL.OP_NAMES[op]
        if op != PL.OP_END:                       # (run_plan stops at END: nothing to observe)
            assert tuple(bool(x) for x in facts[:3]) == _run_plan_facts(op), PL.OP_NAMES[op]
    # END is serial for the bundle rule and no transcript operation for the scheduler: the one row where the two differ
    assert [op for op, _a, _b, _w, tr, serial in rows if tr != serial] == [PL.OP_END]


def compile_keys():
    """(name, key) of every verifying-key description the suite sends through h2v_plan_compile"""
    for group in (V.BUILDERS, V.WIDE_BUILDERS):
        for name, build in group.items():
            yield name, build()[0]
    yield "bls12381_chip_alone", V.bls12381_vk(chip_alone=True)[0]
    for name in ("simple_mul", "lookup_table", "trashcan_mix", "phased", "ivc"):
        for key in (None, b"", b"\x5a", V.DEFAULT_BLAKE2B_512_KEY, bytes(range(101, 165))):
            yield "%s/blake2b-512/%s" % (name, "default" if key is None else key.hex()), V.with_transcript_hash(V.BUILDERS[name]()[0], "blake2b-512", key)


# blake2b-128 of h2v_plan_compile's blob of each of them, recorded before the compiler read the opcode table, the slot codec and the
# LDS predicate from the shared headers
COMPILED_BEFORE = {
    "simple_mul": "028ee5ab76ddeb8095aea0ee512391bd",
    "lookup_table": "571bba00085ad3be15f574e9070ff5bb",
    "atms_with_lookups": "907193b9493cc1d58db10598e92c7814",
    "sha256": "dd7e28fe2a7a893a69f47eec794bcc4a",
    "secp256k1": "13d78bf0a9afd4e462fdb0537b0ab2a7",
    "ivc": "b34aec6b7d5a0326c271c0142013d570",
    "trashcan_mix": "346fa914a9a8d7e6ede5b879af2a45de",
    "phased": "cea7f71a3271858eef7dfc9bfad6d13e",
    "bls12381": "69c75a1699e6ca437e6638b504dd6215",
    "composite": "2fcfcc6dd7ade23cc3374207d26846ad",
    "wide335": "487e63610ac18614de83dd4dd08168c6",
    "wide677": "3d6aba67d8146eaee3bb937cdbdcef57",
    "ivc_wide": "29d6f25169d4b089a1f18b69e96aa855",
    "bls12381_chip_alone": "240e8805a1d2af87481f78efd01bbeb0",
    "simple_mul/blake2b-512/default": "aa60720b42d2304db79e5eb2465fa33b",
    "simple_mul/blake2b-512/": "b71fc515d593ffef0dec49b4690f91d8",
    "simple_mul/blake2b-512/5a": "935f11017221f4437398d9c5d92bf3be",
    "simple_mul/blake2b-512/446f6d61696e20736570617261746f7220666f72207472616e736372697074": "aa60720b42d2304db79e5eb2465fa33b",
    "simple_mul/blake2b-512/65666768696a6b6c6d6e6f707172737475767778797a7b7c7d7e7f808182838485868788898a8b8c8d8e8f909192939495969798999a9b9c9d9e9fa0a1a2a3a4": "9c86969fc75ac0b2ab751eaedcf4a712",
    "lookup_table/blake2b-512/default": "1e3ccef648558ded60aa8639c360ba55",
    "lookup_table/blake2b-512/": "31adebd46fd3afd7b5701cf18b4d8e98",
    "lookup_table/blake2b-512/5a": "991eb6a6b357e63da3ad25d28b040882",
    "lookup_table/blake2b-512/446f6d61696e20736570617261746f7220666f72207472616e736372697074": "1e3ccef648558ded60aa8639c360ba55",
    "lookup_table/blake2b-512/65666768696a6b6c6d6e6f707172737475767778797a7b7c7d7e7f808182838485868788898a8b8c8d8e8f909192939495969798999a9b9c9d9e9fa0a1a2a3a4": "025a0ab5e2465b14448e157f5a198bb3",
    "trashcan_mix/blake2b-512/default": "4a2d9b997dd8eb08f14c9891bc6e2f19",
    "trashcan_mix/blake2b-512/": "a70cd8a90e657cea689bb2900e48800c",
    "trashcan_mix/blake2b-512/5a": "7b90fcdec0174d58b4494d5ae0a70609",
    "trashcan_mix/blake2b-512/446f6d61696e20736570617261746f7220666f72207472616e736372697074": "4a2d9b997dd8eb08f14c9891bc6e2f19",
    "trashcan_mix/blake2b-512/65666768696a6b6c6d6e6f707172737475767778797a7b7c7d7e7f808182838485868788898a8b8c8d8e8f909192939495969798999a9b9c9d9e9fa0a1a2a3a4": "af109f2873d011898b0929927af1ad5a",
    "phased/blake2b-512/default": "620a57d0986439c4382bbd73dda7f20d",
    "phased/blake2b-512/": "e6c569597a14106381ac8d9b2b790f2f",
    "phased/blake2b-512/5a": "368d9f7146209e971480ac8296b3c0cc",
    "phased/blake2b-512/446f6d61696e20736570617261746f7220666f72207472616e736372697074": "620a57d0986439c4382bbd73dda7f20d",
    "phased/blake2b-512/65666768696a6b6c6d6e6f707172737475767778797a7b7c7d7e7f808182838485868788898a8b8c8d8e8f909192939495969798999a9b9c9d9e9fa0a1a2a3a4": "808bb79ca8c127162c056c309e988cdd",
    "ivc/blake2b-512/default": "3984590e7ad033e102cb2bb9235197cc",
    "ivc/blake2b-512/": "0ca2a65f41efbcbd465396781fbe83df",
    "ivc/blake2b-512/5a": "70e55adb45fc6f14c316742679ebf344",
    "ivc/blake2b-512/446f6d61696e20736570617261746f7220666f72207472616e736372697074": "3984590e7ad033e102cb2bb9235197cc",
    "ivc/blake2b-512/65666768696a6b6c6d6e6f707172737475767778797a7b7c7d7e7f808182838485868788898a8b8c8d8e8f909192939495969798999a9b9c9d9e9fa0a1a2a3a4": "da6f1a5cb8f75851b274c5bf02994fc6",
}


def test_compiler_output_is_byte_identical():
    got = {name: hashlib.blake2b(backend.plan_compile(key.to_json()), digest_size=16).hexdigest() for name, key in compile_keys()}
    assert got == COMPILED_BEFORE


def _code(name):
    with open(os.path.join(CSRC, name)) as f:
        return "\n".join(line.split("//")[0] for line in f.read().splitlines())


def test_blob_header_has_no_gpu_runtime_in_it():
    code = _code("h2v_planblob.hpp")
    assert "hip" not in code.lower()
    for inc in re.findall(r"#include\s*(\S+)", code):
        assert inc in ("<stdint.h>", "<string.h>", "<string>", "<vector>", '"../../include/h2v.h"', '"h2v_hostmath.hpp"', '"h2v_plan.h"',
                       '"h2v_seed.hpp"'), inc
    assert not re.search(r"#define\s+H2V_(E_|OK|MAX_MSM_TERMS)", code)            # taken from include/h2v.h, not restated


def _function(code, head):
    """the text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    at = code.index(head)
    first = code[at:code.index("\n", at)]
    return first if first.rstrip().endswith("}") else code[at:code.index("\n}", at)]


def test_structure_after_the_consolidation():
    capi, plancc = _code("h2v_capi.hip"), _code("h2v_plancc.hpp")
    assert "H2V_HW_" not in capi and "H2V_OP_" not in capi
    loader = _function(capi, 'extern "C" int h2v_plan_load_ex(')
    assert loader.count("plan_release(") == 1 and "hipFree(" not in loader and "delete p" in loader and loader.count("delete p") == 1
    assert capi.count("planblob::parse(") == 1
    for fn in ("static inline int uses_of(", "static inline bool defines(", "static inline bool is_transcript_op(", "static Allocated allocate("):
        body = _function(plancc, fn)
        assert not re.search(r"H2V_OP_(?!NOP\b)", body), fn          # (allocate writes NOP into the idle lanes)
    # the slot format, the LDS budget and its predicate: once in C++
    srcs = {n: _code(n) for n in os.listdir(CSRC) if n.endswith((".h", ".hpp", ".hip", ".inc"))}
    assert [n for n, s in srcs.items() if "0xfffffffu" in s and "28 * i" in s] == ["h2v_hostmath.hpp"]
    assert [n for n, s in srcs.items() if "160 * 1024" in s] == ["h2v_plan.h"]
    assert [n for n, s in srcs.items() if re.search(r"\* 32 \* \(?64 /", s)] == ["h2v_plan.h"]
    # less code than before: h2v_capi.hip had 4276 lines and h2v_plancc.hpp 1122 when the parser lived in the former
    n = {name: len(open(os.path.join(CSRC, name)).read().splitlines()) for name in ("h2v_capi.hip", "h2v_plancc.hpp", "h2v_planblob.hpp")}
    assert n["h2v_capi.hip"] < 4276 and sum(n.values()) <= 4276 + 1122, n
