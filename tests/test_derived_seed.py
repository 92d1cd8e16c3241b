"""Derived batch seeds (H2V_RLC_SEED_TRANSCRIPT, include/h2v.h), what can be said without a GPU: the public
model plutus_halo2_verifier_gen_amd/seed.py against a second, straight-line statement of the rule written here and against three
committed seeds; what the seed binds; the host-only layout header under ASan + UBSan; the header and the binding."""
import ctypes as C
import hashlib
import os
import random
import re
import struct
import subprocess

import pytest

from plutus_halo2_verifier_gen_amd import seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "csrc")
HEADER = os.path.join(CSRC, "h2v_seed.hpp")


# ---- the rule once more, straight-line: one flat byte string per hash, levels in one loop, nothing shared with seed.py
def _b(x):
    return hashlib.blake2b(x, digest_size=32).digest()


def _straight(tag, form, inst, ci, proofs):
    n = len(proofs)
    level = []
    for i in range(n):
        msg = b"h2v-seed-leaf/1\0" + len(inst[i]).to_bytes(4, "little") + len(ci[i]).to_bytes(4, "little") + len(proofs[i]).to_bytes(4, "little")
        msg += bytes(4) + inst[i] + ci[i] + proofs[i]
        level.append(_b(msg))
    lv = 0
    while True:
        lv += 1
        up = []
        for j in range(0, len(level), 64):
            kids = level[j:j + 64]
            up.append(_b(b"h2v-seed-node/1\0" + lv.to_bytes(4, "little") + len(kids).to_bytes(4, "little") + (j // 64).to_bytes(8, "little") + b"".join(kids)))
        level = up
        if len(level) == 1:
            break
    return _b(b"h2v-seed-root/1\0" + form.to_bytes(4, "little") + bytes(4) + n.to_bytes(8, "little") + tag + level[0])


def kat_inputs(n):
    rng = random.Random(0x5eed0000 + n)
    tag = bytes(rng.randrange(256) for _ in range(32))
    inst = [bytes(rng.randrange(256) for _ in range(32 * (n % 3))) for _ in range(n)]
    ci = [bytes(rng.randrange(256) for _ in range(48 * (n % 2))) for _ in range(n)]
    proofs = [bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 31, 96, 127, 128, 129, 200]))) for _ in range(n)]
    return tag, inst, ci, proofs


# the rule is frozen: these are its answers on kat_inputs(n)
KATS = {1: "d64a8f76b78d1ae2cb0e35ad8d2062662597ba0d52d4916f0034ccb053a16323",
        65: "33186f086532a6ed7da4ae6f3009613404ab68958d3f2420567f6a2fdce8a75d",
        4097: "47df6d53a47a0bd813ff4d41344f1f51d83a229caa2967b6182448135314455b"}


@pytest.mark.parametrize("n", sorted(KATS))
def test_known_answers(n):
    tag, inst, ci, proofs = kat_inputs(n)
    got = seed.batch_seed(tag, seed.FORM_PROOFS, inst, ci, proofs)
    assert got == _straight(tag, 1, inst, ci, proofs)
    assert got.hex() == KATS[n]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 4096])
def test_model_against_the_straight_line_statement(n):
    rng = random.Random(n)
    tag = bytes(rng.randrange(256) for _ in range(32))
    inst = [rng.randbytes(64) for _ in range(n)]
    ci = [rng.randbytes(48) for _ in range(n)]
    proofs = [rng.randbytes(rng.randrange(0, 300)) for _ in range(n)]
    assert seed.batch_seed(tag, 1, inst, ci, proofs) == _straight(tag, 1, inst, ci, proofs)
    assert seed.batch_seed(tag, 1, None, None, proofs) == _straight(tag, 1, [b""] * n, [b""] * n, proofs)
    pairs = [rng.randbytes(96) for _ in range(n)]
    assert seed.pairs_seed(tag, b"".join(pairs)) == _straight(tag, 2, [b""] * n, [b""] * n, pairs)
    # the flat form cuts the same bytes
    off = [7]
    for p in proofs:
        off.append(off[-1] + len(p))
    flat = seed.batch_seed_flat(tag, bytes(7) + b"".join(proofs), off, b"".join(inst), b"".join(ci), n_pi=2, n_ci=1)
    assert flat == _straight(tag, 1, inst, ci, proofs)


def test_key_tag_and_level_counts():
    blob = bytes(range(200))
    assert seed.key_tag(blob) == _b(b"h2v-seed-key/1\0\0" + blob)
    assert seed.key_tag(blob) != seed.key_tag(blob[:-1] + b"\0")
    assert seed.level_counts(1) == [1] and seed.level_counts(64) == [1] and seed.level_counts(65) == [2, 1]
    assert seed.level_counts(4096) == [64, 1] and seed.level_counts(4097) == [65, 2, 1]
    assert seed.level_counts(262144) == [4096, 64, 1] and seed.level_counts(262145) == [4097, 65, 2, 1]
    assert seed.level_counts(1 << 22) == [65536, 1024, 16, 1]


def test_what_the_seed_binds():
    """one change at a time, each gives another seed"""
    n = 70
    rng = random.Random(9)
    tag = rng.randbytes(32)
    inst = [rng.randbytes(32) for _ in range(n)]
    ci = [rng.randbytes(48) for _ in range(n)]
    proofs = [rng.randbytes(100 + i) for i in range(n)]
    base = seed.batch_seed(tag, 1, inst, ci, proofs)
    seen = {base}

    def differs(t=tag, form=1, a=inst, c=ci, p=proofs):
        s = seed.batch_seed(t, form, a, c, p)
        assert s not in seen
        seen.add(s)

    def flip(rows, i, k):
        out = list(rows)
        out[i] = out[i][:k] + bytes([out[i][k] ^ 1]) + out[i][k + 1:]
        return out

    for i, k in ((0, 0), (63, 99), (64, 5), (69, 168)):
        differs(p=flip(proofs, i, k))                               # a byte of a proof
    differs(a=flip(inst, 64, 31))                                   # ... of an instance row
    differs(c=flip(ci, 1, 47))                                      # ... of a committed row
    differs(t=flip([tag], 0, 17)[0])                                # ... of the key tag
    differs(a=inst[:-1], c=ci[:-1], p=proofs[:-1])                  # n
    differs(a=inst + inst[:1], c=ci + ci[:1], p=proofs + proofs[:1])
    swap = list(range(n))
    swap[3], swap[4] = 4, 3
    differs(a=[inst[i] for i in swap], c=[ci[i] for i in swap], p=[proofs[i] for i in swap])      # the order of two proofs
    differs(form=2)                                                 # the form
    # a byte moved across the instance / proof boundary, the lengths adjusted: the hashed bytes behind the header are the same
    moved_i, moved_p = list(inst), list(proofs)
    moved_i[5], moved_p[5] = inst[5][:-1], inst[5][-1:] + b"" + ci[5] + proofs[5]
    moved_c = list(ci)
    moved_c[5] = b""
    assert moved_i[5] + moved_c[5] + moved_p[5] == inst[5] + ci[5] + proofs[5]
    differs(a=moved_i, c=moved_c, p=moved_p)
    # ... and across the proof / next proof boundary
    moved_p = list(proofs)
    moved_p[5], moved_p[6] = proofs[5][:-1], proofs[5][-1:] + proofs[6]
    differs(p=moved_p)


# ---- the host-only layout header
SIZES = list(range(1, 201)) + [4095, 4096, 4097, 262144, 262145, 1 << 22]


def test_layout_program_under_sanitizers(tmp_path):
    """tests/cpp/h2v_seed_layout.cpp: its own main, includes only h2v_seed.hpp; node counts of every level = the model's (passed
    in), levels disjoint, gapless and inside the extent, every level chain ends in one node"""
    out = str(tmp_path / "h2v_seed_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "h2v_seed_layout.cpp"), "-o", out])
    args = ["%d:%s" % (n, ",".join(str(c) for c in seed.level_counts(n))) for n in SIZES]
    r = subprocess.run([out] + args, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-3000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2] == "checked %d sizes" % len(SIZES) and not [ln for ln in lines if ln.startswith("FAIL")]
    # a wrong model count is noticed (the program really compares)
    bad = subprocess.run([out, "65:3,1"], capture_output=True, text=True)
    assert bad.returncode == 1 and "FAIL" in bad.stdout


def test_layout_header_has_no_hip_in_it():
    with open(HEADER) as f:
        text = f.read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "__global__" not in code and "__device__" not in code
    for inc in re.findall(r"#include\s*(\S+)", code):
        assert inc in ("<stddef.h>", "<stdint.h>", "<string.h>"), inc
    with open(os.path.join(ROOT, "tests", "cpp", "h2v_seed_layout.cpp")) as f:
        incs = re.findall(r'#include\s*"([^"]+)"', f.read())
    assert incs == ["../../plutus_halo2_verifier_gen_amd/csrc/h2v_seed.hpp"]


# ---- header and binding
def test_header_and_binding():
    from plutus_halo2_verifier_gen_amd import api, backend
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+H2V_RLC_SEED_TRANSCRIPT\s+(\d+)u", h)
    assert m and int(m.group(1)) == 32 == backend.RLC_SEED_TRANSCRIPT
    assert not re.search(r"#define\s+H2V_RLC_\w+\s+8u", h)                     # bit 8 stays unassigned
    for name in ("h2v_workspace_seed_used", "h2v_probe_batch_seed", "h2v_plan_key_tag"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in backend.EXPORTS, name
    L = backend.lib()
    assert len(L.h2v_workspace_seed_used.argtypes) == 3 and len(L.h2v_probe_batch_seed.argtypes) == 7 and len(L.h2v_plan_key_tag.argtypes) == 2
    # seed_source sits at the offset of `reserved`, the last word of a 48-byte struct: the word keeps its name in the struct (the
    # struct's field names are pinned) and the header and the binding both read it as the seed source
    m = re.search(r"typedef struct \{([^}]*)\}\s*h2v_aggregate_info;", h)
    fields = re.findall(r"(uint8_t|uint32_t)\s+(\w+)(\[32\])?;", m.group(1))
    assert [nm for _, nm, _ in fields] == ["seed_used", "chunk", "n_chunks", "msm_terms", "reserved"]
    assert re.search(r"#define\s+H2V_AGGREGATE_SEED_SOURCE\(info\)\s+\(\(info\)->reserved\)", h)
    assert backend.AggregateInfo.reserved.offset == 44 and C.sizeof(backend.AggregateInfo) == 48
    info = backend.AggregateInfo()
    assert info.seed_source == 0
    C.memmove(C.addressof(info) + 44, C.byref(C.c_uint32(1)), 4)
    assert info.seed_source == 1 and bytes(info)[:44] == bytes(44)
    opts = backend._rlc_opts(None, derive_seed=True)
    assert opts.flags == 32 and bytes(opts.seed) == bytes(32)
    assert backend._rlc_opts(bytes(32), derive_seed=True).flags == 33          # (the library refuses it: H2V_E_ARG)
    # argument rules that come back before any device call: the flag beside a given seed, and the flag in the mixed aggregate call
    pair = C.create_string_buffer(96)
    inc = (C.c_uint8 * 4)()
    mb = backend.MixedBatch(0, None, None, None, None, None)
    plans = (C.c_void_p * 1)()
    flag = backend.RlcOpts((C.c_uint8 * 32)(), backend.RLC_SEED_TRANSCRIPT)
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, inc, None, None, C.byref(flag), None) == -1
    assert L.h2v_aggregate_mixed_device(plans, 0, C.byref(mb), C.addressof(pair), None, None, None, None, C.byref(flag), None) == -1
    assert L.h2v_plan_key_tag(None, pair) == -1 and L.h2v_workspace_seed_used(None, 0, pair) == -1
    # the Python layers
    import inspect
    for fn in (api.Verifier.verify_batch, api.Verifier.check_pairs, api.Verifier.aggregate_batch, api.Aggregator.__init__,
               backend.DevicePlan.verify_batch_rlc, backend.DevicePlan.check_pairs_rlc, backend.DevicePlan.aggregate_batch, backend.DevicePlan.submit):
        assert "derive_seed" in inspect.signature(fn).parameters, fn
    assert callable(backend.Workspace.seed_used) and callable(backend.probe_batch_seed)
    agg = api.Aggregator(None, derive_seed=True)
    with pytest.raises(ValueError, match="single-key"):
        agg.push_mixed([], [], [])
