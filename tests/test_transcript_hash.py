"""The transcript hash as a property of the verifying key (vk.transcript_hash): what can be said without a GPU.  The
big-integer model of the keyed blake2b-512 flavour against hashlib, the blobs of keys without the field against digests
recorded before the field existed (tests/golden/plan_digests.json), plan.py against the C++ compiler for flavoured keys, the
loader's refusals, and the agreement of header, Python binding and C++ wrapper on the two new exports.  The GPU legs are in
tests/test_transcript_hash_gpu.py."""
import ctypes as C
import hashlib
import json
import os
import re
import struct

import pytest

from plutus_halo2_verifier_gen_amd import backend, bls12_381 as bls, plan as PL, synth, vk as V
from tests.plan_loading import plan_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bls.R
KEYS = [b"", b"\x5a", V.DEFAULT_BLAKE2B_512_KEY, bytes(range(101, 165))]   # 0, 1, 31 and 64 bytes
E_ARG, E_PLAN, E_DEVICE = -1, -2, -3


def flavoured(vk, key=None):
    return V.with_transcript_hash(vk, "blake2b-512", key)


def _squeezes_by_hashlib(plan, proof, instances, committed, key):
    """The challenges of the plan's SQUEEZE records from a direct hashlib replay of the byte stream the program absorbs:
    one keyed blake2b-512 state, update(0x00) then the digest of a copy per squeeze, from_uniform_bytes of the 64 bytes."""
    st = hashlib.blake2b(key=key, digest_size=64)
    regs = {}
    out = []
    for op, d, a, c in plan.instrs:
        if op == PL.OP_END:
            break
        if op == PL.OP_LOAD_INSTANCE:
            regs[d] = instances[a] % R
        elif op == PL.OP_ABSORB_REG:
            st.update(b"\x01" + regs[a].to_bytes(32, "little"))
        elif op == PL.OP_ABSORB_CI:
            st.update(b"\x01" + committed)
        elif op == PL.OP_READ_POINT:
            off = a | (c << 16)
            st.update(b"\x01" + proof[off:off + 48])
        elif op == PL.OP_READ_SCALAR:
            off = a | (c << 16)
            st.update(b"\x01" + proof[off:off + 32])
            regs[d] = int.from_bytes(proof[off:off + 32], "little") % R
        elif op == PL.OP_SQUEEZE:
            st.update(b"\x00")
            dg = st.copy().digest()
            out.append((d, (int.from_bytes(dg[:32], "little") + (int.from_bytes(dg[32:], "little") << 256)) % R))
        elif op == PL.OP_CONST:
            regs[d] = plan.consts[a]
        # (simple_mul absorbs constants and public inputs only: no arithmetic result is ever hashed)
    return out


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "key%d" % len(k))
def test_run_plan_models_the_keyed_flavour(key):
    vk, td = V.simple_mul_vk()
    fv = flavoured(vk, key)
    pl = PL.compile_plan(fv, lanes=1)     # one record per bundle: every squeeze's register is still unwritten when it is compared
    assert pl.transcript_kind == PL.TR_BLAKE2B_512 and pl.transcript_key == key
    batch = synth.forge_batch(fv, td, 1, seed=3, plan=pl, workers=1)
    proof, inst = batch.proof(0), batch.instance_ints(0, fv.n_public_inputs)
    want = _squeezes_by_hashlib(pl, proof, inst, None, key)
    assert len(want) == pl.n_squeezes >= 5
    # run_plan's registers, read right after each squeeze (later instructions may reuse a register): replay prefix by prefix
    seen = []
    for k, (reg, val) in enumerate(want):
        upto = [i for i, ins in enumerate(pl.instrs) if ins[0] == PL.OP_SQUEEZE][k] + 1
        cut = PL.Plan(**{**pl.__dict__, "instrs": pl.instrs[:upto] + [(PL.OP_END, 0, 0, 0)]})
        _s, regs, st = PL.run_plan(cut, proof, inst, None)
        assert st is None and regs[reg] == val, (k, reg)
        seen.append(regs[reg])
    # the same proof bytes under the Cardano plan: already the first challenge differs
    cpl = PL.compile_plan(vk, lanes=1)
    assert [i[0] for i in cpl.instrs] == [i[0] for i in pl.instrs]
    first = [i for i, ins in enumerate(cpl.instrs) if ins[0] == PL.OP_SQUEEZE][0]
    ccut = PL.Plan(**{**cpl.__dict__, "instrs": cpl.instrs[:first + 1] + [(PL.OP_END, 0, 0, 0)]})
    _s, cregs, _st = PL.run_plan(ccut, proof, inst, None)
    assert cregs[cpl.instrs[first][1]] != seen[0]
    # and the forged proof satisfies its own plan only
    assert PL.run_plan(pl, proof, inst, None)[2] is None


def test_keys_without_the_field_give_the_blobs_recorded_before_it_existed():
    """tests/golden/plan_digests.json: sha256 of compile_plan(vk).to_bytes() of every built-in key, recorded on the commit
    before the transcript hash became a field.  Both compilers still produce them - field absent, and field naming the
    Cardano flavour explicitly."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_digests.json")) as f:
        gold = json.load(f)
    assert set(gold["BUILDERS"]) == set(V.BUILDERS) and set(gold["WIDE_BUILDERS"]) == set(V.WIDE_BUILDERS)
    for group, table in (("BUILDERS", V.BUILDERS), ("WIDE_BUILDERS", V.WIDE_BUILDERS)):
        for name, build in table.items():
            vk, _ = build()
            assert vk.transcript_hash is None
            explicit = V.with_transcript_hash(vk, "cardano-blake2b-256")
            for key in (vk, explicit):
                py = PL.compile_plan(key).to_bytes()
                assert hashlib.sha256(py).hexdigest() == gold[group][name], (name, key.transcript_hash)
                assert hashlib.sha256(backend.plan_compile(key.to_json())).hexdigest() == gold[group][name], (name, key.transcript_hash)
            w = struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, py, 8)
            assert w[0] == PL.PLAN_VERSION == 4 and w[40:46] == (0,) * 6
    # a description whose JSON has no such member at all (what an exporter written before the field produces)
    d = json.loads(V.simple_mul_vk()[0].to_json())
    del d["transcript_hash"]
    assert hashlib.sha256(backend.plan_compile(json.dumps(d))).hexdigest() == gold["BUILDERS"]["simple_mul"]
    assert V.VerifyingKey.from_json(json.dumps(d)).transcript_hash is None


@pytest.mark.parametrize("name", ["simple_mul", "lookup_table", "trashcan_mix", "phased", "ivc"])
def test_cpp_compiler_matches_plan_py_on_flavoured_keys(name):
    vk, _ = V.BUILDERS[name]()
    base = PL.compile_plan(vk).to_bytes()
    for key in [None] + KEYS:
        fv = flavoured(vk, key)
        want = PL.compile_plan(fv).to_bytes()
        got = backend.plan_compile(fv.to_json())
        assert got == want, (name, key)
        w = struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, want, 8)
        k = V.DEFAULT_BLAKE2B_512_KEY if key is None else key
        assert w[0] == PL.PLAN_VERSION_FLAVOURED == 5 and w[PL.HW_TR_KIND] == 1 and w[PL.HW_TR_KEY_LEN] == len(k)
        assert want[w[PL.HW_TR_KEY_OFF]:w[PL.HW_TR_KEY_OFF] + len(k)] == k and (k == b"") == (w[PL.HW_TR_KEY_OFF] == 0)
        # nothing but the header words and the key section differs from the Cardano blob: the program is flavour-blind
        hdr = 8 + 4 * PL.PLAN_HDR_WORDS
        assert want[hdr:len(base)] == base[hdr:] and len(want) == len(base) + (len(k) + 15) // 16 * 16


def _loader():
    backend.lib()                          # (built and loadable)
    load_plan = plan_loader()
    return lambda blob: load_plan(blob)[0]


def test_loader_takes_version_5_and_refuses_what_it_cannot_replay():
    """The blob is validated on the host before any device work, so without a GPU a good plan comes back as H2V_E_DEVICE
    and a bad one as H2V_E_PLAN."""
    load = _loader()
    ok_rc = 0 if backend.device_count() >= 1 else E_DEVICE
    vk, _ = V.simple_mul_vk()
    blob = PL.compile_plan(flavoured(vk)).to_bytes()
    assert struct.unpack_from("<I", blob, 8)[0] == 5
    assert load(blob) == ok_rc
    assert load(PL.compile_plan(flavoured(vk, b"")).to_bytes()) == ok_rc
    assert load(PL.compile_plan(flavoured(vk, bytes(64))).to_bytes()) == ok_rc

    def patched(**words):
        m = bytearray(blob)
        for k, v in words.items():
            struct.pack_into("<I", m, 8 + 4 * {"version": 0, "kind": PL.HW_TR_KIND, "off": PL.HW_TR_KEY_OFF, "len": PL.HW_TR_KEY_LEN}[k], v)
        return m

    assert load(patched(kind=2)) == E_PLAN                      # an unknown kind
    assert load(patched(kind=0xFFFFFFFF)) == E_PLAN
    assert load(patched(len=65)) == E_PLAN                      # a key longer than blake2b takes
    assert load(patched(off=len(blob) - 16)) == E_PLAN          # 31 bytes from 16 before the end: past the blob
    assert load(patched(off=len(blob))) == E_PLAN
    assert load(patched(off=0xFFFFFFF0)) == E_PLAN
    assert load(patched(off=0)) == E_PLAN                       # a key inside the header
    assert load(patched(version=4)) == E_PLAN                   # version 4 knows no kind: refused, never replayed as Cardano
    assert load(patched(version=6)) == E_PLAN
    assert load(patched(kind=0)) == E_PLAN                      # the Cardano flavour is unkeyed
    assert load(patched(kind=0, off=0, len=0)) == ok_rc         # (version 5 naming the Cardano flavour: harmless)


def test_validate_refuses_the_same_and_json_keeps_the_field():
    vk, _ = V.simple_mul_vk()
    d = json.loads(vk.to_json())

    def desc(th):
        return json.dumps({**d, "transcript_hash": th})

    for th, why in [({"kind": "poseidon"}, "unknown kind"), ({"kind": "blake2b-512", "key_hex": "00" * 65}, "at most 64"),
                    ({"kind": "blake2b-512", "key_hex": "0g"}, "hex"), ({"kind": "blake2b-512", "key_hex": "abc"}, "hex"),
                    ({"kind": "cardano-blake2b-256", "key_hex": "00"}, "unkeyed"), ({"key_hex": "00"}, "object"),
                    ({"kind": "blake2b-512", "salt": "00"}, "object"), ("blake2b-512", "object")]:
        with pytest.raises(V.VKError, match=why):
            V.VerifyingKey.from_json(desc(th))
        with pytest.raises(backend.H2VError, match=why):     # the C++ compiler refuses it with the same reason
            backend.plan_compile(desc(th))
    for key in [None] + KEYS:
        fv = flavoured(vk, key)
        V.validate(fv)
        back = V.VerifyingKey.from_json(fv.to_json())
        assert back == fv and back.transcript_hash == fv.transcript_hash
        assert V.transcript_kind(back) == (1, V.DEFAULT_BLAKE2B_512_KEY if key is None else key)
        assert json.loads(fv.to_json())["transcript_hash"]["kind"] == "blake2b-512"
    assert V.transcript_kind(vk) == (0, b"") and len(V.DEFAULT_BLAKE2B_512_KEY) == 31
    # the schema document names the field and both kinds
    with open(os.path.join(ROOT, "docs", "vk_schema.json")) as f:
        prop = json.load(f)["properties"]["transcript_hash"]
    assert set(prop["properties"]["kind"]["enum"]) == set(V.TRANSCRIPT_KINDS)


def test_verify_files_switch_overrides_the_key_file():
    from plutus_halo2_verifier_gen_amd import verify_files as VF
    vk, _ = V.simple_mul_vk()
    assert V.transcript_kind(VF.with_transcript_spec(vk, "blake2b-512")) == (1, V.DEFAULT_BLAKE2B_512_KEY)
    assert V.transcript_kind(VF.with_transcript_spec(vk, "blake2b-512:")) == (1, b"")
    assert V.transcript_kind(VF.with_transcript_spec(vk, "blake2b-512:0aff")) == (1, b"\x0a\xff")
    assert V.transcript_kind(VF.with_transcript_spec(flavoured(vk), "cardano-blake2b-256")) == (0, b"")
    with pytest.raises(V.VKError):
        VF.with_transcript_spec(vk, "sha3")


def test_api_tag_mismatch_is_misuse_before_any_device_work():
    """No GPU here or none needed: the tag is held against the key description before a plan is compiled or loaded."""
    from plutus_halo2_verifier_gen_amd import api
    vk, _ = V.simple_mul_vk()
    before = dict(api._VERIFIERS)
    t = api.CircuitTranscript.init_from_bytes(bytes(16))
    assert t.hash == api.CARDANO_FRIENDLY_BLAKE2B
    with pytest.raises(ValueError, match="transcript hash mismatch"):
        api.prepare(flavoured(vk), [[]], [[[1, 2, 3]]], t)
    with pytest.raises(ValueError, match="transcript hash mismatch"):
        api.prepare(vk, [[]], [[[1, 2, 3]]], api.CircuitTranscript.init_from_bytes(bytes(16), hash=api.BLAKE2B_512))
    with pytest.raises(ValueError, match="unknown transcript hash"):
        api.CircuitTranscript.init_from_bytes(bytes(16), hash="poseidon")
    assert api._VERIFIERS == before


def _arg_count(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, name
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


def test_header_binding_and_cpp_wrapper_agree_on_the_new_exports():
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "h2v.hpp")) as f:
        hpp = f.read()
    assert re.search(r"\bint\s+h2v_plan_transcript\s*\(\s*const h2v_plan \*plan,\s*uint32_t \*kind,\s*uint8_t key_out\[64\],\s*uint32_t \*key_len\)", h)
    assert re.search(r"\bint\s+h2v_probe_blake2b_ex\s*\(\s*int device,\s*uint32_t n,\s*uint32_t len,\s*const uint8_t \*msgs,\s*uint32_t digest_len", h)
    kinds = {name: int(re.search(r"#define\s+%s\s+(\d+)u" % name, h).group(1))
             for name in ("H2V_TRANSCRIPT_CARDANO_BLAKE2B_256", "H2V_TRANSCRIPT_BLAKE2B_512")}
    assert kinds == {"H2V_TRANSCRIPT_CARDANO_BLAKE2B_256": 0, "H2V_TRANSCRIPT_BLAKE2B_512": 1}
    assert (backend.TRANSCRIPT_CARDANO_BLAKE2B_256, backend.TRANSCRIPT_BLAKE2B_512) == (0, 1)
    assert {backend.TRANSCRIPT_NAMES[v]: v for v in (0, 1)} == V.TRANSCRIPT_KINDS
    assert (PL.TR_CARDANO_BLAKE2B_256, PL.TR_BLAKE2B_512) == (0, 1)
    assert "h2v_plan_transcript" in backend.EXPORTS and "h2v_probe_blake2b_ex" in backend.EXPORTS
    L = backend.lib()
    assert len(L.h2v_plan_transcript.argtypes) == _arg_count(h, "h2v_plan_transcript") == 4
    assert len(L.h2v_probe_blake2b_ex.argtypes) == _arg_count(h, "h2v_probe_blake2b_ex") == 8
    assert L.h2v_plan_transcript(None, None, None, None) == E_ARG
    # the C++ wrapper reads the plan's kind through the same export and carries one tag type per kind
    assert "h2v_plan_transcript(p_" in hpp
    assert re.search(r"struct CardanoFriendlyBlake2b \{ static constexpr uint32_t kind = H2V_TRANSCRIPT_CARDANO_BLAKE2B_256; \}", hpp)
    assert re.search(r"struct Blake2b512 \{ static constexpr uint32_t kind = H2V_TRANSCRIPT_BLAKE2B_512; \}", hpp)
    assert "using CircuitTranscript = Transcript<CardanoFriendlyBlake2b>;" in hpp
    assert "vk.transcript_kind() != H::kind" in hpp
