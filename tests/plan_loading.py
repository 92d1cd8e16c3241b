"""What the plan-loader tests share: ONE ctypes prototype of h2v_plan_load, and the deterministic corpus of mutated plan blobs
whose verdicts tests/golden/plan_load_verdicts.txt records (tests/test_plan_blob.py holds both the library and the stand-alone
parser program to that file).  No test in here: an ordinary module."""
import ctypes
import os
import random
import struct

from plutus_halo2_verifier_gen_amd import plan as PL
from plutus_halo2_verifier_gen_amd import vk as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "plutus_halo2_verifier_gen_amd", "libh2v_hip.so")
E_ARG, E_PLAN, E_DEVICE, E_LIMIT = -1, -2, -3, -4
# plan header words (csrc/h2v_plan.h)
HW_N_INSTR, HW_N_POINTS, HW_N_TERMS, HW_N_TRACE, HW_OFF_INSTR, HW_OFF_POINTS, HW_OFF_TERMS, HW_OFF_TRACE = 5, 7, 9, 10, 14, 16, 18, 21
HW_N_REGS, HW_TOTAL_LEN, HW_N_MAIN_TERMS = 4, 22, 26
HW_VM_LANES, HW_VM2_LANES, HW_VM2_N_INSTR, HW_VM2_OFF_INSTR = 35, 36, 38, 39


def plan_loader(lib_path=LIB):
    """load(blob) -> (return code of h2v_plan_load on device 0, h2v_last_error() after it); a plan that loads is freed again.
    A handle of its own, so that the binding's prototypes (backend.lib()) stay as they are."""
    L = ctypes.CDLL(lib_path)
    L.h2v_plan_load.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.h2v_plan_load.restype = ctypes.c_int
    L.h2v_plan_free.argtypes = [ctypes.c_void_p]
    L.h2v_plan_free.restype = None
    L.h2v_last_error.restype = ctypes.c_char_p

    def load(blob):
        h = ctypes.c_void_p()
        rc = L.h2v_plan_load(bytes(blob), len(blob), 0, ctypes.byref(h))
        if rc == 0:
            L.h2v_plan_free(h)
        return rc, (L.h2v_last_error() or b"").decode()
    return load


# ----------------------------------------------------------------------------------------------------------- the corpus
def corpus_plans():
    """name -> blob: simple_mul, ivc, simple_mul under the keyed blake2b-512 transcript, one wide key, 4096 bytes of noise"""
    simple = V.simple_mul_vk()[0]
    return {
        "simple_mul": PL.compile_plan(simple).to_bytes(),
        "ivc": PL.compile_plan(V.ivc_vk()[0]).to_bytes(),
        "keyed": PL.compile_plan(V.with_transcript_hash(simple, "blake2b-512")).to_bytes(),
        "composite": PL.compile_plan(V.composite_vk()[0]).to_bytes(),
        "noise": bytes(random.Random(4096).randrange(256) for _ in range(4096)),
        # sums at and above H2V_MAX_MSM_TERMS (tests/test_wide_keys.py)
        "terms4096": with_terms(PL.compile_plan(simple).to_bytes(), 4096, 4096),
        "terms4097": with_terms(PL.compile_plan(simple).to_bytes(), 4097, 4097),
        "ivc_fold4097": _ivc_fold_over(),
    }


def with_terms(blob: bytes, n_terms: int, n_main: int) -> bytes:
    """The plan with its MSM term table replaced by one of n_terms VK-base terms (appended at the end of the blob)."""
    w = list(struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, blob, 8))
    body = bytearray(blob)
    while len(body) % 16:
        body.append(0)
    off = len(body)
    body += struct.pack("<II", 1, 0) * n_terms             # (H2V_TERM_VK_BASE, base 0)
    w[HW_OFF_TERMS], w[HW_N_TERMS], w[HW_N_MAIN_TERMS], w[HW_TOTAL_LEN] = off, n_terms, n_main, len(body)
    struct.pack_into("<%dI" % PL.PLAN_HDR_WORDS, body, 8, *w)
    return bytes(body)


def _ivc_fold_over():
    blob = PL.compile_plan(V.ivc_wide_vk()[0]).to_bytes()
    n_main = struct.unpack_from("<I", blob, 8 + 4 * HW_N_MAIN_TERMS)[0]
    return with_terms(blob, n_main + 1 + 4097, n_main)


def corpus(plans):
    """[(case id, plan name, cut or None, [(offset, bytes), ...])]: the blob of the case is the named plan with the patches applied
    and then cut to `cut` bytes.  Fixed seeds: the list is the same on every machine and in every run."""
    cases = []

    def add(cid, name, patches=(), cut=None):
        cases.append((cid, name, cut, list(patches)))

    for name in ("simple_mul", "ivc", "keyed", "composite"):
        blob = plans[name]
        rng = random.Random("plan-load-corpus/" + name)
        w = list(struct.unpack_from("<%dI" % PL.PLAN_HDR_WORDS, blob, 8))
        add("%s:asis" % name, name)
        # every header word set to hostile values (the keyed plan is simple_mul's but for the version and the transcript words)
        words = range(PL.PLAN_HDR_WORDS) if name != "keyed" else [0] + list(range(PL.HW_TR_KIND, PL.PLAN_HDR_WORDS))
        for k in words:
            seen = {w[k]}
            for val in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF, w[k] - 1, w[k] + 1, w[k] + 16):
                val &= 0xFFFFFFFF
                if val not in seen:
                    seen.add(val)
                    add("%s:hw%d=%#x" % (name, k, val), name, [(8 + 4 * k, struct.pack("<I", val))])
        # single-byte hits in the instruction streams, the wide one included
        n_hits = 100 if name in ("simple_mul", "ivc") else 40
        streams = [("instr", w[HW_OFF_INSTR], w[HW_N_INSTR])]
        if w[HW_VM2_LANES]:
            streams.append(("wide", w[HW_VM2_OFF_INSTR], w[HW_VM2_N_INSTR]))
        for label, off, n in streams:
            for _ in range(n_hits):
                pos = off + 8 * rng.randrange(n) + rng.randrange(8)
                add("%s:%s@%d=%#x" % (name, label, pos, (v := rng.randrange(256))), name, [(pos, bytes([v]))])
        # term, point and trace tables
        for label, sec_word, count_word, rec in (("term", HW_OFF_TERMS, HW_N_TERMS, 8), ("point", HW_OFF_POINTS, HW_N_POINTS, 4),
                                                 ("trace", HW_OFF_TRACE, HW_N_TRACE, 8)):
            for _ in range(40 if name != "keyed" else 15):
                if w[count_word] == 0:
                    break
                pos = w[sec_word] + rec * rng.randrange(w[count_word]) + rng.randrange(rec)
                add("%s:%s@%d=%#x" % (name, label, pos, (v := rng.randrange(256))), name, [(pos, bytes([v]))])
        for cut in (0, 7, 8, 100, 8 + 4 * PL.PLAN_HDR_WORDS - 1, 8 + 4 * PL.PLAN_HDR_WORDS, len(blob) // 2, len(blob) - 1):
            add("%s:cut=%d" % (name, cut), name, cut=cut)
    for name in ("noise", "terms4096", "terms4097", "ivc_fold4097"):
        add("%s:asis" % name, name)

    # the bundle discipline (test_plan_loader_rejects_broken_bundles)
    pl = PL.compile_plan(V.simple_mul_vk()[0])
    lanes, recs, off_instr = pl.vm_lanes, pl.instrs, struct.unpack_from("<I", plans["simple_mul"], 8 + 4 * HW_OFF_INSTR)[0]
    k = next(s for s in range(0, len(recs), lanes) if recs[s][0] == PL.OP_MUL and recs[s + 1][0] in (PL.OP_MUL, PL.OP_ADD, PL.OP_SUB))
    t = next(s for s in range(0, len(recs), lanes) if recs[s][0] == PL.OP_SQUEEZE)
    (_op0, d0, _a0, _b0), (op1, d1, a1, b1) = recs[k], recs[k + 1]

    def rec(at, *fields):
        return [(off_instr + 8 * at, struct.pack("<BBHHH", fields[0], 0, *fields[1:]))]
    add("bundle:reads-what-lane0-writes", "simple_mul", rec(k + 1, op1, d1, d0, b1))
    add("bundle:two-lanes-write-one", "simple_mul", rec(k + 1, op1, d0, a1, b1))
    add("bundle:squeeze-shares", "simple_mul", rec(t + 1, PL.OP_CONST, 0, 0, 0))
    add("bundle:squeeze-off-lane0", "simple_mul", rec(k + 1, PL.OP_SQUEEZE, d1, 0, 0))
    add("bundle:end-early", "simple_mul", rec(t, PL.OP_END, 0, 0, 0))
    add("bundle:no-end", "simple_mul", rec(len(recs) - lanes, PL.OP_NOP, 0, 0, 0))
    add("bundle:registers-past-lds", "simple_mul", [(8 + 4 * HW_N_REGS, struct.pack("<I", 65535))])
    add("bundle:unknown-opcode", "simple_mul", rec(k, PL.OP_NOP + 1, 0, 0, 0))
    for bad in (3, 0, 64, 128):
        add("bundle:lanes=%d" % bad, "simple_mul", [(8 + 4 * HW_VM_LANES, struct.pack("<I", bad))])
        add("bundle:wide-lanes=%d" % bad, "simple_mul", [(8 + 4 * HW_VM2_LANES, struct.pack("<I", bad))])

    # the transcript words (test_loader_takes_version_5_and_refuses_what_it_cannot_replay)
    blob = plans["keyed"]
    index = {"version": 0, "kind": PL.HW_TR_KIND, "off": PL.HW_TR_KEY_OFF, "len": PL.HW_TR_KEY_LEN}
    for words in ({"kind": 2}, {"kind": 0xFFFFFFFF}, {"len": 65}, {"len": 64}, {"len": 0}, {"off": len(blob) - 16}, {"off": len(blob)},
                  {"off": 0xFFFFFFF0}, {"off": 0}, {"off": 8 + 4 * PL.PLAN_HDR_WORDS}, {"version": 4}, {"version": 6}, {"kind": 0},
                  {"kind": 0, "off": 0, "len": 0}, {"version": 4, "kind": 0, "off": 0, "len": 0}, {"off": 0, "len": 0}):
        add("trkey:" + ",".join("%s=%#x" % kv for kv in words.items()), "keyed",
            [(8 + 4 * index[k], struct.pack("<I", v)) for k, v in words.items()])
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def case_blob(plans, case):
    _cid, name, cut, patches = case
    m = bytearray(plans[name])
    for off, data in patches:
        m[off:off + len(data)] = data
    return bytes(m if cut is None else m[:cut])


def verdict_line(cid, rc, msg):
    """One line of tests/golden/plan_load_verdicts.txt.  A blob that passes validation is `valid` whatever the machine: the load
    then ends as H2V_E_DEVICE where there is no GPU and as 0 where there is one."""
    return "%s\tvalid" % cid if rc in (0, E_DEVICE) else "%s\t%d\t%s" % (cid, rc, msg)
