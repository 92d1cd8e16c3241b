"""The derived seed of the mixed-key calls (H2V_RLC_SEED_KEYED, include/h2v.h; DESIGN.md section 17.1: form 3, keyed leaves), what
can be said without a GPU: plutus_halo2_verifier_gen_amd/seed.py against a second statement of the rule (tests/keyed_seed_cases.py)
and against three committed seeds; what the seed binds and what it does not; the flag in the bindings; the argument rules that
come back before any device call.  On the code before the flag existed seed.mixed_seed does not exist and 64 is an unknown flag."""
import ctypes as C
import inspect
import os
import re

import pytest

from plutus_halo2_verifier_gen_amd import seed
from tests import keyed_seed_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# computed once from BOTH statements (they agreed) and committed: n = 1; n = 65 over 3 keys; n = 4097 over 2 keys
KNOWN = {
    "n1": "feaed2681a9ee84de442949732db381f370fd13b6f97a279f72521457caf98e3",
    "n65": "d83e428cb77810408036c63a35fb66d8fdd7aac6d497221cce45d4c4b825e407",
    "n4097": "7008b9f30eba70f7d66abfe4f9dee8d2c0ab343178fc5b9326d7a4fe8845cb32",
}


def _known_case(name):
    if name == "n1":
        return K.tags(1, "known"), K.Case([(1, 1)], [0], [200], 0, "known-1")
    if name == "n65":
        return K.tags(4, "known"), K.case3(65, 0, "known")
    return K.tags(2, "known"), K.Case([(1, 0), (0, 1)], [(i * i + i // 3) % 2 for i in range(4097)], [K.LENS[i % len(K.LENS)] for i in range(4097)], 0, "known-4097")


def _both(tags, c):
    a = seed.mixed_seed(tags, c.plan_of, c.inst, c.ci, c.proof)
    assert a == K.restated_seed(tags, c.plan_of, c.inst, c.ci, c.proof)
    assert a == seed.mixed_seed_flat(tags, c.shapes, c.plan_of, c.proofs, c.off, c.instances, c.committed)
    return a


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    tags, c = _known_case(name)
    got = _both(tags, c)
    print(name, got.hex())
    assert got.hex() == KNOWN[name]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("first_off", [0, 3])
def test_model_against_the_restatement(n, first_off):
    _both(K.tags(4), K.case3(n, first_off))


def _seed(tags, c):
    return seed.mixed_seed(tags, c.plan_of, c.inst, c.ci, c.proof)


def _flip(b: bytes, k: int = 0) -> bytes:
    return b[:k] + bytes([b[k] ^ 1]) + b[k + 1:]


def test_what_the_seed_binds():
    tags = K.tags(4)
    base = K.case3(70)
    s0 = _seed(tags, base)
    seen = {s0}

    def differs(c, t=tags):
        s = _seed(t, c)
        assert s not in seen
        seen.add(s)

    # a byte of a proof, of an instance row, of a committed row (position 4 is of plan 1: it has all three)
    for field in ("proof", "inst", "ci"):
        c = K.case3(70)
        assert getattr(c, field)[4]
        getattr(c, field)[4] = _flip(getattr(c, field)[4], len(getattr(c, field)[4]) - 1)
        differs(c)
    # one proof's key tag: position 5 (plan 2) is handed to plan 0's tag... by a relisting that gives plan 2 another tag
    t2 = list(tags)
    t2[2] = K.tags(1, "other")[0]
    differs(base, t2)
    # two positions of different keys swapped: positions 6 (plan 0) and 8 (plan 2) with everything that is theirs
    c = K.case3(70)
    for f in (c.plan_of, c.proof, c.inst, c.ci):
        f[6], f[8] = f[8], f[6]
    differs(c)
    # n: the same leaves but the last
    c = K.case3(70)
    for f in (c.plan_of, c.proof, c.inst, c.ci):
        f.pop()
    differs(c)
    # a byte moved across a section boundary with the lengths adjusted: instance -> committed, committed -> proof, instance -> proof
    c = K.case3(70)
    c.inst[4], c.ci[4] = c.inst[4][:-1], c.inst[4][-1:] + c.ci[4]
    differs(c)
    c = K.case3(70)
    c.ci[4], c.proof[4] = c.ci[4][:-1], c.ci[4][-1:] + c.proof[4]
    differs(c)
    c = K.case3(70)
    assert not c.ci[5]
    c.inst[5], c.proof[5] = c.inst[5][:-1], c.inst[5][-1:] + c.proof[5]
    differs(c)
    # the same bytes under ONE key tag for every position: which key a position has is bound
    differs(base, [tags[0]] * 4)


def test_what_the_seed_does_not_bind():
    tags = K.tags(4)
    c = K.case3(70)
    s0 = _seed(tags, c)
    # the plans listed in another order, plan_of renumbered
    order = [2, 3, 0, 1]                                   # new list position -> old plan
    new_of = {old: new for new, old in enumerate(order)}
    assert seed.mixed_seed([tags[o] for o in order], [new_of[k] for k in c.plan_of], c.inst, c.ci, c.proof) == s0
    assert seed.mixed_seed_flat([tags[o] for o in order], [c.shapes[o] for o in order], [new_of[k] for k in c.plan_of], c.proofs, c.off,
                                c.instances, c.committed) == s0
    # one more listed plan without a proof, and the listed-but-unused fourth plan dropped
    assert seed.mixed_seed(tags + K.tags(1, "extra"), c.plan_of, c.inst, c.ci, c.proof) == s0
    assert seed.mixed_seed(tags[:3], c.plan_of, c.inst, c.ci, c.proof) == s0


def test_one_plan_mixed_is_not_form_one():
    tag = K.tags(1)[0]
    c = K.Case([(2, 1)], [0] * 5, [300] * 5, 0, "one-plan")
    assert seed.FORM_MIXED == 3
    assert _seed([tag], c) != seed.batch_seed(tag, seed.FORM_PROOFS, c.inst, c.ci, c.proof)
    # ... and a keyed leaf is not a form 1 leaf of the same sections
    assert seed.mixed_leaf(tag, c.inst[0], c.ci[0], c.proof[0]) != seed.leaf(c.inst[0], c.ci[0], c.proof[0])
    assert seed.mixed_leaf(tag, c.inst[0], c.ci[0], c.proof[0]) != seed.leaf(tag + c.inst[0], c.ci[0], c.proof[0])


def test_header_binding_and_argument_rules():
    from plutus_halo2_verifier_gen_amd import api, backend
    with open(os.path.join(ROOT, "include", "h2v.h")) as f:
        h = f.read()
    m = re.search(r"#define\s+H2V_RLC_SEED_KEYED\s+(\d+)u", h)
    assert m and int(m.group(1)) == 64 == backend.RLC_SEED_KEYED
    assert re.search(r"\bint\s+h2v_probe_mixed_seed\s*\(", h) and "h2v_probe_mixed_seed" in backend.EXPORTS
    assert backend._rlc_opts(None, keyed_seed=True).flags == 64 and bytes(backend._rlc_opts(None, keyed_seed=True).seed) == bytes(32)
    assert backend._rlc_opts(None, grouped=True, keyed_seed=True).flags == 64 | 16
    assert backend._rlc_opts(bytes(32), keyed_seed=True).flags == 65               # (the library refuses it)
    assert backend._rlc_opts(None, derive_seed=True, keyed_seed=True).flags == 96  # (the library refuses it)
    for fn in (backend.verify_mixed, backend.verify_mixed_device, backend.aggregate_mixed, backend.aggregate_mixed_device, api.verify_mixed,
               api.batch_verify, api.Aggregator.__init__):
        assert "keyed_seed" in inspect.signature(fn).parameters, fn
    assert callable(backend.probe_mixed_seed)
    # argument rules that come back before any device call
    L = backend.lib()
    pair = C.create_string_buffer(96)
    inc = (C.c_uint8 * 4)()
    mb = backend.MixedBatch(0, None, None, None, None, None)
    plans = (C.c_void_p * 1)()

    def refused(flags, word):
        o = backend.RlcOpts((C.c_uint8 * 32)(), flags)
        assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, inc, None, None, C.byref(o), None) == -1
        assert word in L.h2v_last_error().decode(), L.h2v_last_error().decode()
        assert L.h2v_aggregate_mixed_device(plans, 0, C.byref(mb), C.addressof(pair), None, None, None, None, C.byref(o), None) == -1
        assert word in L.h2v_last_error().decode()
        acc = (C.c_uint8 * 4)()
        assert L.h2v_verify_mixed(plans, 0, C.byref(mb), acc, None, None, backend.MIXED_RLC, C.byref(o), None) == -1
        assert word in L.h2v_last_error().decode()

    refused(64 | 1, "H2V_RLC_SEED_GIVEN")
    refused(64 | 32, "H2V_RLC_SEED_TRANSCRIPT")
    # the flag alone passes the argument rules of a mixed call of no proofs: nothing is derived, (inf, inf), H2V_OK
    o = backend.RlcOpts((C.c_uint8 * 32)(), 64)
    info = backend.AggregateInfo()
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, inc, None, None, C.byref(o), C.byref(info)) == 0
    assert pair.raw[0] == 0xc0 and pair.raw[48] == 0xc0 and bytes(info.seed_used) == bytes(32)
    # ... a mixed call without H2V_MIXED_RLC has no coefficients
    acc = (C.c_uint8 * 4)()
    assert L.h2v_verify_mixed(plans, 0, C.byref(mb), acc, None, None, 0, C.byref(o), None) == -1
    assert "H2V_MIXED_RLC" in L.h2v_last_error().decode()
    # ... and the single-key aggregate call names the reason, before it looks at anything else
    one = backend.Batch(0, None, None, None, None)
    assert L.h2v_aggregate_batch(None, C.byref(one), pair, inc, None, None, C.byref(o), None) == -1
    assert "H2V_RLC_SEED_KEYED" in L.h2v_last_error().decode() and "mixed" in L.h2v_last_error().decode()
    # flag 32 keeps its refusal in the mixed calls
    t = backend.RlcOpts((C.c_uint8 * 32)(), 32)
    assert L.h2v_aggregate_mixed(plans, 0, C.byref(mb), pair, inc, None, None, C.byref(t), None) == -1
    assert "not available in the mixed calls" in L.h2v_last_error().decode()


def test_aggregator_rules():
    from plutus_halo2_verifier_gen_amd import api
    with pytest.raises(ValueError, match="exclude each other"):
        api.Aggregator(None, derive_seed=True, keyed_seed=True)
    with pytest.raises(ValueError, match="single-key"):
        api.Aggregator(None, derive_seed=True).push_mixed([], [], [])
    agg = api.Aggregator(None, keyed_seed=True)
    assert agg.keyed_seed and not agg.derive_seed
    assert "one-plan mixed call" in api.Aggregator.__init__.__doc__.lower().replace("\n", " ").replace("  ", " ")
    with pytest.raises(ValueError, match="keyed_seed needs mode='rlc'"):
        api.verify_mixed([], [], [], keyed_seed=True)
