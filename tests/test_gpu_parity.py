"""GPU parity tests (run with -m gpu on the MI355X box).  Everything goes through the C-ABI (libh2v_hip.so) and is
compared bit-for-bit with the CPU oracle / the reference golden vectors.  /root/reference is NOT needed."""
import hashlib
import json
import random

import pytest

from plutus_halo2_verifier_gen_amd import bls12_381 as bls

pytestmark = pytest.mark.gpu
P, R = bls.P, bls.R


@pytest.fixture(scope="module")
def be():
    from plutus_halo2_verifier_gen_amd import backend
    assert backend.device_count() >= 1, "no GPU visible"
    return backend


@pytest.fixture(scope="module")
def circuits():
    """name -> (vk, trapdoor, plan, device plan, oracle vk)"""
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, vk as V
    from oracle import binding as orc
    out = {}
    for name, build in V.BUILDERS.items():
        vk, td = build()
        pl = PL.compile_plan(vk)
        dp = backend.DevicePlan(pl.to_bytes(), 0)
        ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
        out[name] = (vk, td, pl, dp, ov)
    return out


def test_field_ops(be):
    rng = random.Random(1)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, (1 << 380), (1 << 381) - 1 - ((1 << 381) - 1 >= P) * ((1 << 381) - P)]
    a = edge + [rng.randrange(P) for _ in range(200)]
    b = list(reversed(edge)) + [rng.randrange(P) for _ in range(200)]
    assert be.probe_field(0, a, b) == [x * y % P for x, y in zip(a, b)]
    assert be.probe_field(1, a, b) == [(x + y) % P for x, y in zip(a, b)]
    assert be.probe_field(2, a, b) == [(x - y) % P for x, y in zip(a, b)]
    inv = be.probe_field(3, a, b)
    assert inv == [pow(x, P - 2, P) if x else 0 for x in a]
    edge_r = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, 1 << 254]
    a = edge_r + [rng.randrange(R) for _ in range(200)]
    b = list(reversed(edge_r)) + [rng.randrange(R) for _ in range(200)]
    assert be.probe_field(4, a, b) == [x * y % R for x, y in zip(a, b)]
    assert be.probe_field(5, a, b) == [pow(x, R - 2, R) if x else 0 for x in a]


def test_blake2b(be):
    rng = random.Random(2)
    for ln in [0, 1, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 1000, 1325]:
        msgs = [bytes(rng.randrange(256) for _ in range(ln)) for _ in range(70)]
        assert be.probe_blake2b(msgs) == [hashlib.blake2b(m, digest_size=32).digest() for m in msgs]


def test_g1_decompress(be, orc, kats):
    rng = random.Random(3)
    cases = [bytes.fromhex(kats[k]) for k in ("point_generator", "point_neg_generator", "point_42g")]
    proof = bytes.fromhex(kats["simple_mul_full"]["proof"])
    cases += [proof[48 * i:48 * i + 48] for i in range(8)]           # the golden proof's leading G1 elements
    cases += [bls.g1_compress(bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))) for _ in range(20)]
    gen = bls.g1_compress(bls.G1_GEN)
    cases += [bytes([gen[0] & 0x7F]) + gen[1:], bytes([0xC0]) + bytes(47), bytes([0xE0]) + bytes(47),
              bytes([0xC0]) + bytes(46) + b"\x01", bytes([0x9F]) + b"\xff" * 47, bytes([0x80]) + bytes(47)]
    for _ in range(40):                                               # random x: off-curve / on-curve-not-in-subgroup
        raw = bytearray(rng.randrange(P).to_bytes(48, "big"))
        raw[0] |= 0x80 | (0x20 if rng.random() < 0.5 else 0)
        cases.append(bytes(raw))
    # points of small order (the cofactor is 3 * 11^2 * 10177^2 * ...): the subgroup test's double-and-add chain meets
    # P + (-P) and the point at infinity in the middle of the ladder
    h = 0x396c8c005555e1568c00aaab0000aaab            # #E(Fp) = h * r
    assert h % 3 == 0 and h % 11 == 0 and h % 10177 == 0
    found = 0
    x = 1
    while found < 6:
        x += 1
        y = bls.fp_sqrt((x * x * x + 4) % P)
        if y is None:
            continue
        for q in (3, 11, 10177):
            t = bls.g1_mul((x, y), h * R // q)
            if t is not None:
                cases.append(bls.g1_compress(t))
                found += 1
    got = be.probe_g1_decompress(cases)
    for c, (ok, pt) in zip(cases, got):
        ook, opt = orc.g1_decompress(c)
        assert ok == ook, c.hex()
        if ok:
            assert pt == opt, c.hex()
    # the whole table of tests/g1_encodings.py through the same one-block form (the MSM and pairing probes decompress with it):
    # the merged verdict, the point where it is 1 and (0, 0) where it is 0
    from tests import g1_encodings as G
    table = G.cases()
    got = be.probe_g1_decompress([c.enc for c in table] * 3)          # (three times: every case in three lane positions)
    for c, (ok, pt) in zip(table * 3, got):
        assert ok == c.in_g1, (c.name, c.enc.hex())
        assert pt == (c.point if c.in_g1 else None), (c.name, c.enc.hex())


def test_g1_msm(be, orc):
    rng = random.Random(4)
    for T in (1, 2, 5, 16, 34, 58, 64):
        groups_s, groups_b, pts = [], [], []
        for g in range(5):
            ps = [bls.g1_mul(bls.G1_GEN, rng.randrange(1, R)) for _ in range(T)]
            ss = [rng.randrange(R) for _ in range(T)]
            if g == 1:
                ss[0] = 0
                ss[-1] = R - 1
            if g == 2 and T >= 2:
                ps[1] = ps[0]                     # equal bases: the reduction must double
                ss[1] = ss[0]
            if g == 3 and T >= 2:
                ps[1] = bls.g1_neg(ps[0])         # opposite bases with equal scalars: partial sums cancel
                ss[1] = ss[0]
            if g == 4:
                ps[0] = None                      # infinity base
                # GLV / window edge scalars: halves that vanish, lambda +- 1, digits at the window borders
                lam = bls.GLV_LAMBDA
                edge = [1, 2, 7, 8, 9, 15, 16, 17, lam - 1, lam, lam + 1, 2 * lam, R - lam, (1 << 128) - 1, 1 << 128,
                        (1 << 255) % R, 0x8888888888888888888888888888888888888888888888888888888888888888 % R]
                for t in range(1, T):
                    ss[t] = edge[(t - 1) % len(edge)]
            groups_s.append(ss)
            pts.append(ps)
            groups_b.append([bls.g1_compress(p) for p in ps])
        got = be.probe_g1_msm(groups_s, groups_b)
        for ss, ps, r in zip(groups_s, pts, got):
            assert r == orc.g1_msm(ss, ps)


def test_g1_msm_fixed_base_edge_scalars(be, orc, circuits):
    """The fixed-base launch of a split MSM (k_g1_msm_fixed: signed 12-bit windows over all-window tables of the VK bases) on its
    own, against the oracle's fold, on the scalars at the edges of the recoding - among them r - 2, the ONE scalar whose last
    window is a doubling (digit -1 onto the prefix r - 1: ADVICE r3), r - 1, 0, 1, window borders, all-ones windows - with 1, 2
    and 4 bases per lane."""
    rng = random.Random(21)
    for name in ("simple_mul", "lookup_table"):
        vk, td, pl, dp, ov = circuits[name]
        from plutus_halo2_verifier_gen_amd import plan as PL
        bases = [pl.vk_bases[idx] for kind, idx in pl.terms if kind == PL.TERM_VK_BASE]
        nf = be.probe_g1_msm_fixed(dp, None)
        assert nf == len(bases) and nf > 0
        edge = [R - 2, R - 1, 0, 1, 2, 2047, 2048, 2049, 4095, 4096, (1 << 12) - 1, (1 << 24) - 1, (1 << 252) + 2048, R - 2049, R - 2048, R - 2047,
                int("800" * 21, 16) % R, int("7ff" * 21, 16) % R, int("801" * 21, 16) % R, (R - 2) // 2, (R + 1) // 2]
        rows = []
        for e in edge:                                   # the edge scalar on every base in turn, random ones elsewhere
            for t in range(nf):
                row = [rng.randrange(R) for _ in range(nf)]
                row[t] = e
                rows.append(row)
        rows.append([R - 2] * nf)
        rows.append([0] * nf)
        for k in (1, 2, 4):
            got = be.probe_g1_msm_fixed(dp, rows, bases_per_lane=k)
            for row, r in zip(rows, got):
                assert r == orc.g1_msm(row, bases), (name, k, [hex(x) for x in row])


def test_null_stream_contract_of_deferred_joins(be, circuits):
    """include/h2v.h, h2v_workspace_defer_joins: the lanes run on blocking streams, so a deferring workspace refuses the
    legacy NULL stream (PyTorch's default stream) with H2V_E_ARG instead of silently serialising; without deferred joins NULL
    is accepted; h2v_workspace_join(ws, NULL) blocks the HOST (results readable right after it, nothing on the NULL stream)."""
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n = 150
    b = synth.forge_batch(vk, td, n, seed=8, plan=pl, workers=2)
    b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.2, seed=9, kinds=list(synth.CORRUPTIONS))
    dev = torch.device("cuda", 0)
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    dpr, din = up(b.proofs), up(b.instances)
    dof = torch.tensor(b.proof_off, dtype=torch.int64).to(dev)
    ws = be.Workspace(dp, n, lanes=3, chunk=40)
    acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    dp.verify_batch_device(n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None, acc.data_ptr(), None, ws=ws, stream=None)   # joins not deferred: fine
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == b.expected
    ws.defer_joins(True)
    with pytest.raises(be.H2VError, match="NULL stream"):
        dp.verify_batch_device(n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None, acc.data_ptr(), None, ws=ws, stream=None)
    with pytest.raises(be.H2VError, match="NULL stream"):
        dp.verify_batch_rlc_device(n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None, acc.data_ptr(), None, ws=ws, stream=None)
    s = torch.cuda.Stream(device=dev)
    accs = [torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(4)]
    for a in accs:
        dp.verify_batch_device(n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None, a.data_ptr(), None, ws=ws, stream=s.cuda_stream)
    ws.join(None)                                    # the host waits; no torch synchronisation before the reads below
    for a in accs:
        assert a.cpu().tolist() == b.expected
    ws.close()


def test_batch_stream_keeps_batches_in_flight(be, circuits):
    """backend.BatchStream (depth 4: the in-flight launch shapes) over nine batches of different content and size, per proof
    and RLC: every collected vector is the blocking call's, in order."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    batches = []
    for k in range(9):
        n = 40 + 7 * k
        b = synth.forge_batch(vk, td, n, seed=300 + k, plan=pl, workers=2)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.2, seed=400 + k, kinds=list(synth.CORRUPTIONS))
        batches.append(b)
    for rlc in (False, True):
        bs = be.BatchStream(dp, 128, 4, rlc=rlc)
        got, keep = [], []
        for b in batches:
            hb, k_ = dp.host_batch(b.proofs, b.proof_off, b.instances, b.committed)
            keep.append(k_)
            r = bs.push(hb, b.n)
            if r is not None:
                got.append(r)
        got += bs.drain()
        assert [list(a) for a, _fb in got] == [b.expected for b in batches], rlc
        bs.close()
    # the stream is ONE laned workspace: as many host batches in flight as it has lanes, the next submit is refused
    ws = be.Workspace(dp, 128, lanes=2, chunk=128)
    hb, k_ = dp.host_batch(batches[0].proofs, batches[0].proof_off, batches[0].instances, batches[0].committed)
    dp.submit(hb, ws)
    dp.submit(hb, ws)
    with pytest.raises(be.H2VError, match="in flight"):
        dp.submit(hb, ws)
    assert list(ws.wait(batches[0].n)[0]) == batches[0].expected and list(ws.wait(batches[0].n)[0]) == batches[0].expected
    with pytest.raises(be.H2VError, match="no batch"):
        ws.wait(1)
    ws.close()


@pytest.mark.parametrize("name", ["simple_mul", "trashcan_mix", "ivc"])
def test_verdicts_do_not_depend_on_the_chunking(be, circuits, name):
    """Laned workspaces (h2v_workspace_create_lanes): a call is cut into chunks that run through library-owned lanes.  For
    every (lanes, chunk) - ragged last chunk, more lanes than chunks, more chunks than lanes, chunk of 1 - the accept vector
    is the unchunked call's and the oracle's, per proof and in RLC mode, through the host-buffer and the device-resident
    entry points; and with deferred joins three consecutive calls on ONE workspace overlap in the lanes and still give
    each call its own vector."""
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits[name]
    n = 203
    batch = synth.forge_batch(vk, td, n, seed=71, plan=pl, workers=4)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.3, seed=72, kinds=list(synth.CORRUPTIONS))
    want = list(ov.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, threads=16))
    assert want == batch.expected and 0 < sum(want) < n
    plain = be.Workspace(dp, n)
    assert plain.lanes() == (1, n) and plain.depth(n) == 1
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=plain)) == want
    plain.close()
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    d_proofs, d_inst, d_ci = up(batch.proofs), up(batch.instances), up(batch.committed)
    d_off = torch.tensor(batch.proof_off, dtype=torch.int64).to(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    for lanes, chunk in [(3, 64), (2, 100), (16, 7), (5, 203), (4, 1000), (3, 1)]:
        ws = be.Workspace(dp, n, lanes=lanes, chunk=chunk)
        assert ws.lanes() == (lanes, min(chunk, n)) and ws.depth(n) == ws.depth(n, rlc=True) == lanes   # (an explicit lane count holds)
        assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == want, (lanes, chunk)
        got, _fb = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws, seed=bytes(range(32)))
        assert list(got) == want, (lanes, chunk, "rlc")
        # device-resident form: accept[] and status[] written in place chunk by chunk
        acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        dp.verify_batch_device(n, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci), acc.data_ptr(), st.data_ptr(), ws=ws)
        torch.cuda.synchronize()
        assert acc.cpu().tolist() == want and [int(x == 0) for x in st.cpu().tolist()] == want
        if -(-n // min(chunk, n)) <= 32:      # (a lane remembers the events of its last 64 chunks)
            tm = ws.timings()
            assert tm.launches == -(-n // min(chunk, n)) and tm.pairing_ms > 0 and tm.total_ms > 0
        ws.close()
    # deferred joins: three calls of different sizes back to back on one workspace and one (non-default) stream
    ws = be.Workspace(dp, n, lanes=3, chunk=40)
    ws.defer_joins(True)
    s = torch.cuda.Stream(device=dev)
    sizes = [n, 150, 77]
    accs = [torch.full((m,), 9, dtype=torch.uint8, device=dev) for m in sizes]
    for m, a in zip(sizes, accs):
        dp.verify_batch_device(m, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci), a.data_ptr(), None, ws=ws, stream=s.cuda_stream)
    ws.join(s.cuda_stream)
    s.synchronize()
    for m, a in zip(sizes, accs):
        assert a.cpu().tolist() == want[:m]
    with pytest.raises(be.H2VError):
        be.Workspace(dp, n).defer_joins(True)      # only laned workspaces
    ws.close()


def test_in_flight_hint_changes_the_shape_not_the_verdicts(be, circuits):
    """h2v_workspace_hint_in_flight(>= 4): the per-proof MSM runs two terms per lane (k_g1_msm_multi with four halves per lane, reported as 18) -
    the accept vector and the statuses stay those of the default shape."""
    from plutus_halo2_verifier_gen_amd import synth
    for name in ("simple_mul", "lookup_table", "atms_with_lookups"):   # (atms at 2048+ proofs: ladders beside a fixed-base launch)
        vk, td, pl, dp, ov = circuits[name]
        batch = synth.forge_batch(vk, td, 96, seed=61, plan=pl, workers=2)
        batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.3, seed=62, kinds=list(synth.CORRUPTIONS))
        ws1, ws5, ws8 = be.Workspace(dp, 96), be.Workspace(dp, 96), be.Workspace(dp, 96)
        ws5.hint_in_flight(5)
        ws8.hint_in_flight(8)     # from 6: the whole pipeline on the caller's stream
        a1 = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws1)
        a5 = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws5)
        a8 = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws8)
        assert list(a1) == list(a5) == list(a8) == batch.expected
        # (a 96-proof launch is a chain of lone waves whatever else is in flight: it keeps the two-lanes-per-term ladder)
        assert ws1.timings().msm_lanes_per_term in (1, 2, 3) and ws5.timings().msm_lanes_per_term in (1, 2, 3)
        with pytest.raises(be.H2VError):
            ws5.hint_in_flight(0)
        ws1.close(); ws5.close(); ws8.close()
    # from a quarter of a wave per SIMD up (simple_mul: 1024 proofs x 16 terms = 256 waves) the hint selects the split MSM, and
    # its ladder launch (10 per-proof terms: 2048 proofs for the same quarter) runs two terms per lane
    vk, td, pl, dp, ov = circuits["simple_mul"]
    batch = synth.forge_batch(vk, td, 2048, seed=65, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.05, seed=66, kinds=list(synth.CORRUPTIONS))
    ws = be.Workspace(dp, 2048)
    ws.hint_in_flight(5)
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == batch.expected
    # (two kernels side by side for a caller that keeps the chip full: two-terms-per-lane ladders over the per-proof terms,
    #  the fixed-base kernel over the VK bases)
    tm = ws.timings()
    assert tm.msm_lanes_per_term == 3 and tm.msm_var_lanes_per_term == 18 and tm.g1_msm_fixed_ms > 0
    ws.close()
    # the split launch (per-proof terms two per lane beside the fixed-base lanes) needs a batch that does not fit one wave per SIMD
    vk, td, pl, dp, ov = circuits["atms_with_lookups"]
    batch = synth.forge_batch(vk, td, 2048, seed=63, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.05, seed=64, kinds=list(synth.CORRUPTIONS))
    ws = be.Workspace(dp, 2048)
    ws.hint_in_flight(5)
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)) == batch.expected
    assert ws.timings().msm_lanes_per_term == 3 and ws.timings().pairing_lanes_per_proof == 16
    ws.close()


def test_workspace_options_change_the_shape_not_the_verdicts(be, circuits):
    """h2v_workspace_set_option: the launch shapes that round 2 could only force through environment variables (terms per lane
    of the per-proof MSM, the pairing engine, the streams of a call) - every combination gives the construction's vector, the
    reported shape is the requested one, and bad values are refused."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["lookup_table"]
    n = 130
    batch = synth.forge_batch(vk, td, n, seed=81, plan=pl, workers=4)
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.3, seed=82, kinds=list(synth.CORRUPTIONS))
    ws = be.Workspace(dp, n)
    W = be.Workspace
    for tpl, lpt_code in ((1, None), (2, 18), (3, 19), (4, 20), (0, None)):
        for engine in (6, 12, 16, 32, 64, 1, 0):
            for streams in (0, 1, 2, -1):
                ws.set_option(W.OPT_MSM_TERMS_PER_LANE, tpl)
                ws.set_option(W.OPT_PAIRING_ENGINE, engine)
                ws.set_option(W.OPT_STREAMS, streams)
                got = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
                assert list(got) == batch.expected, (tpl, engine, streams)
                tm = ws.timings()
                if lpt_code:
                    assert tm.msm_lanes_per_term == lpt_code
                if engine:
                    assert tm.pairing_lanes_per_proof == engine
    for opt, bad in ((W.OPT_MSM_TERMS_PER_LANE, 5), (W.OPT_PAIRING_ENGINE, 8), (W.OPT_STREAMS, 3), (99, 0)):
        with pytest.raises(be.H2VError):
            ws.set_option(opt, bad)
    ws.close()
    # a laned workspace hands the option to its lanes
    lw = be.Workspace(dp, n, lanes=2, chunk=50)
    lw.set_option(W.OPT_PAIRING_ENGINE, 64)
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=lw)) == batch.expected
    assert lw.timings().pairing_lanes_per_proof == 64
    lw.close()


def test_quad_cooperative_addition_in_every_lane(be):
    """The quad-cooperative mixed addition (forced MSM shape H2V_MSM_LPT=8) against the one-lane one and the big-integer
    model, in EVERY lane of the quad: with its DPP broadcasts left to the optimiser, lane 0 alone came out wrong
    (csrc/h2v_curve28.hpp: g1j28_madd_quad) - a result only lanes 1..3 would have hidden."""
    rng = random.Random(23)
    for neg in (False, True):
        P = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
        Q = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
        res = be.probe_quad_madd(P, Q, neg)
        want = bls.g1_add(bls.g1_mul(P, 2), bls.g1_neg(Q) if neg else Q)
        for X, Y, Z in res:
            zi = pow(Z, -1, bls.P)
            assert (X * zi * zi % bls.P, Y * zi * zi * zi % bls.P) == want


def test_pairing(be, orc, circuits):
    vk, td, pl, dp, ov = circuits["simple_mul"]
    rng = random.Random(5)
    s = td.s
    p1, p2, want = [], [], []
    for k in range(6):
        a = rng.randrange(1, R)
        A = bls.g1_mul(bls.G1_GEN, a)
        sA = bls.g1_mul(A, s)
        if k % 3 == 2:
            sA = bls.g1_add(sA, bls.G1_GEN)
        p1.append(bls.g1_compress(A))
        p2.append(bls.g1_compress(sA))
        want.append(orc.pairing_check(A, bytes.fromhex(vk.s_g2), sA, orc.g2_generator_compressed()))
    p1 += [bls.g1_compress(None), bls.g1_compress(bls.G1_GEN), bls.g1_compress(None)]
    p2 += [bls.g1_compress(None), bls.g1_compress(None), bls.g1_compress(bls.G1_GEN)]
    want += [1, 0, 0]
    assert be.probe_pairing(dp, p1, p2) == want
    assert want[:6] == [1, 1, 0, 1, 1, 0]


def test_pairing_cooperative_matches_one_lane_kernel(be, orc, circuits):
    """The 16-lanes-per-proof pairing kernel against the one-lane-per-proof kernel: same Miller-loop value (all 12
    Fp coefficients), same accept; final value == 1 exactly when accepted."""
    vk, td, pl, dp, ov = circuits["simple_mul"]
    rng = random.Random(6)
    p1, p2 = [], []
    for k in range(9):
        A = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
        sA = bls.g1_mul(A, td.s)
        if k % 3 == 2:
            sA = bls.g1_add(sA, bls.G1_GEN)
        p1.append(bls.g1_compress(A))
        p2.append(bls.g1_compress(sA))
    p1 += [bls.g1_compress(None), bls.g1_compress(bls.G1_GEN), bls.g1_compress(None)]
    p2 += [bls.g1_compress(None), bls.g1_compress(None), bls.g1_compress(bls.G1_GEN)]
    for k in range(2):   # 14 pairs: the last wave of every engine has idle groups (two of four in the narrow one, six of ten in the six-lane one)
        A = bls.g1_mul(bls.G1_GEN, rng.randrange(1, R))
        p1.append(bls.g1_compress(A))
        p2.append(bls.g1_compress(bls.g1_mul(A, td.s) if k == 0 else bls.g1_mul(A, td.s + 1)))
    acc0, dump0 = be.probe_pairing_ex(dp, p1, p2, impl=0)
    for impl in (1, 2, 3, 5, 6):   # the launcher's choice (wide for 12 pairs), the narrow engine (16 lanes per proof), the wide one (64), six lanes per proof, twelve
        acc1, dump1 = be.probe_pairing_ex(dp, p1, p2, impl=impl)
        assert acc0 == acc1 == [1, 1, 0] * 3 + [1, 0, 0] + [1, 0], impl
        for i in range(len(p1)):
            assert dump0[i][0] == dump1[i][0], "Miller loop value differs for pair %d (engine %d)" % (i, impl)
            is_one = dump1[i][1] == [1] + [0] * 11
            assert is_one == bool(acc1[i])


TRACE_NAMES = ["theta", "beta", "gamma", "trash", "y", "x", "x1", "x2", "x3", "x4", "x_prev", "x_next", "x_last", "xn",
               "l_last", "l_0", "active_rows", "h_eval", "vanishing_s", "f_eval", "v"]


@pytest.mark.parametrize("name", ["simple_mul", "lookup_table", "atms_with_lookups", "sha256", "secp256k1", "ivc", "trashcan_mix", "phased"])
def test_end_to_end_vs_oracle(be, circuits, name):
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits[name]
    n = 48
    # committed instance: the identity for the sha256 shape (as in examples/sha256.rs:133), a real point for the others
    batch = synth.forge_batch(vk, td, n, seed=21, plan=pl, workers=1, ci_identity=(name == "sha256"))
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.4, seed=9, kinds=list(synth.CORRUPTIONS))
    got = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed)
    want = ov.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, threads=8)
    assert list(got) == list(want) == batch.expected
    assert 0 < sum(got) < n
    # intermediate values (the reference's plutus_debug trace surface) for one accepting and one rejecting proof
    for i in (batch.expected.index(1), batch.expected.index(0)):
        proof = batch.proof(i)
        inst = batch.instances[32 * vk.n_public_inputs * i:32 * vk.n_public_inputs * (i + 1)]
        ok, otr = ov.verify(proof, batch.instance_ints(i, vk.n_public_inputs), batch.ci(i), trace=True)
        tr = dp.trace(proof, inst, batch.ci(i))
        assert tr["accept"] == int(ok)
        if otr.status in (0, 1):  # the oracle fills its trace only when it reaches the pairing
            for slot, val in tr["scalars"].items():
                if slot < 32:
                    assert val == otr.scalar(TRACE_NAMES[slot]), TRACE_NAMES[slot]
                else:
                    assert val == otr.expression(slot - 32), "expression %d" % (slot - 32)
            assert tr["el"] == otr.point("el") and tr["er"] == otr.point("er")


def test_golden_transcript_on_gpu(be, kats, circuits):
    """The reference's full simple_mul proof (transcript.ak:241-382) replayed by the GPU transcript kernel.  The golden
    proof predates the `trash` squeeze (proof.rs:68): with the current layout only theta/beta/gamma are comparable
    (first half of this test); a test-only plan with the legacy layout (compile_plan(legacy_no_trash_squeeze=True))
    replays ALL of it - gamma, y, x, the three advice evaluations, x1..x4 and pi - on the GPU."""
    from plutus_halo2_verifier_gen_amd import plan as PL, vk as V
    vk, td, pl, dp, ov = circuits["simple_mul"]
    k = kats["simple_mul_full"]
    H = lambda h: int(h, 16)
    proof = bytes.fromhex(k["proof"])
    inst = b"".join((42).to_bytes(32, "little") for _ in range(3))
    tr = dp.trace(proof, inst, None)
    assert tr["scalars"][TRACE_NAMES.index("gamma")] == H(k["gamma"])
    assert tr["accept"] == 0   # (different VK / layout: must not verify)
    # the whole vector through the legacy layout, with the vector's own transcript representation
    assert vk.transcript_repr == H(k["transcript_repr"])   # vk.py's simple_mul key carries the vector's representation
    pl2 = PL.compile_plan(vk, legacy_no_trash_squeeze=True)
    assert pl2.proof_len == 1120
    dp2 = be.DevicePlan(pl2.to_bytes(), 0)
    tr2 = dp2.trace(proof, inst, None)
    sc = {PL.TRACE_NAMES[s]: v for s, v in tr2["scalars"].items() if s < PL.TRACE_EXPR0}
    for name in ("gamma", "y", "x", "advice_eval_1", "advice_eval_2", "advice_eval_3", "x1", "x2", "x3", "x4"):
        assert sc[name] == H(k[name]), name
    assert tr2["el"] == bls.g1_decompress(bytes.fromhex(k["pi"]))          # el = pi
    assert not (tr2["status"] & (be.ST_BAD_SCALAR | be.ST_SHORT_PROOF | be.ST_BAD_POINT))   # every element parses
    # the batch path (multi-lane schedule, LDS register file) reads the same proof: rejected by the pairing only
    got = dp2.verify_batch(proof * 3, [0, 1120, 2240, 3360], inst * 3, None)
    assert list(got) == [0, 0, 0]


def test_api_errors(be, circuits):
    vk, td, pl, dp, ov = circuits["simple_mul"]
    blob = pl.to_bytes()
    with pytest.raises(be.H2VError):
        be.DevicePlan(blob[:-8], 0)
    with pytest.raises(be.H2VError):
        be.DevicePlan(b"XXXXXXXX" + blob[8:], 0)
    bad = bytearray(blob)
    bad[8 + 4 * 4] = 1  # n_regs = 1: instructions out of range
    bad[8 + 4 * 4 + 1] = 0
    with pytest.raises(be.H2VError):
        be.DevicePlan(bytes(bad), 0)
    # empty batch is fine
    assert dp.verify_batch(b"", [0], b"", None) == b""
    # a workspace is sized from the plan it was created for: a larger plan (more terms / point slots, recursion
    # buffers) must get H2V_E_ARG, not device memory corruption; a smaller plan may reuse it
    from plutus_halo2_verifier_gen_amd import synth
    ws_small = be.Workspace(dp, 8)
    for other in ("lookup_table", "ivc"):
        vk2, td2, pl2, dp2, ov2 = circuits[other]
        b2 = synth.forge_batch(vk2, td2, 2, seed=3, plan=pl2, workers=1)
        with pytest.raises(be.H2VError, match="workspace"):
            dp2.verify_batch(b2.proofs, b2.proof_off, b2.instances, b2.committed, ws=ws_small)
    vk2, td2, pl2, dp2, ov2 = circuits["lookup_table"]
    ws_big = be.Workspace(dp2, 8)
    b1 = synth.forge_batch(vk, td, 4, seed=3, plan=pl, workers=1)
    assert list(dp.verify_batch(b1.proofs, b1.proof_off, b1.instances, b1.committed, ws=ws_big)) == [1, 1, 1, 1]
    with pytest.raises(be.H2VError):   # offsets beyond the bytes handed over
        dp.verify_batch(b1.proofs[:-1], b1.proof_off, b1.instances, b1.committed)


def test_submit_wait_streams_batches_over_two_workspaces(be, circuits):
    """h2v_verify_batch_submit / _wait: several different batches in flight on two workspaces (pinned staging, one
    upload per batch), per-proof and RLC mode interleaved; every result == the oracle's vector for THAT batch; misuse
    (second submit on a busy workspace, wait without submit) is an API error."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n = 64
    wss = [be.Workspace(dp, n), be.Workspace(dp, n)]
    batches = []
    for k in range(5):
        b = synth.forge_batch(vk, td, n - 3 * k, seed=60 + k, plan=pl, workers=1)
        b = synth.with_rejects(pl, b, 3, fraction=0.25 if k % 2 else 0.0, seed=k, kinds=["flip_first_scalar", "bad_point_flag", "truncated"])
        batches.append(b)
    got = [None] * 5
    held = []
    for k, b in enumerate(batches):
        ws = wss[k % 2]
        if k >= 2:
            got[k - 2] = ws.wait(batches[k - 2].n)
        hb, keep = dp.host_batch(b.proofs, b.proof_off, b.instances, b.committed)
        dp.submit(hb, ws, rlc=(k % 3 == 1), seed=bytes([k]) * 32)
        del hb, keep          # the caller's buffers may go away as soon as submit returns
    with pytest.raises(be.H2VError, match="in flight"):
        hb, keep = dp.host_batch(batches[0].proofs, batches[0].proof_off, batches[0].instances, None)
        dp.submit(hb, wss[0])
    for k in (3, 4):
        got[k] = wss[k % 2].wait(batches[k].n)
    with pytest.raises(be.H2VError, match="no batch"):
        wss[0].wait(1)
    for k, b in enumerate(batches):
        want = ov.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, threads=4)
        assert list(got[k][0]) == list(want) == b.expected, k
        assert got[k][1] == (k % 3 == 1 and any(e == 0 for e in b.expected) and k % 2 == 1 and _has_pairing_reject(b, batches, k, ov))


def _has_pairing_reject(b, batches, k, ov):
    """does batch b hold a proof that only the pairing rejects (the RLC batch check then fails and falls back)?"""
    for i in range(b.n):
        if b.expected[i] == 0:
            ok, tr = ov.verify(b.proof(i), b.instance_ints(i, 3), None, trace=True)
            from oracle import binding as orc
            if orc.STATUS[tr.status] == "pairing":
                return True
    return False


def _permute(batch, order, n_pi):
    from plutus_halo2_verifier_gen_amd import synth
    proofs = [batch.proof(i) for i in order]
    off = [0]
    for p in proofs:
        off.append(off[-1] + len(p))
    inst = b"".join(batch.instances[32 * n_pi * i:32 * n_pi * (i + 1)] for i in order)
    ci = None if batch.committed is None else b"".join(batch.ci(i) for i in order)
    return synth.Batch(n=len(order), proofs=b"".join(proofs), proof_off=off, instances=inst, committed=ci,
                       expected=[batch.expected[i] for i in order])


def test_full_size_batch_properties(be, circuits):
    """BASELINE configs[1] size (simple_mul x 4096): size-independent properties + an oracle sample.
    accept must equal the construction (forged proofs accept, every corruption kind rejects), must not depend on the
    position of a proof in the batch (permutation), nor on the batch it travels in (prefix), and must equal the
    oracle's verdict on a random sample."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n, n_pi = 4096, vk.n_public_inputs
    batch = synth.forge_batch(vk, td, n, seed=77, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, n_pi, fraction=0.1, seed=13, kinds=list(synth.CORRUPTIONS))
    ws = be.Workspace(dp, n)
    got = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
    assert list(got) == batch.expected
    assert 3000 < sum(got) < n
    order = list(range(n))
    random.Random(5).shuffle(order)
    perm = _permute(batch, order, n_pi)
    got_p = dp.verify_batch(perm.proofs, perm.proof_off, perm.instances, perm.committed, ws=ws)
    assert list(got_p) == [got[i] for i in order]
    pre = _permute(batch, list(range(1000)), n_pi)
    assert list(dp.verify_batch(pre.proofs, pre.proof_off, pre.instances, pre.committed)) == list(got[:1000])
    # the library's own laned workspace (what h2v_workspace_create returns from four chunks up): the lanes a call cycles through
    # depend on the chunk it gives the kernels - eight for whole chunks, all sixteen for small ones and for the RLC mode - and the
    # verdicts on neither
    lw = be.Workspace(dp, 4 * n)
    assert lw.lanes() == (16, n) and lw.depth(n) == 8 and lw.depth(64) == 16 and lw.depth(n, rlc=True) == 16
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=lw)) == batch.expected
    small = _permute(batch, list(range(64)), n_pi)
    for _ in range(3):
        assert list(dp.verify_batch(small.proofs, small.proof_off, small.instances, small.committed, ws=lw)) == list(got[:64])
    lw.close()
    # Large single calls through several kinds of workspace in ONE process, ending on the default laned one: every pool stream
    # has run the kernels with the largest private segments by then.  (With 3 KB of scratch per lane in the decompression, MSM and
    # six-lane pairing kernels this very sequence ended in HSA_STATUS_ERROR_OUT_OF_RESOURCES - a queue's scratch arena is sized by
    # the largest segment it has seen, and sixteen queues of them did not fit; the kernels now stay at or below 2 KB.)
    five = _permute(batch, [i % n for i in range(5 * n)], n_pi)
    for make in (lambda: be.Workspace(dp, 2 * n, lanes=1, chunk=2 * n), lambda: be.Workspace(dp, 2 * n),
                 lambda: be.Workspace(dp, 5 * n, lanes=1, chunk=5 * n), lambda: be.Workspace(dp, 5 * n)):
        w_ = make()
        m = min(w_.max_batch, 5 * n)
        part = five if m == 5 * n else _permute(five, list(range(m)), n_pi)
        for _ in range(2):
            assert list(dp.verify_batch(part.proofs, part.proof_off, part.instances, part.committed, ws=w_)) == (batch.expected * 5)[:m]
        w_.close()
    sample = sorted(random.Random(6).sample(range(n), 192))
    sb = _permute(batch, sample, n_pi)
    want = ov.verify_batch(sb.proofs, sb.proof_off, sb.instances, sb.committed, threads=16)
    assert list(want) == [got[i] for i in sample]


def test_ragged_and_edge_batches(be, circuits):
    """Ragged inputs: proofs of different lengths in one buffer (truncated, exact, with trailing bytes, empty), gaps
    between proofs, a single-proof batch, and a batch larger than the workspace it is handed (must be refused, not
    overrun).  prepare() reads exactly the plan's layout; trailing bytes are the business of assert_empty()
    (examples/ivc.rs:92-94), so a proof followed by garbage still verifies."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["simple_mul"]
    n_pi = vk.n_public_inputs
    b = synth.forge_batch(vk, td, 6, seed=31, plan=pl, workers=1)
    L = pl.proof_len
    pieces = [b.proof(0), b.proof(1)[:L - 1], b.proof(2) + b"\xff" * 17, b"", b.proof(4)[:48], b.proof(5)]
    expected = [1, 0, 1, 0, 0, 1]
    # gaps: 5 junk bytes before every proof; offsets are given explicitly, so proof i is [off[i], off[i+1]) and the
    # junk belongs to the previous proof's tail (ignored by prepare)
    buf, off = b"", [0]
    for p in pieces:
        buf += p
        off.append(len(buf))
    got = dp.verify_batch(buf, off, b.instances, None)
    want = ov.verify_batch(buf, off, b.instances, None, threads=2)
    assert list(got) == list(want) == expected
    # single proof
    one = _permute(b, [3], n_pi)
    assert list(dp.verify_batch(one.proofs, one.proof_off, one.instances, None)) == [1]
    # workspace too small for the batch
    ws = be.Workspace(dp, 2)
    with pytest.raises(be.H2VError):
        dp.verify_batch(b.proofs, b.proof_off, b.instances, None, ws=ws)
    # the same workspace keeps working afterwards
    two = _permute(b, [0, 1], n_pi)
    assert list(dp.verify_batch(two.proofs, two.proof_off, two.instances, None, ws=ws)) == [1, 1]


def test_verdict_is_deterministic_and_workspace_reusable(be, circuits):
    """Idempotence: the same batch through the same workspace twice, then through a fresh one, gives one answer; a
    rejecting batch does not poison the workspace for the next accepting one."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits["lookup_table"]
    n_pi = vk.n_public_inputs
    good = synth.forge_batch(vk, td, 96, seed=41, plan=pl, workers=1)
    bad = synth.with_rejects(pl, good, n_pi, fraction=1.0, seed=3, kinds=[k for k in synth.CORRUPTIONS if not k.startswith("acc_")])
    ws = be.Workspace(dp, 96)
    a1 = dp.verify_batch(good.proofs, good.proof_off, good.instances, good.committed, ws=ws)
    r1 = dp.verify_batch(bad.proofs, bad.proof_off, bad.instances, bad.committed, ws=ws)
    a2 = dp.verify_batch(good.proofs, good.proof_off, good.instances, good.committed, ws=ws)
    a3 = dp.verify_batch(good.proofs, good.proof_off, good.instances, good.committed)
    assert list(a1) == list(a2) == list(a3) == [1] * 96
    assert list(r1) == bad.expected and sum(r1) == 0


def test_exported_artefact_files_verify_on_gpu(be, circuits, tmp_path, capsys):
    """The reference's export files (proof hex + JSON, public-input lines, committed x/y, generated VK constants;
    proof_serialization.rs:11-72, shared_utils/mod.rs:23-65) read back and verified through the C-ABI."""
    from plutus_halo2_verifier_gen_amd import synth, verify_files, wire
    vk, td, pl, dp, ov = circuits["sha256"]
    assert vk.n_committed_instances == 1
    b = synth.forge_batch(vk, td, 2, seed=51, plan=pl, workers=1)
    (tmp_path / "vk.json").write_text(vk.to_json())
    (tmp_path / "verifier_key.ak").write_text(wire.render_vk_constants_aiken(vk.constants()))
    args = ["--vk", str(tmp_path / "vk.json"), "--vk-constants", str(tmp_path / "verifier_key.ak")]
    for i in range(2):
        wire.export_proof(str(tmp_path / ("p%d.hex" % i)), b.proof(i))
        wire.serialize_proof(str(tmp_path / ("p%d.json" % i)), b.proof(i))
        with open(tmp_path / ("pi%d.hex" % i), "w") as f:
            wire.export_public_inputs(b.instance_ints(i, vk.n_public_inputs), f)
        with open(tmp_path / ("ci%d.hex" % i), "w") as f:
            wire.export_committed_inputs(bls.g1_decompress(b.ci(i), False) or (0, 0), f)
        args += ["--proof", str(tmp_path / ("p%d.%s" % (i, "hex" if i == 0 else "json"))),
                 "--public-inputs", str(tmp_path / ("pi%d.hex" % i)), "--committed", str(tmp_path / ("ci%d.hex" % i))]
    assert verify_files.main(args) == 0
    assert capsys.readouterr().out.count("accept") == 2
    # swap the public inputs of the two proofs: both must be rejected
    swapped = [a.replace("pi0", "piX").replace("pi1", "pi0").replace("piX", "pi1") for a in args]
    assert verify_files.main(swapped) == 1
    assert capsys.readouterr().out.count("reject") == 2
    # s_g2 from a KZG parameter file (src/kzg_params.rs:15-57; wire.parse_kzg_params: self-validating, layout unpinned):
    # alone it replaces the key's, next to the VK constants it must agree with them
    def params_file(name, s_pt):
        enc = lambda pt: b"".join(v.to_bytes(48, "big") for v in (pt[0][1], pt[0][0], pt[1][1], pt[1][0]))
        (tmp_path / name).write_bytes((4).to_bytes(4, "little") + bytes(2 * 16 * 96) + enc(bls.G2_GEN) + enc(s_pt))
        return str(tmp_path / name)
    s_pt = bls.g2_decompress(bytes.fromhex(vk.s_g2))
    assert verify_files.main(args + ["--kzg-params", params_file("kzg_params_4", s_pt)]) == 0
    capsys.readouterr()
    other = params_file("kzg_params_other", bls.g2_mul(bls.G2_GEN, 5))
    with pytest.raises(wire.WireError, match="differs"):
        verify_files.main(args + ["--kzg-params", other])
    no_constants = [a for i, a in enumerate(args) if i not in (2, 3)]
    with pytest.raises(wire.WireError, match="differs"):                         # a guessed layout never replaces the key's s_g2 by itself
        verify_files.main(no_constants + ["--kzg-params", other])
    assert verify_files.main(no_constants + ["--kzg-params", other, "--trust-kzg-params"]) == 1      # another trapdoor: nothing verifies
    assert capsys.readouterr().out.count("reject") == 2


@pytest.mark.parametrize("name,n", [("simple_mul", 4096), ("lookup_table", 2048), ("atms_with_lookups", 2048), ("sha256", 1024), ("secp256k1", 512),
                                    ("ivc", 1024)])
def test_baseline_config_sizes(be, circuits, name, n):
    """The other BASELINE configurations at their full batch sizes: the verdict vector equals the construction (every
    corruption kind rejects, everything else accepts), does not depend on the order of the batch, and equals the
    oracle's on a sample."""
    from plutus_halo2_verifier_gen_amd import synth
    vk, td, pl, dp, ov = circuits[name]
    n_pi = vk.n_public_inputs
    batch = synth.forge_batch(vk, td, n, seed=90, plan=pl, workers=8)
    batch = synth.with_rejects(pl, batch, n_pi, fraction=0.08, seed=14, kinds=list(synth.CORRUPTIONS))
    ws = be.Workspace(dp, n)
    got = dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
    assert list(got) == batch.expected and 0 < sum(got) < n
    # the launch shapes of a caller that keeps five batches in flight (two MSM terms per lane, narrow pairing engine from
    # 2048 proofs up): the same vector
    ws5 = be.Workspace(dp, n)
    ws5.hint_in_flight(5)
    assert list(dp.verify_batch(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws5)) == list(got)
    ws5.close()
    order = list(range(n))
    random.Random(15).shuffle(order)
    perm = _permute(batch, order, n_pi)
    assert list(dp.verify_batch(perm.proofs, perm.proof_off, perm.instances, perm.committed, ws=ws)) == [got[i] for i in order]
    sample = sorted(random.Random(16).sample(range(n), 64))
    sb = _permute(batch, sample, n_pi)
    assert list(ov.verify_batch(sb.proofs, sb.proof_off, sb.instances, sb.committed, threads=16)) == [got[i] for i in sample]
    # the batch-accept fast path at the same size: the same vector (through the fall-back: the batch holds proofs that only
    # the pairing rejects); with the pairing-only rejects removed the batch check itself passes and nothing falls back
    got_rlc, fell_back = dp.verify_batch_rlc(batch.proofs, batch.proof_off, batch.instances, batch.committed, ws=ws)
    assert list(got_rlc) == list(got)
    keep = [i for i in range(n) if got[i] == 1 or i % 3 == 0]
    clean = _permute(batch, [i for i in keep if got[i] == 1], n_pi)
    # (a fresh workspace: the one above has just met a batch in which most groups of 64 failed and would ROUTE its next RLC
    #  calls straight to the per-proof kernels - include/h2v.h, ROUTING)
    ws2 = be.Workspace(dp, n)
    acc2, fb2 = dp.verify_batch_rlc(clean.proofs, clean.proof_off, clean.instances, clean.committed, ws=ws2)
    assert list(acc2) == [1] * clean.n and (not fb2 or name == "ivc") and (fell_back or name == "ivc")
    ws2.close()


def test_mixed_batch_of_two_plans_in_flight_on_one_device(be, circuits):
    """BASELINE configs[2] AS NAMED - "lookup_table + atms_with_lookups mixed batch, 1 x MI355X": two plans, two laned
    workspaces on one device in one process, 2048 proofs each (8 % corrupted, every corruption kind), the calls of the two
    plans interleaved on ONE caller stream with deferred joins, so that chunks of both plans are in flight on the shared pool
    of sixteen streams at the same time.  Before that the IVC and the sha256 plans have run on laned workspaces in the same
    process: the pool's queues have seen the kernels with the largest private segments (a queue's scratch arena is sized by
    the largest it has run - the one new failure class of round 3 was sixteen arenas that did not fit).  Verdicts == the
    construction for every call, == the oracle on a sample of each plan, and the RLC form of the same interleaving agrees."""
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    for name, m in (("ivc", 96), ("sha256", 160)):
        vk, td, pl, dp, ov = circuits[name]
        b = synth.forge_batch(vk, td, m, seed=31, plan=pl, workers=8)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.2, seed=32, kinds=list(synth.CORRUPTIONS))
        w_ = be.Workspace(dp, m, lanes=4, chunk=40)
        assert list(dp.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=w_)) == b.expected, name
        w_.close()
    n = 2048
    parts = []
    for k, name in enumerate(("lookup_table", "atms_with_lookups")):
        vk, td, pl, dp, ov = circuits[name]
        b = synth.forge_batch(vk, td, n, seed=500 + k, plan=pl, workers=8)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.08, seed=510 + k, kinds=list(synth.CORRUPTIONS))
        assert 0 < sum(b.expected) < n
        ws = be.Workspace(dp, n, lanes=0, chunk=0)      # the library's lanes and chunk for this plan
        ws.defer_joins(True)
        d = (up(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64).to(dev), up(b.instances), up(b.committed))
        parts.append((name, vk, pl, dp, ov, b, ws, d))
    s = torch.cuda.Stream(device=dev)
    rounds = 4
    for rlc in (False, True):
        accs = []
        for r in range(rounds):
            for (name, vk, pl, dp, ov, b, ws, d) in parts:
                acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
                st = torch.full((n,), -1, dtype=torch.int32, device=dev)
                if rlc:
                    dp.verify_batch_rlc_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream,
                                               seed=bytes(range(32)))
                else:
                    dp.verify_batch_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), acc.data_ptr(), st.data_ptr(), ws=ws, stream=s.cuda_stream)
                accs.append((name, b, acc, st))
        for part in parts:
            part[6].join(s.cuda_stream)
        s.synchronize()
        for name, b, acc, st in accs:
            assert acc.cpu().tolist() == b.expected, (name, rlc)
            assert [int(x == 0) for x in st.cpu().tolist()] == b.expected, (name, rlc)
    # the same interleaving on ONE workspace for both plans (h2v_workspace_create_multi: lanes sized for the larger of every
    # dimension - neither of these two plans fits a workspace made for the other); RLC mode: one parked set of buffers per plan
    # shape, and the record of every call stays readable although the lanes switch plans between chunks
    one = be.Workspace.multi([part[3] for part in parts], n)
    one.defer_joins(True)
    with pytest.raises(be.H2VError, match="smaller plan"):
        w_small = be.Workspace(parts[0][3], n, lanes=2, chunk=512)
        try:
            dp1, d1 = parts[1][3], parts[1][7]
            dp1.verify_batch_device(n, ptr(d1[0]), ptr(d1[1]), ptr(d1[2]), ptr(d1[3]), torch.zeros(n, dtype=torch.uint8, device=dev).data_ptr(), None, ws=w_small, stream=s.cuda_stream)
        finally:
            w_small.close()
    for rlc in (False, True):
        accs = []
        for r in range(3):
            for (name, vk, pl, dp, ov, b, ws, d) in parts:
                acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
                if rlc:
                    dp.verify_batch_rlc_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), acc.data_ptr(), None, ws=one, stream=s.cuda_stream, seed=bytes(range(32)))
                else:
                    dp.verify_batch_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), acc.data_ptr(), None, ws=one, stream=s.cuda_stream)
                accs.append((name, b, acc))
        one.join(s.cuda_stream)
        s.synchronize()
        for name, b, acc in accs:
            assert acc.cpu().tolist() == b.expected, (name, rlc, "multi")
        if rlc:
            for back in range(6):
                ok, tm = one.rlc_result(calls_back=back)
                assert not ok, back            # (8 % rejects: the batch check fails, or the call was routed past it - zeros then)
        else:
            for back in range(6):
                assert one.timings(back).pairing_ms > 0
    one.close()
    for (name, vk, pl, dp, ov, b, ws, d) in parts:
        sample = sorted(random.Random(17).sample(range(n), 48))
        sb = _permute(b, sample, vk.n_public_inputs)
        assert list(ov.verify_batch(sb.proofs, sb.proof_off, sb.instances, sb.committed, threads=16)) == [b.expected[i] for i in sample], name
        ws.close()


def test_circuit_without_public_inputs(be):
    """n_public_inputs == 0 with a queried instance column (the Lagrange sum is empty) and instances == NULL at the ABI."""
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V
    from oracle import binding as orc
    adv = [[0, 1]] * 2 + [[0]] * 1
    vk, td = V._shaped_vk("nopi", 77, k=8, degree=4, n_adv=3, n_fix=4, n_cc=3, lookup_arg_exprs=[], gate_exprs=2,
                          gate_ops={"mul": 6, "add": 4, "neg": 1}, adv_rot_sets=adv, n_pi=0, n_ci=0)
    pl = PL.compile_plan(vk)
    ov = orc.OracleVK(orc.vk_desc(json.loads(vk.to_json()), vk.omega, vk.omega_inv, vk.barycentric_weight))
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    b = synth.forge_batch(vk, td, 20, seed=3, plan=pl, workers=1)
    b = synth.with_rejects(pl, b, 0, fraction=0.4, seed=2, kinds=["flip_first_scalar", "wrong_pi", "point_not_on_curve"])
    got = dp.verify_batch(b.proofs, b.proof_off, b"", None)
    assert list(got) == list(ov.verify_batch(b.proofs, b.proof_off, b"", None, threads=4)) == b.expected
    assert 0 < sum(got) < 20


# (option id, value) pairs of h2v_workspace_set_option + the fixed-base window width of h2v_plan_load_ex: every launch-shape
# dimension that used to be an H2V_* environment variable read once per process (round 3: seventeen child processes)
_O = dict(tpl=1, pairing=2, streams=3, lpt=4, bs=5, fix=6, vm=7, vm_p=8, rlc_grp=11, rlc_c=12, rlc_chain=13)
_MODES = [dict(pairing=1), dict(lpt=1), dict(lpt=2, bs=256), dict(fix=1), dict(fix=3),
          dict(fix=2, fix_c=4), dict(fix=1, fix_c=8), dict(fix=-1), dict(vm=2), dict(vm=1), dict(tpl=2), dict(tpl=4), dict(pairing=32), dict(pairing=64),
          dict(pairing=16), dict(pairing=12), dict(pairing=6), dict(vm_p=8), dict(streams=0), dict(streams=1), dict(streams=2)]


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: ",".join("%s=%s" % kv for kv in m.items()))
def test_alternate_pipeline_modes(be, circuits, mode):
    """Every launch-shape option of h2v_workspace_set_option (every pairing engine incl. the one-lane cross-check kernel,
    the MSM launch shape - lanes per term, block size, terms per lane, fixed-base lanes for the VK bases with all-window
    tables of 12- (default), 8- or 4-bit windows -, the narrow / wide schedule of the combiner, the stream layout)
    IN-PROCESS, on three circuits: the same verdicts as the construction.  The launcher would otherwise pick these from
    the batch size.  The retired ids 9 and 10 are refused."""
    from plutus_halo2_verifier_gen_amd import synth
    for name in ("simple_mul", "ivc", "lookup_table"):
        vk, td, pl, dp0, ov = circuits[name]
        dp = be.DevicePlan(pl.to_bytes(), 0, fixed_base_window_bits=mode["fix_c"]) if "fix_c" in mode else dp0
        b = synth.forge_batch(vk, td, 150, seed=4, plan=pl, workers=2)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.3, seed=6, kinds=list(synth.CORRUPTIONS))
        ws = be.Workspace(dp, 150)
        for k, v in mode.items():
            if k != "fix_c":
                ws.set_option(_O[k], v)
                assert ws.get_option(_O[k]) == v
        got = dp.verify_batch(b.proofs, b.proof_off, b.instances, b.committed, ws=ws)
        assert list(got) == b.expected and 0 < sum(got) < 150, (name, mode)
        tm = ws.timings()
        if "pairing" in mode:
            assert tm.pairing_lanes_per_proof == mode["pairing"], (name, mode, tm.pairing_lanes_per_proof)
        if mode.get("fix", 0) > 0 and name != "ivc":
            assert tm.msm_lanes_per_term == 3 and tm.g1_msm_fixed_ms > 0, (name, mode)
        if mode.get("fix", 0) < 0:
            assert tm.msm_lanes_per_term != 3
        got_rlc, _fb = dp.verify_batch_rlc(b.proofs, b.proof_off, b.instances, b.committed, ws=ws, seed=bytes(range(32)))
        assert list(got_rlc) == b.expected, (name, mode, "rlc")
        ws.close()
        if dp is not dp0:
            dp.close()
    with pytest.raises(be.H2VError):
        w_ = be.Workspace(circuits["simple_mul"][3], 8)
        w_.set_option(_O["bs"], 100)
    w_ = be.Workspace(circuits["simple_mul"][3], 8)
    for retired in (9, 10):
        for v in (0, 1, 2):
            with pytest.raises(be.H2VError):
                w_.set_option(retired, v)
        with pytest.raises(be.H2VError):
            w_.get_option(retired)
        with pytest.raises(be.H2VError):
            be.probe_set_option(retired, 0)
    w_.close()


def test_debug_sync_path_in_a_child_process(be):
    """H2V_DEBUG_SYNC (one of the four debug variables that stay): the serialised pipeline that names every kernel; read once
    per process, so it runs in a child."""
    import os
    import subprocess
    import sys
    script = (
        "import sys; sys.path.insert(0, %r)\n"
        "from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V\n"
        "for name in ('simple_mul', 'ivc'):\n"
        "    vk, td = V.BUILDERS[name]()\n"
        "    pl = PL.compile_plan(vk)\n"
        "    b = synth.forge_batch(vk, td, 70, seed=4, plan=pl, workers=1)\n"
        "    b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.3, seed=6, kinds=list(synth.CORRUPTIONS))\n"
        "    got = backend.DevicePlan(pl.to_bytes(), 0).verify_batch(b.proofs, b.proof_off, b.instances, b.committed)\n"
        "    assert list(got) == b.expected and 0 < sum(got) < 70, name\n"
        "print('modes ok')\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, "H2V_DEBUG_SYNC": "1"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "modes ok" in r.stdout and "launching k_g1_msm" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_small_calls_are_coalesced(be, circuits):
    """include/h2v.h, COALESCING: small calls on a deferring laned workspace are gathered into one launch per kernel (RLC calls: one
    batch check per group).
    Sequences of calls of 1 .. chunk / 2 proofs (every corruption kind among them, so ragged lengths too; proof bytes at odd
    device addresses), two plans interleaved (a change of plan runs the open group), a large call and an RLC call in between,
    joins on a stream and on the host: accept[] AND status[] of every call equal the construction and what the same calls give
    with H2V_OPT_COALESCE = -1; h2v_workspace_timings of a coalesced call reports its share of the group's launch."""
    import torch
    from plutus_halo2_verifier_gen_amd import synth
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    rng = random.Random(99)
    pools = {}
    for name in ("simple_mul", "sha256"):
        vk, td, pl, dp, ov = circuits[name]
        b = synth.forge_batch(vk, td, 400, seed=81, plan=pl, workers=8)
        pools[name] = (vk, pl, dp, synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.15, seed=82, kinds=list(synth.CORRUPTIONS)))
    # the calls: (plan, indices into its pool, kind)
    calls = []
    for k in range(40):
        name = rng.choice(list(pools))
        n = rng.choice([1, 2, 7, 33, 64, 100, 128, 200])
        calls.append((name, [rng.randrange(400) for _ in range(n)], "small" if rng.random() < 0.6 else "rlc"))   # (RLC calls are gathered among themselves)
        if k == 13:
            calls.append(("simple_mul", [rng.randrange(400) for _ in range(900)], "large"))
        if k == 27:
            calls.append(("simple_mul", [rng.randrange(400) for _ in range(150)], "rlc"))
    results = {}
    for coalesce in (0, -1):
        wss = {name: be.Workspace(pools[name][2], 1024, lanes=0, chunk=512) for name in pools}
        for w in wss.values():
            w.defer_joins(True)
            w.set_option(be.OPT_COALESCE, coalesce)
            assert w.get_option(be.OPT_COALESCE) == coalesce
        held = []
        for ci_, (name, idx, kind) in enumerate(calls):
            vk, pl, dp, pool = pools[name]
            b = _permute(pool, idx, vk.n_public_inputs)
            raw = torch.frombuffer(bytearray(b"\x00" * (1 + ci_ % 3) + b.proofs), dtype=torch.uint8).to(dev)   # proof bytes at an odd address now and then
            dpr = raw[1 + ci_ % 3:]
            dof = torch.tensor(b.proof_off, dtype=torch.int64).to(dev)
            din = torch.frombuffer(bytearray(b.instances), dtype=torch.uint8).to(dev) if b.instances else None
            dci = torch.frombuffer(bytearray(b.committed), dtype=torch.uint8).to(dev) if b.committed else None
            acc = torch.full((b.n,), 7, dtype=torch.uint8, device=dev)
            st = torch.full((b.n,), -1, dtype=torch.int32, device=dev)
            args = (b.n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr() if din is not None else None, dci.data_ptr() if dci is not None else None, acc.data_ptr(), st.data_ptr())
            if kind == "rlc":
                dp.verify_batch_rlc_device(*args, ws=wss[name], stream=s.cuda_stream, seed=bytes(range(32)))
            else:
                dp.verify_batch_device(*args, ws=wss[name], stream=s.cuda_stream)
            held.append((name, b, acc, st, (raw, dof, din, dci), kind))
            if ci_ == 20:                     # a join in the middle, on the host: everything so far is final
                for w in wss.values():
                    w.join(None)
                for name_, b_, acc_, st_, _k, kind_ in held:
                    assert acc_.cpu().tolist() == b_.expected, (coalesce, name_, kind_)
        if coalesce == 0 and calls[-1][2] != "large":     # the last small call's group is still open: no record of it yet
            with pytest.raises(be.H2VError, match="has not run yet"):
                (wss[calls[-1][0]].rlc_result(0) if calls[-1][2] == "rlc" else wss[calls[-1][0]].timings(0))
        for w in wss.values():
            w.join(s.cuda_stream)
        s.synchronize()
        out = []
        for name, b, acc, st, _keep, kind in held:
            assert acc.cpu().tolist() == b.expected, (coalesce, name, b.n, kind)
            assert [int(x == 0) for x in st.cpu().tolist()] == b.expected, (coalesce, name, kind)
            out.append((acc.cpu().tolist(), st.cpu().tolist()))
        results[coalesce] = out
        # the last call was a small one: its record is a share of its group's launch (or of its group's batch check)
        if calls[-1][2] == "rlc":
            ok_, tm = wss[calls[-1][0]].rlc_result(0)
            assert tm.g1_decompress_ms > 0 or not ok_
        else:
            tm = wss[calls[-1][0]].timings(0)
            assert tm.pairing_ms > 0 and tm.g1_decompress_ms > 0
        for w in wss.values():
            w.close()
    assert results[0] == results[-1]
    # more plans and modes than lanes: a workspace of TWO lanes serving three plans, per proof and RLC alternating - six kinds of
    # group, at most two of them open at a time (the soak met a three-lane workspace whose fifth group was opened on a lane that
    # still held one: the calls of the overwritten group were never run)
    pools["lookup_table"] = (circuits["lookup_table"][0], circuits["lookup_table"][2], circuits["lookup_table"][3],
                             synth.with_rejects(circuits["lookup_table"][2], synth.forge_batch(circuits["lookup_table"][0], circuits["lookup_table"][1], 120, seed=83,
                                                                                            plan=circuits["lookup_table"][2], workers=8),
                                                circuits["lookup_table"][0].n_public_inputs, fraction=0.15, seed=84, kinds=list(synth.CORRUPTIONS)))
    two = be.Workspace.multi([pools[k][2] for k in pools], 512, lanes=2)
    two.defer_joins(True)
    held = []
    for k in range(18):
        name = list(pools)[k % 3]
        vk, pl, dp, pool = pools[name]
        b = _permute(pool, [rng.randrange(pool.n) for _ in range(40 + k)], vk.n_public_inputs)
        dpr = torch.frombuffer(bytearray(b.proofs), dtype=torch.uint8).to(dev)
        dof = torch.tensor(b.proof_off, dtype=torch.int64).to(dev)
        din = torch.frombuffer(bytearray(b.instances), dtype=torch.uint8).to(dev) if b.instances else None
        dci = torch.frombuffer(bytearray(b.committed), dtype=torch.uint8).to(dev) if b.committed else None
        acc = torch.full((b.n,), 7, dtype=torch.uint8, device=dev)
        args = (b.n, dpr.data_ptr(), dof.data_ptr(), din.data_ptr() if din is not None else None, dci.data_ptr() if dci is not None else None, acc.data_ptr(), None)
        if (k // 3) % 2:
            dp.verify_batch_rlc_device(*args, ws=two, stream=s.cuda_stream, seed=bytes(range(32)))
        else:
            dp.verify_batch_device(*args, ws=two, stream=s.cuda_stream)
        held.append((name, b, acc, (dpr, dof, din, dci)))
    two.join(s.cuda_stream)
    s.synchronize()
    for name, b, acc, _keep in held:
        assert acc.cpu().tolist() == b.expected, ("two lanes, three plans", name, b.n)
    two.close()


def test_threads_sharing_plans_and_the_stream_pool(be):
    """include/h2v.h: a plan "may be shared by threads (each with its own workspace)".  Three host threads for twenty seconds
    through tests/soak.py (its own process: it ends with h2v_shutdown): random circuits, sizes, reject mixes and calling forms -
    host buffers, submit / wait streams, device pointers with deferred joins, RLC, forced launch shapes, randomly mutated proofs
    judged by the oracle - every accept vector as constructed.  (Minutes of the same on four threads: profiles/r04_soak_*.log;
    it found the download-block overrun that test_rlc_host_batches_growing_into_the_download_block_slack pins.)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "soak.py"), "--minutes", "0.33", "--threads", "3", "--circuits", "simple_mul,lookup_table,ivc,trashcan_mix",
                        "--max-n", "2048"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "every verdict as constructed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_tuned_shapes_are_measured_not_guessed(be, circuits):
    """h2v_workspace_tune: for the five BASELINE shapes at reduced sizes and two shapes no rule was calibrated on (T = 25 x 3000,
    T = 44 x 700), on laned workspaces with deferred joins: the tuner leaves a configuration whose measured time is at most the
    launcher's own choice's, re-measuring EVERY engine by force afterwards finds nothing more than 3 % (+ noise allowance) faster,
    and the verdicts under the tuned options are the construction's."""
    import time
    import torch
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    dev = torch.device("cuda", 0)
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    shapes = [("simple_mul", 4096), ("lookup_table", 2048), ("atms_with_lookups", 2048), ("sha256", 1024), ("secp256k1", 512)]
    extra = []
    for nm, seed, n_adv, n_fix, n_cc, n in (("t25", 91, 4, 5, 4, 3000), ("t44", 92, 8, 15, 7, 700)):
        adv = [[0, 1]] * 2 + [[0]] * (n_adv - 2)
        vk, td = V._shaped_vk(nm, seed, k=10, degree=4, n_adv=n_adv, n_fix=n_fix, n_cc=n_cc, lookup_arg_exprs=[2], gate_exprs=3,
                              gate_ops={"mul": 20, "add": 12, "neg": 2}, adv_rot_sets=adv, n_pi=2, n_ci=0)
        extra.append((nm, vk, td, n))
    s = torch.cuda.Stream(device=dev)
    seen_terms = []
    for item in shapes + extra:
        if len(item) == 2:
            name, n = item
            vk, td, pl, dp, ov = circuits[name]
        else:
            name, vk, td, n = item
            pl = PL.compile_plan(vk)
            dp = be.DevicePlan(pl.to_bytes(), 0)
        seen_terms.append(pl.n_terms)
        b = synth.forge_batch(vk, td, n, seed=33, plan=pl, workers=8)
        b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.05, seed=34, kinds=list(synth.CORRUPTIONS))
        d = (up(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64).to(dev), up(b.instances), up(b.committed))
        ws = be.Workspace(dp, n, lanes=0, chunk=0)
        ws.defer_joins(True)
        rep = ws.tune(dp, n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), s.cuda_stream)
        assert rep.n_measured >= 3 and rep.best_ms <= rep.default_ms and rep.best_ms > 0
        assert ws.get_option(be.OPT_PAIRING_ENGINE) == rep.pairing_engine and ws.get_option(be.OPT_MSM_TERMS_PER_LANE) == rep.msm_terms_per_lane
        depth = ws.depth(n)

        def ms_per_call(rounds=3):
            accs = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(depth)]
            for a in accs:
                dp.verify_batch_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), a.data_ptr(), None, ws=ws, stream=s.cuda_stream)
            ws.join(s.cuda_stream); s.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                for a in accs:
                    dp.verify_batch_device(n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), a.data_ptr(), None, ws=ws, stream=s.cuda_stream)
            ws.join(s.cuda_stream); s.synchronize()
            return (time.perf_counter() - t0) / (rounds * depth) * 1e3, accs

        tuned_ms, accs = ms_per_call()
        for a in accs:
            assert a.cpu().tolist() == b.expected, name
        forced = {}
        for eng in (6, 12, 16, 32):
            ws.set_option(be.OPT_PAIRING_ENGINE, eng)
            forced[eng], accs = ms_per_call()
            assert accs[0].cpu().tolist() == b.expected, (name, eng)
        # the tuned configuration once more after the forced ones (the first figure of a series has been seen 25 % off the later
        # ones); wall-clock re-measurements of a few milliseconds each: 3 % + 7 % of noise allowance
        ws.set_option(be.OPT_PAIRING_ENGINE, rep.pairing_engine)
        tuned_ms = min(tuned_ms, ms_per_call()[0])
        assert tuned_ms <= min(forced.values()) * 1.10, (name, n, tuned_ms, forced, rep.pairing_engine, rep.msm_terms_per_lane, rep.default_ms, rep.best_ms)
        ws.close()
    assert 25 in seen_terms and 44 in seen_terms


def test_shutdown_releases_the_pool_and_refuses_further_calls(be):
    """h2v_shutdown (include/h2v.h: library lifecycle), in a child process: a laned workspace with deferred joins has chunks
    in flight on the library's pool streams; shutdown waits for them, releases workspace and plan, destroys the streams;
    the verdicts written before it are intact; every further call is H2V_E_DEVICE (-3), the handles are freed as usual, a
    second shutdown is a no-op and the process exits 0 (the exit-time crash of round 3 was a pool stream that outlived
    the runtime)."""
    import os
    import subprocess
    import sys
    script = (
        "import sys; sys.path.insert(0, %r)\n"
        "import ctypes as C, torch\n"
        "from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V\n"
        "vk, td = V.simple_mul_vk()\n"
        "pl = PL.compile_plan(vk)\n"
        "b = synth.forge_batch(vk, td, 96, seed=4, plan=pl, workers=1)\n"
        "b = synth.with_rejects(pl, b, vk.n_public_inputs, fraction=0.3, seed=6, kinds=list(synth.CORRUPTIONS))\n"
        "dev = torch.device('cuda', 0)\n"
        "dp = backend.DevicePlan(pl.to_bytes(), 0)\n"
        "ws = backend.Workspace(dp, 96, lanes=4, chunk=16)\n"
        "ws.defer_joins(True)\n"
        "t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)\n"
        "dpr, dof, din = t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64).to(dev), t(b.instances)\n"
        "acc = [torch.zeros(96, dtype=torch.uint8, device=dev) for _ in range(3)]\n"
        "st = torch.cuda.Stream(device=dev)\n"
        "for a in acc:\n"
        "    dp.verify_batch_device(96, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None, a.data_ptr(), None, ws=ws, stream=st.cuda_stream)\n"
        "backend.shutdown(0)          # no join before it: the chunks are still in flight\n"
        "torch.cuda.synchronize()\n"
        "for a in acc:\n"
        "    assert a.cpu().tolist() == b.expected\n"
        "L = backend.lib()\n"
        "bb = backend.Batch(96, dpr.data_ptr(), dof.data_ptr(), din.data_ptr(), None)\n"
        "assert L.h2v_verify_batch_device(dp.handle, C.byref(bb), acc[0].data_ptr(), None, ws.handle, None, None) == -3\n"
        "assert b'h2v_shutdown' in L.h2v_last_error()\n"
        "assert L.h2v_workspace_join(ws.handle, None) == -3\n"
        "h = C.c_void_p()\n"
        "assert L.h2v_workspace_create(dp.handle, 8, C.byref(h)) == -3\n"
        "raw = pl.to_bytes()\n"
        "assert L.h2v_plan_load(raw, len(raw), 0, C.byref(h)) == -3\n"
        "assert dp.proof_len == pl.proof_len       # host-side facts survive\n"
        "backend.shutdown(-1)\n"
        "ws.close(); dp.close()\n"
        "print('shutdown ok')\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "shutdown ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("lpt", ["1", "2", "8", "tpl2", "tpl3", "tpl4"])
def test_g1_msm_forced_shape(be, orc, lpt):
    """test_g1_msm (edge scalars, equal / opposite / infinity bases, T = 1 .. 64) again with the MSM shape forced through
    h2v_probe_set_option (in-process): the probe's small batches would otherwise always take two lanes per term.  tpl2 / tpl4:
    several terms per lane on one accumulator (k_g1_msm_multi*), where equal and opposite bases exercise the Z test and the
    complete redo - but only in windows 32 and 31, on the second term's slots, in lane 0 and with 4, 6 or 8 halves per lane
    (tests/test_multi_ladder_model.py replays these inputs); every other position and the odd lane shapes:
    tests/test_msm_multi_ladder_gpu.py."""
    opt, val = (be.OPT_MSM_TERMS_PER_LANE, int(lpt[3:])) if lpt.startswith("tpl") else (be.OPT_MSM_LANES_PER_TERM, int(lpt))
    be.probe_set_option(opt, val)
    try:
        test_g1_msm(be, orc)
    finally:
        be.probe_set_option(opt, 0)