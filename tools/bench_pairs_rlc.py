#!/usr/bin/env python3
"""Throughput of the batch-accept pair check (h2v_check_pairs_rlc_device: two bucket MSMs and ONE pairing per batch, the
per-pair kernels only behind a failed check) against the pair check it stands in for (h2v_check_pairs_device), and - for
recursive keys - of verify with H2V_RLC_FOLD_PAIRS against per-proof verify.  Set up as tools/bench_prepare.py: inputs resident
on the device, one laned workspace with deferred joins and one caller stream, warm-up on every lane, three device-synchronised
windows of at least --seconds per kind, all kinds in one run, correctness asserted before timing.
Kinds per case: check (h2v_check_pairs_device on all-valid pairs: the comparison base), rlc_valid (the batch check on the same
pairs), rlc_one (one failing pair per batch), rlc_tenth (the pairs of a batch with a seeded tenth of rejects, pre-pairing and
pairing-only kinds); recursive keys also verify / fold_valid and verify_one / fold_one.  Reported per kind: the best window and
the spread (max - min) / max of the three; a gain counts only when it exceeds the larger spread of the two kinds compared.
Writes one JSON line per case and, with --out, the whole set as one JSON file.
--multi-srs S[,S..] (a mode of its own: nothing of the above runs): ONE h2v_check_pairs_multi_device call over pairs on S SRS
against the S h2v_check_pairs_rlc_device calls, one per SRS, that it stands in for - same pairs, same ordinary workspace, one
stream, one process.  Per S two shapes: S pairs in all, one per SRS (what an Aggregator holds), and 4096 pairs in all.  Both
routes warmed, a given seed, five alternating runs of at least --seconds (0.5) each; every run's ms per window (one window = the
whole list checked once) goes to --out (profiles/pairs_multi_srs.json).  A gain is stated only when the slowest run of the new
call beats the fastest run of the baseline.
usage: bench_pairs_rlc.py [--seconds 1.0] [--warmup 5] [--repeats 3] [--cases simple_mul:4096,sha256:1024,bls12381:1024,ivc:1024]
                          [--out profiles/pairs_rlc.json]
       bench_pairs_rlc.py --multi-srs 2,4,8 [--seconds 0.5] [--out profiles/pairs_multi_srs.json]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DEFAULT_CASES = "simple_mul:4096,sha256:1024,bls12381:1024,ivc:1024"
KINDS = ["bad_point_flag", "point_not_in_subgroup", "noncanonical_scalar", "wrong_pi", "wrong_public_input"]


def run_case(name, B, seconds, warmup, repeats):
    import torch
    from plutus_halo2_verifier_gen_amd import backend, bls12_381 as bls, plan as PL, synth, vk as V
    build = V.WIDE_BUILDERS.get(name) or V.BUILDERS[name]
    vk, td = build()
    pl = PL.compile_plan(vk)
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    clean = synth.forge_batch(vk, td, B, seed=1, plan=pl, workers=16, ci_identity=(name == "sha256"))
    tenth = synth.with_rejects(pl, clean, vk.n_public_inputs, fraction=0.1, seed=2, kinds=KINDS)
    # one reject per batch: proof B / 2 with another pi commitment (caught by the pairing alone; the proof keeps its length)
    k_bad = B // 2
    raw = bytearray(clean.proofs)
    o = clean.proof_off[k_bad] + pl.points[pl.pi_point]
    raw[o:o + 48] = bls.g1_compress(bls.g1_mul(bls.G1_GEN, random.Random(3).randrange(1, bls.R)))
    one = synth.Batch(n=B, proofs=bytes(raw), proof_off=clean.proof_off, instances=clean.instances, committed=clean.committed,
                      expected=[0 if i == k_bad else 1 for i in range(B)])
    dev = torch.device("cuda", 0)
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda t: t.data_ptr() if t is not None else None

    def resident(b):
        keep = (t8(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64).to(dev), t8(b.instances), t8(b.committed))
        return keep, (B,) + tuple(ptr(x) for x in keep)

    data = {"valid": resident(clean), "one": resident(one), "tenth": resident(tenth)}
    expected = {"valid": clean.expected, "one": one.expected, "tenth": tenth.expected}
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws = backend.Workspace(dp, B, lanes=0, chunk=0)       # the laned workspace bench.py uses
    ws.defer_joins(True)
    n_lanes = ws.lanes()[0]
    K = 16
    acc = [torch.zeros(B, dtype=torch.uint8, device=dev) for _ in range(K)]
    st = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(K)]
    pairs = {k: torch.zeros(B * 96, dtype=torch.uint8, device=dev) for k in data}
    seed = bytes(range(32))      # (given, so that runs repeat; the call counter still changes the coefficients of every call)

    def sync():
        ws.join(cs)
        torch.cuda.synchronize()

    # the pairs of the three inputs, and correctness on them: both pair checks == verify == the construction
    for k, (_keep, args) in data.items():
        dp.verify_batch_device(*args, acc[0].data_ptr(), st[0].data_ptr(), ws=ws, stream=cs)
        dp.prepare_batch_device(*args, pairs[k].data_ptr(), st[1].data_ptr(), ws=ws, stream=cs)
        sync()
        dp.check_pairs_device(B, pairs[k].data_ptr(), acc[1].data_ptr(), st[1].data_ptr(), ws=ws, stream=cs)
        dp.check_pairs_rlc_device(B, pairs[k].data_ptr(), acc[2].data_ptr(), st[2].data_ptr(), ws=ws, stream=cs, seed=seed)
        sync()
        assert acc[0].cpu().tolist() == acc[1].cpu().tolist() == acc[2].cpu().tolist() == expected[k], (name, k)
        assert st[1].cpu().tolist() == st[2].cpu().tolist(), (name, k)
        assert ws.rlc_result(timings=False)[0] == (k == "valid"), (name, k)
        if pl.is_recursive:
            dp.verify_batch_rlc_device(*args, acc[3].data_ptr(), st[3].data_ptr(), ws=ws, stream=cs, seed=seed, fold_pairs=True)
            sync()
            assert acc[3].cpu().tolist() == expected[k] and st[3].cpu().tolist() == st[0].cpu().tolist(), (name, k)
            assert ws.rlc_result(timings=False)[0] == (k == "valid"), (name, k)

    def step(kind, k):
        k %= K
        a, s = acc[k].data_ptr(), st[k].data_ptr()
        if kind == "check":
            dp.check_pairs_device(B, pairs["valid"].data_ptr(), a, s, ws=ws, stream=cs)
        elif kind.startswith("rlc_"):
            dp.check_pairs_rlc_device(B, pairs[kind[4:]].data_ptr(), a, s, ws=ws, stream=cs, seed=seed)
        elif kind.startswith("verify"):
            dp.verify_batch_device(*data["one" if kind.endswith("_one") else "valid"][1], a, s, ws=ws, stream=cs)
        else:
            dp.verify_batch_rlc_device(*data[kind[5:]][1], a, s, ws=ws, stream=cs, seed=seed, fold_pairs=True)

    def window(kind, k_steps):
        t0 = time.perf_counter()
        for k in range(k_steps):
            step(kind, k)
        sync()
        return time.perf_counter() - t0

    kinds = ["check", "rlc_valid", "rlc_one", "rlc_tenth"] + (["verify", "fold_valid", "verify_one", "fold_one"] if pl.is_recursive else [])
    rates = {k: [] for k in kinds}
    for kind in kinds:                                   # warm-up of every kind on every lane (first uses allocate)
        for k in range(max(warmup, n_lanes)):
            step(kind, k)
        sync()
    for _ in range(repeats):
        for kind in kinds:
            per_step = window(kind, 2 * n_lanes) / (2 * n_lanes)       # (untimed calibration)
            steps = max(2 * n_lanes, int(1.25 * seconds / per_step) + 1)
            el = window(kind, steps)
            rates[kind].append(steps * B / el)
    # kernel times of one batch check alone (nothing else in flight): what h2v_workspace_rlc_result reports
    step("rlc_valid", 0)
    sync()
    _ok, tm = ws.rlc_result()
    times = {f: round(getattr(tm, f), 4) for f in ("g1_decompress_ms", "prepare_ms", "bucket_sort_ms", "bucket_accumulate_ms",
                                                    "bucket_reduce_ms", "pairing_ms", "total_ms")}
    best = {k: max(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / max(v), 4) for k, v in rates.items()}
    out = {"circuit": name, "batch": B, "lanes": n_lanes, "rejects_in_tenth": B - sum(tenth.expected),
           "per_s": {k: round(v, 1) for k, v in best.items()}, "spread": spread,
           "rlc_valid_over_check": round(best["rlc_valid"] / best["check"], 3),
           "rlc_one_over_check": round(best["rlc_one"] / best["check"], 3),
           "rlc_tenth_over_check": round(best["rlc_tenth"] / best["check"], 3),
           "rlc_valid_gain_exceeds_spread": best["rlc_valid"] / best["check"] - 1.0 > max(spread["rlc_valid"], spread["check"]),
           "rlc_valid_times_one_chunk_alone": times,
           "runs": {k: [round(x, 1) for x in v] for k, v in rates.items()}, "outputs_equal": True}
    if pl.is_recursive:
        out["fold_valid_over_verify"] = round(best["fold_valid"] / best["verify"], 3)
        out["fold_one_over_verify_one"] = round(best["fold_one"] / best["verify_one"], 3)
        out["fold_valid_gain_exceeds_spread"] = best["fold_valid"] / best["verify"] - 1.0 > max(spread["fold_valid"], spread["verify"])
    ws.close()
    dp.close()
    return out


def run_multi_srs(S, total, seconds, runs=5):
    """one shape: `total` valid pairs spread evenly over S SRS; returns the ms per window of every run of both routes"""
    import torch
    from plutus_halo2_verifier_gen_amd import backend, bls12_381 as bls, plan as PL, vk as V
    per = total // S
    assert per >= 1 and per * S == total
    plans, raws = [], []
    for q in range(S):
        s = (0x5a17 + q) << 64 | (11 + q)
        vk, _td = V.on_srs(*V.simple_mul_vk(seed=1 + q), s)
        plans.append(backend.DevicePlan(PL.compile_plan(vk).to_bytes(), 0))
        a, d = bls.g1_mul(bls.G1_GEN, 1000 + q), bls.g1_mul(bls.G1_GEN, 77)
        sa, sd = bls.g1_mul(a, s), bls.g1_mul(d, s)
        out = []
        for _ in range(per):
            out.append(bls.g1_compress(a) + bls.g1_compress(sa))
            a, sa = bls.g1_add(a, d), bls.g1_add(sa, sd)
        raws.append(b"".join(out))
    dev = torch.device("cuda", 0)
    pairs = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev)
    acc = torch.zeros(total, dtype=torch.uint8, device=dev)
    st = torch.zeros(total, dtype=torch.int32, device=dev)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws = backend.Workspace(plans[0], max(total, 64))
    seed = bytes(range(32))
    counts = [per] * S

    def multi():
        backend.check_pairs_multi_device(plans, counts, pairs.data_ptr(), acc.data_ptr(), st.data_ptr(), ws=ws, stream=cs, seed=seed)

    def per_srs():
        for q in range(S):
            plans[q].check_pairs_rlc_device(per, pairs.data_ptr() + 96 * per * q, acc.data_ptr() + per * q, st.data_ptr() + 4 * per * q, ws=ws,
                                            stream=cs, seed=seed)

    def window(route, k):
        t0 = time.perf_counter()
        for _ in range(k):
            route()
        caller.synchronize()
        return time.perf_counter() - t0

    for route in (multi, per_srs):                      # correctness and warm-up (first uses allocate)
        acc.zero_()
        route()
        caller.synchronize()
        assert acc.cpu().tolist() == [1] * total and st.cpu().tolist() == [0] * total and ws.rlc_result(timings=False)[0]
        window(route, 5)
    ms = {"multi": [], "per_srs": []}
    for _ in range(runs):                               # alternating
        for name, route in (("multi", multi), ("per_srs", per_srs)):
            per_window = window(route, 8) / 8           # (untimed calibration)
            k = max(8, int(seconds / per_window) + 1)
            ms[name].append(round(1e3 * window(route, k) / k, 4))
    ws.close()
    for p in plans:
        p.close()
    return {"srs": S, "pairs": total, "ms_per_window": ms, "gain": max(ms["multi"]) < min(ms["per_srs"]),
            "loss": min(ms["multi"]) > max(ms["per_srs"]), "fastest_baseline_over_slowest_new": round(min(ms["per_srs"]) / max(ms["multi"]), 3)}


def main_multi_srs(args):
    import torch
    results = []
    for S in [int(v) for v in args.multi_srs.split(",")]:
        for total in (S, 4096):
            r = run_multi_srs(S, total, args.seconds if args.seconds_given else 0.5)
            print(json.dumps(r), flush=True)
            results.append(r)
    out = args.out or os.path.join(ROOT, "profiles", "pairs_multi_srs.json")
    with open(out, "w") as f:
        json.dump({"tool": "tools/bench_pairs_rlc.py --multi-srs " + args.multi_srs, "device": torch.cuda.get_device_name(0),
                   "window": "the whole list checked once: one h2v_check_pairs_multi_device call (multi) / S h2v_check_pairs_rlc_device calls (per_srs)",
                   "runs": 5, "rule": "a gain only if the slowest run of multi beats the fastest run of per_srs", "shapes": results}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi-srs", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.seconds_given = any(a.startswith("--seconds") for a in sys.argv[1:])
    if args.multi_srs:
        return main_multi_srs(args)
    import torch
    results = []
    for c in args.cases.split(","):
        name, B = c.split(":")
        r = run_case(name, int(B), args.seconds, args.warmup, args.repeats)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_pairs_rlc.py", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
                       "repeats": args.repeats, "cases": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
