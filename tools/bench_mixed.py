#!/usr/bin/env python3
"""The mixed-key call (h2v_verify_mixed_device) against today's route for the same proofs, in ONE process, alternating:
  (a) new:      one call per step on a multi-plan workspace;
  (b) baseline: the same workspace kind with deferred joins, one per-key call per key and step on one caller stream, joined
                at the end of the run (the form tests/test_gpu_parity.py::test_mixed_batch_of_two_plans_in_flight_on_one_device
                drives: the parent's behaviour).
Both modes (per proof, batch-accept), for two shapes on one SRS (vk.on_srs):
  two      lookup_table x 2048 + atms_with_lookups x 2048 (BASELINE configs[2])
  sixteen  16 keys x 64 proofs: simple_mul, lookup_table, trashcan_mix, atms_with_lookups under four seeds each
All proofs accept (the batch-accept mode is measured where it is meant to be used); before timing, both routes must accept
everything.  Every run is `--steps` steps between two device synchronisations; runs alternate new / baseline, `--runs` each.
A gain is claimed only when the slowest new run beats the fastest baseline run.  --cache DIR keeps the forged batches (forging
is CPU work).  Writes one JSON line per (shape, mode) and, with --out, the whole set.
--fold adds a third route to the batch-accept mode and measures that mode alone:
  (c) fold:     the call of (a) with H2V_MIXED_FOLD_MSM - one bucket MSM over the call's per-proof terms and one pairing; it
                synchronises the caller's stream once per call (the verdict comes back to the host).
The three routes alternate (c), (a), (b), `--runs` each, in this one process; the fold form gains on a shape only when its
slowest run beats the fastest run of (a) AND of (b), and loses when its fastest run is behind the slowest of either.
--fold --grouped measures H2V_MIXED_GROUPED (phase 1 of every key in one launch per kernel), batch-accept mode, all-accepting batches:
  (a) grouped:  the fold call with H2V_MIXED_GROUPED;
  (b) fold:     the same call without it (the parent's route, same build) - not for shapes of more than 64 keys, which it cannot take;
  (c) per key:  one h2v_verify_batch_rlc call per key and step (deferred joins, one caller stream).
Shapes sixteen (16 x 64), sixtyfour (64 keys x 16), twofiftysix (256 keys x 4: (a) and (c) only), two (2 x 2048); every shape is
warmed, the routes alternate (a), (b), (c), `--runs` each.  A gain or a loss of (a) over a route is claimed only when its slowest run
is ahead of that route's fastest (behind: its fastest and that route's slowest).  Also records, per shape, the own durations of
the grouped unit's three kernels in the last call (h2v_workspace_timings of the grouped part's record).
--across-srs S measures H2V_MIXED_ACROSS_SRS (one call and ONE multi-pairing for keys on S SRS), 1024 accepting proofs:
  (a) across:   ONE h2v_verify_mixed_device call with H2V_MIXED_ACROSS_SRS | H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM over all keys;
  (b) per SRS:  today's route - one H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM device call per SRS and step, each on its own workspace, on
                one caller stream.
S = 4: 4 SRS x 4 keys x 64 proofs; S = 16: 16 SRS x 1 key x 64.  The routes alternate (a), (b), `--runs` (at least five) each; a
run repeats its step until at least half a second has passed.  Every run goes to --out (default profiles/mixed_across_srs.json); a
gain is claimed only when the slowest run of (a) beats the fastest run of (b).
usage: bench_mixed.py [--shapes two,sixteen] [--runs 5] [--steps 20] [--cache DIR] [--out profiles/mixed_keys.json]
       bench_mixed.py --fold [...] [--out profiles/mixed_fold.json]
       bench_mixed.py --fold --grouped [--shapes sixteen,sixtyfour,twofiftysix,two] [...] [--out profiles/mixed_grouped.json]
       bench_mixed.py --across-srs 4 [--runs 5] [--cache DIR] [--out profiles/mixed_across_srs.json]"""
import argparse
import json
import os
import pickle
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

COMMON_S = 0x6d697865645f6b6579735f6f6e655f535253
SHAPES = {
    "two": [("lookup_table", None, 2048), ("atms_with_lookups", None, 2048)],
    "sixteen": [(name, 0x4d580000 + 16 * k + q, 64) for k, name in enumerate(("simple_mul", "lookup_table", "trashcan_mix", "atms_with_lookups"))
                for q in range(4)],
    "sixtyfour": [(name, 0x4d590000 + 64 * k + q, 16) for k, name in enumerate(("simple_mul", "lookup_table", "trashcan_mix", "atms_with_lookups"))
                  for q in range(16)],
    "twofiftysix": [(name, 0x4d5a0000 + 256 * k + q, 4) for k, name in enumerate(("simple_mul", "lookup_table", "trashcan_mix", "atms_with_lookups"))
                    for q in range(64)],
}


def forged(shape, cache):
    """[(vk, plan, batch)] of the shape, every key on the common SRS"""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    path = os.path.join(cache, "bench_mixed_%s.pkl" % shape) if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    out = []
    for k, (name, seed, cnt) in enumerate(SHAPES[shape]):
        vk, td = V.on_srs(*(V.BUILDERS[name]() if seed is None else V.BUILDERS[name](seed)), COMMON_S)
        pl = PL.compile_plan(vk)
        out.append((vk, pl, synth.forge_batch(vk, td, cnt, seed=100 + k, plan=pl, workers=16)))
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(out, f)
    return out


def run_shape(shape, runs, steps, cache, fold=False):
    import torch
    from plutus_halo2_verifier_gen_amd import backend
    keys = forged(shape, cache)
    dev = torch.device("cuda", 0)
    plans = [backend.DevicePlan(pl.to_bytes(), 0) for _vk, pl, _b in keys]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    # per key: device-resident batch; mixed: the same proofs interleaved by a seeded shuffle
    per_key = []
    for _vk, _pl, b in keys:
        per_key.append((b.n, t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed),
                        torch.zeros(b.n, dtype=torch.uint8, device=dev), torch.zeros(b.n, dtype=torch.int32, device=dev)))
    order = [(k, j) for k, (_vk, _pl, b) in enumerate(keys) for j in range(b.n)]
    random.Random(5).shuffle(order)
    proofs, inst, ci, off = [], [], [], [0]
    for k, j in order:
        vk, _pl, b = keys[k]
        proofs.append(b.proof(j))
        off.append(off[-1] + len(proofs[-1]))
        inst.append(b.instances[32 * vk.n_public_inputs * j:32 * vk.n_public_inputs * (j + 1)])
        if b.committed is not None:
            ci.append(b.ci(j))
    n = len(order)
    plan_of = [k for k, _ in order]
    m_in = (t(b"".join(proofs)), torch.tensor(off, dtype=torch.int64, device=dev), t(b"".join(inst)), t(b"".join(ci)))
    m_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    m_st = torch.zeros(n, dtype=torch.int32, device=dev)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws_new = backend.Workspace.multi(plans, n)
    ws_old = backend.Workspace.multi(plans, n)
    ws_old.defer_joins(True)
    seed = bytes(range(32))
    results = []
    ws_fold = backend.Workspace.multi(plans, n) if fold else None
    for mode in (("rlc",) if fold else ("per-proof", "rlc")):
        def fold_step():
            backend.verify_mixed_device(plans, plan_of, n, *[ptr(x) for x in m_in], m_acc.data_ptr(), m_st.data_ptr(), ws=ws_fold, stream=cs,
                                        mode="rlc", seed=seed, fold_msm=True)

        def new_step():
            backend.verify_mixed_device(plans, plan_of, n, *[ptr(x) for x in m_in], m_acc.data_ptr(), m_st.data_ptr(), ws=ws_new, stream=cs,
                                        mode=mode, seed=seed if mode == "rlc" else None)

        def old_step():
            for dp, (cnt, p, o, i, c, acc, st) in zip(plans, per_key):
                if mode == "rlc":
                    dp.verify_batch_rlc_device(cnt, ptr(p), ptr(o), ptr(i), ptr(c), acc.data_ptr(), st.data_ptr(), ws=ws_old, stream=cs, seed=seed)
                else:
                    dp.verify_batch_device(cnt, ptr(p), ptr(o), ptr(i), ptr(c), acc.data_ptr(), st.data_ptr(), ws=ws_old, stream=cs)

        def run(step, ws, k_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k_steps):
                step()
            ws.join(cs)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / k_steps

        if fold:
            run(fold_step, ws_fold, 3)
            assert m_acc.cpu().tolist() == [1] * n, "the fold form rejects a forged proof"
            assert ws_fold.rlc_result(timings=False)[0], "the fold form's check failed on forged proofs: the runs would time the fall-back"
            m_acc.zero_()
        for step, ws in ((new_step, ws_new), (old_step, ws_old)):      # warm-up: first uses allocate
            run(step, ws, 3)
        assert m_acc.cpu().tolist() == [1] * n, "the mixed call rejects a forged proof"
        assert all(x[5].cpu().tolist() == [1] * x[0] for x in per_key), "a per-key call rejects a forged proof"
        new_ms, old_ms, fold_ms = [], [], []
        for _ in range(runs):
            if fold:
                fold_ms.append(run(fold_step, ws_fold, steps))
            new_ms.append(run(new_step, ws_new, steps))
            old_ms.append(run(old_step, ws_old, steps))
        med = lambda v: sorted(v)[len(v) // 2]
        r = {"shape": shape, "keys": len(keys), "proofs": n, "mode": mode, "steps_per_run": steps,
             "new_ms_per_step": [round(x, 4) for x in new_ms], "baseline_ms_per_step": [round(x, 4) for x in old_ms],
             "new_median_ms": round(med(new_ms), 4), "baseline_median_ms": round(med(old_ms), 4),
             "gain_by_the_rule": max(new_ms) < min(old_ms), "loss_by_the_rule": min(new_ms) > max(old_ms)}
        if fold:
            r.update({"fold_ms_per_step": [round(x, 4) for x in fold_ms], "fold_median_ms": round(med(fold_ms), 4),
                      "fold_terms": ws_fold.rlc_result(timings=True)[1].msm_terms,
                      "fold_gain_by_the_rule": max(fold_ms) < min(new_ms) and max(fold_ms) < min(old_ms),
                      "fold_loss_by_the_rule": min(fold_ms) > max(new_ms) or min(fold_ms) > max(old_ms)})
        print(json.dumps(r), flush=True)
        results.append(r)
    for w in (ws_new, ws_old) + ((ws_fold,) if fold else ()):
        w.close()
    return results


def run_grouped(shape, runs, steps, cache):
    """routes (a) grouped, (b) fold, (c) per key on one shape, batch-accept mode"""
    import torch
    from plutus_halo2_verifier_gen_amd import backend
    keys = forged(shape, cache)
    dev = torch.device("cuda", 0)
    plans = [backend.DevicePlan(pl.to_bytes(), 0) for _vk, pl, _b in keys]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    per_key = []
    for _vk, _pl, b in keys:
        per_key.append((b.n, t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed),
                        torch.zeros(b.n, dtype=torch.uint8, device=dev), torch.zeros(b.n, dtype=torch.int32, device=dev)))
    order = [(k, j) for k, (_vk, _pl, b) in enumerate(keys) for j in range(b.n)]
    random.Random(5).shuffle(order)
    proofs, inst, ci, off = [], [], [], [0]
    for k, j in order:
        vk, _pl, b = keys[k]
        proofs.append(b.proof(j))
        off.append(off[-1] + len(proofs[-1]))
        inst.append(b.instances[32 * vk.n_public_inputs * j:32 * vk.n_public_inputs * (j + 1)])
        if b.committed is not None:
            ci.append(b.ci(j))
    n = len(order)
    plan_of = [k for k, _ in order]
    m_in = (t(b"".join(proofs)), torch.tensor(off, dtype=torch.int64, device=dev), t(b"".join(inst)), t(b"".join(ci)))
    m_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    m_st = torch.zeros(n, dtype=torch.int32, device=dev)
    cs = torch.cuda.Stream(device=dev).cuda_stream
    seed = bytes(range(32))
    with_fold = len(keys) <= backend.MIXED_MAX_PLANS
    ws = {"grouped": backend.Workspace.multi(plans, n), "per_key": backend.Workspace.multi(plans, n)}
    if with_fold:
        ws["fold"] = backend.Workspace.multi(plans, n)
    ws["per_key"].defer_joins(True)

    def mixed_step(route):
        backend.verify_mixed_device(plans, plan_of, n, *[ptr(x) for x in m_in], m_acc.data_ptr(), m_st.data_ptr(), ws=ws[route], stream=cs,
                                    mode="rlc", seed=seed, fold_msm=True, grouped=route == "grouped")

    def per_key_step():
        for dp, (cnt, p, o, i, c, acc, st) in zip(plans, per_key):
            dp.verify_batch_rlc_device(cnt, ptr(p), ptr(o), ptr(i), ptr(c), acc.data_ptr(), st.data_ptr(), ws=ws["per_key"], stream=cs, seed=seed)

    steps_of = {"grouped": lambda: mixed_step("grouped"), "per_key": per_key_step}
    if with_fold:
        steps_of["fold"] = lambda: mixed_step("fold")

    def run(route, k_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k_steps):
            steps_of[route]()
        ws[route].join(cs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k_steps

    routes = [r for r in ("grouped", "fold", "per_key") if r in steps_of]
    for route in routes:                                       # warm-up: first uses allocate; every route must accept everything
        m_acc.zero_()
        run(route, 3)
        if route == "per_key":
            assert all(x[5].cpu().tolist() == [1] * x[0] for x in per_key), "a per-key call rejects a forged proof"
        else:
            assert m_acc.cpu().tolist() == [1] * n, "the %s route rejects a forged proof" % route
            assert ws[route].rlc_result(timings=False)[0], "the %s route's check failed on forged proofs: the runs would time the fall-back" % route
    ms = {route: [] for route in routes}
    for _ in range(runs):
        for route in routes:
            ms[route].append(run(route, steps))
    med = lambda v: sorted(v)[len(v) // 2]
    r = {"shape": shape, "keys": len(keys), "proofs": n, "mode": "rlc", "steps_per_run": steps}
    for route in routes:
        r[route + "_ms_per_step"] = [round(x, 4) for x in sorted(ms[route])]
        r[route + "_median_ms"] = round(med(ms[route]), 4)
    for other in routes[1:]:
        r["grouped_gain_over_" + other] = max(ms["grouped"]) < min(ms[other])
        r["grouped_loss_to_" + other] = min(ms["grouped"]) > max(ms[other])
    # the grouped unit's own kernels in the last grouped call: its record is the one before the tail's (every key here is groupable)
    run("grouped", 1)
    tm = ws["grouped"].timings(1)
    r["grouped_kernels_ms"] = {"transcript_combiner": round(tm.transcript_combiner_ms, 4), "g1_decompress": round(tm.g1_decompress_ms, 4),
                               "mixed_terms": round(tm.g1_msm_ms, 4)}
    r["msm_terms"] = ws["grouped"].rlc_result(timings=True)[1].msm_terms
    print(json.dumps(r), flush=True)
    for w in ws.values():
        w.close()
    return [r]


ACROSS_SHAPES = {4: (4, 64), 16: (1, 64)}          # SRS -> (keys per SRS, proofs per key): 1024 proofs either way
ACROSS_CIRCUITS = ("simple_mul", "lookup_table", "trashcan_mix", "atms_with_lookups")


def forged_across(n_srs, cache):
    """[(SRS index, vk, plan, batch)]: ACROSS_SHAPES[n_srs] keys on each of n_srs SRS"""
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    path = os.path.join(cache, "bench_mixed_across_%d.pkl" % n_srs) if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    per_srs, cnt = ACROSS_SHAPES[n_srs]
    out = []
    for s in range(n_srs):
        secret = (0x4d5b0000 + s) << 64 | (1000003 + 2 * s)
        for q in range(per_srs):
            name = ACROSS_CIRCUITS[(s + q) % 4]
            vk, td = V.on_srs(*V.BUILDERS[name](0x4d5c0000 + 16 * s + q), secret)
            pl = PL.compile_plan(vk)
            out.append((s, vk, pl, synth.forge_batch(vk, td, cnt, seed=300 + per_srs * s + q, plan=pl, workers=16)))
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(out, f)
    return out


def run_across(n_srs, runs, cache):
    """routes (a) across, (b) one fold call per SRS, batch-accept mode, all-accepting proofs"""
    import torch
    from plutus_halo2_verifier_gen_amd import backend
    keys = forged_across(n_srs, cache)
    dev = torch.device("cuda", 0)
    plans = [backend.DevicePlan(pl.to_bytes(), 0) for _s, _vk, pl, _b in keys]
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    order = [(k, j) for k, (_s, _vk, _pl, b) in enumerate(keys) for j in range(b.n)]
    random.Random(5).shuffle(order)

    def call_of(sub, listed):
        """the device-resident mixed batch of the positions `sub` of the order over the listed keys"""
        proofs, inst, ci, off = [], [], [], [0]
        for k, j in sub:
            _s, vk, _pl, b = keys[k]
            proofs.append(b.proof(j))
            off.append(off[-1] + len(proofs[-1]))
            inst.append(b.instances[32 * vk.n_public_inputs * j:32 * vk.n_public_inputs * (j + 1)])
            if b.committed is not None:
                ci.append(b.ci(j))
        n = len(sub)
        return {"plans": [plans[k] for k in listed], "plan_of": [listed.index(k) for k, _ in sub], "n": n,
                "in": (t(b"".join(proofs)), torch.tensor(off, dtype=torch.int64, device=dev), t(b"".join(inst)), t(b"".join(ci))),
                "acc": torch.zeros(n, dtype=torch.uint8, device=dev), "st": torch.zeros(n, dtype=torch.int32, device=dev),
                "ws": backend.Workspace.multi([plans[k] for k in listed], n)}

    whole = call_of(order, list(range(len(keys))))
    per_srs = [call_of([o for o in order if keys[o[0]][0] == s], [k for k in range(len(keys)) if keys[k][0] == s]) for s in range(n_srs)]
    cs = torch.cuda.Stream(device=dev).cuda_stream
    seed = bytes(range(32))

    def step(c, across):
        backend.verify_mixed_device(c["plans"], c["plan_of"], c["n"], *[ptr(x) for x in c["in"]], c["acc"].data_ptr(), c["st"].data_ptr(), ws=c["ws"],
                                    stream=cs, mode="rlc", seed=seed, fold_msm=True, across_srs=across)

    steps_of = {"across": lambda: step(whole, True), "per_srs": lambda: [step(c, False) for c in per_srs]}

    def run(route, min_seconds):
        torch.cuda.synchronize()
        t0, k = time.perf_counter(), 0
        while k < 1 or time.perf_counter() - t0 < min_seconds:
            steps_of[route]()
            k += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k, k

    for route in ("across", "per_srs"):                        # warm-up: first uses allocate; every route must accept everything
        run(route, 0.0)
        run(route, 0.0)
        for c in ([whole] if route == "across" else per_srs):
            assert c["acc"].cpu().tolist() == [1] * c["n"], "the %s route rejects a forged proof" % route
            assert c["ws"].rlc_result(timings=False)[0], "the %s route's check failed on forged proofs: the runs would time the fall-back" % route
    ms = {"across": [], "per_srs": []}
    steps = {"across": [], "per_srs": []}
    for _ in range(runs):
        for route in ("across", "per_srs"):
            m, k = run(route, 0.5)
            ms[route].append(m)
            steps[route].append(k)
    med = lambda v: sorted(v)[len(v) // 2]
    r = {"srs": n_srs, "keys": len(keys), "proofs": whole["n"], "mode": "rlc", "msm_terms": whole["ws"].rlc_result(timings=True)[1].msm_terms}
    for route in ("across", "per_srs"):
        r[route + "_ms_per_step"] = [round(x, 4) for x in ms[route]]
        r[route + "_steps_per_run"] = steps[route]
        r[route + "_median_ms"] = round(med(ms[route]), 4)
    r["across_gain_by_the_rule"] = max(ms["across"]) < min(ms["per_srs"])
    r["across_loss_by_the_rule"] = min(ms["across"]) > max(ms["per_srs"])
    print(json.dumps(r), flush=True)
    for c in [whole] + per_srs:
        c["ws"].close()
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="two,sixteen")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--forge-only", action="store_true", help="forge (and cache) the batches, then stop: no GPU needed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fold", action="store_true", help="batch-accept mode only, with route (c): the call with H2V_MIXED_FOLD_MSM")
    ap.add_argument("--grouped", action="store_true", help="with --fold: H2V_MIXED_GROUPED against the fold form and the per-key calls")
    ap.add_argument("--across-srs", type=int, default=0, choices=(0,) + tuple(sorted(ACROSS_SHAPES)),
                    help="H2V_MIXED_ACROSS_SRS over this many SRS against one fold call per SRS (1024 proofs)")
    args = ap.parse_args()
    if args.across_srs and (args.fold or args.grouped):
        ap.error("--across-srs is a measurement of its own")
    if args.grouped and not args.fold:
        ap.error("--grouped goes with --fold")
    if args.runs < 5 and not args.forge_only:
        ap.error("at least five runs of each route")
    if args.forge_only:
        if args.across_srs:
            forged_across(args.across_srs, args.cache)
            return
        for shape in args.shapes.split(","):
            forged(shape, args.cache)
        return
    import torch
    results = []
    if args.across_srs:
        args.out = args.out or os.path.join(ROOT, "profiles", "mixed_across_srs.json")
        if os.path.exists(args.out):          # (one file for both shapes: the other shape's runs are kept)
            with open(args.out) as f:
                results += [c for c in json.load(f)["cases"] if c.get("srs") != args.across_srs]
        results += run_across(args.across_srs, args.runs, args.cache)
    for shape in ([] if args.across_srs else args.shapes.split(",")):
        results += run_grouped(shape, args.runs, args.steps, args.cache) if args.grouped else run_shape(shape, args.runs, args.steps, args.cache, args.fold)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_mixed.py", "device": torch.cuda.get_device_name(0), "runs": args.runs, "cases": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
