#!/usr/bin/env python3
"""Aggregate calls (h2v_aggregate_batch_device / h2v_aggregate_mixed_device) against the batch-accept forms that check inside the
call, in ONE process, alternating, per WINDOW of calls:
  w16x4096   16 calls of simple_mul x 4096 on a laned workspace with deferred joins:
             (rlc) h2v_verify_batch_rlc_device per call, joined at the end of the window - one pairing per call;
             (agg) h2v_aggregate_batch_device per call + ONE h2v_check_pairs_rlc_device over the window's 16 pairs, everything on
                   one caller stream: an aggregate call joins its lanes inside the call, so the calls of a window run one after
                   the other;
             (agg16) the same with the aggregate calls round robin on sixteen caller streams (the check waits for all of them): the
                   calls of a window overlap in the lanes as the deferred RLC calls do.
  w64x256    64 calls of simple_mul x 256, the same two routes.  The RLC calls of this size are coalesced (one launch per sixteen
             of them), the aggregate calls are not: this shape may lose, and is reported either way.
  mixed16x64 16 keys x 64 proofs in one call (tools/bench_mixed.py's `sixteen`):
             (fold) h2v_verify_mixed_device with H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM - it synchronises the caller's stream once;
             (agg)  h2v_aggregate_mixed_device + ONE h2v_check_pairs_device on its pair - nothing synchronises.
All proofs accept (the forms are measured where they are meant to be used); before timing both routes must accept everything.
Every shape is warmed up, the warm-up sizes the runs (at least --min-run-ms of work each), runs alternate between the routes,
--runs each (at least five), between two device synchronisations.  A route wins a shape only when its slowest run beats the other's
fastest.  --cache DIR keeps the forged batches (forging is CPU work).  One JSON line per shape and, with --out, the whole set.
usage: bench_aggregate.py [--shapes w16x4096,w64x256,mixed16x64] [--runs 5] [--min-run-ms 500] [--cache DIR] [--out profiles/aggregate.json]"""
import argparse
import json
import math
import os
import pickle
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WINDOWS = {"w16x4096": (16, 4096), "w64x256": (64, 256)}
SEED = bytes(range(32))


def forged_simple_mul(n, cache):
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    path = os.path.join(cache, "bench_aggregate_simple_mul_%d.pkl" % n) if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    out = (vk, pl, synth.forge_batch(vk, td, n, seed=7, plan=pl, workers=16))
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(out, f)
    return out


def timed_runs(routes, runs, min_run_ms, sync):
    """routes: [(name, window function)]; returns {name: [ms per window]} from alternating runs of equal length"""
    def run(fn, k):
        sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / k
    warm = {name: min(run(fn, 2), run(fn, 2)) for name, fn in routes}
    k = max(2, int(math.ceil(min_run_ms / min(warm.values()))))
    out = {name: [] for name, _ in routes}
    for _ in range(runs):
        for name, fn in routes:
            out[name].append(run(fn, k))
    return out, k


def report(shape, ms, k, a, b, extra):
    med = lambda v: sorted(v)[len(v) // 2]
    r = {"shape": shape, "windows_per_run": k}
    for name in (a, b):
        r[name + "_ms_per_window"] = [round(x, 4) for x in ms[name]]
        r[name + "_range_ms"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        r[name + "_median_ms"] = round(med(ms[name]), 4)
    r["aggregate_wins_by_the_rule"] = max(ms[b]) < min(ms[a])
    r["aggregate_loses_by_the_rule"] = min(ms[b]) > max(ms[a])
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def run_window(shape, runs, min_run_ms, cache):
    import torch
    from plutus_halo2_verifier_gen_amd import backend
    calls, n = WINDOWS[shape]
    vk, pl, b = forged_simple_mul(n, cache)
    dev = torch.device("cuda", 0)
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    d_in = (t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed))
    args = (n, *[ptr(x) for x in d_in])
    acc = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(calls)]
    inc = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(calls)]
    pairs = torch.zeros(96 * calls, dtype=torch.uint8, device=dev)
    p_acc = torch.zeros(calls, dtype=torch.uint8, device=dev)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws_rlc = backend.Workspace(dp, 16 * 4096, lanes=0, chunk=0)
    ws_agg = backend.Workspace(dp, 16 * 4096, lanes=0, chunk=0)
    ws_aggs = backend.Workspace(dp, 16 * 4096, lanes=0, chunk=0)
    p_accs = torch.zeros(calls, dtype=torch.uint8, device=dev)
    for w in (ws_rlc, ws_agg, ws_aggs):
        w.defer_joins(True)
    ws_chk = backend.Workspace(dp, max(64, calls))

    def rlc_window():
        for k in range(calls):
            dp.verify_batch_rlc_device(*args, acc[k].data_ptr(), None, ws=ws_rlc, stream=cs, seed=SEED)
        ws_rlc.join(cs)

    def agg_window():
        for k in range(calls):
            dp.aggregate_batch_device(*args, pairs.data_ptr() + 96 * k, inc[k].data_ptr(), None, ws=ws_agg, stream=cs, seed=SEED)
        dp.check_pairs_rlc_device(calls, pairs.data_ptr(), p_acc.data_ptr(), None, ws=ws_chk, stream=cs, seed=SEED)

    # sixteen caller streams; two pair buffers in turn, so that a window's calls do not wait for the check of the window before
    streams = [torch.cuda.Stream(device=dev) for _ in range(16)]
    pairs2 = [torch.zeros(96 * calls, dtype=torch.uint8, device=dev) for _ in range(2)]
    checked = [None, None]
    turn = [0]

    def agg16_window():
        q = turn[0] % 2
        turn[0] += 1
        for k in range(calls):
            s = streams[k % 16]
            if k < 16 and checked[q] is not None:
                s.wait_event(checked[q])
            dp.aggregate_batch_device(*args, pairs2[q].data_ptr() + 96 * k, inc[k].data_ptr(), None, ws=ws_aggs, stream=s.cuda_stream, seed=SEED)
        for s in streams:
            ev = torch.cuda.Event()
            ev.record(s)
            caller.wait_event(ev)
        dp.check_pairs_rlc_device(calls, pairs2[q].data_ptr(), p_accs.data_ptr(), None, ws=ws_chk, stream=cs, seed=SEED)
        checked[q] = torch.cuda.Event()
        checked[q].record(caller)

    rlc_window(); agg_window(); agg16_window()
    torch.cuda.synchronize()
    assert all(a.cpu().tolist() == [1] * n for a in acc), "an RLC call rejects a forged proof"
    assert all(a.cpu().tolist() == [1] * n for a in inc) and p_acc.cpu().tolist() == [1] * calls, "the aggregate route rejects a forged proof"
    assert p_accs.cpu().tolist() == [1] * calls and pairs2[0].cpu().tolist() != [0] * (96 * calls), "the aggregate route on sixteen streams rejects a forged proof"
    assert ws_chk.rlc_result(timings=False)[0], "the window's pair check failed on forged proofs"
    ms, k = timed_runs([("rlc", rlc_window), ("aggregate", agg_window), ("aggregate16", agg16_window)], runs, min_run_ms, torch.cuda.synchronize)
    r = report(shape, ms, k, "rlc", "aggregate", {"calls_per_window": calls, "proofs_per_call": n, "lanes_chunk": list(ws_agg.lanes())})
    r["aggregate16_ms_per_window"] = [round(x, 4) for x in ms["aggregate16"]]
    r["aggregate16_range_ms"] = [round(min(ms["aggregate16"]), 4), round(max(ms["aggregate16"]), 4)]
    r["aggregate16_wins_by_the_rule"] = max(ms["aggregate16"]) < min(ms["rlc"])
    r["aggregate16_loses_by_the_rule"] = min(ms["aggregate16"]) > max(ms["rlc"])
    print(json.dumps({"shape": shape, "aggregate16_range_ms": r["aggregate16_range_ms"], "wins": r["aggregate16_wins_by_the_rule"], "loses": r["aggregate16_loses_by_the_rule"]}), flush=True)
    for w in (ws_rlc, ws_agg, ws_aggs, ws_chk):
        w.close()
    return r


def run_mixed(runs, min_run_ms, cache):
    import random
    import torch
    from bench_mixed import forged
    from plutus_halo2_verifier_gen_amd import backend
    keys = forged("sixteen", cache)
    dev = torch.device("cuda", 0)
    plans = [backend.DevicePlan(pl.to_bytes(), 0) for _vk, pl, _b in keys]
    t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
    ptr = lambda x: x.data_ptr() if x is not None else None
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
    tensors = (t(b"".join(proofs)), torch.tensor(off, dtype=torch.int64, device=dev), t(b"".join(inst)), t(b"".join(ci)))   # (alive to the end)
    m_in = [ptr(x) for x in tensors]
    m_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    m_inc = torch.zeros(n, dtype=torch.uint8, device=dev)
    pair = torch.zeros(96, dtype=torch.uint8, device=dev)
    p_acc = torch.zeros(1, dtype=torch.uint8, device=dev)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws_fold, ws_agg = backend.Workspace.multi(plans, n), backend.Workspace.multi(plans, n)
    ws_chk = backend.Workspace(plans[0], 64)

    def fold_call():
        backend.verify_mixed_device(plans, plan_of, n, *m_in, m_acc.data_ptr(), None, ws=ws_fold, stream=cs, mode="rlc", seed=SEED, fold_msm=True)

    def agg_call():
        backend.aggregate_mixed_device(plans, plan_of, n, *m_in, pair.data_ptr(), m_inc.data_ptr(), None, ws=ws_agg, stream=cs, seed=SEED)
        plans[0].check_pairs_device(1, pair.data_ptr(), p_acc.data_ptr(), None, ws=ws_chk, stream=cs)

    fold_call(); agg_call()
    torch.cuda.synchronize()
    assert m_acc.cpu().tolist() == [1] * n and ws_fold.rlc_result(timings=False)[0], "the fold form rejects a forged proof"
    assert m_inc.cpu().tolist() == [1] * n and p_acc.cpu().tolist() == [1], "the aggregate route rejects a forged proof"
    ms, k = timed_runs([("fold", fold_call), ("aggregate", agg_call)], runs, min_run_ms, torch.cuda.synchronize)
    r = report("mixed16x64", ms, k, "fold", "aggregate", {"keys": len(keys), "proofs": n})
    for w in (ws_fold, ws_agg, ws_chk):
        w.close()
    del tensors
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="w16x4096,w64x256,mixed16x64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-run-ms", type=float, default=500.0)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--forge-only", action="store_true", help="forge (and cache) the batches, then stop: no GPU needed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5 and not args.forge_only:
        ap.error("at least five runs of each route")
    shapes = args.shapes.split(",")
    if args.forge_only:
        for shape in shapes:
            if shape in WINDOWS:
                forged_simple_mul(WINDOWS[shape][1], args.cache)
            else:
                from bench_mixed import forged
                forged("sixteen", args.cache)
        return
    import torch
    results = []
    for shape in shapes:
        results.append(run_window(shape, args.runs, args.min_run_ms, args.cache) if shape in WINDOWS else run_mixed(args.runs, args.min_run_ms, args.cache))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_aggregate.py", "device": torch.cuda.get_device_name(0), "runs": args.runs, "min_run_ms": args.min_run_ms,
                       "cases": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
