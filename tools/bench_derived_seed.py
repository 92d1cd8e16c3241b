#!/usr/bin/env python3
"""What a derived batch seed (H2V_RLC_SEED_TRANSCRIPT) costs, in ONE process, alternating, on all-accepting batches:
  simple_mul x 4096 and the sha256 shape x 1024, each as h2v_aggregate_batch_device and as h2v_verify_batch_rlc_device,
    (derived) with the flag: the digest launches run in front of the call;
    (given)   with H2V_RLC_SEED_GIVEN: the same build through the seed_dev == NULL path - what the library did before the flag.
Calls go one after the other on one caller stream and an ordinary workspace.  Every case is warmed up, the warm-up sizes the runs (at
least --min-run-ms of work each), runs alternate between the arms, --runs each (at least five), between two device synchronisations.
Reported per case: every run of both arms (ms per call), the overhead slowest-derived over fastest-given, and - from HIP events of
one more call per run - the summed duration of the digest launches beside that call's transcript_combiner_ms.  THE CONDITION: the
digest launches take less time than the transcript kernel of the same call, which hashes the same bytes and runs the combiner too
("digest_below_transcript" must be true in every run).  --cache DIR keeps the forged batches (forging is CPU work).
--mixed measures the mixed-key calls' flag instead (H2V_RLC_SEED_KEYED, form 3): 16 keys x 64 and 64 keys x 16 proofs (the shapes
"sixteen" and "sixtyfour" of tools/bench_mixed.py, interleaved by its seeded shuffle), each as h2v_aggregate_mixed_device and as
h2v_verify_mixed_device with H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM, each without and with H2V_RLC_GROUPED / H2V_MIXED_GROUPED, on a
multi-plan workspace; (keyed) against (given), the same method, the digest time from h2v_workspace_seed_ms.  There is no condition
on the digest time there: the mixed calls' phase 1 is spread over several records.
usage: bench_derived_seed.py [--runs 5] [--min-run-ms 500] [--cache DIR] [--forge-only] [--out profiles/derived_seed.json]
       bench_derived_seed.py --mixed [...] [--out profiles/derived_seed_mixed.json]"""
import argparse
import json
import math
import os
import pickle
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [("simple_mul", 4096), ("sha256", 1024)]
SEED = bytes(range(32))


def forged(name, n, cache):
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    path = os.path.join(cache, "bench_derived_seed_%s_%d.pkl" % (name, n)) if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    vk, td = V.BUILDERS[name]()
    pl = PL.compile_plan(vk)
    out = (vk, pl, synth.forge_batch(vk, td, n, seed=7, plan=pl, workers=16, ci_identity=(name == "sha256")))
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(out, f)
    return out


def run_case(name, n, form, runs, min_run_ms, cache):
    import torch
    from plutus_halo2_verifier_gen_amd import backend, seed as S
    vk, pl, b = forged(name, n, cache)
    dev = torch.device("cuda", 0)
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    d_in = (t(b.proofs), torch.tensor(b.proof_off, dtype=torch.int64, device=dev), t(b.instances), t(b.committed))
    args = (n, *[ptr(x) for x in d_in])
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    pair = torch.zeros(96, dtype=torch.uint8, device=dev)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws = backend.Workspace(dp, n)
    ws.set_option(backend.OPT_RLC_ROUTE, -1)

    def call(**kw):
        if form == "aggregate":
            dp.aggregate_batch_device(*args, pair.data_ptr(), acc.data_ptr(), None, ws=ws, stream=cs, **kw)
        else:
            dp.verify_batch_rlc_device(*args, acc.data_ptr(), None, ws=ws, stream=cs, **kw)

    arms = [("derived", lambda: call(derive_seed=True)), ("given", lambda: call(seed=SEED))]

    def run(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    for _nm, fn in arms:
        fn()
        torch.cuda.synchronize()
        assert acc.cpu().tolist() == [1] * n, "a forged proof is rejected"
    want = S.batch_seed_flat(dp.key_tag, b.proofs, b.proof_off, b.instances, b.committed or b"", n_pi=vk.n_public_inputs, n_ci=dp.n_ci)
    arms[0][1]()
    torch.cuda.synchronize()
    assert ws.seed_used() == want, "the derived seed is not the model's"
    warm = {nm: min(run(fn, 2), run(fn, 2)) for nm, fn in arms}
    k = max(2, int(math.ceil(min_run_ms / min(warm.values()))))
    ms = {nm: [] for nm, _ in arms}
    digest, transcript = [], []
    for _ in range(runs):
        for nm, fn in arms:
            ms[nm].append(run(fn, k))
        arms[0][1]()                      # one more derived call: its digest launches beside its own transcript kernel
        torch.cuda.synchronize()
        digest.append(ws.seed_ms())
        transcript.append(ws.rlc_result()[1].transcript_combiner_ms)
    r = {"circuit": name, "proofs": n, "form": form, "calls_per_run": k, "proof_bytes": len(b.proofs),
         "derived_ms_per_call": [round(x, 4) for x in ms["derived"]], "given_ms_per_call": [round(x, 4) for x in ms["given"]],
         "overhead_slowest_over_fastest": round(max(ms["derived"]) / min(ms["given"]) - 1.0, 4),
         "overhead_fastest_over_slowest": round(min(ms["derived"]) / max(ms["given"]) - 1.0, 4),
         "digest_launches_ms": [round(x, 4) for x in digest], "transcript_combiner_ms": [round(x, 4) for x in transcript],
         "digest_below_transcript": all(d < tc for d, tc in zip(digest, transcript))}
    print(json.dumps(r), flush=True)
    ws.close()
    return r


MIXED_SHAPES = ["sixteen", "sixtyfour"]


def run_mixed_case(shape, form, grouped, runs, min_run_ms, cache):
    import random
    import torch
    from plutus_halo2_verifier_gen_amd import backend, seed as S
    from tools import bench_mixed
    keys = bench_mixed.forged(shape, cache)
    dev = torch.device("cuda", 0)
    plans = [backend.DevicePlan(pl.to_bytes(), 0) for _vk, pl, _b in keys]
    order = [(k, j) for k, (_vk, _pl, b) in enumerate(keys) for j in range(b.n)]
    random.Random(5).shuffle(order)
    proofs, inst, ci, off = [], [], [], [0]
    for k, j in order:
        vk, _pl, b = keys[k]
        proofs.append(b.proof(j))
        off.append(off[-1] + len(proofs[-1]))
        inst.append(b.instances[32 * vk.n_public_inputs * j:32 * vk.n_public_inputs * (j + 1)])
        ci.append(b.ci(j) if b.committed is not None else b"")
    n, plan_of = len(order), [k for k, _ in order]
    t = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else None
    ptr = lambda x: x.data_ptr() if x is not None else None
    d_in = (t(b"".join(proofs)), torch.tensor(off, dtype=torch.int64, device=dev), t(b"".join(inst)), t(b"".join(ci)))
    args = (plans, plan_of, n, *[ptr(x) for x in d_in])
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    pair = torch.zeros(96, dtype=torch.uint8, device=dev)
    cs = torch.cuda.Stream(device=dev).cuda_stream
    ws = backend.Workspace.multi(plans, n)

    def call(**kw):
        if form == "aggregate_mixed":
            backend.aggregate_mixed_device(*args, pair.data_ptr(), acc.data_ptr(), None, ws=ws, stream=cs, grouped=grouped, **kw)
        else:
            backend.verify_mixed_device(*args, acc.data_ptr(), None, ws=ws, stream=cs, mode="rlc", fold_msm=True, grouped=grouped, **kw)

    arms = [("keyed", lambda: call(keyed_seed=True)), ("given", lambda: call(seed=SEED))]

    def run(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    for _nm, fn in arms:
        fn()
        torch.cuda.synchronize()
        assert acc.cpu().tolist() == [1] * n, "a forged proof is rejected"
    want = S.mixed_seed([p.key_tag for p in plans], plan_of, inst, ci, proofs)
    arms[0][1]()
    torch.cuda.synchronize()
    assert ws.seed_used() == want, "the derived seed is not the model's"
    warm = {nm: min(run(fn, 2), run(fn, 2)) for nm, fn in arms}
    k = max(2, int(math.ceil(min_run_ms / min(warm.values()))))
    ms = {nm: [] for nm, _ in arms}
    digest = []
    for _ in range(runs):
        for nm, fn in arms:
            ms[nm].append(run(fn, k))
        arms[0][1]()                      # one more keyed call: the device time of its digest launches
        torch.cuda.synchronize()
        digest.append(ws.seed_ms())
    r = {"shape": shape, "keys": len(keys), "proofs": n, "form": form, "grouped": grouped, "calls_per_run": k, "proof_bytes": off[-1],
         "keyed_ms_per_call": [round(x, 4) for x in ms["keyed"]], "given_ms_per_call": [round(x, 4) for x in ms["given"]],
         "overhead_slowest_over_fastest": round(max(ms["keyed"]) / min(ms["given"]) - 1.0, 4),
         "overhead_fastest_over_slowest": round(min(ms["keyed"]) / max(ms["given"]) - 1.0, 4),
         "digest_launches_ms": [round(x, 4) for x in digest]}
    print(json.dumps(r), flush=True)
    ws.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-run-ms", type=float, default=500.0)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--forge-only", action="store_true", help="forge (and cache) the batches, then stop: no GPU needed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mixed", action="store_true", help="the mixed-key calls' flag (H2V_RLC_SEED_KEYED) instead")
    a = ap.parse_args()
    if a.forge_only:
        if a.mixed:
            from tools import bench_mixed
            for shape in MIXED_SHAPES:
                bench_mixed.forged(shape, a.cache)
            return
        for name, n in SHAPES:
            forged(name, n, a.cache)
        return
    if a.runs < 5:
        ap.error("at least five runs of each arm")
    import torch
    if a.mixed:
        cases = [run_mixed_case(shape, form, grouped, a.runs, a.min_run_ms, a.cache) for shape in MIXED_SHAPES
                 for form in ("aggregate_mixed", "verify_mixed_fold") for grouped in (False, True)]
        if a.out:
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/bench_derived_seed.py --mixed", "device": torch.cuda.get_device_name(0), "runs": a.runs,
                           "min_run_ms": a.min_run_ms, "cases": cases}, f, indent=1)
                f.write("\n")
        return
    cases = [run_case(name, n, form, a.runs, a.min_run_ms, a.cache) for name, n in SHAPES for form in ("aggregate", "verify_rlc")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_derived_seed.py", "device": torch.cuda.get_device_name(0), "runs": a.runs, "min_run_ms": a.min_run_ms,
                       "cases": cases}, f, indent=1)
            f.write("\n")
    if not all(c["digest_below_transcript"] for c in cases):
        sys.exit("the digest launches took longer than the transcript kernel of their call: the leaf kernel's mapping is wrong")


if __name__ == "__main__":
    main()
