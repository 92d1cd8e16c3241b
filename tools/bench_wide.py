#!/usr/bin/env python3
"""Throughput of the wide keys (vk.WIDE_BUILDERS: final MSMs of more than 64 terms, summed in segments) measured the way
bench.py measures a workload: forged proofs resident on the device, one laned workspace with deferred joins and one caller
stream, h2v_workspace_tune on the batch (per-proof mode), warm-up steps on every lane, then a device-synchronised window of
at least --seconds in which the library keeps the calls in flight (one join at its end).  sha256 x 1024 (vk.BUILDERS) runs
in the same process as the yardstick.  One JSON line per case.
usage: bench_wide.py [--seconds 1.0] [--warmup 5] [--cases bls12381:1024,bls12381:1024:rlc,composite:1024,wide677:256,sha256:1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DEFAULT_CASES = "sha256:1024,bls12381:1024,bls12381:1024:rlc,composite:1024,wide677:256"


def run_case(name, B, mode, seconds, warmup):
    import torch
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V
    build = V.WIDE_BUILDERS.get(name) or V.BUILDERS[name]
    vk, td = build()
    pl = PL.compile_plan(vk)
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    batch = synth.forge_batch(vk, td, B, seed=1, plan=pl, workers=16)
    dev = torch.device("cuda", 0)
    d_proofs = torch.frombuffer(bytearray(batch.proofs), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(batch.proof_off, dtype=torch.int64).to(dev)
    d_inst = torch.frombuffer(bytearray(batch.instances), dtype=torch.uint8).to(dev) if batch.instances else None
    d_ci = torch.frombuffer(bytearray(batch.committed), dtype=torch.uint8).to(dev) if batch.committed else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws = backend.Workspace(dp, B, lanes=0, chunk=0)
    ws.defer_joins(True)
    n_lanes = ws.lanes()[0]
    tuned = None
    if mode == "per-proof":
        r = ws.tune(dp, B, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci), cs)
        tuned = {"pairing_engine": r.pairing_engine, "msm_terms_per_lane": r.msm_terms_per_lane}
    ring = [torch.zeros(B, dtype=torch.uint8, device=dev) for _ in range(16)]

    def step(k):
        args = (B, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci), ring[k % 16].data_ptr(), None)
        if mode == "rlc":
            dp.verify_batch_rlc_device(*args, ws=ws, stream=cs, seed=bytes(range(32)))
        else:
            dp.verify_batch_device(*args, ws=ws, stream=cs)

    for k in range(max(warmup, n_lanes)):
        step(k)
    ws.join(cs)
    torch.cuda.synchronize()

    def window(k_steps):   # k_steps calls kept in flight by the library, ONE join at the end (as bench.py times its steps)
        t0 = time.perf_counter()
        for k in range(k_steps):
            step(k)
        ws.join(cs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    per_step = window(2 * n_lanes) / (2 * n_lanes)        # (untimed calibration)
    steps = max(2 * n_lanes, int(1.25 * seconds / per_step) + 1)
    el = window(steps)
    while el < seconds:
        steps *= 2
        el = window(steps)
    ok = all(int(a.min().item()) == 1 for a in ring[:min(steps, 16)])
    tm = ws.timings(0) if mode == "per-proof" else None
    out = {"circuit": name, "batch": B, "mode": mode, "msm_terms": pl.n_terms, "steps": steps, "seconds": round(el, 4),
           "proofs_per_s": round(steps * B / el, 1), "all_accepted": ok, "tuned": tuned,
           "msm_lanes_per_term": tm.msm_lanes_per_term if tm else None}
    ws.close()
    dp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    args = ap.parse_args()
    for c in args.cases.split(","):
        f = c.split(":")
        name, B, mode = f[0], int(f[1]), (f[2] if len(f) > 2 else "per-proof")
        print(json.dumps(run_case(name, B, mode, args.seconds, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
