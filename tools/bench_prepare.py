#!/usr/bin/env python3
"""Throughput of prepare (h2v_prepare_batch_device: the verify pipeline without the pairing, exporting each proof's pair) and
of the pair check (h2v_check_pairs_device: the pairing alone) against verify, measured the way bench.py measures a workload:
forged proofs resident on the device (a seeded tenth of them corrupted, pre-pairing and pairing-only kinds), one laned
workspace with deferred joins and one caller stream, warm-up calls on every lane, then a device-synchronised window of at
least --seconds in which the library keeps the calls in flight (one join at its end).  verify, prepare and check run on the
same inputs and workspace, one after the other per repeat.  Before timing, check_pairs(prepare(x)) must equal verify(x).
Writes one JSON line per case and, with --out, the whole set as one JSON file.
usage: bench_prepare.py [--seconds 1.0] [--warmup 5] [--repeats 3] [--cases simple_mul:4096,sha256:1024,bls12381:1024,ivc:1024]
                        [--out profiles/prepare_pairs.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DEFAULT_CASES = "simple_mul:4096,sha256:1024,bls12381:1024,ivc:1024"
KINDS = ["bad_point_flag", "point_not_in_subgroup", "noncanonical_scalar", "wrong_pi", "wrong_public_input"]


def run_case(name, B, seconds, warmup, repeats):
    import torch
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V
    build = V.WIDE_BUILDERS.get(name) or V.BUILDERS[name]
    vk, td = build()
    pl = PL.compile_plan(vk)
    dp = backend.DevicePlan(pl.to_bytes(), 0)
    batch = synth.forge_batch(vk, td, B, seed=1, plan=pl, workers=16, ci_identity=(name == "sha256"))
    batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.1, seed=2, kinds=KINDS)
    dev = torch.device("cuda", 0)
    d_proofs = torch.frombuffer(bytearray(batch.proofs), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(batch.proof_off, dtype=torch.int64).to(dev)
    d_inst = torch.frombuffer(bytearray(batch.instances), dtype=torch.uint8).to(dev) if batch.instances else None
    d_ci = torch.frombuffer(bytearray(batch.committed), dtype=torch.uint8).to(dev) if batch.committed else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ws = backend.Workspace(dp, B, lanes=0, chunk=0)       # the laned workspace bench.py uses
    ws.defer_joins(True)
    n_lanes = ws.lanes()[0]
    K = 16
    acc = [torch.zeros(B, dtype=torch.uint8, device=dev) for _ in range(K)]
    st = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(K)]
    pairs = [torch.zeros(B * 96, dtype=torch.uint8, device=dev) for _ in range(K)]
    args = (B, ptr(d_proofs), ptr(d_off), ptr(d_inst), ptr(d_ci))

    def step(kind, k):
        k %= K
        if kind == "verify":
            dp.verify_batch_device(*args, acc[k].data_ptr(), st[k].data_ptr(), ws=ws, stream=cs)
        elif kind == "prepare":
            dp.prepare_batch_device(*args, pairs[k].data_ptr(), st[k].data_ptr(), ws=ws, stream=cs)
        else:
            dp.check_pairs_device(B, pairs[k].data_ptr(), acc[k].data_ptr(), st[k].data_ptr(), ws=ws, stream=cs)

    def sync():
        ws.join(cs)
        torch.cuda.synchronize()

    # correctness on these inputs: check_pairs(prepare(x)) == verify(x), and both == the construction
    step("verify", 0)
    step("prepare", 1)
    sync()
    v_acc, v_st = acc[0].cpu().tolist(), st[0].cpu().tolist()
    p_st = st[1].cpu().tolist()
    step("check", 1)
    sync()
    c_acc = acc[1].cpu().tolist()
    assert v_acc == c_acc == batch.expected, name
    assert p_st == [s & ~backend.ST_PAIRING for s in v_st], name
    # every check call reads the same pairs: fill the ring with prepare's output
    for k in range(2, K):
        pairs[k].copy_(pairs[1])
    torch.cuda.synchronize()

    def window(kind, k_steps):
        t0 = time.perf_counter()
        for k in range(k_steps):
            step(kind, k)
        sync()
        return time.perf_counter() - t0

    rates = {"verify": [], "prepare": [], "check": []}
    for kind in rates:                                   # warm-up of every kind on every lane (first uses allocate)
        for k in range(max(warmup, n_lanes)):
            step(kind, k)
        sync()
    for _ in range(repeats):
        for kind in rates:
            per_step = window(kind, 2 * n_lanes) / (2 * n_lanes)       # (untimed calibration)
            steps = max(2 * n_lanes, int(1.25 * seconds / per_step) + 1)
            el = window(kind, steps)
            rates[kind].append(steps * B / el)
    best = {k: max(v) for k, v in rates.items()}
    out = {"circuit": name, "batch": B, "msm_terms": pl.n_terms, "rejects": B - sum(batch.expected),
           "verify_proofs_per_s": round(best["verify"], 1), "prepare_proofs_per_s": round(best["prepare"], 1),
           "check_pairs_per_s": round(best["check"], 1),
           "prepare_over_verify": round(best["prepare"] / best["verify"], 3),
           # prepare + check in sequence: 1 / (1/prepare + 1/check) proofs per second, against verify
           "prepare_plus_check_over_verify": round((1.0 / (1.0 / best["prepare"] + 1.0 / best["check"])) / best["verify"], 3),
           "runs": {k: [round(x, 1) for x in v] for k, v in rates.items()}, "check_equals_verify": True}
    ws.close()
    dp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    results = []
    for c in args.cases.split(","):
        name, B = c.split(":")
        r = run_case(name, int(B), args.seconds, args.warmup, args.repeats)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_prepare.py", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
                       "repeats": args.repeats, "cases": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
