#!/usr/bin/env python3
"""Cost of the keyed blake2b-512 transcript flavour against the Cardano flavour of the same circuit, in one run: verify
throughput measured the way tools/bench_prepare.py measures it (forged proofs resident on the device, a seeded tenth of them
corrupted, one laned workspace with deferred joins and one caller stream per flavour, warm-up calls on every lane, then
device-synchronised windows of at least --seconds, the two flavours alternating window by window), and the combiner kernel's
own duration (h2v_timings.transcript_combiner_ms of single calls on an ordinary workspace, median of --kernel-calls).  Before
timing, every flavour's verdicts must equal its construction, and each flavour's proofs must all reject under the other's
plan.  Writes one JSON line per case and, with --out, the whole set as one JSON file.
usage: bench_transcript.py [--seconds 1.0] [--warmup 5] [--repeats 3] [--kernel-calls 9] [--cases simple_mul:4096,sha256:1024]
                           [--out profiles/transcript_hash.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DEFAULT_CASES = "simple_mul:4096,sha256:1024"
KINDS = ["bad_point_flag", "point_not_in_subgroup", "noncanonical_scalar", "wrong_pi", "wrong_public_input"]
FLAVOURS = ("cardano-blake2b-256", "blake2b-512")


def run_case(name, B, seconds, warmup, repeats, kernel_calls):
    import torch
    from plutus_halo2_verifier_gen_amd import backend, plan as PL, synth, vk as V
    dev = torch.device("cuda", 0)
    caller = torch.cuda.Stream(device=dev)
    cs = caller.cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None else None
    K = 16
    side = {}
    for fl in FLAVOURS:
        vk, td = V.BUILDERS[name]()
        if fl != FLAVOURS[0]:
            vk = V.with_transcript_hash(vk, fl)
        pl = PL.compile_plan(vk)
        dp = backend.DevicePlan(pl.to_bytes(), 0)
        assert backend.TRANSCRIPT_NAMES[dp.transcript_kind] == fl
        batch = synth.forge_batch(vk, td, B, seed=1, plan=pl, workers=16, ci_identity=(name == "sha256"))
        batch = synth.with_rejects(pl, batch, vk.n_public_inputs, fraction=0.1, seed=2, kinds=KINDS)
        t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else None
        bufs = (t(batch.proofs), torch.tensor(batch.proof_off, dtype=torch.int64).to(dev), t(batch.instances), t(batch.committed))
        ws = backend.Workspace(dp, B, lanes=0, chunk=0)       # the laned workspace bench.py uses
        ws.defer_joins(True)
        side[fl] = {"pl": pl, "dp": dp, "batch": batch, "bufs": bufs, "args": (B,) + tuple(ptr(x) for x in bufs), "ws": ws,
                    "acc": [torch.zeros(B, dtype=torch.uint8, device=dev) for _ in range(K)],
                    "st": [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(K)]}
    n_lanes = side[FLAVOURS[0]]["ws"].lanes()[0]

    def step(fl, k, args=None):
        s = side[fl]
        k %= K
        s["dp"].verify_batch_device(*(args or s["args"]), s["acc"][k].data_ptr(), s["st"][k].data_ptr(), ws=s["ws"], stream=cs)

    def sync(fl):
        side[fl]["ws"].join(cs)
        torch.cuda.synchronize()

    # outputs against the construction before anything is timed; and the other flavour's proofs: every one a pairing reject
    for fl, other in (FLAVOURS, FLAVOURS[::-1]):
        step(fl, 0)
        sync(fl)
        assert side[fl]["acc"][0].cpu().tolist() == side[fl]["batch"].expected, (name, fl)
        valid = [i for i, e in enumerate(side[other]["batch"].expected) if e]
        step(fl, 1, side[other]["args"])
        sync(fl)
        got, st = side[fl]["acc"][1].cpu().tolist(), side[fl]["st"][1].cpu().tolist()
        assert not any(got) and all(st[i] == backend.ST_PAIRING for i in valid), (name, fl, "wrong hash")

    def window(fl, k_steps):
        t0 = time.perf_counter()
        for k in range(k_steps):
            step(fl, k)
        sync(fl)
        return time.perf_counter() - t0

    rates = {fl: [] for fl in FLAVOURS}
    for fl in FLAVOURS:                                   # warm-up on every lane (first uses allocate)
        for k in range(max(warmup, n_lanes)):
            step(fl, k)
        sync(fl)
    for _ in range(repeats):
        for fl in FLAVOURS:
            per_step = window(fl, 2 * n_lanes) / (2 * n_lanes)       # (untimed calibration)
            steps = max(2 * n_lanes, int(1.25 * seconds / per_step) + 1)
            rates[fl].append(steps * B / window(fl, steps))
    # the combiner kernel's own duration: single calls on an ordinary workspace, HIP events around the launch
    kernel_ms = {}
    for fl in FLAVOURS:
        s = side[fl]
        w1 = backend.Workspace(s["dp"], B)
        ms = []
        for k in range(kernel_calls + 2):
            s["dp"].verify_batch_device(*s["args"], s["acc"][0].data_ptr(), s["st"][0].data_ptr(), ws=w1, stream=cs)
            torch.cuda.synchronize()
            tm = w1.timings()
            if k >= 2:
                ms.append(tm.transcript_combiner_ms)
        w1.close()
        kernel_ms[fl] = ms
    a, b = FLAVOURS
    best = {fl: max(v) for fl, v in rates.items()}
    out = {"circuit": name, "batch": B, "msm_terms": side[a]["pl"].n_terms, "squeezes": side[a]["pl"].n_squeezes,
           "stream_bytes": side[a]["pl"].stream_len, "rejects": B - sum(side[a]["batch"].expected),
           "verify_proofs_per_s": {fl: round(best[fl], 1) for fl in FLAVOURS},
           "blake2b_512_over_cardano": round(best[b] / best[a], 4),
           "window_spread": {fl: round((max(v) - min(v)) / max(v), 4) for fl, v in rates.items()},
           "runs": {fl: [round(x, 1) for x in v] for fl, v in rates.items()},
           "combiner_kernel_ms": {fl: round(statistics.median(v), 4) for fl, v in kernel_ms.items()},
           "combiner_kernel_ms_runs": {fl: [round(x, 4) for x in v] for fl, v in kernel_ms.items()},
           "outputs_equal_construction": True}
    for fl in FLAVOURS:
        side[fl]["ws"].close()
        side[fl]["dp"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=9)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    results = []
    for c in args.cases.split(","):
        name, B = c.split(":")
        r = run_case(name, int(B), args.seconds, args.warmup, args.repeats, args.kernel_calls)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_transcript.py", "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
                       "repeats": args.repeats, "cases": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
