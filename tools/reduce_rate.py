#!/usr/bin/env python3
"""Rates of the device-side reductions beside the single sweep of the same plan:
   python tools/reduce_rate.py [--out profiles/reduce_rate.jsonl] [--reps 24] [--small]

One process.  Per configuration, after a warm-up, `reps` rounds that ALTERNATE the things compared -- a single sweep
(lora_plan_step: the yardstick), lora_plan_diff, lora_plan_stats, and the sweep once more (sweep against sweep: the run-to-run
spread the comparison has to allow for) -- each between two device events of its own.  lora_plan_diff / lora_plan_stats block,
so their event pair also holds the copy-back of the record and the host's round trip: an upper bound of the launch pair.
Medians are reported, with bytes read over time and that as a share of 8 TB/s.

Then, at the 2D size only: lora_plan_run_until with check_every = 60 against a plain lora_plan_run of the same number of
sweeps (host clock around run + synchronise), beside the derived expectation: one sweep + one diff + one synchronise per check.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lorastencil_amd as L  # noqa: E402

PEAK = 8.0e12  # bytes / s


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rates(shape, dims, dtype, reps):
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float64
    item = 2 if dtype == "bf16" else 8
    a = (torch.rand(L.padded_shape(shape, dims), device="cuda") * 2 - 1).to(tdt)
    b = (torch.rand(L.padded_shape(shape, dims), device="cuda") * 2 - 1).to(tdt)
    plan = L.Plan(shape, dims, dtype=dtype)
    what = {"sweep": lambda: plan.step(a, b), "diff": lambda: plan.diff(a, b), "stats": lambda: plan.stats(a),
            "sweep_again": lambda: plan.step(a, b)}
    for fn in what.values():  # warm-up: code objects, the plan's record buffer
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    cells = int(np.prod(dims))
    read = {"sweep": cells * item, "diff": 2 * cells * item, "stats": cells * item, "sweep_again": cells * item}
    row = {"shape": shape, "dims": list(dims), "dtype": dtype, "reps": reps, "sweep_kernel": plan.kernel_name}
    for k in what:
        med = statistics.median(us[k])
        moved = read[k] * (2 if k.startswith("sweep") else 1)  # a sweep also writes what it reads
        row[k] = {"median_us": round(med, 1), "min_us": round(min(us[k]), 1), "max_us": round(max(us[k]), 1),
                  "bytes_read": read[k], "bytes_moved": moved, "moved_TBps": round(moved / med / 1e6, 3),
                  "share_of_8TBps": round(moved / (med * 1e-6) / PEAK, 3)}
    row["diff_over_sweep"] = round(row["diff"]["median_us"] / row["sweep"]["median_us"], 3)
    row["sweep_again_over_sweep"] = round(row["sweep_again"]["median_us"] / row["sweep"]["median_us"], 3)
    row["accepted"] = row["diff_over_sweep"] <= 1.10
    return row, plan, a, b


def until_cost(plan_args, reps, base_row):
    shape, dims, dtype = plan_args
    w = np.zeros(49)
    w[[24, 23, 25, 17, 31]] = 0.2
    plan = L.Plan(shape, dims, dtype=dtype).set_weights(w)
    a = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    b0, b1 = a.clone(), torch.zeros_like(a)
    times, every = 120, 60
    plan.prepare_run(every)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    plain, until = [], []
    result = None
    for i in range(max(3, reps // 4) + 1):
        b0.copy_(a)
        b1.zero_()
        ms, _ = wall(lambda: [plan.run(b0, b1, every) for _ in range(times // every)])
        b0.copy_(a)
        b1.zero_()
        ms_u, result = wall(lambda: plan.run_until(b0, b1, 0.0, check_every=every, max_times=times))
        if i:  # (the first round warms up)
            plain.append(ms)
            until.append(ms_u)
    checks = result.checks
    derived = statistics.median(plain) + checks * (base_row["sweep"]["median_us"] + base_row["diff"]["median_us"]) / 1e3
    return {"shape": shape, "dims": list(dims), "what": "run_until against plain runs", "times_done": result.times_done,
            "check_every": every, "checks": checks, "plain_run_ms": round(statistics.median(plain), 3),
            "run_until_ms": round(statistics.median(until), 3),
            "derived_ms (plain + checks x (sweep + diff incl. its synchronise))": round(derived, 3),
            "overhead": round(statistics.median(until) / statistics.median(plain) - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_rate.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    args = ap.parse_args()
    assert args.reps >= 20 or args.small
    n2, n3 = (2048, 128) if args.small else (16384, 768)
    configs = [("star2d1r", (n2, n2), "f64"), ("box3d1r", (n3, n3, n3), "f64"), ("box3d1r", (n3, n3, n3), "bf16")]
    lines = []
    for i, cfg in enumerate(configs):
        row, plan, a, b = rates(*cfg, args.reps)
        lines.append(row)
        print(json.dumps(row), flush=True)
        del plan, a, b
        torch.cuda.empty_cache()
        if i == 0:
            extra = until_cost(cfg, args.reps, row)
            lines.append(extra)
            print(json.dumps(extra), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
