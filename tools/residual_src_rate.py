#!/usr/bin/env python3
"""Rate of lora_plan_residual_src beside lora_plan_residual and the two-pass probe it replaces:
   python tools/residual_src_rate.py [--out profiles/residual_src_rate.jsonl] [--reps 24] [--small] [--no-src]

One process.  Per configuration, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device
events of its own: lora_plan_residual, the same call once more (the spread every ratio has to allow for), lora_plan_residual_src
with f, and the two-pass probe as the Chebyshev driver runs it (a source sweep into a spare grid + lora_plan_diff).  Every call but
the sweep blocks, so the event pairs also hold the fold launch, the copy-back of the record and the host's round trip.  Medians.

Bars (each against code this tool's subject does not touch):
   residual_src / residual                 <= 2 x 1.10   two grids are read against one; the 10 % is section 3.5's margin
   residual_src / two-pass probe           <  1 - spread the fused probe has to win to be the driver's default
   residual here / residual at the parent  <= 1.10       --parent FILE: the jsonl of a `--no-src` run on a parent checkout

Last row: the solve of section 3.8 (star2d1r 2048^2, Dirichlet, f = 0.125, tol 1e-8, a check every 100 steps): steps, wall
time, and the cost of a probe as (run_chebyshev_until - run_leapfrog_src over the same steps) / checks.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("LORA_PACKAGE_ROOT", ROOT))
import lorastencil_amd as L  # noqa: E402


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rates(shape, dims, reps, with_src):
    a = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    plan = L.Plan(shape, dims)
    assert plan.get_option("fused_residual") == 1
    what = {"residual": lambda: plan.residual(a), "residual_again": lambda: plan.residual(a)}
    if with_src:
        f = torch.rand_like(a) - 0.5
        spare = torch.zeros_like(a)
        sourced = L.Plan(shape, dims).set_source(f)

        def two_pass():
            sourced.step(a, spare)
            return sourced.diff(spare, a)

        what["residual_src"] = lambda: plan.residual_src(a, f)
        what["two_pass"] = two_pass
    for fn in what.values():  # warm-up: code objects, the plans' record buffers
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if with_src:
        fused, old = plan.residual_src(a, f), two_pass()
        assert (fused.max_abs, fused.a_abs_max, fused.argmax, fused.count, fused.nonfinite) == (
            old.max_abs, old.a_abs_max, old.argmax, old.count, old.nonfinite), (fused, old)
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    row = {"shape": shape, "dims": list(dims), "dtype": "f64", "reps": reps}
    for k in what:
        row[k] = {"median_us": round(statistics.median(us[k]), 1), "min_us": round(min(us[k]), 1), "max_us": round(max(us[k]), 1)}
    plain = row["residual"]["median_us"]
    row["residual_again_over_residual"] = round(row["residual_again"]["median_us"] / plain, 3)
    row["spread"] = round(abs(row["residual_again_over_residual"] - 1.0), 3)
    if with_src:
        row["src_over_residual"] = round(row["residual_src"]["median_us"] / plain, 3)
        row["src_over_two_pass"] = round(row["residual_src"]["median_us"] / row["two_pass"]["median_us"], 3)
        row["src_over_residual_bar_met"] = row["src_over_residual"] <= 2 * 1.10
        row["src_over_two_pass_bar_met"] = row["src_over_two_pass"] < 1.0 - row["spread"]
    return row


def solve(n, reps):
    shape, dims, every = "star2d1r", (n, n), 100
    w = np.zeros(49)
    w[[23, 25, 17, 31]] = 0.25
    plan = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet")
    rho = math.cos(math.pi / (n + 1))
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    prev, cur = torch.zeros_like(f), torch.zeros_like(f)
    plan.prepare_leapfrog(every)

    def wall(fn):
        prev.zero_()
        cur.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms = {"until": [], "steps": []}
    r = None
    for i in range(max(3, reps // 6) + 1):
        t_until, r = wall(lambda: plan.run_chebyshev_until(prev, cur, f, rho, tol=1e-8, check_every=every, max_times=40000))
        a, c = L.chebyshev_coeffs(rho, 1, r.times_done)
        t_steps, _ = wall(lambda: [plan.run_leapfrog_src(prev, cur, f, a[k:k + every], c[k:k + every], every)
                                   for k in range(0, r.times_done, every)])
        if i:  # (the first round warms up)
            ms["until"].append(t_until)
            ms["steps"].append(t_steps)
    until, steps = statistics.median(ms["until"]), statistics.median(ms["steps"])
    return {"shape": shape, "dims": list(dims), "what": "Chebyshev solve: Dirichlet, f = 0.125, tol 1e-8, a check every 100 steps",
            "steps": r.times_done, "checks": r.checks, "converged": bool(r.converged), "residual": r.residual,
            "run_chebyshev_until_ms": round(until, 3), "same_steps_without_probes_ms": round(steps, 3),
            "us_per_probe": round((until - steps) * 1e3 / max(r.checks, 1), 1),
            "us_per_step": round(steps * 1e3 / max(r.times_done, 1), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_src_rate.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--no-src", action="store_true", help="the lora_plan_residual rows alone (a checkout without the entry)")
    ap.add_argument("--parent", default=None, help="jsonl of a --no-src run on the parent commit: adds residual_over_parent")
    args = ap.parse_args()
    assert args.reps >= 20 or args.small
    n2, nb, n3, n1 = (2048, 1024, 128, 2**20) if args.small else (16384, 8192, 768, 2**26)
    configs = [("star2d1r", (n2, n2)), ("box2d3r", (nb, nb)), ("box3d1r", (n3, n3, n3)), ("1d1r", (n1,))]
    parent = {}
    if args.parent:
        for line in open(args.parent):
            row = json.loads(line)
            parent[(row["shape"], tuple(row["dims"]))] = row
    lines = []
    for shape, dims in configs:
        row = rates(shape, dims, args.reps, not args.no_src)
        old = parent.get((shape, tuple(dims)))
        if old:
            row["parent_residual_median_us"] = old["residual"]["median_us"]
            row["parent_spread"] = old["spread"]
            row["residual_over_parent"] = round(row["residual"]["median_us"] / old["residual"]["median_us"], 3)
            row["residual_over_parent_bar_met"] = row["residual_over_parent"] <= 1.10
        lines.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if not args.no_src:
        row = solve(512 if args.small else 2048, args.reps)
        lines.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
