#!/usr/bin/env python3
"""Timings of the implicit time stepper:
   python tools/theta_timing.py [--out profiles/theta_timing.jsonl] [--reps 9] [--small]

One process, its own plans; normalised taps.  Per grid (star2d1r 4096^2 and 16384^2, box3d1r 256^3):
  1. lora_plan_theta_start (with f) beside what it stands for -- a source sweep (lora_plan_step of a plan that carries f), a
     pointwise pass the size of lora_plan_diff (two grids read; a subtraction, a scale and a copy are three such passes, each
     with a store on top) and lora_plan_dot -- and lora_plan_apply_dot_shift(9, 8) beside lora_plan_apply_dot, whose kernels
     this change leaves as the parent commit has them; lora_plan_theta_start once more (`spread`: what two identical calls differ
     by) and lora_plan_defect with and without f, the latter twice (`defect_spread`: the launch does not block).  `reps` rounds
     that ALTERNATE the entries, each between two device events of its own; medians.  The entries with a record block, so their event pairs also hold the fold launch, the copy-back of the
     record and the host's round trip.
Then on star2d1r 2048^2 (u0 = the lowest eigenmode of the zero-boundary problem plus 1 % noise, f = 0):
  2. the cost of a launch that exits early: the same 8 steps at tau = 64 with max_iters = K, the largest count a step needs, and
     with max_iters = 4 K -- the difference over 8 x 15 K launches (five per iteration: apply, fold, update, fold, direction);
  3. wall time to advance 4096 time units: lora_plan_run with 4096 explicit sweeps (zero boundary) against lora_plan_run_theta
     at theta = 1 with tau = 64 and tau = 512, max_iters = the largest count the run needs (found by a first run with room), and
     the amplitude of the smooth mode in each result.
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(xs, unit, digits=1):
    return {f"median_{unit}": round(statistics.median(xs), digits), f"min_{unit}": round(min(xs), digits), f"max_{unit}": round(max(xs), digits)}


def normalised(shape):
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    return w / w.sum()


def kernels(shape, dims, reps):
    w = normalised(shape)
    plan = L.Plan(shape, dims).set_weights(w)
    assert plan.get_option("cg") == 1
    u = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    f = torch.rand_like(u) - 0.5
    r, p, spare = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    with_f = L.Plan(shape, dims).set_weights(w).set_source(f)
    what = {"theta_start": lambda: plan.theta_start(u, f, 8.0, r, p), "source_sweep": lambda: with_f.step(u, spare),
            "diff_sized_pass": lambda: plan.diff(u, f), "dot": lambda: plan.dot(u, f),
            "apply_dot_shift": lambda: plan.apply_dot_shift(u, spare, 9.0, 8.0), "apply_dot": lambda: plan.apply_dot(u, spare),
            # the same call once more: the spread a comparison of two builds has to allow for; and the V-cycle's defect launch
            "theta_start_again": lambda: plan.theta_start(u, f, 8.0, r, p),
            "defect_src": lambda: plan.defect(u, f, spare), "defect": lambda: plan.defect(u, None, spare),
            "defect_again": lambda: plan.defect(u, None, spare)}  # (does not block: a spread of its own)
    for fn in what.values():  # warm-up: code objects, the plans' record buffers
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    row = {"shape": shape, "dims": list(dims), "reps": reps}
    for k in what:
        row[k] = spread(us[k], "us")
    med = lambda k: row[k]["median_us"]
    row["replaced_sweep_3_passes_dot_us"] = round(med("source_sweep") + 3 * med("diff_sized_pass") + med("dot"), 1)
    row["theta_start_over_replaced"] = round(med("theta_start") / row["replaced_sweep_3_passes_dot_us"], 3)
    row["theta_start_over_source_sweep"] = round(med("theta_start") / med("source_sweep"), 3)
    row["apply_dot_shift_over_apply_dot"] = round(med("apply_dot_shift") / med("apply_dot"), 3)
    row["spread"] = round(abs(med("theta_start_again") / med("theta_start") - 1.0), 3)
    row["defect_spread"] = round(abs(med("defect_again") / med("defect") - 1.0), 3)
    return row


def smooth_problem(n):
    shape, dims = "star2d1r", (n, n)
    i = torch.arange(1, n + 1, device="cuda", dtype=torch.float64)
    mode = torch.sin(math.pi * i / (n + 1))[:, None] * torch.sin(math.pi * i / (n + 1))[None, :]
    u0 = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(7)
    L.interior(shape, u0)[...] = mode + 0.01 * (torch.rand(dims, device="cuda", dtype=torch.float64, generator=gen) * 2 - 1)
    amplitude = lambda t: float((L.interior(shape, t) * mode).sum() / (mode * mode).sum())
    return shape, dims, u0, amplitude


def early_exit(n, reps):
    shape, dims, u0, _ = smooth_problem(n)
    plan = L.Plan(shape, dims).set_weights(normalised(shape))
    u = torch.zeros_like(u0)
    steps, tau = 8, 64.0
    plan.prepare_theta(steps)

    def run(max_iters):
        u.copy_(u0)
        return wall_ms(lambda: plan.run_theta(u, None, tau, steps, max_iters=max_iters, rtol=1e-8))

    first = run(400)[1]
    K = first.iterations_max
    assert first.unconverged_steps == 0 and K < 400, first
    run(K), run(4 * K)
    a, b = [], []
    for _ in range(reps):
        (ta, ra), (tb, rb) = run(K), run(4 * K)
        assert ra.iterations == rb.iterations == first.iterations and rb.unconverged_steps == 0, (ra, rb)
        a.append(ta)
        b.append(tb)
    extra = steps * 15 * K
    # at max_iters = K the run still enqueues 5 (K - k_s) launches for a step that stops at k_s < K
    idle_at_k = sum(5 * (K - k) for k in first.iterations)
    return {"what": "cost of a launch that exits early", "shape": shape, "dims": list(dims), "tau": tau, "steps": steps, "rtol": 1e-8,
            "iterations": list(first.iterations), "K": K, "max_iters_K": spread(a, "ms", 3), "max_iters_4K": spread(b, "ms", 3),
            "extra_launches": extra, "early_exits_already_in_the_run_at_K": idle_at_k,
            "us_per_early_exit_launch": round((statistics.median(b) - statistics.median(a)) * 1e3 / extra, 3),
            "us_per_iteration_at_K": round(statistics.median(a) * 1e3 / (steps * K), 1)}


def advance(n, reps, units=4096):
    shape, dims, u0, amplitude = smooth_problem(n)
    w = normalised(shape)
    explicit = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet")
    plan = L.Plan(shape, dims).set_weights(w)
    b0, b1 = torch.zeros_like(u0), torch.zeros_like(u0)
    row = {"what": f"wall time to advance {units} time units", "shape": shape, "dims": list(dims), "amplitude_start": amplitude(u0)}

    def run_explicit():
        b0.copy_(u0)
        b1.zero_()
        return wall_ms(lambda: explicit.run(b0, b1, units))

    run_explicit()
    ms = [run_explicit()[0] for _ in range(reps)]
    torch.cuda.synchronize()
    result = (b0, b1)[units % 2]
    row["explicit"] = dict(spread(ms, "ms", 2), sweeps=units, amplitude=amplitude(result))
    plan.prepare_theta(units)
    for tau in (64.0, 512.0):
        steps = int(units / tau)

        def run(max_iters):
            b0.copy_(u0)
            return wall_ms(lambda: plan.run_theta(b0, None, tau, steps, max_iters=max_iters, rtol=1e-8))

        first = run(1000)[1]
        K = first.iterations_max
        assert first.unconverged_steps == 0 and K < 1000 and not first.breakdown, first
        run(K)
        ms, out = [], None
        for _ in range(reps):
            t, out = run(K)
            ms.append(t)
        assert out.iterations == first.iterations, (out, first)
        a = amplitude(b0)
        row[f"theta1_tau{int(tau)}"] = dict(spread(ms, "ms", 2), steps=steps, max_iters=K, iterations_total=out.iterations_total,
                                            iterations=list(out.iterations) if steps <= 16 else [out.iterations[0], out.iterations[-1]],
                                            steady_max_abs=out.steady.max_abs, amplitude=a,
                                            amplitude_relative_to_explicit=(a - row["explicit"]["amplitude"]) / row["explicit"]["amplitude"],
                                            speedup_over_explicit=round(row["explicit"]["median_ms"] / statistics.median(ms), 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "theta_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    args = ap.parse_args()
    configs = [("star2d1r", (512, 512)), ("box3d1r", (64, 64, 64))] if args.small else [
        ("star2d1r", (4096, 4096)), ("star2d1r", (16384, 16384)), ("box3d1r", (256, 256, 256))]
    lines = []
    for shape, dims in configs:
        lines.append(kernels(shape, dims, args.reps))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    n = 256 if args.small else 2048
    lines.append(early_exit(n, max(3, args.reps // 2)))
    print(json.dumps(lines[-1]), flush=True)
    lines.append(advance(n, max(3, args.reps // 2), 512 if args.small else 4096))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
