#!/usr/bin/env python3
"""Timings of the fused defect kernel, the V-cycle, multigrid-preconditioned CG and the preconditioned implicit stepper (DESIGN
section 3.12):
   python tools/pcg_timing.py [--out profiles/pcg_timing.jsonl] [--reps 12] [--small] [--cycles-only]

One process, its own plans; rows are written as they finish.
  1. lora_plan_defect (with f) at star2d1r 4096^2 and box3d1r 256^3 beside the two launches it replaces in a cycle -- a source
     sweep of a plan that carries f, and an in-place subtraction of two grids (torch's elementwise kernel on the interior views:
     the bytes of the driver's former subtraction, not its code) -- and beside a plain single sweep: `reps` rounds that ALTERNATE
     them, each launch between two device events of its own; medians.
  2. Microseconds per V(2,2) and per V(1,1) cycle of lora_plan_run_mg_until at 2048^2 and 4096^2: the wall time of a run of 2 K
     cycles minus that of a run of K (tol = 0, one probe each, so set-up and probe cancel), over K, with the launches and bytes
     as the driver counted them (lora_plan_mg_cycle_cost).  --cycles-only stops here and needs nothing this change adds: run
     with LORA_PACKAGE_ROOT pointing at a build of the parent commit it gives the cycle BEFORE the fused defect.
  3. Wall time to max |S(u) + f - u| <= 1e-8 on the Jacobi problem of tools/cg_timing.py (f = 0.125, zero boundary, u0 = 0) at
     2048^2, 8192^2 and the thin 16 x 16384: PCG with V(1,1) and V(2,2), multigrid V(2,2) and CG, in this one process.
  4. Wall time to advance 4096 time units of du/dt = S(u) - u (the problem of tools/theta_timing.py: the lowest eigenmode plus
     1 % noise, zero boundary) at 2048^2 with tau = 64 and 512 and at 8192^2 with tau = 512 and 4096: lora_plan_run_theta_mg
     beside lora_plan_run_theta (max_iters = the largest count a first run needs) and lora_plan_run with 4096 explicit sweeps.
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


def jacobi():
    w = np.zeros(49)
    w[[23, 25, 17, 31]] = 0.25
    return w


def defect_kernel(shape, dims, reps):
    w = normalised(shape)
    plan = L.Plan(shape, dims).set_weights(w)
    u = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    spare, f = torch.zeros_like(u), torch.rand_like(u) - 0.5
    with_f = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(f)
    inner = lambda t: L.interior(shape, t)
    what = {"defect": lambda: plan.defect(u, f, spare), "source_sweep": lambda: with_f.step(u, spare),
            "subtraction": lambda: inner(spare).sub_(inner(u)), "single_sweep": lambda: plan.step(u, spare)}
    for fn in what.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    row = {"what": "lora_plan_defect beside the launches it replaces", "shape": shape, "dims": list(dims), "reps": reps}
    for k in what:
        row[k] = spread(us[k], "us")
    med = lambda k: row[k]["median_us"]
    row["replaced_pair_us"] = round(med("source_sweep") + med("subtraction"), 1)
    row["defect_over_pair"] = round(med("defect") / row["replaced_pair_us"], 3)
    row["defect_over_source_sweep"] = round(med("defect") / med("source_sweep"), 3)
    return row


def cycles(n, smooth, reps, k_cycles):
    shape, dims = "star2d1r", (n, n)
    plan = L.Plan(shape, dims).set_weights(jacobi())
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    x = torch.zeros_like(f)
    plan.prepare_mg(pre=smooth, post=smooth)

    def run(k):
        x.zero_()
        return wall_ms(lambda: plan.run_mg_until(x, f, tol=0.0, pre=smooth, post=smooth, check_every=k, max_times=k))

    run(k_cycles)
    per, r2 = [], None
    for _ in range(reps):
        (t1, _), (t2, r2) = run(k_cycles), run(2 * k_cycles)
        per.append((t2 - t1) * 1e3 / k_cycles)
    launches, nbytes = plan.mg_cycle_cost()
    return {"what": f"one V({smooth},{smooth}) cycle of lora_plan_run_mg_until", "package": os.environ.get("LORA_PACKAGE_ROOT", "this tree"),
            "shape": shape, "dims": list(dims), "cycle": dict(spread(per, "us"), launches=launches, bytes=nbytes, levels=r2.levels,
                                                             us_per_launch=round(statistics.median(per) / launches, 2))}


def solve(dims, reps, tol, with_cg):
    shape = "star2d1r"
    plan = L.Plan(shape, dims).set_weights(jacobi())
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    x = torch.zeros_like(f)
    cap_cg = 4 * max(dims)
    big = dims[0] * dims[1] >= 4096 * 4096

    def pcg(smooth):
        def go():
            x.zero_()
            return wall_ms(lambda: plan.run_pcg_until(x, f, tol=tol, smooth=smooth, check_every=2, max_times=100))
        return go

    def mg():
        x.zero_()
        return wall_ms(lambda: plan.run_mg_until(x, f, tol=tol, pre=2, post=2, omega=0.8, check_every=1, max_times=100))

    def cg():
        x.zero_()
        return wall_ms(lambda: plan.run_cg_until(x, f, tol=tol, check_every=20, max_times=cap_cg))

    row = {"what": f"Jacobi solve: f = 0.125, zero boundary, max |S(u) + f - u| <= {tol:g}", "shape": shape, "dims": list(dims), "tol": tol}
    runs = [("pcg_v11", pcg(1)), ("pcg_v22", pcg(2)), ("multigrid_v22", mg)] + ([("cg", cg)] if with_cg else [])
    for name, fn in runs:
        long_run = name == "cg" and big  # tens of seconds: one run, no warm-up run
        if name == "cg":
            plan.prepare_cg(cap_cg)
        if not long_run:
            fn()
        ms, out = [], None
        for _ in range(1 if long_run else (max(1, reps // 4) if name == "cg" else reps)):
            t, out = fn()
            ms.append(t)
        u = out.until
        entry = dict(spread(ms, "ms", 2), runs=len(ms), times_done=u.times_done, converged=u.converged, residual=u.residual)
        if name != "cg":
            launches, nbytes = plan.mg_cycle_cost()
            entry.update(levels=out.levels, launches_per_cycle=launches, bytes_per_cycle=nbytes)
        if name.startswith("pcg"):
            entry.update(lambda_min=out.lambda_min, lambda_max=out.lambda_max, breakdown=out.breakdown)
        row[name] = entry
        print("#", dims, name, json.dumps(entry), flush=True)
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


def advance(n, taus, reps, units=4096):
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
    row["explicit"] = dict(spread(ms, "ms", 2), sweeps=units, amplitude=amplitude((b0, b1)[units % 2]))

    def entry(ms, out, steps, **more):
        a = amplitude(b0)
        return dict(spread(ms, "ms", 2), steps=steps, iterations_total=out.iterations_total, iterations_max=out.iterations_max,
                    iterations=list(out.iterations) if steps <= 16 else [out.iterations[0], out.iterations[-1]],
                    unconverged_steps=out.unconverged_steps, steady_max_abs=out.steady.max_abs, amplitude=a,
                    amplitude_relative_to_explicit=(a - row["explicit"]["amplitude"]) / row["explicit"]["amplitude"],
                    speedup_over_explicit=round(row["explicit"]["median_ms"] / statistics.median(ms), 3), **more)

    plan.prepare_theta(units)
    for tau in taus:
        steps = int(units / tau)

        def run_cg(max_iters):
            b0.copy_(u0)
            return wall_ms(lambda: plan.run_theta(b0, None, tau, steps, max_iters=max_iters, rtol=1e-8))

        first = run_cg(2000)[1]
        K = first.iterations_max
        assert first.unconverged_steps == 0 and K < 2000 and not first.breakdown, first
        ms, out = [], None
        for _ in range(reps):
            t, out = run_cg(K)
            ms.append(t)
        row[f"theta_cg_tau{int(tau)}"] = entry(ms, out, steps, max_iters=K)
        print("#", n, tau, "cg", json.dumps(row[f"theta_cg_tau{int(tau)}"]), flush=True)
        for smooth, every in ((2, 2), (1, 2), (2, 1)):
            def run_mg():
                b0.copy_(u0)
                return wall_ms(lambda: plan.run_theta_mg(b0, None, tau, steps, max_iters=60, rtol=1e-8, smooth=smooth, check_every=every))

            run_mg()
            ms, out = [], None
            for _ in range(reps):
                t, out = run_mg()
                ms.append(t)
            key = f"theta_mg_v{smooth}{smooth}_every{every}_tau{int(tau)}"
            row[key] = entry(ms, out, steps, max_iters=60, check_every=every)
            print("#", n, tau, key, json.dumps(row[key]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--cycles-only", action="store_true", help="section 2 alone: runs on a build without the entries this change adds")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()
        torch.cuda.empty_cache()

    if not args.cycles_only:
        for shape, dims in ([("star2d1r", (512, 512)), ("box3d1r", (64, 64, 64))] if args.small else [("star2d1r", (4096, 4096)), ("box3d1r", (256, 256, 256))]):
            emit(defect_kernel(shape, dims, args.reps))
    for n in ((256, 512) if args.small else (2048, 4096)):
        for smooth in (2, 1):
            emit(cycles(n, smooth, max(3, args.reps // 3), 4 if args.small else 8))
    if args.cycles_only:
        return
    solve_reps = max(2, args.reps // 3)
    for dims in ([(256, 256), (16, 1024)] if args.small else [(2048, 2048), (8192, 8192), (16, 16384)]):
        emit(solve(dims, solve_reps, 1e-8, True))
    stepper_reps = max(2, args.reps // 4)
    for n, taus in ([(256, (64.0, 512.0))] if args.small else [(2048, (64.0, 512.0)), (8192, (512.0, 4096.0))]):
        emit(advance(n, taus, stepper_reps, 512 if args.small else 4096))


if __name__ == "__main__":
    main()
