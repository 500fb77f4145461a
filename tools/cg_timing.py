#!/usr/bin/env python3
"""Timings of the conjugate-gradient kernels and driver:
   python tools/cg_timing.py [--out profiles/cg_timing.jsonl] [--reps 12] [--small]

One process, its own plans.  Per grid (star2d1r 4096^2 and 16384^2, box3d1r 256^3; normalised taps):
  1. lora_plan_apply_dot beside lora_plan_residual on the same plan (the same reads and no store: the yardstick), a plain single
     sweep (lora_plan_step) and lora_plan_dot -- `reps` rounds that ALTERNATE the four, each between two device events of its
     own; medians.  The three entries with a record block, so their event pairs also hold the fold launch, the copy-back of the
     record and the host's round trip.
  2. microseconds per full iteration of lora_plan_run_cg_until: the wall time of a run of 2 K iterations minus that of a run of
     K (tol = 0, one probe each, so start-up and probe cancel), over K -- and the fraction of 11 grid passes at the 4.85 TB/s a
     big copy_ streams at on this chip.
Last rows: wall time to max |S(u) + f - u| <= tol on the 2048^2 Jacobi problem (f = 0.125, zero boundary, u0 = 0; the solution
is of the order 1e5, so fp64 rounding alone leaves a residual of some 1e-9) for CG, for Chebyshev with the exact rho, and for 40
CG iterations followed by Chebyshev with CG's rho_estimate -- at tol = 1e-9 and at the 1e-8 of section 3.8, 30000 steps at most.
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

COPY_TBS = 4.85


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


def kernels(shape, dims, reps, k_iter):
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    plan = L.Plan(shape, dims).set_weights(w / w.sum())
    assert plan.get_option("cg") == 1
    p = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    q, spare = torch.zeros_like(p), torch.zeros_like(p)
    what = {"residual": lambda: plan.residual(p), "apply_dot": lambda: plan.apply_dot(p, q), "single_sweep": lambda: plan.step(p, spare),
            "dot": lambda: plan.dot(p, q), "apply_dot_again": lambda: plan.apply_dot(p, q)}  # (again: the spread of two identical calls)
    for fn in what.values():  # warm-up: code objects, the plan's record buffer
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    row = {"shape": shape, "dims": list(dims), "reps": reps}
    for k in what:
        row[k] = {"median_us": round(statistics.median(us[k]), 1), "min_us": round(min(us[k]), 1), "max_us": round(max(us[k]), 1)}
    row["spread"] = round(abs(row["apply_dot_again"]["median_us"] / row["apply_dot"]["median_us"] - 1.0), 3)
    row["apply_dot_over_residual"] = round(row["apply_dot"]["median_us"] / row["residual"]["median_us"], 3)
    row["apply_dot_over_residual_plus_sweep"] = round(
        row["apply_dot"]["median_us"] / (row["residual"]["median_us"] + row["single_sweep"]["median_us"]), 3)
    # full iterations through the driver
    f = torch.rand_like(p) - 0.5
    x = torch.zeros_like(p)
    plan.prepare_cg(2 * k_iter)

    def run(n):
        x.zero_()
        return wall_ms(lambda: plan.run_cg_until(x, f, tol=0.0, check_every=n, max_times=n))

    run(k_iter)
    per = []
    for _ in range(max(3, reps // 3)):
        (t1, _), (t2, r2) = run(k_iter), run(2 * k_iter)
        assert r2.until.times_done == 2 * k_iter and not r2.breakdown, r2
        per.append((t2 - t1) * 1e3 / k_iter)
    points = float(np.prod(dims))
    ideal = 11 * 8 * points / (COPY_TBS * 1e12) * 1e6
    row["iteration"] = {"median_us": round(statistics.median(per), 1), "min_us": round(min(per), 1), "max_us": round(max(per), 1),
                        "eleven_passes_at_copy_rate_us": round(ideal, 1), "fraction_of_copy_rate": round(ideal / statistics.median(per), 3)}
    return row


def solve(n, reps, tol):
    shape, dims = "star2d1r", (n, n)
    w = np.zeros(49)
    w[[23, 25, 17, 31]] = 0.25
    plan = L.Plan(shape, dims).set_weights(w)
    cheb = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet")
    rho = math.cos(math.pi / (n + 1))
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    x, prev = torch.zeros_like(f), torch.zeros_like(f)
    cap = 30000
    plan.prepare_cg(cap)
    cheb.prepare_leapfrog(100)

    def cg():
        x.zero_()
        return wall_ms(lambda: plan.run_cg_until(x, f, tol=tol, check_every=20, max_times=cap))

    def chebyshev():
        x.zero_()
        prev.zero_()
        return wall_ms(lambda: cheb.run_chebyshev_until(prev, x, f, rho, tol=tol, check_every=100, max_times=cap))

    def both():
        x.zero_()

        def go():
            first = plan.run_cg_until(x, f, tol=0.0, check_every=40, max_times=40)
            prev.copy_(x)
            return first, cheb.run_chebyshev_until(prev, x, f, first.rho_estimate, tol=tol, check_every=100, max_times=cap)

        return wall_ms(go)

    row = {"shape": shape, "dims": list(dims), "what": f"Jacobi solve: f = 0.125, zero boundary, max |S(u) + f - u| <= {tol:g}, at most {cap} steps",
           "tol": tol, "rho": rho}
    for name, fn in (("cg", cg), ("chebyshev_exact_rho", chebyshev), ("cg40_then_chebyshev", both)):
        fn()
        ms, out = [], None
        for _ in range(max(3, reps // 4)):
            t, out = fn()
            ms.append(t)
        entry = {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2)}
        if name == "cg":
            entry.update(iterations=out.until.times_done, converged=out.until.converged, residual=out.until.residual,
                         rho_estimate=out.rho_estimate, rho_estimate_minus_rho=out.rho_estimate - rho)
        elif name == "chebyshev_exact_rho":
            entry.update(steps=out.times_done, converged=out.converged, residual=out.residual)
        else:
            entry.update(cg_iterations=out[0].until.times_done, rho_estimate=out[0].rho_estimate, rho_estimate_minus_rho=out[0].rho_estimate - rho,
                         chebyshev_steps=out[1].times_done, converged=out[1].converged, residual=out[1].residual)
        row[name] = entry
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    args = ap.parse_args()
    configs = [("star2d1r", (512, 512)), ("box3d1r", (64, 64, 64))] if args.small else [
        ("star2d1r", (4096, 4096)), ("star2d1r", (16384, 16384)), ("box3d1r", (256, 256, 256))]
    lines = []
    for shape, dims in configs:
        row = kernels(shape, dims, args.reps, 10 if args.small else 20)
        lines.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    for tol in (1e-9, 1e-8):
        row = solve(256 if args.small else 2048, args.reps, tol)
        lines.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
