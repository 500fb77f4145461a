#!/usr/bin/env python3
"""Timings of the multigrid transfer kernels and the V-cycle driver:
   python tools/mg_timing.py [--out profiles/mg_timing.jsonl] [--reps 12] [--small]

One process, its own plans.
  1. Per grid (star2d1r 4096^2, box3d1r 256^3; normalised taps): lora_plan_mg_restrict and lora_plan_mg_prolong_add beside a plain
     single sweep of the same plan (lora_plan_step) and the two halves of a level's residual pass -- a source sweep of a plan
     that carries f, and an in-place subtraction of two grids (torch's elementwise kernel on the interior views: the bytes of the
     driver's own subtraction, not its code) -- `reps` rounds that ALTERNATE them, each between two device events of its own;
     medians.
  2. Microseconds per V(2,2) cycle of lora_plan_run_mg_until: the wall time of a run of 2 K cycles minus that of a run of K
     (tol = 0, one probe each, so set-up and probe cancel), over K -- with the launches and bytes of a cycle as the driver
     counted them (lora_plan_mg_cycle_cost) and what those bytes would take at the 4.85 TB/s a big copy_ streams at.
  3. Wall time to max |S(u) + f - u| <= 1e-8 on the Jacobi problem of tools/cg_timing.py (f = 0.125, zero boundary, u0 = 0) at
     2048^2 and 8192^2 for multigrid V(2,2), CG, and Chebyshev with the exact rho, in this one process.  The solution grows with
     the square of the side, and fp64 rounding with it: a row says whether its run converged and what residual it reached.
Capturing a cycle in a hipGraph is NOT measured here: lora_plan_run_mg_until returns its probe to the host and, like every
reduction entry, refuses a capturing stream; there is no entry that enqueues cycles without a probe.
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


def summary(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def kernels(shape, dims, reps, k_cycles):
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    w = w / w.sum()
    plan = L.Plan(shape, dims).set_weights(w)
    assert plan.get_option("mg") == 1
    cdims = L.mg_coarse_dims(shape, dims)
    fine = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    spare, f = torch.zeros_like(fine), torch.rand_like(fine) - 0.5
    coarse = torch.rand(L.padded_shape(shape, cdims), device="cuda", dtype=torch.float64) * 2 - 1
    with_f = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(f)
    inner = lambda t: L.interior(shape, t)
    what = {"restrict": lambda: plan.mg_restrict(fine, coarse, 1.0), "prolong_add": lambda: plan.mg_prolong_add(coarse, fine),
            "single_sweep": lambda: plan.step(fine, spare), "source_sweep": lambda: with_f.step(fine, spare),
            "subtraction": lambda: inner(spare).sub_(inner(fine))}
    for fn in what.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    row = {"shape": shape, "dims": list(dims), "coarse_dims": list(cdims), "reps": reps}
    for k in what:
        row[k] = summary(us[k])
    sweep = row["single_sweep"]["median_us"]
    row["restrict_over_sweep"] = round(row["restrict"]["median_us"] / sweep, 3)
    row["prolong_add_over_sweep"] = round(row["prolong_add"]["median_us"] / sweep, 3)
    row["residual_pass_us"] = round(row["source_sweep"]["median_us"] + row["subtraction"]["median_us"], 1)
    # whole cycles through the driver
    x = torch.zeros_like(fine)
    plan.prepare_mg()

    def run(n):
        x.zero_()
        return wall_ms(lambda: plan.run_mg_until(x, f, tol=0.0, check_every=n, max_times=n))

    run(k_cycles)
    per = []
    for _ in range(max(3, reps // 3)):
        (t1, _), (t2, r2) = run(k_cycles), run(2 * k_cycles)
        assert r2.until.times_done == 2 * k_cycles and not r2.until.diverged, r2
        per.append((t2 - t1) * 1e3 / k_cycles)
    launches, nbytes = plan.mg_cycle_cost()
    ideal = nbytes / (COPY_TBS * 1e12) * 1e6
    row["cycle"] = dict(summary(per), launches=launches, bytes=nbytes, levels=r2.levels, level_dims=[list(d) for d in r2.level_dims],
                        bytes_at_copy_rate_us=round(ideal, 1), us_per_launch=round(statistics.median(per) / launches, 2))
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
    cap_cg, cap_cheb = 4 * n, 10 * n  # CG needs about 2 n iterations, Chebyshev about 6 n steps
    long_runs = n >= 4096           # CG and Chebyshev then take tens of seconds: one run each, no warm-up run
    plan.prepare_mg()
    plan.prepare_cg(cap_cg)
    cheb.prepare_leapfrog(100)

    def mg():
        x.zero_()
        return wall_ms(lambda: plan.run_mg_until(x, f, tol=tol, pre=2, post=2, omega=0.8, check_every=1, max_times=60))

    def cg():
        x.zero_()
        return wall_ms(lambda: plan.run_cg_until(x, f, tol=tol, check_every=20, max_times=cap_cg))

    def chebyshev():
        x.zero_()
        prev.zero_()
        return wall_ms(lambda: cheb.run_chebyshev_until(prev, x, f, rho, tol=tol, check_every=100, max_times=cap_cheb))

    row = {"shape": shape, "dims": list(dims), "what": f"Jacobi solve: f = 0.125, zero boundary, max |S(u) + f - u| <= {tol:g}", "tol": tol, "rho": rho}
    for name, fn in (("multigrid_v22", mg), ("cg", cg), ("chebyshev_exact_rho", chebyshev)):
        quick = name == "multigrid_v22" or not long_runs
        if quick:
            fn()  # warm-up
        ms, out = [], None
        for _ in range(reps if name == "multigrid_v22" else (max(1, reps // 4) if quick else 1)):
            t, out = fn()
            ms.append(t)
        entry = {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2), "runs": len(ms)}
        u = out if name == "chebyshev_exact_rho" else out.until
        entry.update(times_done=u.times_done, converged=u.converged, residual=u.residual)
        if name == "multigrid_v22":
            launches, nbytes = plan.mg_cycle_cost()
            entry.update(levels=out.levels, launches_per_cycle=launches, bytes_per_cycle=nbytes, ms_per_cycle=round(entry["median_ms"] / max(u.times_done, 1), 3))
        row[name] = entry
        print("#", name, json.dumps(entry), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--solve-reps", type=int, default=4, help="runs of a timed solve (the CG and Chebyshev runs take a quarter, at least one)")
    args = ap.parse_args()
    configs = [("star2d1r", (512, 512)), ("box3d1r", (64, 64, 64))] if args.small else [("star2d1r", (4096, 4096)), ("box3d1r", (256, 256, 256))]
    lines = []
    for shape, dims in configs:
        row = kernels(shape, dims, args.reps, 4 if args.small else 8)
        lines.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    for n in ((256, 512) if args.small else (2048, 8192)):
        row = solve(n, args.solve_reps, 1e-8)
        lines.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
