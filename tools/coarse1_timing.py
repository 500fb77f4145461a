#!/usr/bin/env python3
"""Timings of the one-launch coarsest-level CG, lora_plan_cg_small, and of plan option coarse1:
   python tools/coarse1_timing.py [--out profiles/coarse1_timing.jsonl] [--reps 12] [--small]

One process, its own plans, warm-ups outside the timing; option off and option on ALTERNATE inside every round; medians; rows are
written as they finish.  No ratio is asked of any row: the comparison is the option-off path of the same process.
  a. The kernel alone against the 5 + 5 iters launches it replaces, at 4 x 4, 6 x 6, 32 x 32 and 4 x 4 x 4 with iters =
     min(64, cells).  The kernel: one launch between two device events of its own.  What it replaces has no public entry of its
     own, so it is measured where it runs: lora_plan_mg_precondition on a two-level hierarchy whose coarsest level has that size
     (the fine grid twice the extents, max_levels = 2), one call between two events, option off and on; the launches replaced
     take (cycle off - cycle on) + the kernel.  Then the same at the corners of the admission bound: 64 x 64 (star2d1r and the
     49 taps of box2d3r), 4 x 512 and 16 x 16 x 16.
  b. Microseconds per V(2,2) cycle of lora_plan_run_mg_until at 2048^2 and 4096^2 (star2d1r, Jacobi taps) and 256^3 (box3d1r,
     normalised taps), as tools/pcg_timing.py measures a cycle (a run of 2 K cycles minus a run of K), with the launches and
     bytes of lora_plan_mg_cycle_cost.
  c. The wall-time rows of DESIGN 3.12 again: to max |S(u) + f - u| <= 1e-8 on the Jacobi problem at 2048^2 and 8192^2 (PCG with
     V(1,1) and V(2,2), multigrid V(2,2)), and 4096 time units of du/dt = S(u) - u at 2048^2 with tau = 64 and 512
     (lora_plan_run_theta_mg, V(2,2), read back every 2 iterations).
  d. With the option on at 2048^2: max_levels chosen so that the coarsest level is 16^2 and 32^2, beside the full depth (4^2) --
     whether stopping the hierarchy earlier pays: a cycle, and the solve of c.
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

OPTION = (("off", 0), ("on", 1))


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


def plans(shape, dims, w):
    return {name: L.Plan(shape, dims).set_weights(w).set_option("coarse1", value) for name, value in OPTION}


def kernel_alone(shape, coarse, reps):
    fine = tuple(2 * n for n in coarse)
    w = normalised(shape)
    iters = min(64, int(np.prod(coarse)))
    small = L.Plan(shape, coarse).set_weights(w)
    assert small.get_option("cg_small") == 1 and L.mg_coarse_dims(shape, fine) == coarse
    gen = torch.Generator(device="cuda").manual_seed(3)
    r0 = torch.zeros(L.padded_shape(shape, coarse), device="cuda", dtype=torch.float64)
    L.interior(shape, r0)[...] = torch.randn(coarse, device="cuda", dtype=torch.float64, generator=gen)
    x, r = torch.zeros_like(r0), torch.zeros_like(r0)
    rf = torch.zeros(L.padded_shape(shape, fine), device="cuda", dtype=torch.float64)
    L.interior(shape, rf)[...] = torch.randn(fine, device="cuda", dtype=torch.float64, generator=gen)
    z = torch.zeros_like(rf)
    two = plans(shape, fine, w)

    def kernel():
        x.zero_()
        r.copy_(r0)
        torch.cuda.synchronize()
        return event_us(lambda: small.cg_small(x, r, iters))

    cycle = {name: (lambda p=p: event_us(lambda: p.mg_precondition(rf, z, max_levels=2))) for name, p in two.items()}
    for _ in range(3):  # warm-up: code objects, the hierarchies
        kernel()
        for fn in cycle.values():
            fn()
    us = {"kernel": [], "off": [], "on": []}
    for _ in range(reps):
        us["kernel"].append(kernel())
        for name, fn in cycle.items():
            us[name].append(fn())
    row = {"what": "lora_plan_cg_small beside the 5 + 5 iters launches it replaces", "shape": shape, "dims": list(coarse), "iters": iters,
           "launches_replaced": 5 + 5 * iters, "reps": reps, "kernel": spread(us["kernel"], "us"),
           "two_level_cycle_off": dict(spread(us["off"], "us"), launches=two["off"].mg_cycle_cost()[0]),
           "two_level_cycle_on": dict(spread(us["on"], "us"), launches=two["on"].mg_cycle_cost()[0])}
    med = lambda k: statistics.median(us[k])
    row["replaced_us"] = round(med("off") - med("on") + med("kernel"), 1)
    row["kernel_over_replaced"] = round(med("kernel") / row["replaced_us"], 4)
    row["us_per_iteration"] = round(med("kernel") / iters, 2)
    return row


def jacobi_problem(dims):
    shape = "star2d1r"
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    return shape, f, torch.zeros_like(f)


def cycles(shape, dims, w, reps, k_cycles, max_levels=0, only=None):
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    x = torch.zeros_like(f)
    ps = {k: p for k, p in plans(shape, dims, w).items() if only is None or k == only}

    def run(p, k):
        x.zero_()
        return wall_ms(lambda: p.run_mg_until(x, f, tol=0.0, pre=2, post=2, check_every=k, max_times=k, max_levels=max_levels))

    for p in ps.values():
        p.prepare_mg(max_levels=max_levels)
        run(p, k_cycles)
    per, last = {k: [] for k in ps}, None
    for _ in range(reps):
        for name, p in ps.items():
            (t1, _), (t2, last) = run(p, k_cycles), run(p, 2 * k_cycles)
            per[name].append((t2 - t1) * 1e3 / k_cycles)
    row = {"what": "one V(2,2) cycle of lora_plan_run_mg_until", "shape": shape, "dims": list(dims), "levels": last.levels,
           "coarsest": list(last.level_dims[-1])}
    for name, p in ps.items():
        launches, nbytes = p.mg_cycle_cost()
        row[name] = dict(spread(per[name], "us"), launches=launches, bytes=nbytes, us_per_launch=round(statistics.median(per[name]) / launches, 2))
    if len(ps) == 2:
        row["on_over_off"] = round(row["on"]["median_us"] / row["off"]["median_us"], 4)
    return row


def solve(dims, reps, tol, max_levels=0, only=None):
    shape, f, x = jacobi_problem(dims)
    ps = {k: p for k, p in plans(shape, dims, jacobi()).items() if only is None or k == only}

    def pcg(smooth):
        return lambda p: p.run_pcg_until(x, f, tol=tol, smooth=smooth, check_every=2, max_times=100, max_levels=max_levels)

    mg = lambda p: p.run_mg_until(x, f, tol=tol, pre=2, post=2, omega=0.8, check_every=1, max_times=100, max_levels=max_levels)
    row = {"what": f"Jacobi solve: f = 0.125, zero boundary, max |S(u) + f - u| <= {tol:g}", "shape": shape, "dims": list(dims), "tol": tol,
           "max_levels": max_levels}
    for name, call in (("pcg_v11", pcg(1)), ("pcg_v22", pcg(2)), ("multigrid_v22", mg)):
        def go(p):
            x.zero_()
            return wall_ms(lambda: call(p))

        for p in ps.values():
            go(p)
        ms, out = {k: [] for k in ps}, {}
        for _ in range(reps):
            for k, p in ps.items():
                t, out[k] = go(p)
                ms[k].append(t)
        row[name] = {}
        for k, p in ps.items():
            u = out[k].until
            launches, nbytes = p.mg_cycle_cost()
            row[name][k] = dict(spread(ms[k], "ms", 2), runs=reps, times_done=u.times_done, converged=u.converged, residual=u.residual,
                                levels=out[k].levels, launches_per_cycle=launches)
        if len(ps) == 2:
            row[name]["on_over_off"] = round(row[name]["on"]["median_ms"] / row[name]["off"]["median_ms"], 4)
        print("#", dims, name, json.dumps(row[name]), flush=True)
    return row


def advance(n, taus, reps, units=4096):
    shape, dims = "star2d1r", (n, n)
    i = torch.arange(1, n + 1, device="cuda", dtype=torch.float64)
    mode = torch.sin(math.pi * i / (n + 1))[:, None] * torch.sin(math.pi * i / (n + 1))[None, :]
    u0 = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(7)
    L.interior(shape, u0)[...] = mode + 0.01 * (torch.rand(dims, device="cuda", dtype=torch.float64, generator=gen) * 2 - 1)
    amplitude = lambda t: float((L.interior(shape, t) * mode).sum() / (mode * mode).sum())
    ps = plans(shape, dims, normalised(shape))
    b0 = torch.zeros_like(u0)
    row = {"what": f"wall time to advance {units} time units, lora_plan_run_theta_mg V(2,2), read back every 2 iterations", "shape": shape,
           "dims": list(dims)}
    for tau in taus:
        steps = int(units / tau)

        def go(p):
            b0.copy_(u0)
            return wall_ms(lambda: p.run_theta_mg(b0, None, tau, steps, max_iters=60, rtol=1e-8, smooth=2, check_every=2))

        for p in ps.values():
            p.prepare_theta(units)
            go(p)
        ms, out, amp = {k: [] for k in ps}, {}, {}
        for _ in range(reps):
            for k, p in ps.items():
                t, out[k] = go(p)
                ms[k].append(t)
                amp[k] = amplitude(b0)
        entry = {k: dict(spread(ms[k], "ms", 2), steps=steps, iterations_total=out[k].iterations_total, iterations_max=out[k].iterations_max,
                         unconverged_steps=out[k].unconverged_steps, amplitude=amp[k], launches_per_cycle=ps[k].mg_cycle_cost()[0]) for k in ps}
        entry["on_over_off"] = round(entry["on"]["median_ms"] / entry["off"]["median_ms"], 4)
        row[f"tau{int(tau)}"] = entry
        print("#", n, tau, json.dumps(entry), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse1_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()
        torch.cuda.empty_cache()

    # (the last four: the corners of the admission bound of option "cg_small" -- four cells a lane, the widest ring, 49 taps)
    for shape, coarse in (("star2d1r", (4, 4)), ("star2d1r", (6, 6)), ("star2d1r", (32, 32)), ("star3d1r", (4, 4, 4)),
                          ("star2d1r", (64, 64)), ("box2d3r", (64, 64)), ("star2d1r", (4, 512)), ("box3d1r", (16, 16, 16))):
        emit(kernel_alone(shape, coarse, args.reps))
    cycle_reps, k = max(3, args.reps // 3), 4 if args.small else 8
    for shape, dims, w in ([("star2d1r", (256, 256), jacobi()), ("box3d1r", (32, 32, 32), normalised("box3d1r"))] if args.small else
                           [("star2d1r", (2048, 2048), jacobi()), ("star2d1r", (4096, 4096), jacobi()), ("box3d1r", (256, 256, 256), normalised("box3d1r"))]):
        emit(cycles(shape, dims, w, cycle_reps, k))
    solve_reps = max(2, args.reps // 3)
    for dims in ([(256, 256)] if args.small else [(2048, 2048), (8192, 8192)]):
        emit(solve(dims, solve_reps, 1e-8))
    n = 256 if args.small else 2048
    emit(advance(n, (64.0, 512.0), max(2, args.reps // 4), 512 if args.small else 4096))
    # d. a shallower hierarchy under the one-launch level: the coarsest level 16^2 and 32^2
    full = int(math.log2(n)) - 1  # n, n / 2, ..., 4
    for levels in (0, full - 2, full - 3):
        row = cycles("star2d1r", (n, n), jacobi(), cycle_reps, k, max_levels=levels, only="on")
        row["what"] += ", option on, the hierarchy cut short"
        emit(row)
        row = solve((n, n), solve_reps, 1e-8, max_levels=levels, only="on")
        row["what"] += ", option on, the hierarchy cut short"
        emit(row)


if __name__ == "__main__":
    main()
