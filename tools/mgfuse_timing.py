#!/usr/bin/env python3
"""Timings of the fused defect-and-restrict launch, lora_plan_mg_defect_restrict, and of plan option mgfuse:
   python tools/mgfuse_timing.py [--out profiles/mgfuse_timing.jsonl] [--reps 12] [--small] [--part a|b|all]

One process, its own plans, warm-ups outside the timing; the variants ALTERNATE inside every round; medians; rows are written as
they finish.  No ratio is asked of any row: the comparison is the unfused path of the same process.
  a. The launch against the pair it replaces at star2d1r 4096^2 and box3d1r 256^3 (normalised taps, the sizes of DESIGN 3.11's
     table), with f and without: lora_plan_mg_defect_restrict, lora_plan_defect and lora_plan_mg_restrict each between two device
     events of its own, and the pair once more between one pair of events.  The row also says whether the coarse grids of the
     two paths hold the same bits at that size.
  b. Microseconds per V(2,2) cycle of lora_plan_run_mg_until (a run of 2 K cycles minus a run of K) and the wall time to
     max |S(u) + f - u| <= 1e-8 on the Jacobi problem of DESIGN 3.11 at 2048^2 and 8192^2, with mgfuse off and on, and the same
     with coarse1 on in both; launches and bytes from lora_plan_mg_cycle_cost.
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
sys.path.insert(0, os.environ.get("LORA_PACKAGE_ROOT", ROOT))
import lorastencil_amd as L  # noqa: E402

VARIANTS = (("off", 0, 0), ("on", 1, 0), ("coarse1_off", 0, 1), ("coarse1_on", 1, 1))  # name, mgfuse, coarse1


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
    return {name: L.Plan(shape, dims).set_weights(w).set_option("mgfuse", fuse).set_option("coarse1", c1) for name, fuse, c1 in VARIANTS}


def launch(shape, dims, with_f, reps):
    plan = L.Plan(shape, dims).set_weights(normalised(shape))
    cdims = L.mg_coarse_dims(shape, dims)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rand = lambda ps: torch.randn(ps, device="cuda", dtype=torch.float64, generator=gen)
    u, f = rand(L.padded_shape(shape, dims)), rand(L.padded_shape(shape, dims))
    spare = torch.zeros_like(u)
    c_fused, c_pair = (torch.zeros(L.padded_shape(shape, cdims), device="cuda", dtype=torch.float64) for _ in range(2))
    src = f if with_f else None
    calls = {
        "fused": lambda: plan.mg_defect_restrict(u, src, c_fused, 0.37),
        "defect": lambda: plan.defect(u, src, spare),
        "restrict": lambda: plan.mg_restrict(spare, c_pair, 0.37),
        "pair_one_window": lambda: (plan.defect(u, src, spare), plan.mg_restrict(spare, c_pair, 0.37)),
    }
    for _ in range(3):  # warm-up: code objects
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(c_fused.view(torch.int64), c_pair.view(torch.int64)))
    us = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            us[name].append(event_us(fn))
    pair = [a + b for a, b in zip(us["defect"], us["restrict"])]
    cells, ccells = float(np.prod(dims)), float(np.prod(cdims))
    row = {"what": "lora_plan_mg_defect_restrict beside lora_plan_defect + lora_plan_mg_restrict", "shape": shape, "dims": list(dims),
           "coarse_dims": list(cdims), "with_f": with_f, "reps": reps, "same_bits": same}
    for name in calls:
        row[name] = spread(us[name], "us")
    row["pair"] = spread(pair, "us")
    med = lambda xs: statistics.median(xs)
    row["pair_spread_us"] = round(max(pair) - min(pair), 1)
    row["saved_us"] = round(med(pair) - med(us["fused"]), 1)
    row["fused_over_pair"] = round(med(us["fused"]) / med(pair), 4)
    # the bytes the launches need when each grid is read or written once: u, f (interior) and the coarse grid; the pair also
    # writes and reads the defect grid
    fused_bytes = 8.0 * (cells * (2 if with_f else 1) + ccells)
    row["fused_gbs"] = round(fused_bytes / med(us["fused"]) / 1e3, 1)
    row["pair_gbs"] = round((fused_bytes + 16.0 * cells) / med(pair) / 1e3, 1)
    return row


def jacobi_problem(dims):
    shape = "star2d1r"
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f)[...] = 0.125
    return shape, f, torch.zeros_like(f)


def cycles(dims, reps, k_cycles):
    shape, f, x = jacobi_problem(dims)
    ps = plans(shape, dims, jacobi())

    def run(p, k):
        x.zero_()
        return wall_ms(lambda: p.run_mg_until(x, f, tol=0.0, pre=2, post=2, check_every=k, max_times=k))

    for p in ps.values():
        p.prepare_mg()
        run(p, k_cycles)
    per, last = {k: [] for k in ps}, None
    for _ in range(reps):
        for name, p in ps.items():
            (t1, _), (t2, last) = run(p, k_cycles), run(p, 2 * k_cycles)
            per[name].append((t2 - t1) * 1e3 / k_cycles)
    row = {"what": "one V(2,2) cycle of lora_plan_run_mg_until", "shape": shape, "dims": list(dims), "levels": last.levels,
           "coarsest": list(last.level_dims[-1]), "reps": reps}
    for name, p in ps.items():
        launches, nbytes = p.mg_cycle_cost()
        row[name] = dict(spread(per[name], "us"), launches=launches, bytes=nbytes)
    row["on_over_off"] = round(row["on"]["median_us"] / row["off"]["median_us"], 4)
    row["coarse1_on_over_off"] = round(row["coarse1_on"]["median_us"] / row["coarse1_off"]["median_us"], 4)
    return row


def solve(dims, reps, tol):
    shape, f, x = jacobi_problem(dims)
    ps = plans(shape, dims, jacobi())

    def go(p):
        x.zero_()
        return wall_ms(lambda: p.run_mg_until(x, f, tol=tol, pre=2, post=2, omega=0.8, check_every=1, max_times=100))

    row = {"what": f"Jacobi solve by multigrid V(2,2): f = 0.125, zero boundary, max |S(u) + f - u| <= {tol:g}", "shape": shape,
           "dims": list(dims), "tol": tol, "reps": reps}
    results = {}
    for name, p in ps.items():
        go(p)
        results[name] = x.clone()
    row["same_bits_off_on"] = bool(torch.equal(results["off"].view(torch.int64), results["on"].view(torch.int64)))
    row["same_bits_coarse1_off_on"] = bool(torch.equal(results["coarse1_off"].view(torch.int64), results["coarse1_on"].view(torch.int64)))
    del results
    ms, out = {k: [] for k in ps}, {}
    for _ in range(reps):
        for k, p in ps.items():
            t, out[k] = go(p)
            ms[k].append(t)
    for k, p in ps.items():
        u = out[k].until
        row[k] = dict(spread(ms[k], "ms", 2), times_done=u.times_done, converged=u.converged, residual=u.residual, levels=out[k].levels,
                      launches_per_cycle=p.mg_cycle_cost()[0])
    row["on_over_off"] = round(row["on"]["median_ms"] / row["off"]["median_ms"], 4)
    row["coarse1_on_over_off"] = round(row["coarse1_on"]["median_ms"] / row["coarse1_off"]["median_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mgfuse_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--part", choices=("a", "b", "all"), default="all", help="the launch alone (a), cycles and solves (b), or both")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()
        torch.cuda.empty_cache()

    for shape, dims in ([("star2d1r", (256, 256)), ("box3d1r", (32, 32, 32))] if args.small else
                        [("star2d1r", (4096, 4096)), ("box3d1r", (256, 256, 256))]):
        for with_f in (True, False) if args.part != "b" else ():
            emit(launch(shape, dims, with_f, args.reps))
    k = 4 if args.small else 8
    for dims in ([(256, 256)] if args.small else [(2048, 2048), (8192, 8192)]) if args.part != "a" else ():
        emit(cycles(dims, args.reps, k))
        emit(solve(dims, args.reps, 1e-8))


if __name__ == "__main__":
    main()
