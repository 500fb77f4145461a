#!/usr/bin/env python3
"""Rate of the leapfrog steps with a source and a scale beside the leapfrog steps of the same plan:
   python tools/leapfrog_src_rate.py [--out profiles/leapfrog_src_rate.jsonl] [--reps 24] [--small] [--lib PATH]

One process.  Per configuration, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device
events of its own; medians are reported, and beside every ratio the spread of two identical launches in the same rounds.  Every
bar is against code this change does not touch, with the 10 % margin section 3.5 grants.

  single step      lora_plan_step_leapfrog_src with f / without f / lora_plan_step_leapfrog (the yardstick) / that once more (the
                   spread).  Bars: with f <= 4/3 x leapfrog x 1.10 (four grids of traffic against three); without f <= leapfrog
                   x 1.10.
  two per launch   2D only: lora_plan_step2_leapfrog_src with f / a lora_plan_step2_leapfrog launch / that once more / two single
                   steps with f.  Bars: <= 5/4 x leapfrog2 x 1.10 (five grids against four), and faster than two single steps by
                   more than the spread.
  solve            star2d1r 2048^2 (--small: 256^2), 5-point Jacobi taps, zero halos, f = 0.125: steps and wall time to
                   max |S(u) + f - u| <= 1e-8 for lora_plan_run_chebyshev_until against lora_plan_run_until with the source, and
                   the cost of one probe (source sweep + difference, blocking) against one step.  Reported, no bar.
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
sys.path.insert(0, ROOT)
import lorastencil_amd as L  # noqa: E402

MARGIN = 1.10
A1, C1, A2, C2 = 1.7, -0.7, 1.6, -0.6  # Chebyshev-like coefficients: every product rounds


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(what, reps):
    for fn in what.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in us.items()}


def ratio(t, num, den):
    return round(t[num]["median_us"] / t[den]["median_us"], 3)


def rates(shape, dims, reps):
    cur = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    prev = torch.rand_like(cur) * 2 - 1
    f = torch.rand_like(cur)
    w = L.effective_weights(shape)
    w = w / w.sum()
    p = L.Plan(shape, dims).set_weights(w)
    row = {"shape": shape, "dims": list(dims), "reps": reps, "coefficients": [A1, C1, A2, C2], "leapfrog_depth": p.leapfrog_depth}
    # what a step must equal: a = 1 without f is the leapfrog step, bit for bit
    x, y = prev.clone(), prev.clone()
    p.step_leapfrog(cur, x, C1)
    p.step_leapfrog_src(cur, y, None, 1.0, C1)
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    del x, y
    one = alternate({"src": lambda: p.step_leapfrog_src(cur, prev, f, A1, C1), "nosrc": lambda: p.step_leapfrog_src(cur, prev, None, A1, C1),
                     "leapfrog": lambda: p.step_leapfrog(cur, prev, C1), "leapfrog_again": lambda: p.step_leapfrog(cur, prev, C1)}, reps)
    row["single"] = one
    row["single_src_over_leapfrog"] = ratio(one, "src", "leapfrog")
    row["single_nosrc_over_leapfrog"] = ratio(one, "nosrc", "leapfrog")
    row["single_spread"] = round(abs(ratio(one, "leapfrog_again", "leapfrog") - 1.0), 3)
    row["single_src_bar"] = round(4.0 / 3.0 * MARGIN, 3)
    row["single_src_bar_met"] = row["single_src_over_leapfrog"] <= 4.0 / 3.0 * MARGIN
    row["single_nosrc_bar_met"] = row["single_nosrc_over_leapfrog"] <= MARGIN
    if p.leapfrog_depth == 2:
        o1, o2 = torch.zeros_like(cur), torch.zeros_like(cur)

        def two_singles():
            p.step_leapfrog_src(cur, prev, f, A1, C1)
            p.step_leapfrog_src(prev, cur, f, A2, C2)

        two = alternate({"src2": lambda: p.step2_leapfrog_src(prev, cur, f, o1, o2, A1, C1, A2, C2),
                         "leapfrog2": lambda: p.step2_leapfrog(prev, cur, o1, o2, C1),
                         "leapfrog2_again": lambda: p.step2_leapfrog(prev, cur, o1, o2, C1), "two_single_src": two_singles}, reps)
        row["two"] = two
        row["two_src_over_leapfrog2"] = ratio(two, "src2", "leapfrog2")
        row["two_spread"] = round(abs(ratio(two, "leapfrog2_again", "leapfrog2") - 1.0), 3)
        row["two_src_over_two_singles"] = ratio(two, "src2", "two_single_src")
        row["two_bar"] = round(5.0 / 4.0 * MARGIN, 3)
        row["two_bar_met"] = row["two_src_over_leapfrog2"] <= 5.0 / 4.0 * MARGIN
        row["two_beats_singles"] = row["two_src_over_two_singles"] < 1.0 - row["two_spread"]
        del o1, o2
    return row


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def solve(n, tol, cap_chebyshev, cap_plain):
    shape, dims = "star2d1r", (n, n)
    w = np.zeros(49)
    w[24 - 1] = w[24 + 1] = w[24 - 7] = w[24 + 7] = 0.25
    rho = math.cos(math.pi / (n + 1))
    f = torch.zeros(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64)
    L.interior(shape, f).fill_(0.125)
    row = {"solve": shape, "dims": list(dims), "bc": "dirichlet", "source": "const:0.125", "tol": tol, "rho": rho, "check_every": 100}
    p = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet")
    prev, cur = torch.zeros_like(f), torch.zeros_like(f)
    p.run_chebyshev_until(prev, cur, f, rho, tol, check_every=100, max_times=200)  # warm-up: scratch and probe grids
    prev.zero_()
    cur.zero_()
    r, secs = wall(lambda: p.run_chebyshev_until(prev, cur, f, rho, tol, check_every=100, max_times=cap_chebyshev))
    row["chebyshev"] = {"steps": r.times_done, "converged": r.converged, "residual": r.residual, "seconds": round(secs, 4)}
    q = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(f)
    b0, b1 = torch.zeros_like(f), torch.zeros_like(f)
    q.run_until(b0, b1, tol, check_every=100, max_times=200)
    b0.zero_()
    b1.zero_()
    r, secs = wall(lambda: q.run_until(b0, b1, tol, check_every=100, max_times=cap_plain))
    row["plain_until"] = {"sweeps": r.times_done, "converged": r.converged, "residual": r.residual, "seconds": round(secs, 4)}
    # one probe (what a check adds: a source sweep into a third grid, a difference, the wait for its record) against one step
    probe, step = [], []
    for _ in range(20):
        probe.append(wall(lambda: (q.step(cur, b1), p.diff(b1, cur)))[1])
        step.append(wall(lambda: p.step_leapfrog_src(cur, prev, f, A1, C1))[1])
    row["probe_us"] = round(statistics.median(probe) * 1e6, 1)
    row["step_us_with_sync"] = round(statistics.median(step) * 1e6, 1)
    row["probe_over_step"] = round(statistics.median(probe) / statistics.median(step), 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leapfrog_src_rate.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--lib", help="time this build of liblorastencil_hip.so instead of the tree's (A/B against another commit)")
    args = ap.parse_args()
    if args.lib:
        L._lib.LIB_PATH = os.path.abspath(args.lib)  # before the first call into the engine
    assert args.reps >= 20 or args.small
    configs = [("star2d1r", (2048, 2048)), ("box2d3r", (1024, 1024)), ("box3d1r", (128, 128, 128))] if args.small else \
              [("star2d1r", (16384, 16384)), ("box2d3r", (8192, 8192)), ("box3d1r", (768, 768, 768))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for cfg in configs:
            row = rates(*cfg, args.reps)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
            torch.cuda.empty_cache()
        row = solve(256, 1e-8, 4000, 20000) if args.small else solve(2048, 1e-8, 40000, 40000)
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
