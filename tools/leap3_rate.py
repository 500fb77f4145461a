#!/usr/bin/env python3
"""Rate of the 3D two-step leapfrog launch (plan option leap3) beside code it does not touch:
   python tools/leap3_rate.py [--out profiles/leap3_rate.jsonl] [--reps 24] [--small] [--lib PATH]

One process.  Per grid and rule, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device
events of its own; medians are reported, and beside every ratio the spread of two identical launches in the same rounds.

  two-step launch  lora_plan_step2_leapfrog[_src] / two single steps of the same plan (stencil3d_step_kernel) / those once more
                   (the spread).  Bar: ratio < 1 - spread.
                   ... / one stencil3d_fused2_kernel launch (two plain sweeps: steps_per_launch = 2, stream3 = 0, lanes3 = 0) /
                   that once more.  Bar: ratio <= 2 (four grids against two) x 1.10 (the margin section 3.5 grants).
  run of 120       lora_plan_run_leapfrog[_src] with leap3 = 1 and 0: GStencils/s and their ratio, reported, no bar.

Rules: "c" (c = -1, the wave equation) and "a,c,f" (scale, coefficient and source; per-step Chebyshev coefficients in the run).
Before anything is timed the launch is compared with two single steps bit for bit on the grid itself.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lorastencil_amd as L  # noqa: E402

MARGIN = 1.10
C = -1.0
A1, C1, A2, C2 = 1.25, -0.25, 1.5, -0.5


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(what, reps):
    for fn in what.values():  # warm-up: code objects, scratch grids
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in us.items()}


def ratio(t, a, b):
    return round(t[a]["median_us"] / t[b]["median_us"], 3)


def rates(shape, dims, rule, reps):
    cur = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    prev = torch.rand_like(cur) * 2 - 1
    f = torch.rand_like(cur) if rule == "a,c,f" else None
    o1, o2 = torch.zeros_like(cur), torch.zeros_like(cur)
    w = L.effective_weights(shape)
    w = w / w.sum()
    on = L.Plan(shape, dims).set_weights(w).set_option("leap3", 1)
    off = L.Plan(shape, dims).set_weights(w)
    plain = L.Plan(shape, dims).set_weights(w).set_option("stream3", 0).set_option("lanes3", 0).set_option("steps_per_launch", 2)
    assert on.leapfrog_depth == 2 and off.leapfrog_depth == 1 and plain.kernel_name == "stencil3d_fused2_kernel"
    h = dims[0]
    row = {"shape": shape, "dims": list(dims), "rule": rule, "reps": reps, "fused2_kernel": plain.kernel_signature}

    if rule == "c":
        def two():
            on.step2_leapfrog(prev, cur, o1, o2, C)

        def singles(x=prev, y=cur):
            off.step_leapfrog(y, x, C)
            off.step_leapfrog(x, y, C)
    else:
        def two():
            on.step2_leapfrog_src(prev, cur, f, o1, o2, A1, C1, A2, C2)

        def singles(x=prev, y=cur):
            off.step_leapfrog_src(y, x, f, A1, C1)
            off.step_leapfrog_src(x, y, f, A2, C2)

    # what the launch must equal, on this grid: two single steps on copies
    two()
    x, y = prev.clone(), cur.clone()
    singles(x, y)
    torch.cuda.synchronize()
    assert torch.equal(L.interior(shape, o1).contiguous().view(torch.int64), L.interior(shape, x).contiguous().view(torch.int64))
    assert torch.equal(L.interior(shape, o2).contiguous().view(torch.int64), L.interior(shape, y).contiguous().view(torch.int64))
    del x, y
    keep = (prev.clone(), cur.clone())  # (timed single steps run in place: they are restored between the phases)

    t = alternate({"two": two, "two_singles": singles, "two_singles_again": singles, "fused2": lambda: plain.stepn_region(2, cur, o1, 0, h),
                   "fused2_again": lambda: plain.stepn_region(2, cur, o1, 0, h)}, reps)
    row["launch"] = t
    row["two_over_two_singles"] = ratio(t, "two", "two_singles")
    row["two_singles_spread"] = round(abs(ratio(t, "two_singles_again", "two_singles") - 1.0), 3)
    row["two_beats_singles"] = row["two_over_two_singles"] < 1.0 - row["two_singles_spread"]
    row["two_over_fused2"] = ratio(t, "two", "fused2")
    row["fused2_spread"] = round(abs(ratio(t, "fused2_again", "fused2") - 1.0), 3)
    row["two_within_fused2_bar"] = row["two_over_fused2"] <= 2.0 * MARGIN
    prev.copy_(keep[0])
    cur.copy_(keep[1])
    del o1, o2, keep

    # a run of 120 steps, leap3 on and off (reported, no bar)
    a, c = L.chebyshev_coeffs(0.9, 1, 120)
    runs = {}
    for name, p in (("run120_leap3", on), ("run120", off)):
        p.prepare_leapfrog(120)
        runs[name] = (lambda p=p: p.run_leapfrog(prev, cur, C, 120)) if rule == "c" else (lambda p=p: p.run_leapfrog_src(prev, cur, f, a, c, 120))
    long = alternate(runs, max(4, reps // 6))
    points = 1.0
    for d in dims:
        points *= d
    for name in runs:
        row[name] = long[name]
        row[name + "_gstencils"] = round(points * 120 / (long[name]["median_us"] * 1e-6) / 1e9, 1)
    row["run120_leap3_over_run120"] = ratio(long, "run120_leap3", "run120")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leap3_rate.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--lib", help="time this build of liblorastencil_hip.so instead of the tree's (A/B against another commit)")
    args = ap.parse_args()
    if args.lib:
        L._lib.LIB_PATH = os.path.abspath(args.lib)  # before the first call into the engine
    assert args.reps >= 20 or args.small
    grids = [("star3d1r", (64, 64, 128)), ("box3d1r", (96, 96, 96))] if args.small else [("star3d1r", (512, 512, 512)), ("box3d1r", (768, 768, 768))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for shape, dims in grids:
            for rule in ("c", "a,c,f"):
                row = rates(shape, dims, rule, args.reps)
                print(json.dumps(row), flush=True)
                out.write(json.dumps(row) + "\n")
                out.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
