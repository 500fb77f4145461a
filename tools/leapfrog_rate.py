#!/usr/bin/env python3
"""Rate of the leapfrog steps beside the source sweeps of the same plan:
   python tools/leapfrog_rate.py [--out profiles/leapfrog_rate.jsonl] [--reps 24] [--small] [--lib PATH]

One process.  Per configuration, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device
events of its own; medians are reported, and beside every ratio the spread of two identical launches in the same rounds.

  single step      lora_plan_step_leapfrog / lora_plan_step of a plan with a source (the yardstick: the same three grids of
                   traffic) / that once more (the spread).  Bar: leapfrog <= source x 1.10 (the margin section 3.5 grants).
  two per launch   2D only: lora_plan_step2_leapfrog / a stencil2d_source2_kernel launch (three grids against four) / that once
                   more / two single leapfrog steps.  Bars: leapfrog <= 4/3 x source x 1.10, and faster than two single steps by
                   more than the spread.
  run of 120       lora_plan_run_leapfrog: GStencils/s, reported, no bar.
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


def rates(shape, dims, reps):
    cur = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    prev = torch.rand_like(cur) * 2 - 1
    b = torch.zeros_like(cur)
    f = torch.rand_like(cur)
    w = L.effective_weights(shape)
    w = w / w.sum()
    leap = L.Plan(shape, dims).set_weights(w)
    plain = L.Plan(shape, dims).set_weights(w)
    src = L.Plan(shape, dims).set_weights(w).set_source(f)
    row = {"shape": shape, "dims": list(dims), "reps": reps, "c": C, "leapfrog_depth": leap.leapfrog_depth, "source_kernel": src.kernel_signature}
    # one step, and what it must equal: the plain sweep, then + c * prev on the interior (c = -1: the product is exact)
    plain.step(cur, b)
    want = prev.clone()
    L.interior(shape, want).copy_(L.interior(shape, b) + C * L.interior(shape, prev))
    keep = prev.clone()
    leap.step_leapfrog(cur, prev, C)
    torch.cuda.synchronize()
    assert torch.equal(prev, want)
    prev.copy_(keep)
    del want, keep
    one = alternate({"leapfrog": lambda: leap.step_leapfrog(cur, prev, C), "source": lambda: src.step(cur, b),
                     "source_again": lambda: src.step(cur, b)}, reps)
    row["single"] = one
    row["single_leapfrog_over_source"] = round(one["leapfrog"]["median_us"] / one["source"]["median_us"], 3)
    row["single_spread"] = round(abs(one["source_again"]["median_us"] / one["source"]["median_us"] - 1.0), 3)
    row["single_bar_met"] = row["single_leapfrog_over_source"] <= MARGIN
    if leap.leapfrog_depth == 2:
        assert src.kernel_name == "stencil2d_source2_kernel"
        n = dims[0]
        o1, o2 = torch.zeros_like(cur), torch.zeros_like(cur)

        def two_singles():
            leap.step_leapfrog(cur, prev, C)
            leap.step_leapfrog(prev, cur, C)

        two = alternate({"leapfrog2": lambda: leap.step2_leapfrog(prev, cur, o1, o2, C), "source2": lambda: src.stepn_region(2, cur, b, 0, n),
                         "source2_again": lambda: src.stepn_region(2, cur, b, 0, n), "two_single_leapfrog": two_singles}, reps)
        row["two"] = two
        row["two_leapfrog_over_source2"] = round(two["leapfrog2"]["median_us"] / two["source2"]["median_us"], 3)
        row["two_spread"] = round(abs(two["source2_again"]["median_us"] / two["source2"]["median_us"] - 1.0), 3)
        row["two_leapfrog_over_two_singles"] = round(two["leapfrog2"]["median_us"] / two["two_single_leapfrog"]["median_us"], 3)
        row["two_bar_met"] = row["two_leapfrog_over_source2"] <= 4.0 / 3.0 * MARGIN
        row["two_beats_singles"] = row["two_leapfrog_over_two_singles"] < 1.0 - row["two_spread"]
        del o1, o2
    # a run of 120 steps (reported, no bar)
    leap.prepare_leapfrog(120)
    long = alternate({"run120": lambda: leap.run_leapfrog(prev, cur, C, 120)}, max(3, reps // 6))
    row["run120"] = long["run120"]
    points = 1.0
    for d in dims:
        points *= d
    row["run120_gstencils"] = round(points * 120 / (long["run120"]["median_us"] * 1e-6) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leapfrog_rate.jsonl"))
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


if __name__ == "__main__":
    main()
