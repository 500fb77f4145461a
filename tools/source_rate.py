#!/usr/bin/env python3
"""Rate of the sweeps with a source term beside the plain sweeps of the same plan:
   python tools/source_rate.py [--out profiles/source_rate.jsonl] [--reps 24] [--small] [--lib PATH]

One process.  Per configuration, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device
events of its own; medians are reported, and beside every ratio the spread of two identical launches in the same rounds.

  single sweep     lora_plan_step with a source / without one (the yardstick) / without one once more (the spread).
                   Bar: source <= 1.5 x plain (24 instead of 16 bytes per point) x 1.10 (the margin section 3.5 grants).
  two per launch   2D only: lora_plan_stepn_region(2) with a source / a two-application launch of the existing tile kernel
                   (options steps_per_launch = 2, stream = 0, wg = 0) / that once more / two single source sweeps.
                   Bars: source <= 1.5 x tile kernel x 1.10, and faster than two single source sweeps by more than the spread.
  run of 120       lora_plan_run with and without a source: reported, no bar.
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
    a = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    b = torch.zeros_like(a)
    f = torch.rand_like(a)
    w = L.effective_weights(shape)
    w = w / w.sum()
    plain = L.Plan(shape, dims).set_weights(w)
    src = L.Plan(shape, dims).set_weights(w).set_source(f)
    row = {"shape": shape, "dims": list(dims), "reps": reps, "plain_kernel": plain.kernel_signature, "source_kernel": src.kernel_signature}
    # one sweep, and what it must equal: the plain sweep + f on the interior
    plain.step(a, b)
    want = b.clone()
    L.interior(shape, want).add_(L.interior(shape, f))
    b.zero_()
    src.step(a, b)
    torch.cuda.synchronize()
    assert torch.equal(b, want)
    one = alternate({"source": lambda: src.step(a, b), "plain": lambda: plain.step(a, b), "plain_again": lambda: plain.step(a, b)}, reps)
    row["single"] = one
    row["single_source_over_plain"] = round(one["source"]["median_us"] / one["plain"]["median_us"], 3)
    row["single_spread"] = round(abs(one["plain_again"]["median_us"] / one["plain"]["median_us"] - 1.0), 3)
    row["single_bar_met"] = row["single_source_over_plain"] <= 1.5 * MARGIN
    if len(dims) == 2:
        tile = L.Plan(shape, dims).set_weights(w).set_option("steps_per_launch", 2).set_option("stream", 0).set_option("wg", 0)
        assert tile.kernel_name == "stencil2d_fused2_kernel" and src.get_option("steps_per_launch") == 2
        n = dims[0]
        c = torch.zeros_like(a)

        def two_singles():
            src.step(a, c)
            src.step(c, b)

        two = alternate({"source2": lambda: src.stepn_region(2, a, b, 0, n), "tile2": lambda: tile.stepn_region(2, a, b, 0, n),
                         "tile2_again": lambda: tile.stepn_region(2, a, b, 0, n), "two_single_source": two_singles}, reps)
        row["tile_kernel"] = tile.kernel_signature
        row["two"] = two
        row["two_source_over_tile"] = round(two["source2"]["median_us"] / two["tile2"]["median_us"], 3)
        row["two_spread"] = round(abs(two["tile2_again"]["median_us"] / two["tile2"]["median_us"] - 1.0), 3)
        row["two_source_over_two_singles"] = round(two["source2"]["median_us"] / two["two_single_source"]["median_us"], 3)
        row["two_bar_met"] = row["two_source_over_tile"] <= 1.5 * MARGIN
        row["two_beats_singles"] = row["two_source_over_two_singles"] < 1.0 - row["two_spread"]
        del c
    # a run of 120 sweeps with and without a source (reported, no bar)
    src.prepare_run(120)
    plain.prepare_run(120)

    def run(p):
        p.run(a, b, 120)

    long = alternate({"source": lambda: run(src), "plain": lambda: run(plain)}, max(3, reps // 6))
    row["run120"] = long
    row["run120_source_over_plain"] = round(long["source"]["median_us"] / long["plain"]["median_us"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_rate.jsonl"))
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
