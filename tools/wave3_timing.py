#!/usr/bin/env python3
"""Time of the 3D two-step wave launch (plan option wave3) beside code it does not touch:
   python tools/wave3_timing.py [--out profiles/wave3_timing.jsonl] [--reps 24] [--small] [--form TEXT] [--append] [--lib PATH]

One process.  Per grid, after a warm-up, `reps` rounds that ALTERNATE the things compared, each between two device events of its
own; medians are reported, and beside every ratio the spread of two identical baselines in the same rounds.

  launch      lora_plan_step2_wave / two lora_plan_step_wave launches of the same plan (stencil3d_step_kernel<EPI_WAVE>) / those
              once more (the spread).  Bar: ratio < 1 - spread.  Five grids move where two single steps move eight: 0.625.
  run of 120  lora_plan_run_wave with wave3 = 1 / with wave3 = 0 / that once more (the spread): GStencils/s and the ratio.  Same bar.

The taps are the shape's own in zero-sum form, k is uniform in 0.05 .. 0.25, b = 2, c = -1: a stable wave equation, so the
in-place baseline stays finite however long it is timed.  Before anything is timed the launch is compared with two single steps
bit for bit on the timed grid.  --form names the form of the kernel the library was built with; the word goes into every row.
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

B, C = 2.0, -1.0
STEPS = 120


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


def timings(shape, dims, reps, form):
    cur = torch.rand(L.padded_shape(shape, dims), device="cuda", dtype=torch.float64) * 2 - 1
    prev = cur + (torch.rand_like(cur) * 2 - 1) * 1e-3
    k = torch.rand_like(cur) * 0.2 + 0.05
    o1, o2 = torch.zeros_like(cur), torch.zeros_like(cur)
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)].copy()
    w = w / w.sum()
    w[w.size // 2] -= w.sum()  # the zero-sum form
    on = L.Plan(shape, dims).set_weights(w).set_option("wave3", 1)
    off = L.Plan(shape, dims).set_weights(w)
    assert on.wave_depth == 2 and off.wave_depth == 1
    row = {"shape": shape, "dims": list(dims), "form": form, "reps": reps, "b": B, "c": C}

    def two():
        on.step2_wave(prev, cur, k, o1, o2, B, C)

    def singles(x=prev, y=cur):
        off.step_wave(y, x, k, B, C)
        off.step_wave(x, y, k, B, C)

    # what the launch must equal, on this grid: two single steps on copies
    two()
    x, y = prev.clone(), cur.clone()
    singles(x, y)
    torch.cuda.synchronize()
    assert torch.equal(L.interior(shape, o1).contiguous().view(torch.int64), L.interior(shape, x).contiguous().view(torch.int64))
    assert torch.equal(L.interior(shape, o2).contiguous().view(torch.int64), L.interior(shape, y).contiguous().view(torch.int64))
    del x, y
    row["bit_equal"] = True
    keep = (prev.clone(), cur.clone())  # (timed single steps run in place: they are restored between the phases)

    t = alternate({"two": two, "two_singles": singles, "two_singles_again": singles}, reps)
    row["launch"] = t
    row["two_over_two_singles"] = ratio(t, "two", "two_singles")
    row["two_singles_spread"] = round(abs(ratio(t, "two_singles_again", "two_singles") - 1.0), 3)
    row["launch_bar_met"] = row["two_over_two_singles"] < 1.0 - row["two_singles_spread"]
    prev.copy_(keep[0])
    cur.copy_(keep[1])
    del o1, o2, keep

    # a run of 120 steps, wave3 on and off, the baseline twice per round
    runs = {}
    for name, p in (("run120_wave3", on), ("run120", off), ("run120_again", off)):
        p.prepare_wave(STEPS)
        runs[name] = lambda p=p: p.run_wave(prev, cur, k, B, C, STEPS)
    long = alternate(runs, reps)
    points = 1.0
    for d in dims:
        points *= d
    for name in runs:
        row[name] = long[name]
        row[name + "_gstencils"] = round(points * STEPS / (long[name]["median_us"] * 1e-6) / 1e9, 1)
    row["run120_wave3_over_run120"] = ratio(long, "run120_wave3", "run120")
    row["run120_spread"] = round(abs(ratio(long, "run120_again", "run120") - 1.0), 3)
    row["run_bar_met"] = row["run120_wave3_over_run120"] < 1.0 - row["run120_spread"]
    assert bool(torch.isfinite(cur).all())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave3_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    ap.add_argument("--form", default="carried, 2 workgroups per CU", help="the form of the kernel this build holds")
    ap.add_argument("--append", action="store_true", help="add the rows to --out (another form of the kernel) instead of replacing it")
    ap.add_argument("--lib", help="time this build of liblorastencil_hip.so instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        L._lib.LIB_PATH = os.path.abspath(args.lib)  # before the first call into the engine
    assert args.reps >= 24 or args.small
    small = [("star3d1r", (64, 64, 128)), ("box3d1r", (96, 96, 96))]
    grids = small if args.small else [("star3d1r", (384, 384, 384)), ("box3d1r", (384, 384, 384)), ("star3d1r", (512, 512, 512))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as out:
        for shape, dims in grids:
            row = timings(shape, dims, args.reps, args.form)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
