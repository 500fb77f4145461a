#!/usr/bin/env python3
"""Time of the variable-coefficient wave step beside the leapfrog step with a source of the same plan:
   python tools/wave_timing.py [--out profiles/wave_timing.jsonl] [--reps 24] [--small]

Both rules move the same four grids per step (cur, prev and a per-cell operand read, prev written), so the expectation is parity.
One process.  Per configuration, after a warm-up of each thing compared on that shape, `reps` rounds that ALTERNATE them, each
between two device events of its own; medians are reported.  The baseline is launched twice per round: the distance of its two
medians is the repeat-to-repeat spread, measured before any ratio is judged.

  single step   lora_plan_step_wave against lora_plan_step_leapfrog_src with a source
  run           120 steps of lora_plan_run_wave against lora_plan_run_leapfrog_src with a source (2D: pairs of two-step launches
                through the plan's scratch grids in both; 3D and 1D: single steps in both)

The wave rule passes where its median is within the larger of that spread and 5 % of the baseline: the 5 % covers the one extra
multiply-add pair per point.
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

MARGIN = 0.05
RUN_STEPS = 120
B, C = 1.9, -0.9     # every product rounds
A_SRC, C_SRC = 1.7, -0.7


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(what, reps):
    for fn in what.values():  # warm-up: code objects, first-need grids
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in what}
    for _ in range(reps):
        for k, fn in what.items():
            us[k].append(event_us(fn))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in us.items()}


def judge(row, name, t):
    base = t["leapfrog_src"]["median_us"]
    spread = abs(t["leapfrog_src_again"]["median_us"] / base - 1.0)
    ratio = t["wave"]["median_us"] / base
    row[name] = t
    row[name + "_spread"] = round(spread, 4)
    row[name + "_wave_over_leapfrog_src"] = round(ratio, 4)
    row[name + "_allowed"] = round(1.0 + max(spread, MARGIN), 4)
    row[name + "_pass"] = ratio <= 1.0 + max(spread, MARGIN)


def timing(shape, dims, reps, run_reps):
    ps = L.padded_shape(shape, dims)
    cur = torch.rand(ps, device="cuda", dtype=torch.float64) * 2 - 1
    prev = torch.rand_like(cur) * 2 - 1
    f = torch.rand_like(cur) * 1e-3
    k = torch.rand_like(cur) * 0.1  # small, so 120 steps of either rule stay finite
    w = L.effective_weights(shape)
    w = w / w.sum()
    p = L.Plan(shape, dims).set_weights(w)
    row = {"shape": shape, "dims": list(dims), "reps": reps, "run_reps": run_reps, "run_steps": RUN_STEPS, "wave_depth": p.wave_depth,
           "leapfrog_depth": p.leapfrog_depth}
    judge(row, "single", alternate({"leapfrog_src": lambda: p.step_leapfrog_src(cur, prev, f, A_SRC, C_SRC),
                                    "wave": lambda: p.step_wave(cur, prev, k, B, C),
                                    "leapfrog_src_again": lambda: p.step_leapfrog_src(cur, prev, f, A_SRC, C_SRC)}, reps))
    cur.uniform_(-1, 1)
    prev.copy_(cur)
    p.prepare_wave(RUN_STEPS)
    # (contractive coefficients: 0.5 u + 0.4 u- and a small k keep both runs bounded over every repetition)
    judge(row, "run", alternate({"leapfrog_src": lambda: p.run_leapfrog_src(prev, cur, f, [0.05], [0.4], RUN_STEPS),
                                 "wave": lambda: p.run_wave(prev, cur, k, 0.5, 0.4, RUN_STEPS),
                                 "leapfrog_src_again": lambda: p.run_leapfrog_src(prev, cur, f, [0.05], [0.4], RUN_STEPS)}, run_reps))
    assert bool(torch.isfinite(cur).all()) and bool(torch.isfinite(prev).all())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_timing.jsonl"))
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--run-reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal on small grids")
    args = ap.parse_args()
    assert (args.reps >= 20 and args.run_reps >= 5) or args.small
    configs = [("star2d1r", (1024, 1024)), ("box2d3r", (512, 512)), ("star3d1r", (64, 64, 64)), ("box3d1r", (64, 64, 64)), ("1d1r", (1 << 18,))] \
        if args.small else \
        [("star2d1r", (8192, 8192)), ("box2d3r", (4096, 4096)), ("star3d1r", (384, 384, 384)), ("box3d1r", (384, 384, 384)), ("1d1r", (1 << 24,))]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for cfg in configs:
            row = timing(*cfg, args.reps, args.run_reps)
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")
            out.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
