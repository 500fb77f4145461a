#!/usr/bin/env python3
"""The bits of every solver driver (csrc/cg.cpp, mg.cpp, chebyshev.cpp, hostrun.cpp; DESIGN sections 3.8 - 3.15), for a line-by-line
comparison of two builds:
   python tools/solver_bits.py --out profiles/solver_bits_new.jsonl
   LORA_PACKAGE_ROOT=<a build of another commit> python tools/solver_bits.py --out profiles/solver_bits_parent.jsonl

One process, the shapes' own taps divided by their sum (the thread's normalise default: point-symmetric, every shape).  Entries:
run_cg_until, run_pcg_until, run_mg_until, run_chebyshev_until, run_theta, run_theta_mg, mg_precondition with (1, 1) and (9, 8),
and the six run_host_* operators on them.  Grids, the smallest at which each path exists: 1D 1026 (CG and the stepper only);
star2d1r and box2d3r at 37 x 70 (levels 18 x 34, 9 x 16, 4 x 8: odd extents, three coarsenings); star3d1r and box3d1r at
18 x 20 x 36.  Per entry and grid a few calls that between them take every value of every choice -- both norms against with and
without f, check_every 2 and 4 (1 and 3 where cycles or read-backs are counted), the options mgfuse and coarse1 each off and on for
everything with a V-cycle in it -- and a run with max_times below check_every, a run of no steps and a stepper run whose max_iters
is exhausted.  Per call: inputs from a fixed seed, the halo of f and every grid the call only writes filled with one NaN pattern,
one call, then one JSON line with the SHA-256 of each caller grid (whole padded array: a cell the call must not write keeps what
it held), every field of the result (floats as hex), iterations[] and mg_cycle_cost.  Nothing here depends on the build, so two
builds that compute the same bits write the same file.
"""
import argparse
import hashlib
import itertools
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("LORA_PACKAGE_ROOT", ROOT))
import lorastencil_amd as L  # noqa: E402

GRIDS = [("1d2r", (1026,)), ("star2d1r", (37, 70)), ("box2d3r", (37, 70)), ("star3d1r", (18, 20, 36)), ("box3d1r", (18, 20, 36))]
POISON = 0x7ff8dead0000beef  # a quiet NaN no arithmetic produces
# (norm, with_f, which check_every, (mgfuse, coarse1)): every pair of norm and f, every value of the rest twice
COVER = [("max", True, 0, (0, 0)), ("rms", False, 1, (1, 1)), ("rms", True, 0, (1, 0)), ("max", False, 1, (0, 1))]


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def plain(r):
    """a result with its floats as hex, its tuples as lists"""
    if isinstance(r, float):
        return r.hex()
    if isinstance(r, (bool, np.bool_)):
        return int(r)
    if isinstance(r, (tuple, list)):
        return [plain(v) for v in r]
    return r


class Problem:
    """u0 (boundary values in its halo) and f (its halo the NaN pattern: no entry reads it) of one grid, on the host and device"""

    def __init__(self, shape, dims):
        rng = np.random.default_rng(zlib.crc32(repr(("solver_bits", shape, dims)).encode()))
        ps = L.padded_shape(shape, dims)
        self.shape, self.dims, self.nd = shape, dims, len(dims)
        self.u0 = rng.standard_normal(ps)
        f = np.full(ps, np.array([POISON], dtype=np.uint64).view(np.float64)[0])
        L.interior(shape, f)[...] = rng.standard_normal(dims)
        self.f0 = f
        self.u, self.f, self.v = (torch.from_numpy(a.copy()).cuda() for a in (self.u0, f, self.u0))

    def reset(self):
        self.u.copy_(torch.from_numpy(self.u0))
        self.f.copy_(torch.from_numpy(self.f0))
        self.v.copy_(torch.from_numpy(self.u0))

    def poison(self, t):
        t.view(torch.int64).fill_(POISON)

    def source(self, with_f):  # (a host operator uploads the whole array: no NaN pattern in its source)
        return np.nan_to_num(self.f0) if with_f else None


class Defaults:
    """the thread's mgfuse and coarse1 defaults, which the plans made inside take"""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        self.old = L.set_default_mgfuse(self.opts[0]), L.set_default_coarse1(self.opts[1])

    def __exit__(self, *exc):
        L.set_default_mgfuse(self.old[0])
        L.set_default_coarse1(self.old[1])


def cost(plan):
    try:
        return plain(plan.mg_cycle_cost())
    except L.LoraError:
        return None


def plan_rows(pb):
    shape, dims, multigrid = pb.shape, pb.dims, pb.nd > 1
    plans = {}
    for opts in (itertools.product((0, 1), (0, 1)) if multigrid else [(0, 0)]):
        with Defaults(opts):
            plans[opts] = L.Plan(shape, dims)
    w = plans[0, 0].weights
    assert plans[0, 0].get_option("cg") == 1 and np.array_equal(w, w[::-1]) and abs(w.sum() - 1.0) < 1e-12

    def row(entry, opts, args, grids, result):
        return dict(entry=entry, shape=shape, dims=list(dims), mgfuse=opts[0], coarse1=opts[1], args=plain(args), grids=[sha(g) for g in grids],
                    result=plain(result), mg_cycle_cost=cost(plans[opts]))

    def until(entry, every, call, grids, with_options):
        """the covering calls with two rounds each, and a run shorter than its first round"""
        for i, (norm, with_f, which, opts) in enumerate(COVER + COVER[:1]):
            opts = opts if with_options else (0, 0)
            ce = every[which]
            cap = 2 * ce if i < len(COVER) else ce - 1
            pb.reset()
            r = call(plans[opts], pb.f if with_f else None, dict(tol=0.0, norm=norm, check_every=ce, max_times=cap))
            yield row(entry, opts, (norm, with_f, ce, cap), grids, r)

    yield from until("run_cg_until", (2, 4), lambda p, f, kw: p.run_cg_until(pb.u, f, **kw), (pb.u, pb.f), False)
    for with_f, theta, steps, max_iters in ((True, 1.0, 3, 40), (False, 0.5, 3, 40), (True, 0.5, 3, 2), (False, 1.0, 0, 40)):
        pb.reset()
        r = plans[0, 0].run_theta(pb.u, pb.f if with_f else None, 8.0, steps, theta=theta, max_iters=max_iters, rtol=1e-8)
        yield row("run_theta", (0, 0), (with_f, theta, steps, max_iters), (pb.u, pb.f), r)
    if not multigrid:
        return
    yield from until("run_chebyshev_until", (2, 4), lambda p, f, kw: p.run_chebyshev_until(pb.v, pb.u, f, 0.9, **kw), (pb.v, pb.u, pb.f), False)
    yield from until("run_pcg_until", (2, 4), lambda p, f, kw: p.run_pcg_until(pb.u, f, smooth=1, **kw), (pb.u, pb.f), True)
    yield from until("run_mg_until", (1, 3), lambda p, f, kw: p.run_mg_until(pb.u, f, pre=1, post=2, **kw), (pb.u, pb.f), True)
    for (_, with_f, which, opts), (steps, max_iters) in zip(COVER + COVER[:1], ((2, 30), (2, 30), (2, 2), (2, 30), (0, 30))):
        pb.reset()
        r = plans[opts].run_theta_mg(pb.u, pb.f if with_f else None, 8.0, steps, theta=0.5, max_iters=max_iters, rtol=1e-8, smooth=1,
                                     check_every=(1, 3)[which])
        yield row("run_theta_mg", opts, (with_f, (1, 3)[which], steps, max_iters), (pb.u, pb.f), r)
    for (_, _, which, opts) in COVER:
        sigma, tau = ((1.0, 1.0), (9.0, 8.0))[which]
        pb.reset()
        pb.poison(pb.v)  # z: written whole
        r = pb.u.clone()
        pb.poison(pb.u)  # r: only its interior is read
        L.interior(shape, pb.u).copy_(L.interior(shape, r))
        plans[opts].mg_precondition(pb.u, pb.v, sigma=sigma, tau=tau, pre=2, post=2)
        yield row("mg_precondition", opts, (sigma, tau), (pb.u, pb.v), None)


def host_rows(pb):
    shape, dims, multigrid = pb.shape, pb.dims, pb.nd > 1

    def row(entry, opts, args, out, result):
        return dict(entry=entry, shape=shape, dims=list(dims), mgfuse=opts[0], coarse1=opts[1], args=plain(args),
                    grids=[hashlib.sha256(out.tobytes()).hexdigest()], result=plain(result))

    for norm, with_f, _, opts in COVER[:2]:
        src = pb.source(with_f)
        out, r, _ = L.run_host_cg(shape, pb.u0, 0.0, source=src, norm=norm, check_every=2, max_times=4)
        yield row("run_host_cg", (0, 0), (norm, with_f), out, r)
        out, r, _ = L.run_host_theta(shape, pb.u0, 8.0, 2, source=src, theta=0.5, max_iters=40, rtol=1e-8)
        yield row("run_host_theta", (0, 0), (with_f,), out, r)
        if not multigrid:
            continue
        out, r, _ = L.run_host_chebyshev(shape, pb.u0, 0.9, source=src, tol=0.0, norm=norm, check_every=2, max_times=4)
        yield row("run_host_chebyshev", (0, 0), (norm, with_f), out, r)
        with Defaults(opts):
            out, r, _ = L.run_host_pcg(shape, pb.u0, 0.0, source=src, smooth=1, norm=norm, check_every=2, max_times=4)
            yield row("run_host_pcg", opts, (norm, with_f), out, r)
            out, r, _ = L.run_host_mg(shape, pb.u0, 0.0, source=src, pre=1, post=2, norm=norm, check_every=1, max_times=2)
            yield row("run_host_mg", opts, (norm, with_f), out, r)
            out, r, _ = L.run_host_theta_mg(shape, pb.u0, 8.0, 2, source=src, theta=0.5, max_iters=30, rtol=1e-8, smooth=1, check_every=3)
            yield row("run_host_theta_mg", opts, (with_f,), out, r)
    if multigrid:
        out, r, _ = L.run_host_chebyshev(shape, pb.u0, 0.9, times=5, source=pb.source(True))
        yield row("run_host_chebyshev", (0, 0), ("times", True), out, r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    old = L._lib.lib().lora_set_default_normalize(1)
    try:
        with open(args.out, "w") as fh:
            for shape, dims in GRIDS:
                pb = Problem(shape, dims)
                n = 0
                for row in itertools.chain(plan_rows(pb), host_rows(pb)):
                    fh.write(json.dumps(row) + "\n")
                    fh.flush()
                    n += 1
                print(shape, dims, n, "rows", flush=True)
                torch.cuda.empty_cache()
    finally:
        L._lib.lib().lora_set_default_normalize(old)


if __name__ == "__main__":
    main()
