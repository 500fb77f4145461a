#!/usr/bin/env python3
"""The bits of every entry on the shared fp64 tile walk (csrc/tile_walk.h), for a line-by-line comparison of
two builds:
   python tools/tile_walk_bits.py --out profiles/tile_walk_bits_new.jsonl [--small]
   LORA_PACKAGE_ROOT=<a build of another commit> python tools/tile_walk_bits.py --out profiles/tile_walk_bits_parent.jsonl

One process.  Entries: lora_plan_residual, _residual_src, _apply_dot, _apply_dot_shift(9, 8), _theta_start(tau = 8) with and without
f, _defect with and without f.  Grids: the edges of the walk (the odd 1D tail and a region that does not begin at 0; 2D one row
and one column pair in second tiles, a region inside tiles, all three tap sets; 3D regions of 1, 2 and 3 planes, both tap sets)
and two grids on which a workgroup walks more than one tile (2D 1024 x 4096: 1024 tiles on 768 workgroups; 3D 33 x 1040 x 1024:
1040 tiles on 1024).  Per call: inputs from a fixed seed, every output grid filled with one NaN pattern, one call, then one JSON
line with the SHA-256 of each output grid (whole padded array: a cell the call must not write keeps the pattern) and the
returned record.  Nothing here depends on the build, so two builds that compute the same bits write the same file.
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("LORA_PACKAGE_ROOT", ROOT))
import lorastencil_amd as L  # noqa: E402

EDGES = [("1d2r", (1027,), [(0, 0), (510, 1027)])]
EDGES += [(s, d, r) for s in ("star2d1r", "star2d3r", "box2d3r") for d, r in (((33, 130), [(0, 0)]), ((70, 258), [(5, 37)]))]
EDGES += [(s, (34, 18, 130), [(0, 0), (3, 4), (3, 5), (3, 6)]) for s in ("star3d1r", "box3d1r")]
SEVERAL_TILES = [("star2d1r", (1024, 4096), [(0, 0)]), ("box3d1r", (33, 1040, 1024), [(0, 0)])]
SMALL_TILES = [("star2d1r", (64, 256), [(0, 0)]), ("box3d1r", (33, 32, 128), [(0, 0)])]
POISON = 0x7ff8dead0000beef  # a quiet NaN no arithmetic produces


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def record(r):
    return None if r is None else [v.hex() if isinstance(v, float) else v for v in r]


def cases(shape, dims, regions):
    rng = np.random.default_rng(zlib.crc32(repr(("tile_walk_bits", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    u = torch.from_numpy(rng.standard_normal(ps) * 3.0).cuda()
    f = torch.from_numpy(rng.standard_normal(ps) * 3.0).cuda()
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    plan = L.Plan(shape, dims).set_weights(w / w.sum())
    assert plan.get_option("fused_residual") == 1 and plan.get_option("cg") == 1
    out = [torch.empty_like(u), torch.empty_like(u)]
    entries = [("residual", 0, lambda o, b, e: plan.residual(u, b, e)),
               ("residual_src", 0, lambda o, b, e: plan.residual_src(u, f, b, e)),
               ("apply_dot", 1, lambda o, b, e: plan.apply_dot(u, o[0], b, e)),
               ("apply_dot_shift", 1, lambda o, b, e: plan.apply_dot_shift(u, o[0], 9.0, 8.0, b, e)),
               ("theta_start_f", 2, lambda o, b, e: plan.theta_start(u, f, 8.0, o[0], o[1], b, e)),
               ("theta_start", 2, lambda o, b, e: plan.theta_start(u, None, 8.0, o[0], o[1], b, e)),
               ("defect_f", 1, lambda o, b, e: plan.defect(u, f, o[0], b, e)),
               ("defect", 1, lambda o, b, e: plan.defect(u, None, o[0], b, e))]
    for begin, end in regions:
        for name, n_out, call in entries:
            for o in out[:n_out]:
                o.view(torch.int64).fill_(POISON)
            got = call(out, begin, end)
            yield {"entry": name, "shape": shape, "dims": list(dims), "region": [begin, end], "grids": [sha(o) for o in out[:n_out]],
                   "record": record(got)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--small", action="store_true", help="a quick rehearsal: small grids in place of the two big ones")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for shape, dims, regions in EDGES + (SMALL_TILES if args.small else SEVERAL_TILES):
            for row in cases(shape, dims, regions):
                fh.write(json.dumps(row) + "\n")
                fh.flush()
            print(shape, dims, "done", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
