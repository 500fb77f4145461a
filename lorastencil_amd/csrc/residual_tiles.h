// residual_tiles.h -- how a launch of the fused residual kernels (kernels_residual.hip) and of the other kernels on tile_walk.h's
// walks (kernels_cg.hip, kernels_theta.hip) is cut: tile -> workgroup -> cells.
//
// The interior range [begin, end) of the outermost dimension (times the whole inner dimensions) is cut into TILES of fixed
// extents per kernel family -- the tiles of the single-sweep kernels they mirror, at one fixed set of sizes:
//   1D        512 points            (256 lanes x 2)
//   2D fp64   32 rows x 128 columns (stencil2d_direct_kernel at 8 rows per lane)
//   3D fp64   32 planes x 16 rows x 128 columns (stencil3d_stream_kernel at 4 rows per lane)
//   3D bf16   32 planes x 16 rows x 256 columns (stencil3d_bf16_kernel at 4 columns per lane)
// Tiles are numbered innermost direction first; G = min(tiles, the family's cap) workgroups run, and workgroup g reduces
// tiles g, g + G, g + 2 G, ... in that order into ONE record.  Nothing here looks at a tuning option or at the device, so
// the order in which every cell enters the sums is a function of dtype, extents and region alone.  The cap is the number
// of workgroups resident at once on 256 CUs (2D: three per CU by its 41 KB of LDS, else four), never above kReduceMaxGroups.
// One launch does not fit its cap: the 3D fp64 kernels with a source operand (lora_plan_residual_src) are bounded to three
// workgroups per CU by their registers, so of 1024 workgroups 768 are resident and the rest follow as slots free up.  The cap
// stays 1024 there too: the tiles a workgroup walks, and so the order of every sum, do not depend on whether f is given.
//
// The decode is plain integer arithmetic: the kernels run it, and lora_debug_residual_cover replays it on the host.
#pragma once

#include "engine.h"

namespace lora {

struct ResidualTiles {
    int ndim, bf16;
    int dims[3];   // interior extents as planes, rows, columns (leading ones for 1D / 2D)
    int lo[3];     // first interior index of the region per direction (only the outermost real one can be non-zero) ...
    int hi[3];     // ... and one past its last
    int ext[3];    // tile extents
    int cnt[3];    // tiles per direction
    long tiles;
    int groups;
};

#ifdef __HIPCC__
#define LORA_RES_FN __host__ __device__ __forceinline__
#else
#define LORA_RES_FN inline
#endif

// Host: false for an empty region.
inline bool residual_tiles_setup(ResidualTiles &rt, const Plan &p, int begin, int end) {
    rt.ndim = p.ndim;
    rt.bf16 = p.dtype == LORA_BF16;
    const int shift = 3 - p.ndim;
    for (int d = 0; d < 3; ++d) {
        rt.dims[d] = d < shift ? 1 : p.dims[d - shift];
        rt.lo[d] = 0;
        rt.hi[d] = rt.dims[d];
        rt.ext[d] = 1;
    }
    rt.lo[shift] = begin;
    rt.hi[shift] = end;
    if (end <= begin) return false;
    int cap = kReduceMaxGroups;
    if (p.ndim == 1) {
        rt.ext[2] = 512;
    } else if (p.ndim == 2) {
        rt.ext[1] = 32;
        rt.ext[2] = 128;
        cap = 768;
    } else {
        rt.ext[0] = 32;
        rt.ext[1] = 16;
        rt.ext[2] = rt.bf16 ? 256 : 128;
    }
    rt.tiles = 1;
    for (int d = 0; d < 3; ++d) {
        rt.cnt[d] = (rt.hi[d] - rt.lo[d] + rt.ext[d] - 1) / rt.ext[d];
        rt.tiles *= rt.cnt[d];
    }
    rt.groups = (int) (rt.tiles < cap ? rt.tiles : cap);
    return true;
}

// tile t -> its first interior index per direction (o[]) and how many cells it holds per direction (n[]: the tile's extent,
// less at the region's far edges)
LORA_RES_FN void residual_tile_box(const ResidualTiles &rt, long t, int *o, int *n) {
    const long row = t / rt.cnt[2];
    const int c2 = (int) (t - row * rt.cnt[2]);
    const int c0 = (int) (row / rt.cnt[1]);
    const int c1 = (int) (row - (long) c0 * rt.cnt[1]);
    const int c[3] = {c0, c1, c2};
    for (int d = 0; d < 3; ++d) {
        o[d] = rt.lo[d] + c[d] * rt.ext[d];
        const int left = rt.hi[d] - o[d];
        n[d] = left < rt.ext[d] ? left : rt.ext[d];
    }
}

}  // namespace lora
