// tile_walk.h -- the fp64 tile walk of the fused residual kernel, written once for the kernel families that sit on it:
// residual1d/2d/3d_kernel (kernels_residual.hip), apply_dot1d/2d/3d_kernel (kernels_cg.hip), theta1d/2d_kernel
// (kernels_theta.hip; theta3d_kernel restates the 3D walk in its own file, for the reason given there).  A walk RESTATES the per-point arithmetic of its family's single-sweep kernel (kernels_1d.hip,
// kernels_2d.hip, kernels_3d.hip: accumulator from 0, one fused multiply-add per tap of the plan's resolved tap set, in that
// family's tap order), so a finished tap sum has the bits lora_plan_step_region would have stored, at ONE fixed set of tile sizes:
//   1D   a lane owns two points: five aligned 16-byte loads, the odd tail point by scalar loads
//   2D   the (32 + 6) x 136 LDS window; when output row r completes its centre values are re-read from window row r + 3
//   3D   the double-buffered (16 + 2) x 136 plane tile; when output plane o = p - 2 completes its centre plane o + 1 is still
//        in the OTHER buffer, so the epilogue -- and a barrier behind it -- comes before that buffer is refilled
// Tiles, workgroups and their order: residual_tiles.h.  Workgroup g walks tiles g, g + G, ...
//
// What happens to a finished tap sum is the caller's: a walk takes a POLICY with
//   static constexpr bool kSrc         f is read: the lane's 16-byte piece at its own two cells (1D tail: 8 bytes), under the
//                                      predicate of the row it feeds, so no halo cell of f is ever loaded
//   void row(a0, a1, c, f, nvalid, idx0)
//                                      the lane's two tap sums of one row, the two centre values, the piece of f (zeros
//                                      without kSrc), how many of the two cells are inside the region (2; 1 for the odd 1D
//                                      tail point) and the padded linear index of cell 0
// and nothing else: windows, clamps, tap order, register pins, predicates and barriers are here.  One spelling is the register
// allocator's ("The tile-walk fold, checked"; guarded by tests/test_tile_walk_resources.py): the 2D walk takes tiles
// and taps by value, as a kernel holds them; by reference the kernel arguments are read through generic pointers for longer,
// and two more instantiations move by a register or two.
// Every name here is in lora::walk: other kernel files define kThreads, kTileW, ... of their own in their anonymous namespaces,
// and a file on these walks says `using namespace walk;` inside its own.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "residual_tiles.h"

namespace lora {
namespace walk {

constexpr int kThreads = 256;  // lanes of a workgroup of every kernel on these walks
constexpr int kTileW = 128;
constexpr int kLdsW = kTileW + 8;
constexpr int kChunksPerRow = kLdsW / 2;
constexpr int kWalk2dTile = (4 * 8 + 6) * kLdsW;  // doubles of LDS a 2D walk needs: RPT = 8 rows per lane, four waves, six halo rows
constexpr int kWalk3dTile = (4 * 4 + 2) * kLdsW;  // per buffer of a 3D walk (it needs two): RY = 4, two halo rows

// ---- 1D (kernels_1d.hip: stencil1d_kernel) ---------------------------------------------------------------------------------
template <typename POLICY>
__device__ __forceinline__ void tile_walk1d(const double *in, const double *f, const ResidualTiles &rt, const Taps9 &W, POLICY &pol) {
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o[3], n[3];
        residual_tile_box(rt, t, o, n);
        const int i = o[2] + 2 * (int) threadIdx.x;  // even: the region begins on an even point, tiles are 512 points
        const int left = o[2] + n[2] - i;
        if (left <= 0) continue;
        double win[10];
        d2 fv = {0.0, 0.0};
        if (left >= 2) {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const d2 v = *reinterpret_cast<const d2 *>(in + i + 2 * q);
                win[2 * q] = v.x;
                win[2 * q + 1] = v.y;
            }
            if constexpr (POLICY::kSrc) fv = *reinterpret_cast<const d2 *>(f + i + 4);
        } else {  // odd tail: one point, scalar loads stay inside the padded array
#pragma unroll
            for (int q = 0; q < 9; ++q) win[q] = in[i + q];
            win[9] = 0.0;
            if constexpr (POLICY::kSrc) fv.x = f[i + 4];
        }
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            a0 = fma(W.w[q], win[q], a0);
            a1 = fma(W.w[q], win[q + 1], a1);
        }
        pol.row(a0, a1, (d2){win[4], win[5]}, fv, left >= 2 ? 2 : 1, (long long) i + 4);
    }
}

// ---- 2D (kernels_2d.hip: stencil2d_direct_kernel at RPT = 8) ---------------------------------------------------------------
// tile: kWalk2dTile doubles of LDS, 16-byte aligned.  kSrc: a lane's piece of f of an output row is issued kAhead window rows
// before that row completes, so at most four pieces are in flight.
template <int TAPSET, typename POLICY>
__device__ __forceinline__ void tile_walk2d(double *tile, const double *in, const double *f, const ResidualTiles rt, const Taps49 W,
                                            POLICY &pol) {
    constexpr int RPT = 8;
    constexpr int TH = 4 * RPT;
    constexpr int LH = TH + 6;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    constexpr bool SRC = POLICY::kSrc;
    constexpr int kAhead = 4;  // window rows between the load of a row's piece of f and its use: 6 (and all eight up front) spill at three workgroups per CU
    static_assert(LH * kLdsW == kWalk2dTile, "the kernels' tile is the walk's");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int m = rt.dims[1], n = rt.dims[2], ld = n + 8;
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o[3], nn[3];
        residual_tile_box(rt, t, o, nn);
        const int i0 = o[1], j0 = o[2], row_end = o[1] + nn[1];
        const int col = j0 + 2 * lane;
        d2 fv[SRC ? RPT : 1] = {};
        // ---- stage the input window: padded rows i0+1 .. i0+TH+6, padded columns j0 .. j0+135 (clamped into the array)
        {
            d2 stage[NIT];
            const int max_row = m + 7;
            const int max_col = n + 6;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int k = tid + it * 256;
                if (NCHUNK % 256 == 0 || k < NCHUNK) {
                    const int r = k / kChunksPerRow;
                    const int c = k - r * kChunksPerRow;
                    const int gr = min(i0 + 1 + r, max_row);
                    const int gc = min(j0 + 2 * c, max_col);
                    stage[it] = *reinterpret_cast<const d2 *>(in + (size_t) gr * ld + gc);
                }
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int k = tid + it * 256;
                if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(tile + 2 * k) = stage[it];
            }
        }
        __syncthreads();

        // ---- compute: lane owns tile columns 2*lane+4, 2*lane+5 (window 2*lane .. 2*lane+9)
        double acc0[RPT], acc1[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
        }
        const double *strip = tile + (wv * RPT) * kLdsW + 2 * lane;
        d2 cur[5], nxt[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) cur[q] = *reinterpret_cast<const d2 *>(strip + 2 * q);
#pragma unroll
        for (int j = 0; j < RPT + 6; ++j) {
            if (j + 1 < RPT + 6) {
#pragma unroll
                for (int q = 0; q < 5; ++q) nxt[q] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kLdsW + 2 * q);
            }
            if constexpr (SRC) {  // the piece of f of output row j - 6 + kAhead, which completes kAhead window rows from here
                const int r = j - 6 + kAhead;
                if (r >= 0 && r < RPT) {
                    const int row = i0 + wv * RPT + r;
                    if (col < n && row < row_end) fv[r] = *reinterpret_cast<const d2 *>(f + (size_t) (row + 4) * ld + (col + 4));
                }
            }
            double win[10];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                win[2 * q] = cur[q].x;
                win[2 * q + 1] = cur[q].y;
            }
            // input row j of the strip is tap row dy = j - r of output row r
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const int dy = j - r;
                if (dy >= 0 && dy < 7) {
#pragma unroll
                    for (int dx = 0; dx < 7; ++dx) {
                        if (tap_on<TAPSET>(dy, dx)) {
                            const double wt = W.w[dy * 7 + dx];
                            acc0[r] = fma(wt, win[dx + 1], acc0[r]);
                            acc1[r] = fma(wt, win[dx + 2], acc1[r]);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                if (j - r >= 0 && j - r < 7) asm volatile("" : "+v"(acc0[r]), "+v"(acc1[r]));
            }
            // output row j-6 is complete: its centre values are window row r + 3, this lane's columns
            if (j >= 6) {
                const int r = j - 6;
                const int row = i0 + wv * RPT + r;
                if (col < n && row < row_end) {  // (n and col are even: both cells or none)
                    const d2 c = *reinterpret_cast<const d2 *>(strip + (r + 3) * kLdsW + 4);
                    pol.row(acc0[r], acc1[r], c, fv[SRC ? r : 0], 2, (long long) (row + 4) * ld + (col + 4));
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) cur[q] = nxt[q];
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave is done with the window before the next tile's is staged
    }
}

// ---- 3D (kernels_3d.hip: stencil3d_stream_kernel at RY = 4) ----------------------------------------------------------------
// tile: two buffers of kWalk3dTile doubles of LDS, 16-byte aligned.  kSrc: the four 16-byte pieces of f of output plane
// o = p - 2 (one per row of the lane, at its two own cells) are issued at the head of consume(p), beside the next plane's loads,
// and used in its epilogue; predicated as the rows they feed.  Eight more live registers through the tap loop (residual3d_kernel
// with SRC is bounded to three workgroups per CU).
template <int TAPSET, typename POLICY>
__device__ __forceinline__ void tile_walk3d(double (*tile)[kWalk3dTile], const double *in, const double *f, const ResidualTiles &rt,
                                            const Taps27 &W, POLICY &pol) {
    constexpr int RY = 4;
    constexpr int TY = 4 * RY;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    constexpr bool SRC = POLICY::kSrc;
    static_assert(LH * kLdsW == kWalk3dTile, "the kernels' tile is the walk's");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int h = rt.dims[0], m = rt.dims[1], n = rt.dims[2], ld = n + 8;
    const long plane = (long) (m + 4) * ld;
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o3[3], n3[3];
        residual_tile_box(rt, t, o3, n3);
        const int k0 = o3[0], zc = n3[0], i0 = o3[1], j0 = o3[2], row_end = o3[1] + n3[1];
        const int nplanes = zc + 2;  // input planes: padded k0 .. k0+zc+1

        long goff[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            const int r = k / kChunksPerRow;
            const int c = k - r * kChunksPerRow;
            const int gr = min(i0 + 1 + r, m + 3);  // padded rows i0+1 .. i0+TY+2
            const int gc = min(j0 + 2 * c, n + 6);
            goff[it] = (long) gr * ld + gc;
        }
        d2 stage[NIT];
        auto load_plane = [&](int p) {
            const double *src = in + (long) min(k0 + p, h + 1) * plane;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (NCHUNK % 256 == 0 || tid + it * 256 < NCHUNK) stage[it] = *reinterpret_cast<const d2 *>(src + goff[it]);
            }
        };
        auto write_plane = [&](int buf) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int k = tid + it * 256;
                if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(&tile[buf][2 * k]) = stage[it];
            }
        };

        double acc0[3][RY], acc1[3][RY];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                acc0[s][r] = 0.0;
                acc1[s][r] = 0.0;
            }

        const int col = j0 + 2 * lane;
        const bool col_ok = col < n;
        const int strip_off = (wv * RY) * kLdsW + 2 * lane + 2;  // window = tile cols 2*lane+2 .. 2*lane+7
        const long cell0 = (long) (i0 + wv * RY + 2) * ld + (col + 4);  // this lane's first cell inside a plane

        load_plane(0);
        write_plane(0);
        __syncthreads();

        auto consume = [&](int p, auto phase_tag) {
            constexpr int PHASE = decltype(phase_tag)::value;
            const bool more = p + 1 < nplanes;
            if (more) load_plane(p + 1);
            d2 fv[SRC ? RY : 1] = {};
            if constexpr (SRC) {
                if (p >= 2 && p - 2 < zc && col_ok) {
                    const double *fp = f + (long) (k0 + p - 1) * plane + cell0;  // (p >= 2: a plane inside d_f)
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        if (i0 + wv * RY + r < row_end) fv[r] = *reinterpret_cast<const d2 *>(fp + (long) r * ld);
                    }
                }
            }
            const double *strip = &tile[p & 1][strip_off];
#pragma unroll
            for (int j = 0; j < RY + 2; ++j) {
                double win[6];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const d2 v = *reinterpret_cast<const d2 *>(strip + j * kLdsW + 2 * q);
                    win[2 * q] = v.x;
                    win[2 * q + 1] = v.y;
                }
#pragma unroll
                for (int dz = 0; dz < 3; ++dz) {
                    const int s = (PHASE - dz + 3) % 3;
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        const int dy = j - r;
                        if (dy >= 0 && dy < 3) {
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) {
                                if (tap_on3<TAPSET>(dz, dy, dx)) {
                                    const double wt = W.w[dz * 9 + dy * 3 + dx];
                                    acc0[s][r] = fma(wt, win[dx + 1], acc0[s][r]);
                                    acc1[s][r] = fma(wt, win[dx + 2], acc1[s][r]);
                                }
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < RY; ++r) asm volatile("" : "+v"(acc0[s][r]), "+v"(acc1[s][r]));

            // output plane o = p - 2 is complete; its centre plane o + 1 = p - 1 is the other buffer's
            {
                constexpr int s = (PHASE - 2 + 3) % 3;
                const int o = p - 2;
                if (o >= 0 && o < zc && col_ok) {
                    const double *centre = &tile[(p - 1) & 1][strip_off + kLdsW + 2];  // tile row wv*RY + r + 1, cols 2*lane+4, +5
                    const long base = (long) (k0 + o + 1) * plane + cell0;
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        if (i0 + wv * RY + r < row_end) {
                            const d2 c = *reinterpret_cast<const d2 *>(centre + r * kLdsW);
                            pol.row(acc0[s][r], acc1[s][r], c, fv[SRC ? r : 0], 2, base + (long) r * ld);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    acc0[s][r] = 0.0;
                    acc1[s][r] = 0.0;
                }
            }
            // the refill goes into the buffer of plane p - 1, which other waves' epilogues may still be reading: one more
            // barrier per plane than the sweep kernel, which never looks at that buffer again
            if (p >= 2) __syncthreads();
            if (more) write_plane((p + 1) & 1);
            __syncthreads();
        };

        for (int p = 0; p < nplanes; p += 3) {
            consume(p, std::integral_constant<int, 0>{});
            if (p + 1 < nplanes) consume(p + 1, std::integral_constant<int, 1>{});
            if (p + 2 < nplanes) consume(p + 2, std::integral_constant<int, 2>{});
        }
    }
}

}  // namespace walk
}  // namespace lora
