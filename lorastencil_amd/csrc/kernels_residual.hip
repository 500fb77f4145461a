// kernels_residual.hip -- one sweep's change, reduced in the sweep (lora_plan_residual; host side: reduce.cpp).
//
// d = sweep(in) - in over the interior of a region, as the lora_grid_diff record of a = sweep(in), b = in -- without ever
// storing the swept level: a launch reads the grid once and writes one record per workgroup.  `a` has the bits
// lora_plan_step_region would have stored.  The three fp64 families are wrappers: the tile walk -- window, tap order, centre
// value re-read from the window, predicates, barriers -- is tile_walk.h's, shared with kernels_cg.hip and kernels_theta.hip, and
// this file supplies what happens to a row's tap sums (ResidualRow: reduce_cells, with_source).  The bf16 kernel has a walk of
// its own, the 3D fp64 one on the (16 + 2) x 264 bf16 tile with four columns per lane: it RESTATES kernels_3d_bf16.hip's
// arithmetic (fp32, the separable T / U / out form where the plan has it, one round-to-nearest-even to bf16), and
// d = (double) a - (double) b has one rounding.
// Tiles, workgroups and the order of the walk: residual_tiles.h.  Workgroup g walks tiles g, g + G, ... and keeps ONE
// DiffAcc per lane across all of them.  A lane's cells of one row (2, bf16: 4) are reduced piece-first as in
// kernels_reduce.hip: one finite test of the piece's sum of squares, the exact cell-by-cell path only when it fails.  The
// index carried is the CELL's padded linear index, and every take uses DiffAcc's full rule (larger, or equal and lower
// index): a lane does not meet its cells in ascending order here.  Lanes, waves and the workgroup fold as there (xor
// butterfly, waves through LDS in wave order), the records by combine_kernel as KIND_CELL.  No atomics; records are
// written with plain vector stores.
//
// With a source (lora_plan_residual_src; template parameter SRC of the three fp64 families): a = fl(sweep(in) + f), f read at
// the reduced cells alone -- DESIGN 3.5c.  SRC = false is the code above, unchanged.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "reduce_device.h"
#include "residual_tiles.h"
#include "step_epilogue.h"
#include "tile_walk.h"

namespace lora {

namespace {

using namespace walk;

typedef unsigned short u16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

// N cells a lane holds of one row: a = the swept values, b = the centre values, the first `nvalid` (>= 1) of them inside the
// region; idx0 = padded linear index of cell 0.  Cells outside count as a = b = 0, which adds nothing to any result.
template <int N>
__device__ __forceinline__ void reduce_cells(DiffAcc &acc, const double (&a)[N], const double (&b)[N], int nvalid, long long idx0) {
    double d[N], s = 0.0, pm = 0.0, am = 0.0;
    long long nf = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool valid = j < nvalid;
        const double x = valid ? a[j] : 0.0;
        d[j] = x - (valid ? b[j] : 0.0);
        s = fma(d[j], d[j], s);
        pm = fmax(pm, fabs(d[j]));
        am = fmax(am, fabs(x));
    }
    if (!finite64(s)) {  // some difference is not finite (or a square overflowed): cell by cell
        s = am = 0.0;
        pm = -1.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool valid = j < nvalid;
            d[j] = a[j] - b[j];
            const bool ok = valid && finite64(d[j]);
            nf += (valid && !ok) ? 1 : 0;
            s += ok ? d[j] * d[j] : 0.0;
            am = (ok && fabs(a[j]) > am) ? fabs(a[j]) : am;  // d finite => a finite
            pm = (ok && fabs(d[j]) > pm) ? fabs(d[j]) : pm;
        }
    }
    int found = 0;  // the first cell inside the region whose difference is finite and as large
#pragma unroll
    for (int j = N - 1; j >= 0; --j) found = (j < nvalid && finite64(d[j]) && fabs(d[j]) == pm) ? j : found;
    acc.merge(pm, s, am, pm >= 0.0 ? idx0 + found : kNoIndex, nf);
}

// The value reduced as `a` when the call has a source: fl(acc + f), one rounding on top of the sweep's bits -- the update rule
// EPI_SOURCE of step_epilogue.h, which is what a plan that carries f as its source stores.  Without one, acc itself: "no
// source" is not "add a zero" (-0.0 + 0.0 changes bits), so SRC = false never reaches an addition.
template <bool SRC>
__device__ __forceinline__ double with_source(double acc, double f) {
    if constexpr (SRC) return step_epilogue<EPI_SOURCE>(acc, f, 0.0, 0.0, 0.0);
    return acc;
}

// What the residual does with a row's tap sums: nothing is stored, the cells go into the lane's one DiffAcc.
template <bool SRC>
struct ResidualRow {
    static constexpr bool kSrc = SRC;
    // (3D: eight more live registers through the tap loop, so SRC = true is bounded to three workgroups per CU, as the 3D source
    // step.  The launch is still cut by residual_tiles.h's 3D cap of 1024 workgroups (four per CU of 256): with SRC a quarter of
    // them waits for a slot when the region has that many tiles.)
    DiffAcc acc;
    __device__ __forceinline__ void row(double a0, double a1, d2 c, d2 f, int nvalid, long long idx0) {
        const double a[2] = {with_source<SRC>(a0, f.x), with_source<SRC>(a1, f.y)}, b[2] = {c.x, c.y};
        reduce_cells<2>(acc, a, b, nvalid, idx0);
    }
};

template <bool SRC>
__global__ __launch_bounds__(kThreads) void residual1d_kernel(const double *__restrict__ in, const double *__restrict__ f, const ResidualTiles rt,
                                                              const Taps9 W, ReduceRecord *__restrict__ partial) {
    ResidualRow<SRC> pol;
    pol.acc.init();
    tile_walk1d(in, f, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
}

template <int TAPSET, bool SRC>
__global__ __launch_bounds__(kThreads, 3) void residual2d_kernel(const double *__restrict__ in, const double *__restrict__ f,
                                                                 const ResidualTiles rt, const Taps49 W, ReduceRecord *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double tile[kWalk2dTile];
    ResidualRow<SRC> pol;
    pol.acc.init();
    tile_walk2d<TAPSET>(tile, in, f, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
}

template <int TAPSET, bool SRC>
__global__ __launch_bounds__(kThreads, SRC ? 3 : 4) void residual3d_kernel(const double *__restrict__ in, const double *__restrict__ f,
                                                                           const ResidualTiles rt, const Taps27 W,
                                                                           ReduceRecord *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double tile[2][kWalk3dTile];
    ResidualRow<SRC> pol;
    pol.acc.init();
    tile_walk3d<TAPSET>(tile, in, f, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
}

// ---- 3D bf16 (kernels_3d_bf16.hip: stencil3d_bf16_kernel at RY = 4, four columns per lane) -----------------------------
constexpr int kHTileW = 256;              // output columns per tile: 64 lanes x 4
constexpr int kHLdsW = kHTileW + 8;       // staged bf16 columns
constexpr int kHChunksPerRow = kHLdsW / 8;  // 16-byte pieces per staged row

struct Taps27f {
    float w[27];
};

__device__ __forceinline__ float bf16_lo(unsigned pair) { return __builtin_bit_cast(float, pair << 16); }
__device__ __forceinline__ float bf16_hi(unsigned pair) { return __builtin_bit_cast(float, pair & 0xffff0000u); }
__device__ __forceinline__ float win_elem(const unsigned *d, int e) { return (e & 1) ? bf16_hi(d[e >> 1]) : bf16_lo(d[e >> 1]); }
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {  // round-to-nearest-even, NaN stays NaN
    const u16 l = __builtin_bit_cast(u16, (__bf16) lo);
    const u16 h = __builtin_bit_cast(u16, (__bf16) hi);
    return (unsigned) l | ((unsigned) h << 16);
}
__device__ __forceinline__ float fmac_scalar(float w, float x, float acc) {  // acc + w * x as one v_fmac_f32
    asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc) : "s"(w), "v"(x));
    return acc;
}

// One staged row `j` of plane phase PHASE applied to the rotating output-plane accumulators of a lane: the arithmetic of
// kernels_3d_bf16.hip's accumulate_row, restated.  pr[k] = window elements (3+k, 4+k) as an fp32 pair.
template <int TAPSET, int RY, int NP, int PHASE>
__device__ __forceinline__ void accumulate_row(f2 (&acc)[3][RY][NP], f2 (&u)[RY][NP], const f2 *pr, int j, const Taps27f &W) {
    if constexpr (TAPSET == TAPS3D_SEP) {
        // W.w[0..2] = c (x), [3..5] = b (y), [6..8] = a (z): T = fma(c2,x+,fma(c1,x0,c0*x-)), U and out likewise over y and z
        f2 t[NP];
#pragma unroll
        for (int c = 0; c < NP; ++c) {
            t[c] = (f2){W.w[0], W.w[0]} * pr[2 * c];
            t[c].x = fmac_scalar(W.w[1], pr[2 * c].y, t[c].x);
            t[c].y = fmac_scalar(W.w[1], pr[2 * c + 2].x, t[c].y);
            t[c] = __builtin_elementwise_fma((f2){W.w[2], W.w[2]}, pr[2 * c + 2], t[c]);
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int r = j - dy;
            if (r >= 0 && r < RY) {
                const f2 b2 = (f2){W.w[3 + dy], W.w[3 + dy]};
#pragma unroll
                for (int c = 0; c < NP; ++c) u[r][c] = dy == 0 ? b2 * t[c] : __builtin_elementwise_fma(b2, t[c], u[r][c]);
            }
        }
        if (j >= 2) {
            const int r = j - 2;
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                const int s = (PHASE - dz + 3) % 3;
                const f2 a2 = (f2){W.w[6 + dz], W.w[6 + dz]};
#pragma unroll
                for (int c = 0; c < NP; ++c)
                    acc[s][r][c] = dz == 0 ? a2 * u[r][c] : __builtin_elementwise_fma(a2, u[r][c], acc[s][r][c]);
            }
        }
    } else {
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
                            const float wt = W.w[dz * 9 + dy * 3 + dx];
                            const f2 wt2 = (f2){wt, wt};
#pragma unroll
                            for (int c = 0; c < NP; ++c)
                                acc[s][r][c] = __builtin_elementwise_fma(wt2, pr[2 * c + dx], acc[s][r][c]);
                        }
                    }
                }
            }
        }
    }
}

template <int TAPSET>
__global__ __launch_bounds__(kThreads, 4) void residual3d_bf16_kernel(const u16 *__restrict__ in, const ResidualTiles rt, const Taps27f W,
                                                                      ReduceRecord *__restrict__ partial) {
    constexpr int RY = 4, CPL = 4;
    constexpr int TY = 4 * RY;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kHChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    constexpr int ND = (CPL + 8) / 2;
    __shared__ u32x4 tile[2][NCHUNK];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int h = rt.dims[0], m = rt.dims[1], n = rt.dims[2], ld = n + 8;
    const long plane = (long) (m + 4) * ld;
    DiffAcc dacc;
    dacc.init();
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o3[3], n3[3];
        residual_tile_box(rt, t, o3, n3);
        const int k0 = o3[0], zc = n3[0], i0 = o3[1], j0 = o3[2], row_end = o3[1] + n3[1];
        const int nplanes = zc + 2;

        long goff[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            const int r = k / kHChunksPerRow;
            const int c = k - r * kHChunksPerRow;
            const int gr = min(i0 + 1 + r, m + 3);  // padded rows i0+1 .. i0+TY+2
            const int gc = min(j0 + 8 * c, n);      // padded columns j0 .. in 8-element pieces
            goff[it] = (long) gr * ld + gc;
        }
        u32x4 stage[NIT];
        auto load_plane = [&](int p) {
            const u16 *src = in + (long) min(k0 + p, h + 1) * plane;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (NCHUNK % 256 == 0 || tid + it * 256 < NCHUNK) stage[it] = *reinterpret_cast<const u32x4 *>(src + goff[it]);
            }
        };
        auto write_plane = [&](int buf) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int k = tid + it * 256;
                if (NCHUNK % 256 == 0 || k < NCHUNK) tile[buf][k] = stage[it];
            }
        };

        f2 acc[3][RY][CPL / 2];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r = 0; r < RY; ++r)
#pragma unroll
                for (int c = 0; c < CPL / 2; ++c) acc[s][r][c] = (f2){0.0f, 0.0f};

        const int col = j0 + CPL * lane;
        const bool col_ok = col < n;  // (n is a multiple of 8: all four cells or none)
        const int strip_off = (wv * RY) * kHLdsW + CPL * lane;  // window: tile columns 4*lane .. 4*lane+11, own columns from +4
        const long cell0 = (long) (i0 + wv * RY + 2) * ld + (col + 4);

        load_plane(0);
        write_plane(0);
        __syncthreads();

        auto consume = [&](int p, auto phase_tag) {
            constexpr int PHASE = decltype(phase_tag)::value;
            const bool more = p + 1 < nplanes;
            if (more) load_plane(p + 1);
            const u16 *strip = reinterpret_cast<const u16 *>(&tile[p & 1][0]) + strip_off;
            f2 u[RY][CPL / 2];
#pragma unroll
            for (int j = 0; j < RY + 2; ++j) {
                unsigned d[ND];
#pragma unroll
                for (int q = 0; q < ND / 2; ++q) {
                    const u32x2 v = *reinterpret_cast<const u32x2 *>(strip + j * kHLdsW + 4 * q);
                    d[2 * q] = v.x;
                    d[2 * q + 1] = v.y;
                }
                f2 pr[CPL + 1];  // pr[k] = elements (3+k, 4+k)
#pragma unroll
                for (int k = 0; k < CPL + 1; ++k) pr[k] = (f2){win_elem(d, 3 + k), win_elem(d, 4 + k)};
                accumulate_row<TAPSET, RY, CPL / 2, PHASE>(acc, u, pr, j, W);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < RY; ++r)
#pragma unroll
                    for (int c = 0; c < CPL / 2; ++c) asm volatile("" : "+v"(acc[s][r][c]));

            {
                constexpr int s = (PHASE - 2 + 3) % 3;
                const int o = p - 2;
                if (o >= 0 && o < zc && col_ok) {
                    // centre plane o + 1 = p - 1 in the other buffer: tile row wv*RY + r + 1, this lane's four columns
                    const u16 *centre = reinterpret_cast<const u16 *>(&tile[(p - 1) & 1][0]) + strip_off + kHLdsW + 4;
                    const long base = (long) (k0 + o + 1) * plane + cell0;
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        if (i0 + wv * RY + r < row_end) {
                            // W.w[9]: 1 unless the plan follows the matrix-pipe variant's contract (as stencil3d_bf16_kernel)
                            const float sc = TAPSET == TAPS3D_SEP ? W.w[9] : 1.0f;
                            const unsigned x = pack_bf16(acc[s][r][0].x * sc, acc[s][r][0].y * sc);
                            const unsigned y = pack_bf16(acc[s][r][1].x * sc, acc[s][r][1].y * sc);
                            const u32x2 c = *reinterpret_cast<const u32x2 *>(centre + r * kHLdsW);
                            // bf16 -> fp64 is exact, so d = a - b has one rounding
                            const double a[4] = {(double) bf16_lo(x), (double) bf16_hi(x), (double) bf16_lo(y), (double) bf16_hi(y)};
                            const double b[4] = {(double) bf16_lo(c.x), (double) bf16_hi(c.x), (double) bf16_lo(c.y), (double) bf16_hi(c.y)};
                            reduce_cells<4>(dacc, a, b, 4, base + (long) r * ld);
                        }
                    }
                }
                if constexpr (TAPSET != TAPS3D_SEP) {  // the separable form assigns on its first z tap
#pragma unroll
                    for (int r = 0; r < RY; ++r)
#pragma unroll
                        for (int c = 0; c < CPL / 2; ++c) acc[s][r][c] = (f2){0.0f, 0.0f};
                }
            }
            if (p >= 2) __syncthreads();  // (as in residual3d_kernel: every wave is done with the centre plane's buffer)
            if (more) write_plane((p + 1) & 1);
            __syncthreads();
        };

        for (int p = 0; p < nplanes; p += 3) {
            consume(p, std::integral_constant<int, 0>{});
            if (p + 1 < nplanes) consume(p + 1, std::integral_constant<int, 1>{});
            if (p + 2 < nplanes) consume(p + 2, std::integral_constant<int, 2>{});
        }
    }
    finish<kThreads>(dacc, partial);
}

template <int TAPSET>
void launch_bf16(const Plan &p, const ResidualTiles &rt, const void *in, ReduceRecord *partial, hipStream_t s) {
    Taps27f w;
    for (int k = 0; k < 27; ++k) w.w[k] = (float) p.w[k];
    if (TAPSET == TAPS3D_SEP) {  // (as kernels_3d_bf16.hip's launch_bf16)
        for (int k = 0; k < 9; ++k) w.w[k] = p.sep[k];
        w.w[9] = 1.0f;
        if (p.variant == LORA_VARIANT_MFMA && p.mfma3_valid) {
            for (int k = 0; k < 9; ++k) w.w[k] = p.mfma3_abc[k];
            w.w[9] = p.mfma3_scale;
        }
    }
    hipLaunchKernelGGL((residual3d_bf16_kernel<TAPSET>), dim3((unsigned) rt.groups), dim3(kThreads), 0, s, static_cast<const u16 *>(in), rt, w,
                       partial);
}

}  // namespace

namespace {

template <bool SRC>
void launch_f64(const Plan &p, const ResidualTiles &rt, const double *din, const double *f, ReduceRecord *partial, hipStream_t s) {
    const dim3 grid((unsigned) rt.groups), block(kThreads);
    if (p.ndim == 1) {
        Taps9 w;
        for (int k = 0; k < 9; ++k) w.w[k] = p.w[k];
        hipLaunchKernelGGL(residual1d_kernel<SRC>, grid, block, 0, s, din, f, rt, w, partial);
    } else if (p.ndim == 2) {
        Taps49 w;
        for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
        if (p.tapset == TAPS2D_DIAMOND)
            hipLaunchKernelGGL((residual2d_kernel<TAPS2D_DIAMOND, SRC>), grid, block, 0, s, din, f, rt, w, partial);
        else if (p.tapset == TAPS2D_STAR)
            hipLaunchKernelGGL((residual2d_kernel<TAPS2D_STAR, SRC>), grid, block, 0, s, din, f, rt, w, partial);
        else
            hipLaunchKernelGGL((residual2d_kernel<TAPS2D_BOX, SRC>), grid, block, 0, s, din, f, rt, w, partial);
    } else {
        Taps27 w;
        for (int k = 0; k < 27; ++k) w.w[k] = p.w[k];
        if (p.tapset == TAPS3D_STAR)
            hipLaunchKernelGGL((residual3d_kernel<TAPS3D_STAR, SRC>), grid, block, 0, s, din, f, rt, w, partial);
        else
            hipLaunchKernelGGL((residual3d_kernel<TAPS3D_BOX, SRC>), grid, block, 0, s, din, f, rt, w, partial);
    }
}

}  // namespace

// f: the source of `a = sweep(in) + f` (fp64 plans only), nullptr = none -- the kernels without the operand
hipError_t launch_residual(const Plan &p, const ResidualTiles &rt, const void *in, const double *f, ReduceRecord *partial, hipStream_t s) {
    if (!has_fused_residual(p) || rt.groups < 1 || rt.groups > kReduceMaxGroups) return hipErrorInvalidValue;
    if (f && p.dtype == LORA_BF16) return hipErrorInvalidValue;
    const double *din = static_cast<const double *>(in);
    if (p.dtype == LORA_BF16) {
        if (p.tapset == TAPS3D_SEP)
            launch_bf16<TAPS3D_SEP>(p, rt, in, partial, s);
        else if (p.tapset == TAPS3D_STAR)
            launch_bf16<TAPS3D_STAR>(p, rt, in, partial, s);
        else
            launch_bf16<TAPS3D_BOX>(p, rt, in, partial, s);
    } else if (f) {
        launch_f64<true>(p, rt, din, f, partial, s);
    } else {
        launch_f64<false>(p, rt, din, nullptr, partial, s);
    }
    if (hipError_t e = hipGetLastError()) return e;
    return launch_reduce_fold_cells(rt.groups, partial, s);
}

}  // namespace lora
