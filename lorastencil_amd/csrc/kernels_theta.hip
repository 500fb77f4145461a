// kernels_theta.hip -- the two stencil launches of the implicit time stepper (host side: cg.cpp) and the fused
// defect launch of the V-cycle (mg.cpp), siblings of apply_dot in kernels_cg.hip.  The 1D and 2D
// kernels are wrappers round tile_walk.h's walk, as apply_dot and the residual kernels are (window, tile sizes, tap order, centre
// value re-read from the window; residual_tiles.h for the tiles); theta3d_kernel RESTATES tile_walk3d in a body of its own (the
// reason stands above it).  Either way `acc` has the bits lora_plan_step_region stores; template parameter MODE picks
// what happens with a row's finished tap sums (ThetaRow):
//
//   TH_SHIFT      q = fl(fl(sigma c) - fl(tau acc)), c the centre value: the operator sigma I - tau S applied to p, stored at
//                 the lane's own two cells, and the record of dot(p, q)                               (lora_plan_apply_dot_shift)
//   TH_START      r = fl(tau fl(acc - c)), stored to BOTH o0 and o1 (the stepper's r and p), and the record of dot(r, r)
//   TH_START_SRC  r = fl(tau fl(fl(acc + f) - c)): f is read at the stored cells alone, with the store's own addressing -- as
//                 the SRC form of kernels_residual.hip reads it -- so no halo cell of f is ever loaded.  "No source" is its
//                 own instantiation, not "add a zero".                                                  (lora_plan_theta_start)
//   TH_DEFECT     d = fl(acc - c), stored to o0 alone: the start without the scale, the second store and the dot
//   TH_DEFECT_SRC d = fl(fl(acc + f) - c), f read as TH_START_SRC reads it.  Neither writes a record, so nothing folds behind
//                 them: one launch where a source sweep and a subtraction stood, at every level of the V-cycle of mg.cpp.
//                                                                                                        (lora_plan_defect)
// Stores are 16 bytes at the lane's own two cells, 8 bytes for the odd tail point in 1D: interior cells only, so the halos of
// the stored grids are neither read nor written.  Every operation behind the tap sum is its own fp64 rounding (#pragma clang
// fp contract(off)).  No atomics; records are written with plain vector stores, one per workgroup, folded by cg_fold_kernel.
//
// The state.  In the stepper every launch gets the CgState: its `breakdown` word carries two bits, CG_HALT_BREAKDOWN (sticky
// for the run) and CG_HALT_DONE (the step met its stop rule; cleared behind the next start's fold).  A TH_SHIFT launch that
// finds either returns before it loads or stores anything -- the uniform early exit of kernels_cg.hip; a start launch ignores
// `done`, which belongs to the step before it.  The public entries pass no state.
//
// kernels_cg.hip's apply_dot kernels are left as they are: these are separate instantiations in a separate translation unit.
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

enum { TH_SHIFT = 0, TH_START = 1, TH_START_SRC = 2, TH_DEFECT = 3, TH_DEFECT_SRC = 4 };

constexpr bool mode_src(int mode) { return mode == TH_START_SRC || mode == TH_DEFECT_SRC; }  // f is read
constexpr bool mode_two(int mode) { return mode == TH_START || mode == TH_START_SRC; }       // o1 is stored too
constexpr bool mode_dot(int mode) { return mode < TH_DEFECT; }                               // a record is written

struct ThetaCoef {
    double sigma, tau;
};

template <int MODE>
__device__ __forceinline__ bool halted(const CgState *st) {
    if (!st) return false;
    return MODE == TH_SHIFT ? st->breakdown != 0 : (st->breakdown & CG_HALT_BREAKDOWN) != 0;
}

// One cell: a = the swept value, c = the centre value, f = the source's (the SRC modes alone).  Returns the stored value; x, y
// are the factors of the cell's product in the record.
template <int MODE>
__device__ __forceinline__ double theta_cell(double a, double c, double f, const ThetaCoef k, double &x, double &y) {
#pragma clang fp contract(off)
    if constexpr (MODE == TH_SHIFT) {
        const double t = k.sigma * c;
        const double u = k.tau * a;
        const double q = t - u;
        x = c;
        y = q;
        return q;
    } else {
        double t = a;
        if constexpr (mode_src(MODE)) t = step_epilogue<EPI_SOURCE>(a, f, 0.0, 0.0, 0.0);
        const double d = t - c;
        if constexpr (!mode_dot(MODE)) {
            x = d;
            y = d;
            return d;
        } else {
            const double r = k.tau * d;
            x = r;
            y = r;
            return r;
        }
    }
}

// N cells a lane holds of one row, the first `nvalid` (>= 1) of them inside the region: v = what the caller stores at the valid
// cells; their products go into `acc`.
template <int MODE, int N>
__device__ __forceinline__ void theta_cells(DotAcc &acc, const double (&a)[N], const double (&c)[N], const double (&f)[N], const ThetaCoef k,
                                            int nvalid, double (&v)[N]) {
    double x[N], y[N];
    bool valid[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        valid[j] = j < nvalid;
        double xj, yj;
        v[j] = theta_cell<MODE>(a[j], c[j], f[j], k, xj, yj);
        x[j] = valid[j] ? xj : 0.0;
        y[j] = valid[j] ? yj : 0.0;
    }
    if constexpr (mode_dot(MODE)) acc.cells<N>(x, y, valid);
}

// What a mode does with a row's tap sums: the stored value at the row's cells inside the region, 16 bytes, or 8 for the odd 1D
// tail point, to o0 and, in the start modes, o1.
template <int MODE>
struct ThetaRow {
    static constexpr bool kSrc = mode_src(MODE);
    double *__restrict__ o0, *__restrict__ o1;
    ThetaCoef k;
    DotAcc acc;
    __device__ __forceinline__ void row(double a0, double a1, d2 c, d2 f, int nvalid, long long idx0) {
        const double a[2] = {a0, a1}, b[2] = {c.x, c.y}, ff[2] = {f.x, f.y};
        double v[2];
        theta_cells<MODE, 2>(acc, a, b, ff, k, nvalid, v);
        if (nvalid >= 2) {
            *reinterpret_cast<d2 *>(o0 + idx0) = (d2){v[0], v[1]};
            if constexpr (mode_two(MODE)) *reinterpret_cast<d2 *>(o1 + idx0) = (d2){v[0], v[1]};
        } else {
            o0[idx0] = v[0];
            if constexpr (mode_two(MODE)) o1[idx0] = v[0];
        }
    }
};

// (the defect modes write no record: no finish(), and its 192 bytes of LDS are not theirs)
template <int MODE>
__global__ __launch_bounds__(kThreads) void theta1d_kernel(const double *__restrict__ in, const double *__restrict__ f, double *__restrict__ o0,
                                                           double *__restrict__ o1, const ThetaCoef k, const CgState *st, const ResidualTiles rt,
                                                           const Taps9 W, ReduceRecord *__restrict__ partial) {
    if (halted<MODE>(st)) return;
    ThetaRow<MODE> pol{o0, o1, k};
    pol.acc.init();
    tile_walk1d(in, f, rt, W, pol);
    if constexpr (mode_dot(MODE)) finish<kThreads>(pol.acc, partial);
}

template <int TAPSET, int MODE>
__global__ __launch_bounds__(kThreads, 3) void theta2d_kernel(const double *__restrict__ in, const double *__restrict__ f, double *__restrict__ o0,
                                                              double *__restrict__ o1, const ThetaCoef kc, const CgState *st,
                                                              const ResidualTiles rt, const Taps49 W, ReduceRecord *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double tile[kWalk2dTile];
    if (halted<MODE>(st)) return;
    ThetaRow<MODE> pol{o0, o1, kc};
    pol.acc.init();
    tile_walk2d<TAPSET>(tile, in, f, rt, W, pol);
    if constexpr (mode_dot(MODE)) finish<kThreads>(pol.acc, partial);
}

// ---- 3D: NOT on tile_walk.h.  This is tile_walk3d's walk RESTATED (geometry, staging, tap order, pins, barriers), with the pieces
// of f loaded in the epilogue, behind the tap loop, so that they are not live through it: the stores' addresses already are.  On
// the shared walk the box's DEFECT kernel kept its registers and waves but reloaded 58 more SGPRs from VGPR lanes and
// lora_plan_defect lost 2 -- 4 % on box3d1r 256^3 ("The tile-walk fold, checked"); no spelling of the walk's
// parameters gave the allocation back, so the body stays here until one does.  A fix to tile_walk3d belongs here too.
template <int TAPSET, int MODE>
__global__ __launch_bounds__(kThreads, 3) void theta3d_kernel(const double *__restrict__ in, const double *__restrict__ f, double *__restrict__ o0,
                                                              double *__restrict__ o1, const ThetaCoef kc, const CgState *st,
                                                              const ResidualTiles rt, const Taps27 W, ReduceRecord *__restrict__ partial) {
    constexpr int RY = 4;
    constexpr int TY = 4 * RY;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    constexpr bool SRC = mode_src(MODE);
    __shared__ __attribute__((aligned(16))) double tile[2][LH * kLdsW];
    if (halted<MODE>(st)) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int h = rt.dims[0], m = rt.dims[1], n = rt.dims[2], ld = n + 8;
    const long plane = (long) (m + 4) * ld;
    DotAcc dacc;
    dacc.init();
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

            // output plane o = p - 2 is complete; its centre plane o + 1 = p - 1 is the other buffer's.  The pieces of f are
            // loaded here, behind the tap loop, so that they are not live through it: the stores' addresses already are.
            {
                constexpr int s = (PHASE - 2 + 3) % 3;
                const int o = p - 2;
                if (o >= 0 && o < zc && col_ok) {
                    const double *centre = &tile[(p - 1) & 1][strip_off + kLdsW + 2];  // tile row wv*RY + r + 1, cols 2*lane+4, +5
                    const long base = (long) (k0 + o + 1) * plane + cell0;
                    d2 fv[SRC ? RY : 1] = {};
                    if constexpr (SRC) {
#pragma unroll
                        for (int r = 0; r < RY; ++r) {
                            if (i0 + wv * RY + r < row_end) fv[r] = *reinterpret_cast<const d2 *>(f + base + (long) r * ld);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        if (i0 + wv * RY + r < row_end) {
                            const d2 c = *reinterpret_cast<const d2 *>(centre + r * kLdsW);
                            const d2 fr = fv[SRC ? r : 0];
                            const double a[2] = {acc0[s][r], acc1[s][r]}, b[2] = {c.x, c.y}, ff[2] = {fr.x, fr.y};
                            double v[2];
                            theta_cells<MODE, 2>(dacc, a, b, ff, kc, 2, v);
                            *reinterpret_cast<d2 *>(o0 + base + (long) r * ld) = (d2){v[0], v[1]};
                            if constexpr (mode_two(MODE)) *reinterpret_cast<d2 *>(o1 + base + (long) r * ld) = (d2){v[0], v[1]};
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    acc0[s][r] = 0.0;
                    acc1[s][r] = 0.0;
                }
            }
            // (as tile_walk3d: the refill goes into the buffer of plane p - 1, which other waves' epilogues may still read)
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
    if constexpr (mode_dot(MODE)) finish<kThreads>(dacc, partial);
}

template <int MODE>
void launch_mode(const Plan &p, const ResidualTiles &rt, const double *in, const double *f, double *o0, double *o1, const ThetaCoef k,
                 const CgState *st, ReduceRecord *partial, hipStream_t s) {
    const dim3 grid((unsigned) rt.groups), block(kThreads);
    if (p.ndim == 1) {
        Taps9 w;
        for (int t = 0; t < 9; ++t) w.w[t] = p.w[t];
        hipLaunchKernelGGL(theta1d_kernel<MODE>, grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
    } else if (p.ndim == 2) {
        Taps49 w;
        for (int t = 0; t < 49; ++t) w.w[t] = p.w[t];
        if (p.tapset == TAPS2D_DIAMOND)
            hipLaunchKernelGGL((theta2d_kernel<TAPS2D_DIAMOND, MODE>), grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
        else if (p.tapset == TAPS2D_STAR)
            hipLaunchKernelGGL((theta2d_kernel<TAPS2D_STAR, MODE>), grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
        else
            hipLaunchKernelGGL((theta2d_kernel<TAPS2D_BOX, MODE>), grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
    } else {
        Taps27 w;
        for (int t = 0; t < 27; ++t) w.w[t] = p.w[t];
        if (p.tapset == TAPS3D_STAR)
            hipLaunchKernelGGL((theta3d_kernel<TAPS3D_STAR, MODE>), grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
        else
            hipLaunchKernelGGL((theta3d_kernel<TAPS3D_BOX, MODE>), grid, block, 0, s, in, f, o0, o1, k, st, rt, w, partial);
    }
}

}  // namespace

hipError_t launch_apply_dot_shift(const Plan &p, const ResidualTiles &rt, const double *d_p, double *d_q, double sigma, double tau,
                                  const CgState *st, ReduceRecord *partial, hipStream_t s) {
    if (!has_cg(p) || rt.groups < 1 || rt.groups > kReduceMaxGroups) return hipErrorInvalidValue;
    launch_mode<TH_SHIFT>(p, rt, d_p, nullptr, d_q, nullptr, ThetaCoef{sigma, tau}, st, partial, s);
    return hipGetLastError();
}

hipError_t launch_theta_start(const Plan &p, const ResidualTiles &rt, const double *d_u, const double *d_f, double tau, double *d_r,
                              double *d_p, const CgState *st, ReduceRecord *partial, hipStream_t s) {
    if (!has_cg(p) || rt.groups < 1 || rt.groups > kReduceMaxGroups) return hipErrorInvalidValue;
    if (d_f)
        launch_mode<TH_START_SRC>(p, rt, d_u, d_f, d_r, d_p, ThetaCoef{1.0, tau}, st, partial, s);
    else
        launch_mode<TH_START>(p, rt, d_u, nullptr, d_r, d_p, ThetaCoef{1.0, tau}, st, partial, s);
    return hipGetLastError();
}

hipError_t launch_defect(const Plan &p, const ResidualTiles &rt, const double *d_u, const double *d_f, double *d_out, hipStream_t s) {
    if (!has_cg(p) || rt.groups < 1 || rt.groups > kReduceMaxGroups) return hipErrorInvalidValue;
    if (d_f)
        launch_mode<TH_DEFECT_SRC>(p, rt, d_u, d_f, d_out, nullptr, ThetaCoef{1.0, 1.0}, nullptr, nullptr, s);
    else
        launch_mode<TH_DEFECT>(p, rt, d_u, nullptr, d_out, nullptr, ThetaCoef{1.0, 1.0}, nullptr, nullptr, s);
    return hipGetLastError();
}

}  // namespace lora
