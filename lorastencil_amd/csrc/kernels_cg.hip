// kernels_cg.hip -- the hot path of the conjugate-gradient solver for u = S(u) + f (host side: cg.cpp).  The operator
// is A = I - S, S the plan's raw single sweep; fp64 plans with the fused residual kernel only.
//
//   apply_dot     q = fl(p - acc) on every interior cell of the range and, in the same launch, the record of dot(p, q).  `acc`
//                 has the bits lora_plan_step_region stores for p: each kernel here RESTATES the body of its family in
//                 kernels_residual.hip (window, tile sizes, tap order, centre value re-read from the window -- see that file and
//                 residual_tiles.h for the walk).  That kernel has a = acc and b = centre and reduces b - a; this one STORES
//                 b - a (a separate rounding, 16-byte stores at the lane's own two cells, 8 bytes for the odd tail point in 1D:
//                 interior cells only) and accumulates b * (b - a).  p is read once, q written once, one record per workgroup.
//   cg_update     x = fl(x + fl(alpha p)), r = fl(r - fl(alpha q)) and the record of dot(r, r) (its amax: max |r|)
//   cg_direction  p = fl(r + fl(beta p))
//   cg_start      r = fl(r - x), p = r: the first residual from the source sweep the driver put into r
//                 The three walk the interior like the reductions (reduce.cpp: reduce_geometry; 16-byte pieces, a piece with one
//                 interior cell -- the odd tail of a 1D array -- by 8-byte loads and stores), so no halo cell is loaded or stored.
//   cg_fold       one wave folds the workgroups' records in the order of kernels_reduce.hip's fold (lane l takes records l,
//                 l + 64, ..., then the butterfly) into record kReduceMaxGroups; in the driver its last act is the one-lane
//                 update of the device-resident scalars (CgState: alpha = rr / pq, beta = rr' / rr in IEEE fp64 division).
//                 The implicit stepper (cg.cpp, kernels_theta.hip) adds three phases: the reset at the head of
//                 a run, the step start (rr = rr0, thresh = fl(rtol2 rr0)) and the update with the step's stop rule.
//                 The preconditioned drivers (mg.cpp) add phases for rz = r.z (engine.h: CgFold, PcgState).
// Every arithmetic operation outside a tap sum is its own rounding (#pragma clang fp contract(off), as step_epilogue.h).  No
// atomics; records and scalars are written with plain vector stores.
//
// Breakdown.  In the driver every launch gets the state: one that finds its sticky `breakdown` flag set returns before it loads
// or stores anything (a uniform early exit), so x stays the last good iterate.  The public entries pass no state.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "reduce_device.h"
#include "residual_tiles.h"

namespace lora {

namespace {

constexpr int kThreads = 256;

// N cells a lane holds of one row: a = the swept values, b = the centre values, the first `nvalid` (>= 1) of them inside the
// region.  qv = fl(b - a), what the caller stores at the valid cells; the products b * qv of those cells go into `acc`.
template <int N>
__device__ __forceinline__ void apply_cells(DotAcc &acc, const double (&a)[N], const double (&b)[N], int nvalid, double (&qv)[N]) {
    double x[N], y[N];
    bool valid[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        valid[j] = j < nvalid;
        qv[j] = b[j] - a[j];
        x[j] = valid[j] ? b[j] : 0.0;
        y[j] = valid[j] ? qv[j] : 0.0;
    }
    acc.cells<N>(x, y, valid);
}

// the workgroup's record into its own slot
__device__ __forceinline__ void finish(DotAcc &acc, ReduceRecord *__restrict__ partial) {
    wave_reduce(acc);
    __shared__ ReduceRecord sh[kThreads / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) acc.to(sh[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) acc.merge_record(sh[w]);
        ReduceRecord r;
        acc.to(r);
        partial[blockIdx.x] = r;
    }
}

__device__ __forceinline__ bool broken(const CgState *st) { return st && st->breakdown != 0; }

// ---- 1D (kernels_residual.hip: residual1d_kernel) --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void apply_dot1d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                               const ResidualTiles rt, const Taps9 W, ReduceRecord *__restrict__ partial) {
    if (broken(st)) return;
    DotAcc acc;
    acc.init();
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o[3], n[3];
        residual_tile_box(rt, t, o, n);
        const int i = o[2] + 2 * (int) threadIdx.x;  // even: the region begins on an even point, tiles are 512 points
        const int left = o[2] + n[2] - i;
        if (left <= 0) continue;
        double win[10];
        if (left >= 2) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const d2 v = *reinterpret_cast<const d2 *>(in + i + 2 * k);
                win[2 * k] = v.x;
                win[2 * k + 1] = v.y;
            }
        } else {  // odd tail: one point, scalar loads stay inside the padded array
#pragma unroll
            for (int k = 0; k < 9; ++k) win[k] = in[i + k];
            win[9] = 0.0;
        }
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            a0 = fma(W.w[k], win[k], a0);
            a1 = fma(W.w[k], win[k + 1], a1);
        }
        const double a[2] = {a0, a1}, b[2] = {win[4], win[5]};
        double qv[2];
        apply_cells<2>(acc, a, b, left >= 2 ? 2 : 1, qv);
        if (left >= 2)
            *reinterpret_cast<d2 *>(q + i + 4) = (d2){qv[0], qv[1]};
        else
            q[i + 4] = qv[0];
    }
    finish(acc, partial);
}

// ---- 2D (kernels_residual.hip: residual2d_kernel) --------------------------------------------------------------------------
constexpr int kTileW = 128;
constexpr int kLdsW = kTileW + 8;
constexpr int kChunksPerRow = kLdsW / 2;

template <int TAPSET>
__global__ __launch_bounds__(kThreads, 3) void apply_dot2d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                                  const ResidualTiles rt, const Taps49 W, ReduceRecord *__restrict__ partial) {
    constexpr int RPT = 8;
    constexpr int TH = 4 * RPT;
    constexpr int LH = TH + 6;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    __shared__ __attribute__((aligned(16))) double tile[LH * kLdsW];
    if (broken(st)) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int m = rt.dims[1], n = rt.dims[2], ld = n + 8;
    DotAcc dacc;
    dacc.init();
    for (long t = blockIdx.x; t < rt.tiles; t += gridDim.x) {
        int o[3], nn[3];
        residual_tile_box(rt, t, o, nn);
        const int i0 = o[1], j0 = o[2], row_end = o[1] + nn[1];
        const int col = j0 + 2 * lane;
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
        for (int k = 0; k < 5; ++k) cur[k] = *reinterpret_cast<const d2 *>(strip + 2 * k);
#pragma unroll
        for (int j = 0; j < RPT + 6; ++j) {
            if (j + 1 < RPT + 6) {
#pragma unroll
                for (int k = 0; k < 5; ++k) nxt[k] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kLdsW + 2 * k);
            }
            double win[10];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                win[2 * k] = cur[k].x;
                win[2 * k + 1] = cur[k].y;
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
            // output row j-6 is complete: q = centre (window row r + 3, this lane's columns) - acc at the row's two own cells
            if (j >= 6) {
                const int r = j - 6;
                const int row = i0 + wv * RPT + r;
                if (col < n && row < row_end) {  // (n and col are even: both cells or none)
                    const d2 c = *reinterpret_cast<const d2 *>(strip + (r + 3) * kLdsW + 4);
                    const double a[2] = {acc0[r], acc1[r]}, b[2] = {c.x, c.y};
                    double qv[2];
                    apply_cells<2>(dacc, a, b, 2, qv);
                    *reinterpret_cast<d2 *>(q + (size_t) (row + 4) * ld + (col + 4)) = (d2){qv[0], qv[1]};
                }
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) cur[k] = nxt[k];
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave is done with the window before the next tile's is staged
    }
    finish(dacc, partial);
}

// ---- 3D (kernels_residual.hip: residual3d_kernel) --------------------------------------------------------------------------
template <int TAPSET>
__host__ __device__ constexpr bool tap_on3(int dz, int dy, int dx) {
    return TAPSET == TAPS3D_BOX ? true : (((dz != 1) + (dy != 1) + (dx != 1)) <= 1);
}

// (bounded to three workgroups per CU like residual3d_kernel with a source: the store's address and values are as many more
// live registers through the tap loop, and at four the kernel spills; the launch is still cut by residual_tiles.h's cap)
template <int TAPSET>
__global__ __launch_bounds__(kThreads, 3) void apply_dot3d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                                  const ResidualTiles rt, const Taps27 W, ReduceRecord *__restrict__ partial) {
    constexpr int RY = 4;
    constexpr int TY = 4 * RY;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    __shared__ __attribute__((aligned(16))) double tile[2][LH * kLdsW];
    if (broken(st)) return;

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
                for (int k = 0; k < 3; ++k) {
                    const d2 v = *reinterpret_cast<const d2 *>(strip + j * kLdsW + 2 * k);
                    win[2 * k] = v.x;
                    win[2 * k + 1] = v.y;
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
                            const double a[2] = {acc0[s][r], acc1[s][r]}, b[2] = {c.x, c.y};
                            double qv[2];
                            apply_cells<2>(dacc, a, b, 2, qv);
                            *reinterpret_cast<d2 *>(q + base + (long) r * ld) = (d2){qv[0], qv[1]};
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    acc0[s][r] = 0.0;
                    acc1[s][r] = 0.0;
                }
            }
            // (as residual3d_kernel: the refill goes into the buffer of plane p - 1, which other waves' epilogues may still read)
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
    finish(dacc, partial);
}

// ---- the pointwise kernels: a walk over the interior's 16-byte pieces (ReduceArgs of the interior box, KIND_F64X2) -----------
// One cell of each rule.  UPDATE: x, r = g0, g1 (in place), p, q = g2, g3.  DIRECTION: p = g0 (in place), r = g2.  START:
// r = g0 (in place), p = g1 (stored), x = g2.  v0 / v1: the values to store at g0 / g1; the return value enters the record.
template <int OP>
__device__ __forceinline__ double cg_cell(double c, double e0, double e1, double e2, double e3, double &v0, double &v1) {
#pragma clang fp contract(off)
    if constexpr (OP == CG_OP_UPDATE) {
        const double t = c * e2;
        v0 = e0 + t;
        const double u = c * e3;
        v1 = e1 - u;
        return v1;
    } else if constexpr (OP == CG_OP_DIRECTION) {
        const double t = c * e0;
        v0 = e2 + t;
        v1 = 0.0;
        return 0.0;
    } else {
        v0 = e0 - e2;
        v1 = v0;
        return 0.0;
    }
}

template <int OP>
__global__ __launch_bounds__(kThreads, 4) void cg_pointwise_kernel(double *__restrict__ g0, double *__restrict__ g1, const double *__restrict__ g2,
                                                                   const double *__restrict__ g3, double coef, const CgState *st,
                                                                   const ReduceArgs a, ReduceRecord *__restrict__ partial) {
    constexpr bool kReads1 = OP == CG_OP_UPDATE, kReads3 = OP == CG_OP_UPDATE, kWrites1 = OP != CG_OP_DIRECTION;
    if (broken(st)) return;
    if (st) coef = OP == CG_OP_UPDATE ? st->alpha : st->beta;
    DotAcc acc;
    acc.init();
    const long first = (long) blockIdx.x * a.chunk;
    const long end = first + a.chunk < a.total ? first + a.chunk : a.total;
    long i = first + threadIdx.x;
    Cursor c;
    {
        const long row = i / a.ppr;
        const long i0 = row / a.e1;
        c.q = (int) (i - row * a.ppr);
        c.i1 = (int) (row - i0 * a.e1);
        c.off = a.off0 + i0 * a.plane_stride + c.i1 * a.row_stride + (long) c.q * 2;
    }
    const unsigned width = (unsigned) (a.col_hi - a.col_lo);
    for (; i < end; i += kThreads) {
        const unsigned col = (unsigned) ((a.q0 + c.q) * 2 - a.col_lo);  // (unsigned: a cell left of the box wraps to a huge value)
        const bool in0 = col < width, in1 = col + 1 < width;
        if (in0 && in1) {
            const d2 e0 = *reinterpret_cast<const d2 *>(g0 + c.off), e2 = *reinterpret_cast<const d2 *>(g2 + c.off);
            d2 e1 = {0.0, 0.0}, e3 = {0.0, 0.0};
            if constexpr (kReads1) e1 = *reinterpret_cast<const d2 *>(g1 + c.off);
            if constexpr (kReads3) e3 = *reinterpret_cast<const d2 *>(g3 + c.off);
            double v0[2], v1[2], s[2];
            s[0] = cg_cell<OP>(coef, e0.x, e1.x, e2.x, e3.x, v0[0], v1[0]);
            s[1] = cg_cell<OP>(coef, e0.y, e1.y, e2.y, e3.y, v0[1], v1[1]);
            *reinterpret_cast<d2 *>(g0 + c.off) = (d2){v0[0], v0[1]};
            if constexpr (kWrites1) *reinterpret_cast<d2 *>(g1 + c.off) = (d2){v1[0], v1[1]};
            if constexpr (OP == CG_OP_UPDATE) {
                const bool valid[2] = {true, true};
                acc.cells<2>(s, s, valid);
            }
        } else if (in0 || in1) {  // a piece with one interior cell: 8-byte loads and stores of that cell alone
            const long off = c.off + (in0 ? 0 : 1);
            const double e0 = g0[off], e2 = g2[off], e1 = kReads1 ? g1[off] : 0.0, e3 = kReads3 ? g3[off] : 0.0;
            double v0, v1;
            const double s[1] = {cg_cell<OP>(coef, e0, e1, e2, e3, v0, v1)};
            g0[off] = v0;
            if constexpr (kWrites1) g1[off] = v1;
            if constexpr (OP == CG_OP_UPDATE) {
                const bool valid[1] = {true};
                acc.cells<1>(s, s, valid);
            }
        }
        c.advance(a);
    }
    if constexpr (OP == CG_OP_UPDATE) finish(acc, partial);
}

// ---- the fold and, behind it, the one-lane update of the scalars -----------------------------------------------------------
// the stepper: a step is finished after `iters` iterations at r.r = rr -- its entry in the history, and the counts
__device__ __forceinline__ void theta_step_done(ThetaState *ts, long long iters, double rr, bool unconverged) {
    long long *hist_iters = reinterpret_cast<long long *>(ts + 1);
    double *hist_rr = reinterpret_cast<double *>(hist_iters + ts->cap);
    const long long n = ts->steps_done;
    if (n < ts->cap) {
        hist_iters[n] = iters;
        hist_rr[n] = rr;
    }
    ts->steps_done = n + 1;
    ts->unconverged += unconverged ? 1 : 0;
}
__global__ __launch_bounds__(64) void cg_fold_kernel(ReduceRecord *__restrict__ partial, int groups, CgState *st, int phase, int cap, ThetaState *ts,
                                                     double rtol2, int max_iters) {
    if (phase == CG_FOLD_THETA_INIT) {  // the head of a stepper's run: both states reset, no record read
        if (threadIdx.x != 0) return;
        const CgState s0 = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
        *st = s0;
        const ThetaState t0 = {0.0, 0.0, rtol2, max_iters, 0, 0, cap};
        *ts = t0;
        return;
    }
    if (phase == CG_FOLD_PCG_INIT) {  // the head of a preconditioned run: the state reset, no record read
        if (threadIdx.x != 0) return;
        const CgState s0 = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
        *st = s0;
        return;
    }
    // a start is not held back by `done`, which belongs to the step before it
    if (phase == CG_FOLD_THETA_START ? (st->breakdown & CG_HALT_BREAKDOWN) != 0 : (phase != CG_FOLD_START && broken(st))) return;
    const bool from_dot = phase == CG_FOLD_START || phase == CG_FOLD_PCG_RZ0 || phase == CG_FOLD_PCG_RZ;
    DotAcc acc;
    acc.init();
    if (from_dot) {  // the record lora_plan_dot's own fold left
        acc.merge_record(partial[kReduceMaxGroups]);
    } else {
        for (int g = threadIdx.x; g < groups; g += 64) acc.merge_record(partial[g]);
        wave_reduce(acc);
    }
    if (threadIdx.x != 0) return;
    if (!from_dot) {
        ReduceRecord r;
        acc.to(r);
        partial[kReduceMaxGroups] = r;
    }
    if (!st) return;
    double *hist_alpha = reinterpret_cast<double *>(st + 1), *hist_beta = hist_alpha + cap;
    PcgState *ps = reinterpret_cast<PcgState *>(hist_beta + cap);  // (read and written by the PCG phases alone)
    if (phase == CG_FOLD_PCG_RZ0 || phase == CG_FOLD_PCG_RZ) {
        // rz = r.z with z = M r: not finite or negative is a breakdown; zero (r vanished) halts the launches behind it as well
        const double rz_new = acc.dot;
        if (phase == CG_FOLD_PCG_RZ) {
            const double beta = rz_new / ps->rz;
            const long long it = st->iteration - 1;  // the iteration whose update ran before z = M r
            if (it >= 0 && it < cap) hist_beta[it] = beta;
            st->beta = beta;
        }
        ps->rz = rz_new;
        if (acc.nf > 0 || !finite64(rz_new) || !(rz_new > 0.0)) st->breakdown |= CG_HALT_BREAKDOWN;
    } else if (phase == CG_FOLD_PCG_APPLY) {
        const double pq = acc.dot, rz = ps->rz;
        st->pq = pq;
        if (acc.nf > 0 || !finite64(pq) || !(pq > 0.0) || !finite64(rz))
            st->breakdown = 1;
        else
            st->alpha = rz / pq;
    } else if (phase == CG_FOLD_PCG_UPDATE || phase == CG_FOLD_PCG_THETA_UPDATE) {  // the iteration is applied; beta follows z = M r
        const double rr_new = acc.dot;
        const long long it = st->iteration;
        if (it < cap) hist_alpha[it] = st->alpha;
        st->rr = rr_new;
        st->r_abs_max = acc.amax;
        st->iteration = it + 1;
        if (acc.nf > 0 || !finite64(rr_new)) {
            st->breakdown = 1;
        } else if (phase == CG_FOLD_PCG_THETA_UPDATE) {
            const bool met = rr_new <= ts->thresh;
            if (met || it + 1 >= ts->max_iters) {
                st->breakdown = CG_HALT_DONE;
                theta_step_done(ts, it + 1, rr_new, !met);
            }
        }
    } else if (phase == CG_FOLD_START) {
        CgState s0 = {acc.dot, 0.0, 0.0, 0.0, acc.amax, 0, (acc.nf > 0 || !finite64(acc.dot)) ? 1 : 0};
        *st = s0;
    } else if (phase == CG_FOLD_THETA_START) {
#pragma clang fp contract(off)
        const double rr0 = acc.dot;
        const bool bad = acc.nf > 0 || !finite64(rr0);
        CgState s0 = {rr0, 0.0, 0.0, 0.0, acc.amax, 0, bad ? CG_HALT_BREAKDOWN : (rr0 == 0.0 ? CG_HALT_DONE : 0)};
        *st = s0;
        ts->rr0 = rr0;
        ts->thresh = ts->rtol2 * rr0;
        if (!bad && rr0 == 0.0) theta_step_done(ts, 0, 0.0, false);  // nothing to do: the level is steady
    } else if (phase == CG_FOLD_APPLY) {
        const double pq = acc.dot, rr = st->rr;
        st->pq = pq;
        if (acc.nf > 0 || !finite64(pq) || !(pq > 0.0) || !finite64(rr))
            st->breakdown = 1;
        else
            st->alpha = rr / pq;
    } else {  // CG_FOLD_UPDATE, CG_FOLD_THETA_UPDATE: the iteration is applied
        const double rr_new = acc.dot, beta = rr_new / st->rr;
        const long long it = st->iteration;
        if (phase == CG_FOLD_UPDATE && it < cap) {
            hist_alpha[it] = st->alpha;
            hist_beta[it] = beta;
        }
        st->beta = beta;
        st->rr = rr_new;
        st->r_abs_max = acc.amax;
        st->iteration = it + 1;
        if (acc.nf > 0 || !finite64(rr_new)) {
            st->breakdown = 1;
        } else if (phase == CG_FOLD_THETA_UPDATE) {
            const bool met = rr_new <= ts->thresh;
            if (met || it + 1 >= ts->max_iters) {
                st->breakdown = CG_HALT_DONE;
                theta_step_done(ts, it + 1, rr_new, !met);
            }
        }
    }
}

}  // namespace

hipError_t launch_apply_dot(const Plan &p, const ResidualTiles &rt, const double *d_p, double *d_q, const CgState *st, ReduceRecord *partial,
                            hipStream_t s) {
    if (!has_cg(p) || rt.groups < 1 || rt.groups > kReduceMaxGroups) return hipErrorInvalidValue;
    const dim3 grid((unsigned) rt.groups), block(kThreads);
    if (p.ndim == 1) {
        Taps9 w;
        for (int k = 0; k < 9; ++k) w.w[k] = p.w[k];
        hipLaunchKernelGGL(apply_dot1d_kernel, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
    } else if (p.ndim == 2) {
        Taps49 w;
        for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
        if (p.tapset == TAPS2D_DIAMOND)
            hipLaunchKernelGGL(apply_dot2d_kernel<TAPS2D_DIAMOND>, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
        else if (p.tapset == TAPS2D_STAR)
            hipLaunchKernelGGL(apply_dot2d_kernel<TAPS2D_STAR>, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
        else
            hipLaunchKernelGGL(apply_dot2d_kernel<TAPS2D_BOX>, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
    } else {
        Taps27 w;
        for (int k = 0; k < 27; ++k) w.w[k] = p.w[k];
        if (p.tapset == TAPS3D_STAR)
            hipLaunchKernelGGL(apply_dot3d_kernel<TAPS3D_STAR>, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
        else
            hipLaunchKernelGGL(apply_dot3d_kernel<TAPS3D_BOX>, grid, block, 0, s, d_p, d_q, st, rt, w, partial);
    }
    return hipGetLastError();
}

hipError_t launch_cg_pointwise(int op, const ReduceArgs &a, int kind, int groups, double *g0, double *g1, const double *g2, const double *g3,
                               double coef, const CgState *st, ReduceRecord *partial, hipStream_t s) {
    if (kind != KIND_F64X2 || groups < 1 || groups > kReduceMaxGroups) return hipErrorInvalidValue;
    const dim3 grid((unsigned) groups), block(kThreads);
    if (op == CG_OP_UPDATE)
        hipLaunchKernelGGL(cg_pointwise_kernel<CG_OP_UPDATE>, grid, block, 0, s, g0, g1, g2, g3, coef, st, a, partial);
    else if (op == CG_OP_DIRECTION)
        hipLaunchKernelGGL(cg_pointwise_kernel<CG_OP_DIRECTION>, grid, block, 0, s, g0, g1, g2, g3, coef, st, a, partial);
    else
        hipLaunchKernelGGL(cg_pointwise_kernel<CG_OP_START>, grid, block, 0, s, g0, g1, g2, g3, coef, st, a, partial);
    return hipGetLastError();
}

hipError_t launch_cg_fold(ReduceRecord *partial, int groups, CgState *st, int phase, int cap, hipStream_t s, ThetaState *ts, double rtol2,
                          int max_iters) {
    const bool theta = (phase >= CG_FOLD_THETA_INIT && phase <= CG_FOLD_THETA_UPDATE) || phase == CG_FOLD_PCG_THETA_UPDATE;
    if ((theta && !ts) || (phase >= CG_FOLD_THETA_INIT && !st)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cg_fold_kernel, dim3(1), dim3(64), 0, s, partial, groups, st, phase, cap, ts, rtol2, max_iters);
    return hipGetLastError();
}

}  // namespace lora
