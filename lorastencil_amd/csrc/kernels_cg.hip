// kernels_cg.hip -- the hot path of the conjugate-gradient solver for u = S(u) + f (host side: cg.cpp).  The operator
// is A = I - S, S the plan's raw single sweep; fp64 plans with the fused residual kernel only.
//
//   apply_dot     q = fl(p - acc) on every interior cell of the range and, in the same launch, the record of dot(p, q).  `acc`
//                 has the bits lora_plan_step_region stores for p: the kernels are wrappers round tile_walk.h's walk (window,
//                 tile sizes, tap order, centre value re-read from the window), which the residual kernels run too, and supply
//                 the row's epilogue (ApplyRow).  The residual has a = acc and b = centre and reduces b - a; this one STORES
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
#include "tile_walk.h"

namespace lora {

namespace {

using namespace walk;

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

__device__ __forceinline__ bool broken(const CgState *st) { return st && st->breakdown != 0; }

// What apply_dot does with a row's tap sums: q = fl(centre - acc) stored at the row's cells inside the region, 16 bytes, or 8 for
// the odd 1D tail point.
struct ApplyRow {
    static constexpr bool kSrc = false;
    double *__restrict__ q;
    DotAcc acc;
    __device__ __forceinline__ void row(double a0, double a1, d2 c, d2, int nvalid, long long idx0) {
        const double a[2] = {a0, a1}, b[2] = {c.x, c.y};
        double qv[2];
        apply_cells<2>(acc, a, b, nvalid, qv);
        if (nvalid >= 2)
            *reinterpret_cast<d2 *>(q + idx0) = (d2){qv[0], qv[1]};
        else
            q[idx0] = qv[0];
    }
};

__global__ __launch_bounds__(kThreads) void apply_dot1d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                               const ResidualTiles rt, const Taps9 W, ReduceRecord *__restrict__ partial) {
    if (broken(st)) return;
    ApplyRow pol{q};
    pol.acc.init();
    tile_walk1d(in, nullptr, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
}

template <int TAPSET>
__global__ __launch_bounds__(kThreads, 3) void apply_dot2d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                                  const ResidualTiles rt, const Taps49 W, ReduceRecord *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double tile[kWalk2dTile];
    if (broken(st)) return;
    ApplyRow pol{q};
    pol.acc.init();
    tile_walk2d<TAPSET>(tile, in, nullptr, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
}

// (bounded to three workgroups per CU like residual3d_kernel with a source: the store's address and values are as many more
// live registers through the tap loop, and at four the kernel spills; the launch is still cut by residual_tiles.h's cap)
template <int TAPSET>
__global__ __launch_bounds__(kThreads, 3) void apply_dot3d_kernel(const double *__restrict__ in, double *__restrict__ q, const CgState *st,
                                                                  const ResidualTiles rt, const Taps27 W, ReduceRecord *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double tile[2][kWalk3dTile];
    if (broken(st)) return;
    ApplyRow pol{q};
    pol.acc.init();
    tile_walk3d<TAPSET>(tile, in, nullptr, rt, W, pol);
    finish<kThreads>(pol.acc, partial);
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
    if constexpr (OP == CG_OP_UPDATE) finish<kThreads>(acc, partial);
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
