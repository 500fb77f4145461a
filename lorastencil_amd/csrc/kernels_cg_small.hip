// kernels_cg_small.hip -- fixed-count conjugate gradients for A = sigma I - tau S on a grid small enough for ONE workgroup: the
// whole solve is ONE launch (host side: cg.cpp, lora_plan_cg_small; the coarsest level of a multigrid cycle behind plan option
// coarse1: mg.cpp).  fp64, 2D and 3D plans with the CG kernels, any taps, zero Dirichlet halo.
//
// Data.  Lane t of the workgroup owns the interior cells t, t + T, t + 2 T, ... (T lanes, row-major cell index, at most
// kCgSmallCellsPerLane of them) and keeps their x, r, p and q in registers.  p also lives in LDS inside a ring of zeros as wide
// as the tap radius (3 cells per side in 2D, 1 in 3D), so a tap that reaches past the grid reads a zero of the ring and no halo
// cell of a global grid is ever loaded.  x and r are read once (8-byte loads of interior cells), written once at the end;
// nothing touches global memory in between.
//
// Arithmetic.  Every operation outside a tap sum is its own rounding (#pragma clang fp contract(off), as kernels_cg.hip); the tap
// sum is a chain of fused multiply-adds from 0 over the non-zero taps in ascending tap index.  Per iteration
//     q = fl(fl(sigma p) - fl(tau acc))   (sigma == tau == 1: q = fl(p - acc))
//     pq = p.q;  alpha = rr / pq;  x = fl(x + fl(alpha p));  r = fl(r - fl(alpha q));  rr' = r.r;  beta = rr' / rr;
//     p = fl(r + fl(beta p))
// A dot folds in a fixed order: a lane's products in the order of its cells, added from 0; the 64 lanes of a wave by the butterfly
// of reduce_device.h; the waves in wave order, each lane adding the same LDS slots.  No atomics: every lane divides the same two
// sums, so alpha and beta have the same bits in every lane and the same call gives the same bits every time.
//
// Halting is uniform (every lane decides on the same bits): rr == 0 before an iteration ends the loop as converged (halt 1);
// pq not finite or <= 0 ends it as a breakdown (halt 2) with x and r as they were before the iteration; a non-finite rr' ends it
// as a breakdown behind the update that produced it, which counts as done.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "reduce_device.h"

namespace lora {

namespace {

constexpr int kMaxThreads = 1024;
constexpr int kMaxWaves = kMaxThreads / 64;

// the non-zero taps in ascending tap index: weight and offset inside the ringed LDS array
struct SmallTaps {
    int count;
    int off[49];
    double w[49];
};

// interior extents e (2D: e[0] = 1), the ringed LDS array and the padded global array, all in cells
struct SmallGeom {
    int cells;
    int e1, e2;
    int ring0, ring1, ring2, lds_row, lds_plane, lds_cells;
    int pad0, pad1, pad2, g_row;
    long g_plane;
};

struct SumAcc {
    double s;
    __device__ __forceinline__ void merge_lane(int m) { s += __shfl_xor(s, m); }
};

// the workgroup's sum of v in every lane: butterfly, then the waves' sums in wave order (`slot`: kMaxWaves doubles of LDS that
// nothing else writes before the workgroup's next barrier)
__device__ __forceinline__ double block_sum(double v, double *slot, int lane, int wave, int nwaves) {
#pragma clang fp contract(off)
    SumAcc a = {v};
    wave_reduce(a);
    if (lane == 0) slot[wave] = a.s;
    __syncthreads();
    double s = slot[0];
    for (int w = 1; w < nwaves; ++w) s += slot[w];
    return s;
}

template <int CPL>
__global__ __launch_bounds__(kMaxThreads) void cg_small_kernel(double *__restrict__ gx, double *__restrict__ gr, const SmallGeom g,
                                                               const SmallTaps T, int iters, double sigma, double tau, int shifted,
                                                               double *__restrict__ info) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *slot_pq = lds, *slot_rr = lds + kMaxWaves, *P = lds + 2 * kMaxWaves;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;

    bool own[CPL];
    int po[CPL];
    long go[CPL];
    double x[CPL], r[CPL], p[CPL], q[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = tid + j * nthreads;
        own[j] = c < g.cells;
        const int cc = own[j] ? c : 0;
        const int i2 = cc % g.e2, t = cc / g.e2;
        const int i1 = t % g.e1, i0 = t / g.e1;
        po[j] = (i0 + g.ring0) * g.lds_plane + (i1 + g.ring1) * g.lds_row + (i2 + g.ring2);
        go[j] = (long) (i0 + g.pad0) * g.g_plane + (long) (i1 + g.pad1) * g.g_row + (i2 + g.pad2);
        x[j] = own[j] ? gx[go[j]] : 0.0;
        r[j] = own[j] ? gr[go[j]] : 0.0;
        p[j] = r[j];
        q[j] = 0.0;
    }
    for (int k = tid; k < g.lds_cells; k += nthreads) P[k] = 0.0;
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        if (own[j]) P[po[j]] = p[j];
        const double rr_j = r[j] * r[j];
        part += rr_j;
    }
    double rr = block_sum(part, slot_rr, lane, wave, nwaves);
    const double rr0 = rr;

    int done = 0, halt = 0;
    for (int it = 0; it < iters; ++it) {
        if (rr == 0.0) {
            halt = 1;
            break;
        }
        __syncthreads();  // every lane's p is in LDS
        part = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            double acc = 0.0;
            if (own[j]) {
                const double *centre = P + po[j];
                for (int t = 0; t < T.count; ++t) acc = fma(T.w[t], centre[T.off[t]], acc);
            }
            if (shifted) {
                const double sp = sigma * p[j];
                const double ta = tau * acc;
                q[j] = sp - ta;
            } else {
                q[j] = p[j] - acc;
            }
            const double pq_j = p[j] * q[j];
            part += pq_j;
        }
        const double pq = block_sum(part, slot_pq, lane, wave, nwaves);
        if (!finite64(pq) || !(pq > 0.0)) {
            halt = 2;
            break;
        }
        const double alpha = rr / pq;
        part = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double ap = alpha * p[j];
            x[j] = x[j] + ap;
            const double aq = alpha * q[j];
            r[j] = r[j] - aq;
            const double rr_j = r[j] * r[j];
            part += rr_j;
        }
        const double rr_new = block_sum(part, slot_rr, lane, wave, nwaves);
        done = it + 1;
        if (!finite64(rr_new)) {
            rr = rr_new;
            halt = 2;
            break;
        }
        const double beta = rr_new / rr;
        rr = rr_new;
        // (every lane has read p for this iteration: two barriers lie between the tap sums and here)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double bp = beta * p[j];
            p[j] = r[j] + bp;
            if (own[j]) P[po[j]] = p[j];
        }
    }

#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        if (own[j]) {
            gx[go[j]] = x[j];
            gr[go[j]] = r[j];
        }
    }
    if (info && tid == 0) {
        info[0] = rr0;
        info[1] = rr;
        info[2] = (double) done;
        info[3] = (double) halt;
    }
}

}  // namespace

hipError_t launch_cg_small(const Plan &p, double *d_x, double *d_r, int iters, double sigma, double tau, double *d_info, hipStream_t s) {
    if (!has_cg_small(p) || iters < 1) return hipErrorInvalidValue;
    const bool two = p.ndim == 2;
    SmallGeom g;
    const int e0 = two ? 1 : p.dims[0];
    g.e1 = two ? p.dims[0] : p.dims[1];
    g.e2 = two ? p.dims[1] : p.dims[2];
    g.cells = e0 * g.e1 * g.e2;
    g.ring0 = two ? 0 : 1;
    g.ring1 = g.ring2 = two ? 3 : 1;
    g.lds_row = g.e2 + 2 * g.ring2;
    g.lds_plane = (g.e1 + 2 * g.ring1) * g.lds_row;
    g.lds_cells = (e0 + 2 * g.ring0) * g.lds_plane;
    g.pad0 = two ? 0 : 1;
    g.pad1 = two ? 4 : 2;
    g.pad2 = 4;
    g.g_row = g.e2 + 8;
    g.g_plane = (long) (g.e1 + 2 * g.pad1) * g.g_row;
    SmallTaps t;
    t.count = 0;
    for (int k = 0; k < p.ntaps; ++k) {
        if (p.w[k] == 0.0) continue;
        const int d0 = two ? 0 : k / 9 - 1, d1 = two ? k / 7 - 3 : k / 3 % 3 - 1, d2 = two ? k % 7 - 3 : k % 3 - 1;
        t.off[t.count] = d0 * g.lds_plane + d1 * g.lds_row + d2;
        t.w[t.count] = p.w[k];
        ++t.count;
    }
    for (int k = t.count; k < 49; ++k) {
        t.off[k] = 0;
        t.w[k] = 0.0;
    }
    const int threads = g.cells >= kMaxThreads ? kMaxThreads : (g.cells + 63) / 64 * 64;
    const int cpl = (g.cells + threads - 1) / threads;
    const size_t lds_bytes = cg_small_lds_bytes(p);
    const int shifted = !(sigma == 1.0 && tau == 1.0);  // (1, 1) takes the plain form
    const dim3 grid(1), block((unsigned) threads);
    if (cpl == 1)
        hipLaunchKernelGGL(cg_small_kernel<1>, grid, block, lds_bytes, s, d_x, d_r, g, t, iters, sigma, tau, shifted, d_info);
    else if (cpl == 2)
        hipLaunchKernelGGL(cg_small_kernel<2>, grid, block, lds_bytes, s, d_x, d_r, g, t, iters, sigma, tau, shifted, d_info);
    else if (cpl <= kCgSmallCellsPerLane)
        hipLaunchKernelGGL(cg_small_kernel<kCgSmallCellsPerLane>, grid, block, lds_bytes, s, d_x, d_r, g, t, iters, sigma, tau, shifted, d_info);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace lora
