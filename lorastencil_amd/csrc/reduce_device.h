// reduce_device.h -- device pieces the reductions share (kernels_reduce.hip, kernels_residual.hip, kernels_cg.hip,
// kernels_theta.hip): the states of a difference and of a product reduction, their merge rules, the walk over a box's pieces,
// the fixed orders in which lanes and waves are folded, and finish(), which writes a workgroup's record.
#pragma once

#include <hip/hip_runtime.h>

#include "engine.h"

namespace lora {

constexpr long long kNoIndex = 0x7fffffffffffffffLL;


__device__ __forceinline__ bool finite64(double x) {
    return (__double_as_longlong(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// (`idx`: in kernels_reduce.hip the cell offset of the PIECE that holds the maximum -- lanes walk pieces in ascending order
// and take a piece on a strictly larger maximum, merges prefer the lower offset, and the fold launch finds the cell inside
// the piece; in kernels_residual.hip the cell's own padded linear index, KIND_CELL to the fold)
struct DiffAcc {
    double mx, sq, amax;  // mx = -1 while no finite difference was seen
    long long idx, nf;
    __device__ __forceinline__ void init() {
        mx = -1.0;
        sq = amax = 0.0;
        idx = kNoIndex;
        nf = 0;
    }
    __device__ __forceinline__ void merge(double omx, double osq, double oamax, long long oidx, long long onf) {
        const bool take = omx > mx || (omx == mx && oidx < idx);
        mx = take ? omx : mx;
        idx = take ? oidx : idx;
        sq += osq;
        amax = oamax > amax ? oamax : amax;
        nf += onf;
    }
    __device__ __forceinline__ void merge_lane(int m) {  // with the state of lane ^ m
        merge(__shfl_xor(mx, m), __shfl_xor(sq, m), __shfl_xor(amax, m), __shfl_xor(idx, m), __shfl_xor(nf, m));
    }
    __device__ __forceinline__ void merge_record(const ReduceRecord &r) { merge(r.f[0], r.f[1], r.f[2], r.i[0], r.i[1]); }
    __device__ __forceinline__ void to(ReduceRecord &r) const {
        r.f[0] = mx;
        r.f[1] = sq;
        r.f[2] = amax;
        r.f[3] = 0.0;
        r.i[0] = idx;
        r.i[1] = nf;
    }
};

// The state of a product reduction (lora_plan_dot, the fused reductions of kernels_cg.hip): sum of the finite products a * b,
// sum of their magnitudes, the largest |a| among them, and how many products were not finite.
struct DotAcc {
    double dot, sabs, amax;
    long long nf;
    __device__ __forceinline__ void init() {
        dot = sabs = amax = 0.0;
        nf = 0;
    }
    // N cells a lane holds at once (a piece, or its cells of one row); cells that are not `valid` must come in as a = b = 0.
    // Every product is its own rounding.  One finite test of the magnitudes' sum, the exact cell-by-cell path only when it fails.
    template <int N>
    __device__ __forceinline__ void cells(const double (&a)[N], const double (&b)[N], const bool (&valid)[N]) {
#pragma clang fp contract(off)
        double pr[N], s = 0.0, sa = 0.0, am = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            pr[j] = a[j] * b[j];
            s += pr[j];
            sa += fabs(pr[j]);
            am = fmax(am, fabs(a[j]));
        }
        if (!finite64(sa)) {  // some product is not finite (or the sum overflowed): cell by cell
            s = sa = am = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const bool ok = valid[j] && finite64(pr[j]);
                nf += (valid[j] && !ok) ? 1 : 0;
                s += ok ? pr[j] : 0.0;
                sa += ok ? fabs(pr[j]) : 0.0;
                am = (ok && fabs(a[j]) > am) ? fabs(a[j]) : am;
            }
        }
        dot += s;
        sabs += sa;
        amax = am > amax ? am : amax;
    }
    __device__ __forceinline__ void merge(double odot, double osabs, double oamax, long long onf) {
        dot += odot;
        sabs += osabs;
        amax = oamax > amax ? oamax : amax;
        nf += onf;
    }
    __device__ __forceinline__ void merge_lane(int m) {  // with the state of lane ^ m
        merge(__shfl_xor(dot, m), __shfl_xor(sabs, m), __shfl_xor(amax, m), __shfl_xor(nf, m));
    }
    __device__ __forceinline__ void merge_record(const ReduceRecord &r) { merge(r.f[0], r.f[1], r.f[2], r.i[0]); }
    __device__ __forceinline__ void to(ReduceRecord &r) const {
        r.f[0] = dot;
        r.f[1] = sabs;
        r.f[2] = amax;
        r.f[3] = 0.0;
        r.i[0] = nf;
        r.i[1] = 0;
    }
};

// Where a lane is on the line of pieces of a box (reduce.cpp: reduce_geometry): the piece within its row, the row within its
// plane, and the cell offset; one stride of the lanes further by the step's precomputed digits with carries.
struct Cursor {
    int q, i1;
    long off;
    __device__ __forceinline__ void advance(const ReduceArgs &a) {
        q += a.dq;
        const bool c = q >= a.ppr;
        q -= c ? a.ppr : 0;
        i1 += a.d1 + (c ? 1 : 0);
        const bool c1 = i1 >= a.e1;
        i1 -= c1 ? a.e1 : 0;
        off += a.step_off + (c ? a.row_carry : 0) + (c1 ? a.plane_carry : 0);
    }
};

// a wave's 64 states into every lane, always in the same order; sums commute bit for bit, so both sides of a pair agree
template <typename ACC>
__device__ __forceinline__ void wave_reduce(ACC &acc) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc.merge_lane(m);
}

// the record of a workgroup into its own slot: lanes by wave_reduce, the waves through LDS in wave order.  THREADS is the
// launch's block size: the number of waves folded is fixed at compile time, so a caller names it
template <int THREADS, typename ACC>
__device__ __forceinline__ void finish(ACC &acc, ReduceRecord *__restrict__ partial) {
    static_assert(THREADS % 64 == 0, "whole waves");
    constexpr int kWaves = THREADS / 64;
    wave_reduce(acc);
    __shared__ ReduceRecord sh[kWaves];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) acc.to(sh[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) acc.merge_record(sh[w]);
        ReduceRecord r;
        acc.to(r);
        partial[blockIdx.x] = r;
    }
}

}  // namespace lora
