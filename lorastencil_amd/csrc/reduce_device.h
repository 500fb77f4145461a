// reduce_device.h -- device pieces the reductions share (kernels_reduce.hip, kernels_residual.hip): the state of a
// difference reduction, its merge rule, and the fixed orders in which lanes and waves are folded.
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

// a wave's 64 states into every lane, always in the same order; sums commute bit for bit, so both sides of a pair agree
template <typename ACC>
__device__ __forceinline__ void wave_reduce(ACC &acc) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc.merge_lane(m);
}

}  // namespace lora
