// step_epilogue.h -- the ONE definition of what a step kernel does with a finished tap sum, and of the direct tap loop of
// the 2D two-step kernel.  Shared by kernels_step.hip (one step per launch) and step2_body.h (two per launch:
// kernels_2d_step2.hip, kernels_2d_wave2.hip): "a two-step launch equals two single steps bit for bit" holds because both sides
// call these functions.
#pragma once

#include "device_common.h"

namespace lora {

// The update rule at the store.  `acc` has the bits the plan's plain single sweep stores; every operation after it is its
// own fp64 rounding.  Each rule is its own instantiation: "no source" is not "add a zero" (-0.0 + 0.0 changes bits) and
// leapfrog is not "scale by 1" (a multiply per point).  An operand a rule does not read is never loaded.
enum {
    EPI_SOURCE = 0,       // out  = fl(acc + f)
    EPI_LEAP = 1,         // prev = fl(acc + fl(c prev))
    EPI_LEAP_SCALED = 2,  // prev = fl(fl(a acc) + fl(c prev))
    EPI_LEAP_SRC = 3,     // prev = fl(fl(a fl(acc + f)) + fl(c prev))
    EPI_WAVE = 4,         // prev = fl(fl(fl(k acc) + fl(b u)) + fl(c prev)): k a per-cell grid in f's place, u the centre cell of cur
};
constexpr bool epi_reads_f(int epi) { return epi == EPI_SOURCE || epi == EPI_LEAP_SRC || epi == EPI_WAVE; }
constexpr bool epi_reads_prev(int epi) { return epi != EPI_SOURCE; }
constexpr bool epi_reads_u(int epi) { return epi == EPI_WAVE; }

// acc + c * x in two roundings: contraction is switched off around the expression
__device__ __forceinline__ double leap(double acc, double c, double x) {
#pragma clang fp contract(off)
    const double t = c * x;
    return acc + t;
}

// a * (acc + f) + c * x, every operation its own rounding: contraction is switched off around the expression
template <bool SRC>
__device__ __forceinline__ double leap_src(double acc, double f, double sa, double c, double x) {
#pragma clang fp contract(off)
    double t = acc;
    if constexpr (SRC) t = acc + f;
    const double p = sa * t;
    const double q = c * x;
    return p + q;
}

// k * acc + b * u + c * x, five roundings: contraction is switched off around the expression
__device__ __forceinline__ double wave(double acc, double k, double b, double u, double c, double x) {
#pragma clang fp contract(off)
    const double p = k * acc;
    const double q = b * u;
    const double s = p + q;
    const double t = c * x;
    return s + t;
}

// The stored value of rule EPI; `f`, `sa`, `c`, `x` (the old value at the store's address) and `u` (the cell of the swept grid
// at the store's address) are ignored where the rule has none.  EPI_WAVE: f carries k, sa carries b.
template <int EPI>
__device__ __forceinline__ double step_epilogue(double acc, double f, double sa, double c, double x, double u = 0.0) {
    if constexpr (EPI == EPI_SOURCE) {
        return acc + f;
    } else if constexpr (EPI == EPI_LEAP) {
        return leap(acc, c, x);
    } else if constexpr (EPI == EPI_WAVE) {
        return wave(acc, f, sa, u, c, x);
    } else {
        return leap_src<EPI == EPI_LEAP_SRC>(acc, f, sa, c, x);
    }
}

// One window row (8 values) into the accumulators of the rows it contributes to: direct taps, row-major order.
template <int TAPSET, int R>
__device__ __forceinline__ void taps_row(int j, const double (&win)[8], double (&acc0)[R], double (&acc1)[R], const Taps49 &W) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int dy = j - r;
        if (dy >= 0 && dy < 7) {
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                if (tap_on<TAPSET>(dy, dx)) {
                    const double wt = W.w[dy * 7 + dx];
                    acc0[r] = fma(wt, win[dx], acc0[r]);
                    acc1[r] = fma(wt, win[dx + 1], acc1[r]);
                }
            }
        }
    }
}

}  // namespace lora
