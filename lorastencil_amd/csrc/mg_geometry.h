// mg_geometry.h -- the restriction's per-axis geometry, shared by the transfer kernels (kernels_mg.hip) and the fused
// defect-and-restrict kernel (kernels_mg_fused.hip): which fine cells a coarse cell gathers, with which integer numerators, and
// the one coefficient the host rounds.  kernels_mg.hip has the derivation.
#pragma once

#include <hip/hip_runtime.h>

namespace lora {

// t = q N + rem, 0 <= rem < N, for t >= 0: 32-bit division whenever t allows it
__device__ __forceinline__ void mg_divide(long long t, int N, int &q, int &rem) {
    if (t <= 0x7fffffffLL) {
        const unsigned u = (unsigned) t, d = (unsigned) N;
        const unsigned k = u / d;
        q = (int) k;
        rem = (int) (u - k * d);
    } else {
        const long long k = t / N;
        q = (int) k;
        rem = (int) (t - k * N);
    }
}

// the first fine cell (0-based) that may have a positive numerator for coarse cell j: floor(j N / M)
__device__ __forceinline__ int restrict_lo(int j, int n, int nc) {
    int q, rem;
    mg_divide((long long) j * (n + 1), nc + 1, q, rem);
    return q;
}
// the numerator of fine cell i for coarse cell j, 0 where it is not positive or i is outside the interior
__device__ __forceinline__ double restrict_num(int i, int j, int n, int nc) {
    const long long N = n + 1, d = (long long) (i + 1) * (nc + 1) - (long long) (j + 1) * N;
    const long long a = N - (d < 0 ? -d : d);
    return (a > 0 && i < n) ? (double) a : 0.0;
}

// a grid's extents as z, y, x and the padded layout of lora_padded_count: 2D pads (4, 4), 3D pads (1, 2, 4)
inline void mg_side(int ndim, const int *dims, int *n, long &row, long &plane, long &off) {
    n[0] = ndim == 3 ? dims[0] : 1;
    n[1] = dims[ndim - 2];
    n[2] = dims[ndim - 1];
    row = n[2] + 8;
    plane = ndim == 3 ? (long) (n[1] + 4) * row : 0;
    off = ndim == 3 ? plane + 2 * row + 4 : 4 * row + 4;
}

// the restriction's coefficient, scale prod_a (M_a / N_a) / prod_a N_a over the last `ndim` of the axes z, y, x, rounded once
inline double restrict_coef(int ndim, const int *n, const int *nc, double scale) {
    long double c = scale;
    for (int d = 3 - ndim; d < 3; ++d) c = c * (long double) (nc[d] + 1) / ((long double) (n[d] + 1) * (long double) (n[d] + 1));
    return (double) c;
}

}  // namespace lora
