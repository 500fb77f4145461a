// kernels_mg.hip -- the inter-grid transfers of the geometric multigrid solver (host side: mg.cpp), fp64, 2D and 3D.
//
// Coarsening is boundary-aligned and non-nested: per axis a fine grid of n interior cells and a coarse one of n_c span the same
// interval from halo centre to halo centre, so with N = n + 1 and M = n_c + 1 fine cell i sits at (i + 1) / N and coarse cell j at
// (j + 1) / M.  The linear-interpolation weight of the pair is
//     p(i, j) = max(0, num(i, j)) / N,   num(i, j) = N - |(i + 1) M - (j + 1) N|,
// an exact integer over N.  Both kernels sum INTEGER numerators times values -- in several dimensions the product of the per-axis
// numerators, below 2^53 for any grid a plan takes, so exact in fp64 -- and scale the sum once by a coefficient the host rounded
// once: no weight is ever rounded, and an output cell is within (terms + 2) 2^-53 sum |weight value| of the exact sum.
//
//   prolong_add  fine = fl(fine + fl(coef s)), s = sum_j num(i, j) coarse[j] over the at most two coarse cells per axis around
//                the fine cell, J = floor((i + 1) M / N) and J + 1 (1-based) with numerators N - rem and rem.  A coarse index
//                outside the interior, and the second cell when rem == 0, is selected away BEFORE any arithmetic: its value is
//                replaced by 0, so nothing a halo cell holds reaches a result.  Coarse cells are read by 8-byte loads at clamped
//                interior indices; the fine side is one 16-byte load and one 16-byte store per lane and row.
//   restrict     coarse = fl(coef s), s = sum_i num(i, j) fine[i]: a gather over the fine cells with a positive numerator,
//                i + 1 in the open interval ((j) N / M, (j + 2) N / M).  N / M <= 2 on the outer axes (n_c = floor(n / 2)): at
//                most 4 cells from lo = floor(j N / M); on the innermost axis, rounded down to even, N / M <= 2.2: at most 5.  A
//                lane owns two adjacent coarse cells; their windows together fit the 8 cells from (lo & ~1), read as four
//                16-byte pieces, each loaded only if it lies inside the row's interior (both extents are even, so a piece is
//                wholly inside or wholly outside).  Rows are summed first, then scaled by the exact integer num_y num_z.
// Every operation is its own rounding (#pragma clang fp contract(off)); no atomics, a fixed order: the same call gives the same
// bits.  A workgroup is four waves; a wave walks rows, its lanes 128 cells of the row, so the row's weights are wave-uniform.
//
// The two pointwise kernels of the driver walk an interior the same way: a = fl(a - b) (the residual of a level from its extra
// sweep) and a = fl(c b) (the level-0 right-hand side).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "mg_geometry.h"

namespace lora {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerGroup = 16;  // rows a workgroup walks: four per wave

struct MgArgs {
    int n[3], nc[3];           // fine / coarse interior extents as z, y, x (2D: n[0] = nc[0] = 1)
    long frow, fplane, foff;   // fine padded array: row and plane strides, offset of interior cell (0, 0, 0), in cells
    long crow, cplane, coff;   // the same of the coarse one
    double coef;
};

// the two coarse cells around fine cell i of an axis: 0-based j and j + 1 (j may be -1), their numerators and whether each counts
struct Pair {
    int j;
    double w0, w1;
    bool v0, v1;
};
__device__ __forceinline__ Pair prolong_pair(int i, int n, int nc) {
    const int N = n + 1;
    int J, rem;
    mg_divide((long long) (i + 1) * (nc + 1), N, J, rem);  // J <= nc since i + 1 < N
    Pair r;
    r.j = J - 1;
    r.w0 = (double) (N - rem);
    r.w1 = (double) rem;
    r.v0 = J >= 1;
    r.v1 = rem != 0 && J < nc;
    return r;
}

template <bool D3>
__global__ __launch_bounds__(kThreads) void mg_prolong_add_kernel(const double *__restrict__ coarse, double *__restrict__ fine, const MgArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = 2 * ((int) blockIdx.y * 64 + lane);
    if (x >= a.n[2]) return;  // (no barrier below)
    const Pair px0 = prolong_pair(x, a.n[2], a.nc[2]), px1 = prolong_pair(x + 1, a.n[2], a.nc[2]);
    const int ncx = a.nc[2];
    // clamped coarse columns of the four loads of a row
    const int c00 = min(max(px0.j, 0), ncx - 1), c01 = min(max(px0.j + 1, 0), ncx - 1);
    const int c10 = min(max(px1.j, 0), ncx - 1), c11 = min(max(px1.j + 1, 0), ncx - 1);
    const long rows = (long) a.n[0] * a.n[1];
    const long r0 = (long) blockIdx.x * kRowsPerGroup, r1 = r0 + kRowsPerGroup < rows ? r0 + kRowsPerGroup : rows;
    for (long r = r0 + wave; r < r1; r += kThreads / 64) {
        const int z = D3 ? (int) (r / a.n[1]) : 0, y = (int) (r - (long) z * a.n[1]);
        const Pair py = prolong_pair(y, a.n[1], a.nc[1]);
        Pair pz = {0, 1.0, 0.0, true, false};
        if (D3) pz = prolong_pair(z, a.n[0], a.nc[0]);
        double *fp = fine + a.foff + z * a.fplane + y * a.frow + x;
        d2 f = *reinterpret_cast<const d2 *>(fp);
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int kz = 0; kz < (D3 ? 2 : 1); ++kz) {
            const bool vz = kz ? pz.v1 : pz.v0;
            const double wz = kz ? pz.w1 : pz.w0;
            const int cz = D3 ? min(max(pz.j + kz, 0), a.nc[0] - 1) : 0;
#pragma unroll
            for (int ky = 0; ky < 2; ++ky) {
                const bool v = vz && (ky ? py.v1 : py.v0);
                const double w = wz * (ky ? py.w1 : py.w0);  // exact: integers below 2^53
                const int cy = min(max(py.j + ky, 0), a.nc[1] - 1);
                const double *cp = coarse + a.coff + cz * a.cplane + cy * a.crow;
                const double v00 = (v && px0.v0) ? cp[c00] : 0.0, v01 = (v && px0.v1) ? cp[c01] : 0.0;
                const double v10 = (v && px1.v0) ? cp[c10] : 0.0, v11 = (v && px1.v1) ? cp[c11] : 0.0;
                s0 = s0 + (w * px0.w0) * v00;
                s0 = s0 + (w * px0.w1) * v01;
                s1 = s1 + (w * px1.w0) * v10;
                s1 = s1 + (w * px1.w1) * v11;
            }
        }
        f.x = f.x + s0 * a.coef;
        f.y = f.y + s1 * a.coef;
        *reinterpret_cast<d2 *>(fp) = f;
    }
}

template <bool D3>
__global__ __launch_bounds__(kThreads) void mg_restrict_kernel(const double *__restrict__ fine, double *__restrict__ coarse, const MgArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jx = 2 * ((int) blockIdx.y * 64 + lane);
    if (jx >= a.nc[2]) return;  // (no barrier below)
    const int nx = a.n[2];
    const int first = restrict_lo(jx, nx, a.nc[2]) & ~1;  // even: a 16-byte boundary of the row
    double wx0[8], wx1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        wx0[k] = restrict_num(first + k, jx, nx, a.nc[2]);
        wx1[k] = restrict_num(first + k, jx + 1, nx, a.nc[2]);
    }
    const long rows = (long) a.nc[0] * a.nc[1];
    const long r0 = (long) blockIdx.x * kRowsPerGroup, r1 = r0 + kRowsPerGroup < rows ? r0 + kRowsPerGroup : rows;
    for (long r = r0 + wave; r < r1; r += kThreads / 64) {
        const int jz = D3 ? (int) (r / a.nc[1]) : 0, jy = (int) (r - (long) jz * a.nc[1]);
        const int ylo = restrict_lo(jy, a.n[1], a.nc[1]), zlo = D3 ? restrict_lo(jz, a.n[0], a.nc[0]) : 0;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int kz = 0; kz < (D3 ? 4 : 1); ++kz) {
            const double wz = D3 ? restrict_num(zlo + kz, jz, a.n[0], a.nc[0]) : 1.0;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const double w = wz * restrict_num(ylo + ky, jy, a.n[1], a.nc[1]);  // exact; 0 outside the window or the interior
                if (w == 0.0) continue;                                             // wave-uniform
                const double *fp = fine + a.foff + (long) (zlo + kz) * a.fplane + (long) (ylo + ky) * a.frow + first;
                double t0 = 0.0, t1 = 0.0;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    d2 v = {0.0, 0.0};
                    if (first + 2 * m < nx) v = *reinterpret_cast<const d2 *>(fp + 2 * m);
                    // a cell without a numerator is selected away, whatever it holds
                    const double a0 = wx0[2 * m] != 0.0 ? v.x : 0.0, b0 = wx0[2 * m + 1] != 0.0 ? v.y : 0.0;
                    const double a1 = wx1[2 * m] != 0.0 ? v.x : 0.0, b1 = wx1[2 * m + 1] != 0.0 ? v.y : 0.0;
                    t0 = t0 + wx0[2 * m] * a0;
                    t0 = t0 + wx0[2 * m + 1] * b0;
                    t1 = t1 + wx1[2 * m] * a1;
                    t1 = t1 + wx1[2 * m + 1] * b1;
                }
                s0 = s0 + w * t0;
                s1 = s1 + w * t1;
            }
        }
        double *cp = coarse + a.coff + jz * a.cplane + jy * a.crow + jx;
        *reinterpret_cast<d2 *>(cp) = (d2){s0 * a.coef, s1 * a.coef};
    }
}

// OP 0: a = fl(a - b); OP 1: a = fl(c b), on the interior cells of one grid (MgArgs: its fine side)
template <int OP>
__global__ __launch_bounds__(kThreads) void mg_pointwise_kernel(double *__restrict__ ga, const double *__restrict__ gb, const MgArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = 2 * ((int) blockIdx.y * 64 + lane);
    if (x >= a.n[2]) return;
    const long rows = (long) a.n[0] * a.n[1];
    const long r0 = (long) blockIdx.x * kRowsPerGroup, r1 = r0 + kRowsPerGroup < rows ? r0 + kRowsPerGroup : rows;
    for (long r = r0 + wave; r < r1; r += kThreads / 64) {
        const long z = r / a.n[1], y = r - z * a.n[1];
        const long off = a.foff + z * a.fplane + y * a.frow + x;
        const d2 vb = *reinterpret_cast<const d2 *>(gb + off);
        d2 va;
        if (OP == 0) {
            va = *reinterpret_cast<const d2 *>(ga + off);
            va.x = va.x - vb.x;
            va.y = va.y - vb.y;
        } else {
            va.x = a.coef * vb.x;
            va.y = a.coef * vb.y;
        }
        *reinterpret_cast<d2 *>(ga + off) = va;
    }
}

bool fill(MgArgs &a, int ndim, const int *dims, const int *cdims) {
    if (ndim != 2 && ndim != 3) return false;
    mg_side(ndim, dims, a.n, a.frow, a.fplane, a.foff);
    mg_side(ndim, cdims ? cdims : dims, a.nc, a.crow, a.cplane, a.coff);
    for (int d = 0; d < 3; ++d)
        if (a.n[d] < 1 || a.nc[d] < 1) return false;
    return !(a.n[2] & 1) && !(a.nc[2] & 1);
}

dim3 grid_of(const int *n) {
    const long rows = (long) n[0] * n[1];
    return dim3((unsigned) ((rows + kRowsPerGroup - 1) / kRowsPerGroup), (unsigned) ((n[2] / 2 + 63) / 64));
}

}  // namespace

hipError_t launch_mg_restrict(int ndim, const int *dims, const int *cdims, const double *d_fine, double *d_coarse, double scale, hipStream_t s) {
    MgArgs a;
    if (!fill(a, ndim, dims, cdims)) return hipErrorInvalidValue;
    a.coef = restrict_coef(ndim, a.n, a.nc, scale);
    if (ndim == 3)
        hipLaunchKernelGGL(mg_restrict_kernel<true>, grid_of(a.nc), dim3(kThreads), 0, s, d_fine, d_coarse, a);
    else
        hipLaunchKernelGGL(mg_restrict_kernel<false>, grid_of(a.nc), dim3(kThreads), 0, s, d_fine, d_coarse, a);
    return hipGetLastError();
}

hipError_t launch_mg_prolong_add(int ndim, const int *dims, const int *cdims, const double *d_coarse, double *d_fine, hipStream_t s) {
    MgArgs a;
    if (!fill(a, ndim, dims, cdims)) return hipErrorInvalidValue;
    double den = 1.0;  // prod_a N_a: exact
    for (int d = 3 - ndim; d < 3; ++d) den *= (double) (a.n[d] + 1);
    a.coef = 1.0 / den;
    if (ndim == 3)
        hipLaunchKernelGGL(mg_prolong_add_kernel<true>, grid_of(a.n), dim3(kThreads), 0, s, d_coarse, d_fine, a);
    else
        hipLaunchKernelGGL(mg_prolong_add_kernel<false>, grid_of(a.n), dim3(kThreads), 0, s, d_coarse, d_fine, a);
    return hipGetLastError();
}

hipError_t launch_mg_sub(int ndim, const int *dims, double *d_a, const double *d_b, hipStream_t s) {
    MgArgs a;
    if (!fill(a, ndim, dims, nullptr)) return hipErrorInvalidValue;
    a.coef = 0.0;
    hipLaunchKernelGGL(mg_pointwise_kernel<0>, grid_of(a.n), dim3(kThreads), 0, s, d_a, d_b, a);
    return hipGetLastError();
}

hipError_t launch_mg_scale(int ndim, const int *dims, double *d_a, const double *d_b, double c, hipStream_t s) {
    MgArgs a;
    if (!fill(a, ndim, dims, nullptr)) return hipErrorInvalidValue;
    a.coef = c;
    hipLaunchKernelGGL(mg_pointwise_kernel<1>, grid_of(a.n), dim3(kThreads), 0, s, d_a, d_b, a);
    return hipGetLastError();
}

}  // namespace lora
