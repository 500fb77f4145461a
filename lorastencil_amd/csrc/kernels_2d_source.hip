// kernels_2d_source.hip -- TWO applications with a source term per launch, 2D fp64 (the hot path of plans that carry a source:
// lora_plan_set_source):   level 1 = S(u) + f,   out = S(level 1) + f.
//
// The tile structure is that of stencil2d_fused2_kernel (kernels_2d_fused.hip), restated here:
//   output tile        TH = 4 R1 - 6 rows x 122 columns          (61 lanes x 2 columns; j0 = 122 tx is even)
//   level-1 tile       4 R1 rows      x 128 columns  in LDS (B)  (the output tile plus a ring of 3 cells)
//   input window       4 R1 + 6 rows  x 136 columns  in LDS (A)  (starts 6 left: 16-byte aligned pieces of a row)
// B overwrites A once every wave has consumed its part of it.
//
// Arithmetic: the DIRECT taps of the plan's tap set in row-major order at both levels, always -- never the structured forms
// of rows_2d.h, whatever the plan's fused_eval says -- one fma per tap from an accumulator of 0, then ONE separate fp64
// addition of f.  That is the single source sweep's arithmetic (kernels_step.hip, EPI_SOURCE) at each level, so a launch
// equals two single source sweeps bit for bit on any data.  The tap loop is taps_row of step_epilogue.h.
//
// Boundary: level-1 cells outside the interior take no source; they are 0 under the reference boundary and the input halo
// under Dirichlet, as in stencil2d_fused2_kernel.  The source adds to interior cells only.
//
// f: at level 1 a lane owns two columns that start at an ODD padded column (the tiles are shifted by 3), so it reads its two
// cells of f with two 8-byte loads per row, each under "this cell is interior" -- no halo cell of f is loaded at all there.
// At level 2 it reads the 16-byte piece it is about to store to, under the store's predicate.  The level-1 loads of row r
// are issued six window rows before the row completes; the level-2 loads before the level's first window row.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step_epilogue.h"

namespace lora {

namespace {

constexpr int kOutW = 122;            // output columns per tile
constexpr int kMidW = 128;            // level-1 columns per tile
constexpr int kInW = 136;             // staged input columns per tile
constexpr int kInChunks = kInW / 2;   // 16-byte chunks per staged row

struct ArgsSource2 {
    const double *in, *f;
    double *out;
    int ld, m, n;
    int row_begin, row_end;
    int tiles_x, tiles_y, panel_w;
    int dirichlet;  // level-1 cells outside the interior keep the input halo value instead of 0
};

template <int TAPSET, int R1>
__global__ __launch_bounds__(256, 3) void stencil2d_source2_kernel(const ArgsSource2 a, const Taps49 W) {
    constexpr int IH = 4 * R1;            // level-1 rows
    constexpr int TH = IH - 6;            // output rows
    constexpr int AH = IH + 6;            // input rows
    constexpr int R2 = (TH + 3) / 4;      // output rows per wave (the last wave owns fewer)
    constexpr int BH = 3 * R2 + R2 + 6;   // rows of B the last wave may touch (rows >= IH are never written)
    constexpr int NCHUNK = AH * kInChunks;
    constexpr int NIT = (NCHUNK + 255) / 256;
    static_assert((BH > IH ? BH : IH) * kMidW <= AH * kInW, "B must fit in A's space");
    __shared__ __attribute__((aligned(16))) double A[AH * kInW];
    double *const B = A;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    int ty, tx;
    panel_major(xcd_contiguous(blockIdx.x, gridDim.x), a.tiles_x, a.tiles_y, a.panel_w, ty, tx);
    const int i0 = a.row_begin + ty * TH;  // first output row (interior coordinates)
    const int j0 = tx * kOutW;             // first output column

    // ---- staging: padded rows i0-2 .., padded columns j0-2 ..; pieces outside the padded array are clamped (they only feed
    //      level-1 cells outside the interior, which are replaced below) ---------------------------------------------------
    {
        d2 stage[NIT];
        const int max_row = a.m + 7, max_col = a.n + 6;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) {
                const int r = k / kInChunks, c = k - r * kInChunks;
                const int gr = min(max(i0 - 2 + r, 0), max_row);
                const int gc = min(max(j0 - 2 + 2 * c, 0), max_col);
                stage[it] = *reinterpret_cast<const d2 *>(a.in + (size_t) gr * a.ld + gc);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(A + 2 * k) = stage[it];
        }
    }
    __syncthreads();

    // ---- application 1: level-1 rows wv*R1 .. +R1-1, columns 2*lane, 2*lane+1 of B ---------------------------------------
    {
        double acc0[R1], acc1[R1], f0[R1], f1[R1];
#pragma unroll
        for (int r = 0; r < R1; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
            f0[r] = 0.0;
            f1[r] = 0.0;
        }
        const double *strip = A + (wv * R1) * kInW + 2 * lane;  // window = A columns 2*lane .. 2*lane+7
        const int jm = j0 - 3 + 2 * lane;                        // interior column of B column 2*lane
        const bool c0_in = jm >= 0 && jm < a.n;
        const bool c1_in = jm + 1 >= 0 && jm + 1 < a.n;
        d2 cur[4], nxt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const d2 *>(strip + 2 * q);
#pragma unroll
        for (int j = 0; j < R1 + 6; ++j) {
            if (j + 1 < R1 + 6) {
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kInW + 2 * q);
            }
            if (j < R1) {
                // the source cells of level-1 row j, six window rows ahead of their use: interior cells only
                const int im = i0 - 3 + wv * R1 + j;
                if (im >= 0 && im < a.m) {
                    const double *fr = a.f + (size_t) (im + 4) * a.ld + (jm + 4);
                    if (c0_in) f0[j] = fr[0];
                    if (c1_in) f1[j] = fr[1];
                }
            }
            double win[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                win[2 * q] = cur[q].x;
                win[2 * q + 1] = cur[q].y;
            }
            taps_row<TAPSET, R1>(j, win, acc0, acc1, W);
#pragma unroll
            for (int r = 0; r < R1; ++r) {
                if (j - r >= 0 && j - r < 7) asm volatile("" : "+v"(acc0[r]), "+v"(acc1[r]));
            }
            if (j >= 6) {
                // level-1 row j - 6 is complete.  Interior cells: + f.  Cells outside the interior are halo cells of the
                // level: 0 (reference boundary: "buffer 1", never written) or the caller's value (Dirichlet), which is the
                // cell itself in the input window, 3 rows / columns further in A
                const int r = j - 6;
                const int im = i0 - 3 + wv * R1 + r;
                const bool row_in = im >= 0 && im < a.m;
                double h0 = 0.0, h1 = 0.0;
                if (a.dirichlet) {
                    const double *cell = A + (wv * R1 + r + 3) * kInW + 2 * lane + 3;
                    h0 = cell[0];
                    h1 = cell[1];
                }
                acc0[r] = (row_in && c0_in) ? acc0[r] + f0[r] : h0;
                acc1[r] = (row_in && c1_in) ? acc1[r] + f1[r] : h1;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave has consumed its part of A: its space now takes the level-1 tile
#pragma unroll
        for (int r = 0; r < R1; ++r) {
            d2 v;
            v.x = acc0[r];
            v.y = acc1[r];
            *reinterpret_cast<d2 *>(B + (wv * R1 + r) * kMidW + 2 * lane) = v;
        }
    }
    __syncthreads();

    // ---- application 2: output rows wv*R2 .. +R2-1, columns 2*lane, 2*lane+1 (lanes 0..60) -------------------------------
    {
        double acc0[R2], acc1[R2];
        d2 fv[R2];
        const int col = j0 + 2 * lane;
        const bool col_ok = lane < kOutW / 2 && col < a.n;
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
            fv[r].x = 0.0;
            fv[r].y = 0.0;
            const int ro = wv * R2 + r, row = i0 + ro;
            if (col_ok && ro < TH && row < a.row_end) fv[r] = *reinterpret_cast<const d2 *>(a.f + (size_t) (row + 4) * a.ld + (col + 4));
        }
        const double *strip = B + (wv * R2) * kMidW + 2 * min(lane, 60);  // window = B columns 2*lane .. 2*lane+7
        d2 cur[4], nxt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const d2 *>(strip + 2 * q);
#pragma unroll
        for (int j = 0; j < R2 + 6; ++j) {
            if (j + 1 < R2 + 6) {
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kMidW + 2 * q);
            }
            double win[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                win[2 * q] = cur[q].x;
                win[2 * q + 1] = cur[q].y;
            }
            taps_row<TAPSET, R2>(j, win, acc0, acc1, W);
#pragma unroll
            for (int r = 0; r < R2; ++r) {
                if (j - r >= 0 && j - r < 7) asm volatile("" : "+v"(acc0[r]), "+v"(acc1[r]));
            }
            if (j >= 6) {
                const int r = j - 6;
                const int ro = wv * R2 + r;  // output row inside the tile
                const int row = i0 + ro;
                if (col_ok && ro < TH && row < a.row_end) {
                    d2 v;
                    v.x = acc0[r] + fv[r].x;
                    v.y = acc1[r] + fv[r].y;
                    *reinterpret_cast<d2 *>(a.out + (size_t) (row + 4) * a.ld + (col + 4)) = v;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int TAPSET, int R1>
hipError_t launch_source2_t(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s) {
    constexpr int TH = 4 * R1 - 6;
    ArgsSource2 a;
    a.in = in;
    a.f = static_cast<const double *>(p.source);
    a.out = out;
    a.m = p.dims[0];
    a.n = p.dims[1];
    a.ld = a.n + 8;
    a.row_begin = begin;
    a.row_end = end;
    a.tiles_x = (a.n + kOutW - 1) / kOutW;
    a.tiles_y = (end - begin + TH - 1) / TH;
    a.panel_w = a.tiles_x < 32 ? a.tiles_x : 32;  // the block -> tile map only
    a.dirichlet = p.boundary == LORA_BC_DIRICHLET;
    Taps49 w;
    for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
    const long nblocks = (long) a.tiles_x * a.tiles_y;
    if (nblocks <= 0) return hipSuccess;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((stencil2d_source2_kernel<TAPSET, R1>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

}  // namespace

// Two applications with the plan's source over the interior rows [begin, end).  The tile height follows the tap set (the
// light star the small tile, the FMA-heavier sets the tall one: the rule of the plain tile kernel); no tuning option moves it.
hipError_t launch_source2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s) {
    switch (p.tapset) {
        case TAPS2D_STAR:
            return launch_source2_t<TAPS2D_STAR, 6>(p, in, out, begin, end, s);
        case TAPS2D_DIAMOND:
            return launch_source2_t<TAPS2D_DIAMOND, 10>(p, in, out, begin, end, s);
        default:
            return launch_source2_t<TAPS2D_BOX, 10>(p, in, out, begin, end, s);
    }
}

const char *source2_kernel_name(const Plan &) { return "stencil2d_source2_kernel"; }

}  // namespace lora
