// kernels_2d_leapfrog_src.hip -- TWO scaled leapfrog steps with a source per launch, 2D fp64 (lora_plan_step2_leapfrog_src, the
// hot path of lora_plan_run_leapfrog_src):
//     out1 = a1 (S(cur) + f) + c1 prev,   out2 = a2 (S(out1) + f) + c2 cur.
//
// The tile structure is that of stencil2d_leapfrog2_kernel (kernels_2d_leapfrog.hip), restated here:
//   output tile        TH = 4 R1 - 6 rows x 122 columns          (61 lanes x 2 columns; j0 = 122 tx is even)
//   level-1 tile       4 R1 rows      x 128 columns  in LDS (B)  (the output tile plus a ring of 3 cells)
//   input window       4 R1 + 6 rows  x 136 columns  in LDS (A)  (of cur; starts 6 left: 16-byte aligned pieces of a row)
// B overwrites A once every wave has consumed its part of it.
//
// Arithmetic: the DIRECT taps of the plan's tap set in row-major order at both levels, always -- one fma per tap from an
// accumulator of 0, then t = fl(acc + f) (no source: t = acc) and fl(fl(a t) + fl(c x)), every operation its own rounding
// (contraction off).  That is the single step's arithmetic (kernels_step.hip) at each level, through the same taps_row and
// leap_src of step_epilogue.h, so a launch equals two single steps bit for bit on any data.  "No source" is its own
// instantiation, not "add a zero".
//
// Boundary: a level-1 cell outside the interior takes the value prev holds at that cell, as in stencil2d_leapfrog2_kernel.
//
// prev at level 1: two 8-byte loads per row, each under "this cell is within 3 of the interior"; f at level 1: two 8-byte loads
// per row under "this cell is interior" (as the level-1 lanes of stencil2d_source2_kernel read it).  Without a source they are
// issued six window rows before the row completes, with one two rows before it (register budget: no scratch).  cur and f at
// level 2: the 16-byte pieces of the store's address under the store's predicate, six window rows ahead.
// out1: the level-2 lanes store it (the level-1 centre cells of a lane's output piece pass through its window registers).
// Halo cells of out1 / out2 are never written; halo cells of f are never used; prev, cur and f are never written.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step_epilogue.h"

namespace lora {

namespace {

constexpr int kOutW = 122;            // output columns per tile
constexpr int kMidW = 128;            // level-1 columns per tile
constexpr int kInW = 136;             // staged input columns per tile
constexpr int kInChunks = kInW / 2;   // 16-byte chunks per staged row

struct ArgsLeapSrc2 {
    const double *prev, *cur;
    const double *f;  // the source (nullptr: none, the !SRC instantiations)
    double *out1, *out2;
    double a1, c1, a2, c2;
    int ld, m, n;
    int row_begin, row_end;
    int tiles_x, tiles_y, panel_w;
};

template <int TAPSET, int R1, bool SRC>
__global__ __launch_bounds__(256, 3) void stencil2d_leapfrog2_src_kernel(const ArgsLeapSrc2 a, const Taps49 W) {
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

    // ---- staging of cur: padded rows i0-2 .., padded columns j0-2 ..; pieces outside the padded array are clamped (they
    //      only feed level-1 cells outside the interior, which are replaced below) --------------------------------------------
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
                stage[it] = *reinterpret_cast<const d2 *>(a.cur + (size_t) gr * a.ld + gc);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(A + 2 * k) = stage[it];
        }
    }
    __syncthreads();

    // ---- step 1: level-1 rows wv*R1 .. +R1-1, columns 2*lane, 2*lane+1 of B ----------------------------------------------
    {
        double acc0[R1], acc1[R1], p0[R1], p1[R1], f0[R1], f1[R1];
#pragma unroll
        for (int r = 0; r < R1; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
            p0[r] = 0.0;
            p1[r] = 0.0;
            f0[r] = 0.0;
            f1[r] = 0.0;
        }
        // how many window rows after row j's first use its prev (and f) cells are asked for: with a source four, which keeps the
        // cells in flight within the register budget of three workgroups per CU (no scratch); without one none, as
        // stencil2d_leapfrog2_kernel has it
        constexpr int LEAD = SRC ? 4 : 0;
        const double *strip = A + (wv * R1) * kInW + 2 * lane;  // window = A columns 2*lane .. 2*lane+7
        const int jm = j0 - 3 + 2 * lane;                        // interior column of B column 2*lane
        const bool c0_in = jm >= 0 && jm < a.n;
        const bool c1_in = jm + 1 >= 0 && jm + 1 < a.n;
        const bool c0_ring = jm >= -3 && jm < a.n + 3;           // within 3 of the interior: inside the padded row
        const bool c1_ring = jm + 1 >= -3 && jm + 1 < a.n + 3;
        d2 cur[4], nxt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const d2 *>(strip + 2 * q);
#pragma unroll
        for (int j = 0; j < R1 + 6; ++j) {
            if (j + 1 < R1 + 6) {
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kInW + 2 * q);
            }
            if (j >= LEAD && j - LEAD < R1) {
                // the prev cells of level-1 row j - LEAD, 6 - LEAD window rows ahead of their use: cells within 3 of the interior
                // only; with a source also the f cells of that row: interior cells only
                const int rr = j - LEAD;
                const int im = i0 - 3 + wv * R1 + rr;
                if (im >= -3 && im < a.m + 3) {
                    const double *pr = a.prev + (ptrdiff_t) (im + 4) * a.ld + (jm + 4);
                    if (c0_ring) p0[rr] = pr[0];
                    if (c1_ring) p1[rr] = pr[1];
                }
                if constexpr (SRC) {
                    if (im >= 0 && im < a.m) {
                        const double *fr = a.f + (ptrdiff_t) (im + 4) * a.ld + (jm + 4);
                        if (c0_in) f0[rr] = fr[0];
                        if (c1_in) f1[rr] = fr[1];
                    }
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
                // level-1 row j - 6 is complete.  Interior cells: a1 (acc + f) + c1 prev.  Cells outside the interior are halo cells of
                // the level: what prev holds there (0 here for cells further out than 3, which feed no stored result)
                const int r = j - 6;
                const int im = i0 - 3 + wv * R1 + r;
                const bool row_in = im >= 0 && im < a.m;
                acc0[r] = (row_in && c0_in) ? leap_src<SRC>(acc0[r], f0[r], a.a1, a.c1, p0[r]) : p0[r];
                acc1[r] = (row_in && c1_in) ? leap_src<SRC>(acc1[r], f1[r], a.a1, a.c1, p1[r]) : p1[r];
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

    // ---- step 2: output rows wv*R2 .. +R2-1, columns 2*lane, 2*lane+1 (lanes 0..60) ---------------------------------------
    {
        double acc0[R2], acc1[R2];
        d2 cv[R2], fv[R2], mid[R2];  // the cur and f pieces and the level-1 centre cells of each output piece
        const int col = j0 + 2 * lane;
        const bool col_ok = lane < kOutW / 2 && col < a.n;
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
            cv[r].x = 0.0;
            cv[r].y = 0.0;
            fv[r] = cv[r];
            mid[r].x = 0.0;
            mid[r].y = 0.0;
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
            if (j < R2) {
                // the cur and f pieces of output row j, six window rows ahead of its use: the store's address and predicate
                const int ro = wv * R2 + j, row = i0 + ro;
                if (col_ok && ro < TH && row < a.row_end) {
                    const size_t cell = (size_t) (row + 4) * a.ld + (col + 4);
                    cv[j] = *reinterpret_cast<const d2 *>(a.cur + cell);
                    if constexpr (SRC) fv[j] = *reinterpret_cast<const d2 *>(a.f + cell);
                }
            }
            double win[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                win[2 * q] = cur[q].x;
                win[2 * q + 1] = cur[q].y;
            }
            if (j >= 3 && j - 3 < R2) {
                // window row j is the centre row of output row j - 3: its level-1 cells are out1's piece
                mid[j - 3].x = win[3];
                mid[j - 3].y = win[4];
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
                    const size_t cell = (size_t) (row + 4) * a.ld + (col + 4);
                    d2 v;
                    v.x = leap_src<SRC>(acc0[r], fv[r].x, a.a2, a.c2, cv[r].x);
                    v.y = leap_src<SRC>(acc1[r], fv[r].y, a.a2, a.c2, cv[r].y);
                    *reinterpret_cast<d2 *>(a.out1 + cell) = mid[r];
                    *reinterpret_cast<d2 *>(a.out2 + cell) = v;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

struct Coef2 {
    double a1, c1, a2, c2;
};

template <int TAPSET, int R1, bool SRC>
hipError_t launch_leapfrog2_src_t(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                  const Coef2 &k, int begin, int end, hipStream_t s) {
    constexpr int TH = 4 * R1 - 6;
    ArgsLeapSrc2 a;
    a.prev = prev;
    a.cur = cur;
    a.f = f;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = k.a1;
    a.c1 = k.c1;
    a.a2 = k.a2;
    a.c2 = k.c2;
    a.m = p.dims[0];
    a.n = p.dims[1];
    a.ld = a.n + 8;
    a.row_begin = begin;
    a.row_end = end;
    a.tiles_x = (a.n + kOutW - 1) / kOutW;
    a.tiles_y = (end - begin + TH - 1) / TH;
    a.panel_w = a.tiles_x < 32 ? a.tiles_x : 32;  // the block -> tile map only
    Taps49 w;
    for (int t = 0; t < 49; ++t) w.w[t] = p.w[t];
    const long nblocks = (long) a.tiles_x * a.tiles_y;
    if (nblocks <= 0) return hipSuccess;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((stencil2d_leapfrog2_src_kernel<TAPSET, R1, SRC>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

template <bool SRC>
hipError_t launch_leapfrog2_src_s(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                  const Coef2 &k, int begin, int end, hipStream_t s) {
    switch (p.tapset) {
        case TAPS2D_STAR:
            return launch_leapfrog2_src_t<TAPS2D_STAR, 6, SRC>(p, prev, cur, f, out1, out2, k, begin, end, s);
        case TAPS2D_DIAMOND:
            return launch_leapfrog2_src_t<TAPS2D_DIAMOND, 10, SRC>(p, prev, cur, f, out1, out2, k, begin, end, s);
        default:
            return launch_leapfrog2_src_t<TAPS2D_BOX, 10, SRC>(p, prev, cur, f, out1, out2, k, begin, end, s);
    }
}

}  // namespace

// Two steps over the interior rows [begin, end); f == nullptr: no source.  The tile height follows the tap set as in
// launch_leapfrog2; no tuning option moves it.
hipError_t launch_leapfrog2_src(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s) {
    const Coef2 k = {a1, c1, a2, c2};
    return f ? launch_leapfrog2_src_s<true>(p, prev, cur, f, out1, out2, k, begin, end, s)
             : launch_leapfrog2_src_s<false>(p, prev, cur, nullptr, out1, out2, k, begin, end, s);
}

}  // namespace lora
