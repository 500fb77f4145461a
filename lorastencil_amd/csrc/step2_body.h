// step2_body.h -- the ONE body of the 2D two-step kernel, stencil2d_step2_kernel<TAPSET, R1, EPI>, and its launcher template
// (DESIGN 3.6).  Included by the translation units that instantiate it: kernels_2d_step2.hip (EPI_SOURCE, EPI_LEAP,
// EPI_LEAP_SCALED, EPI_LEAP_SRC; its header has the tile, the arithmetic and the table of what EPI selects) and
// kernels_2d_wave2.hip (EPI_WAVE).  Everything here has internal linkage: each unit owns the instantiations it asks for.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step_epilogue.h"

namespace lora {

namespace {

constexpr int kOutW = 122;            // output columns per tile
constexpr int kMidW = 128;            // level-1 columns per tile
constexpr int kInW = 136;             // staged input columns per tile
constexpr int kInChunks = kInW / 2;   // 16-byte chunks per staged row

// Fields a rule does not read stay null / 0 and unread.
struct ArgsStep2 {
    const double *prev;  // the older level (leapfrog rules)
    const double *cur;   // the staged grid: the newer level; EPI_SOURCE: `in`
    const double *f;     // the source (rules that read one); EPI_WAVE: the coefficient grid k
    double *out1;        // the first new level (leapfrog rules)
    double *out2;        // the second new level; EPI_SOURCE: `out`
    double a1, c1, a2, c2;  // scale and prev / cur coefficient of each level; EPI_LEAP reads c1 alone, its c at both levels;
                            // EPI_WAVE: a1 = a2 = b, the coefficient of the level's own centre cell
    int ld, m, n;
    int row_begin, row_end;
    int tiles_x, tiles_y, panel_w;
    int dirichlet;  // EPI_SOURCE: level-1 cells outside the interior keep the input halo value instead of 0
};

template <int TAPSET, int R1, int EPI>
__global__ __launch_bounds__(256, 3) void stencil2d_step2_kernel(const ArgsStep2 a, const Taps49 W) {
    constexpr bool RF = epi_reads_f(EPI), RP = epi_reads_prev(EPI), RU = epi_reads_u(EPI);
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

    // ---- level 1: rows wv*R1 .. +R1-1, columns 2*lane, 2*lane+1 of B -------------------------------------------------------
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
        // how many window rows after row j's first use its prev and f cells are asked for (the file header has the reason)
        constexpr int LEAD = (EPI == EPI_LEAP_SRC || EPI == EPI_WAVE) ? 4 : 0;
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
                // the prev cells of level-1 row j - LEAD, 6 - LEAD window rows ahead of their use: cells within 3 of the
                // interior only; its f cells: interior cells only
                const int rr = j - LEAD;
                const int im = i0 - 3 + wv * R1 + rr;
                if constexpr (RP) {
                    if (im >= -3 && im < a.m + 3) {
                        const double *pr = a.prev + (ptrdiff_t) (im + 4) * a.ld + (jm + 4);
                        if (c0_ring) p0[rr] = pr[0];
                        if (c1_ring) p1[rr] = pr[1];
                    }
                }
                if constexpr (RF) {
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
                // level-1 row j - 6 is complete.  Interior cells: the rule.  Cells outside the interior are halo cells of the
                // level.  Leapfrog rules: what prev holds there -- the halo of the buffer the level lives in under the in-place
                // driver (0 here for cells further out than 3, which feed no stored result).  EPI_SOURCE: 0 (reference boundary:
                // "buffer 1", never written) or the caller's value (Dirichlet), which is the cell itself in the input window,
                // 3 rows / columns further in A
                const int r = j - 6;
                const int im = i0 - 3 + wv * R1 + r;
                const bool row_in = im >= 0 && im < a.m;
                // (two spellings here are measured, DESIGN 3.6: h1 before h0 keeps the star's EPI_SOURCE at 96 registers, five
                // waves per SIMD; choosing p0[r] at the use, not copying it into h0, keeps EPI_SOURCE's unread p0, p1 out of scratch)
                double h1 = 0.0, h0 = 0.0;
                if constexpr (!RP) {
                    if (a.dirichlet) {
                        const double *cell = A + (wv * R1 + r + 3) * kInW + 2 * lane + 3;
                        h0 = cell[0];
                        h1 = cell[1];
                    }
                }
                // EPI_WAVE: the centre cells of cur, the cells the Dirichlet branch addresses (A is intact until the barrier below)
                double u1 = 0.0, u0 = 0.0;
                if constexpr (RU) {
                    const double *cell = A + (wv * R1 + r + 3) * kInW + 2 * lane + 3;
                    u0 = cell[0];
                    u1 = cell[1];
                }
                acc0[r] = (row_in && c0_in) ? step_epilogue<EPI>(acc0[r], f0[r], a.a1, a.c1, p0[r], u0) : (RP ? p0[r] : h0);
                acc1[r] = (row_in && c1_in) ? step_epilogue<EPI>(acc1[r], f1[r], a.a1, a.c1, p1[r], u1) : (RP ? p1[r] : h1);
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

    // ---- level 2: output rows wv*R2 .. +R2-1, columns 2*lane, 2*lane+1 (lanes 0..60) ---------------------------------------
    {
        double acc0[R2], acc1[R2];
        // the level-2 side operands, each the 16-byte piece at the store's address under the store's predicate, and the
        // level-1 centre cells of each output piece
        d2 cv[R2], fv[R2], mid[R2];
        const double c2 = EPI == EPI_LEAP ? a.c1 : a.c2;
        const int col = j0 + 2 * lane;
        const bool col_ok = lane < kOutW / 2 && col < a.n;
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            acc0[r] = 0.0;
            acc1[r] = 0.0;
            cv[r].x = 0.0;
            cv[r].y = 0.0;
            fv[r] = cv[r];
            mid[r] = cv[r];
        }
        if constexpr (!RP) {
            // f alone: the pieces of every output row before the level's first window row
#pragma unroll
            for (int r = 0; r < R2; ++r) {
                const int ro = wv * R2 + r, row = i0 + ro;
                if (col_ok && ro < TH && row < a.row_end) fv[r] = *reinterpret_cast<const d2 *>(a.f + (size_t) (row + 4) * a.ld + (col + 4));
            }
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
            if constexpr (RP) {
                if (j < R2) {
                    // the cur and f pieces of output row j, six window rows ahead of its use
                    const int ro = wv * R2 + j, row = i0 + ro;
                    if (col_ok && ro < TH && row < a.row_end) {
                        const size_t cell = (size_t) (row + 4) * a.ld + (col + 4);
                        cv[j] = *reinterpret_cast<const d2 *>(a.cur + cell);
                        if constexpr (RF) fv[j] = *reinterpret_cast<const d2 *>(a.f + cell);
                    }
                }
            }
            double win[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                win[2 * q] = cur[q].x;
                win[2 * q + 1] = cur[q].y;
            }
            if constexpr (RP) {
                if (j >= 3 && j - 3 < R2) {
                    // window row j is the centre row of output row j - 3: its level-1 cells are out1's piece
                    mid[j - 3].x = win[3];
                    mid[j - 3].y = win[4];
                }
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
                    v.x = step_epilogue<EPI>(acc0[r], fv[r].x, a.a2, c2, cv[r].x, mid[r].x);  // (EPI_WAVE: the level-1 centre is mid)
                    v.y = step_epilogue<EPI>(acc1[r], fv[r].y, a.a2, c2, cv[r].y, mid[r].y);
                    if constexpr (RP) *reinterpret_cast<d2 *>(a.out1 + cell) = mid[r];
                    *reinterpret_cast<d2 *>(a.out2 + cell) = v;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// `a` arrives with its operands and coefficients set; the geometry is a function of the extents, the tap set and the region.
template <int TAPSET, int R1, int EPI>
hipError_t launch_step2_t(const Plan &p, ArgsStep2 a, int begin, int end, hipStream_t s) {
    constexpr int TH = 4 * R1 - 6;
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
    hipLaunchKernelGGL((stencil2d_step2_kernel<TAPSET, R1, EPI>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

// The tile height follows the tap set (the light star the small tile, the FMA-heavier sets the tall one: the rule of the plain
// tile kernel); no tuning option moves it.
template <int EPI>
hipError_t launch_step2_e(const Plan &p, const ArgsStep2 &a, int begin, int end, hipStream_t s) {
    switch (p.tapset) {
        case TAPS2D_STAR:
            return launch_step2_t<TAPS2D_STAR, 6, EPI>(p, a, begin, end, s);
        case TAPS2D_DIAMOND:
            return launch_step2_t<TAPS2D_DIAMOND, 10, EPI>(p, a, begin, end, s);
        default:
            return launch_step2_t<TAPS2D_BOX, 10, EPI>(p, a, begin, end, s);
    }
}

}  // namespace

}  // namespace lora
