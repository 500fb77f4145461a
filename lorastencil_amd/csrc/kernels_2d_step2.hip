// kernels_2d_step2.hip -- TWO applications per launch with an update rule at both stores, 2D fp64: ONE kernel
// body, stencil2d_step2_kernel<TAPSET, R1, EPI>, whose rule EPI (step_epilogue.h) is a template parameter:
//     EPI_SOURCE        level 1 = S(in) + f,               out  = S(level 1) + f             launch_source2 (plans with a source)
//     EPI_LEAP          out1 = S(cur) + c prev,            out2 = S(out1) + c cur            launch_leapfrog2_2d
//     EPI_LEAP_SCALED   out1 = a1 S(cur) + c1 prev,        out2 = a2 S(out1) + c2 cur        launch_leapfrog2_src_2d, f == nullptr
//     EPI_LEAP_SRC      out1 = a1 (S(cur) + f) + c1 prev,  out2 = a2 (S(out1) + f) + c2 cur  launch_leapfrog2_src_2d
//
// The tile (that of stencil2d_fused2_kernel, kernels_2d_fused.hip):
//   output tile        TH = 4 R1 - 6 rows x 122 columns          (61 lanes x 2 columns; j0 = 122 tx is even)
//   level-1 tile       4 R1 rows      x 128 columns  in LDS (B)  (the output tile plus a ring of 3 cells)
//   input window       4 R1 + 6 rows  x 136 columns  in LDS (A)  (starts 6 left: 16-byte aligned pieces of a row)
// B overwrites A once every wave has consumed its part of it.  R1 = 6 for the star, 10 for the diamond and the box.
//
// Arithmetic: the DIRECT taps of the plan's tap set in row-major order at both levels, always -- never the structured forms of
// rows_2d.h, whatever the plan's fused_eval says -- one fma per tap from an accumulator of 0 (taps_row), then the rule's separate
// fp64 roundings (step_epilogue).  That is the single step's arithmetic (kernels_step.hip) at each level through the same two
// functions, so a launch equals two single steps bit for bit on any data.  Each rule is its own instantiation: "no source" is
// not "add a zero", leapfrog is not "scale by 1", and an operand a rule does not read produces no load and no live register.
//
// What EPI selects, and nothing else (the load schedule and the boundary rule; DESIGN 3.6 has the one complete table, with the
// interior values, which are the formulas above through step_epilogue<EPI>, one column per rule):
//                                  EPI_SOURCE               EPI_LEAP, EPI_LEAP_SCALED       EPI_LEAP_SRC
//   staged grid                    in                       cur                             cur
//   level-1 side loads, per row    f under "cell is         prev under "cell is within 3    prev as left, and f under
//   two 8-byte loads               interior"                of the interior"                "cell is interior"
//   ... asked for at window row    row + 0                  row + 0                         row + 4
//   level-1 cell outside the       Dirichlet: the cell      what prev holds there           what prev holds there
//   interior                       itself from A; else 0
//   level-2 side loads: 16-byte    f, all rows before       cur, in the window loop at      cur and f, as left
//   piece at the store's address   the window loop          window row = output row
//   under the store's predicate
//   out1                           none (B only)            stored by the level-2 lanes     as left
// A level-1 lane owns two columns that start at an ODD padded column (the tiles are shifted by 3), hence two 8-byte loads per
// row there and never a 16-byte one; under "cell is interior" no halo cell of f is loaded at all.  The ring is 3 and the pad 4,
// so a level-1 cell outside the interior is always inside the padded array of prev; a cell further out than 3 is never loaded
// (it feeds no stored result).  Level-1 loads are asked for six window rows before their row completes; with both prev and f
// only two rows before, which keeps the cells in flight within the register budget of three workgroups per CU (no scratch).
// The level-2 piece of cur was staged by this or a neighbouring workgroup just before: it comes from L2.
// out1 passes through the window registers: the level-1 centre cells of a lane's output piece are win[3] and win[4] of window
// row r + 3, so out1 and out2 both leave as 16-byte pieces under one predicate.
// Never written: in / cur, prev, f, and every halo cell of out / out1 / out2.  Never read: halo cells of f; anything outside
// the padded arrays (staged pieces are clamped into them and only feed level-1 cells that the boundary rule replaces).
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
    const double *f;     // the source (rules that read one)
    double *out1;        // the first new level (leapfrog rules)
    double *out2;        // the second new level; EPI_SOURCE: `out`
    double a1, c1, a2, c2;  // scale and prev / cur coefficient of each level; EPI_LEAP reads c1 alone, its c at both levels
    int ld, m, n;
    int row_begin, row_end;
    int tiles_x, tiles_y, panel_w;
    int dirichlet;  // EPI_SOURCE: level-1 cells outside the interior keep the input halo value instead of 0
};

template <int TAPSET, int R1, int EPI>
__global__ __launch_bounds__(256, 3) void stencil2d_step2_kernel(const ArgsStep2 a, const Taps49 W) {
    constexpr bool RF = epi_reads_f(EPI), RP = epi_reads_prev(EPI);
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
        constexpr int LEAD = EPI == EPI_LEAP_SRC ? 4 : 0;
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
                acc0[r] = (row_in && c0_in) ? step_epilogue<EPI>(acc0[r], f0[r], a.a1, a.c1, p0[r]) : (RP ? p0[r] : h0);
                acc1[r] = (row_in && c1_in) ? step_epilogue<EPI>(acc1[r], f1[r], a.a1, a.c1, p1[r]) : (RP ? p1[r] : h1);
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
                    v.x = step_epilogue<EPI>(acc0[r], fv[r].x, a.a2, c2, cv[r].x);
                    v.y = step_epilogue<EPI>(acc1[r], fv[r].y, a.a2, c2, cv[r].y);
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

// The rule chosen at run time -> its instantiation.  Two applications over the interior rows [begin, end).
hipError_t launch_step2(int epi, const Plan &p, const ArgsStep2 &a, int begin, int end, hipStream_t s) {
    switch (epi) {
        case EPI_SOURCE:
            return launch_step2_e<EPI_SOURCE>(p, a, begin, end, s);
        case EPI_LEAP:
            return launch_step2_e<EPI_LEAP>(p, a, begin, end, s);
        case EPI_LEAP_SCALED:
            return launch_step2_e<EPI_LEAP_SCALED>(p, a, begin, end, s);
        default:
            return launch_step2_e<EPI_LEAP_SRC>(p, a, begin, end, s);
    }
}

}  // namespace

// Two applications with the plan's source.
hipError_t launch_source2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.cur = in;
    a.f = static_cast<const double *>(p.source);
    a.out2 = out;
    return launch_step2(EPI_SOURCE, p, a, begin, end, s);
}

// Two leapfrog steps (2D plans; launch_leapfrog2 of engine.h dispatches).
hipError_t launch_leapfrog2_2d(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                               int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.prev = prev;
    a.cur = cur;
    a.out1 = out1;
    a.out2 = out2;
    a.c1 = c;
    return launch_step2(EPI_LEAP, p, a, begin, end, s);
}

// Two scaled leapfrog steps; f == nullptr: no source (2D plans; launch_leapfrog2_src of engine.h dispatches).
hipError_t launch_leapfrog2_src_2d(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                   double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.prev = prev;
    a.cur = cur;
    a.f = f;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = a1;
    a.c1 = c1;
    a.a2 = a2;
    a.c2 = c2;
    return launch_step2(f ? EPI_LEAP_SRC : EPI_LEAP_SCALED, p, a, begin, end, s);
}

// The name lora_plan_kernel_name reports for a two-application source launch: the EPI_SOURCE instantiation of
// stencil2d_step2_kernel (DESIGN 3.6 maps the reported names to the device symbols).
const char *source2_kernel_name(const Plan &) { return "stencil2d_source2_kernel"; }

}  // namespace lora
