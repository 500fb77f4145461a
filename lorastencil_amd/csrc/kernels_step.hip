// kernels_step.hip -- ONE application per launch with an update rule at the store, for gfx950: on every interior
// cell of the swept range `acc` gets exactly the bits the plan's plain single sweep of `in` stores, and the epilogue EPI
// (step_epilogue.h) turns it into the stored value:
//     EPI_SOURCE        out  = fl(acc + f)                               lora_plan_set_source         (launch_source)
//     EPI_LEAP          prev = fl(acc + fl(c prev))                      lora_plan_step_leapfrog      (launch_leapfrog)
//     EPI_LEAP_SCALED   prev = fl(fl(a acc) + fl(c prev))                lora_plan_step_leapfrog_src  (launch_leapfrog_src, f == nullptr)
//     EPI_LEAP_SRC      prev = fl(fl(a fl(acc + f)) + fl(c prev))        lora_plan_step_leapfrog_src  (launch_leapfrog_src)
//     EPI_WAVE          prev = fl(fl(fl(k acc) + fl(b u)) + fl(c prev))  lora_plan_step_wave          (launch_wave; k: a grid
//                       in f's place, read as f is; u: the cell of `in` at the store's address, on chip in every family)
// Every operation after `acc` is one separate fp64 rounding, never a fused multiply-add.  Each rule is its own instantiation of
// one kernel body per family; an operand the rule does not read produces no load.
//
// Each body restates the geometry and the per-point arithmetic of the single-sweep kernel of its family -- one fma per tap
// that the resolved tap set has on, in that kernel's order, from an accumulator of 0 -- so that a step equals "plain sweep,
// then the rule's separate operations on the interior" bit for bit, non-finite values included:
//   1D                      kernels_1d.hip: two points per lane, nine taps in tap order
//   2D, even rows           stencil2d_direct_kernel at eight rows per lane: (32 + 6) x 136 window in LDS, two columns per lane,
//                           row-major tap_on order
//   3D fp64, even rows      stencil3d_stream_kernel: 16 x 128 columns, planes streamed through two LDS tiles, dz, dy, dx order
//   odd innermost extent    kernels_generic.hip: one thread per point, non-zero taps in table order
// `out` is the array stored to: the output grid (EPI_SOURCE) or `prev`, updated IN PLACE (the leapfrog rules).  A lane reads
// of `prev` and of `f` only the cells it is about to store -- the 16-byte piece (generic kernels and the 1D tail: the cell) at
// the store's address, under the store's predicate.  So no workgroup reads a cell of prev that another one writes, no halo
// cell of prev or f is read, nothing outside the padded arrays is read, `in` and `f` are never written.  The loads are issued
// ahead of the arithmetic they follow (2D: with the window's staging; 3D: as the last plane of an output plane arrives).
// The geometry is a function of dtype, extents, tap set and region alone: no tuning option moves a cell.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step_epilogue.h"

namespace lora {

namespace {

// The cell / the 16-byte piece of an operand at an offset the caller's predicate has admitted (READ false: no load).
template <bool READ>
__device__ __forceinline__ double cell_at(const double *g, long off) {
    if constexpr (READ) return g[off];
    return 0.0;
}
template <bool READ>
__device__ __forceinline__ d2 piece_at(const double *g, long off) {
    if constexpr (READ) return *reinterpret_cast<const d2 *>(g + off);
    d2 z;
    z.x = 0.0;
    z.y = 0.0;
    return z;
}

// ---- 1D ----------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void stencil1d_step_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                             const double *__restrict__ f, int begin, int end, const double sa,
                                                             const double c, const Taps9 W) {
    const long pair = (long) blockIdx.x * 256 + threadIdx.x;
    const long i = begin + 2 * pair;  // begin is even (checked on the host)
    if (i >= end) return;
    if (i + 1 < end) {
        const d2 pv = piece_at<epi_reads_prev(EPI)>(out, i + 4);
        const d2 sv = piece_at<epi_reads_f(EPI)>(f, i + 4);
        double win[10];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const d2 v = *reinterpret_cast<const d2 *>(in + i + 2 * q);
            win[2 * q] = v.x;
            win[2 * q + 1] = v.y;
        }
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            a0 = fma(W.w[t], win[t], a0);
            a1 = fma(W.w[t], win[t + 1], a1);
        }
        d2 r;
        r.x = step_epilogue<EPI>(a0, sv.x, sa, c, pv.x, win[4]);
        r.y = step_epilogue<EPI>(a1, sv.y, sa, c, pv.y, win[5]);
        *reinterpret_cast<d2 *>(out + i + 4) = r;
    } else {
        // odd tail: one point, scalar loads stay inside the padded arrays
        double a0 = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) a0 = fma(W.w[t], in[i + t], a0);
        out[i + 4] = step_epilogue<EPI>(a0, cell_at<epi_reads_f(EPI)>(f, i + 4), sa, c, cell_at<epi_reads_prev(EPI)>(out, i + 4),
                                        cell_at<epi_reads_u(EPI)>(in, i + 4));
    }
}

// ---- 2D, even innermost extent -------------------------------------------------------------------------------------------
constexpr int kTileW = 128;               // output columns per tile: 64 lanes x 2
constexpr int kLdsW = kTileW + 8;         // staged columns (halo 3 each side, widened to 4 for alignment)
constexpr int kChunksPerRow = kLdsW / 2;  // 16-byte chunks per staged row
constexpr int kRPT = 8;                   // output rows per lane: tiles of 32 x 128

struct ArgsStep2D {
    const double *in;
    double *out;      // stored to; the leapfrog rules read it first (prev)
    const double *f;  // the source (nullptr where the rule has none)
    double sa, c;
    int ld;         // padded row length n + 8
    int m, n;       // interior extents
    int row_begin;  // first interior row of this launch
    int row_end;    // one past the last interior row of this launch
    int tiles_x, tiles_y;
    int panel_w;
};

template <int TAPSET, int EPI>
__global__ __launch_bounds__(256, 3) void stencil2d_step_kernel(const ArgsStep2D a, const Taps49 W) {
    constexpr int RPT = kRPT;
    constexpr int TH = 4 * RPT;
    constexpr int LH = TH + 6;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    __shared__ __attribute__((aligned(16))) double tile[LH * kLdsW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    int ty, tx;
    panel_major(xcd_contiguous(blockIdx.x, gridDim.x), a.tiles_x, a.tiles_y, a.panel_w, ty, tx);
    const int i0 = a.row_begin + ty * TH;  // first interior row of the tile
    const int j0 = tx * kTileW;            // first interior column of the tile
    const int col = j0 + 2 * lane;

    // ---- stage the input window: padded rows i0+1 .. i0+TH+6, padded columns j0 .. j0+135; behind its loads, the pieces
    //      of prev and f this lane's stores will cover (the store's address and predicate) --------------------------------------
    d2 pv[RPT], sv[RPT];
    {
        d2 stage[NIT];
        const int max_row = a.m + 7;  // last padded row
        const int max_col = a.n + 6;  // last 16-byte chunk start in a padded row
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) {
                const int r = k / kChunksPerRow;
                const int c = k - r * kChunksPerRow;
                const int gr = min(i0 + 1 + r, max_row);
                const int gc = min(j0 + 2 * c, max_col);
                stage[it] = *reinterpret_cast<const d2 *>(a.in + (size_t) gr * a.ld + gc);
            }
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int row = i0 + wv * RPT + r;
            pv[r].x = 0.0;
            pv[r].y = 0.0;
            sv[r] = pv[r];
            if (col < a.n && row < a.row_end) {
                const size_t cell = (size_t) (row + 4) * a.ld + (col + 4);
                pv[r] = piece_at<epi_reads_prev(EPI)>(a.out, (long) cell);
                sv[r] = piece_at<epi_reads_f(EPI)>(a.f, (long) cell);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(tile + 2 * k) = stage[it];
        }
    }
    __syncthreads();

    // ---- compute: lane owns tile columns 2*lane+4, 2*lane+5 (window 2*lane .. 2*lane+9) ----------
    double acc0[RPT], acc1[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        acc0[r] = 0.0;
        acc1[r] = 0.0;
    }
    const double *strip = tile + (wv * RPT) * kLdsW + 2 * lane;
    d2 cur[5], nxt[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) cur[q] = *reinterpret_cast<const d2 *>(strip + 2 * q);
#pragma unroll
    for (int j = 0; j < RPT + 6; ++j) {
        if (j + 1 < RPT + 6) {
#pragma unroll
            for (int q = 0; q < 5; ++q) nxt[q] = *reinterpret_cast<const d2 *>(strip + (j + 1) * kLdsW + 2 * q);
        }
        double win[10];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            win[2 * q] = cur[q].x;
            win[2 * q + 1] = cur[q].y;
        }
        // input row j of the strip is tap row dy = j - r of output row r
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int dy = j - r;
            if (dy >= 0 && dy < 7) {
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) {
                    if (tap_on<TAPSET>(dy, dx)) {
                        const double wt = W.w[dy * 7 + dx];
                        acc0[r] = fma(wt, win[dx + 1], acc0[r]);
                        acc1[r] = fma(wt, win[dx + 2], acc1[r]);
                    }
                }
            }
        }
        // pin the partial sums (see stencil2d_direct_kernel)
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            if (j - r >= 0 && j - r < 7) asm volatile("" : "+v"(acc0[r]), "+v"(acc1[r]));
        }
        // output row j-6 is complete: the rule, then the store (16 bytes per lane); halo cells are never written
        if (j >= 6) {
            const int r = j - 6;
            const int row = i0 + wv * RPT + r;
            if (col < a.n && row < a.row_end) {
                // EPI_WAVE: the centre cells of the row, re-read from the tile (it is never overwritten)
                d2 u;
                u.x = 0.0;
                u.y = 0.0;
                if constexpr (epi_reads_u(EPI)) u = *reinterpret_cast<const d2 *>(tile + (wv * RPT + r + 3) * kLdsW + 2 * lane + 4);
                d2 v;
                v.x = step_epilogue<EPI>(acc0[r], sv[r].x, a.sa, a.c, pv[r].x, u.x);
                v.y = step_epilogue<EPI>(acc1[r], sv[r].y, a.sa, a.c, pv[r].y, u.y);
                *reinterpret_cast<d2 *>(a.out + (size_t) (row + 4) * a.ld + (col + 4)) = v;
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) cur[q] = nxt[q];
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int TAPSET, int EPI>
hipError_t launch_step2d(const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                         hipStream_t s) {
    constexpr int TH = 4 * kRPT;
    ArgsStep2D a;
    a.in = in;
    a.out = out;
    a.f = f;
    a.sa = sa;
    a.c = c;
    a.m = p.dims[0];
    a.n = p.dims[1];
    a.ld = a.n + 8;
    a.row_begin = begin;
    a.row_end = end;
    a.tiles_x = (a.n + kTileW - 1) / kTileW;
    a.tiles_y = (end - begin + TH - 1) / TH;
    a.panel_w = a.tiles_x < 32 ? a.tiles_x : 32;  // the block -> tile map only: which workgroup computes a tile
    Taps49 w;
    for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
    const long nblocks = (long) a.tiles_x * a.tiles_y;
    if (nblocks <= 0) return hipSuccess;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((stencil2d_step_kernel<TAPSET, EPI>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

// ---- 3D fp64, even innermost extent --------------------------------------------------------------------------------------
constexpr int kRY = 4;      // rows per lane: columns of 16 rows x 128
constexpr int kZChunk = 16; // output planes per workgroup

struct ArgsStep3D {
    const double *in;
    double *out;         // stored to; the leapfrog rules read it first (prev)
    const double *f;     // the source (nullptr where the rule has none)
    double sa, c;
    int h, m, n;         // interior extents
    int ld;              // padded row length n + 8
    long plane;          // padded plane size (m + 4) * (n + 8)
    int z_begin, z_end;  // interior plane range of this launch
    int zc;              // output planes per workgroup
    int tiles_x, tiles_y;
};

// (the four pieces of f per plane do not fit the 128 registers of four workgroups per CU beside the prev pieces: three for the
// rule that reads both, as the 2D kernel has)
template <int TAPSET, int EPI>
__global__ __launch_bounds__(256, (EPI == EPI_LEAP_SRC || EPI == EPI_WAVE) ? 3 : 4) void stencil3d_step_kernel(const ArgsStep3D a, const Taps27 W) {
    constexpr int RY = kRY;
    constexpr int TY = 4 * RY;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    __shared__ __attribute__((aligned(16))) double tile[2][LH * kLdsW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;

    const int lin = xcd_contiguous(blockIdx.x, gridDim.x);
    const int per_chunk = a.tiles_x * a.tiles_y;
    const int chunk = lin / per_chunk;
    const int rem = lin - chunk * per_chunk;
    const int ty = rem / a.tiles_x;
    const int tx = rem - ty * a.tiles_x;
    const int k0 = a.z_begin + chunk * a.zc;  // first interior plane of the chunk
    const int i0 = ty * TY;
    const int j0 = tx * kTileW;
    const int zc = min(a.zc, a.z_end - k0);   // output planes this workgroup really owns
    const int nplanes = zc + 2;               // input planes: padded k0 .. k0+zc+1

    long goff[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int k = tid + it * 256;
        const int r = k / kChunksPerRow;
        const int c = k - r * kChunksPerRow;
        const int gr = min(i0 + 1 + r, a.m + 3);  // padded rows i0+1 .. i0+TY+2
        const int gc = min(j0 + 2 * c, a.n + 6);
        goff[it] = (long) gr * a.ld + gc;
    }
    d2 stage[NIT];
    auto load_plane = [&](int p) {
        const double *src = a.in + (long) min(k0 + p, a.h + 1) * a.plane;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (NCHUNK % 256 == 0 || tid + it * 256 < NCHUNK) stage[it] = *reinterpret_cast<const d2 *>(src + goff[it]);
        }
    };
    auto write_plane = [&](int buf) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(&tile[buf][2 * k]) = stage[it];
        }
    };

    double acc0[3][RY], acc1[3][RY];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            acc0[s][r] = 0.0;
            acc1[s][r] = 0.0;
        }

    const int col = j0 + 2 * lane;
    const bool col_ok = col < a.n;
    const int strip_off = (wv * RY) * kLdsW + 2 * lane + 2;  // window = tile cols 2*lane+2 .. 2*lane+7
    const long cell_off = (long) (i0 + wv * RY + 2) * a.ld + (col + 4);
    double *const out_col = a.out + cell_off;

    load_plane(0);
    write_plane(0);
    __syncthreads();

    d2 uc[RY];  // EPI_WAVE: the centre cells of the plane consumed last (unread, and gone, in every other rule)
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        uc[r].x = 0.0;
        uc[r].y = 0.0;
    }

    auto consume = [&](int p, auto phase_tag) {
        constexpr int PHASE = decltype(phase_tag)::value;
        const bool more = p + 1 < nplanes;
        if (more) load_plane(p + 1);
        // the prev and f pieces of output plane o = p - 2, which this step completes: the store's address and predicate
        const int o = p - 2;
        const bool store_plane = o >= 0 && o < zc && col_ok;
        d2 pv[RY], sv[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            pv[r].x = 0.0;
            pv[r].y = 0.0;
            sv[r] = pv[r];
            if (store_plane && i0 + wv * RY + r < a.m) {
                const long off = (long) (k0 + o + 1) * a.plane + (long) r * a.ld;
                pv[r] = piece_at<epi_reads_prev(EPI)>(out_col, off);
                sv[r] = piece_at<epi_reads_f(EPI)>(a.f, cell_off + off);
            }
        }
        const double *strip = &tile[p & 1][strip_off];
#pragma unroll
        for (int j = 0; j < RY + 2; ++j) {
            double win[6];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const d2 v = *reinterpret_cast<const d2 *>(strip + j * kLdsW + 2 * q);
                win[2 * q] = v.x;
                win[2 * q + 1] = v.y;
            }
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                const int s = (PHASE - dz + 3) % 3;
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const int dy = j - r;
                    if (dy >= 0 && dy < 3) {
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            if (tap_on3<TAPSET>(dz, dy, dx)) {
                                const double wt = W.w[dz * 9 + dy * 3 + dx];
                                acc0[s][r] = fma(wt, win[dx + 1], acc0[s][r]);
                                acc1[s][r] = fma(wt, win[dx + 2], acc1[s][r]);
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r = 0; r < RY; ++r) asm volatile("" : "+v"(acc0[s][r]), "+v"(acc1[s][r]));

        // output plane o = p - 2 is complete (it received dz = 0, 1, 2 from planes o, o+1, o+2)
        {
            constexpr int s = (PHASE - 2 + 3) % 3;
            if (store_plane) {
                double *dst = out_col + (long) (k0 + o + 1) * a.plane;
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    if (i0 + wv * RY + r < a.m) {
                        d2 v;
                        v.x = step_epilogue<EPI>(acc0[s][r], sv[r].x, a.sa, a.c, pv[r].x, uc[r].x);
                        v.y = step_epilogue<EPI>(acc1[s][r], sv[r].y, a.sa, a.c, pv[r].y, uc[r].y);
                        *reinterpret_cast<d2 *>(dst + (long) r * a.ld) = v;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                acc0[s][r] = 0.0;
                acc1[s][r] = 0.0;
            }
        }
        // EPI_WAVE: plane p is the centre plane of the output plane the NEXT step completes.  That step's write_plane refills
        // this tile before its barrier -- a faster wave may already be overwriting it at the store -- so the lane's centre
        // pieces (strip row r + 1, window columns 2, 3) are carried in registers from here, in front of this step's barrier
        if constexpr (epi_reads_u(EPI)) {
#pragma unroll
            for (int r = 0; r < RY; ++r) uc[r] = *reinterpret_cast<const d2 *>(strip + (r + 1) * kLdsW + 2);
        }
        if (more) write_plane((p + 1) & 1);
        __syncthreads();
    };

    for (int p = 0; p < nplanes; p += 3) {
        consume(p, std::integral_constant<int, 0>{});
        if (p + 1 < nplanes) consume(p + 1, std::integral_constant<int, 1>{});
        if (p + 2 < nplanes) consume(p + 2, std::integral_constant<int, 2>{});
    }
}

template <int TAPSET, int EPI>
hipError_t launch_step3d(const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                         hipStream_t s) {
    constexpr int TY = 4 * kRY;
    ArgsStep3D a;
    a.in = in;
    a.out = out;
    a.f = f;
    a.sa = sa;
    a.c = c;
    a.h = p.dims[0];
    a.m = p.dims[1];
    a.n = p.dims[2];
    a.ld = a.n + 8;
    a.plane = (long) (a.m + 4) * (a.n + 8);
    a.z_begin = begin;
    a.z_end = end;
    a.tiles_x = (a.n + kTileW - 1) / kTileW;
    a.tiles_y = (a.m + TY - 1) / TY;
    // enough workgroups to fill 256 CUs a few times over, chunks as long as that allows: a function of the extents alone
    {
        const long tiles = (long) a.tiles_x * a.tiles_y;
        int zc = kZChunk;
        while (zc > 4 && tiles * ((a.h + zc - 1) / zc) < 2048) zc = (zc == kZChunk) ? 7 : 4;
        a.zc = zc;
    }
    const long chunks = ((long) end - begin + a.zc - 1) / a.zc;
    const long nblocks = chunks * a.tiles_x * a.tiles_y;
    if (nblocks <= 0) return hipSuccess;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    Taps27 w;
    for (int k = 0; k < 27; ++k) w.w[k] = p.w[k];
    hipLaunchKernelGGL((stencil3d_step_kernel<TAPSET, EPI>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

// ---- odd innermost extent: one thread per point ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void stencil2d_generic_step_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                                     const double *__restrict__ f, const double sa, const double cf,
                                                                     int m, int n, int row_begin, int row_end, const Taps49 W) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = row_begin + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= n || i >= row_end) return;
    const long ld = n + 8;
    const long cell = (long) (i + 4) * ld + (j + 4);
    const double pv = cell_at<epi_reads_prev(EPI)>(out, cell);
    const double sv = cell_at<epi_reads_f(EPI)>(f, cell);
    const double *c = in + cell;
    double s = 0.0;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy)
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
            const double w = W.w[dy * 7 + dx];
            if (w != 0.0) s = fma(w, c[(dy - 3) * ld + (dx - 3)], s);
        }
    out[cell] = step_epilogue<EPI>(s, sv, sa, cf, pv, cell_at<epi_reads_u(EPI)>(in, cell));
}

template <int EPI>
__global__ __launch_bounds__(256) void stencil3d_generic_step_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                                     const double *__restrict__ f, const double sa, const double cf,
                                                                     int h, int m, int n, int z_begin, int z_end, const Taps27 W) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = z_begin + blockIdx.z;
    if (j >= n || i >= m || k >= z_end) return;
    const long ld = n + 8, plane = (long) (m + 4) * ld;
    const long cell = (long) (k + 1) * plane + (long) (i + 2) * ld + (j + 4);
    const double pv = cell_at<epi_reads_prev(EPI)>(out, cell);
    const double sv = cell_at<epi_reads_f(EPI)>(f, cell);
    const double *c = in + cell;
    double s = 0.0;
#pragma unroll
    for (int dz = 0; dz < 3; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const double w = W.w[dz * 9 + dy * 3 + dx];
                if (w != 0.0) s = fma(w, c[(dz - 1) * plane + (dy - 1) * ld + (dx - 1)], s);
            }
    out[cell] = step_epilogue<EPI>(s, sv, sa, cf, pv, cell_at<epi_reads_u(EPI)>(in, cell));
}

template <int EPI>
hipError_t launch_step2d_generic(const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                                 hipStream_t s) {
    Taps49 w;
    for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
    const unsigned gx = (p.dims[1] + 63) / 64;
    const int rows = 65535 * 4;  // grid.y is limited to 65535
    for (int b = begin; b < end; b += rows) {
        const int e = b + rows < end ? b + rows : end;
        hipLaunchKernelGGL(stencil2d_generic_step_kernel<EPI>, dim3(gx, (e - b + 3) / 4), dim3(256), 0, s, in, out, f, sa, c, p.dims[0],
                           p.dims[1], b, e, w);
    }
    return hipGetLastError();
}

template <int EPI>
hipError_t launch_step3d_generic(const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                                 hipStream_t s) {
    Taps27 w;
    for (int k = 0; k < 27; ++k) w.w[k] = p.w[k];
    for (int b = begin; b < end; b += 65535) {
        const int e = b + 65535 < end ? b + 65535 : end;
        const dim3 grid((p.dims[2] + 63) / 64, (p.dims[1] + 3) / 4, e - b);
        if (grid.y > 65535u) return hipErrorInvalidValue;
        hipLaunchKernelGGL(stencil3d_generic_step_kernel<EPI>, grid, dim3(256), 0, s, in, out, f, sa, c, p.dims[0], p.dims[1], p.dims[2], b,
                           e, w);
    }
    return hipGetLastError();
}

// The family and tap set of the plan, for one rule.
template <int EPI>
hipError_t launch_step_t(const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                         hipStream_t s) {
    if (p.ndim == 1) {
        if (begin & 1) return hipErrorInvalidValue;
        Taps9 w;
        for (int t = 0; t < 9; ++t) w.w[t] = p.w[t];
        const long pairs = ((long) end - begin + 1) / 2;
        const long blocks = (pairs + 255) / 256;
        hipLaunchKernelGGL(stencil1d_step_kernel<EPI>, dim3((unsigned) blocks), dim3(256), 0, s, in, out, f, begin, end, sa, c, w);
        return hipGetLastError();
    }
    if (p.generic)
        return p.ndim == 2 ? launch_step2d_generic<EPI>(p, in, out, f, sa, c, begin, end, s)
                           : launch_step3d_generic<EPI>(p, in, out, f, sa, c, begin, end, s);
    if (p.ndim == 2) {
        switch (p.tapset) {
            case TAPS2D_DIAMOND:
                return launch_step2d<TAPS2D_DIAMOND, EPI>(p, in, out, f, sa, c, begin, end, s);
            case TAPS2D_STAR:
                return launch_step2d<TAPS2D_STAR, EPI>(p, in, out, f, sa, c, begin, end, s);
            default:
                return launch_step2d<TAPS2D_BOX, EPI>(p, in, out, f, sa, c, begin, end, s);
        }
    }
    if (p.tapset == TAPS3D_STAR) return launch_step3d<TAPS3D_STAR, EPI>(p, in, out, f, sa, c, begin, end, s);
    return launch_step3d<TAPS3D_BOX, EPI>(p, in, out, f, sa, c, begin, end, s);
}

// The rule chosen at run time -> its instantiation.  One application over [begin, end) of the outermost dimension.
hipError_t launch_step(int epi, const Plan &p, const double *in, double *out, const double *f, double sa, double c, int begin, int end,
                       hipStream_t s) {
    if (end <= begin) return hipSuccess;
    switch (epi) {
        case EPI_SOURCE:
            return launch_step_t<EPI_SOURCE>(p, in, out, f, sa, c, begin, end, s);
        case EPI_LEAP:
            return launch_step_t<EPI_LEAP>(p, in, out, f, sa, c, begin, end, s);
        case EPI_LEAP_SCALED:
            return launch_step_t<EPI_LEAP_SCALED>(p, in, out, f, sa, c, begin, end, s);
        case EPI_WAVE:
            return launch_step_t<EPI_WAVE>(p, in, out, f, sa, c, begin, end, s);
        default:
            return launch_step_t<EPI_LEAP_SRC>(p, in, out, f, sa, c, begin, end, s);
    }
}

}  // namespace

// One application with the plan's source (fp64 plans; the 2D matrix-pipe variant and bf16 never get here: lora_plan_set_source
// refuses them).
hipError_t launch_source(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s) {
    return launch_step(EPI_SOURCE, p, in, out, static_cast<const double *>(p.source), 1.0, 0.0, begin, end, s);
}

// One leapfrog step in place over `prev` (fp64 plans; the 2D matrix-pipe variant, bf16 and plans with a source never get here:
// lora_plan_step_leapfrog_region refuses them).
hipError_t launch_leapfrog(const Plan &p, const double *in, double *prev, double c, int begin, int end, hipStream_t s) {
    return launch_step(EPI_LEAP, p, in, prev, nullptr, 1.0, c, begin, end, s);
}

// One step prev <- a (S(in) + f) + c prev in place over `prev`; f == nullptr: no source (the same plans: the entries of
// chebyshev.cpp refuse the others).
hipError_t launch_leapfrog_src(const Plan &p, const double *in, double *prev, const double *f, double sa, double c, int begin, int end,
                               hipStream_t s) {
    return launch_step(f ? EPI_LEAP_SRC : EPI_LEAP_SCALED, p, in, prev, f, sa, c, begin, end, s);
}

// One step prev <- k S(in) + b in + c prev in place over `prev`, k a padded grid read like the f above (the same plans: the
// entries of leapfrog.cpp refuse the others).
hipError_t launch_wave(const Plan &p, const double *in, double *prev, const double *k, double b, double c, int begin, int end,
                       hipStream_t s) {
    return launch_step(EPI_WAVE, p, in, prev, k, b, c, begin, end, s);
}

// The kernel lora_plan_kernel_name reports for a single source sweep of this plan: the EPI_SOURCE instantiation of
// stencil{1d,2d,3d,2d_generic,3d_generic}_step_kernel (DESIGN 3.6 maps the reported names to the device symbols).
const char *source_kernel_name(const Plan &p) {
    if (p.ndim == 1) return "stencil1d_source_kernel";
    if (p.generic) return p.ndim == 2 ? "stencil2d_generic_source_kernel" : "stencil3d_generic_source_kernel";
    return p.ndim == 2 ? "stencil2d_source_kernel" : "stencil3d_source_kernel";
}

}  // namespace lora
