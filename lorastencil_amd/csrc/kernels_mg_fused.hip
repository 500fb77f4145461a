// kernels_mg_fused.hip -- the defect of a multigrid level restricted in the launch that computes it (host side: mg.cpp, plan
// option "mgfuse"), fp64, 2D and 3D.  One launch where lora_plan_defect into the level's free grid and
// lora_plan_mg_restrict out of it stood: the defect grid is neither written nor read back.
//
// BITS.  On every interior coarse cell the launch stores what that pair of launches stores.  The defect of a fine cell is
// d = fl(fl(acc + f) - u) (no f: fl(acc - u)), acc the FMA chain of the plan's tile family from 0 over the taps of the plan's
// resolved tapset in ascending tap order -- the 2D and 3D walks of tile_walk.h (theta2d_kernel / theta3d_kernel), restated here
// with another tile height.  The restriction is mg_restrict_kernel's (kernels_mg.hip; geometry: mg_geometry.h): per fine row the
// 8 cells from `first` in ascending order into t0, t1 of a coarse pair, then s = s + fl(w t) over ky inside kz, both ascending,
// rows with w == 0 skipped, then fl(s coef) with the coefficient the host rounded once.  Every operation behind the tap sum is
// its own rounding (#pragma clang fp contract(off)); no atomics, a fixed order: the same call gives the same bits.
//
// SHAPE.  A workgroup (four waves) owns a tile of coarse cells and the window of fine cells their numerators reach.  Per axis
// a coarse cell j gathers from floor(j N / M): on the outer axes N / M <= 2, so C coarse cells need at most 2 C + 2 fine ones;
// on the innermost axis pairs start on an even column and N / M <= 2.2, so the host picks the widest even count of coarse
// columns, at most 60, whose fine columns fit the 128 the walk computes.  Neighbouring tiles overlap by about two fine cells a
// side: a defect is computed 24 / 22 x 128 / 120 = 1.16 times in 2D, 34 / 32 x 12 / 10 x 128 / 120 = 1.36
// times in 3D.
//   1. the window of u, with the tap radius on every side, goes to LDS, clamped into the padded array as the theta kernels do;
//   2. a lane computes the defects of its two columns row by row in registers (f is loaded at interior cells alone);
//   3. the row sums of a coarse pair need 8 consecutive fine cells, which four consecutive lanes of the same wave hold: they are
//      fetched by lane shuffles, so the defect itself never reaches memory of any kind.  LDS keeps t0, t1 per fine row and coarse
//      pair, 2.2 times smaller than the defect;
//   4. behind a barrier a lane gathers a coarse pair from the t rows with the exact integer weights and stores 16 bytes.
// In 3D the workgroup walks z as tile_walk3d does, two planes of u in LDS and three planes of tap sums in registers, and
// keeps the t of the last four fine planes in a ring: a coarse plane is gathered as soon as its last fine plane is complete.
// Fine cells outside the interior have no defect: their numerators are 0 and whatever was computed for them is selected away,
// exactly as mg_restrict_kernel selects a cell without a numerator away.  The halo of the coarse grid is never touched.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "mg_geometry.h"

namespace lora {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128;             // fine columns a workgroup computes: two per lane
constexpr int kLdsW = kTileW + 8;
constexpr int kChunksPerRow = kLdsW / 2;
constexpr int kPairs = 30;              // slots of a t row: the coarse pairs of a tile, kMaxCw / 2
constexpr int kMaxCw = 60;              // coarse columns of a tile at most

// 2D: 6 fine rows per wave, 24 per tile, 11 coarse rows (2 x 10 + 3 < 24); 3D: 3 and 12, 5 coarse rows (2 x 4 + 3 < 12), which
// keeps two planes of u and four of t under a third of a CU's 160 KiB of LDS
constexpr int kRpt2 = 6, kTh2 = 4 * kRpt2, kCy2 = 11;
constexpr int kRy3 = 3, kTy3 = 4 * kRy3, kCy3 = 5;
constexpr int kCz3 = 16;                // coarse planes a 3D workgroup walks

struct FusedArgs {
    int n[3], nc[3];           // fine / coarse interior extents as z, y, x (2D: n[0] = nc[0] = 1)
    long crow, cplane, coff;   // coarse padded array: row and plane strides, offset of interior cell (0, 0, 0), in cells
    int cw;                    // coarse columns per tile: even, <= kMaxCw, its fine columns fit kTileW
    int tiles_x, tiles_y;
    double coef;
};

// What a lane needs to sum the rows of its coarse pair: the numerators of the 8 fine cells from `first` and the lane that holds
// the first two of them.
struct PairWeights {
    double w0[8], w1[8];
    int src;
    bool ok;
};
__device__ __forceinline__ PairWeights pair_weights(int lane, int jx0, int j0, int cw, int n, int nc) {
    PairWeights p;
    const int jx = jx0 + 2 * lane;
    p.ok = 2 * lane < cw && jx < nc;
    const int j = p.ok ? jx : jx0;
    const int first = restrict_lo(j, n, nc) & ~1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        p.w0[k] = restrict_num(first + k, j, n, nc);
        p.w1[k] = restrict_num(first + k, j + 1, n, nc);
    }
    p.src = min((first - j0) >> 1, 60);  // (the host's choice of cw keeps it there)
    return p;
}

// t0, t1 of the lane's coarse pair from the defects d0, d1 every lane of the wave holds for its two columns of one fine row:
// the sums of mg_restrict_kernel, term for term.  Every lane of the wave must be here.
__device__ __forceinline__ d2 row_sums(double d0, double d1, const PairWeights &p) {
#pragma clang fp contract(off)
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double vx = __shfl(d0, p.src + m), vy = __shfl(d1, p.src + m);
        // a cell without a numerator is selected away, whatever it holds
        const double a0 = p.w0[2 * m] != 0.0 ? vx : 0.0, b0 = p.w0[2 * m + 1] != 0.0 ? vy : 0.0;
        const double a1 = p.w1[2 * m] != 0.0 ? vx : 0.0, b1 = p.w1[2 * m + 1] != 0.0 ? vy : 0.0;
        t0 = t0 + p.w0[2 * m] * a0;
        t0 = t0 + p.w0[2 * m + 1] * b0;
        t1 = t1 + p.w1[2 * m] * a1;
        t1 = t1 + p.w1[2 * m + 1] * b1;
    }
    return (d2){t0, t1};
}

template <bool SRC>
__device__ __forceinline__ double defect_of(double acc, double f, double c) {
#pragma clang fp contract(off)
    if constexpr (SRC) {
        const double t = acc + f;
        return t - c;
    } else {
        return acc - c;
    }
}

// ---- 2D (tile_walk.h's 2D walk, as theta2d_kernel runs it, with six rows per lane) ---------------------------------------------
template <int TAPSET, bool SRC>
__global__ __launch_bounds__(kThreads, 3) void mg_fused2d_kernel(const double *__restrict__ in, const double *__restrict__ f,
                                                                 double *__restrict__ coarse, const FusedArgs a, const Taps49 W) {
#pragma clang fp contract(off)
    constexpr int RPT = kRpt2;
    constexpr int TH = kTh2;
    constexpr int LH = TH + 6;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    constexpr int kAhead = 4;  // window rows between the load of a row's piece of f and its use
    __shared__ __attribute__((aligned(16))) double tile[LH * kLdsW];
    __shared__ __attribute__((aligned(16))) d2 trow[TH * kPairs];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int m = a.n[1], n = a.n[2], ld = n + 8, ncy = a.nc[1], ncx = a.nc[2];
    const int ty = (int) blockIdx.x / a.tiles_x, tx = (int) blockIdx.x - ty * a.tiles_x;
    const int jy0 = ty * kCy2, jy1 = min(jy0 + kCy2, ncy), jx0 = tx * a.cw;
    const int i0 = restrict_lo(jy0, m, ncy);       // the tile's first fine row ...
    const int j0 = restrict_lo(jx0, n, ncx) & ~1;  // ... and column: even, a 16-byte boundary of the row
    const int col = j0 + 2 * lane;
    d2 fv[SRC ? RPT : 1] = {};
    // ---- stage the window of u: padded rows i0+1 .. i0+TH+6, padded columns j0 .. j0+135 (clamped into the array)
    {
        d2 stage[NIT];
        const int max_row = m + 7;
        const int max_col = n + 6;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) {
                const int r = k / kChunksPerRow;
                const int c = k - r * kChunksPerRow;
                const int gr = min(i0 + 1 + r, max_row);
                const int gc = min(j0 + 2 * c, max_col);
                stage[it] = *reinterpret_cast<const d2 *>(in + (size_t) gr * ld + gc);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = tid + it * 256;
            if (NCHUNK % 256 == 0 || k < NCHUNK) *reinterpret_cast<d2 *>(tile + 2 * k) = stage[it];
        }
    }
    const PairWeights pw = pair_weights(lane, jx0, j0, a.cw, n, ncx);
    __syncthreads();

    // ---- the defects: lane owns tile columns 2*lane+4, 2*lane+5 (window 2*lane .. 2*lane+9), wave wv rows wv*RPT ..
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
        if constexpr (SRC) {  // the piece of f of fine row j - 6 + kAhead: interior cells alone
            const int r = j - 6 + kAhead;
            if (r >= 0 && r < RPT) {
                const int row = i0 + wv * RPT + r;
                if (col < n && row < m) fv[r] = *reinterpret_cast<const d2 *>(f + (size_t) (row + 4) * ld + (col + 4));
            }
        }
        double win[10];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            win[2 * q] = cur[q].x;
            win[2 * q + 1] = cur[q].y;
        }
        // input row j of the strip is tap row dy = j - r of fine row r
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
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            if (j - r >= 0 && j - r < 7) asm volatile("" : "+v"(acc0[r]), "+v"(acc1[r]));
        }
        // fine row j-6 is complete: its centre values are window row r + 3, this lane's columns.  Every lane goes through the
        // shuffles; what a lane outside the interior computed has no numerator anywhere.
        if (j >= 6) {
            const int r = j - 6;
            const d2 c = *reinterpret_cast<const d2 *>(strip + (r + 3) * kLdsW + 4);
            const d2 fr = fv[SRC ? r : 0];
            const double d0 = defect_of<SRC>(acc0[r], fr.x, c.x), d1 = defect_of<SRC>(acc1[r], fr.y, c.y);
            const d2 t = row_sums(d0, d1, pw);
            if (pw.ok) trow[(wv * RPT + r) * kPairs + lane] = t;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) cur[q] = nxt[q];
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();

    // ---- the gather: 32 lanes per row group (30 pair slots) x 8 row groups; s = s + fl(w t) over ky ascending, rows without a numerator skipped
    const int gp = tid & 31, rg = tid >> 5;
    const int gjx = jx0 + 2 * gp;
    if (2 * gp < a.cw && gjx < ncx) {
        for (int jy = jy0 + rg; jy < jy1; jy += kThreads / 32) {
            const int ylo = restrict_lo(jy, m, ncy);
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const double w = restrict_num(ylo + ky, jy, m, ncy);  // exact; 0 outside the window or the interior
                if (w == 0.0) continue;
                const d2 t = trow[min(ylo + ky - i0, TH - 1) * kPairs + gp];
                s0 = s0 + w * t.x;
                s1 = s1 + w * t.y;
            }
            *reinterpret_cast<d2 *>(coarse + a.coff + (long) jy * a.crow + gjx) = (d2){s0 * a.coef, s1 * a.coef};
        }
    }
}

// ---- 3D (tile_walk.h's 3D walk, as theta3d_kernel runs it; a ring of four planes of t) ---------------------------------------
template <int TAPSET, bool SRC>
__global__ __launch_bounds__(kThreads, 3) void mg_fused3d_kernel(const double *__restrict__ in, const double *__restrict__ f,
                                                                 double *__restrict__ coarse, const FusedArgs a, const Taps27 W) {
#pragma clang fp contract(off)
    constexpr int RY = kRy3;
    constexpr int TY = kTy3;
    constexpr int LH = TY + 2;
    constexpr int NCHUNK = LH * kChunksPerRow;
    constexpr int NIT = (NCHUNK + 255) / 256;
    __shared__ __attribute__((aligned(16))) double tile[2][LH * kLdsW];
    __shared__ __attribute__((aligned(16))) d2 tring[4][TY * kPairs];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int h = a.n[0], m = a.n[1], n = a.n[2], ld = n + 8, ncz = a.nc[0], ncy = a.nc[1], ncx = a.nc[2];
    const long plane = (long) (m + 4) * ld;
    int b = (int) blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int ty = b % a.tiles_y, tz = b / a.tiles_y;
    const int jz0 = tz * kCz3, jz1 = min(jz0 + kCz3, ncz);
    const int jy0 = ty * kCy3, jy1 = min(jy0 + kCy3, ncy), jx0 = tx * a.cw;
    const int k0 = restrict_lo(jz0, h, ncz);                     // the first fine plane, row and column of the tile
    const int zc = min(restrict_lo(jz1 - 1, h, ncz) + 4, h) - k0;  // its fine planes
    const int i0 = restrict_lo(jy0, m, ncy);
    const int j0 = restrict_lo(jx0, n, ncx) & ~1;
    const int nplanes = zc + 2;  // input planes: padded k0 .. k0+zc+1

    long goff[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int k = tid + it * 256;
        const int r = k / kChunksPerRow;
        const int c = k - r * kChunksPerRow;
        const int gr = min(i0 + 1 + r, m + 3);  // padded rows i0+1 .. i0+TY+2
        const int gc = min(j0 + 2 * c, n + 6);
        goff[it] = (long) gr * ld + gc;
    }
    d2 stage[NIT];
    auto load_plane = [&](int p) {
        const double *src = in + (long) min(k0 + p, h + 1) * plane;
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
    const bool col_ok = col < n;
    const int strip_off = (wv * RY) * kLdsW + 2 * lane + 2;  // window = tile cols 2*lane+2 .. 2*lane+7
    const long cell0 = (long) (i0 + wv * RY + 2) * ld + (col + 4);  // this lane's first cell inside a plane
    const PairWeights pw = pair_weights(lane, jx0, j0, a.cw, n, ncx);
    // the gather's own cell: 32 lanes (30 pair slots) x 8 coarse rows (kCy3 <= 8)
    const int gp = tid & 31, gjy = jy0 + (tid >> 5), gjx = jx0 + 2 * gp;
    const bool gather_ok = 2 * gp < a.cw && gjx < ncx && gjy < jy1;
    int jz_next = jz0;

    load_plane(0);
    write_plane(0);
    __syncthreads();

    auto consume = [&](int p, auto phase_tag) {
        constexpr int PHASE = decltype(phase_tag)::value;
        const bool more = p + 1 < nplanes;
        if (more) load_plane(p + 1);
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

        // fine plane o = p - 2 of the tile is complete; its centre plane o + 1 = p - 1 is the other buffer's.  Every lane goes
        // through the shuffles (o is uniform); f is loaded at interior cells alone.
        const int o = p - 2;
        {
            constexpr int s = (PHASE - 2 + 3) % 3;
            if (o >= 0 && o < zc) {
                const double *centre = &tile[(p - 1) & 1][strip_off + kLdsW + 2];  // tile row wv*RY + r + 1, cols 2*lane+4, +5
                const long base = (long) (k0 + o + 1) * plane + cell0;
                d2 fv[SRC ? RY : 1] = {};
                if constexpr (SRC) {
#pragma unroll
                    for (int r = 0; r < RY; ++r) {
                        if (col_ok && i0 + wv * RY + r < m) fv[r] = *reinterpret_cast<const d2 *>(f + base + (long) r * ld);
                    }
                }
                d2 *trows = &tring[(k0 + o) & 3][(wv * RY) * kPairs + lane];
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const d2 c = *reinterpret_cast<const d2 *>(centre + r * kLdsW);
                    const d2 fr = fv[SRC ? r : 0];
                    const double d0 = defect_of<SRC>(acc0[s][r], fr.x, c.x), d1 = defect_of<SRC>(acc1[s][r], fr.y, c.y);
                    const d2 t = row_sums(d0, d1, pw);
                    if (pw.ok) trows[r * kPairs] = t;
                }
            }
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                acc0[s][r] = 0.0;
                acc1[s][r] = 0.0;
            }
        }
        // (as tile_walk3d: the refill goes into the buffer of plane p - 1, which other waves' epilogues may still read)
        if (p >= 2) __syncthreads();
        if (more) write_plane((p + 1) & 1);
        __syncthreads();

        // the coarse planes whose last fine plane is k0 + o: s = s + fl(w t) over ky inside kz, both ascending
        if (o >= 0 && o < zc) {
            bool any = false;
            while (jz_next < jz1 && min(restrict_lo(jz_next, h, ncz) + 3, h - 1) <= k0 + o) {
                const int jz = jz_next, zlo = restrict_lo(jz, h, ncz);
                if (gather_ok) {
                    const int ylo = restrict_lo(gjy, m, ncy);
                    double s0 = 0.0, s1 = 0.0;
#pragma unroll
                    for (int kz = 0; kz < 4; ++kz) {
                        const double wz = restrict_num(zlo + kz, jz, h, ncz);
#pragma unroll
                        for (int ky = 0; ky < 4; ++ky) {
                            const double w = wz * restrict_num(ylo + ky, gjy, m, ncy);  // exact; 0 outside the window or the interior
                            if (w == 0.0) continue;
                            const d2 t = tring[(zlo + kz) & 3][min(ylo + ky - i0, TY - 1) * kPairs + gp];
                            s0 = s0 + w * t.x;
                            s1 = s1 + w * t.y;
                        }
                    }
                    *reinterpret_cast<d2 *>(coarse + a.coff + (long) jz * a.cplane + (long) gjy * a.crow + gjx) = (d2){s0 * a.coef, s1 * a.coef};
                }
                ++jz_next;
                any = true;
            }
            if (any) __syncthreads();  // the next plane's t goes into the slot of the oldest one just read
        }
    };

    for (int p = 0; p < nplanes; p += 3) {
        consume(p, std::integral_constant<int, 0>{});
        if (p + 1 < nplanes) consume(p + 1, std::integral_constant<int, 1>{});
        if (p + 2 < nplanes) consume(p + 2, std::integral_constant<int, 2>{});
    }
}

}  // namespace

int mg_fused_tile_width(int n, int nc) {
    // the pairs of a tile of cw columns start at most ceil((cw - 2) N / M) + 1 fine columns behind the tile's first and reach 7
    // further: all inside the kTileW columns the walk computes
    const long N = n + 1, M = nc + 1;
    int cw = kMaxCw;
    while (cw > 2 && ((cw - 2) * N + M - 1) / M + 8 > kTileW - 1) cw -= 2;
    return cw;
}

hipError_t launch_mg_defect_restrict(const Plan &p, const int *cdims, const double *d_u, const double *d_f, double *d_coarse, double scale,
                                     hipStream_t s) {
    if (!has_mg(p)) return hipErrorInvalidValue;
    FusedArgs a;
    long frow, fplane, foff;
    mg_side(p.ndim, p.dims, a.n, frow, fplane, foff);
    mg_side(p.ndim, cdims, a.nc, a.crow, a.cplane, a.coff);
    for (int d = 0; d < 3; ++d)
        if (a.n[d] < 1 || a.nc[d] < 1) return hipErrorInvalidValue;
    if ((a.n[2] & 1) || (a.nc[2] & 1)) return hipErrorInvalidValue;
    a.coef = restrict_coef(p.ndim, a.n, a.nc, scale);
    a.cw = mg_fused_tile_width(a.n[2], a.nc[2]);
    a.tiles_x = (a.nc[2] + a.cw - 1) / a.cw;
    const dim3 block(kThreads);
    if (p.ndim == 2) {
        a.tiles_y = (a.nc[1] + kCy2 - 1) / kCy2;
        const dim3 grid((unsigned) ((long) a.tiles_x * a.tiles_y));
        Taps49 w;
        for (int t = 0; t < 49; ++t) w.w[t] = p.w[t];
#define LORA_FUSED2D(TS)                                                                                              \
    do {                                                                                                              \
        if (d_f)                                                                                                      \
            hipLaunchKernelGGL((mg_fused2d_kernel<TS, true>), grid, block, 0, s, d_u, d_f, d_coarse, a, w);           \
        else                                                                                                          \
            hipLaunchKernelGGL((mg_fused2d_kernel<TS, false>), grid, block, 0, s, d_u, d_f, d_coarse, a, w);          \
    } while (0)
        if (p.tapset == TAPS2D_DIAMOND)
            LORA_FUSED2D(TAPS2D_DIAMOND);
        else if (p.tapset == TAPS2D_STAR)
            LORA_FUSED2D(TAPS2D_STAR);
        else
            LORA_FUSED2D(TAPS2D_BOX);
#undef LORA_FUSED2D
    } else {
        a.tiles_y = (a.nc[1] + kCy3 - 1) / kCy3;
        const long tiles_z = (a.nc[0] + kCz3 - 1) / kCz3;
        const dim3 grid((unsigned) ((long) a.tiles_x * a.tiles_y * tiles_z));
        Taps27 w;
        for (int t = 0; t < 27; ++t) w.w[t] = p.w[t];
#define LORA_FUSED3D(TS)                                                                                              \
    do {                                                                                                              \
        if (d_f)                                                                                                      \
            hipLaunchKernelGGL((mg_fused3d_kernel<TS, true>), grid, block, 0, s, d_u, d_f, d_coarse, a, w);           \
        else                                                                                                          \
            hipLaunchKernelGGL((mg_fused3d_kernel<TS, false>), grid, block, 0, s, d_u, d_f, d_coarse, a, w);          \
    } while (0)
        if (p.tapset == TAPS3D_STAR)
            LORA_FUSED3D(TAPS3D_STAR);
        else
            LORA_FUSED3D(TAPS3D_BOX);
#undef LORA_FUSED3D
    }
    return hipGetLastError();
}

}  // namespace lora
