// kernels_3d_step2.hip -- TWO leapfrog or wave steps per launch, 3D fp64 (plan options leap3, wave3): ONE
// kernel body, stencil3d_step2_kernel<TAPSET, EPI>, whose rule EPI (step_epilogue.h) is a template parameter:
//     EPI_LEAP          out1 = S(cur) + c prev,            out2 = S(out1) + c cur            launch_leapfrog2
//     EPI_LEAP_SCALED   out1 = a1 S(cur) + c1 prev,        out2 = a2 S(out1) + c2 cur        launch_leapfrog2_src, f == nullptr
//     EPI_LEAP_SRC      out1 = a1 (S(cur) + f) + c1 prev,  out2 = a2 (S(out1) + f) + c2 cur  launch_leapfrog2_src
//     EPI_WAVE          out1 = k S(cur) + b cur + c prev,  out2 = k S(out1) + b out1 + c cur  launch_wave2_3d
//                       (k travels where f travels, b in a1 / a2, c in c1 / c2; the centre cells u: at `u1`, `u2` below)
// The 3D counterpart of kernels_2d_step2.hip.  EPI_SOURCE is not built: a 3D plan with a source runs single sweeps.
//
// Geometry: that of stencil3d_fused2_kernel (kernels_3d_fused.hip) at four rows per lane -- 256 threads, a wave = 2 row
// groups x 32 lanes, a lane owns 2 adjacent columns x 4 rows of 8 strips:
//   output tile    30 rows x 60 columns   (lanes 0..29 of a row group; tile origin J = 60 tx is even)
//   level-1 tile   32 rows x 64 columns   in LDS (B), starts 1 row / 2 columns before the output tile
//   input window   34 rows x 68 columns   in LDS (A), starts 2 rows / 4 columns before it: an even padded column
// z is streamed: a chunk of zc output planes consumes zc + 4 planes of cur; three rotating accumulator sets per level.  The
// chunk length is option fused_z_chunk with that kernel's automatic rule.  The level-1 tile starts at an even padded column
// too (J + 2), so every side operand -- prev and f at level 1, cur and f at level 2 -- is an aligned 16-byte piece.
//
// Arithmetic: scatter_row (planes_3d.h) at both levels.  A cell's accumulator starts at 0 and takes one fma per tap that
// tap_on3<TAPSET> has on, dz outermost (input planes arrive in ascending order), then dy (window rows ascending), then dx:
// exactly the chain of stencil3d_step_kernel (kernels_step.hip).  Then step_epilogue<EPI> with its separate roundings, the
// function the single step calls.  So a launch equals two single steps bit for bit on any data.  Each rule is its own
// instantiation; an operand a rule does not read produces no load and no live register.
//
// Boundary rule (the 2D rule): a level-1 cell outside the interior takes the value prev holds at that padded cell -- the
// halo of the buffer the level lives in under the in-place driver.  Only the ring of 1 cell around the interior feeds a
// stored result, and with pads of 1 / 2 / 4 the ring is inside prev's padded array; cells further out are not loaded and
// read as 0.  f is loaded under "cell is interior" alone: its halo is never read.  Level 1 is computed, not stored, on
// planes begin - 1 and end where those are interior.  Staged pieces of cur are clamped into its padded array; clamped
// pieces only feed level-1 cells the rule replaces or cells beyond the ring.
//
// Stores: out1 and out2 on interior cells of planes [begin, end), each cell once, by the workgroup that owns it in the output
// tile and chunk, as 16-byte pieces.  out1's values are the level-1 cells: the lane that publishes a level-1 piece into B
// stores the same registers to out1 where the piece lies in the workgroup's output tile (tile rows 1 .. 30, lanes 1 .. 30 of
// a row group) and chunk -- one iteration before out2 of that plane completes.  (Storing them from the level-2 window
// reads instead puts a divergent store into every window row: the compiler then wanted 32 more registers.)  The cur and f
// pieces of a level-2 cell are loaded at the store's own address under the store's predicate.
// Never written: prev, cur, f, any halo cell of out1 / out2.  Never touched: anything outside the padded arrays.
//
// One plane iteration p (as the fused kernel's):
//   (1) prefetch cur plane p + 1 into registers; ask for the prev / f pieces of level-1 plane p - 1
//   (2) level-1 scatter: read A, accumulate
//   (3) publish level-1 plane p - 1 into B and, where owned, store it to out1 (plane p - 3 of the chunk); ask for the cur / f
//       pieces of output plane p - 4
//   (4) barrier X
//   (5) level-2 scatter: read B, accumulate
//   (6) store out2 plane p - 4; write the prefetched plane into A
//   (7) barrier Y
// Every rewrite of A and B against the reads before it:
//   A is written in (6) and read in (2).  Between a wave's write (6) of iteration p and any wave's read (2) of iteration
//   p + 1 lies barrier Y of p.  Between any wave's read (2) of iteration p and a wave's write (6) of iteration p lies
//   barrier X of p: no wave passes X before every wave has finished its (2).  The first plane is written before the loop
//   behind a barrier of its own.
//   B is written in (3) and read in (5).  Between a wave's write (3) of iteration p and any wave's read (5) of p lies
//   barrier X of p.  Between any wave's read (5) of iteration p and a wave's write (3) of iteration p + 1 lies barrier Y of
//   p.  Rows 32 and 33 of B are never written; they only reach output rows 30 and 31 of the last strip, which are not stored.
// The side loads go to global memory and registers only, so they take no part in this.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "planes_3d.h"
#include "step_epilogue.h"

namespace lora {

namespace {

constexpr int kRY = 4;                       // rows per lane
constexpr int kLanesX = 32;                  // lanes per row group
constexpr int kGroups = 64 / kLanesX;        // row groups per wave
constexpr int kStrips = 4 * kGroups;         // strips per workgroup
constexpr int kMidH = kStrips * kRY;         // level-1 rows per tile
constexpr int kOutH = kMidH - 2;             // output rows per tile
constexpr int kInH = kMidH + 2;              // staged input rows (B is given the same height)
constexpr int kMidW = 2 * kLanesX;           // level-1 columns per tile
constexpr int kOutW = kMidW - 4;             // output columns per tile
constexpr int kInW = kMidW + 4;              // staged input columns (also the LDS row stride of both tiles)
constexpr int kInChunks = kInW / 2;          // 16-byte pieces per staged row
constexpr int kStageRows = 256 / kInChunks;  // whole rows staged per round of the workgroup's threads

// Fields a rule does not read stay null / 0 and unread.
struct ArgsStep23 {
    const double *prev;  // the older level
    const double *cur;   // the staged grid: the newer level
    const double *f;     // the source (EPI_LEAP_SRC)
    double *out1;        // the first new level
    double *out2;        // the second new level
    double a1, c1, a2, c2;  // scale and prev / cur coefficient of each level; EPI_LEAP reads c1 alone, its c at both levels
    int h, m, n;
    int ld;
    long plane;
    int z_begin, z_end;
    int zc;
    int tiles_x, tiles_y;
};

// A 16-byte piece at a byte offset from a base that is the same for every lane of the wave.  In-plane offsets are kept as
// unsigned 32-bit byte counts (the launcher checks that a padded plane has fewer than 2^28 cells): the load takes the base
// from scalar registers and the offset from one vector register, where a 64-bit offset per piece costs two and a
// multiplication.
__device__ __forceinline__ d2 ld16(const double *base, unsigned byte_off) {
    return *reinterpret_cast<const d2 *>(reinterpret_cast<const char *>(base) + byte_off);
}
__device__ __forceinline__ void st16(double *base, unsigned byte_off, const d2 &v) {
    *reinterpret_cast<d2 *>(reinterpret_cast<char *>(base) + byte_off) = v;
}

// The four window elements the taps read (1 .. 4; 0 and 5 exist for the alignment of the pieces and stay unread): the
// lane's own pair as one 16-byte read, its two neighbours as 8-byte reads -- two register pairs fewer than three whole pieces.
__device__ __forceinline__ void load_window(double (&win)[6], const double *row) {
    const d2 v = *reinterpret_cast<const d2 *>(row + 2);
    win[0] = 0.0;
    win[1] = row[1];
    win[2] = v.x;
    win[3] = v.y;
    win[4] = row[4];
    win[5] = 0.0;
}

// Workgroups per CU the kernel is bounded to, a function of the rule: the wave rule carries its centre cells of both levels
// across an iteration (below), sixteen register pairs the 168 registers of three workgroups do not hold.
constexpr int step23_wgs(int epi) { return epi_reads_u(epi) ? 2 : 3; }

// Three workgroups per CU (168 registers) in every leapfrog instantiation, as stencil3d_fused2_kernel has; no scratch.  What
// keeps the rule that reads both prev and f inside them: a finished accumulator slot is not cleared but reopened by its first tap
// (scatter_row's FRESH), the window reads skip the two elements no tap uses, and the lane offsets stay 32-bit (below).
template <int TAPSET, int EPI>
__global__ __launch_bounds__(256, step23_wgs(EPI)) void stencil3d_step2_kernel(const ArgsStep23 a, const Taps27 W) {
    static_assert(EPI != EPI_SOURCE, "a 3D plan with a source runs single sweeps");
    constexpr bool RF = epi_reads_f(EPI);
    constexpr bool RU = epi_reads_u(EPI);
    constexpr int RY = kRY;
    constexpr int NIT = (kInH + kStageRows - 1) / kStageRows;
    __shared__ __attribute__((aligned(16))) double A[kInH * kInW];
    __shared__ __attribute__((aligned(16))) double B[kInH * kInW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int sid = wv * kGroups + lane / kLanesX;  // strip: level-1 rows sid*RY .., output rows sid*RY ..
    const int cl = lane % kLanesX;                  // column pair inside the tile

    const int lin = xcd_contiguous(blockIdx.x, gridDim.x);
    const int per_chunk = a.tiles_x * a.tiles_y;
    const int chunk = lin / per_chunk;
    const int rem = lin - chunk * per_chunk;
    const int ty = rem / a.tiles_x;
    const int tx = rem - ty * a.tiles_x;
    const int k0 = a.z_begin + chunk * a.zc;  // first output plane (interior index) of the chunk
    const int I = ty * kOutH;                 // first output row
    const int J = tx * kOutW;                 // first output column (even)
    const int zc = min(a.zc, a.z_end - k0);
    const int nplanes = zc + 4;               // planes of cur: interior k0-2 .. k0+zc+1
    const unsigned ldb = 8u * (unsigned) a.ld;  // a padded row in bytes

    // staging: a round covers kStageRows whole tile rows, one 16-byte piece per thread (threads past them idle along), so a
    // thread's pieces lie kStageRows rows apart and their offsets come from two registers.  Tile row r / piece c <-> padded
    // row I + r, padded column J + 2c, clamped inside the array
    const int sr = tid / kInChunks;
    const int sc = tid - sr * kInChunks;
    const bool stager = sr < kStageRows;
    int stage_row = I + sr;
    unsigned stage_col = 8u * (unsigned) min(J + 2 * sc, a.n + 6);
    d2 stage[NIT];
    auto load_plane = [&](int p) {
        const double *src = a.cur + (long) min(max(k0 - 1 + p, 0), a.h + 1) * a.plane;
#pragma unroll
        for (int it = 0; it < NIT; ++it) stage[it] = ld16(src, (unsigned) min(stage_row + kStageRows * it, a.m + 3) * ldb + stage_col);
    };
    auto write_plane = [&]() {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (stager && sr + kStageRows * it < kInH) *reinterpret_cast<d2 *>(&A[(sr + kStageRows * it) * kInW + 2 * sc]) = stage[it];
        }
    };

    double a0[3][RY], a1[3][RY];  // level-1 partial sums
    double b0[3][RY], b1[3][RY];  // level-2 partial sums
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < RY; ++r) a0[s][r] = a1[s][r] = b0[s][r] = b1[s][r] = 0.0;

    // level-1 cells of this lane: interior rows I - 1 + sid*RY + r, interior columns J - 2 + 2 cl (+1).  n is even, so both
    // columns of the pair fall on the same side of every column bound
    const int col1 = J - 2 + 2 * cl;
    const bool col1_in = col1 >= 0 && col1 < a.n;
    const bool col1_ring = col1 <= a.n;  // (col1 >= -2 always) the pair is interior or holds a cell of the ring
    const int row1 = I - 1 + sid * RY;
    unsigned cell1 = 8u * (unsigned) ((row1 + 2) * a.ld + (col1 + 4));  // its padded in-plane byte offset: an even column
    // output cells: interior rows I + sid*RY + r, interior columns J + 2 cl (+1), lanes 0..29 of a row group only
    const int colo = J + 2 * cl;
    const bool colo_ok = cl < kLanesX - 2 && colo < a.n;
    const int rowo = I + sid * RY;
    unsigned cello = 8u * (unsigned) ((rowo + 2) * a.ld + (colo + 4));
    const int strip_off = (sid * RY) * kInW + 2 * cl;
    // the level-1 cells this lane owns in the output tile: it stores them to out1 as it publishes them
    const bool own1_col = cl >= 1 && cl <= kLanesX - 2 && col1 < a.n;
    const double c2 = EPI == EPI_LEAP ? a.c1 : a.c2;
    // EPI_WAVE: the centre cells u of the plane each level completes next -- the lane's own pair (win[2], win[3]) of window
    // rows 1 .. RY, taken from the scatter one iteration before the epilogue that reads them, when the tile still held that
    // plane.  Level 1: cells of cur; level 2: the level-1 cells themselves.  (Other rules: never touched, no register.)
    d2 u1[RY], u2[RY];
    if constexpr (RU) {
#pragma unroll
        for (int r = 0; r < RY; ++r) u1[r].x = u1[r].y = u2[r].x = u2[r].y = 0.0;
    }

    load_plane(0);
    write_plane();
    __syncthreads();

    auto consume = [&](int p, auto phase_tag) {
        constexpr int PH = decltype(phase_tag)::value;  // p mod 3
        constexpr int PH2 = (PH + 2) % 3;               // (p - 1) mod 3: phase of the level-1 plane finished below
        const bool more = p + 1 < nplanes;
        // (the offsets are opaque to the optimiser in every iteration: hoisted out of the loop they become one 64-bit address per
        // piece and buffer, thirteen register pairs that do not fit beside the accumulators)
        asm volatile("" : "+v"(stage_row), "+v"(stage_col), "+v"(cell1), "+v"(cello));
        if (more) load_plane(p + 1);

        // the side operands of level-1 plane z1 = k0 - 3 + p, which this iteration completes (p >= 2: the planes before it
        // feed no stored result): prev on the interior and its ring, f on the interior
        const int z1 = k0 - 3 + p;
        const bool z_in = p >= 2 && z1 >= 0 && z1 < a.h;
        const bool z_ring = p >= 2 && z1 >= -1 && z1 <= a.h;
        const bool own_z = p >= 3 && p - 3 < zc;  // z1 is a plane of this chunk
        const long pl1 = (long) min(max(z1 + 1, 0), a.h + 1) * a.plane;  // (uniform; the plane itself wherever a predicate below holds)
        d2 pv[RY], fv[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int row = row1 + r;
            pv[r].x = 0.0;
            pv[r].y = 0.0;
            fv[r] = pv[r];
            if (z_ring && col1_ring && row >= -1 && row <= a.m) pv[r] = ld16(a.prev + pl1, cell1 + r * ldb);
            if constexpr (RF) {
                if (z_in && col1_in && row >= 0 && row < a.m) fv[r] = ld16(a.f + pl1, cell1 + r * ldb);
            }
        }

        // ---- level 1: plane p of cur (interior k0-2+p) -> level-1 planes p+1, p, p-1 ----
        d2 n1[RY], n2[RY];  // (EPI_WAVE) the centre cells this iteration's scatters pass: next iteration's u1, u2
        {
            const double *strip = &A[strip_off];
#pragma unroll
            for (int j = 0; j < RY + 2; ++j) {
                double win[6];
                load_window(win, strip + j * kInW);
                scatter_row<TAPSET, RY, PH, true>(a0, a1, win, j, W);
                if constexpr (RU) {
                    if (j >= 1 && j <= RY) {
                        n1[j - 1].x = win[2];
                        n1[j - 1].y = win[3];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < RY; ++r) asm volatile("" : "+v"(a0[s][r]), "+v"(a1[s][r]));
        }
        // level-1 plane z1 is complete in slot (PH - 2) mod 3: the rule on interior cells, what prev holds elsewhere; into B,
        // and the cells of this workgroup's output tile and chunk into out1
        {
            constexpr int s = (PH + 1) % 3;
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                const bool in = z_in && col1_in && row1 + r >= 0 && row1 + r < a.m;
                d2 v = pv[r];
                if (in) {
                    if constexpr (RU) {
                        v.x = step_epilogue<EPI>(a0[s][r], fv[r].x, a.a1, a.c1, pv[r].x, u1[r].x);
                        v.y = step_epilogue<EPI>(a1[s][r], fv[r].y, a.a1, a.c1, pv[r].y, u1[r].y);
                    } else {
                        v.x = step_epilogue<EPI>(a0[s][r], fv[r].x, a.a1, a.c1, pv[r].x);
                        v.y = step_epilogue<EPI>(a1[s][r], fv[r].y, a.a1, a.c1, pv[r].y);
                    }
                }
                if constexpr (RU) u1[r] = n1[r];
                *reinterpret_cast<d2 *>(&B[strip_off + r * kInW]) = v;
                if (own_z && own1_col && sid * RY + r >= 1 && sid * RY + r <= kOutH && row1 + r < a.m) st16(a.out1 + pl1, cell1 + r * ldb, v);
            }
        }
        // the side operands of output plane o = p - 4, which this iteration completes: the store's address and predicate
        const int o = p - 4;
        const bool store2 = o >= 0 && o < zc && colo_ok;
        const long plo = (long) min(max(k0 + o + 1, 0), a.h) * a.plane;  // (uniform; the plane itself wherever store2 holds)
        d2 cv[RY], gv[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            cv[r].x = 0.0;
            cv[r].y = 0.0;
            gv[r] = cv[r];
            if (store2 && sid * RY + r < kOutH && rowo + r < a.m) {
                cv[r] = ld16(a.cur + plo, cello + r * ldb);
                if constexpr (RF) gv[r] = ld16(a.f + plo, cello + r * ldb);
            }
        }
        __syncthreads();

        // ---- level 2: level-1 plane p-1 -> output planes p, p-1, p-2 (same index convention) ----
        {
            const double *strip = &B[strip_off];
#pragma unroll
            for (int j = 0; j < RY + 2; ++j) {
                double win[6];
                load_window(win, strip + j * kInW);
                scatter_row<TAPSET, RY, PH2, true>(b0, b1, win, j, W);
                if constexpr (RU) {
                    if (j >= 1 && j <= RY) {
                        n2[j - 1].x = win[2];
                        n2[j - 1].y = win[3];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < RY; ++r) asm volatile("" : "+v"(b0[s][r]), "+v"(b1[s][r]));
        }
        // output plane k0 + p - 4 is complete in slot (PH2 - 2) mod 3 = PH
        {
            constexpr int s = PH;
            if (store2) {
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    if (sid * RY + r < kOutH && rowo + r < a.m) {
                        d2 v;
                        if constexpr (RU) {
                            v.x = step_epilogue<EPI>(b0[s][r], gv[r].x, a.a2, c2, cv[r].x, u2[r].x);
                            v.y = step_epilogue<EPI>(b1[s][r], gv[r].y, a.a2, c2, cv[r].y, u2[r].y);
                        } else {
                            v.x = step_epilogue<EPI>(b0[s][r], gv[r].x, a.a2, c2, cv[r].x);
                            v.y = step_epilogue<EPI>(b1[s][r], gv[r].y, a.a2, c2, cv[r].y);
                        }
                        st16(a.out2 + plo, cello + r * ldb, v);
                    }
                }
            }
            if constexpr (RU) {
#pragma unroll
                for (int r = 0; r < RY; ++r) u2[r] = n2[r];
            }
        }
        if (more) write_plane();
        __syncthreads();
    };

    for (int p = 0; p < nplanes; p += 3) {
        consume(p, std::integral_constant<int, 0>{});
        if (p + 1 < nplanes) consume(p + 1, std::integral_constant<int, 1>{});
        if (p + 2 < nplanes) consume(p + 2, std::integral_constant<int, 2>{});
    }
}

// `a` arrives with its operands and coefficients set; the geometry is a function of the extents, the region and option
// fused_z_chunk.
template <int TAPSET, int EPI>
hipError_t launch_step23_t(const Plan &p, ArgsStep23 a, int begin, int end, hipStream_t s) {
    a.h = p.dims[0];
    a.m = p.dims[1];
    a.n = p.dims[2];
    a.ld = a.n + 8;
    a.plane = (long) (a.m + 4) * (a.n + 8);
    if (a.plane >= (1L << 28)) return hipErrorInvalidValue;  // in-plane byte offsets in 32 bits
    a.z_begin = begin;
    a.z_end = end;
    a.tiles_x = (a.n + kOutW - 1) / kOutW;
    a.tiles_y = (a.m + kOutH - 1) / kOutH;
    // the rule of stencil3d_fused2_kernel: every chunk re-reads 4 planes, so long chunks while they still leave a few
    // workgroups per CU slot
    int zc = p.fused_z_chunk;
    if (zc <= 0) {
        zc = 32;
        const long per_plane = (long) a.tiles_x * a.tiles_y;
        while (zc > 8 && per_plane * ((end - begin + zc - 1) / zc) < 6 * 768) zc /= 2;  // 768 = 3 per CU
    }
    a.zc = zc;
    const long chunks = ((long) end - begin + a.zc - 1) / a.zc;
    const long nblocks = chunks * a.tiles_x * a.tiles_y;
    if (nblocks <= 0) return hipSuccess;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    Taps27 w;
    for (int k = 0; k < 27; ++k) w.w[k] = p.w[k];
    hipLaunchKernelGGL((stencil3d_step2_kernel<TAPSET, EPI>), dim3((unsigned) nblocks), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

template <int EPI>
hipError_t launch_step23_e(const Plan &p, const ArgsStep23 &a, int begin, int end, hipStream_t s) {
    if (p.tapset == TAPS3D_STAR) return launch_step23_t<TAPS3D_STAR, EPI>(p, a, begin, end, s);
    return launch_step23_t<TAPS3D_BOX, EPI>(p, a, begin, end, s);
}

}  // namespace

// Two leapfrog steps over the interior planes [begin, end) (plans of leapfrog_depth 2 in 3D).
hipError_t launch_leapfrog2_3d(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                               int end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    ArgsStep23 a = {};
    a.prev = prev;
    a.cur = cur;
    a.out1 = out1;
    a.out2 = out2;
    a.c1 = c;
    return launch_step23_e<EPI_LEAP>(p, a, begin, end, s);
}

// Two scaled leapfrog steps; f == nullptr: no source.
hipError_t launch_leapfrog2_src_3d(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                   double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    ArgsStep23 a = {};
    a.prev = prev;
    a.cur = cur;
    a.f = f;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = a1;
    a.c1 = c1;
    a.a2 = a2;
    a.c2 = c2;
    return f ? launch_step23_e<EPI_LEAP_SRC>(p, a, begin, end, s) : launch_step23_e<EPI_LEAP_SCALED>(p, a, begin, end, s);
}

// Two wave steps over the interior planes [begin, end) (plans of wave_depth 2 in 3D): k in f's place, b as both scales.
hipError_t launch_wave2_3d(const Plan &p, const double *prev, const double *cur, const double *k, double *out1, double *out2, double b,
                           double c, int begin, int end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    ArgsStep23 a = {};
    a.prev = prev;
    a.cur = cur;
    a.f = k;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = a.a2 = b;
    a.c1 = a.c2 = c;
    return launch_step23_e<EPI_WAVE>(p, a, begin, end, s);
}

}  // namespace lora
