// kernels_2d_wg.hip -- K = KL x S applications of a radius-3 2D stencil per launch: workgroup-wide rows, the K time
// levels pipelined over S groups of four waves ("stages").
//
// Where round 2 left the headline (counters profiles/r02_star2d1r_final2_pmc.json): the row-streaming
// kernel of kernels_2d_stream.hip runs four levels inside every wave on a PRIVATE strip of 128 input columns.  Its
// instruction stream is 88 % fp64 arithmetic, but
//   * 24 of a strip's 128 columns (19 %) are halo that every level recomputes and the launch discards;
//   * four levels of seven rotating partial rows are 112 of its 130 VGPRs: three waves per SIMD, and the occupancy
//     counter reads 2.47 because 5.9 workgroups per CU run as two ragged rounds;
//   * a wave that both loads and stores cannot tell its own loads from its stores in vmcnt, so "row r has landed" must be
//     waited for as "all but D - 1 vector-memory operations done" -- which also waits for the next row;
//   * at four sweeps per pass the launch still moves 4.46 GB in 1.24 ms = 3.6 TB/s beside a 65 % busy vector pipe.
// The matrix pipe is no way out for fp64: v_mfma_f64_16x16x4 and v_fma_f64 share one datapath on gfx950 -- issued
// together, from one wave or from two waves of a SIMD, their times ADD (tools/probes/fp64_coissue_probe.hip,
// profiles/r03_fp64_coissue_probe.txt: 64 + 81 -> 149 cycles).
//
// This kernel keeps the scatter evaluation of rows_2d.h and the ring of LDS-DMA'd input rows, and changes the ownership:
//   * A ROW belongs to the WORKGROUP: 512 input columns = one 16-byte piece per lane of four waves.  Every level shifts
//     the lane -> column map by 3 (aligned 8-wide LDS windows, as before), but now once per workgroup: a strip yields
//     512 - 6 (K - 1) output columns (482 of 512 = 94 % at K = 6; 104 of 128 = 81 % before): the ring holds the six
//     positions behind the row too, so level 1 is complete on all 512 positions and only levels 2 .. K lose six each.  A lane's window reaches 6 columns
//     into its right neighbour's piece -- also the next wave's -- so every level row goes through a workgroup-shared LDS
//     row buffer, two copies per level (written in step r, read in step r + 1), and ONE s_barrier per step orders it all.
//   * The K levels are split over S stages of KL levels: waves 4 s .. 4 s + 3 run levels s KL + 1 .. (s + 1) KL of the same
//     512 columns.  The hand-off between stages is the same row buffer every level already goes through, so a stage
//     costs nothing extra in LDS traffic, and a wave carries KL x 7 partial rows instead of K x 7: K = 6 in 2 x 3 levels
//     fits 128 VGPRs = four waves per SIMD (two 8-wave workgroups per CU) where six levels in one wave would need 190.
//   * Stage 0 issues the loads (global -> LDS, one 1 KiB piece per wave and row, D rows ahead), the last stage the stores:
//     no wave has both in its vmcnt, so "row r has landed" is exactly vmcnt(D - 1) and stores are never waited for.
//   * What a lane reads back from a level row it mostly wrote itself: pieces 0 of the window of level l are the pair the
//     same lane published as level l - 1 one step earlier.  Where both levels belong to one wave (all but the first level
//     of a stage) that pair stays in two registers per level and the window is three 16-byte LDS reads, not four
//     (K = 6: 70 instead of 84 per wave and 7 steps).  In interior steps of the nested-profile form the window of the
//     level below is fetched between the profile phase of a level (after which its own window is dead) and its fourteen
//     scatter multiply-adds, and waited for ahead of the level's ds_write: no more registers than before (116).
//   * The launch is ONE round: strips x chunks = the workgroups that are resident at once (2 per CU), every chunk as
//     long as that allows (16384^2: 32 strips x 15 chunks of 1093 rows + 2 rim strips x 16 of 1030 = 512 workgroups, 7 K - 1 = 41
//     recomputed steps each = 3.8 %).
//   * Halo semantics (as kernels_2d_stream.hip): cells of an intermediate level outside the interior are 0 at
//     odd levels and the source buffer's own halo value at even levels.  Only workgroups at the rim of the grid can see
//     such cells, and of those only the waves that hold such a column: they run a second copy of the step (EDGE) that forces them.  The halo values come straight from the
//     input array -- while fused launches run, every buffer carries buffer 0's halo (capi.cpp) -- but NOT through a load
//     the consuming wave waits for: vmcnt completes in order, so that wait would also drain the rows in flight (stage 0) or
//     the store just issued (last stage), every step (measured: rim workgroups 2.3 x slower).  Instead stage 0 fetches
//     them one step ahead (right behind the barrier of the step before), global -> LDS like the rows, into a row of halo values per even level (range-checked offsets:
//     lanes that need nothing make no memory request), where every stage picks them up behind the step's barrier.
//     Under the Dirichlet option every level keeps the source's values: a row of halo values per level (K = 4 and 2).
// Per accumulator the taps arrive in the same order as in the other fused 2D kernels: results are bit-identical to them.
//
// Replaces the reference's time-step loop 2d/gpu.cu:544-546 (K steps per pass) and kernels 2d/gpu.cu:31-273.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.h"
#include "rows_2d.h"

namespace lora {

struct ArgsWG {
    const double *in;
    double *out;
    int ld, m, n;
    int row_begin, row_end;
    int strips;  // column strips of outw output columns
    int outw;    // output columns per strip: 512 - 6 (K - 1)
    // Row chunks.  The first and the last strip ("rim strips": some of their lanes see columns outside the interior in every
    // step) run the slower EDGE loop in the waves of those lanes and get shorter chunks, so that every workgroup of the one round takes about
    // the same time: rim strips have chunks_e chunks of rows_e rows, the others chunks_i of rows_i.
    int rim;  // number of rim strips in this launch: 2, or all of them when there are fewer than three
    int rows_i, groups_i, chunks_i;
    int rows_e, groups_e, chunks_e;
    int prio_split;  // 0, or the number of workgroups dispatched first (one per CU): see the time-sliced priorities in the kernel
    int prio_shift;  // a priority slice is 2^prio_shift ticks of the 100 MHz counter
#ifdef LORA_DIAGNOSTICS
    long long *stamps;  // per workgroup: s_memrealtime at entry / exit, HW_ID, XCC_ID (tools/probes/wg_stamps.hip only)
#endif
};

namespace {

constexpr int kRowW = 512;  // doubles of a workgroup row: 4 waves x 64 lanes x 2 columns
constexpr int kBufW = 520;  // doubles of a ring slot and of a level row buffer: the last lanes' windows run 6 doubles past the row

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ring of input rows | two copies of a row per intermediate level | two copies of a row of halo values per even level | 8
// spare doubles (where the stage-0 waves that do not hold the row's end drop their tail piece)
// (DIRI: the Dirichlet option -- every intermediate level keeps the source's halo values, not only the even ones)
__host__ __device__ constexpr int wg_halo_levels(int K, bool DIRI) { return DIRI ? K - 1 : K / 2 - 1; }
__host__ __device__ constexpr int wg_lds_doubles(int K, int D, bool DIRI) { return (D + 1) * kBufW + (K - 1) * 2 * kBufW + wg_halo_levels(K, DIRI) * 2 * kRowW + 8; }

// Step r of a chunk whose first output row is i0: stage 0 consumes input row i0 - 3 K + r; level l completes its row
// i0 - 3 K - 4 l + 1 + r (a level lags 3 rows -- its radius -- plus one step of hand-off behind the level below).
// Level K is the output.  Ring slot of input row r: r mod (D + 1); row buffer of level l written in step r: copy r mod 2.
template <int EVAL, int KL, int S, int D, int WPS, bool DIRI>
__global__ __launch_bounds__(256 * S, WPS) void stencil2d_wg_kernel(const ArgsWG a, const Taps49 W, const LowRankTaps F) {
    constexpr int K = KL * S, NS = D + 1;
    static_assert(NS == 4 || NS == 2, "ring slots: a power of two");
    static_assert(K % 2 == 0, "fused launches move an even number of levels");
    __shared__ __attribute__((aligned(128))) double lds[wg_lds_doubles(K, D, DIRI)];
    double *const ring = lds;
    constexpr int RB = NS * kBufW;  // doubles of the ring: slots of kBufW, as wide as a level row
    double *const rb = lds + RB;    // rb + ((l - 1) * 2 + copy) * kBufW: row of level l

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int stage = S == 1 ? 0 : (wv >> 2);
    const int wq = wv & 3;
    const int t = wq * 64 + lane;  // this lane's column pair of the workgroup's rows
    const bool first = stage == 0;  // stage s runs levels s KL + 1 .. (s + 1) KL

    // workgroup -> (strip, chunk): rim strips first
    const int blk = xcd_contiguous(blockIdx.x, gridDim.x);
    int strip, chunk, rows, groups;
    if (blk < a.rim * a.chunks_e) {
        const int q = blk / a.chunks_e;
        chunk = blk - q * a.chunks_e;
        strip = a.rim == 2 ? (q == 0 ? 0 : a.strips - 1) : q;
        rows = a.rows_e;
        groups = a.groups_e;
    } else {
        const int b2 = blk - a.rim * a.chunks_e, ni = a.strips - a.rim;
        chunk = b2 / ni;
        strip = 1 + (b2 - chunk * ni);
        rows = a.rows_i;
        groups = a.groups_i;
    }
#ifdef LORA_DIAGNOSTICS
    if (a.stamps && threadIdx.x == 0) {
        a.stamps[4 * blockIdx.x + 0] = __builtin_amdgcn_s_memrealtime();
        a.stamps[4 * blockIdx.x + 2] = __builtin_amdgcn_s_getreg(63492) | ((long long) __builtin_amdgcn_s_getreg(63508) << 32);
        a.stamps[4 * blockIdx.x + 3] = ((long long) strip << 32) | (unsigned) chunk;
    }
#endif
    const int i0 = a.row_begin + chunk * rows;  // first output row of the chunk (interior coordinates)
    const int j0 = strip * a.outw;              // first output column of the strip
    const int row_hi = min(i0 + rows, a.row_end);
    groups = min(groups, (row_hi - i0 + 7 * K - 1 + 6) / 7);  // the last chunk of a strip may be shorter
    // Does one of THIS WAVE's 128 positions lie on a column outside the interior at some intermediate level?  (Level l
    // puts position p on column j0 - 3 K + 3 l + p.)  Only waves of rim strips, and of those only the ones that hold the
    // rim -- at 16384 columns wave 0 of the first strip and wave 3 of the last; the same for both stages.
    const bool col_edge = j0 - 3 * K + 3 + 128 * wq < 0 || j0 - 3 + 128 * wq + 127 >= a.n;

    // input: interior columns j0 - 3 K + 2 t, +1 = padded columns j0 - 3 K + 4 + 2 t, clamped into the padded array
    // (clamped pieces only feed cells outside the interior, which the EDGE steps force)
    const int gcol = min(max(j0 - 3 * K + 4 + 2 * t, 0), a.n + 6);
    // Positions 512 .. 517 of the row -- what the windows of the last three lanes reach past the workgroup's 512 columns, so
    // that level 1 is complete on all 512 positions and only levels 2 .. K lose six columns each: three 16-byte pieces,
    // clamped like gcol, fetched by lanes 0 .. 2 of wave 3 into the slot's tail.  Every stage-0 wave issues the piece
    // (one instruction stream, the same vmcnt arithmetic for all four); the other three drop theirs into the eight spare
    // doubles at the end of the LDS block, which nobody reads.  The lanes are chosen by EXEC, not by a range check: a
    // lane that is switched off writes nothing to LDS, where a lane whose address is out of range may write a zero -- into
    // the next slot, here.  (One asm statement: M0 is the compiler's, and a branch in the step is what this kernel avoids.)
    const unsigned xoff = 8u * (unsigned) min(max(j0 - 3 * K + 4 + kRowW + 2 * lane, 0), a.n + 6);
    const unsigned lds_base = (unsigned) (size_t) (__attribute__((address_space(3))) void *) lds;  // the block's LDS address
    auto issue = [&](int r) {
        const int pr = min(max(i0 - 3 * K + 4 + r, 0), a.m + 7);
        const double *const grow = a.in + (size_t) pr * a.ld;
        double *const slot = ring + (r & (NS - 1)) * kBufW;
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned tail = lds_base + 8u * (unsigned) (wq == 3 ? (r & (NS - 1)) * kBufW + kRowW : wg_lds_doubles(K, D, DIRI) - 8);
        unsigned long long keep_exec;
        unsigned keep_m0;
        asm volatile(
            "s_mov_b64 %0, exec\n\t"
            "s_mov_b32 %1, m0\n\t"
            "s_mov_b64 exec, 7\n\t"
            "s_mov_b32 m0, %4\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %2, %3\n\t"
            "s_mov_b32 m0, %1\n\t"
            "s_mov_b64 exec, %0"
            : "=&s"(keep_exec), "=&s"(keep_m0)
            : "v"(xoff), "s"(grow), "s"(tail)
            : "memory");
#endif
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *) (grow + gcol),
                                         (__attribute__((address_space(3))) void *) (slot + wq * 128), 16, 0, 0);
    };
    // stores: lanes t < outw / 2 write interior columns j0 + 2 t, +1; the descriptor's range check drops the rest
    const unsigned store_off = t < a.outw / 2 ? 16u * t : 0x80000000u;
    const unsigned row_bytes = (unsigned) (max(min(a.outw, a.n - j0), 0) * 8);
    double *const out_strip = a.out + (j0 + 4);

    // the row buffers start as zeros (the first 6 rows of every level are partial sums that nothing uses)
    for (int k = threadIdx.x; k < (K - 1) * 2 * kBufW / 2 + 4; k += 256 * S) *reinterpret_cast<d2 *>(rb + 2 * k) = (d2){0.0, 0.0};
    if (first)
#pragma unroll
        for (int k = 0; k < D; ++k) issue(k);

    // One copy of the 7-step group per (stage, EDGE): inside it the level numbers, the LDS addresses and the roles (who
    // loads, who stores) are compile-time constants and the instruction stream has NO branches -- with branches in it the
    // compiler sinks the partial-sum updates of a row towards their use, 7 steps later, and keeps every window alive
    // meanwhile (256 VGPRs and scratch instead of 128).  EDGE is chosen per group and wave: always in the waves that hold a
    // column outside the interior (col_edge: one wave per stage of a rim strip on wide grids), in all others only in the
    // few groups whose level rows lie outside the interior (first / last chunk); both copies have one barrier per step,
    // so waves of one workgroup run different copies side by side.
    auto run_stage = [&](auto stage_tag) {
        constexpr int STAGE = decltype(stage_tag)::value;
        constexpr bool FIRST = STAGE == 0;
        constexpr int LB = STAGE * KL;                             // levels LB + 1 .. LB + KL
        double pa[KL][7], pb[KL][7];  // rotating partial sums of this wave's KL levels, columns 2 t / 2 t + 1
#pragma unroll
        for (int j = 0; j < KL; ++j)
#pragma unroll
            for (int k = 0; k < 7; ++k) pa[j][k] = pb[j][k] = 0.0;
        const double *const winp = lds + 2 * t;  // + constant offsets: every window and row-buffer access of this lane
        // The pair this lane published as level LB + j one step ago, j < KL - 1: pieces 0 of the window of level LB + j + 1,
        // which the same lane evaluates -- kept in registers, so that level's window is three LDS reads, not four.  (EDGE
        // steps: the blended pair, as written.)  The first level of a stage reads another wave's row: four pieces, as does
        // level 1 from the ring.  A chunk starts with the zeros the row buffers start with.
        constexpr int NC = KL > 1 ? KL - 1 : 1;
        d2 own[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) own[j] = (d2){0.0, 0.0};
        // EDGE-only state, set up by edge_state() ahead of each EDGE range of groups and dead in between: the interior
        // groups carry none of it in registers.
        // cmask*: per intermediate level of this wave, which of the lane's two columns are interior columns (as all-ones /
        // zero masks).
        // Stage 0: per even level 2 e + 2 (of ANY stage) the byte offset of this lane's cell in a padded row when the
        // lane needs the source's value there (0x80000000 = beyond the descriptor's range: no memory request) --
        // `hcol` in rows of the interior (rim columns only), `hall` in rows outside it (every lane)
        unsigned cmask0[KL], cmask1[KL];
        constexpr int NH = wg_halo_levels(K, DIRI);  // levels with halo values: level DIRI ? e + 1 : 2 e + 2 is number e
        unsigned hcol[NH > 0 ? NH : 1], hall[NH > 0 ? NH : 1];
        auto edge_state = [&]() {
            // an opaque copy of the lane's column: two calls share no subexpression that could stay live between them
            int te = t;
            asm volatile("" : "+v"(te));
#pragma unroll
            for (int j = 0; j < KL; ++j) {
                const int c0 = j0 - 3 * K + 3 * (LB + j + 1) + 2 * te;
                cmask0[j] = (unsigned) c0 < (unsigned) a.n ? ~0u : 0u;
                cmask1[j] = (unsigned) (c0 + 1) < (unsigned) a.n ? ~0u : 0u;
                asm volatile("" : "+v"(cmask0[j]), "+v"(cmask1[j]));
            }
            if (FIRST) {
#pragma unroll
                for (int e = 0; e < NH; ++e) {
                    const int c0 = j0 - 3 * K + 3 * (DIRI ? e + 1 : 2 * e + 2) + 2 * te;
                    hall[e] = 8u * (unsigned) min(max(c0 + 4, 0), a.n + 6);
                    hcol[e] = ((unsigned) c0 < (unsigned) a.n && (unsigned) (c0 + 1) < (unsigned) a.n) ? 0x80000000u : hall[e];
                    asm volatile("" : "+v"(hcol[e]), "+v"(hall[e]));
                }
            }
        };
        double *const hb = lds + RB + (K - 1) * 2 * kBufW;  // hb + (e * 2 + copy) * kRowW: halo values of level 2 e + 2

        auto step = [&](const int r, auto phase_tag, auto edge_tag) {
            constexpr int P = decltype(phase_tag)::value;  // r mod 7: logical row 0 (the one completed now) is acc[P]
            constexpr bool EDGE = decltype(edge_tag)::value;
            const int par = r & 1;
            // "input row r has landed": the D - 1 younger rows, two loads each (the row piece and the tail piece), may be
            // outstanding (S > 1: stage 0 has no stores in its vmcnt; S == 1: as in kernels_2d_stream.hip, the interleaved
            // stores only make the wait stricter).  EDGE: this step's halo values were issued in the previous step, BEFORE
            // its row: one younger row.
            if (FIRST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(EDGE && NH > 0 ? 2 : 2 * (D - 1)) : "memory");
            // one barrier per step: behind it every wave's piece of input row r (and of this step's halo values) and every
            // level row of step r - 1 is visible, and nobody still reads what this step overwrites (ring slot of row r - 1,
            // row copies of step r - 2, halo values of step r - 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (FIRST && EDGE) {
                // Halo values of step r + 1, every level that keeps any: this wave's 128 columns of them, into the copy that
                // step r does not read (step r - 1 did, and every wave is past it).  Issued right behind the barrier they
                // have the whole step to arrive; in vmcnt they stand in front of this step's row.
#pragma unroll
                for (int e = 0; e < NH; ++e) {
                    const int row1 = i0 - 3 * K - 4 * (DIRI ? e + 1 : 2 * e + 2) + 1 + (r + 1);
                    const int pr = min(max(row1 + 4, 0), a.m + 7);
                    const __amdgpu_buffer_rsrc_t hsrc = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<double *>(a.in) + (size_t) pr * a.ld, 0, (unsigned) a.ld * 8u, 0x00020000);
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass does not know this builtin and then drops the kernel's stub without a word)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        hsrc, (__attribute__((address_space(3))) void *) (hb + (e * 2 + (par ^ 1)) * kRowW + wq * 128), 16,
                        (unsigned) row1 < (unsigned) a.m ? hcol[e] : hall[e], 0, 0, 0);
#else
                    (void) hsrc;
                    (void) hb;
#endif
                }
                // (the compiler does not know that these overwrite LDS: nothing of the step may rise above them)
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
            const int cur = par * kBufW, prev = kBufW - cur;  // this step's / the previous step's copy of a level row
            // the window of this wave's level number jj (global level LB + jj + 1): the pair the lane holds + three pieces, or
            // four pieces of another wave's row / of the ring
            auto window = [&](const int jj, double (&w)[8]) {
                const int lw = LB + jj + 1;
                const double *const src = lw == 1 ? winp + (r & (NS - 1)) * kBufW : winp + RB + (lw - 2) * 2 * kBufW + prev;
                const bool own_pair = jj >= 1;  // the level below is this wave's: its pair is in `own`
                if (own_pair) {
                    w[0] = own[jj >= 1 ? jj - 1 : 0].x;
                    w[1] = own[jj >= 1 ? jj - 1 : 0].y;
                }
#pragma unroll
                for (int q = own_pair ? 1 : 0; q < 4; ++q) {
                    const d2 w2 = *reinterpret_cast<const d2 *>(src + 2 * q);
                    w[2 * q] = w2.x;
                    w[2 * q + 1] = w2.y;
                }
            };
            // Interior steps of the nested-profile form fetch the window of the level below between the two phases of a level
            // (rows_2d.h).  Not the EDGE steps: they are where the registers run out; not the other forms:
            // their windows stay live through the whole level.
            constexpr bool kEarly = !EDGE && EVAL == EVAL_NEST;
            double win[8];
#pragma unroll
            for (int j = KL - 1; j >= 0; --j) {
                const int l = LB + j + 1;                    // global level (a constant after unrolling)
                const int row = i0 - 3 * K - 4 * l + 1 + r;  // the row this level completes now
                const bool to_global = l == K;               // level K is the output
                if (!kEarly || j == KL - 1) window(j, win);  // (kEarly: the level above fetched it)
                // EDGE: what this lane's cells are forced to when they lie outside the interior
                d2 h = {0.0, 0.0};
                if (EDGE && !to_global && ((l & 1) == 0 || DIRI))
                    h = *reinterpret_cast<const d2 *>(winp + RB + (K - 1) * 2 * kBufW + ((DIRI ? l - 1 : l / 2 - 1) * 2 + par) * kRowW);
                // the newest logical row (6) starts from zero: stated here, so that the zero is an inline constant of its
                // first multiply-add and not a register carried around the loop
                pa[j][(P + 6) % 7] = 0.0;
                pb[j][(P + 6) % 7] = 0.0;
                if constexpr (kEarly) {
                    // the profiles use the window up; the pieces of the next level's window travel while this level's
                    // fourteen scatter multiply-adds issue
                    double t0[4], t1[4];
                    nest_profiles(win, t0, t1, F);
                    __builtin_amdgcn_sched_barrier(0);
                    if (j > 0) window(j - 1, win);
                    __builtin_amdgcn_sched_barrier(0);
                    nest_scatter<7, P>(6, t0, t1, pa[j], pb[j], F);
                    // a use of the fetched pieces AHEAD of this level's ds_write: the wait for them lands here and is a plain
                    // lgkmcnt(0) over reads alone -- behind the write the compiler's count would wait for the write as well
                    if (j > 0) {
                        if (j - 1 == 0) asm volatile("" ::"v"(win[0]), "v"(win[1]));
                        asm volatile("" ::"v"(win[2]), "v"(win[3]), "v"(win[4]), "v"(win[5]), "v"(win[6]), "v"(win[7]));
                    }
                } else {
                    apply_row<EVAL, 7, P>(6, win, pa[j], pb[j], W, F);
                }
                d2 v;
                v.x = pa[j][P];
                v.y = pb[j][P];
                if (to_global) {
                    const bool live = row >= i0 && row < row_hi;
                    const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(
                        out_strip + (size_t) (max(row, 0) + 4) * a.ld, 0, live ? row_bytes : 0u, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), dst, store_off, 0, kStoreNT);
                } else {
                    if (EDGE) {
                        // v = inside ? v : h as a bitwise blend under integer masks the compiler cannot see through: from a
                        // select it builds a branch around the row's last multiply-add, and with branches in the step the
                        // register blow-up is back
                        const unsigned rmask = (unsigned) row < (unsigned) a.m ? ~0u : 0u;
                        const unsigned m0 = cmask0[j] & rmask, m1 = cmask1[j] & rmask;
                        const u32x4 vb = __builtin_bit_cast(u32x4, v), hb4 = __builtin_bit_cast(u32x4, h);
                        u32x4 o;
                        o.x = (vb.x & m0) | (hb4.x & ~m0);
                        o.y = (vb.y & m0) | (hb4.y & ~m0);
                        o.z = (vb.z & m1) | (hb4.z & ~m1);
                        o.w = (vb.w & m1) | (hb4.w & ~m1);
                        v = __builtin_bit_cast(d2, o);
                    }
                    *reinterpret_cast<d2 *>(const_cast<double *>(winp) + RB + (l - 1) * 2 * kBufW + cur) = v;
                    // what level l + 1 of this wave reads in the next step (it ran before this level in this step, on the
                    // pair of the step before)
                    if (j < KL - 1) own[j < KL - 1 ? j : 0] = v;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // The compiler does not know that the LDS-DMAs below overwrite LDS; nothing of this step may sink below them
            // (row r + D goes where row r - 1 was: every wave finished with that one before this step's barrier)
            asm volatile("" ::: "memory");
            if (FIRST) issue(r + D);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto group = [&](const int r0, auto edge_tag) {
            step(r0 + 0, std::integral_constant<int, 0>{}, edge_tag);
            step(r0 + 1, std::integral_constant<int, 1>{}, edge_tag);
            step(r0 + 2, std::integral_constant<int, 2>{}, edge_tag);
            step(r0 + 3, std::integral_constant<int, 3>{}, edge_tag);
            step(r0 + 4, std::integral_constant<int, 4>{}, edge_tag);
            step(r0 + 5, std::integral_constant<int, 5>{}, edge_tag);
            step(r0 + 6, std::integral_constant<int, 6>{}, edge_tag);
        };

        // Rows the workgroup's intermediate levels complete in group g: [lo0 + 7 g, hi0 + 7 g].  Groups [0, g1) and
        // [g2, groups) have rows outside the interior (first / last chunk only); waves with col_edge run EDGE throughout.  The second
        // EDGE range starts one group early: its first step finds no halo values fetched for it, and needs none there.
        // The ranges are the same for the waves of both stages that share a quarter of the row (wq): the stage-0 wave
        // fetches the halo values of its own 128 columns, for itself and for its partner above.  Three plain loops: a branch
        // inside one loop brings the register blow-up described above back.
        const int lo0 = i0 - 3 * K - 4 * (K - 1) + 1, hi0 = i0 - 3 * K - 4 + 1 + 6;
        int g1 = lo0 >= 0 ? 0 : (-lo0 + 6) / 7, g2 = hi0 >= a.m ? 0 : (a.m - hi0 + 6) / 7 - 1;
        if (col_edge) g1 = groups;
        g1 = min(g1, groups);
        g2 = min(max(g2, g1), groups);
        // Two workgroups share a CU, and the SIMD arbiter favours the OLDER wave: left alone, the first-dispatched workgroup
        // runs at nearly full speed, finishes at 60 % of the launch, and the other one runs the rest of the time without a
        // partner (measured timeline: tools/probes/wg_stamps.hip -- 730 us and 1180 us on every CU; a workgroup alone
        // takes 810).  Time-sliced priorities share the CU evenly instead: every group of 7 steps a wave sets its
        // priority to one bit of the 100 MHz real-time counter (it flips every 2^prio_shift ticks), inverted in the
        // workgroups dispatched second (block index >= prio_split = number of CUs), so that the two workgroups of a CU
        // hold complementary priorities and swap them every slice: both progress at the same average rate, finish
        // together, and neither runs without a partner.
        const int cls = a.prio_split > 0 ? ((int) blockIdx.x >= a.prio_split ? 1 : 0) : -1;
        auto slice = [&]() {
            if (cls >= 0) {
                const int bit = (int) (__builtin_amdgcn_s_memrealtime() >> a.prio_shift) & 1;
                if (bit != cls)
                    __builtin_amdgcn_s_setprio(1);
                else
                    __builtin_amdgcn_s_setprio(0);
            }
        };
        int g = 0;
        if constexpr (STAGE > 0) {
            // Level l needs its first row complete in step 7 l - 1 and starts accumulating it six steps earlier: the levels
            // of stage s have nothing to do in the first s KL groups of a chunk.  Their waves only keep the barrier count
            // there, and the stages below have the vector pipe to themselves (a chunk costs about rows + 30 steps instead
            // of rows + 41 at K = 6: what thin shares of a multi-GPU run and small grids lose most).
            const int idle = min(STAGE * KL, groups);
            for (int q = 0; q < 7 * idle; ++q) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            g = idle;
        }
        edge_state();
        for (; g < g1; ++g) {
            slice();
            group(7 * g, std::true_type{});
        }
        for (; g < g2; ++g) {
            slice();
            group(7 * g, std::false_type{});
        }
        // again: pure functions of the arguments and the lane, cheaper than ten registers through the loop above.  (Not at one
        // level per wave: registers are no concern there, and the scalars the second call keeps alive cost two
        // instantiations of the two-application launch their eighth wave per SIMD.)
        if constexpr (KL > 1) edge_state();
        for (; g < groups; ++g) {
            slice();
            group(7 * g, std::true_type{});
        }
    };
    static_assert(S >= 1 && S <= 4, "stages");
    if (stage == 0) run_stage(std::integral_constant<int, 0>{});
    if constexpr (S >= 2)
        if (stage == 1) run_stage(std::integral_constant<int, 1>{});
    if constexpr (S >= 3)
        if (stage == 2) run_stage(std::integral_constant<int, 2>{});
    if constexpr (S >= 4)
        if (stage == 3) run_stage(std::integral_constant<int, 3>{});
#ifdef LORA_DIAGNOSTICS
    if (a.stamps && threadIdx.x == 0) a.stamps[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    // drain: the last D loads target this workgroup's LDS, which the next workgroup on this CU may own
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// How much later a rim-strip workgroup finishes than any other with the same number of steps, in per cent (plan option
// wg_edge_pct; -1 = this).  One wave per stage of such a workgroup runs the EDGE copy of the step, the others the interior
// copy.  Six applications: a step's median cost is 1.14 - 1.19 x, the slowest workgroups of both classes are 1.05 - 1.16 x apart
// (tools/wg_rim_ratio.py, profiles/r06_wg_rim_ratio.jsonl); up to 13 the 16384-column grid gets the layout that fills all 512
// slots, which is the faster one there (bench.py, builds alternating: profiles/r06_wg_strips_ab.jsonl).  Four and two: those
// launches wait for HBM, an interior step is shorter and the rim's extra work weighs more -- 16384^2, four applications, us
// per launch at 12 / 60: 920 / 867 (profiles/r06_wg_tails.jsonl).
constexpr int wg_edge_pct_default(int K) { return K >= 6 ? 12 : 60; }

// The row chunks of one launch of K applications over rows_total rows and `strips` column strips, on `slots` resident
// workgroups.  Rim strips (the first and the last; all of them below three) have chunks_e chunks of rows_e rows, the others
// chunks_i of rows_i.
struct WgLayout {
    int rim, rows_i, chunks_i, rows_e, chunks_e;
    long workgroups;
};

inline WgLayout wg_layout(int K, int strips, int rows_total, long slots, int edge_pct, int wg_rows) {
    const int lag = 7 * K - 1;  // steps of a chunk beyond its output rows
    auto fit = [&](long rows) {
        long g = (rows + lag + 6) / 7;
        if (g < K + 1) g = K + 1;
        return (int) (7 * g - lag);
    };
    auto chunks = [&](int rows) { return (rows_total + rows - 1) / rows; };
    WgLayout L{};
    L.rim = strips >= 3 ? 2 : strips;
    const int ni = strips - L.rim;
    const long ratio = 100 + (edge_pct >= 0 ? edge_pct : wg_edge_pct_default(K));
    // the most rows whose rim chunk finishes with an interior chunk of ri rows
    auto rim_target = [&](int ri) { return std::max(1L, (long) (ri + lag) * 100 / ratio - lag); };
    if (wg_rows > 0) {
        L.rows_i = fit(wg_rows);
        L.rows_e = ni > 0 ? fit(rim_target(L.rows_i)) : L.rows_i;
    } else {
        // ONE round: every workgroup of the launch resident at once.  Candidates: c interior chunks, and for the rim
        // strips the fewest chunks that finish with those -- or as many as the slots the interior chunks leave allow --
        // split evenly.  Score: the predicted finish, max(interior steps, ratio x rim steps); the first minimum wins.
        // Small grids: filling the round matters more than the rows a chunk recomputes -- down to chunks of about 1.5 x
        // the 7 K - 1 warm-up rows (star2d1r, six sweeps, GStencils/s at chunks of 64 / 100 / 128 / 164 / 256 rows: 4096^2
        // 636 / 837 / 762 / 675 / 595, 2048^2 375 / 289 / 245 / 208 / 149, 1024 x 16384 685 / 875 / 775 / 816 / 595 --
        // tools/wg_small.py; the first rule, four times the warm-up, left half the CUs idle on such grids)
        const long min_rows = 3 * lag / 2;
        long best = -1;
        for (long c = 1; c <= rows_total; ++c) {
            const int ri = fit((rows_total + c - 1) / c);
            if (ri < min_rows && c > 1) break;
            int re = ri;
            if (ni > 0) {
                const long ce_max = (slots - (long) ni * chunks(ri)) / L.rim;
                if (ce_max < 1 && c > 1) break;
                const long want = (rows_total + rim_target(ri) - 1) / rim_target(ri);
                const long ce = std::max(1L, std::min(want, ce_max));
                re = fit((rows_total + ce - 1) / ce);
            }
            if ((long) ni * chunks(ri) + (long) L.rim * chunks(re) > slots && c > 1) break;
            const long score = std::max(100L * (ri + lag), ratio * (re + lag));
            if (best < 0 || score < best) {
                best = score;
                L.rows_i = ri;
                L.rows_e = re;
            }
        }
    }
    L.chunks_i = chunks(L.rows_i);
    L.chunks_e = chunks(L.rows_e);
    L.workgroups = (long) ni * L.chunks_i + (long) L.rim * L.chunks_e;
    return L;
}

// Workgroups of this instantiation that are resident per CU (cached per device).  The first query of an instantiation
// also makes the runtime load and resolve the kernel -- half a millisecond of host time that lora_plan_create /
// lora_plan_set_* pay through prepare_2d_wg(), not the first launch of a run.
template <int EVAL, int KL, int S, int D, int WPS, bool DIRI>
int wg_per_cu(int dev) {
    static int per_cu[64] = {0};
    if (dev < 0 || dev >= 64) dev = 0;
    if (per_cu[dev] == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, stencil2d_wg_kernel<EVAL, KL, S, D, WPS, DIRI>, 256 * S, 0) != hipSuccess || nb < 1) {
            (void) hipGetLastError();
            return 1;  // (no device: asked again later)
        }
        per_cu[dev] = nb;
    }
    return per_cu[dev];
}

template <int EVAL, int KL, int S, int D, int WPS, bool DIRI>
hipError_t launch_wg_t(const Plan &p, ArgsWG a, int rows_total, hipStream_t s) {
    constexpr int K = KL * S;
    auto kernel = stencil2d_wg_kernel<EVAL, KL, S, D, WPS, DIRI>;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    // one round: as many workgroups as are resident at once
    const int per_cu_dev = wg_per_cu<EVAL, KL, S, D, WPS, DIRI>(dev);
    if (rows_total <= 0) return hipSuccess;  // prepare_2d_wg(): the query above is all that was wanted
    const WgLayout lay = wg_layout(K, a.strips, rows_total, (long) per_cu_dev * cus, p.wg_edge_pct, p.wg_rows);
    a.rim = lay.rim;
    const int ni = a.strips - a.rim;
    a.rows_i = lay.rows_i;
    a.rows_e = lay.rows_e;
    a.groups_i = (a.rows_i + 7 * K - 1 + 6) / 7;
    a.groups_e = (a.rows_e + 7 * K - 1 + 6) / 7;
    a.chunks_i = lay.chunks_i;
    a.chunks_e = lay.chunks_e;
    a.prio_split = (p.wg_prio != 0 && per_cu_dev == 2) ? cus : 0;
    a.prio_shift = p.wg_prio > 0 ? p.wg_prio : 12;
    Taps49 w;
    for (int k = 0; k < 49; ++k) w.w[k] = p.w[k];
    LowRankTaps f{};
    for (int tt = 0; tt < 3; ++tt)
        for (int e = 0; e < 7; ++e) {
            f.u[tt][e] = p.lowrank.u[tt][e];
            f.v[tt][e] = p.lowrank.v[tt][e];
        }
    f.rc = p.lowrank_rc;
    if (EVAL == EVAL_NEST)
        for (int k = 0; k < 4; ++k) {
            f.u[0][k] = p.nest_g[k];
            f.v[0][k] = p.nest_a[k];
        }
    const long nblocks = (long) ni * a.chunks_i + (long) a.rim * a.chunks_e;
    if (nblocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned) nblocks), dim3(256 * S), 0, s, a, w, f);
    return hipGetLastError();
}

// This file is compiled once per launch depth (LORA_WG_K = 6, 4, 2: eight tap evaluations each).  Two stages of K / 2
// levels, three rows in flight, four waves per SIMD in every case.
#ifndef LORA_WG_K
#define LORA_WG_K 6
#endif
#ifndef LORA_WG_S  // stages: 2 (two 8-wave workgroups per CU) for K <= 6; 4 (one 16-wave workgroup per CU) for K = 12 and 8
#define LORA_WG_S 2
#endif
template <int EVAL>
hipError_t launch_wg_e(const Plan &p, const ArgsWG &a, int rows_total, hipStream_t s) {
#if LORA_WG_K <= 4  // the Dirichlet option: halo values at every level (K = 6 would need 98 KB of LDS per workgroup)
    if (p.boundary == LORA_BC_DIRICHLET) return launch_wg_t<EVAL, LORA_WG_K / 2, 2, 3, 4, true>(p, a, rows_total, s);
#endif
    return launch_wg_t<EVAL, LORA_WG_K / LORA_WG_S, LORA_WG_S, 3, 4, false>(p, a, rows_total, s);
}

}  // namespace

#define LORA_WG_CAT2(a, b) a##b
#define LORA_WG_CAT(a, b) LORA_WG_CAT2(a, b)
#define LORA_WG_ENTRY LORA_WG_CAT(launch_2d_wg_k, LORA_WG_K)

// LORA_WG_K applications in one launch over interior rows [begin, end)
hipError_t LORA_WG_ENTRY(const Plan &p, ArgsWG a, int rows_total, hipStream_t s) {
    switch (p.fused_eval) {
        case EVAL_NEST:
            return launch_wg_e<EVAL_NEST>(p, a, rows_total, s);
        case EVAL_LR_DIAMOND:
            return launch_wg_e<EVAL_LR_DIAMOND>(p, a, rows_total, s);
        case EVAL_LR_PYRAMID:
            return launch_wg_e<EVAL_LR_PYRAMID>(p, a, rows_total, s);
        case EVAL_LR_PYRAMID_SYM:
            return launch_wg_e<EVAL_LR_PYRAMID_SYM>(p, a, rows_total, s);
        case EVAL_LR_PYRAMID_SYM_GAP:
            return launch_wg_e<EVAL_LR_PYRAMID_SYM_GAP>(p, a, rows_total, s);
        default:
            break;
    }
    switch (p.tapset) {
        case TAPS2D_DIAMOND:
            return launch_wg_e<TAPS2D_DIAMOND>(p, a, rows_total, s);
        case TAPS2D_STAR:
            return launch_wg_e<TAPS2D_STAR>(p, a, rows_total, s);
        default:
            return launch_wg_e<TAPS2D_BOX>(p, a, rows_total, s);
    }
}

#if LORA_WG_K == 6
hipError_t launch_2d_wg_k4(const Plan &p, ArgsWG a, int rows_total, hipStream_t s);
hipError_t launch_2d_wg_k2(const Plan &p, ArgsWG a, int rows_total, hipStream_t s);

// One-time host work of the three instantiations this plan's runs launch (six applications and the four / two of the
// tails): kernel resolution + the residency query.  No launch; without a device nothing happens.
void prepare_2d_wg(const Plan &p) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void) hipGetLastError();
        return;
    }
    ArgsWG a{};
    (void) launch_2d_wg_k6(p, a, 0, nullptr);
#ifndef LORA_WG_ONLY_K6
    (void) launch_2d_wg_k4(p, a, 0, nullptr);
    (void) launch_2d_wg_k2(p, a, 0, nullptr);
#endif
}

// Level 1 is complete on all 512 positions of a row (the ring holds the six positions behind them); levels 2 .. K lose six each
int wg_strip_width(int K) { return kRowW - 6 * (K - 1); }

// The layout of a launch of K applications over `rows` rows of the plan's grid on cus x per_cu resident workgroups, for
// lora_debug_wg_layout (no device): out = strips, outw, rows_i, chunks_i, rows_e, chunks_e, workgroups, rim strips
bool wg_layout_debug(const Plan &p, int K, int rows, int cus, int per_cu, int out[8]) {
    if ((K != 6 && K != 4 && K != 2) || rows < 1 || cus < 1 || per_cu < 1 || p.ndim != 2) return false;
    const int outw = wg_strip_width(K), strips = (p.dims[1] + outw - 1) / outw;
    const WgLayout L = wg_layout(K, strips, rows, (long) cus * per_cu, p.wg_edge_pct, p.wg_rows);
    if (L.workgroups > 0x7fffffffL) return false;
    const int v[8] = {strips, outw, L.rows_i, strips > L.rim ? L.chunks_i : 0, L.rows_e, L.chunks_e, (int) L.workgroups, L.rim};
    std::copy(v, v + 8, out);
    return true;
}

#ifdef LORA_DIAGNOSTICS
long long *g_wg_stamps = nullptr;  // set by the probe: 4 x int64 per workgroup
#endif

// K = 6, 4 or 2 applications in one launch over interior rows [begin, end)
hipError_t launch_2d_wg(const Plan &p, int K, const double *in, double *out, int begin, int end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    if (K != 6 && K != 4 && K != 2) return hipErrorInvalidValue;
    if (p.boundary == LORA_BC_PERIODIC || (p.boundary == LORA_BC_DIRICHLET && K == 6)) return hipErrorNotSupported;
    ArgsWG a;
    a.in = in;
    a.out = out;
    a.m = p.dims[0];
    a.n = p.dims[1];
    a.ld = a.n + 8;
    a.row_begin = begin;
    a.row_end = end;
    a.outw = wg_strip_width(K);
    a.strips = (a.n + a.outw - 1) / a.outw;
    a.rim = a.rows_i = a.groups_i = a.chunks_i = a.rows_e = a.groups_e = a.chunks_e = 0;
    a.prio_split = a.prio_shift = 0;
#ifdef LORA_DIAGNOSTICS
    a.stamps = g_wg_stamps;
#endif
#ifdef LORA_WG_ONLY_K6  // (tools/probes/wg_stamps.hip includes this file alone)
    return launch_2d_wg_k6(p, a, end - begin, s);
#else
    return K == 6 ? launch_2d_wg_k6(p, a, end - begin, s)
                  : (K == 4 ? launch_2d_wg_k4(p, a, end - begin, s) : launch_2d_wg_k2(p, a, end - begin, s));
#endif
}

const char *kernel_name_2d_wg(const Plan &) { return "stencil2d_wg_kernel"; }
#endif  // LORA_WG_K == 6

}  // namespace lora
