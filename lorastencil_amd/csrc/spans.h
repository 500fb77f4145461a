// spans.h -- how a launch of the register-resident 3D kernels (kernels_3d_lanes.hip, kernels_3d_bf16_lanes.hip) is cut
// along z: the host's choice of a layout (cut3_plan, under each kernel's CutRules) and the decode both kernels -- and the
// host tests -- run for it (cut3_begin / cut3_next).  Mostly about SPANS, the layout that is not equal chunks per tile:
//
// Those kernels run ONE workgroup per CU; a workgroup that starts anywhere along z runs S steps (its pipeline filling)
// before its first output plane, and a launch takes as long as its busiest CU.  Equal chunks per tile leave CUs idle
// whenever tiles x chunks is not a multiple of the CU count (768^3 bf16: 98 tiles x 5 chunks = 490 workgroups of 165 steps
// on 256 CUs = 330 steps, where 98 x 768 / 256 + 11 = 305 would do).  SPANS put all (tile, plane) pairs on one line --
// tile-major, tiles in rim-first order, a step of a rim tile weighted by what its EDGE steps cost, S steps of start per
// tile -- and cut the line into one equal piece per resident workgroup; a workgroup runs the one or two (on shallow regions
// several) tile SEGMENTS its piece touches.
//
// What it buys is measured, not assumed (tools/spans_sweep.py, profiles/r04_spans_*): fewer cycles everywhere, but
// neighbouring tiles are no longer at the same depth at the same time, so the rows they share -- and the 128-byte lines
// their misaligned row pieces straddle -- are fetched from HBM twice.  TEAM spans (the line over tile rows, a piece per
// team of a row's workgroups) keep the neighbours in x together.  Plan option spans3: -1 by the kernels' rules (spans_pay,
// teams_pay), 0 chunks, 1 spans, 2 team spans.  Chunked launches of the fp64 kernel have two layouts of their own: chunks
// dealt to resident workgroups when there are more chunks than CUs, and one chunk more for the slow rim tiles when a
// single round has CUs to spare.
#pragma once

#include <algorithm>

namespace lora {

struct Spans {
    int q, r;        // a workgroup's share of the line's cost units: q, the first r workgroups one more
    int vt;          // steps of a whole tile: the region's planes + the S steps of a start
    int wrim, win;   // cost units of a step of a tile on the rim of the grid (EDGE steps throughout) / of an inner tile
    int nrim;        // tiles on the rim (they come first on the line)
};

// Host: fill `sp` for a region of `depth` planes of tiles_x x tiles_y tiles on `slots` resident workgroups; returns the
// number of workgroups to launch, or 0 when the line does not fit 31 bits of cost units (then: chunks).
inline long spans_setup(Spans &sp, int tiles_x, int tiles_y, long depth, int S, long slots, int wrim, int win) {
    const long tiles = (long) tiles_x * tiles_y;
    const long nrim = (tiles_x < 3 || tiles_y < 3) ? tiles : 2L * tiles_x + 2L * (tiles_y - 2);
    sp.vt = (int) (depth + S);
    sp.wrim = wrim;
    sp.win = win;
    sp.nrim = (int) nrim;
    const long units = (depth + S) * (nrim * wrim + (tiles - nrim) * win);
    if (units >= (1L << 31)) return 0;
    // no more workgroups than pieces worth a start (a piece of at least ~S steps)
    const long wgs = std::max(1L, std::min(slots, units / ((long) S * win)));
    sp.q = (int) (units / wgs);
    sp.r = (int) (units % wgs);
    return wgs;
}

// The line of ONE tile column (team spans): tiles_y tiles, the first and last of them (rim rows: EDGE steps) at weight wrim and
// FIRST on the line, the others at win.  Tile t of this line is row column_line_row(t, tiles_y).
inline long spans_setup_column(Spans &sp, int tiles_y, long depth, int S, long slots, int wrim, int win) {
    const long nrim = tiles_y >= 3 ? 2 : tiles_y;
    sp.vt = (int) (depth + S);
    sp.wrim = wrim;
    sp.win = win;
    sp.nrim = (int) nrim;
    const long units = (depth + S) * (nrim * wrim + (tiles_y - nrim) * win);
    if (units >= (1L << 31)) return 0;
    const long wgs = std::max(1L, std::min(slots, units / ((long) S * win)));
    sp.q = (int) (units / wgs);
    sp.r = (int) (units % wgs);
    return wgs;
}

// Team spans with the rim columns cut finer: how many pieces a tile column between the rim columns gets (ni) and how many a
// rim column (nr >= ni), so that (tiles_x - 2) ni + 2 nr <= slots and nr / ni is about what a rim tile's steps cost more
// (EDGE steps: ~5.5 %).  768^3 bf16 (7 columns, 256 CUs): 36 and 38.
inline void team_pieces(int tiles_x, long slots, bool finer_rims, long *ni, long *nr) {
    *ni = *nr = slots / tiles_x;
    if (tiles_x >= 3 && finer_rims) {
        *ni = (long) ((double) slots / ((double) (tiles_x - 2) + 2.0 * 1.055));
        *nr = *ni > 0 ? std::min((slots - (tiles_x - 2) * *ni) / 2, (long) ((double) *ni * 1.07) + 1) : 0;
    }
}

// Equal chunks per tile: the chunk length by a model of rounds of workgroups.  A chunk runs S steps beyond its own planes,
// so chunks should be long; a round of workgroups (one per slot) takes its steps whatever its kernels do, and a LAST,
// partly filled round is cheaper than a full one only down to about two thirds of it.  Fitted to a sweep of chunk lengths
// (star3d1r 512^3 fp64, 110 tiles on 256 CUs, tools/thin3d_check.py; x = workgroups / CUs, time / 2.4 us / steps per chunk:
// x = 0.86 -> 1.00, 1.29 -> 1.78, 1.72 -> 1.99, 2.15 -> 2.70, 2.58 -> 2.97, 3.008 -> 3.65, 3.44 -> 3.97, 3.87 -> 4.16,
// 4.30 -> 4.88, 5.16 -> 5.8, 6.9 -> 7.2):   rounds_eff(x) = 1.03 floor(x) + (0.65 + 0.4 frac(x) if frac(x) > 0)
// and the chunk count that minimises rounds_eff x (zc + S) wins (chunks of at least `min_chunk` planes while the depth
// allows).  `cost`: that minimum, in steps.
inline int chunk_model(long tiles, long depth, int S, long slots, long min_chunk, double *cost) {
    double best = 0.0;
    long best_c = 1;
    for (long c = 1; c <= std::max(1L, depth / min_chunk); ++c) {
        const long zc = (depth + c - 1) / c, wgs = tiles * ((depth + zc - 1) / zc);
        const double x = (double) wgs / (double) slots;
        const double whole = (double) (long) x, part = x - whole;
        const double rounds = 1.03 * whole + (part > 1e-9 ? 0.65 + 0.4 * part : 0.0);
        const double c_steps = rounds * (double) (zc + S);
        if (best == 0.0 || c_steps < best) {
            best = c_steps;
            best_c = c;
        }
    }
    if (cost) *cost = best;
    return (int) ((depth + best_c - 1) / best_c);
}

// Do spans pay?  By measurement (tools/spans_sweep.py, profiles/r04_spans_sweep_*.jsonl, r04_spans_vs_chunks_pmc.txt), not
// by the step counts alone: spans always take fewer CYCLES (768^3 bf16: 14.2 M against 15.8 M per launch), but neighbouring
// tiles are no longer at the same depth at the same time, so the rows they share and the 128-byte lines their misaligned
// row pieces straddle come from HBM twice (768^3 bf16: 1.82 GB fetched against 1.19 GB) -- and with that traffic the clock
// sinks (1.77 GHz from the third launch on against 2.0 GHz: 1000 us against 867 us).  In short bursts the fp64 separable
// box gained 5 - 18 % at 768^3 / 512^3; over the 50 sweeps of a bench.py run it did not (790 - 900 against a steady
// 851 - 865 GStencils/s at 768^3, tools/spans_bench_ab.sh) -- the same clock effect on a slower fuse.  So: spans where their
// busiest workgroup runs fewer steps than the chunked launch's (whole rounds of workgroups) AND the region's
// input is small enough for the 256 MB Infinity Cache to serve the second fetches (`bytes_cap`; bf16: + 5 - 12 % on
// 64 - 192 x 768^2, - 2.5 % at 384, - 20 % at 768; fp64 star: + 27 % on 32 x 512^2, + 6 % on 128 x 512^2, - 6 - 10 % at 512^3 and
// 768^3) -- the z-slabs and end regions of the multi-GPU drivers, mostly.
inline bool spans_pay(long tiles, long depth, int S, long slots, int zc_model, double bytes, double bytes_cap) {
    const long wgs = tiles * ((depth + zc_model - 1) / zc_model), rounds = (wgs + slots - 1) / slots;
    const double chunk_steps = (double) rounds * (double) (zc_model + S);
    const double span_steps = 1.5 * S + (double) (tiles * (depth + S)) / (double) slots;  // a start, the share, half a second start
    return span_steps < chunk_steps && (bytes_cap <= 0.0 || bytes <= bytes_cap);
}

// TEAM spans: the line runs over tile ROWS and is cut into one piece per team of tiles_x workgroups, one per tile of the
// row.  The tiles of a row stay at the same depth -- and, dealt out contiguously, in the same XCD's L2 -- so the lines their
// row pieces share are fetched once, as with chunks; what is given up is the rows shared with the tile rows above and
// below, and a team runs at the pace of its rim tiles.  Measured (tools/spans_sweep.py, tools/spans_bench_ab.sh): bf16
// 768^3 732 us per launch against 754 (chunks) and 954 (spans), 2115 - 2134 against 2055 - 2093 GStencils/s over 50 sweeps;
// fp64 star 512^3 and box 768^3 4 - 9 % SLOWER than chunks (their rows overlap by a quarter, the bf16 tile's by an eighth).
// So: the bf16 kernel, on regions too big for plain spans, where a team's busiest member runs at least 3 % fewer steps.
inline bool teams_pay(int tiles_x, int tiles_y, long depth, int S, long slots, int zc_model) {
    if (tiles_x > slots) return false;
    const long tiles = (long) tiles_x * tiles_y, wgs = tiles * ((depth + zc_model - 1) / zc_model), rounds = (wgs + slots - 1) / slots;
    const double chunk_steps = (double) rounds * (double) (zc_model + S);
    const double team_steps = 1.5 * S + (double) (tiles_y * (depth + S)) / (double) (slots / tiles_x);
    return team_steps < 0.97 * chunk_steps;
}

// ---- the cut of ONE launch: what the host chooses (cut3_plan) and the kernels decode (cut3_begin / cut3_next) ----
struct Cut3 {
    int z_begin, z_end;
    int z_begin2, z_end2;  // a second range of planes in the same launch (chunks only): the two end regions of a slab
    int zc;                // > 0: chunks of zc planes; 0: spans
    int tiles_x, tiles_y;
    Spans sp;  // zc == 0: spans
    int team;  // zc == 0: 0 = a span per workgroup over all tiles; TX = a span per TEAM of the TX workgroups of a tile row
    // team spans: the first / last tile COLUMN (rim tiles: EDGE steps, 5 % longer each) is cut into team_nr pieces (Spans sp2),
    // the columns between into team_ni (Spans sp); team_nr == team_ni: whole teams in lockstep
    int team_ni, team_nr;
    Spans sp2;
    int deal;  // chunks, more workgroups' worth than slots: the launch is `slots` workgroups and chunk j goes to workgroup j mod slots (0: off)
    int slow_c, slow_zc;  // chunks, one round with slots to spare: the tiles of the first tile column and row get slow_c chunks of slow_zc planes (0: off)
};

// The layouts only one of the two kernels has (a kernel compiles the decode of its own alone), and what cut3_plan reports:
// which layout a launch got (where two apply, the later in this list).
enum : unsigned {
    CUT3_SLOW = 1,    // chunks, one more for the slow rim tiles
    CUT3_DEAL = 2,    // chunks dealt to the resident workgroups
    CUT3_COLUMN = 4,  // team spans over a tile COLUMN's line, its two rim rows first (else: a tile row's teams top to bottom)
    CUT3_FINER = 8,   // team spans with the rim columns cut finer and rim rows weighed 19 : 18
};
enum { CUT3_KIND_FIXED = 1, CUT3_KIND_MODEL, CUT3_KIND_RANGES2, CUT3_KIND_SLOW, CUT3_KIND_DEALT, CUT3_KIND_SPANS, CUT3_KIND_TEAMS, CUT3_KIND_TEAMS_FINER };

// What differs between the two kernels when a launch is cut.
struct CutRules {
    int S;                // steps of a segment beyond its planes
    int min_chunk;        // chunk_model: no shorter chunks while the depth allows
    int min_slow;         // CUT3_SLOW: no shorter chunks on the slow rim tiles
    double cell_bytes, bytes_cap;  // spans_pay: a region's input and what of it the Infinity Cache serves twice
    bool teams_by_rule;   // team spans where teams_pay says so (else by option spans3 = 2 only)
    unsigned decodes;     // CUT3_* the kernel compiles a decode for
    unsigned off;         // CUT3_* a probe build switches off (LORA_L3_ABLATE 256 / 512, LORA_BL_ABLATE 512)
    constexpr bool plans(unsigned layout) const { return (decodes & ~off & layout) != 0; }
};
constexpr CutRules lanes3_rules(int K, int ablate = 0) {  // kernels_3d_lanes.hip (fp64)
    return {2 * K + 1, 8 * K, 2 * K, 8.0, 300.0e6, false, CUT3_SLOW | CUT3_DEAL, ((ablate & 256) ? CUT3_SLOW : 0u) | ((ablate & 512) ? CUT3_DEAL : 0u)};
}
constexpr CutRules bf16_lanes_rules(int K, int ablate = 0) {  // kernels_3d_bf16_lanes.hip
    return {3 * K - 1, 4 * K, 0, 2.0, 256.0e6, true, CUT3_COLUMN | CUT3_FINER, (ablate & 512) ? CUT3_FINER : 0u};
}

// Spans over all tiles of c.tiles_x x c.tiles_y; returns the workgroups, 0: the line does not fit (then: chunks)
inline long cut3_set_spans(Cut3 &c, long depth, int S, long slots) {
    c.zc = c.team = 0;
    return spans_setup(c.sp, c.tiles_x, c.tiles_y, depth, S, slots, 10, 9);
}

// TEAM spans: the line runs over tile rows and is cut into one piece per team of tiles_x workgroups, one per tile of the
// row -- x-neighbours stay at the same depth (and, dealt out contiguously, in the same XCD's L2).  `layouts` & CUT3_COLUMN:
// a column's line has its rim rows first; & CUT3_FINER: the rim columns' tiles run EDGE steps, ~5 % longer each (tools/probes/
// bf16_lanes_timeline.hip: 2.47 against 2.34 us per step; with equal pieces the launch ended with the rim columns' workgroups
// at 775 us, the others at 734), so the rim columns are cut into more, shorter pieces than the columns between -- 38 and 36 at
// 768^3, which also uses all 256 CUs instead of 252 -- and within a column between them the first and last tile ROW are rim
// tiles too: their planes weigh 19 : 18.  The columns between stay in lockstep with one another.  Needs tiles_x <= slots.
inline long cut3_set_teams(Cut3 &c, long depth, int S, long slots, unsigned layouts) {
    const bool finer = (layouts & CUT3_FINER) != 0, weigh = finer && c.tiles_x >= 3;
    long ni, nr, ti, tr;
    team_pieces(c.tiles_x, slots, finer, &ni, &nr);
    if (layouts & CUT3_COLUMN) {
        ti = ni > 0 ? spans_setup_column(c.sp, c.tiles_y, depth, S, ni, weigh ? 19 : 1, weigh ? 18 : 1) : 0;
        tr = nr > 0 ? spans_setup_column(c.sp2, c.tiles_y, depth, S, nr, 1, 1) : 0;
    } else {
        ti = tr = spans_setup(c.sp, 1, c.tiles_y, depth, S, ni, 1, 1);
    }
    if (ti <= 0 || tr < ti) return 0;
    c.zc = 0;
    c.team = c.tiles_x;
    c.team_ni = (int) ti;
    c.team_nr = (int) (c.tiles_x >= 3 ? tr : ti);
    return c.tiles_x >= 3 ? ti * (c.tiles_x - 2) + 2 * tr : ti * c.tiles_x;
}

// How a launch over planes [begin, end) (and [begin2, end2)) of tiles_x x tiles_y tiles is cut along z on `slots` resident
// workgroups: chunks of option fused_z_chunk; else spans or team spans (option spans3 = 1 / 2, or by themselves where they
// pay: spans_pay, teams_pay); else equal chunks by the model of rounds of workgroups, with the kernel's own tails (slow rim
// tiles, dealt chunks).  `plane`: cells of a padded plane.  Fills `c`; returns the workgroups to launch, -1: too many.
inline long cut3_plan(const CutRules &R, int tiles_x, int tiles_y, long plane, int begin, int end, int begin2, int end2, long slots,
                      int fused_z_chunk, int spans3, Cut3 &c, int *kind = nullptr) {
    const long tiles = (long) tiles_x * tiles_y, depth = end - begin, depth2 = std::max(end2 - begin2, 0);
    c = Cut3{};
    c.z_begin = begin;
    c.z_end = end;
    c.z_begin2 = begin2;
    c.z_end2 = begin2 + (int) depth2;
    c.tiles_x = tiles_x;
    c.tiles_y = tiles_y;
    long nblocks = 0;
    int k = CUT3_KIND_MODEL;
    if (fused_z_chunk > 0) {
        c.zc = (int) std::min((long) fused_z_chunk, std::max(depth, depth2));
        k = CUT3_KIND_FIXED;
    } else if (depth2 > 0) {  // two ranges (a slab's end regions): chunks, as many workgroups as two ranges of the longer depth
        c.zc = chunk_model(2 * tiles, std::max(depth, depth2), R.S, slots, R.min_chunk, nullptr);
    } else {
        const int zc_model = chunk_model(tiles, depth, R.S, slots, R.min_chunk, nullptr);
        const bool spans = spans3 >= 1 || (spans3 < 0 && spans_pay(tiles, depth, R.S, slots, zc_model, R.cell_bytes * (double) plane * (double) depth, R.bytes_cap));
        // (fp64 by option only: team spans measured 4 - 9 % slower than chunks on fp64 grids, teams_pay)
        const bool teams = spans3 == 2 || (R.teams_by_rule && spans3 < 0 && !spans && teams_pay(tiles_x, tiles_y, depth, R.S, slots, zc_model));
        if (teams && tiles_x <= slots) {
            nblocks = cut3_set_teams(c, depth, R.S, slots, R.decodes & ~R.off);
            k = c.team_nr != c.team_ni ? CUT3_KIND_TEAMS_FINER : CUT3_KIND_TEAMS;
        } else if (spans) {
            nblocks = cut3_set_spans(c, depth, R.S, slots);
            k = CUT3_KIND_SPANS;
        }
        if (nblocks == 0) c.zc = zc_model, k = CUT3_KIND_MODEL;  // (or a line that does not fit 31 bits of cost units)
    }
    if (c.zc > 0) nblocks = tiles * ((depth + c.zc - 1) / c.zc + (depth2 + c.zc - 1) / c.zc);
    if (c.zc > 0 && depth2 > 0) k = CUT3_KIND_RANGES2;
    if (R.plans(CUT3_SLOW) && c.zc > 0 && depth2 == 0 && fused_z_chunk <= 0 && tiles_x >= 2 && tiles_y >= 2) {
        // one round with slots to spare: one chunk more for the tiles of the first tile column and row (cut3_next)
        const long ch = (depth + c.zc - 1) / c.zc, nslow = tiles_x + tiles_y - 1;
        const long slow_zc = (depth + ch) / (ch + 1);
        if (nblocks <= slots && nblocks + nslow <= slots && slow_zc >= R.min_slow) {
            c.slow_c = (int) ((depth + slow_zc - 1) / slow_zc);
            c.slow_zc = (int) slow_zc;
            nblocks = nslow * c.slow_c + (tiles - nslow) * ch;
            k = CUT3_KIND_SLOW;
        }
    }
    if (R.plans(CUT3_DEAL) && c.zc > 0 && c.slow_c == 0 && nblocks > slots) {  // several rounds: deal the chunks out
        if (nblocks > 0x7fffffffL) return -1;
        c.deal = (int) nblocks;
        nblocks = slots;
        k = CUT3_KIND_DEALT;
    }
    if (kind) *kind = k;
    return nblocks > 0x7fffffffL ? -1 : nblocks;
}

#ifdef __HIPCC__
// The workgroups of `Kernel` (launched with `threads` threads) resident at once on the current device, resolved once per
// device (and with it the kernel itself: lora_plan_create's share); -1: none fits a CU, the plan must not choose it.
template <auto Kernel>
long resident_slots(int threads) {
    static int per_cu[64] = {0};
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    if (per_cu[dev] == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, threads, 0) != hipSuccess || nb < 1) {
            (void) hipGetLastError();
            nb = -1;
        }
        per_cu[dev] = nb;
    }
    return per_cu[dev] < 0 ? -1 : (long) per_cu[dev] * cus;
}
#define LORA_SPANS_FN __host__ __device__ __forceinline__
#else
#define LORA_SPANS_FN inline
#endif
// (the decode below is what the kernels run; it is plain integer arithmetic and also compiles for the host, where
// lora_debug_span_cover and lora_debug_cut_cover walk every workgroup of a launch with it for the tests)
// tile t of the rim-first order -> (tx, ty): the TX x TY tiles' rim (first and last row, then first and last column), then
// the inner tiles row by row
LORA_SPANS_FN void rim_first_tile(int t, int TX, int TY, int &tx, int &ty) {
    if (TX < 3 || TY < 3) {
        ty = t / TX;
        tx = t - ty * TX;
        return;
    }
    const int rim = 2 * TX + 2 * (TY - 2);
    if (t < 2 * TX) {
        ty = t < TX ? 0 : TY - 1;
        tx = t < TX ? t : t - TX;
    } else if (t < rim) {
        const int k = t - 2 * TX;
        ty = 1 + (k >> 1);
        tx = (k & 1) ? TX - 1 : 0;
    } else {
        const int idx = t - rim;
        ty = 1 + idx / (TX - 2);
        tx = 1 + idx - (ty - 1) * (TX - 2);
    }
}

// workgroup `lin` of a chunked launch (`chunks` chunks per tile) -> (chunk, tile): all chunks of the rim tiles first
LORA_SPANS_FN void chunk_of(int lin, int chunks, int TX, int TY, int &chunk, int &tx, int &ty) {
    if (TX < 3 || TY < 3) {
        const int per_chunk = TX * TY;
        chunk = lin / per_chunk;
        rim_first_tile(lin - chunk * per_chunk, TX, TY, tx, ty);
        return;
    }
    const int rim = 2 * TX + 2 * (TY - 2), inner = (TX - 2) * (TY - 2);
    if (lin < rim * chunks) {
        chunk = lin / rim;
        rim_first_tile(lin - chunk * rim, TX, TY, tx, ty);
    } else {
        const int l2 = lin - rim * chunks;
        chunk = l2 / inner;
        rim_first_tile(rim + l2 - chunk * inner, TX, TY, tx, ty);
    }
}

// tile t of a tile column's line (spans_setup_column) -> tile row: the two rim rows first
LORA_SPANS_FN int column_line_row(int t, int TY) { return TY < 3 ? t : (t == 0 ? 0 : (t == 1 ? TY - 1 : t - 1)); }

// this workgroup's range [v0, v1) of the line
LORA_SPANS_FN void span_range(const Spans &sp, int lin, unsigned &v0, unsigned &v1) {
    v0 = (unsigned) lin * (unsigned) sp.q + (unsigned) (lin < sp.r ? lin : sp.r);
    v1 = v0 + (unsigned) sp.q + (lin < sp.r ? 1u : 0u);
}

// The next segment of [v0, v1): its tile and planes [z0, z0 + zc) of the region; advances v0.  A tile's first S steps'
// worth of units stand for the start every segment pays (charged once per workgroup outside the line, so a range that
// ENTERS a tile spends them here).  false: this piece of the range holds no plane (it ends inside a tile's start).
LORA_SPANS_FN bool span_next(const Spans &sp, int S, unsigned &v0, unsigned v1, int TX, int TY, int &tx, int &ty,
                                          int &z0, int &zc) {
    const unsigned rim_units = (unsigned) sp.nrim * (unsigned) sp.vt * (unsigned) sp.wrim;
    const bool in_rim = v0 < rim_units;
    const unsigned w = in_rim ? sp.wrim : sp.win, tile_units = (unsigned) sp.vt * w;
    const unsigned base = in_rim ? 0u : rim_units, ti = (v0 - base) / tile_units;
    const unsigned tile_v = base + ti * tile_units, e = v1 < tile_v + tile_units ? v1 : tile_v + tile_units;
    const int p0 = (int) ((v0 - tile_v) / w) - S, p1 = (int) ((e - tile_v) / w) - S;
    z0 = p0 > 0 ? p0 : 0;
    const int z1 = p1 > 0 ? p1 : 0;
    rim_first_tile((int) ti + (in_rim ? 0 : sp.nrim), TX, TY, tx, ty);
    v0 = e;
    zc = z1 - z0;
    return zc > 0;
}

// A workgroup's walk over its SEGMENTS (a tile and planes [k0, k0 + zc) of it), whatever the layout of the cut: spans -- the
// workgroup owns a range of the line of all (tile, plane) pairs and runs one segment per tile the range touches; chunks -- one
// segment, chunk `lin / tiles` of its tile, the tiles on the rim of the grid first (they run the slower EDGE steps
// throughout, and with the long workgroups dispatched first the short ones even out the end of the launch), or several when
// the chunks are dealt.  DEC: the CUT3_* layouts compiled in (CutRules::decodes); all of it is uniform scalar work.
struct Cut3Cursor {
    unsigned v0, v1;  // spans: what is left of the workgroup's range
    int job;          // chunks: the workgroup's (next) chunk
    int col;          // team spans: the workgroup's tile column
    const Spans *line;  // ... and its column's line: c.sp2 for a rim column with pieces of its own, else c.sp
};

LORA_SPANS_FN int cut3_min(int a, int b) { return a < b ? a : b; }

template <unsigned DEC>
LORA_SPANS_FN void cut3_begin(const Cut3 &c, int lin, Cut3Cursor &s) {
    s.v0 = s.v1 = 0;
    s.job = lin;
    s.col = 0;
    // (The range is taken from c.sp / c.sp2 by name and the line chosen in a statement of its own on purpose: with the range
    // taken through s.line the four-application bf16 kernel, which has no register to spare, spills 8 bytes per lane.)
    if (c.zc == 0 && c.team) {
        // workgroups 0 .. TX team_ni - 1: piece lin / TX of column lin mod TX (x-neighbours side by side: one L2); the rest:
        // the extra pieces of the two rim columns
        int j;
        if (!(DEC & CUT3_FINER) || lin < c.team * c.team_ni) {
            j = lin / c.team;
            s.col = lin - j * c.team;
        } else {
            const int r = lin - c.team * c.team_ni;
            j = c.team_ni + (r >> 1);
            s.col = (r & 1) ? c.team - 1 : 0;
        }
        if ((DEC & CUT3_FINER) && c.team_nr != c.team_ni && (s.col == 0 || s.col == c.team - 1))
            span_range(c.sp2, j, s.v0, s.v1);
        else
            span_range(c.sp, j, s.v0, s.v1);
    } else if (c.zc == 0) {
        span_range(c.sp, lin, s.v0, s.v1);
    }
    s.line = ((DEC & CUT3_FINER) && c.team && c.team_nr != c.team_ni && (s.col == 0 || s.col == c.team - 1)) ? &c.sp2 : &c.sp;
}

// The next segment of workgroup `lin` of `nwg`; `more`: call again.  false: this piece of a span holds no plane.
template <unsigned DEC>
LORA_SPANS_FN bool cut3_next(const Cut3 &c, int S, int nwg, Cut3Cursor &s, int &tx, int &ty, int &k0, int &zc, bool &more) {
    const int TX = c.tiles_x, TY = c.tiles_y;
    if (c.zc == 0) {
        int z0;
        bool any;
        if (c.team) {  // the line runs over tile ROWS; this workgroup is column s.col of its team's row
            int t0;
            any = span_next((DEC & CUT3_FINER) ? *s.line : c.sp, S, s.v0, s.v1, 1, TY, t0, ty, z0, zc);
            if (DEC & CUT3_COLUMN) ty = column_line_row(ty, TY);
            tx = s.col;
        } else {
            any = span_next(c.sp, S, s.v0, s.v1, TX, TY, tx, ty, z0, zc);
        }
        more = s.v0 < s.v1;
        k0 = c.z_begin + z0;
        return any;
    }
    int chunk;
    const int c0 = (c.z_end - c.z_begin + c.zc - 1) / c.zc, c1 = (c.z_end2 - c.z_begin2 + c.zc - 1) / c.zc;
    if ((DEC & CUT3_SLOW) && c.slow_c > 0) {
        // A launch of ONE round with slots to spare: the full rim tiles -- first tile column and first tile row: EDGE
        // steps on every lane's worth of memory traffic, 8 - 17 % longer than an inner tile's (tools/probes/
        // lanes3_timeline.hip) -- are cut into one chunk more than the others, so that the launch no longer waits for them.
        const int lin = s.job, nslow = TX + TY - 1, na = nslow * c.slow_c;
        if (lin < na) {
            const int j = lin / c.slow_c;
            chunk = lin - j * c.slow_c;
            tx = j < TY ? 0 : j - TY + 1;
            ty = j < TY ? j : 0;
            k0 = c.z_begin + chunk * c.slow_zc;
            zc = cut3_min(c.slow_zc, c.z_end - k0);
        } else {
            const int l2 = lin - na, i = l2 / c0;
            chunk = l2 - i * c0;
            ty = 1 + i / (TX - 1);
            tx = 1 + i - (ty - 1) * (TX - 1);
            k0 = c.z_begin + chunk * c.zc;
            zc = cut3_min(c.zc, c.z_end - k0);
        }
    } else {
        // (c.deal: the chunks of a launch of several rounds are DEALT to the resident workgroups, chunk j to workgroup
        // j mod slots, instead of being dispatched one workgroup each as slots fall free.  Every workgroup then runs the
        // same number of chunks and about the same number of rim chunks.  Dispatched one by one, the 1792 chunks of
        // box3d1r 768^3 -- seven rounds exactly, rim chunks 259 us, inner ones 225 -- left some CUs with eight chunks and
        // others with six: the last tenth of the launch ran on 96 of 256 CUs, profiles/r04_lanes3_timeline.txt.)
        chunk_of(s.job, c0 + c1, TX, TY, chunk, tx, ty);
        const int zb = chunk < c0 ? c.z_begin : c.z_begin2, ze = chunk < c0 ? c.z_end : c.z_end2;
        k0 = zb + (chunk < c0 ? chunk : chunk - c0) * c.zc;
        zc = cut3_min(c.zc, ze - k0);
        if (DEC & CUT3_DEAL) s.job += nwg;
    }
    more = (DEC & CUT3_DEAL) && c.deal > 0 && s.job < c.deal;
    return true;
}

// Host, for the tests (lora_debug_span_cover, lora_debug_cut_cover): every workgroup of a launch of `wgs` cut as `c` walked
// with the cursor above; cover[(ty * tiles_x + tx) * h + z] += 1 per segment that sweeps plane z of h of the tile, *max_steps =
// the busiest workgroup's steps (S per segment + its planes).  false: a segment outside the tiles or the planes.
template <unsigned DEC>
inline bool cut3_walk(const Cut3 &c, int S, long wgs, int h, int *cover, int *max_steps) {
    int busiest = 0;
    for (long lin = 0; lin < wgs; ++lin) {
        Cut3Cursor cur;
        cut3_begin<DEC>(c, (int) lin, cur);
        int steps = 0;
        for (bool more = true; more;) {
            int tx, ty, k0, zc;
            if (!cut3_next<DEC>(c, S, (int) wgs, cur, tx, ty, k0, zc, more)) continue;
            if (tx < 0 || tx >= c.tiles_x || ty < 0 || ty >= c.tiles_y || k0 < 0 || k0 + zc > h) return false;
            for (int z = k0; z < k0 + zc; ++z) cover[((long) ty * c.tiles_x + tx) * h + z] += 1;
            steps += S + zc;
        }
        busiest = std::max(busiest, steps);
    }
    if (max_steps) *max_steps = busiest;
    return true;
}
}  // namespace lora
