// engine.h -- internal interfaces of liblorastencil_hip (not installed; the public surface is
// include/lorastencil.h).
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

#include "lorastencil.h"

namespace lora {

// ---- host helpers (weights.cpp) ------------------------------------------------------------
int shape_ndim(int shape);
int shape_ntaps(int shape);
int default_params(int shape, double *params);
int effective_weights(int shape, const double *params, double *weights);
int factorize_7x7(const double *params, double u[4][7], double v[4][7], double *residual_max);
int svd_7x7(const double *W, double u[7][7], double v[7][7], double sigma[7]);
int separable_27(const float *w27, float *cba9);
int separable_27d(const double *w27, double *cba9);  // the same in fp64 (3D fp64 plane-streaming kernel)  // exact rank-1 test of fp32 3x3x3 taps; cba = c(x), b(y), a(z)
int mfma_factors_27(const float *cba9, float *scale, float *cba9_normalised);  // bf16-exact normalised factors or 0

// ---- tap sets: which of the 49 / 27 taps a kernel instantiation evaluates --------------------
enum TapSet2D { TAPS2D_DIAMOND = 0, TAPS2D_STAR = 1, TAPS2D_BOX = 2 };
enum TapSet3D { TAPS3D_STAR = 0, TAPS3D_BOX = 1, TAPS3D_SEP = 2 };  // SEP: w = a (x) b (x) c exactly (bf16 path)

struct Taps9 {
    double w[9];
};
struct Taps49 {
    double w[49];
};
struct Taps27 {
    double w[27];
};

// Band factors of the low-rank MFMA formulation: out = sum_t (U_t X) V_t + sparse residual.
struct LowRank2D {
    int rank;         // 1..3 terms
    double u[3][7];   // vertical profile of term t
    double v[3][7];   // horizontal profile of term t
    int nresid;       // residual taps applied on the vector pipe
    int rdy[16], rdx[16];
    double rw[16];
};

// ---- plan -------------------------------------------------------------------------------------
// What a refresh derives from the taps and the requested state below (plan.cpp: resolve_1d / _2d / _3d).  Every refresh
// starts from these defaults, so nothing here outlives the state it was derived from.
struct Resolved {
    int tapset = 0;
    int fused_rows = 8;       // 2D fused: intermediate rows per wave (tile = 4x this - 6 output rows)
    int steps_per_launch = 1;
    int fused_eval = 0;       // 0..2 = direct taps of `tapset`, 3 = low-rank diamond, 4..6 = low-rank pyramid forms, 7 = nested profiles
    double lowrank_rc = 0.0;  // weight of the diamond form's 8-point correction
    double nest_g[4] = {0, 0, 0, 0}, nest_a[4] = {0, 0, 0, 0};  // fused_eval 7: nested-profile form (rows_2d.h)
    bool lowrank_valid = false;
    LowRank2D lowrank{};
    int wg_active = 0;        // 2D fused launches go through the workgroup-row kernel
    int stream3_active = 0;   // 3D fused launches go through the plane-streaming kernel
    int lanes3_active = 0;    // 3D fused launches go through the register-resident kernels
    double sep64[9] = {0};    // fp64 factors c(x), b(y), a(z) of exactly separable 3D taps (plane-streaming / register-resident kernels)
    int sep64_valid = 0;      // the fp64 taps are exactly separable and the option allows that form
    float sep[9] = {0};       // factors c(x), b(y), a(z) when tapset == TAPS3D_SEP
    bool mfma3_valid = false; // bf16: the taps are scale * a (x) b (x) c with bf16-exact normalised factors (MFMA variant)
    float mfma3_scale = 0.0f, mfma3_abc[9] = {0};  // normalised c, b, a
    std::string kernel_name;
};

// The requested state: what the caller fixed at creation or set since.  (`variant` is a request a refresh may downgrade
// when the taps / boundary no longer allow the matrix-pipe kernels.)
struct Plan : Resolved {
    int shape = 0, ndim = 0, dtype = LORA_F64;
    int dims[3] = {0, 0, 0};  // interior extents, outermost first
    int ntaps = 0;
    double w[49] = {0};  // taps applied per sweep
    int variant = LORA_VARIANT_DIRECT;
    bool generic = false;  // odd innermost extent: rows are only 8-byte aligned, the tiled kernels do not apply
    int boundary = LORA_BC_REFERENCE;  // what halo cells hold between sweeps (lora_plan_set_boundary)
    unsigned epoch = 0;   // bumped by every change of taps / options: invalidates a cached graph
    const void *source = nullptr;  // lora_plan_set_source: the caller's padded grid f of u <- S(u) + f (borrowed; nullptr = none)
    // tuning knobs (lora_plan_set_option; plan.cpp: kOptions)
    int rows_per_thread = 8;  // 2D direct: output rows per lane (tile height = 4x this)
    int panel_width = 32;     // 2D: tile columns per L2 panel of the block->tile map
    int nt_store = 0;         // 2D: non-temporal output stores
    int fused_rows_req = 0;   // 0 = auto, else 6 / 8 / 10
    int cols_per_lane = 4;    // 3D bf16: 4 (512-byte row pieces per wave) or 8 (1 KiB)
    int separable = -1;       // 3D bf16: evaluate exactly-separable taps as x/y/z passes: -1 auto (= on), 0 off
    int mfma_split = 1;       // bf16 MFMA variant: intermediate as hi + lo bf16 halves (1, the contract) or one bf16 rounding (0)
    int ablate = 0;           // diagnostics only (2D fused, 3D bf16): 1 = skip stores, 2 = skip loads; results wrong
    int lds_dma = 0;          // 3D bf16: global_load_lds ring, two planes ahead (hand-counted vmcnt)
    int persistent = 0;       // 2D fused: persistent workgroups with register prefetch of the next tile
    int stream2 = 1;          // 2D fused: row-streaming kernel (kernels_2d_stream.hip, default) or the tile kernel (0)
    int stream_rows = 0;      // ... output rows per chunk (0 = auto: whole rounds of resident waves)
    int stream_depth = 4;     // ... input rows in flight per wave (2..6; at most 3 with four applications per launch)
    int stream_share = 0;     // ... one ring of whole rows per workgroup, a barrier per row (fewer, aligned L2 requests)
    int stream_prefetch = 0;  // ... K = 4: fetch the next level's LDS window while the current level computes (measured: no gain)
    int stream_sync = 1;      // ... s_barrier per 7 rows (1) / per row (2) keeps a workgroup's four strips in step
    int wg = -1;              // 2D fused launches through the workgroup-row kernel (kernels_2d_wg.hip): -1 = when the plan fuses six applications per launch (then also its four / two tails), 0 never, 1 always
    int wg_rows = 0;          // 2D workgroup-row kernel (kernels_2d_wg.hip): output rows per chunk (0 = auto: one round of resident workgroups)
    int wg_prio = 12;         // ... time-sliced wave priorities that share a CU evenly between its two workgroups: log2 of the slice in 10 ns ticks (0 = off)
    int wg_edge_pct = -1;     // ... how much shorter the chunks of the first / last strip are, in per cent of a step's cost (-1 = default)
    int z_chunk = 16;         // 3D: output planes streamed per workgroup
    int fused_pipeline = 0;   // 3D bf16 fused: 1 = level 2 one plane behind level 1, one barrier per plane (no gain measured)
    int stream3 = -1;         // 3D fp64 fused: plane-streaming kernel (kernels_3d_planes.hip: 2 or 3 applications per launch) always (1), never (0: the tile kernel, 2 applications), or by grid size (-1)
    int stream3_waves = 0;    // 3D plane-streaming kernel: waves per workgroup: 0 = automatic, 8 (one workgroup per CU) or 4 (two); output tiles of 8 x waves - 2 (K - 1) rows x 60 columns
    int stream3_pipe = 0;     // 3D plane-streaming kernel: 1 = every level consumes what was published one step earlier (one barrier per step, two buffers per level)
    int stream3_async = 0;    // 3D plane-streaming kernel: 1 = no workgroup barriers (neighbour-wave counters in LDS, private input rings)
    int stream3_slots = 0;    // 3D plane-streaming kernel: input plane slots of the LDS ring (0 or kStream3Slots: the one ring there is)
    int lanes3 = -1;          // 3D fused launches through the register-resident kernels (kernels_3d_lanes.hip, fp64; kernels_3d_bf16_lanes.hip, bf16: four applications per launch): -1 by grid size, 0 never, 1 always (star / separable box taps, reference boundary)
    int fused_z_chunk = 0;    // 3D fused: output planes per workgroup (0 = auto: 32, shorter on small grids)
    int leap3 = 0;            // 3D fp64: leapfrog runs take the two-step launch (kernels_3d_step2.hip); no effect outside 3D
    int wave3 = 0;            // 3D fp64: wave runs take the two-step launch (kernels_3d_step2.hip, EPI_WAVE); no effect outside 3D
    int coarse1 = 0;          // multigrid cycles of this plan run a coarsest level that fits as ONE launch (lora_plan_cg_small; mg.cpp)
    int mgfuse = 0;           // multigrid cycles of this plan restrict a level's defect in the launch that computes it (lora_plan_mg_defect_restrict; mg.cpp)
    int spans3 = -1;          // 3D register-resident kernels: cut the (tile, plane) line into equal pieces per CU (1), equal chunks per tile (0), by region depth (-1)
    int torus = 1;            // periodic boundary: runs in fused launches on a ghost-extended grid (1), single sweeps behind a wrap each (0)
    int steps_per_launch_req = 0;  // 0 = auto, 1, 2 (2D / 3D), 3 / 4 (3D), 4 / 6 (2D), 2 .. 32 (1D)
    int lowrank_valu = -1;    // 2D fused: low-rank evaluation on the vector pipe: -1 auto, 0 off, 1 on when the factors fit
    int use_scratch = -1; // odd numbers of fused launches route through a scratch grid owned by the plan: -1 / 1 yes, 0 no
    int use_graph = -1;   // -1 auto (small grids, many launches, non-default stream), 0 never, 1 whenever possible
};

// ---- one predicate per fact about a plan ------------------------------------------------------------------------------
// The deepest launch a plan of `ndim` dimensions can have (1D fused kernel / 2D workgroup-row kernel / 3D register-resident
// kernels).
constexpr int max_depth(int ndim) { return ndim == 1 ? 32 : (ndim == 2 ? 6 : 4); }
// The 3D plane-streaming kernel's LDS ring has two input plane slots (deeper rings -- 7 waves x 3 slots, 6 x 4 -- were
// built and measured within 3 % of it; they are gone again).
constexpr int kStream3Slots = 2;
// Whether the plan has kernels that fuse applications at all: every 1D plan, 2D plans of the direct variant, 3D plans --
// with an odd innermost extent only where `odd_ok` says one of them takes such rows.
inline bool has_fused_kernels(const Plan &p, bool odd_ok) {
    return p.ndim == 1 || ((p.ndim == 3 || p.variant == LORA_VARIANT_DIRECT) && (!p.generic || odd_ok));
}
// ... as resolved: odd rows go through the 2D row-streaming family under the reference boundary (the source's own halo),
// in 3D through the register-resident kernels.
inline bool has_fused_kernels(const Plan &p) {
    return has_fused_kernels(p, p.ndim == 2 ? p.stream2 && p.boundary == LORA_BC_REFERENCE : p.lanes3_active != 0);
}
// Whether the 3D matrix-pipe variant applies: bf16 box taps with bf16-exact factors, reference boundary, fused launches.
inline bool mfma3_applies(const Plan &p) {
    return p.dtype == LORA_BF16 && p.mfma3_valid && p.boundary == LORA_BC_REFERENCE && p.steps_per_launch_req != 1;
}

void plan_refresh(Plan &p);  // plan.cpp: re-derive everything in Resolved from w + the requested state

// ---- kernel launchers (kernels_*.hip).  Interior index range [begin, end) of the outermost
// dimension; all return the launch status. ----------------------------------------------------
hipError_t launch_1d(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
// K (2 / 4 / 8 / 16 / 32) applications per launch, intermediate levels in LDS
hipError_t launch_1d_fused(const Plan &p, int K, const double *in, double *out, int begin, int end, hipStream_t s);
const char *kernel_name_1d_fused(const Plan &p);
hipError_t launch_2d_direct(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
hipError_t launch_2d_mfma(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
// two applications per launch (intermediate level in LDS, its halo = 0); 2D direct taps only
hipError_t launch_2d_fused2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
// halo cells of a padded array (any shape / element type): copy from src, zero, or periodic wrap from dst itself
enum HaloMode { HALO_COPY = 0, HALO_ZERO = 1, HALO_WRAP = 2 };
hipError_t launch_halo(const Plan &p, void *dst, const void *src, int mode, hipStream_t s);
// rows x cols doubles between two strided arrays (pack / unpack of a block decomposition's column ghost zones)
hipError_t launch_copy_block(double *dst, long dst_ld, const double *src, long src_ld, long rows, long cols, hipStream_t s);
// the torus by ghost zones (capi.cpp: run_torus): wrap of a ring of any width, interior-to-interior copies
hipError_t launch_ring_wrap(int dtype, int nd, const int *dims, const int *ring, void *ptr, hipStream_t s);
hipError_t launch_copy_interior(int dtype, int nd, const int *dims, void *dst, const int *pad_dst, const void *src, const int *pad_src,
                                hipStream_t s);
const char *kernel_name_2d_fused2(const Plan &p);
// the same two applications per launch, row-streaming form (wave-autonomous column strips)
// (K = 2 or 4 applications per launch)
hipError_t launch_2d_stream(const Plan &p, int K, const double *in, double *out, int begin, int end, hipStream_t s);
const char *kernel_name_2d_stream(const Plan &p);
int stream_rows_per_chunk(const Plan &p, int K, int rows_total, int strips);  // resolved chunk height of a launch
int stream_strip_width(int K);
// K = 6, 4 or 2 applications per launch: workgroup-wide rows, levels pipelined over two groups of waves (kernels_2d_wg.hip)
hipError_t launch_2d_wg(const Plan &p, int K, const double *in, double *out, int begin, int end, hipStream_t s);
const char *kernel_name_2d_wg(const Plan &p);
void prepare_2d_wg(const Plan &p);  // one-time host work of the plan's instantiations (no launch)
int wg_strip_width(int K);
bool wg_layout_debug(const Plan &p, int K, int rows, int cus, int per_cu, int out[8]);  // host only: the chunks of a launch
hipError_t launch_3d(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
// two applications per launch, level 1 in LDS (fp64, reference boundary: level-1 halo = 0)
hipError_t launch_3d_fused2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
const char *kernel_name_3d_fused2(const Plan &p);
hipError_t launch_3d_stream(const Plan &p, int K, const double *in, double *out, const double *halo_src, int parity,
                            int begin, int end, hipStream_t s);
const char *kernel_name_3d_stream(const Plan &p);
// K = 4 (or 2) applications per launch with the levels in registers (star / exactly separable box taps, fp64, any extents)
hipError_t launch_3d_lanes(const Plan &p, int K, const double *in, double *out, int begin, int end, hipStream_t s, int begin2 = 0, int end2 = 0);
const char *kernel_name_3d_lanes(const Plan &p);
bool prepare_3d_lanes(const Plan &p);
int stream3_waves(const Plan &p, int K, int pipe);
// any size, any taps (odd innermost extents): one thread per point
hipError_t launch_2d_generic(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
hipError_t launch_3d_generic(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
const char *kernel_name_generic(const Plan &p);
hipError_t launch_3d_bf16(const Plan &p, const void *in, void *out, int begin, int end, hipStream_t s);
const char *kernel_name_3d_bf16(const Plan &p);
hipError_t launch_3d_bf16_fused2(const Plan &p, const void *in, void *out, int begin, int end, hipStream_t s);
const char *kernel_name_3d_bf16_fused2(const Plan &p);
// bf16, exactly separable box taps: K = 4 (or 2) applications per launch with the levels in registers (kernels_3d_bf16_lanes.hip)
hipError_t launch_3d_bf16_lanes(const Plan &p, int K, const void *in, void *out, int begin, int end, hipStream_t s, int begin2 = 0, int end2 = 0);
const char *kernel_name_3d_bf16_lanes(const Plan &p);
bool prepare_3d_bf16_lanes(const Plan &p);  // false: no workgroup of it fits a CU of the current device
// bf16 box, two applications per launch, in-plane passes on v_mfma_f32_16x16x32_bf16 (LORA_VARIANT_MFMA)
hipError_t launch_3d_bf16_mfma2(const Plan &p, const void *in, void *out, int begin, int end, hipStream_t s);
const char *kernel_name_3d_bf16_mfma2(const Plan &p);

// ---- reductions over a box of a padded array (kernels_reduce.hip; host side and geometry: reduce.cpp) ----------------
// The unit one lane loads: 16 bytes (two fp64 cells, eight bf16 cells) or 8 (fp64 rows of odd length).
enum ReduceKind { KIND_F64X2 = 0, KIND_F64X1 = 1, KIND_BF16X8 = 2, KIND_CELL = 3 };  // KIND_CELL: no pieces, a record's index is a cell's (the fold of a fused residual)
constexpr int kReduceMaxGroups = 1024;  // workgroups of a launch at most; record [kReduceMaxGroups] is the folded result
struct ReduceRecord {  // what a workgroup leaves: stats {min, max, sum, sum_sq | nonfinite}, diff {max_abs, sum_sq, a_abs_max | argmax, nonfinite}
    double f[4];
    long long i[2];
};
struct ReduceArgs {
    long total, chunk;              // pieces of the box; pieces per workgroup
    int ppr, e1;                    // pieces per row of the box; rows per outermost index
    int q0, col_lo, col_hi;         // first piece of a row; padded column range of the box (cells outside are masked)
    long off0;                      // cell offset of piece q0 of the box's first row
    long row_stride, plane_stride;  // in cells
    int dq, d1;                     // one stride of the lanes (reduce_threads() pieces) in digits: pieces, rows ...
    long step_off, row_carry, plane_carry;  // ... and as cell offsets: the stride, a piece carry, a row carry
};
int reduce_threads();
// The box lo[d] <= x < hi[d] in PADDED coordinates of a (1 x 1 x) ... array, outermost first as in Plan::dims: fills the
// launch arguments, the piece kind and the number of workgroups -- functions of dtype, extents and box alone.  False for
// an empty box.
bool reduce_geometry(const Plan &p, const int *lo, const int *hi, ReduceArgs &a, int &kind, int &groups);
// Each: the reduction launch (one record per workgroup into partial[0 .. groups)) and the fold into partial[kReduceMaxGroups].
hipError_t launch_reduce_stats(const ReduceArgs &a, int kind, int groups, const void *buf, ReduceRecord *partial, hipStream_t s);
hipError_t launch_reduce_diff(const ReduceArgs &a, int kind, int groups, const void *buf_a, const void *buf_b, ReduceRecord *partial,
                              hipStream_t s);
hipError_t launch_reduce_fold_cells(int groups, ReduceRecord *partial, hipStream_t s);
// sum of a * b: records {dot, sum |a b|, max |a| | nonfinite} over the cells whose product is finite (lora_plan_dot)
hipError_t launch_reduce_dot(const ReduceArgs &a, int kind, int groups, const void *buf_a, const void *buf_b, ReduceRecord *partial,
                             hipStream_t s);

// ---- one sweep's change, reduced in the sweep (kernels_residual.hip; tile geometry: residual_tiles.h) -----------------
struct ResidualTiles;
// Whether the plan has the fused residual kernel: 1D, the tiled 2D direct-variant and 3D fp64 kernels' plans, 3D bf16.
// A plan that carries a source has none: the source of lora_plan_residual_src is a call argument.
inline bool has_fused_residual(const Plan &p) {
    return !p.source && (p.ndim == 1 || p.dtype == LORA_BF16 || (!p.generic && (p.ndim == 3 || p.variant == LORA_VARIANT_DIRECT)));
}
// The records of `d = a - in` over the tiles of `rt`, one per workgroup into partial[0 .. rt.groups), and the fold:
// a = sweep(in), or with `f` (fp64 plans only; nullptr = none) a = fl(sweep(in) + f), f read at the reduced cells alone.
hipError_t launch_residual(const Plan &p, const ResidualTiles &rt, const void *in, const double *f, ReduceRecord *partial, hipStream_t s);

// ---- conjugate gradients on A = I - S (kernels_cg.hip; host side: cg.cpp) ---------------------------------------
// Whether the plan has the CG kernels: fp64 plans with the fused residual kernel (so: no source, an even innermost extent in
// 2D / 3D, the 2D direct variant).  Read-only option "cg".
inline bool has_cg(const Plan &p) { return p.dtype == LORA_F64 && has_fused_residual(p); }
// The scalars of a run, resident on the device; behind them in the same allocation the run's history: `cap` alphas, `cap` betas.
struct CgState {
    double rr, pq, alpha, beta, r_abs_max;  // r.r of the current residual, p.q of the last apply, rr / pq, rr' / rr, max |r|
    long long iteration, breakdown;         // iterations applied; sticky: pq or rr not finite, pq <= 0, a non-finite product (bits: CgHalt)
};
// The bits of CgState::breakdown, the word every launch of a run tests before it touches memory.  The CG driver only ever sets
// the first; the implicit stepper (cg.cpp) also sets the second when a step has met its stop rule and clears it behind the
// next step's start, so that the step's remaining launches are the same uniform early exit.
enum CgHalt { CG_HALT_BREAKDOWN = 1, CG_HALT_DONE = 2 };
enum CgOp { CG_OP_UPDATE = 0, CG_OP_DIRECTION = 1, CG_OP_START = 2 };
// what the fold does with the scalars: nothing; rr = the record lora_plan_dot's fold left, the rest reset; pq and alpha; rr, beta,
// the history and the iteration count
// the stepper's: THETA_INIT resets both states at the head of a run (no records read); THETA_START takes rr = rr0 from the
// start launch's records, clears `done` and the step's iteration count, thresh = fl(rtol2 rr0), done at once if rr0 == 0;
// THETA_UPDATE is UPDATE followed by the stop rule (rr' <= thresh, or the step's max_iters-th iteration) and the step's
// entry in the history
// the preconditioned drivers' (mg.cpp), whose rz = r.z lives in the PcgState behind the history while CgState::rr
// stays r.r: PCG_INIT resets the CgState at the head of a run (no records read); PCG_RZ0 takes rz from the record lora_plan_dot's
// fold left; PCG_APPLY is APPLY with alpha = rz / pq; PCG_UPDATE is UPDATE without beta (rr, the count, alpha into the history),
// PCG_THETA_UPDATE the same followed by the stepper's stop rule; PCG_RZ takes rz' from lora_plan_dot's record: beta = rz' / rz
// into the state and the history entry of the iteration just applied, rz = rz'
enum CgFold { CG_FOLD_PLAIN = 0, CG_FOLD_START = 1, CG_FOLD_APPLY = 2, CG_FOLD_UPDATE = 3, CG_FOLD_THETA_INIT = 4, CG_FOLD_THETA_START = 5,
              CG_FOLD_THETA_UPDATE = 6, CG_FOLD_PCG_INIT = 7, CG_FOLD_PCG_RZ0 = 8, CG_FOLD_PCG_APPLY = 9, CG_FOLD_PCG_UPDATE = 10,
              CG_FOLD_PCG_THETA_UPDATE = 11, CG_FOLD_PCG_RZ = 12 };
// The preconditioned drivers' scalar beside the CgState: in the same allocation, behind the `cap` alphas and `cap` betas.
struct PcgState {
    double rz, spare;  // r.z of the current residual
};
// The stepper's scalars beside the CgState, resident on the device; behind them in the same allocation the per-step history:
// `cap` iteration counts (long long), then `cap` final rr (double).
struct ThetaState {
    double rr0, thresh, rtol2;  // r.r at the step's start; fl(rtol2 rr0); fl(rtol rtol) from the host
    long long max_iters, steps_done, unconverged, cap;
};
// q = fl(p - sweep(p)) on the interior cells of the tiles of `rt` and the records of dot(p, q), one per workgroup (no fold)
hipError_t launch_apply_dot(const Plan &p, const ResidualTiles &rt, const double *d_p, double *d_q, const CgState *st, ReduceRecord *partial,
                            hipStream_t s);
// the pointwise kernels over the pieces of an interior box (reduce_geometry; kind must be KIND_F64X2):
//   CG_OP_UPDATE     g0 = x, g1 = r, g2 = p, g3 = q: x += coef p, r -= coef q, the records of dot(r, r) (no fold)
//   CG_OP_DIRECTION  g0 = p, g2 = r:                 p = r + coef p
//   CG_OP_START      g0 = r, g1 = p, g2 = x:         r = r - x, p = r
// With a state, coef is its alpha (UPDATE) / beta (DIRECTION) and a set breakdown flag makes the launch a no-op.
hipError_t launch_cg_pointwise(int op, const ReduceArgs &a, int kind, int groups, double *g0, double *g1, const double *g2, const double *g3,
                               double coef, const CgState *st, ReduceRecord *partial, hipStream_t s);
hipError_t launch_cg_fold(ReduceRecord *partial, int groups, CgState *st, int phase, int cap, hipStream_t s, ThetaState *ts = nullptr,
                          double rtol2 = 0.0, int max_iters = 0);

// ---- the implicit stepper's stencil launches (kernels_theta.hip; host side: cg.cpp).  Plans: has_cg().
// q = fl(fl(sigma p) - fl(tau sweep(p))) on the interior cells of the tiles of `rt` and the records of dot(p, q) (no fold)
hipError_t launch_apply_dot_shift(const Plan &p, const ResidualTiles &rt, const double *d_p, double *d_q, double sigma, double tau,
                                  const CgState *st, ReduceRecord *partial, hipStream_t s);
// r = p = fl(tau fl(fl(sweep(u) + f) - u)) (f == nullptr: no addition) on those cells and the records of dot(r, r) (no fold)
hipError_t launch_theta_start(const Plan &p, const ResidualTiles &rt, const double *d_u, const double *d_f, double tau, double *d_r,
                              double *d_p, const CgState *st, ReduceRecord *partial, hipStream_t s);
// out = fl(fl(sweep(u) + f) - u) (f == nullptr: no addition) on those cells: no record, no fold (lora_plan_defect)
hipError_t launch_defect(const Plan &p, const ResidualTiles &rt, const double *d_u, const double *d_f, double *d_out, hipStream_t s);

// ---- the whole small CG in one launch of one workgroup (kernels_cg_small.hip; host side: cg.cpp) -----------------
// Size admission.  A lane keeps x, r, p, q of its cells in registers: a 1024-lane workgroup has 128 VGPRs a lane, and four cells
// (32 VGPRs of state, the addresses and a tap sum beside them) stay far from spilling -- 4096 cells.  p in its ring of zeros and
// the waves' partial sums must fit 64 KiB of LDS, what a launch gets without asking for more and well inside the CU's 160 KiB,
// so that a workgroup of another stream still finds room beside it.  Admits 4 x 512, 32 x 32, 12 x 12 x 12; not 4 x 1024.
constexpr int kCgSmallCellsPerLane = 4;
constexpr long kCgSmallMaxCells = 1024L * kCgSmallCellsPerLane;
constexpr size_t kCgSmallMaxLds = 64 * 1024;
inline size_t cg_small_lds_bytes(const Plan &p) {  // 2 x 16 wave sums, then p with a ring of 3 (2D) / 1 (3D) zeros per side
    const double cells = p.ndim == 2 ? (p.dims[0] + 6.0) * (p.dims[1] + 6.0) : (p.dims[0] + 2.0) * (p.dims[1] + 2.0) * (p.dims[2] + 2.0);
    return cells > 1e9 ? (size_t) 1 << 40 : sizeof(double) * (32 + (size_t) cells);
}
// Whether lora_plan_cg_small takes the plan: the CG plans of 2D / 3D shapes that fit.  Read-only option "cg_small".
inline bool has_cg_small(const Plan &p) {
    if (!has_cg(p) || p.ndim < 2) return false;
    double cells = 1.0;
    for (int a = 0; a < p.ndim; ++a) cells *= p.dims[a];
    return cells <= (double) kCgSmallMaxCells && cg_small_lds_bytes(p) <= kCgSmallMaxLds;
}
// `iters` >= 1 iterations on the interiors of d_x and d_r (the residual); d_info: nullptr or {rr0, rr, iterations, halt}
hipError_t launch_cg_small(const Plan &p, double *d_x, double *d_r, int iters, double sigma, double tau, double *d_info, hipStream_t s);

// ---- geometric multigrid (kernels_mg.hip; host side: mg.cpp) ------------------------------------------------------
// The extents of the next coarser grid (lora_mg_coarse_dims): LORA_OK, LORA_EUNSUPPORTED for 1D or an extent below 4.
int mg_coarse_dims(int ndim, const int *dims, int *cdims);
// Whether the plan has the transfer kernels and the V-cycle driver: the CG plans of 2D / 3D shapes that can be coarsened once.
// Read-only option "mg".
inline bool has_mg(const Plan &p) {
    int c[3];
    return has_cg(p) && p.ndim >= 2 && mg_coarse_dims(p.ndim, p.dims, c) == LORA_OK;
}
// A fine grid of `dims` and the next coarser one of `cdims` (both with an even innermost extent), padded like a plan's arrays.
//   restrict     coarse = fl(coef sum_i (prod_a num_a(i_a, j_a)) fine[i]) on every interior coarse cell, num_a the integer
//                numerator (n + 1) - |(i + 1)(n_c + 1) - (j + 1)(n + 1)| where positive; coef = scale prod_a rho_a / (n_a + 1),
//                rounded once on the host
//   prolong_add  fine = fl(fine + fl(coef sum_j (prod_a num_a) coarse[j])) on every interior fine cell; coef = 1 / prod_a (n_a + 1)
hipError_t launch_mg_restrict(int ndim, const int *dims, const int *cdims, const double *d_fine, double *d_coarse, double scale, hipStream_t s);
hipError_t launch_mg_prolong_add(int ndim, const int *dims, const int *cdims, const double *d_coarse, double *d_fine, hipStream_t s);
// kernels_mg_fused.hip: coarse = what launch_defect of `p` (a plan with has_mg(); f may be nullptr) into a spare grid
// and launch_mg_restrict out of it leave on the interior of d_coarse, bit for bit, in ONE launch and without the spare grid
hipError_t launch_mg_defect_restrict(const Plan &p, const int *cdims, const double *d_u, const double *d_f, double *d_coarse, double scale,
                                     hipStream_t s);
// the driver's two pointwise launches over the interior of a grid of `dims`: a = fl(a - b) and a = fl(c b)
hipError_t launch_mg_sub(int ndim, const int *dims, double *d_a, const double *d_b, hipStream_t s);
hipError_t launch_mg_scale(int ndim, const int *dims, double *d_a, const double *d_b, double c, hipStream_t s);
// cg.cpp: the coarsest level of a cycle.  `iters` CG iterations on A = I - S of `plan` from d_x (whose halo is zero) with the
// first residual in the plan's own r grid (plan->cg[0], written by the caller): p = r with a zero halo, rr = r.r, then the
// iterations of lora_plan_run_cg_until through the same launches, no probe and no host wait.  *launches += what it enqueued.
// With (sigma, tau) other than (1, 1) the operator is sigma I - tau S: apply_dot_shift in place of apply_dot.
int cg_fixed_iterations(lora_plan *plan, void *d_x, int iters, double sigma, double tau, hipStream_t s, long *launches);
// cg.cpp: the fused defect launch over the whole interior of `p` (a plan without a source; f may be nullptr) -- what
// lora_plan_defect enqueues, for the V-cycle's internal plans
int defect_whole(const Plan &p, const double *d_u, const double *d_f, double *d_out, hipStream_t s);
int ensure_cg_grids(lora_plan *plan);  // cg.cpp: the plan's three CG grids and its state (lora_plan_prepare_cg's, unchecked)
int dirichlet_run_launches(lora_plan *plan, int times);  // capi.cpp: the launches of lora_plan_run(times) under the Dirichlet boundary, no graph
struct MgHierarchy;                    // mg.cpp: the levels a plan owns for lora_plan_run_mg_until
void mg_release(lora_plan *plan);      // mg.cpp: frees them (release_run_state)
// mg.cpp, for the preconditioned drivers of cg.cpp.  mg_admit: what lora_plan_mg_precondition refuses before a
// device is asked for (a bad `m` or pair: LORA_EINVAL; the plan, point symmetry, the level diagonals: LORA_EUNSUPPORTED);
// *levels = the depth of the hierarchy.  mg_prepare: the hierarchy for (m, sigma, tau) with every grid a cycle needs.
// mg_precondition: z = M r enqueued on `s`, nothing checked.  mg_owns: whether `buf` is one of the hierarchy's grids.
// mg_cost: the launches and bytes of the last cycle enqueued.
bool mg_bad(const lora_mg *m, double sigma, double tau);  // what mg_admit answers with LORA_EINVAL
int mg_admit(const lora_plan *plan, const lora_mg *m, double sigma, double tau, int *levels);
int mg_prepare(lora_plan *plan, const lora_mg *m, double sigma, double tau);
int mg_precondition(lora_plan *plan, const double *d_r, double *d_z, const lora_mg *m, double sigma, double tau, hipStream_t s);
bool mg_owns(const lora_plan *plan, const void *buf);
void mg_cost(const lora_plan *plan, long *launches, double *bytes);

// ---- sweeps with a source term, out = fl(acc + f) (kernels_step.hip: one application; kernels_2d_step2.hip: two, 2D) -------
// Plans whose `source` is set; the launch dispatcher picks them, nothing else does.
hipError_t launch_source(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
hipError_t launch_source2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s);
const char *source_kernel_name(const Plan &p);
const char *source2_kernel_name(const Plan &p);
// Whether a plan with a source fuses two applications per launch: 2D, direct variant, even innermost extent, reference or
// Dirichlet boundary, unless single sweeps were asked for.  Every other plan with a source runs single sweeps.
inline bool source_fuses_two(const Plan &p) {
    return p.ndim == 2 && p.variant == LORA_VARIANT_DIRECT && !p.generic && p.boundary != LORA_BC_PERIODIC && p.steps_per_launch_req != 1;
}

// ---- leapfrog steps, prev <- S(cur) + c prev in place (kernels_step.hip: one step; two per launch: kernels_2d_step2.hip in
// 2D, kernels_3d_step2.hip in 3D).  Picked by the leapfrog entries of leapfrog.cpp and by nothing else.
hipError_t launch_leapfrog(const Plan &p, const double *cur, double *prev, double c, int begin, int end, hipStream_t s);
hipError_t launch_leapfrog2_2d(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                               int end, hipStream_t s);
hipError_t launch_leapfrog2_3d(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                               int end, hipStream_t s);
inline hipError_t launch_leapfrog2(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                                   int end, hipStream_t s) {
    return p.ndim == 3 ? launch_leapfrog2_3d(p, prev, cur, out1, out2, c, begin, end, s)
                       : launch_leapfrog2_2d(p, prev, cur, out1, out2, c, begin, end, s);
}
// 0: no leapfrog kernel (bf16, the 2D matrix-pipe variant, a plan with a source); 1: single steps; 2: also the two-step launch
// (2D: direct variant, even innermost extent; 3D: even innermost extent and option leap3 on).
inline int leapfrog_depth(const Plan &p) {
    if (p.dtype != LORA_F64 || p.source || (p.ndim == 2 && p.variant != LORA_VARIANT_DIRECT)) return 0;
    if (p.ndim == 3) return p.leap3 && !p.generic ? 2 : 1;
    return p.ndim == 2 && !p.generic ? 2 : 1;
}

// ---- scaled leapfrog steps with a source, prev <- a (S(cur) + f) + c prev (kernels_step.hip: one step; two per launch:
// kernels_2d_step2.hip, kernels_3d_step2.hip).  f is a call argument (nullptr = none), never the plan's source; the plans are
// those of leapfrog_depth().  Picked by the *_leapfrog_src entries of leapfrog.cpp and by nothing else.
hipError_t launch_leapfrog_src(const Plan &p, const double *cur, double *prev, const double *f, double a, double c, int begin, int end,
                               hipStream_t s);
hipError_t launch_leapfrog2_src_2d(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                   double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s);
hipError_t launch_leapfrog2_src_3d(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                   double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s);
inline hipError_t launch_leapfrog2_src(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                       double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s) {
    return p.ndim == 3 ? launch_leapfrog2_src_3d(p, prev, cur, f, out1, out2, a1, c1, a2, c2, begin, end, s)
                       : launch_leapfrog2_src_2d(p, prev, cur, f, out1, out2, a1, c1, a2, c2, begin, end, s);
}

// ---- variable-coefficient wave steps, prev <- k S(cur) + b cur + c prev with k a padded grid (kernels_step.hip: one step;
// kernels_2d_wave2.hip: two per launch in 2D; kernels_3d_step2.hip: two per launch in 3D behind option wave3 -- option leap3
// alone leaves 3D wave runs at single steps).  k is a call argument.  Picked by the *_wave entries of leapfrog.cpp and by
// nothing else.
hipError_t launch_wave(const Plan &p, const double *cur, double *prev, const double *k, double b, double c, int begin, int end,
                       hipStream_t s);
hipError_t launch_wave2_2d(const Plan &p, const double *prev, const double *cur, const double *k, double *out1, double *out2, double b,
                           double c, int begin, int end, hipStream_t s);
hipError_t launch_wave2_3d(const Plan &p, const double *prev, const double *cur, const double *k, double *out1, double *out2, double b,
                           double c, int begin, int end, hipStream_t s);
inline hipError_t launch_wave2(const Plan &p, const double *prev, const double *cur, const double *k, double *out1, double *out2, double b,
                               double c, int begin, int end, hipStream_t s) {
    return p.ndim == 3 ? launch_wave2_3d(p, prev, cur, k, out1, out2, b, c, begin, end, s)
                       : launch_wave2_2d(p, prev, cur, k, out1, out2, b, c, begin, end, s);
}
// 0: no wave kernel (the plans of leapfrog depth 0); 2: also the two-step launch (2D: direct variant, even innermost extent;
// 3D: even innermost extent and option wave3 on); 1: single steps (every other plan).
inline int wave_depth(const Plan &p) {
    if (leapfrog_depth(p) == 0) return 0;
    if (p.ndim == 3) return p.wave3 && !p.generic ? 2 : 1;
    return p.ndim == 2 && !p.generic ? 2 : 1;
}

// ---- the launch dispatcher (capi.cpp): the one place that picks a launch's kernel ----------------------------
// One launch of `napps` applications over the outermost interior range [begin, end) and, in the same launch,
// [begin2, end2) (register-resident 3D kernels only; empty = none).
struct Apps {
    int napps = 1;
    int begin = 0, end = 0, begin2 = 0, end2 = 0;
    const void *halo = nullptr;  // three applications (3D): the buffer with the caller's halo (nullptr = d_in) ...
    int parity = 0;              // ... and the parity of the launch's first global step
    int depth = 0;               // the deepest launch the caller allows: 0 = the plan's own; a 1D run passes its run depth
    bool step2 = false;          // lora_plan_step2's two-application kernel rather than the plan's family at depth 2
};
// Whether the plan's kernels have a launch of `napps` applications (lora_plan_stepn_region's contract).
bool has_depth(const Plan &p, int napps);
// Validates buffers and ranges, launches, and turns a launch error into LORA_EHIP; LORA_EUNSUPPORTED (checked first) for a
// launch the plan's kernels do not have.
int launch_apps(const Plan &p, const Apps &a, const void *d_in, void *d_out, hipStream_t s);

const char *kernel_name_1d(const Plan &p);
const char *kernel_name_2d_direct(const Plan &p);
const char *kernel_name_2d_mfma(const Plan &p);
const char *kernel_name_3d(const Plan &p);
int region_granularity(const Plan &p);

void set_last_error(const char *what, hipError_t e);
void set_last_error_text(const char *text);
void set_last_run_info(const lora_run_info &info);  // what lora_last_run_info returns on this thread
void release_run_state(lora_plan *plan);            // capi.cpp: the one place that releases what a plan owns on a device (graph, torus, every DeviceGrid)
int admit_reduction(const void *a, const void *b, hipStream_t s);  // reduce.cpp: what every reduction entry checks before it touches the device
int reduction_range(const Plan &p, int &begin, int &end);  // reduce.cpp: the reductions' range rule: 1 = the whole interior (0, 0) or a proper range, 0 = an empty one, LORA_EINVAL = a bad one
int reduction_records(lora_plan *plan, ReduceRecord **out);  // reduce.cpp: the plan's records on the current device
bool interior_geometry(const Plan &p, int begin, int end, ReduceArgs &a, int &kind, int &groups, long long &count);  // reduce.cpp: reduce_geometry of the interior box of [begin, end) and its number of cells
int folded_record(const ReduceRecord *records, ReduceRecord &rec, hipStream_t s);  // reduce.cpp: the folded record back on the host (blocks)
int residual_whole(lora_plan *plan,const void *d_in, const void *d_f, lora_grid_diff *out, hipStream_t s);  // reduce.cpp: lora_plan_residual_src over the whole interior, unchecked (blocks)
int diff_whole(lora_plan *plan, const void *d_a, const void *d_b, lora_grid_diff *out, hipStream_t s);  // reduce.cpp: lora_plan_diff over the whole interior, unchecked (blocks)
// reduce.cpp: the plan's own single sweep with d_f (nullptr = none) as its source, d_out = fl(S(d_in) + f), on a copy of the plan's
// resolved state -- the caller's plan keeps its options, kernel name, signature and leapfrog depth
int sweep_with_source(const Plan &p, const void *d_f, const void *d_in, void *d_out, hipStream_t s);
// reduce.cpp: the probe of the CG, PCG, multigrid and Chebyshev drivers, the TRUE residual S(u) + f - u of the whole interior
// (blocks).  fused: residual_whole, no grid written; else sweep_with_source into d_scratch and diff_whole of it against d_u.
// Under the max norm every deciding field of the fused record is bit for bit the two-pass one's; sum_sq -- the RMS norm's -- is
// summed in another order there, so the callers keep the two passes for that norm.
int true_residual(lora_plan *plan, const void *d_u, const void *d_f, void *d_scratch, bool fused, lora_grid_diff *out, hipStream_t s);
int check_buffers(const void *a, const void *b);    // capi.cpp: LORA_EINVAL for a null buffer, LORA_EUNSUPPORTED for a misaligned one
int default_source_refused(const char *who);       // capi.cpp: LORA_EUNSUPPORTED while the thread has a default source (drivers that take none)
int attach_default_source(lora_plan *plan, size_t bytes, void **d_source);  // capi.cpp: upload the thread's default source (if any) and set it on the plan; *d_source is the caller's to hipFree, whatever the status
const char *run_label(int shape);                  // hostrun.cpp: the operator's first stdout line (e.g. 2d/gpu.cu:549)

// ---- what the entries of capi.cpp, leapfrog.cpp, chebyshev.cpp and reduce.cpp refuse and report alike ----------------------
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
// the halo widths of a padded grid of `ndim` dimensions, outermost first: the pads launch_copy_interior takes for a plan's grid
inline const int *interior_pads(int ndim) {
    static const int pads[3][3] = {{4, 0, 0}, {4, 4, 0}, {1, 2, 4}};
    return pads[ndim - 1];
}
// I - S and sigma I - tau S are symmetric when the taps are point-symmetric (what CG and multigrid need)
inline bool taps_symmetric(const double *w, int ntaps) {
    for (int t = 0; t < ntaps; ++t)
        if (w[t] != w[ntaps - 1 - t]) return false;
    return true;
}
inline int unsupported(const char *text) {
    set_last_error_text(text);
    return LORA_EUNSUPPORTED;
}
inline int hip_status(hipError_t e, const char *what) {  // LORA_OK, or LORA_EHIP and the error as the thread's text
    if (e == hipSuccess) return LORA_OK;
    set_last_error(what, e);
    return LORA_EHIP;
}
inline int no_device() {
    set_last_error_text("no HIP device visible");
    return LORA_ENODEVICE;
}
// reduce.cpp: a lora_until's schedule (check_every, max_times) / any of its fields is out of range
bool bad_until_schedule(const lora_until *u);
bool bad_until(const lora_until *u);
// reduce.cpp: one check of an until-loop, its probe in r->last: counts it, takes the norm, marks diverged or else converged;
// whether the loop stops
bool until_decide(const lora_until *u, lora_until_result *r);

// ---- a device grid a plan owns (capi.cpp): allocated on first need, kept while size and device match, freed by
// release_run_state ----------------------------------------------------------------------------------------------------------
struct DeviceGrid {
    void *ptr = nullptr;
    size_t bytes = 0;
    int device = -1;
    bool ready(size_t want) const;        // a grid of `want` bytes on the current device is there (no allocation)
    // ... or is now, in place of what was held; false: no grid (the holder is empty).  A fresh grid is NOT initialised: no
    // stream is known here, and a hipMemset on the null stream returns before it has run and orders nothing against the
    // caller's non-blocking stream ("Stream ordering").  Every driver writes each cell of its grid, on its caller's
    // stream, before anything reads it.
    bool ensure(size_t want);
    void release();
};

// ---- what the host-buffer operators share (hostrun.cpp): the device check, the plan, N padded grids, a stream of the
// operator's own, the two clocks, the run info and the reference's three stdout lines.  lora_run_host_dtype, _until, _leapfrog
// and _chebyshev keep their uploads, warm-up, prepare call, the timed call between tic() and toc(), and their download.  The
// five source solvers (lora_run_host_cg, _theta, _pcg, _theta_mg, _mg) go through open_solver(), ready() and timed(), and
// keep their checks, their prepare and warm-up lines between the first two, the driver call and the grids-moved figure.
struct HostRun {
    lora_plan *plan = nullptr;
    void *b[3] = {nullptr, nullptr, nullptr};  // alloc(): padded grids
    void *src = nullptr;                       // the thread's default source on the device (attach_default_source)
    hipStream_t s = nullptr;
    size_t esize = 0, bytes = 0;               // of a cell, of a padded grid
    ~HostRun();
    int open(int shape, int dtype, const int *dims, const double *params);  // LORA_ENODEVICE, or what plan creation says
    hipError_t alloc(int n);  // starts the total clock, then n grids; a failure leaves no sticky error
    hipError_t stream();      // non-blocking: launch-bound runs are replayed from a hipGraph, which the legacy default stream cannot capture
    void tic();
    void toc();
    // after the download: `steps` steps that each moved `grids_moved` grids; LORA_OK
    int finish(int steps, double grids_moved, int steps_per_launch, int quiet, lora_run_info *info);
    // a source solver's start: open() as fp64, alloc() of the iterate's grid b[0] and, with a source, its grid b[1], both uploaded
    int open_solver(int shape, const int *dims, const double *params, const double *in, const double *source);
    // behind the operator's prepare and warm-up (whose launches go to the null stream): stream(), then a device synchronise
    int ready();
    // the timed region: tic(), `run` (the driver call on `s`), a stream synchronise, toc(); then b[0] into `out`
    template <class Run>
    int timed(double *out, Run run) {
        tic();
        if (int rc = run()) return rc;
        return timed_end(out);
    }
    int timed_end(double *out);
    int shape = 0;
    double points = 1.0;              // interior points
    long long ticks[3] = {0, 0, 0};  // steady_clock: alloc(), tic(), toc()
};

}  // namespace lora

struct lora_plan {
    lora::Plan p;
    // hipGraph of the last lora_plan_run (launch-bound small grids): replayed while buffers / step count match
    hipGraphExec_t graph_exec = nullptr;
    void *graph_buf[2] = {nullptr, nullptr};
    int graph_times = -1;
    unsigned graph_epoch = 0;  // value of p.epoch the graph was captured at
    bool capturing = false;    // lora_plan_run is capturing its launches: no allocations meanwhile
    // the periodic option's fused runs (run_torus): a plan of the grid extended by a ghost zone on every side and the ghost
    // widths; rebuilt, with its two buffers below, when the plan's taps / options or the device change
    lora_plan *torus = nullptr;
    int torus_device = -1;
    int torus_ghost[3] = {0, 0, 0};
    unsigned torus_epoch = 0;
    bool torus_tried = false;  // at torus_epoch: the answer was already "no" (grid too small, no fused kernel, no memory)
    // Grids allocated on first need, each keyed on its own size and device and used by its driver alone:
    lora::DeviceGrid scratch;       // lora_plan_run: one more padded grid for an odd number of fused launches (a cached graph holds its address)
    lora::DeviceGrid torus_buf[2];  // run_torus: the extended grid's two buffers (keyed by the torus fields above)
    lora::DeviceGrid records;       // reduce.cpp: the reductions' records, one per workgroup and the folded one (not zeroed)
    lora::DeviceGrid leap[2];       // lora_plan_run_leapfrog[_src]: the two scratch grids, both or neither
    lora::DeviceGrid cheb_probe;    // lora_plan_run_chebyshev_until: S(u) + f of the newest level, for the two-pass probe (the RMS norm, plans without the fused residual kernel)
    lora::DeviceGrid cg[3];         // lora_plan_run_cg_until: r, p, q -- all three or none
    lora::DeviceGrid cg_state;      // ... its CgState and, behind it, the history of cg_cap alphas and cg_cap betas
    int cg_cap = 0;
    lora::DeviceGrid theta_state;   // lora_plan_run_theta: its ThetaState and, behind it, the history of theta_cap steps
    int theta_cap = 0;
    lora::MgHierarchy *mg = nullptr;  // lora_plan_run_mg_until: the level plans and their grids (mg.cpp; freed by mg_release)
    lora::DeviceGrid pcg_z;           // lora_plan_run_pcg_until, lora_plan_run_theta_mg: z = M r, beside the CG set
};
