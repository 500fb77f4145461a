/*
 * lorastencil.h -- C ABI of the MI355X-native low-rank stencil engine (liblorastencil_hip.so).
 *
 * This is the drop-in boundary for the hot path of zondie17/LoRAStencil: the stencil sweep and
 * its time-step driver behind `lorastencil_{1d,2d,3d} shape input_size time_size`.  Plain C,
 * plain pointers and sizes, no C++/torch types.  Every entry point names the reference
 * interface it replaces (file:line under /root/reference/src/).
 *
 * Three groups:
 *   A. host-buffer operators  -- one-to-one replacements of the reference's seven gpu_*()
 *      functions (same argument meaning, padded host arrays in and out, same stdout lines);
 *   B. device-resident plans  -- the same sweep on caller-owned device buffers and a caller
 *      stream (what bench.py, the multi-GPU slab driver and the CLIs are built on);
 *   C. host helpers on the path -- params tables, the low-rank factor precompute, the
 *      glibc-rand() fill of the reference harness.
 *
 * Error model: every function returns LORA_OK (0) or a negative LORA_E* code and never exits
 * the process (the reference prints and exit(1)/abort()s: 2d_utils.h:6-36).  The C++ shims in
 * lorastencil_ref_shims.h restore the reference's print-and-exit behaviour on top of this.
 */
#ifndef LORASTENCIL_H
#define LORASTENCIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_VERSION 100

/* ---- status codes ---------------------------------------------------------------------- */
#define LORA_OK 0
#define LORA_EINVAL (-1)       /* bad shape / null pointer / negative size               */
#define LORA_EUNSUPPORTED (-2) /* size/dtype/variant combination the kernels cannot take       */
#define LORA_EHIP (-3)         /* a HIP runtime call failed (see lora_last_error())        */
#define LORA_ENOMEM (-4)
#define LORA_ENODEVICE (-5) /* no HIP device visible: the engine has NO CPU fallback     */

/* ---- shapes: the CLI `shape` argument (README.md:37-48) ---------------------------------- */
typedef enum lora_shape {
    LORA_1D1R = 0,     /* 1d_utils.h:38-42 star_1d1r */
    LORA_1D2R = 1,     /* star_1d2r */
    LORA_STAR2D1R = 2, /* 2d_utils.h:38-44 star_2d1r */
    LORA_BOX2D1R = 3,  /* box_2d1r (served by the box2d3r operator, 2d/main.cu:276-279) */
    LORA_STAR2D3R = 4, /* star_2d3r */
    LORA_BOX2D3R = 5,  /* box_2d3r */
    LORA_STAR3D1R = 6, /* 3d_utils.h:39-42 star_3d1r */
    LORA_BOX3D1R = 7,  /* box_3d1r */
    LORA_NUM_SHAPES = 8
} lora_shape;

typedef enum lora_dtype {
    LORA_F64 = 0, /* the reference's only type (DATA_TYPE double, 2d_utils.h:1) */
    LORA_BF16 = 1 /* NEW (no reference counterpart): bf16 storage, fp32 accumulation in tap order, one
                     round-to-nearest-even per sweep; 3D shapes only, innermost extent a multiple of 8 */
} lora_dtype;

/* Kernel formulation of one sweep (B: lora_plan_set_variant). */
typedef enum lora_variant {
    LORA_VARIANT_AUTO = 0,   /* what the roofline evidence in DESIGN.md picked per shape           */
    LORA_VARIANT_DIRECT = 1, /* LDS-tiled direct taps on the fp64 vector FMA pipe                  */
    LORA_VARIANT_MFMA = 2    /* low-rank (U X) V products on v_mfma_f64_16x16x4 (2D shapes only)   */
} lora_variant;

/* What the halo cells hold between sweeps of the time-step driver (lora_plan_run and the host operators).
 * Only LORA_BC_REFERENCE is behaviour of the reference; the other two are SURVEY section 8f-3 options. */
typedef enum lora_boundary {
    LORA_BC_REFERENCE = 0, /* halo cells are never written: sweep i reads the halo of buffer i % 2 -- the caller's
                              values at even steps, the second buffer's (zeros) at odd ones            */
    LORA_BC_DIRICHLET = 1, /* halo cells keep the caller's input values at every time level                        */
    LORA_BC_PERIODIC = 2   /* the grid is a torus: before every sweep each halo cell is refreshed from the interior
                              cell it is a periodic image of (every extent must be >= its halo width)              */
} lora_boundary;

/* Number of taps in `params` / weights for a shape: 9 (1D), 49 (2D), 27 (3D). */
int lora_shape_ntaps(int shape);
/* Number of interior dimensions of a shape (1, 2 or 3), 0 for an unknown shape. */
int lora_shape_ndim(int shape);
/* Parse the CLI spelling ("star2d1r", ...) -> shape id, or LORA_EINVAL. */
int lora_shape_from_name(const char *name);
/* The spelling the reference prints in its INFO line ("star_2d1r", 2d/main.cu:5-10). */
const char *lora_shape_info_name(int shape);
/* Padded element count: 1D n+8; 2D (m+8)(n+8); 3D (h+2)(m+4)(n+8) (2d/main.cu:217-221). */
size_t lora_padded_count(int shape, const int *dims);
/* GStencil/s accounting factor F the reference multiplies by. */
int lora_shape_gstencil_factor(int shape);

const char *lora_strerror(int status);
/* Text of the last HIP failure on this thread ("" if none). */
const char *lora_last_error(void);
/* Number of visible HIP devices (0 if none; never fails). */
int lora_device_count(void);

/* ========================================================================================
 * A. Host-buffer operators: drop-in for the reference's gpu_*().
 *
 *   in, out : caller-owned PADDED host arrays (1D n+8; 2D (m+8)(n+8); 3D (h+2)(m+4)(n+8)),
 *             row-major; the whole padded `in` is read (halo values matter), the whole padded
 *             `out` is written (1D: all but the last element, 1d/gpu_1r.cu:134).
 *   params  : 9 / 49 / 27 doubles, row-major, centre at 4 / 24 / 13.  Honoured exactly as far as
 *             the reference honours them (ignored by star2d1r and star3d1r; box3d1r reads
 *             params[0..2]; box2d goes through the pyramid factoriser).
 *   times   : number of kernel applications; result = ping-pong buffer [times % 2].
 *   Side effect: prints the reference's three stdout lines (label, Time, GStencil/s).
 *   Device memory is allocated and freed inside the call.
 * ====================================================================================== */
int lora_gpu_1d1r(const double *in, double *out, const double *params, int times, int input_n);      /* gpu_1d1r      1d_utils.h:45, 1d/gpu_1r.cu:90   */
int lora_gpu_1d2r(const double *in, double *out, const double *params, int times, int input_n);      /* gpu_1d2r      1d_utils.h:47, 1d/gpu_2r.cu:91   */
int lora_gpu_star_2d1r(const double *in, double *out, const double *params, int times, int input_m,
                       int input_n);                                                                 /* gpu_star_2d1r 2d_utils.h:47, 2d/gpu.cu:484     */
int lora_gpu_star_2d3r(const double *in, double *out, const double *params, int times, int input_m,
                       int input_n);                                                                 /* gpu_star_2d3r 2d_utils.h:49, 2d/gpu.cu:426     */
int lora_gpu_box_2d3r(const double *in, double *out, const double *params, int times, int input_m,
                      int input_n);                                                                  /* gpu_box_2d3r  2d_utils.h:51, 2d/gpu.cu:276     */
int lora_gpu_box_3d1r(const double *in, double *out, const double *params, int times, int input_h,
                      int input_m, int input_n);                                                     /* gpu_box_3d1r  3d_utils.h:44, 3d/gpu_box.cu:143 */
int lora_gpu_star_3d1r(const double *in, double *out, const double *params, int times, int input_h,
                       int input_m, int input_n);                                                    /* gpu_star_3d1r 3d_utils.h:47, 3d/gpu_star.cu:136 */

/* Timing of the last host-buffer run, as the reference measures it (steady_clock around the
 * launch loop + one device sync, transfers excluded: 2d/gpu.cu:542-552), plus the transfer
 * inclusive time. */
typedef struct lora_run_info {
    double sweep_seconds;    /* launch loop + sync                      */
    double total_seconds;    /* H2D + sweep + D2H                       */
    double gstencils;        /* points*times/sweep_seconds/1e9 (F = 1)  */
    double gstencils_refconv; /* the same times the reference's factor F */
    double hbm_gbs;          /* algorithmic 2*sizeof(T) bytes per point */
    int variant;             /* lora_variant actually used              */
    int steps_per_launch;    /* 1 unless temporal fusion is active      */
} lora_run_info;

/* Generic form of group A (shape chosen at run time).  `quiet` != 0 suppresses the stdout
 * lines; `info` may be NULL. */
int lora_run_host(int shape, const double *in, double *out, const double *params, int times, const int *dims,
                  int quiet, lora_run_info *info);
/* The same for a given element type: `in` / `out` are padded host arrays of doubles (LORA_F64) or of bf16 bit
 * patterns in uint16_t (LORA_BF16). */
int lora_run_host_dtype(int shape, int dtype, const void *in, void *out, const double *params, int times,
                        const int *dims, int quiet, lora_run_info *info);
/* lora_run_host_dtype with the run-until-steady driver of group B (lora_plan_run_until: see there for `u` and `r`) in place
 * of a fixed number of sweeps: `out` receives level r->times_done; the three lines and lora_run_info are computed from
 * times_done, the timed region holding the sweeps and their checks. */
struct lora_until;
struct lora_until_result;
int lora_run_host_until(int shape, int dtype, const void *in, void *out, const double *params, const int *dims,
                        const struct lora_until *u, struct lora_until_result *r, int quiet, lora_run_info *info);
/* Leapfrog stepping u(t+1) = S(u(t)) + c u(t-1) on host arrays (fp64; see lora_plan_run_leapfrog in group B): uploads the
 * padded host arrays `in_cur` (level 0) and `in_prev` (level -1), runs `times` steps with lora_plan_run_leapfrog and copies
 * level `times` (the whole padded array) to `out`.  Prints the operator's three lines
 * unless `quiet`; fills lora_run_info with hbm_gbs counting 3 x 8 bytes per point and step and steps_per_launch = the plan's
 * leapfrog depth.  LORA_EUNSUPPORTED while the thread has a default source (lora_set_default_source). */
int lora_run_host_leapfrog(int shape, const double *in_cur, const double *in_prev, double *out, const double *params, double c,
                           int times, const int *dims, int quiet, lora_run_info *info);
/* Variable-coefficient wave steps u(t+1) = kappa(x) S(u(t)) + b u(t) + c u(t-1) on host arrays (fp64; see lora_plan_run_wave in
 * group B): uploads the padded host arrays `in_cur` (level 0), `in_prev` (level -1) and `kappa` (the coefficient grid, laid out
 * like them; its halo is never read) outside the timed region, runs `times` steps with lora_plan_run_wave and copies level
 * `times` (the whole padded array) to `out`.  With laplacian != 0 the operator runs on the zero-sum form of its taps: after the
 * plan is opened its centre tap (index 4 / 24 / 13 in 1D / 2D / 3D) is replaced by centre - s, s the sum of all taps accumulated
 * sequentially in table order in fp64 (lora_plan_get_weights / lora_plan_set_weights), so b = 2, c = -1 is
 * 2 u - u- + kappa L u.  Prints the operator's three lines unless `quiet`; fills lora_run_info with hbm_gbs counting 4 x 8 bytes
 * per point and step and steps_per_launch = the plan's wave depth.  LORA_EINVAL for a null array, times < 0, a non-finite b or c;
 * LORA_EUNSUPPORTED while the thread has a default source (lora_set_default_source). */
int lora_run_host_wave(int shape, const double *in_cur, const double *in_prev, const double *kappa, double *out, const double *params,
                       double b, double c, int laplacian, int times, const int *dims, int quiet, lora_run_info *info);
/* The Chebyshev semi-iteration for u = S(u) + f on host arrays (fp64; see lora_plan_run_chebyshev_until in group B): uploads
 * the padded host array `in` as BOTH levels and `source` (a padded host array of f, or NULL: none) beside it, runs `times` steps
 * of lora_plan_run_leapfrog_src with lora_chebyshev_coeffs(rho, 1, times) -- or, with `u` not NULL, lora_plan_run_chebyshev_until
 * (`times` is then ignored, `r` must not be NULL) -- and copies the newest level (the whole padded array) to `out`.  With
 * u == NULL, `r` may be NULL; if it is not, r->times_done = times.  Prints the operator's three lines unless `quiet`; fills
 * lora_run_info with hbm_gbs counting 4 x 8 bytes per point and step with a source and 3 x 8 without, and steps_per_launch = the
 * plan's leapfrog depth; the timed region holds the steps and their probes.  LORA_EINVAL unless 0 <= rho < 1;
 * LORA_EUNSUPPORTED while the thread has a default source (lora_set_default_source): the source is an argument here. */
int lora_run_host_chebyshev(int shape, const double *in, const double *source, double *out, const double *params, double rho,
                            int times, const struct lora_until *u, struct lora_until_result *r, const int *dims, int quiet,
                            lora_run_info *info);
/* Conjugate gradients for u = S(u) + f on host arrays (fp64; see lora_plan_run_cg_until in group B): uploads the padded host
 * array `in` (the start iterate, its halo the boundary values) and `source` (a padded host array of f, or NULL: none) outside
 * the timed region, runs lora_plan_run_cg_until and copies the iterate (the whole padded array) to `out`.  `u` and `r` must
 * not be NULL.  Prints the operator's three lines unless `quiet`; fills lora_run_info with hbm_gbs counting 11 x 8 bytes per
 * point and iteration and steps_per_launch = 1; the timed region holds the start-up, the iterations and their probes.
 * LORA_EUNSUPPORTED for the plans lora_plan_run_cg_until refuses and while the thread has a default source
 * (lora_set_default_source): the source is an argument here. */
struct lora_cg_result;
int lora_run_host_cg(int shape, const double *in, const double *source, double *out, const double *params, const struct lora_until *u,
                     struct lora_cg_result *r, const int *dims, int quiet, lora_run_info *info);
/* Implicit time steps of du/dt = S(u) + f - u on host arrays (fp64; see lora_plan_run_theta in group B): uploads the padded
 * host array `in` (level 0, its halo the boundary values) and `source` (a padded host array of f, or NULL: none) outside the
 * timed region, runs lora_plan_run_theta over `steps` steps and copies the last level (the whole padded array) to `out`.
 * `result` must not be NULL.  Prints the operator's three lines unless `quiet`, counting STEPS; fills lora_run_info with
 * steps_per_launch = 1 and hbm_gbs counting, per point and step, 3 x 8 bytes for the step's start (4 x 8 with a source) and
 * 11 x 8 for each of its iterations on average; the timed region holds every step and the steady-state probe.  Argument rules
 * and LORA_EUNSUPPORTED as lora_plan_run_theta, and LORA_EUNSUPPORTED while the thread has a default source
 * (lora_set_default_source): the source is an argument here. */
struct lora_theta_result;
int lora_run_host_theta(int shape, const double *in, const double *source, double *out, const double *params, double theta, double tau,
                        int steps, int max_iters, double rtol, const int *dims, int quiet, lora_run_info *info,
                        struct lora_theta_result *result);
/* Multigrid V-cycles for u = S(u) + f on host arrays (fp64, 2D and 3D; see lora_plan_run_mg_until in group B): uploads the
 * padded host array `in` (the start iterate, its halo the boundary values) and `source` (a padded host array of f, or NULL: none)
 * outside the timed region, runs lora_plan_prepare_mg and then, timed, lora_plan_run_mg_until, and copies the iterate (the
 * whole padded array) to `out`.  `m`, `u` and `r` must not be NULL.  Prints the operator's three lines unless `quiet`, counting
 * CYCLES; fills lora_run_info with steps_per_launch = 1 and hbm_gbs from the bytes of one cycle as lora_plan_mg_cycle_cost
 * counts them -- per launch actually enqueued, 8 bytes for every interior cell of every grid it reads or writes (the padded
 * grid for a zeroing), summed over the levels; the probes are not counted.  The timed region holds the cycles and their
 * probes.  LORA_EUNSUPPORTED for what lora_plan_run_mg_until refuses and while the thread has a default source
 * (lora_set_default_source): the source is an argument here. */
struct lora_mg;
struct lora_mg_result;
int lora_run_host_mg(int shape, const double *in, const double *source, double *out, const double *params, const struct lora_mg *m,
                     const struct lora_until *u, struct lora_mg_result *r, const int *dims, int quiet, lora_run_info *info);
/* Multigrid-preconditioned conjugate gradients for u = S(u) + f on host arrays (fp64, 2D and 3D; lora_plan_run_pcg_until in
 * group B): as lora_run_host_mg, with lora_plan_prepare_pcg and one probe outside the timed region and lora_plan_run_pcg_until
 * inside it.  `steps` of the printed lines are ITERATIONS; hbm_gbs from the bytes of one iteration: the cycle's tally
 * (lora_plan_mg_cycle_cost) plus thirteen grids for the CG passes.  LORA_EINVAL also unless m->pre == m->post >= 1. */
struct lora_pcg_result;
int lora_run_host_pcg(int shape, const double *in, const double *source, double *out, const double *params, const struct lora_mg *m,
                      const struct lora_until *u, struct lora_pcg_result *r, const int *dims, int quiet, lora_run_info *info);
/* lora_run_host_theta with every step's solve preconditioned (lora_plan_run_theta_mg in group B): the hierarchy for the step's
 * operator is built outside the timed region; the timed region holds the run with its state read-backs every `check_every`
 * iterations.  hbm_gbs from counted bytes: per step the start, one cycle, the copy and the dot, per iteration a cycle and the
 * thirteen grids of lora_run_host_pcg. */
int lora_run_host_theta_mg(int shape, const double *in, const double *source, double *out, const double *params, double theta, double tau,
                           int steps, int max_iters, double rtol, const struct lora_mg *m, int check_every, const int *dims, int quiet,
                           lora_run_info *info, struct lora_theta_result *result);
/* lora_run_info of the last group-A call on this thread (what the CLIs print after the reference's lines). */
int lora_last_run_info(lora_run_info *info);

/* ========================================================================================
 * B. Device-resident plans.
 *    A plan fixes shape, interior dims, weights and kernel variant; it owns no grid memory.
 *    Buffers are PADDED device arrays laid out like the host arrays of group A; `stream` is a
 *    hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous.
 *    Stream ordering: everything a call enqueues -- kernels, halo copies, resets and wraps, the copies in and out of the
 *    extended periodic grid, a graph launch, record read-backs -- is ordered on `stream` and on no other stream, the null
 *    stream included; a non-blocking stream with work pending on other streams is served as well as an idle device.  The
 *    grids a plan allocates on first need (scratch grid, leapfrog grids, probe grid, records, extended periodic grids) are
 *    allocated inside the call (a hipMalloc, on the host) and are NOT initialised by it: the call writes every cell of them
 *    on `stream` before it reads it, so first-need allocation waits for no stream and leaves no work on any other one.
 *    The lora_plan_prepare_* calls only move that hipMalloc out of a timed region.  The entries that return a result to
 *    the host (stats, diff, residual, residual_src, the until-drivers) wait for `stream`, not for the device.
 *    (tests/test_gpu_stream_order.py; DESIGN section 7, "Stream ordering".)
 *    Alignment: every buffer given to a launch or a run must be 16-byte aligned (LORA_EUNSUPPORTED otherwise) and need
 *    not be more -- a sub-array of a bigger allocation will do.  No kernel reads or writes global memory in pieces wider
 *    than 16 bytes, and each piece sits at a multiple of its width from the buffer's base (of 8 bytes on the paths that
 *    take odd innermost extents).  Nothing outside [base, base + lora_plan_padded_bytes) is written, and nothing read
 *    there reaches a result.
 *    Different plans may be used from different threads at the same time; one plan must not be (it caches the
 *    hipGraph of its last run and its options are plain fields).
 * ====================================================================================== */
typedef struct lora_plan lora_plan;

/* params -> effective weights exactly like the reference operator (incl. the low-rank factor
 * precompute for box2d).  params == NULL uses the reference harness's table for the shape. */
int lora_plan_create(lora_plan **plan, int shape, int dtype, const int *dims, const double *params);
/* Replace the taps (9/49/27 doubles) applied per sweep, bypassing the params mapping
 * (normalised-weights mode). */
int lora_plan_set_weights(lora_plan *plan, const double *weights, int count);
int lora_plan_get_weights(const lora_plan *plan, double *weights, int count);
int lora_plan_set_variant(lora_plan *plan, int variant);
/* Boundary condition applied by lora_plan_run (lora_boundary; lora_plan_step* stay raw sweeps). */
int lora_plan_set_boundary(lora_plan *plan, int boundary);
/* Boundary condition given to plans created afterwards on this thread, i.e. also to the host operators of group A
 * (what the CLIs' --bc flag sets).  Returns the previous value. */
int lora_set_default_boundary(int boundary);
/* A source term: while `d_source` is set, every application of the plan is u <- S(u) + f on the interior cells of the swept
 * range -- out = fl(acc + f), where acc has exactly the bits the plan's single sweep without a source stores and + f is one
 * separate fp64 addition.  f is a caller-owned device array laid out as a padded grid of the plan; its halo cells are never
 * used, nothing outside [d_source, d_source + lora_plan_padded_bytes) is read, and it is never written.  The plan borrows
 * the pointer (lora_plan_destroy frees nothing of it); NULL removes the source, after which the plan resolves exactly as
 * before.  A single source sweep equals "plain sweep, then + f on the interior" bit for bit; a zero source equals no source as
 * numbers, not necessarily as bits (-0.0 + 0.0 = +0.0).  Halo cells of the output are never written; in a fused launch the
 * source adds to interior cells of the intermediate level only.
 *   With a source, option "steps_per_launch" reads 2 for 2D plans of the direct variant with an even innermost extent under
 * the reference and Dirichlet boundaries (1 if 1 was requested), and 1 for every other plan; the launch entries answer
 * LORA_EUNSUPPORTED for any other depth.  Option "source" reads 1, "fused_residual" 0: lora_plan_residual answers
 * LORA_EUNSUPPORTED, lora_plan_run_until probes with a step (which includes the source) and a difference.  A launch whose
 * d_out is the source is LORA_EINVAL.  A cached graph is dropped (it holds the old pointer).
 *   LORA_EINVAL for a null plan; LORA_EUNSUPPORTED for a pointer that is not 16-byte aligned, for a LORA_BF16 plan and for a
 * 2D plan of the LORA_VARIANT_MFMA variant -- and lora_plan_set_variant(plan, LORA_VARIANT_MFMA) on a plan that has a source
 * answers LORA_EUNSUPPORTED and leaves the plan as it was.  Needs no device: the pointer is only stored. */
int lora_plan_set_source(lora_plan *plan, const void *d_source);
/* The source given to the plans of the host operators of group A called afterwards on this thread: a padded HOST array of the
 * operator's grid (it stays the caller's; NULL = none).  lora_run_host / lora_run_host_dtype / lora_run_host_until for
 * LORA_F64 upload it beside the grid, outside the timed region; with one set, LORA_BF16 runs, lora_run_host_multi and
 * lora_run_host_blocks answer LORA_EUNSUPPORTED.  lora_run_info.hbm_gbs then counts 3 x sizeof(T) bytes per point and sweep.
 * Returns the previous value. */
const double *lora_set_default_source(const double *padded_host_source);
/* Normalised-weights mode for plans created afterwards on this thread, i.e. also for the host operators of group A
 * (what the CLIs' --normalize flag sets): the operator's effective taps are divided by their sum, so that runs longer
 * than the fp64 range of the reference's integer taps allows stay finite (box2d3r overflows at step ~129, SURVEY B7;
 * BASELINE config 3 asks for 200).  Not reference behaviour.  Returns the previous value. */
int lora_set_default_normalize(int on);
/* Option "leap3" (below) of the plans created afterwards on this thread, i.e. also of lora_run_host_leapfrog and
 * lora_run_host_chebyshev (what lorastencil_3d's --leap3 flag sets).  Returns the previous value. */
int lora_set_default_leap3(int on);
/* Option "wave3" (below) of the plans created afterwards on this thread, i.e. also of lora_run_host_wave (what
 * lorastencil_3d's --wave3 flag sets).  Returns the previous value. */
int lora_set_default_wave3(int on);
/* Option "coarse1" (below) of the plans created afterwards on this thread, i.e. also of lora_run_host_mg, lora_run_host_pcg and
 * lora_run_host_theta_mg (what the CLIs' --coarse1 flag sets); never of the internal plans of a multigrid hierarchy.  Returns
 * the previous value. */
int lora_set_default_coarse1(int on);
/* Option "mgfuse" (below) of the plans created afterwards on this thread, i.e. also of lora_run_host_mg, lora_run_host_pcg and
 * lora_run_host_theta_mg (what the CLIs' --mgfuse flag sets); never of the internal plans of a multigrid hierarchy.  Returns
 * the previous value. */
int lora_set_default_mgfuse(int on);
/* Integer options.  Results never depend on them except where stated.
 *   steps_per_launch  0 auto / 1 / 2 (2D also 4 with the row-streaming kernel and 6 with the workgroup-row kernel, 3D fp64
 *                     also 3 with the plane-streaming kernel, 1D also 4, 8, 16, 32) : applications per launch in
 *                     lora_plan_run (temporal fusion).  2D auto: 6 (reference boundary; what six leave of a run is covered by
 *                     one launch of four and / or two), plain 49-tap tables included; 4 under the Dirichlet option.  1D auto:
 *                     the plan's own depth is 8 (lora_plan_stepk, slabs); lora_plan_run uses 16 from 32 sweeps on and
 *                     32 from 64 on
 *   rows_per_thread, panel_width, nt_store, fused_rows, persistent      2D tile shape / block->tile map / stores
 *   lowrank_valu      -1 auto / 0 off / 1 on / 2, 3 (plain / symmetric pyramid form) / 4 (rank-1 + correction instead of the
 *                     nested-profile form) : structured evaluation of the taps inside the fused 2D kernels (summation
 *                     order changes: identical while values are exact integers, ~1 ulp afterwards)
 *   z_chunk, fused_z_chunk             3D output planes per workgroup (single-sweep / fused kernels; 0 = auto)
 *   leap3             0 (default) / 1 : 3D fp64 plans with an even innermost extent and no source get the two-step leapfrog
 *                     launch (kernels_3d_step2.hip; lora_plan_leapfrog_depth reads 2, the lora_plan_step2_leapfrog* entries
 *                     work, leapfrog and Chebyshev runs take pairs of launches).  Any non-zero value reads back as 1; no
 *                     effect on other plans, and none on the kernel name, signature or depth of the plain sweeps.  Same
 *                     bits either way.  Measured: a launch takes 0.72 - 0.89 of the time
 *                     of two single steps, a run of 120 steps 0.79 - 0.95; off until the default is decided on those figures
 *   wave3             0 (default) / 1 : 3D fp64 plans with an even innermost extent and no source get the two-step wave launch
 *                     (kernels_3d_step2.hip; lora_plan_wave_depth reads 2, the lora_plan_step2_wave* entries work, wave runs
 *                     take pairs of launches).  Any non-zero value reads back as 1; independent of "leap3"; no effect on other
 *                     plans, and none on the kernel name, signature, leapfrog depth or depth of the plain sweeps.  Same bits
 *                     either way.  Measured: a launch takes 0.78 - 0.83 of the time of two single steps, a run of 120 steps
 *                     0.76 - 0.86; off until the default is decided on those figures
 *   coarse1           0 (default) / 1 : the multigrid cycles this plan drives (lora_plan_run_mg_until, lora_plan_mg_precondition,
 *                     lora_plan_run_pcg_until, lora_plan_run_theta_mg) run their coarsest level as ONE launch,
 *                     lora_plan_cg_small, when that level's plan reads "cg_small" = 1; otherwise nothing changes.  The level's
 *                     sums fold in another order than the 5 launches per iteration it replaces, so the bits of a cycle
 *                     differ at rounding level (its own bit contract: lora_plan_cg_small).  Any non-zero value reads back as
 *                     1; no effect on a kernel name, signature or sweep.  Measured: DESIGN 3.13
 *   mgfuse            0 (default) / 1 : the multigrid cycles this plan drives (lora_plan_run_mg_until, lora_plan_mg_precondition,
 *                     lora_plan_run_pcg_until, lora_plan_run_theta_mg) compute and restrict the defect of every level below
 *                     the coarsest in ONE launch, lora_plan_mg_defect_restrict, where lora_plan_defect into the level's free
 *                     grid and lora_plan_mg_restrict out of it stood: one launch and two passes over the level's cells fewer
 *                     per level, the free grid not written by that step.  Same bits either way (the entry's bit contract).
 *                     Any non-zero value reads back as 1; no effect on a kernel name, signature or sweep; independent of
 *                     "coarse1".  Measured: DESIGN 3.14
 *   stream3           3D fp64 fused launches: 1 = plane-streaming kernel (kernels_3d_planes.hip: LDS-DMA plane ring, three
 *                     applications per launch for the 7-point star, two for the box), 0 = the two-application tile kernel,
 *                     -1 (default) = by grid size: three applications from ~1.2e8 points (star), the plane-streaming
 *                     kernel with two from ~2.4e7, the tile kernel below;
 *                     stream3_waves (0 automatic; 8 waves per workgroup, one per CU, or 4, two per CU), stream3_pipe (1 = one barrier per plane, two buffers
 *                     per published level; always on for two applications), stream3_async (1 = no workgroup barriers:
 *                     neighbour-wave counters in LDS; bit-identical, measured slower, off)
 *   separable         -1 auto / 0     exactly separable 3D taps as x/y/z passes: bf16 kernels (changes the fp32 summation
 *                     order; the oracle restates both orders, see lora_separable_3x3x3) and the fp64 plane-streaming
 *                     kernel (27 -> 9-10 multiply-adds per point; identical on integer data, ~1e-16 per sweep otherwise)
 *   cols_per_lane, lds_dma, fused_pipeline                              bf16 kernel variants
 *   graph             -1 auto / 0 / 1 : hipGraph replay of lora_plan_run
 *   scratch           -1 auto (= 1) / 0 / 1 : lora_plan_run may allocate one more grid (see there)
 *   mfma_split        bf16 matrix-pipe variant: 1 = hi + lo split of the intermediate (its contract), 0 = one bf16 rounding
 *   stream            2D fused launches: 1 = row-streaming kernel (wave-autonomous column strips, kernels_2d_stream.hip),
 *                     0 = tile kernel; stream_rows (output rows per chunk, 0 = auto), stream_depth (2..6 input rows in
 *                     flight per wave), stream_sync (one barrier per 7 rows keeps a workgroup's strips in step)
 *   wg                2D fused launches through the workgroup-row kernel (kernels_2d_wg.hip: 512-column rows owned by a
 *                     workgroup, the time levels pipelined over two groups of waves): -1 (default) = in plans that fuse six
 *                     applications per launch, where it also runs the four- / two-application tails; 0 never; 1 at every
 *                     depth (6 / 4 / 2).  wg_rows (output rows per chunk; 0 = one round of resident workgroups),
 *                     wg_edge_pct (how much shorter the chunks of the first / last column strip are, per cent; -1 = 12 at six applications, 60 below),
 *                     wg_prio (log2 of the time slice, in 10 ns ticks, of the alternating wave priorities that share a
 *                     CU evenly between its two workgroups; 0 = off)
 *   lanes3            3D fused launches through the register-resident kernels (kernels_3d_lanes.hip, kernels_3d_bf16_lanes.hip:
 *                     four applications per launch with the time levels in registers): -1 (default) by grid size (fp64 from
 *                     ~1e7 points, bf16 separable boxes from 1.2e7), 0 never, 1 always; steps_per_launch = 4 asks for them too
 *   spans3            3D register-resident kernels (fp64 and bf16, four applications per launch): how a launch is cut along
 *                     z.  0 = equal chunks per tile, 1 = spans (the line of all (tile, plane) pairs in equal pieces, one per
 *                     resident workgroup; csrc/spans.h), 2 = team spans (the line over tile rows, a piece per team of a
 *                     row's workgroups), -1 (default) = by measurement: spans on regions that fit the Infinity Cache, team
 *                     spans on bigger bf16 grids where they save steps, chunks otherwise.  Same bits every way
 *   torus             periodic boundary: 1 (default) = lora_plan_run goes through fused launches on a grid extended by a
 *                     ghost zone of periodic images on every side (two more buffers); 0 = single sweeps behind a halo wrap
 *                     each.  Grids smaller than a ghost zone and plans with steps_per_launch = 1 use the latter anyway
 * ("ablate", the load/store-removing timing experiment of round 1, exists only in -DLORA_DIAGNOSTICS builds of the
 * library; the shipped one answers LORA_EINVAL.)
 * lora_plan_get_option reads every key lora_plan_set_option takes -- the value that was set; for "steps_per_launch" and
 * "fused_rows" the resolved value the plan runs with -- and the read-only resolved "tapset", "variant", "fused_eval",
 * "boundary".  ("ablate": only in -DLORA_DIAGNOSTICS builds, like its set.) */
int lora_plan_set_option(lora_plan *plan, const char *key, int value);
int lora_plan_get_option(const lora_plan *plan, const char *key, int *value);
size_t lora_plan_padded_bytes(const lora_plan *plan);
/* Name of the kernel a sweep of this plan launches (for matching rocprof rows). */
const char *lora_plan_kernel_name(const lora_plan *plan);
/* The same plus every resolved option that selects the kernel instantiation or its launch geometry, e.g.
 * "stencil2d_wg_kernel[eval=7,k=6,rows=0,edge=-1,prio=12,bc=0]": the key measured per-launch HBM traffic is filed under
 * (profiles/pmc_traffic.json), so that a changed option can never be paired with a stale measurement. */
const char *lora_plan_kernel_signature(const lora_plan *plan);

/* One kernel application: interior of d_out <- stencil(d_in).  Halo cells of d_out are not
 * touched (2d/gpu.cu:266-271). */
int lora_plan_step(lora_plan *plan, const void *d_in, void *d_out, void *stream);
/* The same restricted to outermost-dimension interior indices [begin, end) (rows in 2D, planes
 * in 3D, points in 1D) -- used to compute slab boundaries first and overlap the halo exchange
 * with the rest.  begin must be a multiple of lora_plan_region_granularity() (2 in 1D, 1 otherwise). */
int lora_plan_step_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream);
int lora_plan_region_granularity(const lora_plan *plan);
/* TWO kernel applications in one launch (temporal fusion; tiled 2D direct-variant and 3D plans): the intermediate time level
 * lives in LDS and its halo cells are taken as 0 -- the state of the reference driver's second buffer --
 * so d_in must be an even time level (halo = the caller's input halo).  Interior of d_out <- stencil(stencil(d_in)).
 * lora_plan_run uses it when the plan's resolved "steps_per_launch" is 2 (3D tile / bf16 kernels, 2D under the Dirichlet
 * option). */
int lora_plan_step2(lora_plan *plan, const void *d_in, void *d_out, void *stream);
int lora_plan_step2_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream);
/* The plan's resolved "steps_per_launch" applications in ONE launch: 1 = lora_plan_step, 2 = lora_plan_step2 (2D / 3D),
 * 4 / 6 in 2D, 3 in 3D fp64, 2 / 4 / 8 in 1D (intermediate levels in LDS; halo cells of odd intermediate levels are 0, of even ones the source
 * buffer's halo -- the state the step-by-step driver would leave).  d_in must be an even time level.
 * lora_plan_run uses an even number of these and finishes with single sweeps; three-application 3D launches have an
 * odd count and run on the reference's alternating buffer state instead (launch k reads buffer k mod 2, whose halo
 * is the caller's for even k and zero for odd k), any number of them. */
int lora_plan_stepk(lora_plan *plan, const void *d_in, void *d_out, void *stream);
int lora_plan_stepk_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream);
/* `napps` applications in one launch: 1, the plan's own depth, or one of the shallower depths its runs use for their tails
 * (2D workgroup-row kernel: 4 and 2 under a six-application plan; 1D: powers of two below the plan's depth; else 2).
 * LORA_EUNSUPPORTED for a depth the plan's kernels do not have. */
int lora_plan_stepn_region(lora_plan *plan, int napps, const void *d_in, void *d_out, int begin, int end, void *stream);
/* The same over TWO disjoint ranges [begin0, end0) and [begin1, end1): what a slab or block driver sweeps behind its
 * deferred wait (the two ends of its share).  One launch where the kernel family takes two ranges (the register-resident 3D
 * kernels), two launches otherwise; an empty range is skipped. */
int lora_plan_stepn_region2(lora_plan *plan, int napps, const void *d_in, void *d_out, int begin0, int end0, int begin1, int end1,
                            void *stream);
/* Test support, no device needed: walks every workgroup of a launch with the decode the register-resident 3D kernels run (the
 * same code, compiled for the host), for a launch cut into
 * spans (team = 0), team spans (team = 1) or team spans with the rim columns cut finer (team = 2; csrc/spans.h) over tiles_x x tiles_y tiles and `depth` planes on `slots`
 * resident workgroups with S steps of start per segment.  cover[(ty * tiles_x + tx) * depth + z] is incremented once per
 * segment that sweeps the pair (the caller zeroes it): every entry must come out 1. */
int lora_debug_span_cover(int tiles_x, int tiles_y, int depth, int S, int slots, int team, int *cover, int *workgroups, int *max_steps);
/* Test support, no device needed: the layout the workgroup-row 2D kernel's launcher chooses for one launch of K = 6, 4 or 2
 * applications over `rows` rows of a 2D plan's grid on cus x per_cu resident workgroups, under the plan's wg_rows and
 * wg_edge_pct options.  out[0..7] = column strips, output columns per strip, rows per chunk and chunks per strip of the
 * strips between the rim strips (chunks 0 where there are none), the same two of the rim strips, workgroups of the launch,
 * rim strips (the first and the last strip; every strip where there are fewer than three). */
int lora_debug_wg_layout(lora_plan *plan, int K, int rows, int cus, int per_cu, int *out);
/* The same for the cut the launcher of the fp64 (kernel = 0) or bf16 (1) register-resident kernel itself chooses for a launch
 * of K = 2 or 4 applications over planes [begin, end) (and [begin2, end2), empty if end2 <= begin2) of h, on tiles_x x tiles_y
 * tiles and `slots` resident workgroups under plan options fused_z_chunk and spans3: cover[(ty * tiles_x + tx) * h + z] counts
 * the segments that sweep plane z of the tile (every entry inside the ranges must come out 1, every other 0), *kind is the
 * layout chosen; where two apply, the later of the list. */
enum lora_cut_kind {
    LORA_CUT_FIXED = 1,    /* chunks of fused_z_chunk planes */
    LORA_CUT_MODEL,        /* equal chunks by the model of rounds of workgroups */
    LORA_CUT_RANGES2,      /* chunks over two ranges of planes */
    LORA_CUT_SLOW,         /* fp64: chunks, one more for the slow rim tiles */
    LORA_CUT_DEALT,        /* fp64: chunks dealt to the resident workgroups */
    LORA_CUT_SPANS,
    LORA_CUT_TEAMS,
    LORA_CUT_TEAMS_FINER   /* bf16: team spans with the rim columns cut finer */
};
int lora_debug_cut_cover(int kernel, int K, int tiles_x, int tiles_y, int h, int begin, int end, int begin2, int end2, int slots,
                         int fused_z_chunk, int spans3, int *cover, int *workgroups, int *max_steps, int *kind);
/* Halo cells of a padded device array (every cell outside the interior, any shape / dtype of the plan): copied from
 * d_src (LORA_HALO_COPY), zeroed (LORA_HALO_ZERO) or wrapped from d_dst's own opposite interior edges
 * (LORA_HALO_WRAP, periodic; LORA_EUNSUPPORTED if an extent is smaller than its halo).  What lora_plan_run uses for
 * the boundary options and the fused launches' halo bookkeeping; exported for drivers that step themselves. */
enum lora_halo_mode { LORA_HALO_COPY = 0, LORA_HALO_ZERO = 1, LORA_HALO_WRAP = 2 };
int lora_plan_halo(lora_plan *plan, void *d_dst, const void *d_src, int mode, void *stream);
/* rows x cols fp64 elements from one strided device array to another (leading dimensions in elements): the pack / unpack
 * kernel of a 2-D block decomposition's COLUMN ghost zones (lorastencil_amd/blocks.py) -- a slab's ghost rows
 * are contiguous and need none.  Asynchronous on `stream`. */
int lora_copy_block_f64(void *d_dst, long dst_ld, const void *d_src, long src_ld, long rows, long cols, void *stream);
/* The time-step driver (2d/gpu.cu:544-546): `times` applications ping-ponging between the two
 * buffers starting from d_buf0; the result is in buffer [times % 2] (the other buffer's interior is
 * unspecified).  The caller must have put the padded input in d_buf0 and zeros in d_buf1 to get the
 * reference semantics.
 * What is read of d_buf1 as the caller left it: under LORA_BC_REFERENCE its HALO cells only (odd sweeps read them: zeros
 * are the reference's), its interior may hold anything -- every interior cell is written before it is read; under
 * LORA_BC_DIRICHLET and LORA_BC_PERIODIC nothing -- the run rewrites the halo before the first read --, so the whole
 * buffer may hold anything.  times == 0 touches neither buffer.
 * Fused launches move K time levels per buffer flip, so an ODD number of them
 * would leave the data in the wrong buffer: the plan then routes the last two through a scratch grid of
 * its own (one more padded array, allocated on first need, freed with the plan; option "scratch" = 0
 * trades it for a shorter launch schedule instead). */
int lora_plan_run(lora_plan *plan, void *d_buf0, void *d_buf1, int times, void *stream);
/* Allocates now what lora_plan_run(plan, ..., times, ...) would allocate on first need (the scratch grid of a schedule with
 * an odd number of fused launches, the extended grid of a periodic run), so that a timed or latency-sensitive first run
 * does not pay for it.  Optional and idempotent. */
int lora_plan_prepare_run(lora_plan *plan, int times);
/* lora_plan_run with HIP events recorded on `stream` around its two kinds of launches -- the fused multi-application
 * launches and the single-sweep tail -- so that a caller can quote the average duration of the dominant kernel over
 * the very region it timed (bench.py's roofline).  Launches directly (no hipGraph) and BLOCKS until the run has
 * finished.  Halo bookkeeping kernels (O(surface)) are inside the fused segment. */
typedef struct lora_run_profile {
    int fused_launches;        /* launches of the K-application kernel                               */
    int apps_per_fused_launch; /* K (1 if the plan does not fuse)                                    */
    int two_launches;          /* shallower fused launches of the tail: 2D: four and / or two applications; 1D: K/2 .. 2 */
    int single_launches;       /* single-sweep launches (the whole run if K = 1)                     */
    float fused_ms;            /* event time of the K-application launches (+ the halo copy)         */
    float two_ms;              /* ... of the shallower fused launches (+ the halo reset)             */
    float single_ms;           /* ... of the single-sweep segment                                    */
} lora_run_profile;
int lora_plan_run_profiled(lora_plan *plan, void *d_buf0, void *d_buf1, int times, void *stream,
                           lora_run_profile *profile);

/* ---- leapfrog stepping (NEW: two time levels, u(t+1) = S(u(t)) + c u(t-1); c = -1 is the wave equation, -1 < c < 0 a damped
 * wave, and second-order Chebyshev / Richardson iterations have the same shape).  S is the plan's raw single sweep, as
 * lora_plan_step applies it.  `c` and the buffers are call arguments, not plan state: no option, kernel name or signature of
 * the plan changes, no cached graph is touched.
 *   Status codes, in this order, before anything is dereferenced or launched: LORA_EINVAL for a null plan or pointer, a
 * non-finite c, a bad range (begin obeys lora_plan_region_granularity), times < 0, and any two of a call's buffers being
 * equal; LORA_EUNSUPPORTED for a buffer that is not 16-byte aligned and for plans without the kernels (below);
 * LORA_ENODEVICE when the launch fails for want of a device.  All entries are asynchronous on `stream`. */
/* 0: the plan has no leapfrog kernel (LORA_BF16 plans, 2D plans of LORA_VARIANT_MFMA, plans that currently carry a source);
 * 1: single steps (every other plan); 2: also the two-step launch (2D plans of the direct variant with an even innermost
 * extent; 3D plans with an even innermost extent on which option "leap3" is 1 -- without the option a 3D plan reads 1).  A
 * function of the plan alone; needs no device. */
int lora_plan_leapfrog_depth(const lora_plan *plan);
/* One step, in place: on every interior cell of the swept range d_prev = fl(acc + fl(c * d_prev)), where acc has exactly the
 * bits the plan's plain single sweep from d_cur stores, c * d_prev is one fp64 multiplication and + one separate fp64
 * addition (two roundings, never a fused multiply-add).  The new level overwrites the oldest one, so leapfrog needs two
 * grids.  Of d_prev only the cells that are stored are read, each by the lane that stores it; its halo cells are never
 * written and never enter a result; d_cur is never written; nothing outside the two padded arrays is touched.  A step equals
 * "lora_plan_step_region into a spare grid, then + c * d_prev on the interior of the region" bit for bit. */
int lora_plan_step_leapfrog(lora_plan *plan, const void *d_cur, void *d_prev, double c, void *stream);
int lora_plan_step_leapfrog_region(lora_plan *plan, const void *d_cur, void *d_prev, double c, int begin, int end, void *stream);
/* Two steps in one launch (plans of leapfrog depth 2; LORA_EUNSUPPORTED otherwise): d_out1 = S(d_cur) + c d_prev and
 * d_out2 = S(d_out1) + c d_cur on the interior cells of rows [begin, end); the four buffers are pairwise distinct.  Level-1
 * cells outside the interior take the value d_prev holds there (the halo of the buffer the level would live in under the
 * in-place entry), so a launch equals two single steps bit for bit on any data; direct taps in row-major order at both levels
 * whatever option "lowrank_valu" says.  Halo cells of d_out1 / d_out2 are never written, d_prev and d_cur never at all.
 *   3D (option "leap3"): the same contract with [begin, end) counting planes.  Level 1 is computed on the interior cells of
 * planes begin - 1 .. end (stored to d_out1 on [begin, end) only); the ring of level-1 cells around the interior, one cell wide,
 * takes d_prev's halo values; the taps are applied in the single step's order (dz, dy, dx ascending).  The chunk length along z
 * is option "fused_z_chunk" (0 = automatic); it moves no bit. */
int lora_plan_step2_leapfrog(lora_plan *plan, const void *d_prev, const void *d_cur, void *d_out1, void *d_out2, double c,
                             void *stream);
int lora_plan_step2_leapfrog_region(lora_plan *plan, const void *d_prev, const void *d_cur, void *d_out1, void *d_out2, double c,
                                    int begin, int end, void *stream);
/* `times` steps from d_prev = level -1 and d_cur = level 0: afterwards level `times` is in d_cur if `times` is even and in
 * d_prev if it is odd, level `times` - 1 in the other buffer; times == 0 touches nothing.  Under LORA_BC_REFERENCE and
 * LORA_BC_DIRICHLET no halo cell is ever written: each buffer keeps the halo the caller gave it (the same halo in both is a
 * fixed boundary).  Under LORA_BC_PERIODIC d_cur's halo is wrapped before the first step and every new level after its step
 * (lora_plan_halo with LORA_HALO_WRAP, with its LORA_EUNSUPPORTED for extents below the halo width); single steps only.
 *   Plans of depth 2 under the other two boundaries run times / 4 pairs of two-step launches through two scratch grids owned
 * by the plan -- (prev, cur) -> (s0, s1) -> (prev, cur); their halos are copied from d_prev and d_cur once per run; they are
 * allocated on first need or by lora_plan_prepare_leapfrog and freed with the plan -- and times % 4 single steps after them;
 * option "scratch" = 0 means single steps only.  Launches directly (no hipGraph).  Whatever the schedule, the result is bit
 * for bit that of `times` single steps. */
int lora_plan_run_leapfrog(lora_plan *plan, void *d_prev, void *d_cur, double c, int times, void *stream);
/* Allocates now what lora_plan_run_leapfrog(plan, ..., times, ...) would allocate on first need.  Optional and idempotent. */
int lora_plan_prepare_leapfrog(lora_plan *plan, int times);
/* The group-A form is lora_run_host_leapfrog (section A). */

/* ---- leapfrog steps with a source and a scale (NEW): u+ = a (S(u) + f) + c u-.  a = 1, c = -1 is a forced wave equation; per-step
 * a = w(k), c = 1 - w(k) is the Chebyshev semi-iteration below.  `f` (d_f: a padded device grid of the plan, or NULL for none),
 * `a`, `c` and the buffers are call arguments, not plan state: no option, kernel name, signature or leapfrog depth of the plan
 * changes.  The plans are exactly those of lora_plan_leapfrog_depth; in particular a plan on which lora_plan_set_source was
 * called is refused with LORA_EUNSUPPORTED, as the leapfrog entries refuse it.
 *   Status codes, in this order, before anything is dereferenced or launched: LORA_EINVAL for a null plan or pointer (d_f may
 * be null), a non-finite a or c, a bad range, times < 0, ncoef < 1, and any two of a call's buffers being equal (d_f included);
 * LORA_EUNSUPPORTED for a buffer that is not 16-byte aligned and for a refused plan; LORA_ENODEVICE when the launch fails for
 * want of a device.  Asynchronous on `stream` unless stated. */
/* One step, in place: on every interior cell of the swept range
 *     t = fl(acc + f)   (d_f == NULL: t = acc, no addition at all)      d_prev = fl( fl(a * t) + fl(c * d_prev) )
 * where acc has exactly the bits the plan's plain single sweep of d_cur stores and every other operation is a separate fp64
 * rounding, never a fused multiply-add.  With d_f == NULL and a == 1 a step equals lora_plan_step_leapfrog bit for bit on
 * non-NaN data; with d_f it equals "source sweep into a spare grid, then a * spare + c * d_prev as two multiplications and one
 * addition" bit for bit.  f is read with the store's own addressing and predicate: its halo cells are never used, it is never
 * written; d_cur is never written; of d_prev only the cells stored are read, each by the lane that stores it; nothing outside
 * the padded arrays is touched. */
int lora_plan_step_leapfrog_src(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_f, double a, double c, void *stream);
int lora_plan_step_leapfrog_src_region(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_f, double a, double c, int begin,
                                       int end, void *stream);
/* Two steps in one launch (plans of leapfrog depth 2; LORA_EUNSUPPORTED otherwise): d_out1 = a1 (S(d_cur) + f) + c1 d_prev and
 * d_out2 = a2 (S(d_out1) + f) + c2 d_cur on the interior cells of rows [begin, end), with the rounding rule above at both
 * levels; the buffers are pairwise distinct.  Level-1 cells outside the interior take the value d_prev holds there; direct taps
 * in row-major order at both levels whatever option "lowrank_valu" says: a launch equals two single steps bit for bit on any
 * data.  Halo cells of d_out1 / d_out2 are never written, d_prev, d_cur and d_f never at all.  3D plans with option "leap3":
 * as lora_plan_step2_leapfrog states it, in planes; d_f is read on interior cells alone, at both levels. */
int lora_plan_step2_leapfrog_src(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_f, void *d_out1, void *d_out2,
                                 double a1, double c1, double a2, double c2, void *stream);
int lora_plan_step2_leapfrog_src_region(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_f, void *d_out1,
                                        void *d_out2, double a1, double c1, double a2, double c2, int begin, int end, void *stream);
/* `times` steps from d_prev = level -1 and d_cur = level 0; step i (0-based) uses a[min(i, ncoef - 1)] and c[min(i, ncoef - 1)]
 * (ncoef == 1: constant coefficients, the forced wave).  The host arrays are read during the call only; LORA_EINVAL for a
 * non-finite entry among those that will be used.  Buffer placement, the three boundary modes and the schedule are
 * lora_plan_run_leapfrog's: times / 4 pairs of two-step launches through the plan's two scratch grids (the same two;
 * lora_plan_prepare_leapfrog allocates them), times % 4 single steps at the end, single steps only under LORA_BC_PERIODIC and
 * with option "scratch" = 0, direct launches.  Whatever the schedule, the result is bit for bit that of `times` single steps. */
int lora_plan_run_leapfrog_src(lora_plan *plan, void *d_prev, void *d_cur, const void *d_f, const double *a, const double *c, int ncoef,
                               int times, void *stream);
/* Host only: the Chebyshev schedule for an iteration matrix S whose spectrum lies in [-rho, rho]:  w(1) = 1,
 * w(2) = 1 / (1 - rho^2 / 2),  w(k+1) = 1 / (1 - rho^2 w(k) / 4).  For step k = first_step + i (steps count from 1) a[i] = w(k)
 * and c[i] = 1 - w(k); a[0] == 1 and c[0] == 0 exactly for first_step == 1.  The caller supplies rho; for the 5-point Jacobi taps
 * (1/4 on the four neighbours) on an m x n interior with zero (Dirichlet) halos it is (cos(pi / (m+1)) + cos(pi / (n+1))) / 2.
 * With it the residual after k steps is at most 2 s^k / (1 + s^2k) of the first, s = rho / (1 + sqrt(1 - rho^2)), for a
 * symmetric S; rho = 0 gives w = 1 throughout (plain sweeps).  An underestimated rho slows convergence, it does not break it
 * while rho < 1.  LORA_EINVAL unless 0 <= rho < 1 (NaN included), first_step >= 1, count >= 0. */
int lora_chebyshev_coeffs(double rho, int first_step, int count, double *a, double *c);
/* The group-A form is lora_run_host_chebyshev (section A); lora_plan_run_chebyshev_until follows lora_plan_run_until below. */

/* ---- variable-coefficient wave steps (NEW): u+ = k(x) S(u) + b u + c u-.  k (d_k: a padded device grid of the
 * plan, laid out like d_cur) is a per-cell coefficient, b and c are scalars.  With S the zero-sum form L of the taps, b = 2,
 * c = -1 is the wave equation in a heterogeneous medium, u(t+1) = 2 u(t) - u(t-1) + kappa(x) L u(t); b = 1, c = 0 is the explicit
 * heterogeneous diffusion step u + kappa(x) L u.  d_k, b, c and the buffers are call arguments, not plan state: no option,
 * kernel name, signature or leapfrog depth of the plan changes, no cached graph is touched.  The plans are those of
 * lora_plan_wave_depth; a plan on which lora_plan_set_source was called is refused, as the leapfrog entries refuse it.
 *   Status codes, in this order, before anything is dereferenced or launched: LORA_EINVAL for a null plan or pointer (d_k is
 * mandatory), a non-finite b or c, a bad range (begin obeys lora_plan_region_granularity), times < 0, and any two of a call's
 * buffers being equal (d_k included); LORA_EUNSUPPORTED for a buffer that is not 16-byte aligned, for a refused plan and for a
 * two-step entry on a plan of wave depth below 2; LORA_ENODEVICE when the launch fails for want of a device.  All entries are
 * asynchronous on `stream`. */
/* 0: the plan has no wave kernel (LORA_BF16 plans, 2D plans of LORA_VARIANT_MFMA, plans that currently carry a source);
 * 2: also the two-step launch (2D plans of the direct variant with an even innermost extent; 3D plans with an even innermost
 * extent on which option "wave3" is 1); 1: single steps (every other plan; without "wave3" a 3D plan reads 1 with or without
 * option "leap3", which moves the leapfrog depth alone).  A function of the plan alone; needs no device. */
int lora_plan_wave_depth(const lora_plan *plan);
/* One step, in place: on every interior cell of the swept range
 *     d_prev = fl( fl( fl(k * acc) + fl(b * u) ) + fl(c * d_prev) )
 * where acc has exactly the bits the plan's plain single sweep of d_cur stores, u is the cell of d_cur and k the cell of d_k at
 * the store's address, and the five operations are separate fp64 roundings, never a fused multiply-add.  A step equals
 * "lora_plan_step_region into a spare grid, then the five operations one at a time on the interior of the region" bit for bit,
 * non-finite values included.  k is read with the store's own addressing and predicate: its halo cells are never used, it is
 * never written; d_cur is never written; of d_prev only the cells stored are read, each by the lane that stores it; nothing
 * outside the padded arrays is touched. */
int lora_plan_step_wave(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_k, double b, double c, void *stream);
int lora_plan_step_wave_region(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_k, double b, double c, int begin, int end,
                               void *stream);
/* Two steps in one launch (plans of wave depth 2; LORA_EUNSUPPORTED otherwise): d_out1 = k S(d_cur) + b d_cur + c d_prev and
 * d_out2 = k S(d_out1) + b d_out1 + c d_cur on the interior cells of rows [begin, end), with the rounding rule above at both
 * levels; the five buffers are pairwise distinct.  Level-1 cells outside the interior take the value d_prev holds there; direct
 * taps in row-major order at both levels whatever option "lowrank_valu" says: a launch equals two single steps bit for bit on
 * any data.  Halo cells of d_out1 / d_out2 are never written, d_prev, d_cur and d_k never at all; d_k is read on interior
 * cells alone, at both levels.
 *   3D (option "wave3"): the same contract with [begin, end) counting planes, the geometry and the boundary rule of the 3D
 * lora_plan_step2_leapfrog (level 1 is computed, not stored, on planes begin - 1 and end), the tap chain of the plan's single
 * step.  A padded plane of 2^28 cells or more is refused by the launch (LORA_EHIP), as there. */
int lora_plan_step2_wave(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_k, void *d_out1, void *d_out2, double b,
                         double c, void *stream);
int lora_plan_step2_wave_region(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_k, void *d_out1, void *d_out2,
                                double b, double c, int begin, int end, void *stream);
/* `times` steps from d_prev = level -1 and d_cur = level 0.  Buffer placement, the three boundary modes and the schedule are
 * lora_plan_run_leapfrog's with the wave depth in place of the leapfrog depth: on plans of wave depth 2, times / 4 pairs of
 * two-step launches through the plan's two scratch grids (the same two; lora_plan_prepare_wave allocates them; d_k must differ
 * from them as from d_prev and d_cur, else the run takes single steps), times % 4 single steps at the end; single steps only
 * under LORA_BC_PERIODIC (d_k is never wrapped: its halo is never read), with option "scratch" = 0, and on every plan of wave
 * depth 1: a 3D plan without option "wave3", whatever option "leap3" says.  Direct launches.  Whatever the schedule, the result is bit for bit that of `times` single
 * steps. */
int lora_plan_run_wave(lora_plan *plan, void *d_prev, void *d_cur, const void *d_k, double b, double c, int times, void *stream);
/* Allocates now what lora_plan_run_wave(plan, ..., times, ...) would allocate on first need.  Optional and idempotent. */
int lora_plan_prepare_wave(lora_plan *plan, int times);
/* The group-A form is lora_run_host_wave (section A). */

/* ---- reductions over grids on the device (NEW: the reference prints its "Result range" from a host loop over the copied-back
 * array).  Both read the interior cells of the outermost range [begin, end) as lora_plan_step_region counts it (begin == end
 * == 0: the whole interior; begin == end otherwise: no cell, the empty record), accumulate in fp64, and return the same bits
 * for the same call every time (the work is cut by dtype and region shape alone; no atomics).  They keep the buffer
 * contract above: pieces of at most 16 bytes, nothing read outside [base, base + lora_plan_padded_bytes), and no halo value
 * reaches a result.  UNLIKE the launches above both BLOCK: they enqueue on `stream` (two small launches and a copy of the
 * record), then wait until the result is in *out.  LORA_EINVAL for a null pointer or a bad range, LORA_EUNSUPPORTED for a
 * misaligned buffer or a stream that is capturing, LORA_ENODEVICE without a device. */
typedef struct lora_grid_stats {
    double min, max, abs_max, sum, sum_sq; /* over the FINITE cells; none: min = +inf, max = -inf, the rest 0 */
    long long count, nonfinite;            /* cells of the region; NaN or +-inf cells among them               */
} lora_grid_stats;
typedef struct lora_grid_diff {
    double max_abs, sum_sq, a_abs_max; /* of d = (double) a - (double) b, one rounding, over the cells with finite d;
                                          a_abs_max = max |a| over the same cells                                    */
    long long argmax;                  /* LOWEST linear index in the PADDED array of a cell with |d| == max_abs; -1 if none */
    long long count, nonfinite;        /* cells of the region; cells whose d is not finite                            */
} lora_grid_diff;
int lora_plan_stats(lora_plan *plan, const void *d_buf, int begin, int end, lora_grid_stats *out, void *stream);
int lora_plan_diff(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_diff *out, void *stream);
/* One sweep's change in a single pass: *out = the lora_grid_diff of a = ONE raw sweep of d_in and b = d_in, over the outermost
 * interior range [begin, end) -- "how far is this level from a fixed point?", asked of one buffer.  The sweep is exactly what
 * lora_plan_step_region(plan, d_in, scratch, begin, end) would store (same taps, same order, bf16: the single rounding
 * included), but the swept level is never written anywhere: the call reads d_in once and writes no grid memory at all.
 * Ranges as for the reductions (0, 0: the whole interior; begin == end otherwise: the empty record), and begin obeys
 * lora_plan_region_granularity like lora_plan_step_region.  BLOCKS, like the reductions, and answers their status codes in
 * their order: LORA_EINVAL for a null pointer or a bad range; LORA_EUNSUPPORTED for a misaligned buffer, a plan without the
 * kernel, or a stream that is capturing; LORA_ENODEVICE without a device.
 *   Contract.  max_abs, a_abs_max, argmax, count and nonfinite are BIT FOR BIT what the two calls lora_plan_step_region(plan,
 *   d_in, scratch, begin, end) and lora_plan_diff(plan, scratch, d_in, begin, end) give, non-finite data included; argmax is
 *   the lowest padded linear index among equal maxima.  sum_sq sums the same finite d in this kernel's own fixed order: the
 *   same call gives the same bits every time, whatever the plan's tuning options ("rows_per_thread", "panel_width",
 *   "nt_store", "z_chunk", "cols_per_lane", ...) -- the launch geometry follows from dtype, extents, tap set and region
 *   alone, and there are no atomics.  The buffer contract above holds: pieces of at most 16 bytes, nothing outside [base,
 *   base + lora_plan_padded_bytes) is read, and halo values are read because the stencil needs them but never enter the
 *   reduction as cells.
 *   Which plans have the kernel (read-only option "fused_residual": 1 or 0): every 1D plan; 2D plans of the direct variant
 *   and 3D fp64 plans with an even innermost extent; 3D bf16 plans.  Plans on the one-thread-per-point kernels (odd innermost
 *   extent) and 2D plans of LORA_VARIANT_MFMA (whose sums run in another order than the direct taps) answer
 *   LORA_EUNSUPPORTED. */
int lora_plan_residual(lora_plan *plan, const void *d_in, int begin, int end, lora_grid_diff *out, void *stream);
/* The TRUE residual of u = S(u) + f in one pass: *out = the lora_grid_diff of a = S(d_in) + f against b = d_in over the
 * outermost interior range [begin, end), ranges and granularity as lora_plan_residual.  d_f is a padded fp64 grid of the plan's
 * layout and a CALL ARGUMENT like the f of the *_leapfrog_src entries, never plan state: no option, kernel name, signature or
 * depth of the plan changes.  The launch reads d_in once and the interior cells of d_f once (16-byte pieces at the reduced
 * cells' own padded indices, 8 bytes for the odd tail point in 1D: no halo cell of d_f is ever loaded, nothing outside [d_f,
 * d_f + lora_plan_padded_bytes) is read) and writes no grid memory at all.  BLOCKS like the reductions.
 *   Contract.  max_abs, a_abs_max, argmax, count and nonfinite are BIT FOR BIT what a single sweep over [begin, end) of a plan
 *   that carries f as its source (lora_plan_set_source + lora_plan_step_region) into a spare grid, then lora_plan_diff(spare,
 *   d_in, begin, end) give -- a = fl(acc + f), one rounding on top of the sweep's bits -- non-finite data in d_in or in interior
 *   cells of f included; argmax is the lowest padded index among equal maxima; sum_sq sums the same finite d in the kernel's own
 *   fixed order, the same bits every time whatever the plan's tuning options.  d_f == NULL is exactly lora_plan_residual, on
 *   the same plans (bf16 included), in all six fields.
 *   Status, in this order, before anything is dereferenced or launched: LORA_EINVAL for a null plan, d_in or out, a bad range
 *   or begin, or d_f == d_in; LORA_EUNSUPPORTED for a misaligned d_in or d_f; LORA_EUNSUPPORTED, with d_f != NULL, for a plan
 *   whose option "fused_residual" reads 0, a LORA_BF16 plan (a source is fp64) and a plan on which lora_plan_set_source was
 *   called; then the reductions' codes (a capturing stream, LORA_ENODEVICE). */
int lora_plan_residual_src(lora_plan *plan, const void *d_in, const void *d_f, int begin, int end, lora_grid_diff *out, void *stream);
/* Test support, no device needed: replays on the host the tile -> workgroup -> cells map of lora_plan_residual's launch over
 * [begin, end) (csrc/residual_tiles.h).  cover[padded linear index] is incremented once per cell a workgroup would reduce (the
 * caller zeroes it: lora_padded_count ints): every interior cell of the range must come out 1, every other cell 0.
 * *workgroups = the launch's size.  LORA_EUNSUPPORTED for a plan without the kernel. */
int lora_debug_residual_cover(const lora_plan *plan, int begin, int end, int *cover, int *workgroups);
/* Host only: *into becomes the record of the union of two DISJOINT regions (the own rows of N slabs: lora_plan_stats takes
 * lora_slab_plan, lora_slab_buffer(s, 2) and the own-row range of lora_slab_info as they are).  Start from a record of a
 * region, or from the empty one {+inf, -inf, 0, 0, 0, 0, 0}. */
void lora_grid_stats_merge(lora_grid_stats *into, const lora_grid_stats *part);

/* Sweep until nothing changes.
 *   check_every must be even and >= 2, otherwise LORA_EINVAL (also: a negative or NaN tol / rtol, an unknown norm, max_times < 0).
 *   The loop runs while times_done + check_every <= max_times.  Each round:
 *     lora_plan_run(plan, d_buf0, d_buf1, check_every, stream) -- an even run leaves the level in d_buf0 and both halos as a
 *     fresh run expects them;
 *     a PROBE of one raw sweep's change (under LORA_BC_PERIODIC after lora_plan_halo(..., LORA_HALO_WRAP) on d_buf0) -> `last`:
 *       under LORA_NORM_MAX on a plan whose option "fused_residual" reads 1: ONE lora_plan_residual on d_buf0 (d_buf1 is not
 *       touched by the probe);
 *       otherwise (LORA_NORM_RMS, where sum_sq decides the stop; plans without that kernel): one raw lora_plan_step from
 *       d_buf0 into d_buf1, then diff(a = d_buf1, b = d_buf0) over the whole interior.
 *     The two forms agree bit for bit in last.{max_abs, a_abs_max, argmax, count, nonfinite} and so in everything they decide;
 *     last.sum_sq carries the summation order of the form that ran.  The code picks the form from the plan and the norm.
 *     residual = last.max_abs (LORA_NORM_MAX) or sqrt(last.sum_sq / last.count) (LORA_NORM_RMS).
 *   Stop with diverged = 1 when last.nonfinite > 0; else with converged = 1 when residual <= tol + rtol * last.a_abs_max;
 *   otherwise continue.
 *   On return d_buf0 holds level times_done, BIT FOR BIT what lora_plan_run(times_done) gives from the same input; d_buf1's
 *   interior is unspecified, as after any run, and its halo is as a run leaves it.  Not converging is not an error: LORA_OK
 *   with converged = 0.  `residual` is for level times_done -> times_done + 1 (+inf if no round ran); checks = rounds done.
 *   Cost per check, fused probe: ONE read of the grid (no more than a single sweep's time; DESIGN.md 3.5 has the figures)
 *   plus ONE synchronise of the host with the stream.  Two-pass probe: ONE single sweep plus ONE diff (about a sweep's
 *   bytes, read only) plus the synchronise -- about eight sweeps of a six-sweep launch: check_every = 60 adds 12 % to a
 *   star2d1r run at 16384^2, 300 under 3 %.  Choose check_every accordingly.  Blocks like the reductions, and answers their
 *   status codes. */
enum lora_norm { LORA_NORM_MAX = 0, LORA_NORM_RMS = 1 }; /* max |d|, sqrt(sum_sq / count) */
typedef struct lora_until {
    double tol, rtol;
    int norm, check_every, max_times;
} lora_until;
typedef struct lora_until_result {
    int times_done, checks, converged, diverged;
    double residual;
    lora_grid_diff last;
} lora_until_result;
int lora_plan_run_until(lora_plan *plan, void *d_buf0, void *d_buf1, const lora_until *u, lora_until_result *r, void *stream);
/* Solve u = S(u) + f by the Chebyshev semi-iteration until the TRUE residual is small.  d_cur is level 0; d_prev may hold any
 * FINITE values (step 1 has c = 0, and 0 x NaN is NaN); d_f may be NULL.  `u` obeys lora_plan_run_until's rules (even
 * check_every >= 2, ...); LORA_EINVAL also unless 0 <= rho < 1; the plans and the other status codes are those of
 * lora_plan_run_leapfrog_src, then the reductions'.  Each round runs check_every steps of lora_plan_run_leapfrog_src with the
 * schedule's next coefficients (lora_chebyshev_coeffs(rho, times_done + 1, check_every)) and then probes the newest level:
 * `last` = the lora_grid_diff of a = S(d_cur) + f against b = d_cur over the whole interior, bit for bit in max_abs, a_abs_max,
 * argmax, count and nonfinite what a source sweep into a spare grid plus lora_plan_diff give.  Under LORA_NORM_MAX on a plan
 * whose option "fused_residual" reads 1 the probe is ONE lora_plan_residual_src(d_cur, d_f): no third grid is allocated or
 * touched, and last.sum_sq carries that kernel's order.  Otherwise (LORA_NORM_RMS, where sum_sq decides the stop; plans
 * without that kernel) the probe sweeps into a third grid owned by the plan (allocated on first need of this form, freed with
 * the plan) and takes the difference.  Neither form changes d_prev or d_cur.  Stop rule and
 * result fields are lora_plan_run_until's.  On return d_cur holds level times_done, bit for bit what
 * lora_plan_run_leapfrog_src(times_done) with the same coefficients gives, and d_prev the level before it.  BLOCKS, and answers
 * the reductions' status codes.  Cost of a probe: fused, one read of d_cur and of d_f; two-pass, one single sweep
 * with a source plus one difference. */
int lora_plan_run_chebyshev_until(lora_plan *plan, void *d_prev, void *d_cur, const void *d_f, double rho, const lora_until *u,
                                  lora_until_result *r, void *stream);

/* ---- conjugate gradients for u = S(u) + f (NEW).  The operator is A = I - S, S the plan's raw single sweep; a
 * grid the operator is applied to carries a ZERO halo, so the boundary is homogeneous on the correction and the caller's
 * boundary values enter the first residual only.  Needs no spectral estimate, and its coefficients give the extreme eigenvalues
 * of A -- a rho for lora_plan_run_chebyshev_until.  fp64.
 *   Which plans (read-only option "cg": 1 or 0): fp64 plans whose option "fused_residual" reads 1 and that carry no source.
 *   Every other plan -- bf16, the 2D matrix-pipe variant, an odd innermost extent in 2D / 3D, a plan on which
 *   lora_plan_set_source was called -- answers LORA_EUNSUPPORTED; lora_plan_dot alone takes every plan, as lora_plan_diff does.
 *   The three entries with a record BLOCK like the reductions and use their range rules (0, 0: the whole interior; begin == end
 *   otherwise: the empty record {0, 0, 0, 0}; begin obeys lora_plan_region_granularity).  Status, in this order: LORA_EINVAL for
 *   a null pointer, a bad range or begin, or two buffers of different roles that are equal (d_a == d_b of lora_plan_dot is
 *   allowed); LORA_EUNSUPPORTED for a misaligned buffer, then for a plan without the kernels; then the reductions' codes (a
 *   capturing stream, LORA_ENODEVICE).  The same call returns the same bits every time, whatever the plan's tuning options:
 *   the launch geometry follows from extents, tap set and region alone, lanes, waves and workgroups fold in fixed orders, and
 *   there are no atomics.  Every arithmetic operation named below is its own fp64 rounding, fl(); nothing is contracted.  The
 *   buffer contract above holds: pieces of at most 16 bytes, nothing outside [base, base + lora_plan_padded_bytes). */
typedef struct lora_grid_dot {
    double dot, sum_abs;        /* sum of a b and of |a b| over the cells whose product is finite */
    long long count, nonfinite; /* cells of the region; cells whose product is not finite        */
} lora_grid_dot;
/* *out = the lora_grid_dot of two grids over the interior cells of [begin, end), cut like lora_plan_diff; halo cells of a
 * 16-byte piece are selected away before any arithmetic, so no halo value -- a NaN included -- reaches a result. */
int lora_plan_dot(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_dot *out, void *stream);
/* q = A p in one pass: on every interior cell of [begin, end) d_q = fl(d_p - acc), where acc has the bits
 * lora_plan_step_region(plan, d_p, spare, begin, end) stores, and *out = the lora_grid_dot of a = d_p, b = d_q over those
 * cells.  d_p is read once (halo included: the stencil needs it), d_q is written once on interior cells only -- its halo is
 * neither read nor written.  Tiled like lora_plan_residual (csrc/residual_tiles.h). */
int lora_plan_apply_dot(lora_plan *plan, const void *d_p, void *d_q, int begin, int end, lora_grid_dot *out, void *stream);
/* On every interior cell of [begin, end): d_x = fl(d_x + fl(alpha d_p)), d_r = fl(d_r - fl(alpha d_q)); *out_rr = the
 * lora_grid_dot of a = b = the new d_r.  Four reads, two writes, interior cells only (16-byte pieces; 8 bytes for the odd tail
 * point in 1D): no halo cell of any of the four grids is loaded or stored. */
int lora_plan_cg_update(lora_plan *plan, void *d_x, void *d_r, const void *d_p, const void *d_q, double alpha, int begin, int end,
                        lora_grid_dot *out_rr, void *stream);
/* On every interior cell of [begin, end): d_p = fl(d_r + fl(beta d_p)); the halo of d_p is not touched.  ASYNCHRONOUS: enqueues
 * one launch on `stream` like lora_plan_step_region and takes a capturing stream; status codes otherwise as above. */
int lora_plan_cg_direction(lora_plan *plan, void *d_p, const void *d_r, double beta, int begin, int end, void *stream);
/* Solve u = S(u) + f by conjugate gradients until the TRUE residual is small.  d_x holds the start iterate, the caller's
 * boundary values in its halo; d_f may be NULL.  `u` obeys lora_plan_run_until's rules unchanged.  Three grids r, p, q the plan
 * owns (allocated on first need or by lora_plan_prepare_cg, never memset, freed with the plan) and a device-resident scalar
 * state {rr, pq, alpha, beta, iteration, breakdown} with a history of max_times alphas and betas carry the run.
 *   Start-up:  r = fl(fl(S(x) + f) - x) on the interior -- the plan's single sweep with f as its source (without f: r =
 *   fl(S(x) - x), no zero is added), then one subtraction -- p = r with a zeroed halo (once per run, on `stream`), rr = the dot
 *   of lora_plan_dot(r, r).
 *   Each round enqueues check_every iterations with NO host wait between them; iteration k is
 *     pq = lora_plan_apply_dot(p, q).dot;  alpha = rr / pq;  rr' = lora_plan_cg_update(x, r, p, q, alpha).dot;
 *     beta = rr' / rr;  lora_plan_cg_direction(p, r, beta);  rr = rr'
 *   over the whole interior, alpha and beta divided in IEEE fp64 on the device by one lane behind each fold and read from the
 *   state by the next launch.  Then the round probes the true residual exactly as lora_plan_run_chebyshev_until does -- `last`
 *   = the lora_grid_diff of a = S(d_x) + f against b = d_x: ONE lora_plan_residual_src(d_x, d_f) under LORA_NORM_MAX, else the
 *   source sweep into q and lora_plan_diff -- and reads the state back in the same wait.  Stop rule and fields of `until` are
 *   lora_plan_run_until's, times_done = the device's iteration count.
 *   Breakdown: if pq is not finite or pq <= 0 (A is not positive definite on p), or rr or any product is not finite, the
 *   one-lane update sets a sticky flag; every later launch of the run that finds it set returns before it loads or stores
 *   anything, so d_x stays the last good iterate.  The run stops at its next probe with breakdown = 1 and diverged = 1 --
 *   unless that probe meets the stop rule: a residual that vanished exactly (p = 0, pq = 0) is convergence, converged = 1
 *   with breakdown = 1.  A non-finite probe gives diverged = 1.
 *   BIT CONTRACT: d_x after k iterations is bit for bit what the caller gets by looping the four public entries above as
 *   written, alpha and beta divided in host fp64 -- the driver launches the same kernels at the same geometry.
 *   No halo cell of d_x is ever written, d_f is never written, everything is ordered on `stream` alone.
 *   On return lambda_min / lambda_max are the extreme eigenvalues of the run's Lanczos tridiagonal (lora_cg_spectrum over the
 *   times_done coefficients) -- Ritz values, inside the spectrum of A and closing in on its ends -- and rho_estimate =
 *   max(|1 - lambda_min|, |1 - lambda_max|), the spectral radius of S to hand to lora_plan_run_chebyshev_until; all three NaN
 *   when times_done == 0.
 *   LORA_EINVAL for a null plan, d_x, u or r, a bad `u`, d_f == d_x, or a caller's buffer that is one of the plan's grids;
 *   LORA_EUNSUPPORTED for a misaligned buffer, a plan whose option "cg" reads 0, and taps that are not point-symmetric (w[t] ==
 *   w[ntaps - 1 - t] exactly, decided on the host: without it A is not symmetric); then the reductions' codes.  BLOCKS. */
typedef struct lora_cg_result {
    lora_until_result until;
    double lambda_min, lambda_max, rho_estimate;
    int breakdown;
} lora_cg_result;
int lora_plan_run_cg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_until *u, lora_cg_result *r, void *stream);
/* Allocate now what lora_plan_run_cg_until(..., u->max_times = max_times) would allocate on first need: the three grids and
 * the scalar state with its history.  LORA_EINVAL for max_times < 0, LORA_EUNSUPPORTED for a plan whose option "cg" reads 0. */
int lora_plan_prepare_cg(lora_plan *plan, int max_times);
/* Host only: the extreme eigenvalues of the n x n Lanczos tridiagonal of a CG run's coefficients,
 *   T[k][k] = 1 / alpha[k] + beta[k-1] / alpha[k-1] (the second term absent for k = 0),  T[k][k+1] = sqrt(beta[k]) / alpha[k],
 * by bisection on the Sturm count, to a few ulps of the largest.  beta[n-1] is not read (beta may be NULL for n == 1).
 * LORA_EINVAL for n < 1, a null pointer, an alpha that is not positive and finite, a beta that is negative or not finite. */
int lora_cg_spectrum(const double *alpha, const double *beta, int n, double *lambda_min, double *lambda_max);

/* ---- implicit time stepping (NEW).  One sweep is one forward-Euler step of du/dt = S(u) + f - u with step 1.
 * The theta scheme with step tau > 0 and 0 <= theta <= 1 (1: backward Euler, 1/2: Crank-Nicolson, 0: the explicit step) is
 *     (1 + theta tau) u+ - theta tau S(u+) = u + (1 - theta) tau (S(u) - u) + tau f,
 * one solve per step with A = sigma I - tau' S, sigma = fl(1 + tau'), tau' = fl(theta tau).  Started from x0 = u the first
 * residual of that system is exactly r0 = tau (S(u) + f - u) -- the right-hand side cancels -- so no right-hand-side grid
 * exists: conjugate gradients accumulate the increment straight into d_u.  A is symmetric for point-symmetric taps and positive
 * definite whenever rho(S) <= 1.  Plans, range rules, status codes and their order, the bit-for-bit repeatability and the
 * buffer contract are those of lora_plan_apply_dot above (option "cg" = 1, no source on the plan); every operation named
 * below is its own fp64 rounding. */
/* q = (sigma I - tau S) p in one pass: on every interior cell of [begin, end) d_q = fl(fl(sigma d_p) - fl(tau acc)), acc as in
 * lora_plan_apply_dot, and *out = the lora_grid_dot of a = d_p, b = d_q.  Also LORA_EINVAL for a sigma or tau that is not
 * finite.  With sigma == tau == 1 it equals lora_plan_apply_dot bit for bit in d_q and in the record on data without NaNs
 * (1 x is exact).  The general shifted operator: screened Poisson / Helmholtz-type solves through the public CG entries. */
int lora_plan_apply_dot_shift(lora_plan *plan, const void *d_p, void *d_q, double sigma, double tau, int begin, int end,
                              lora_grid_dot *out, void *stream);
/* The start of a step in one launch: on every interior cell of [begin, end) t = fl(acc + d_f) (d_f == NULL: t = acc, no zero is
 * added), d = fl(t - d_u), r = fl(tau d), stored to BOTH d_r and d_p; *out_rr = the lora_grid_dot of a = b = r.  acc has the
 * bits lora_plan_step_region(plan, d_u, spare, begin, end) stores.  d_u is read once, halo included; d_f at the stored cells
 * alone, so its halo is never loaded; the halos of d_r and d_p are neither read nor written (16-byte stores, 8 bytes for the
 * odd tail point in 1D).  d_f may be NULL, the other buffers must be pairwise distinct; LORA_EINVAL also for a tau that is not
 * finite.  It stands for a source sweep, a subtraction, a scale, a copy and a dot. */
int lora_plan_theta_start(lora_plan *plan, const void *d_u, const void *d_f, double tau, void *d_r, void *d_p, int begin, int end,
                          lora_grid_dot *out_rr, void *stream);
/* `steps` theta steps of d_u in place, the whole run enqueued on `stream` with NO host wait inside it.  The plan's three CG
 * grids r, p, q and two device-resident states carry the run (lora_plan_prepare_theta allocates them ahead of time).
 *   The run zeroes the halo of p once.  Each step enqueues lora_plan_theta_start(d_u, d_f, tau) -> r, p and then max_iters
 *   iterations of
 *     pq = lora_plan_apply_dot_shift(p, q, sigma, tau').dot;  alpha = rr / pq;  rr' = lora_plan_cg_update(d_u, r, p, q, alpha).dot;
 *     beta = rr' / rr;  lora_plan_cg_direction(p, r, beta);  rr = rr'
 *   over the whole interior.  One lane behind each fold keeps the scalars: behind the start's, rr = rr0 = the start's dot, the
 *   step's iteration count 0, thresh = fl(rtol2 rr0) with rtol2 = fl(rtol rtol) from the host, and `done` cleared -- or set at
 *   once when rr0 == 0 (the level is steady; the step counts with 0 iterations); behind the update's, alpha / beta / rr as in
 *   lora_plan_run_cg_until and then the STOP RULE: if rr' <= thresh the step is done and counted; if it was the step's
 *   max_iters-th iteration the step is done, counted, and counted as unconverged -- not an error.  Every launch that finds
 *   `done` or `breakdown` set returns before it loads or stores anything, so the launches a step does not need cost a launch
 *   each and no memory traffic; the next step's start clears `done`.  Breakdown (lora_plan_run_cg_until's rule, also a start
 *   whose dot is not finite) is sticky for the run: d_u keeps the last good iterate and steps_done the steps finished before.
 *   At the end the call waits ONCE on `stream`, reads the states and the history back, and stores ONE
 *   lora_plan_residual_src(d_u, d_f) over the whole interior in r->steady: how far the last level is from the steady state.
 *   iterations (NULL, or `steps` ints): the iterations of each finished step; for the step a breakdown interrupted the
 *   iterations applied before it; 0 for the steps behind it.
 *   BIT CONTRACT: d_u after the run is bit for bit what a host loop over the public entries gives that calls, per step s,
 *   lora_plan_theta_start and then iterations[s] iterations as written above, alpha, beta, thresh and the stop test in host
 *   fp64 -- the driver launches the same kernels at the same geometry.
 *   No halo cell of d_u is ever written, d_f is never written, everything is ordered on `stream` alone.
 *   LORA_EINVAL unless 0 <= theta <= 1, tau > 0 and finite, steps >= 0, max_iters >= 1, rtol >= 0 and finite; for a null plan,
 *   d_u or r; for d_f == d_u or a caller's buffer that is one of the plan's grids.  LORA_EUNSUPPORTED for a misaligned buffer,
 *   a plan whose option "cg" reads 0, and taps that are not point-symmetric; then the reductions' codes.  steps == 0 returns
 *   LORA_OK and touches nothing.  BLOCKS (once, at its end).  Choose max_iters near the iterations a step needs: DESIGN 3.10
 *   has the cost of a launch that exits early. */
typedef struct lora_theta_result {
    int steps_done, breakdown, unconverged_steps;
    long long iterations_total; /* over the finished steps ...                                                     */
    int iterations_max;         /* ... and the largest of them                                                     */
    double last_rr0, last_rr;   /* r.r at the start of the last step begun and at the run's end (NaN: no step ran) */
    lora_grid_diff steady;      /* a = S(d_u) + f against b = d_u after the run                                    */
} lora_theta_result;
int lora_plan_run_theta(lora_plan *plan, void *d_u, const void *d_f, double theta, double tau, int steps, int max_iters, double rtol,
                        int *iterations, lora_theta_result *r, void *stream);
/* Allocate now what lora_plan_run_theta(..., steps) would allocate on first need: the three grids, the two states and the
 * history.  LORA_EINVAL for steps < 0, LORA_EUNSUPPORTED for a plan whose option "cg" reads 0. */
int lora_plan_prepare_theta(lora_plan *plan, int steps);

/* ---- geometric multigrid for u = S(u) + f (NEW).  Every solver above needs iterations that grow with the
 * grid's side; a V-cycle reduces the residual by a factor that does not.  fp64, 2D and 3D shapes.
 *   Coarsening is boundary-aligned and non-nested: a coarse grid spans the same interval as the fine one, from halo centre to
 * halo centre, with n_c interior cells per axis in place of n, so its spacing is H = h (n + 1) / (n_c + 1) and any extents will
 * do.  Prolongation is linear interpolation with position-dependent weights, restriction its scaled transpose, and the coarse
 * taps are the fine ones rescaled by (h / H)^2 per axis.
 *   Interpolation weights.  A fine index i and a coarse index j of one axis (both 0-based interior indices) have
 *     p(i, j) = max(0, 1 - |(i + 1)(n_c + 1) - (j + 1)(n + 1)| / (n + 1)),
 *   the numerator an exact integer; a coarse index outside [0, n_c) counts as a zero value (the zero halo of a correction).
 *   In more dimensions the weight is the product over the axes.
 *   Which plans (read-only option "mg": 1 or 0): plans whose option "cg" reads 1, of a 2D or 3D shape, for whose extents
 *   lora_mg_coarse_dims succeeds. */
/* Host only: the extents of the next coarser grid.  Per axis n_c = floor(n / 2), the innermost then rounded down to even (the
 * fast kernels need an even innermost extent): (70, 260) -> (35, 130), (9, 10) -> (4, 4), (250, 250) -> (125, 124),
 * (35, 17, 130) -> (17, 8, 64).  LORA_EINVAL for a null pointer, an unknown shape or an extent < 1; LORA_EUNSUPPORTED for a 1D
 * shape and when any n_c would be below 4. */
int lora_mg_coarse_dims(int shape, const int *dims, int *cdims);
/* Host only: the taps of the coarse operator from the fine taps `w` (lora_shape_ntaps doubles, as lora_plan_set_weights takes
 * them) for the grids `dims` -> `cdims`.  Per axis rho_a = (n_c + 1) / (n + 1) and q_a = rho_a^2 = (h / H)^2.  A tap at offset
 * d != 0 becomes wc = w prod_a q_a^(d_a^2 / |d|^2) -- exactly w q_a for a tap along one axis -- and the centre tap
 * wc[centre] = (sum of w) - (sum of the other wc), so the tap sum and point symmetry are kept: I - S scales like a second-order
 * operator, which is what point-symmetric taps (no first moment) are to leading order.  LORA_EINVAL for a null pointer, an
 * unknown shape or an extent < 1; LORA_EUNSUPPORTED for a 1D shape. */
int lora_mg_coarse_taps(int shape, const double *w, const int *dims, const int *cdims, double *wc);
/* The two transfer kernels.  `plan` is the FINE level's plan; the coarse grid is a padded array of the layout
 * lora_padded_count(shape, cdims) with cdims = lora_mg_coarse_dims(dims).  Both are ASYNCHRONOUS on `stream` like
 * lora_plan_cg_direction and take a capturing stream.  The buffer contract of this group holds (pieces of at most 16 bytes,
 * nothing outside the two padded arrays); the same call gives the same bits every time (no atomics, a fixed order); nothing is
 * contracted into a fused multiply-add.  Each output cell is a sum of exact integer numerators times values, scaled once:
 * within (terms + 4) 2^-53 sum |weight value| of the exact result, `terms` the non-zero weights of the cell.
 *   Status, in this order: LORA_EINVAL for a null plan or buffer, a non-finite scale, or equal buffers; LORA_EUNSUPPORTED for a
 *   misaligned buffer; LORA_EUNSUPPORTED for a plan whose option "mg" reads 0; LORA_ENODEVICE without a device. */
/* Restriction, a gather: on every interior cell j of the coarse grid
 *     d_coarse[j] = fl(scale (prod_a rho_a) sum_i prod_a p(i_a, j_a) d_fine[i]),
 * at most 5 fine cells per axis in range.  Only interior cells of d_fine are read; the halo of d_coarse is not written. */
int lora_plan_mg_restrict(lora_plan *plan, const void *d_fine, void *d_coarse, double scale, void *stream);
/* Prolongation and correction: on every interior cell i of the fine grid
 *     d_fine[i] = fl(d_fine[i] + sum_j prod_a p(i_a, j_a) d_coarse[j]),
 * at most 2 coarse cells per axis.  Halo cells of d_coarse are selected away before any arithmetic, so a NaN there reaches
 * nothing; the halo of d_fine is not written. */
int lora_plan_mg_prolong_add(lora_plan *plan, const void *d_coarse, void *d_fine, void *stream);
/* The defect of u = S(u) + f restricted in the launch that computes it (NEW; plan option "mgfuse").  `plan` is
 * the FINE level's plan and carries no source: f is an argument, as with lora_plan_defect (declared below); d_f may be NULL.
 * d_coarse has the layout of lora_mg_coarse_dims.  ASYNCHRONOUS: exactly one kernel on `stream` and nothing else -- no host
 * wait, no allocation; it takes a capturing stream.
 *   BIT CONTRACT.  On every interior cell of the coarse grid d_coarse holds exactly the bits of
 *     lora_plan_defect(plan, d_u, d_f, spare, 0, 0, stream);  lora_plan_mg_restrict(plan, spare, d_coarse, scale, stream);
 *   without the spare grid.  That fixes two orders.  The defect of a fine interior cell is fl(fl(acc + d_f) - d_u), with
 *   d_f == NULL fl(acc - d_u), acc with the bits lora_plan_step_region stores: the chain of fused multiply-adds of the plan's
 *   tile family from 0 over the plan's resolved tapset in its tap order.  The restriction sums as lora_plan_mg_restrict does: per
 *   fine row the 8 cells from the pair's first (even) column in ascending order, each integer numerator times its cell, into t;
 *   then s = s + fl(w t) over the rows inside the planes, both ascending, w the exact integer product of the outer axes'
 *   numerators, rows with w == 0 skipped; then fl(s coef), coef = scale prod_a rho_a / (n_a + 1) rounded once on the host in
 *   long double.  (A term with a zero numerator adds +0.0 to a sum that began at +0.0 and cannot move a bit.)  Nothing behind the
 *   tap sum is contracted; no atomics; the same call gives the same bits every time.
 *   Memory: pieces of at most 16 bytes; nothing outside the three padded arrays is touched.  d_u is read halo included (its halo
 *   holds the boundary values), d_f on interior cells alone; fine cells outside the interior have no defect and contribute
 *   nothing; the halo of d_coarse is neither read nor written; d_u and d_f are never written.
 *   Status, in this order: LORA_EINVAL for a null plan, d_u or d_coarse; LORA_EINVAL for a non-finite scale; LORA_EINVAL for any
 *   two buffers equal; LORA_EUNSUPPORTED for a misaligned buffer; LORA_EUNSUPPORTED for a plan whose option "mg" reads 0;
 *   LORA_ENODEVICE without a device. */
int lora_plan_mg_defect_restrict(lora_plan *plan, const void *d_u, const void *d_f, void *d_coarse, double scale, void *stream);
/* V-cycles until the TRUE residual of u = S(u) + f is small.  d_x holds the start iterate, the caller's boundary values in its
 * halo; d_f may be NULL.
 *   Levels.  Level 0 is the plan's grid with its taps w_0; level l + 1 has lora_mg_coarse_dims(dims_l) and
 *   w_(l+1) = lora_mg_coarse_taps(w_l).  The hierarchy is as deep as lora_mg_coarse_dims goes (16 levels at most), or
 *   m->max_levels levels (>= 2) if that is fewer.  On every level l below the coarsest, L, the smoother is damped Jacobi folded
 *   into a source sweep: with d_l = fl(1 - w_l[centre]) and c_l = fl(omega / d_l) an internal plan (lora_plan_create +
 *   lora_plan_set_weights + lora_plan_set_boundary(LORA_BC_DIRICHLET) + lora_plan_set_source(g_l)) carries the taps
 *   s_l[t] = fl(c_l w_l[t]) for t != centre, s_l[centre] = fl(fl(c_l w_l[centre]) + fl(1 - c_l)), and the source g_l, the
 *   level's right-hand side times c_l; g_0 = fl(c_0 d_f) is formed once per run (d_f == NULL: level 0 has no source).  Level
 *   L is a plain plan with the taps w_L.
 *   One cycle at level l < L:  m->pre applications of the smoothing plan on x_l, with the values lora_plan_run of that plan
 *   gives;  rs = lora_plan_defect(x_l, g_l) with that plan's taps, fl(fl(acc + g_l) - x_l) on the interior: c_l times the
 *   residual (the same bits as one more source sweep of it and a subtraction);
 *   lora_plan_mg_restrict(rs -> g_(l+1)) with scale = fl(c_(l+1) / c_l), or fl(1 / c_l) when l + 1 == L;  x_(l+1) = 0 over its
 *   whole padded grid;  the cycle at level l + 1;  lora_plan_mg_prolong_add(x_(l+1) -> x_l);  m->post applications.
 *   At level L:  r = g_L, p = r on the interior with a zero halo, rr = lora_plan_dot(r, r).dot, then m->coarse_iters (0: min(64,
 *   cells of the coarsest interior)) conjugate-gradient iterations on x_L exactly as lora_plan_run_cg_until writes them, with the
 *   same kernels, device-resident scalars and sticky halt flag, and no probe; a residual that vanishes exactly halts the
 *   level's remaining launches harmlessly.  With plan option "coarse1" on and a level L whose plan reads "cg_small" = 1 the level
 *   is instead ONE launch, lora_plan_cg_small(plan_L, x_L, g_L, iterations, sigma, tau) -- here and in the three drivers below.
 *   With plan option "mgfuse" on, the defect and the restriction of every level l < L are ONE launch,
 *   lora_plan_mg_defect_restrict(x_l, g_l -> g_(l+1)) with the same scale: the same bits in g_(l+1), rs never written -- here
 *   and in the three drivers below.
 *   A cycle is enqueued with NO host wait inside it.  u->check_every and u->max_times count CYCLES, and any check_every >= 1 is
 *   legal here; the other rules of `u`, the stop rule and the fields of r->until are lora_plan_run_until's (times_done counts
 *   cycles).  After each round the run probes the true residual of the caller's problem, S(d_x) + f - d_x with the plan's own
 *   taps, exactly as lora_plan_run_cg_until does: ONE lora_plan_residual_src under LORA_NORM_MAX, else a source sweep into the
 *   level's spare grid and lora_plan_diff.  The call BLOCKS at its probes only.
 *   BIT CONTRACT: d_x after k cycles is bit for bit what a caller gets by building the level plans from the formulas above and
 *   looping the public entries as written -- the residual subtraction and the g_0 scale single IEEE operations, the CG scalars
 *   divided in host fp64.
 *   Memory the plan owns (allocated on first need or by lora_plan_prepare_mg, never read before the run wrote it on `stream`,
 *   freed with the plan): two fine-size grids (g_0 and the spare), three grids per level in between, one grid and the CG set
 *   (three grids, the scalars) on the coarsest level.  d_x's halo is never written, d_f never at all.
 *   r->levels and r->level_dims (level 0 first) describe the hierarchy.
 *   LORA_EINVAL for a null plan, d_x, m, u or r; a bad `u`; pre < 0, post < 0 or pre + post < 1; omega not in (0, 2) or not
 *   finite; max_levels < 0 or == 1; coarse_iters < 0; d_f == d_x; a caller's buffer that is one of the plan's own.
 *   LORA_EUNSUPPORTED for a misaligned buffer, a plan whose option "mg" reads 0, taps that are not point-symmetric, and any
 *   level's d_l not positive and finite; then the reductions' codes.
 *   Limits: coarsening stops when any axis would go below 4, so a very thin grid (16 x 16384) gets a coarsest level that
 *   coarse_iters iterations do not solve, and convergence degrades; there is no semi-coarsening. */
typedef struct lora_mg {
    int pre, post;    /* smoothing applications before / after the coarse correction            */
    double omega;     /* damping of the Jacobi smoother, 0 < omega < 2 (0.8 is a good default)   */
    int max_levels;   /* 0 = as deep as lora_mg_coarse_dims goes, else >= 2                      */
    int coarse_iters; /* CG iterations on the coarsest level; 0 = min(64, its interior cells)    */
} lora_mg;
typedef struct lora_mg_result {
    lora_until_result until;
    int levels;
    int level_dims[16][3]; /* interior extents of level l, outermost first (2D: [l][2] = 0)    */
} lora_mg_result;
int lora_plan_run_mg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_mg *m, const lora_until *u, lora_mg_result *r,
                           void *stream);
/* Allocate now what lora_plan_run_mg_until(plan, ..., m, ...) would allocate on first need.  Status as that call's for `m` and
 * the plan; LORA_ENODEVICE without a device. */
int lora_plan_prepare_mg(lora_plan *plan, const lora_mg *m);
/* What the last cycle the plan enqueued took (lora_plan_run_mg_until, lora_plan_mg_precondition and the drivers on it), counted
 * while it was enqueued: the number of launches (kernels and memsets; a coarsest-level iteration is five) and the bytes they
 * move when every launch reads and writes each of its grids' interiors once (a zeroing writes the padded grid).  With plan
 * option "coarse1" on and a coarsest level that reads "cg_small" = 1 that level counts as one launch and four passes over its
 * cells: 5 + 5 iters - 1 launches fewer.  With plan option "mgfuse" on the defect and the restriction of a level below the
 * coarsest count as one launch that reads the level's cells twice with a source, once without, and writes the coarse cells
 * once: per such level one launch and exactly 16 bytes per cell of the level fewer.  LORA_EINVAL
 * for a null pointer or a plan on which no cycle has run. */
int lora_plan_mg_cycle_cost(const lora_plan *plan, int *launches, double *bytes);

/* ---- multigrid-preconditioned conjugate gradients, also for the implicit stepper's operator (NEW).  fp64, the
 * plans whose read-only option "mg" reads 1; the read-only option "pcg" reads the same value.  Every operation named below is
 * its own fp64 rounding; no atomics, fixed fold orders; pieces of at most 16 bytes, nothing outside the padded arrays;
 * everything ordered on the caller's stream alone; plan-owned memory is allocated on first need or by a prepare call and
 * written on the stream before it is read. */
/* The defect of u = S(u) + f in one launch: on every interior cell of [begin, end) d_out = fl(fl(acc + d_f) - d_u); with
 * d_f == NULL d_out = fl(acc - d_u), and no zero is added.  acc has exactly the bits lora_plan_step_region(plan, d_u, spare,
 * begin, end) stores.  lora_plan_theta_start without the scale, the second store and the dot: it writes no record and needs no
 * fold, so it is ASYNCHRONOUS on `stream` like lora_plan_cg_direction and takes a capturing stream.  d_u is read once, halo
 * included; d_f at the stored cells alone; the halo of d_out is neither read nor written.  Plans and range rules are those of
 * lora_plan_apply_dot (option "cg" = 1, no source on the plan, 1D included).
 *   Status, in this order: LORA_EINVAL for a null plan, d_u or d_out, a bad range or begin, any two buffers equal;
 *   LORA_EUNSUPPORTED for a misaligned buffer, then for a plan whose option "cg" reads 0; LORA_ENODEVICE without a device. */
int lora_plan_defect(lora_plan *plan, const void *d_u, const void *d_f, void *d_out, int begin, int end, void *stream);
/* ---- the whole small CG in one launch (NEW).  `iters` conjugate-gradient iterations for A = sigma I - tau S
 * on a grid small enough for ONE workgroup, in ONE launch: what the coarsest level of a V-cycle needs (plan option "coarse1").
 * fp64, 2D and 3D shapes, any taps, zero Dirichlet halo.  d_r holds the residual b - A x of the iterate in d_x on entry.
 *   Which plans (read-only option "cg_small": 1 or 0): plans whose option "cg" reads 1, of a 2D or 3D shape, with at most 4096
 *   interior cells (1024 lanes, four cells each in registers) and at most 64 KiB of LDS for p inside its ring of zeros:
 *   8 (32 + (m + 6)(n + 6)) bytes in 2D, 8 (32 + (h + 2)(m + 2)(n + 2)) in 3D.  4 x 512, 32 x 32, 64 x 64 and 12 x 12 x 12 fit,
 *   4 x 1024 does not.
 *   CONTRACT.  The interiors of d_x and d_r are read once, in 8-byte pieces; x, r, p, q stay in registers, p also in LDS inside a
 *   ring of zeros as wide as the tap radius, so no halo cell of either grid is read or written and nothing outside the padded
 *   arrays is touched; the interiors are written once, at the end.  p = r, rr = r.r, then per iteration, every named operation
 *   its own fp64 rounding (nothing contracted):
 *     q = fl(fl(sigma p) - fl(tau acc)), acc the sum of w[t] p[cell + offset t] as a chain of fused multiply-adds from 0 over the
 *     non-zero taps in ascending t; with sigma == tau == 1 the plain form q = fl(p - acc);
 *     pq = p.q;  alpha = rr / pq;  x = fl(x + fl(alpha p));  r = fl(r - fl(alpha q));
 *     rr' = r.r;  beta = rr' / rr;  p = fl(r + fl(beta p));  rr = rr'.
 *   A dot folds in a fixed order: with T = min(1024, cells rounded up to 64) lanes, lane t adds fl(a b) of its cells t, t + T,
 *   t + 2 T, ... (row-major interior index) from 0 in that order; the 64 lanes of a wave fold by the butterfly of the reductions
 *   (partner lane ^ 1, ^ 2, ... ^ 32); the waves' sums are added in wave order from wave 0's.  No atomics; every lane divides
 *   the same two sums in IEEE fp64, so the same call gives the same bits every time.
 *   Halting, uniform over the workgroup: rr == 0 before an iteration ends the loop as converged (halt 1); pq not finite or <= 0
 *   ends it as a breakdown (halt 2) and leaves x and r as they were before that iteration; a non-finite rr' ends it as a
 *   breakdown behind the update that produced it (that iteration counts).
 *   d_info: NULL, or four device doubles {rr0, rr, iterations done, halt}, 8-byte aligned, written by plain vector stores.
 *   ASYNCHRONOUS: one launch on `stream`, which may be capturing, like lora_plan_defect.
 *   Status, in this order: LORA_EINVAL for a null plan, d_x or d_r, d_x == d_r, iters < 0, a sigma or tau that is not finite;
 *   LORA_EUNSUPPORTED for a misaligned buffer, then for a plan whose option "cg_small" reads 0; then iters == 0 launches
 *   nothing and returns LORA_OK (it needs no device); LORA_ENODEVICE without a device. */
int lora_plan_cg_small(lora_plan *plan, void *d_x, void *d_r, int iters, double sigma, double tau, double *d_info, void *stream);
/* The V-cycle of lora_plan_run_mg_until for A = sigma I - tau S (both finite, tau >= 0, sigma > 0).  The coarse taps stay
 * lora_mg_coarse_taps of S: A = (sigma - tau) I + tau (I - S), and only the second-order part rescales.  Per level, with w the
 * level's taps:
 *     d = fl(sigma - fl(tau w[centre]))   (positive and finite, else LORA_EUNSUPPORTED)
 *     c = fl(omega / d),  c' = fl(c tau)
 *     s[t] = fl(c' w[t]) for t != centre,  s[centre] = fl(fl(c' w[centre]) + fl(1 - fl(c sigma)))
 * A smoothing application is one source sweep with the taps s and the source c b; lora_plan_defect of that plan is c (b - A x);
 * the restriction scales are lora_plan_run_mg_until's.  On the coarsest level the CG iterations apply
 * lora_plan_apply_dot_shift(sigma, tau) in place of lora_plan_apply_dot -- unless sigma == tau == 1, where every product with 1
 * is exact, the formulas give the d, c, s of lora_plan_run_mg_until bit for bit and the plain kernel runs.
 *   z = M r is ONE such cycle for A z = r from z = 0:  g_0 = fl(c_0 d_r) on the interior;  d_z zeroed over its whole padded
 *   array (its halo is the zero halo of a correction);  the cycle at level 0 with d_z as the iterate, the level's residual
 *   lora_plan_defect(x_l, g_l) of the smoothing plan.  ASYNCHRONOUS: no probe, no host wait.  Only interior cells of d_r are read.
 *   BIT CONTRACT: d_z is what a caller gets by composing the public entries as written: lora_plan_set_weights plans with the
 *   formulas above, lora_plan_defect, the transfers and the CG entries.
 *   Status as lora_plan_run_mg_until's for m, the plan, alignment, a caller's buffer that is one of the plan's own, point
 *   symmetry and the level diagonals; also LORA_EINVAL for d_r == d_z or a bad pair; LORA_ENODEVICE without a device.  The
 *   hierarchy is kept per plan for one (m->omega, m->max_levels, sigma, tau) at a time and rebuilt when they change;
 *   lora_plan_mg_cycle_cost afterwards reports this call's launches (the scale, the zeroing and the halo resets included). */
int lora_plan_mg_precondition(lora_plan *plan, const void *d_r, void *d_z, const lora_mg *m, double sigma, double tau, void *stream);
/* Preconditioned CG for u = S(u) + f until the TRUE residual is small: A = I - S, M the V-cycle above with sigma = tau = 1.
 * The plan owns one more grid, z, beside r, p, q and the hierarchy (lora_plan_prepare_pcg allocates all of it).
 *   Start-up:  r = lora_plan_defect(d_x, d_f);  z = M r;  p = z on the interior, with a zeroed halo;  rz = lora_plan_dot(r, z).dot.
 *   Iteration:
 *     pq = lora_plan_apply_dot(p, q).dot;  alpha = rz / pq;  rr' = lora_plan_cg_update(d_x, r, p, q, alpha).dot;
 *     z = M r;  rz' = lora_plan_dot(r, z).dot;  beta = rz' / rz;  lora_plan_cg_direction(p, z, beta);  rz = rz'
 *   The scalars stay on the device, one lane behind each fold; the history holds alpha and beta as in lora_plan_run_cg_until.
 *   Breakdown is sticky: pq not finite or <= 0; rz' not finite or < 0; a non-finite product; rz' == 0 (the residual vanished)
 *   halts the remaining launches in the same way.  The V-cycle's own launches do not test the halt word and still run after a
 *   halt: they write only z and the hierarchy's grids.  Every launch that could move d_x, r or p behind the start-up exits
 *   first, so d_x stays the last good iterate.
 *   Rounds, probe, stop rule and the fields of r->until are lora_plan_run_cg_until's (check_every even and >= 2; under
 *   LORA_NORM_MAX one lora_plan_residual_src per round, else a source sweep into q and lora_plan_diff; the state is read back
 *   in the probe's wait).  lambda_min / lambda_max: the Ritz values of M A from the run's coefficients (lora_cg_spectrum).
 *   BIT CONTRACT: d_x after k iterations is the host loop over the public entries as written, alpha and beta divided in host
 *   fp64.
 *   Status as lora_plan_run_mg_until's, and LORA_EINVAL unless m->pre == m->post >= 1 (the preconditioner must be symmetric;
 *   lora_plan_mg_precondition itself takes any m).  max_times < check_every returns LORA_OK and touches nothing. */
typedef struct lora_pcg_result {
    lora_until_result until;
    double lambda_min, lambda_max; /* Ritz values of M A from the run's coefficients; NaN if no iteration ran */
    int breakdown, levels;
} lora_pcg_result;
int lora_plan_run_pcg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_mg *m, const lora_until *u, lora_pcg_result *r,
                            void *stream);
/* Allocate now what lora_plan_run_pcg_until(plan, ..., m, u with this max_times, ...) would allocate on first need.  Status as
 * that call's for `m` and the plan; LORA_EINVAL for max_times < 0; LORA_ENODEVICE without a device. */
int lora_plan_prepare_pcg(lora_plan *plan, const lora_mg *m, int max_times);
/* lora_plan_run_theta with every step's solve preconditioned: the scheme, the argument rules, the result record and the
 * per-step stop rule rr' <= fl(rtol2 rr0) (rr = r.r from the update's dot, decided on the device) are that call's;
 * A = sigma I - tau' S is preconditioned by the hierarchy for (sigma, tau').  Per step:  lora_plan_theta_start into r and z (z is
 * overwritten next);  z = M r;  p = z with a zero halo;  rz;  then the iterations of lora_plan_run_pcg_until with
 * lora_plan_apply_dot_shift(sigma, tau').
 *   A V-cycle cannot exit early, so the run does not enqueue max_iters iterations blindly: after every check_every iterations
 *   (>= 1, any parity) the driver reads the state back -- one small copy and one stream wait -- and goes on to the next step
 *   once the step is done.  At most check_every - 1 iterations are enqueued past the one that meets the rule; their CG launches
 *   exit on `done`, their V-cycles run (DESIGN 3.12 has the cost).
 *   iterations[s], unconverged_steps, breakdown handling and the final `steady` probe are lora_plan_run_theta's.
 *   BIT CONTRACT: the host loop over the public entries, with iterations[s] iterations per step.
 *   Also LORA_EINVAL for a null or bad m, unless m->pre == m->post >= 1, and for check_every < 1; LORA_EUNSUPPORTED as
 *   lora_plan_mg_precondition for (sigma, tau').  theta == 0 is legal (A = I). */
int lora_plan_run_theta_mg(lora_plan *plan, void *d_u, const void *d_f, double theta, double tau, int steps, int max_iters, double rtol,
                           const lora_mg *m, int check_every, int *iterations, lora_theta_result *r, void *stream);
void lora_plan_destroy(lora_plan *plan);

/* ========================================================================================
 * D. Multi-GPU slabs (NEW: the reference is single-GPU).  The grid is cut along its outermost interior
 *    dimension into one slab per GPU; the time-step loop (2d/gpu.cu:544-546) runs on every slab with a nearest-
 *    neighbour ghost-zone exchange over RCCL (ncclSend / ncclRecv in one group, on a communication stream) overlapped
 *    with the interior sweeps.  N slabs == 1 GPU bit for bit (same kernels, same per-point arithmetic).
 *    Usual form: one process per GPU, each creating ONE slab with its rank and an RCCL communicator; the CLIs' --gpus N
 *    drive N slabs of one process (lora_run_host_multi).
 * ====================================================================================== */
typedef struct lora_slab lora_slab;

/* How neighbouring slabs exchange ghost rows.  All calls are made from the driving host thread; send / recv enqueue on
 * `stream` (a hipStream_t) and must not block the host; every exchange of a launch sits between one group_begin and
 * one group_end (called on the first slab's table).  `peer` is a rank of the decomposition. */
typedef struct lora_slab_comm {
    void *ctx;
    int (*group_begin)(void *ctx);
    int (*send)(void *ctx, const void *d_buf, size_t bytes, int peer, void *stream);
    int (*recv)(void *ctx, void *d_buf, size_t bytes, int peer, void *stream);
    int (*group_end)(void *ctx);
} lora_slab_comm;
/* RCCL: ctx = an ncclComm_t of this rank (ncclCommInitRank / ncclCommInitAll, or torch's); librccl.so is loaded on
 * first use, the engine library does not link it. */
int lora_slab_comm_rccl(lora_slab_comm *out, void *nccl_comm);
/* In-process loopback for `nranks` slabs that live in ONE process on ONE device: messages become device-to-device
 * copies ordered by events.  Fills out[0 .. nranks-1].  For tests / rehearsals on a one-GPU box. */
int lora_slab_comm_loopback(lora_slab_comm *out, int nranks);

enum lora_slab_flags {
    LORA_SLAB_NO_OVERLAP = 1,  /* sweep the whole slab, then exchange (no boundary-first split); the default
                                  in 2D and 3D: a fused launch is ONE round of workgroups sized to its region,
                                  so a thin boundary strip costs a third of a whole-slab launch (measured:
                                  DESIGN section 6)                                                           */
    LORA_SLAB_NO_DEFER = 2,    /* wait for an exchange at the end of its launch instead of inside the next   */
    LORA_SLAB_NO_FUSION = 4,   /* single sweeps only                                                         */
    LORA_SLAB_OVERLAP = 16,    /* boundary strips first, exchange overlapped with the interior (the default in
                                  1D; forces it in 2D / 3D)                                                   */
    LORA_SLAB_RING_OF_ONE = 8  /* nranks == 1: the slab is its own neighbour (periodic along the split
                                  dimension) -- the complete exchange path on one GPU; with the reference boundary
                                  a rehearsal of one rank's share of an N-GPU run, not a physical result      */
};
typedef struct lora_slab_desc {
    int shape, dtype;          /* lora_shape, lora_dtype                                                      */
    int global_dims[3];        /* interior extents of the WHOLE grid, outermost first                         */
    const double *params;      /* as lora_plan_create (NULL: the reference harness's table)                   */
    const double *weights;     /* nullable: taps applied per sweep, bypassing the params mapping              */
    int rank, nranks;          /* this slab and the number of slabs (GPUs)                                    */
    int device;                /* HIP device the slab lives on                                                */
    int exchange_every;        /* launches between ghost-zone refreshes; 0 = auto (by slab thickness) */
    int boundary;              /* LORA_BC_REFERENCE or LORA_BC_DIRICHLET                                      */
    int flags;                 /* lora_slab_flags                                                             */
    const char *options;       /* nullable "key=value,key=value": plan options, applied before the ghost depth is fixed */
} lora_slab_desc;
typedef struct lora_slab_info_t {
    int begin, end;            /* global interior range of the slab's own rows                                */
    int ghost, ghost_top, ghost_bottom;
    int apps_per_launch, exchange_every, steps_done;
    int local_dims[3];         /* interior extents of the local array (own + ghost rows)                      */
    long launches, exchanges;
    size_t local_bytes;        /* bytes of one local padded buffer                                            */
} lora_slab_info_t;

/* `comm` may be NULL for nranks == 1 without the ring flag.  Allocates the slab's two local buffers and streams. */
int lora_slab_create(lora_slab **slab, const lora_slab_desc *desc, const lora_slab_comm *comm);
void lora_slab_destroy(lora_slab *slab);
int lora_slab_info(const lora_slab *slab, lora_slab_info_t *info);
/* buffer 0 <- this slab's rows of the padded GLOBAL host array (ghost rows and pads included), buffer 1 <- 0 */
int lora_slab_load(lora_slab *slab, const void *host_global_padded);
/* the same from a LOCAL padded device array (own + ghost rows + pads), e.g. data generated on the device;
 * call lora_slab_refresh_ghosts afterwards */
int lora_slab_load_device(lora_slab *slab, const void *d_local_padded);
int lora_slab_refresh_ghosts(lora_slab *slab);
/* `times` kernel applications (fused launches from even time levels, single sweeps otherwise); asynchronous */
int lora_slab_run(lora_slab *slab, int times);
int lora_slab_sync(lora_slab *slab);
/* own rows (+ the pad rows at a global edge) of the current time level -> their place in the padded GLOBAL host array */
int lora_slab_store(lora_slab *slab, void *host_global_padded);
/* which = 0 / 1: the two local device buffers; anything else: the one holding the current time level */
void *lora_slab_buffer(lora_slab *slab, int which);
void *lora_slab_stream(lora_slab *slab); /* the hipStream_t its sweeps run on */
void *lora_slab_comm_stream(lora_slab *slab); /* the hipStream_t its ghost-zone exchanges run on */
lora_plan *lora_slab_plan(lora_slab *slab);
/* Several slabs of ONE decomposition driven by this host thread (one process, N devices): launches and exchanges are
 * interleaved across the slabs, every exchange inside one group. */
int lora_slab_run_many(lora_slab **slabs, int n, int times);
int lora_slab_refresh_ghosts_many(lora_slab **slabs, int n);
/* Group A's generic operator on `ngpus` devices of this node: one slab per device, RCCL from ncclCommInitAll.
 * (LORA_SLAB_LOOPBACK=1 in the environment: all slabs on device 0 with the loopback exchange -- one-GPU rehearsal.) */
int lora_run_host_multi(int shape, int dtype, const void *in, void *out, const double *params, int times,
                        const int *dims, int ngpus, int quiet, lora_run_info *info);

/* ========================================================================================
 * E. Two-axis block decomposition (NEW).  A Pa x Pb process grid cuts the two OUTER dimensions of the grid --
 *    rows x columns of the 2D shapes, planes x rows (z x y) of the 3D ones -- into one block per GPU.  A block's local
 *    array carries ghost zones of radius x applications-per-launch x E cells on every cut side; they are refreshed every E
 *    launches in two phases (axis B: strips packed by the block-copy kernel; then axis A: whole rows / planes in place,
 *    B-side ghost cells included, so corners need no diagonal message) over the same callback table as the slabs
 *    (peer = ia * Pb + ib), the second phase hidden behind the next launch's interior (deferred wait).  The loop that is
 *    distributed is the reference's time-step loop (2d/gpu.cu:544-546, 3d/gpu_star.cu:177-181); the reference itself has
 *    no multi-GPU path.  Reference boundary; fp64, and bf16 for the 3D shapes.  N blocks == 1 GPU bit for bit.
 * ====================================================================================== */
typedef struct lora_block lora_block;
typedef struct lora_block_desc {
    int shape, dtype;          /* a 2D or 3D lora_shape; lora_dtype                                          */
    int global_dims[3];        /* interior extents of the WHOLE grid, outermost first                         */
    int grid[2];               /* Pa x Pb: parts of the outermost (axis A) and of the second dimension (B)    */
    int coords[2];             /* this block: (ia, ib); its rank in the callback table is ia * Pb + ib        */
    const double *params;      /* as lora_plan_create (NULL: the reference harness's table)                   */
    const double *weights;     /* nullable: taps applied per sweep                                            */
    int device;                /* HIP device the block lives on                                               */
    int exchange_every;        /* launches between ghost-zone refreshes; 0 = 2; clipped to the thinnest block */
    int flags;                 /* LORA_SLAB_NO_DEFER, LORA_SLAB_NO_FUSION                                     */
    const char *options;       /* nullable "key=value,key=value": plan options                                */
} lora_block_desc;
typedef struct lora_block_info_t {
    int own_begin[2], own_end[2];    /* global interior ranges of the block's own cells along axis A / B     */
    int ghost, ghost_lo[2], ghost_hi[2];
    int apps_per_launch, exchange_every, steps_done;
    int local_dims[3];               /* interior extents of the local array (own + ghost cells)              */
    long launches, exchanges;
    size_t local_bytes;              /* bytes of one local padded buffer                                     */
    size_t bytes_per_refresh;        /* bytes this block sends per ghost-zone refresh (both phases)          */
} lora_block_info_t;
/* `comm` may be NULL for a 1 x 1 grid.  Allocates the block's two local buffers, its pack strips and streams. */
int lora_block_create(lora_block **block, const lora_block_desc *desc, const lora_slab_comm *comm);
void lora_block_destroy(lora_block *block);
int lora_block_info(const lora_block *block, lora_block_info_t *info);
/* buffer 0 <- this block's cells of the padded GLOBAL host array (ghost cells and pads included), buffer 1 <- 0 */
int lora_block_load(lora_block *block, const void *host_global_padded);
/* `times` kernel applications (fused launches from even time levels, single sweeps otherwise); asynchronous */
int lora_block_run(lora_block *block, int times);
/* several blocks of ONE decomposition driven by this host thread: every exchange phase inside one group */
int lora_block_run_many(lora_block **blocks, int n, int times);
int lora_block_sync(lora_block *block);
/* own cells (+ the pads at a global edge) of the current time level -> their place in the padded GLOBAL host array */
int lora_block_store(lora_block *block, void *host_global_padded);
void *lora_block_buffer(lora_block *block, int which);
void *lora_block_stream(lora_block *block);
void *lora_block_comm_stream(lora_block *block); /* the hipStream_t its ghost-zone exchanges run on */
lora_plan *lora_block_plan(lora_block *block);
/* Group A's generic operator on a grid[0] x grid[1] grid of blocks, one per device of this node (RCCL from
 * ncclCommInitAll; LORA_SLAB_LOOPBACK=1: all blocks on device 0 with the loopback exchange).  What the CLIs' --grid=AxB runs. */
int lora_run_host_blocks(int shape, int dtype, const void *in, void *out, const double *params, int times,
                         const int *dims, const int *grid, int quiet, lora_run_info *info);

/* ========================================================================================
 * C. Host helpers on the path.
 * ====================================================================================== */
/* The params tables the reference harness builds (1d/main.cu:77-78, 2d/main.cu:139-195,
 * 3d/main.cu:112-125).  Returns the tap count. */
int lora_default_params(int shape, double *params);
/* The taps the reference operator applies for `params` (see group A).  Returns the count. */
int lora_effective_weights(int shape, const double *params, double *weights);
/* Low-rank factor precompute of the box2d operator (2d/gpu.cu:280-350): pyramid peeling of a
 * symmetric 7x7 matrix into rank-1 terms u[t] (x) v[t], t = 0..3 (4x7 doubles each, row-major).
 * `residual_max` (nullable) receives max |params - sum_{t<3} u_t v_t^T|: the part the
 * reference silently drops. */
int lora_factorize_7x7(const double *params, double *u, double *v, double *residual_max);

/* Rank-revealing factorisation of ANY 7x7 tap matrix (one-sided Jacobi SVD):
 * weights = sum_k u[k] (x) v[k], u[k] = sigma_k a_k (vertical profile), v[k] = b_k (horizontal profile), k = 0..6 in
 * order of decreasing singular value sigma[k] (7x7, 7x7 and 7 doubles).  Keeping `r` terms leaves a residual of
 * spectral norm sigma[r].  The MFMA variant uses it for taps the pyramid factoriser cannot take. */
int lora_svd_7x7(const double *weights, double *u, double *v, double *sigma);

/* Exact rank-1 test of 3x3x3 taps as the bf16 sweeps see them (cast to fp32): returns 1 and fills
 * cba9 = {c[0..2] (x), b[0..2] (y), a[0..2] (z)} when fl(fl(a[dz] * b[dy]) * c[dx]) == w[dz][dy][dx] for all 27
 * taps, else 0.  Every box3d1r the reference can express passes (gpu_box_3d1r honours params[0..2] only,
 * 3d/gpu_box.cu:143-226); bf16 plans then evaluate the sweep as x-, y- and z-passes (plan option "separable",
 * default on; the evaluation order is documented in kernels_3d_bf16.hip and restated by the oracle). */
int lora_separable_3x3x3(const double *weights27, float *cba9);

/* bf16 <-> double on the host (round-to-nearest-even; bf16 values are bit patterns in uint16_t). */
void lora_f64_to_bf16(const double *src, uint16_t *dst, size_t count);
void lora_bf16_to_f64(const uint16_t *src, double *dst, size_t count);

/* glibc rand() stream (TYPE_3, seed 1 = the reference's un-seeded rand()) so that inputs are
 * identical on any libc.  Fill = (double)(rand() % mod): 1d/main.cu:105-109 (mod 10000),
 * 2d/main.cu:232-236 and 3d/main.cu:164-168 (mod 100). */
typedef struct lora_rng {
    int32_t r[34];
    int32_t pos;
} lora_rng;
void lora_rng_seed(lora_rng *g, unsigned seed);
int lora_rng_next(lora_rng *g);
void lora_fill_rand(double *dst, size_t count, int mod, lora_rng *g);

#ifdef __cplusplus
}
#endif
#endif /* LORASTENCIL_H */
