// leapfrog.cpp -- the leapfrog entries of the C ABI (include/lorastencil.h): u(t+1) = S(u(t)) + c u(t-1), the new level stored
// over the oldest one, their forms with a source and a scale, a (S(u) + f) + c u-, and the variable-coefficient
// wave steps k(x) S(u) + b u + c u- (two per launch in 2D: kernels_2d_wave2.hip, and, behind option wave3, in 3D:
// kernels_3d_step2.hip).  One step in place (kernels_step.hip), two leapfrog steps per launch in 2D
// (kernels_2d_step2.hip) and, behind option leap3, in 3D (kernels_3d_step2.hip),
// the one run driver both rules go through (run_steps) and the host-buffer operator (its skeleton: hostrun.cpp).  The
// coefficients and the buffers are call arguments: nothing here changes what a plan resolves to, and no run is cached in a graph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "engine.h"

namespace lora {
namespace {

bool bad_range(const Plan &p, int begin, int end) {
    return begin < 0 || end > p.dims[0] || begin > end || begin % region_granularity(p) != 0;
}

// LORA_EUNSUPPORTED for the plans that have no leapfrog kernel (`two`: no two-step kernel)
int plan_refused(const Plan &p, bool two) {
    if (p.dtype != LORA_F64) return unsupported("bf16 plans have no leapfrog kernels");
    if (p.source) return unsupported("a plan with a source has no leapfrog kernels: remove the source first");
    if (p.ndim == 2 && p.variant != LORA_VARIANT_DIRECT) return unsupported("the 2D matrix-pipe variant has no leapfrog kernels");
    if (two && leapfrog_depth(p) < 2) return unsupported("two leapfrog steps per launch: 2D plans of the direct variant, 3D plans with option leap3 = 1, each with an even innermost extent");
    return LORA_OK;
}

// a launch error as a status: loud about a missing device, as the source path is
int failed(const char *what, hipError_t e) {
    set_last_error(what, e);
    return lora_device_count() <= 0 ? no_device() : LORA_EHIP;
}

int step1(const Plan &p, const void *d_cur, void *d_prev, double c, int begin, int end, hipStream_t s) {
    const hipError_t e = launch_leapfrog(p, static_cast<const double *>(d_cur), static_cast<double *>(d_prev), c, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("leapfrog kernel launch", e);
}

int step2(const Plan &p, const void *d_prev, const void *d_cur, void *d_out1, void *d_out2, double c, int begin, int end, hipStream_t s) {
    const hipError_t e = launch_leapfrog2(p, static_cast<const double *>(d_prev), static_cast<const double *>(d_cur),
                                          static_cast<double *>(d_out1), static_cast<double *>(d_out2), c, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("two-step leapfrog kernel launch", e);
}

int step1_src(const Plan &p, const void *d_cur, void *d_prev, const void *d_f, double a, double c, int begin, int end, hipStream_t s) {
    const hipError_t e = launch_leapfrog_src(p, static_cast<const double *>(d_cur), static_cast<double *>(d_prev),
                                             static_cast<const double *>(d_f), a, c, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("leapfrog kernel launch (source, scale)", e);
}

int step2_src(const Plan &p, const void *d_prev, const void *d_cur, const void *d_f, void *d_out1, void *d_out2, double a1, double c1,
              double a2, double c2, int begin, int end, hipStream_t s) {
    const hipError_t e = launch_leapfrog2_src(p, static_cast<const double *>(d_prev), static_cast<const double *>(d_cur),
                                              static_cast<const double *>(d_f), static_cast<double *>(d_out1),
                                              static_cast<double *>(d_out2), a1, c1, a2, c2, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("two-step leapfrog kernel launch (source, scale)", e);
}

int step1_wave(const Plan &p, const void *d_cur, void *d_prev, const void *d_k, double b, double c, int begin, int end, hipStream_t s) {
    const hipError_t e = launch_wave(p, static_cast<const double *>(d_cur), static_cast<double *>(d_prev), static_cast<const double *>(d_k),
                                     b, c, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("wave kernel launch", e);
}

int step2_wave(const Plan &p, const void *d_prev, const void *d_cur, const void *d_k, void *d_out1, void *d_out2, double b, double c,
               int begin, int end, hipStream_t s) {
    const hipError_t e = launch_wave2(p, static_cast<const double *>(d_prev), static_cast<const double *>(d_cur),
                                      static_cast<const double *>(d_k), static_cast<double *>(d_out1), static_cast<double *>(d_out2),
                                      b, c, begin, end, s);
    return e == hipSuccess ? LORA_OK : failed("two-step wave kernel launch", e);
}

// LORA_EUNSUPPORTED for the plans that have no wave kernel: those plan_refused refuses (`two`: plans of wave depth below 2)
int wave_refused(const Plan &p, bool two) {
    if (int rc = plan_refused(p, false)) return rc;
    if (two && wave_depth(p) < 2) return unsupported("two wave steps per launch: 2D plans of the direct variant, 3D plans with option wave3 = 1, each with an even innermost extent");
    return LORA_OK;
}

// whether any two of the n buffers are equal (null entries -- an absent source -- equal nothing)
bool any_equal(const void *const *b, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (b[i] && b[i] == b[j]) return true;
    return false;
}

// the two scratch grids, both or neither
bool ensure_scratch(lora_plan *plan) {
    const size_t bytes = lora_plan_padded_bytes(plan);
    // (not zeroed: the ring of each is copied per run, its interior written before it is read, all on the run's stream)
    if (plan->leap[0].ensure(bytes) && plan->leap[1].ensure(bytes)) return true;
    for (DeviceGrid &g : plan->leap) g.release();
    return false;
}

// Whether a run of `times` steps takes two-step launches at all: a rule of depth 2 on this plan (leapfrog_depth / wave_depth),
// a boundary that never writes a halo, the scratch grids allowed, at least one pair of launches.
bool run_fuses(const Plan &p, int depth, int times) {
    return depth == 2 && p.boundary != LORA_BC_PERIODIC && p.use_scratch != 0 && times >= 4;
}

// The run driver of every rule: `times` steps from (d_prev, d_cur), step i as step1(cur, prev, i) in place or, two at a time,
// step2(prev, cur, out1, out2, i) for steps i and i + 1.  d_f: the grid the steps read beside the levels (the source, the wave
// rule's k; nullptr = none).  depth: the rule's depth on this plan, 2 where step2 exists.
template <class Step1, class Step2>
int run_steps(lora_plan *plan, void *d_prev, void *d_cur, const void *d_f, int depth, int times, void *stream, Step1 step1, Step2 step2) {
    const Plan &p = plan->p;
    void *lv[2] = {d_prev, d_cur};  // lv[1] holds the newest level, lv[0] the one before it

    if (p.boundary == LORA_BC_PERIODIC) {
        // the newest level always carries its periodic images; the older one's halo is never read
        auto wrap = [&](void *buf) -> int {
            const int rc = lora_plan_halo(plan, buf, nullptr, LORA_HALO_WRAP, stream);
            return rc == LORA_EHIP && lora_device_count() <= 0 ? no_device() : rc;
        };
        if (int rc = wrap(lv[1])) return rc;
        for (int i = 0; i < times; ++i) {
            if (int rc = step1(lv[1], lv[0], i)) return rc;
            if (int rc = wrap(lv[0])) return rc;
            std::swap(lv[0], lv[1]);
        }
        return LORA_OK;
    }

    // Pairs of two-step launches through the plan's scratch grids: (prev, cur) -> (s0, s1) -> (prev, cur), steps 4k .. 4k + 3.
    // s0 takes levels that live in d_prev under the in-place driver and s1 levels that live in d_cur, so they carry those
    // buffers' halos; four steps later every level is where single steps leave it.
    int done = 0;
    if (run_fuses(p, depth, times) && ensure_scratch(plan)) {
        void *s0 = plan->leap[0].ptr, *s1 = plan->leap[1].ptr;
        const void *all[5] = {d_prev, d_cur, d_f, s0, s1};
        if (!any_equal(all, 5)) {
            if (int rc = lora_plan_halo(plan, s0, d_prev, LORA_HALO_COPY, stream)) return rc;
            if (int rc = lora_plan_halo(plan, s1, d_cur, LORA_HALO_COPY, stream)) return rc;
            for (int i = 0; i + 4 <= times; i += 4) {
                if (int rc = step2(d_prev, d_cur, s0, s1, i)) return rc;
                if (int rc = step2(s0, s1, d_prev, d_cur, i + 2)) return rc;
            }
            done = times / 4 * 4;
        }
    }
    for (int i = done; i < times; ++i) {
        if (int rc = step1(lv[1], lv[0], i)) return rc;
        std::swap(lv[0], lv[1]);
    }
    return LORA_OK;
}

}  // namespace
}  // namespace lora

using lora::Plan;

extern "C" {

int lora_plan_leapfrog_depth(const lora_plan *plan) { return plan ? lora::leapfrog_depth(plan->p) : 0; }

int lora_plan_step_leapfrog_region(lora_plan *plan, const void *d_cur, void *d_prev, double c, int begin, int end, void *stream) {
    if (!plan || !d_cur || !d_prev || !std::isfinite(c)) return LORA_EINVAL;
    const Plan &p = plan->p;
    if (lora::bad_range(p, begin, end) || d_cur == d_prev) return LORA_EINVAL;
    if (lora::misaligned(d_cur) || lora::misaligned(d_prev)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, false)) return rc;
    return lora::step1(p, d_cur, d_prev, c, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step_leapfrog(lora_plan *plan, const void *d_cur, void *d_prev, double c, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step_leapfrog_region(plan, d_cur, d_prev, c, 0, plan->p.dims[0], stream);
}

int lora_plan_step2_leapfrog_region(lora_plan *plan, const void *d_prev, const void *d_cur, void *d_out1, void *d_out2, double c,
                                    int begin, int end, void *stream) {
    if (!plan || !d_prev || !d_cur || !d_out1 || !d_out2 || !std::isfinite(c)) return LORA_EINVAL;
    const Plan &p = plan->p;
    if (lora::bad_range(p, begin, end)) return LORA_EINVAL;
    const void *b[4] = {d_prev, d_cur, d_out1, d_out2};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (b[i] == b[j]) return LORA_EINVAL;
    for (const void *x : b)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, true)) return rc;
    return lora::step2(p, d_prev, d_cur, d_out1, d_out2, c, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step2_leapfrog(lora_plan *plan, const void *d_prev, const void *d_cur, void *d_out1, void *d_out2, double c,
                             void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step2_leapfrog_region(plan, d_prev, d_cur, d_out1, d_out2, c, 0, plan->p.dims[0], stream);
}

int lora_plan_prepare_leapfrog(lora_plan *plan, int times) {
    if (!plan || times < 0) return LORA_EINVAL;
    if (int rc = lora::plan_refused(plan->p, false)) return rc;
    if (lora::run_fuses(plan->p, lora::leapfrog_depth(plan->p), times)) (void) lora::ensure_scratch(plan);  // (without them the run takes single steps)
    return LORA_OK;
}

int lora_plan_run_leapfrog(lora_plan *plan, void *d_prev, void *d_cur, double c, int times, void *stream) {
    if (!plan || !d_prev || !d_cur || !std::isfinite(c) || times < 0 || d_prev == d_cur) return LORA_EINVAL;
    const Plan &p = plan->p;
    if (lora::misaligned(d_prev) || lora::misaligned(d_cur)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, false)) return rc;
    if (times == 0) return LORA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = p.dims[0];
    return lora::run_steps(
        plan, d_prev, d_cur, nullptr, lora::leapfrog_depth(p), times, stream,
        [&](const void *cur, void *prev, int) { return lora::step1(p, cur, prev, c, 0, m, s); },
        [&](const void *prev, const void *cur, void *o1, void *o2, int) { return lora::step2(p, prev, cur, o1, o2, c, 0, m, s); });
}

// ---- a (S(u) + f) + c u-: the same entries with a source and a scale as call arguments ------------------------
int lora_plan_step_leapfrog_src_region(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_f, double a, double c, int begin,
                                       int end, void *stream) {
    if (!plan || !d_cur || !d_prev || !std::isfinite(a) || !std::isfinite(c)) return LORA_EINVAL;
    const Plan &p = plan->p;
    const void *b[3] = {d_cur, d_prev, d_f};
    if (lora::bad_range(p, begin, end) || lora::any_equal(b, 3)) return LORA_EINVAL;
    for (const void *x : b)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, false)) return rc;
    return lora::step1_src(p, d_cur, d_prev, d_f, a, c, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step_leapfrog_src(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_f, double a, double c, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step_leapfrog_src_region(plan, d_cur, d_prev, d_f, a, c, 0, plan->p.dims[0], stream);
}

int lora_plan_step2_leapfrog_src_region(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_f, void *d_out1,
                                        void *d_out2, double a1, double c1, double a2, double c2, int begin, int end, void *stream) {
    if (!plan || !d_prev || !d_cur || !d_out1 || !d_out2) return LORA_EINVAL;
    if (!std::isfinite(a1) || !std::isfinite(c1) || !std::isfinite(a2) || !std::isfinite(c2)) return LORA_EINVAL;
    const Plan &p = plan->p;
    const void *b[5] = {d_prev, d_cur, d_out1, d_out2, d_f};
    if (lora::bad_range(p, begin, end) || lora::any_equal(b, 5)) return LORA_EINVAL;
    for (const void *x : b)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, true)) return rc;
    return lora::step2_src(p, d_prev, d_cur, d_f, d_out1, d_out2, a1, c1, a2, c2, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step2_leapfrog_src(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_f, void *d_out1, void *d_out2,
                                 double a1, double c1, double a2, double c2, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step2_leapfrog_src_region(plan, d_prev, d_cur, d_f, d_out1, d_out2, a1, c1, a2, c2, 0, plan->p.dims[0], stream);
}

int lora_plan_run_leapfrog_src(lora_plan *plan, void *d_prev, void *d_cur, const void *d_f, const double *a, const double *c, int ncoef,
                               int times, void *stream) {
    if (!plan || !d_prev || !d_cur || !a || !c || ncoef < 1 || times < 0) return LORA_EINVAL;
    for (int i = 0; i < std::min(times, ncoef); ++i)  // the entries this run uses
        if (!std::isfinite(a[i]) || !std::isfinite(c[i])) return LORA_EINVAL;
    const void *b[3] = {d_prev, d_cur, d_f};
    if (lora::any_equal(b, 3)) return LORA_EINVAL;
    const Plan &p = plan->p;
    for (const void *x : b)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::plan_refused(p, false)) return rc;
    if (times == 0) return LORA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = p.dims[0];
    auto A = [&](int i) { return a[std::min(i, ncoef - 1)]; };
    auto C = [&](int i) { return c[std::min(i, ncoef - 1)]; };
    return lora::run_steps(
        plan, d_prev, d_cur, d_f, lora::leapfrog_depth(p), times, stream,
        [&](const void *cur, void *prev, int i) { return lora::step1_src(p, cur, prev, d_f, A(i), C(i), 0, m, s); },
        [&](const void *prev, const void *cur, void *o1, void *o2, int i) {
            return lora::step2_src(p, prev, cur, d_f, o1, o2, A(i), C(i), A(i + 1), C(i + 1), 0, m, s);
        });
}

// ---- k S(u) + b u + c u-: a per-cell coefficient grid and a term in u itself, all call arguments ---------------
int lora_plan_wave_depth(const lora_plan *plan) { return plan ? lora::wave_depth(plan->p) : 0; }

int lora_plan_step_wave_region(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_k, double b, double c, int begin, int end,
                               void *stream) {
    if (!plan || !d_cur || !d_prev || !d_k || !std::isfinite(b) || !std::isfinite(c)) return LORA_EINVAL;
    const Plan &p = plan->p;
    const void *bufs[3] = {d_cur, d_prev, d_k};
    if (lora::bad_range(p, begin, end) || lora::any_equal(bufs, 3)) return LORA_EINVAL;
    for (const void *x : bufs)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::wave_refused(p, false)) return rc;
    return lora::step1_wave(p, d_cur, d_prev, d_k, b, c, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step_wave(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_k, double b, double c, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step_wave_region(plan, d_cur, d_prev, d_k, b, c, 0, plan->p.dims[0], stream);
}

int lora_plan_step2_wave_region(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_k, void *d_out1, void *d_out2,
                                double b, double c, int begin, int end, void *stream) {
    if (!plan || !d_prev || !d_cur || !d_k || !d_out1 || !d_out2 || !std::isfinite(b) || !std::isfinite(c)) return LORA_EINVAL;
    const Plan &p = plan->p;
    const void *bufs[5] = {d_prev, d_cur, d_out1, d_out2, d_k};
    if (lora::bad_range(p, begin, end) || lora::any_equal(bufs, 5)) return LORA_EINVAL;
    for (const void *x : bufs)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::wave_refused(p, true)) return rc;
    return lora::step2_wave(p, d_prev, d_cur, d_k, d_out1, d_out2, b, c, begin, end, static_cast<hipStream_t>(stream));
}

int lora_plan_step2_wave(lora_plan *plan, const void *d_prev, const void *d_cur, const void *d_k, void *d_out1, void *d_out2, double b,
                         double c, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step2_wave_region(plan, d_prev, d_cur, d_k, d_out1, d_out2, b, c, 0, plan->p.dims[0], stream);
}

int lora_plan_prepare_wave(lora_plan *plan, int times) {
    if (!plan || times < 0) return LORA_EINVAL;
    if (int rc = lora::wave_refused(plan->p, false)) return rc;
    if (lora::run_fuses(plan->p, lora::wave_depth(plan->p), times)) (void) lora::ensure_scratch(plan);  // (without them: single steps)
    return LORA_OK;
}

int lora_plan_run_wave(lora_plan *plan, void *d_prev, void *d_cur, const void *d_k, double b, double c, int times, void *stream) {
    if (!plan || !d_prev || !d_cur || !d_k || !std::isfinite(b) || !std::isfinite(c) || times < 0) return LORA_EINVAL;
    const void *bufs[3] = {d_prev, d_cur, d_k};
    if (lora::any_equal(bufs, 3)) return LORA_EINVAL;
    const Plan &p = plan->p;
    for (const void *x : bufs)
        if (lora::misaligned(x)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::wave_refused(p, false)) return rc;
    if (times == 0) return LORA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = p.dims[0];
    return lora::run_steps(
        plan, d_prev, d_cur, d_k, lora::wave_depth(p), times, stream,
        [&](const void *cur, void *prev, int) { return lora::step1_wave(p, cur, prev, d_k, b, c, 0, m, s); },
        [&](const void *prev, const void *cur, void *o1, void *o2, int) {
            return lora::step2_wave(p, prev, cur, d_k, o1, o2, b, c, 0, m, s);
        });
}

int lora_run_host_leapfrog(int shape, const double *in_cur, const double *in_prev, double *out, const double *params, double c,
                           int times, const int *dims, int quiet, lora_run_info *info) {
    if (!in_cur || !in_prev || !out || !dims || times < 0 || !std::isfinite(c)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a leapfrog run")) return rc;
    lora::HostRun g;
    int rc = g.open(shape, LORA_F64, dims, params);
    if (rc != LORA_OK) return rc;
    lora_plan *plan = g.plan;
    const size_t bytes = g.bytes;
    if (g.alloc(2) != hipSuccess) return LORA_ENOMEM;
    void *d_prev = g.b[0], *d_cur = g.b[1];
    if ((rc = lora::hip_status(hipMemcpy(d_cur, in_cur, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    // set-up outside the timed region: the scratch grids, and one warm-up step (it writes d_prev, which is uploaded after it)
    if ((rc = lora_plan_prepare_leapfrog(plan, times))) return rc;
    if ((rc = lora::hip_status(hipMemset(d_prev, 0, bytes), "warm-up"))) return rc;
    if (times > 0)
        if ((rc = lora_plan_step_leapfrog(plan, d_cur, d_prev, c, nullptr))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "warm-up"))) return rc;
    if ((rc = lora::hip_status(hipMemcpy(d_prev, in_prev, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if ((rc = lora::hip_status(g.stream(), "stream"))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "upload"))) return rc;

    g.tic();
    if ((rc = lora_plan_run_leapfrog(plan, d_prev, d_cur, c, times, g.s))) return rc;
    if ((rc = lora::hip_status(hipStreamSynchronize(g.s), "run"))) return rc;
    g.toc();
    if ((rc = lora::hip_status(hipMemcpy(out, times % 2 ? d_prev : d_cur, bytes, hipMemcpyDeviceToHost), "download"))) return rc;
    return g.finish(times, 3.0, lora::leapfrog_depth(plan->p), quiet, info);  // cur and prev read, prev written
}

int lora_run_host_wave(int shape, const double *in_cur, const double *in_prev, const double *kappa, double *out, const double *params,
                       double b, double c, int laplacian, int times, const int *dims, int quiet, lora_run_info *info) {
    if (!in_cur || !in_prev || !kappa || !out || !dims || times < 0 || !std::isfinite(b) || !std::isfinite(c)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a wave run")) return rc;
    lora::HostRun g;
    int rc = g.open(shape, LORA_F64, dims, params);
    if (rc != LORA_OK) return rc;
    lora_plan *plan = g.plan;
    if (laplacian) {
        // the zero-sum form of the taps: centre - s, s the sum of all taps in table order
        double w[49];
        const int ntaps = plan->p.ntaps;
        if ((rc = lora_plan_get_weights(plan, w, ntaps))) return rc;
        double sum = 0.0;
        for (int t = 0; t < ntaps; ++t) sum += w[t];
        w[ntaps / 2] -= sum;
        if ((rc = lora_plan_set_weights(plan, w, ntaps))) return rc;
    }
    const size_t bytes = g.bytes;
    if (g.alloc(3) != hipSuccess) return LORA_ENOMEM;
    void *d_prev = g.b[0], *d_cur = g.b[1], *d_k = g.b[2];
    if ((rc = lora::hip_status(hipMemcpy(d_cur, in_cur, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if ((rc = lora::hip_status(hipMemcpy(d_k, kappa, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    // set-up outside the timed region: the scratch grids, and one warm-up step (it writes d_prev, which is uploaded after it)
    if ((rc = lora_plan_prepare_wave(plan, times))) return rc;
    if ((rc = lora::hip_status(hipMemset(d_prev, 0, bytes), "warm-up"))) return rc;
    if (times > 0)
        if ((rc = lora_plan_step_wave(plan, d_cur, d_prev, d_k, b, c, nullptr))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "warm-up"))) return rc;
    if ((rc = lora::hip_status(hipMemcpy(d_prev, in_prev, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if ((rc = lora::hip_status(g.stream(), "stream"))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "upload"))) return rc;

    g.tic();
    if ((rc = lora_plan_run_wave(plan, d_prev, d_cur, d_k, b, c, times, g.s))) return rc;
    if ((rc = lora::hip_status(hipStreamSynchronize(g.s), "run"))) return rc;
    g.toc();
    if ((rc = lora::hip_status(hipMemcpy(out, times % 2 ? d_prev : d_cur, bytes, hipMemcpyDeviceToHost), "download"))) return rc;
    return g.finish(times, 4.0, lora::wave_depth(plan->p), quiet, info);  // cur, prev and k read, prev written
}

}  // extern "C"
