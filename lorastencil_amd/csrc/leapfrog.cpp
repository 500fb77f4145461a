// leapfrog.cpp -- the leapfrog entries of the C ABI (include/lorastencil.h): u(t+1) = S(u(t)) + c u(t-1), the new level stored
// over the oldest one.  One step in place (kernels_step.hip), two steps per launch in 2D (kernels_2d_step2.hip) and, behind option leap3, in 3D
// (kernels_3d_step2.hip), the
// run driver and the host-buffer operator.  `c` and the buffers are call arguments: nothing here changes what a plan resolves
// to, and no run is cached in a graph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

#include "engine.h"

namespace lora {

namespace {

// the two scratch grids alone (the probe grid of a Chebyshev run in progress stays)
void release_scratch(lora_plan *plan) {
    for (void *&b : plan->leap_scratch) {
        if (b) (void) hipFree(b);
        b = nullptr;
    }
    plan->leap_bytes = 0;
    plan->leap_device = -1;
}

}  // namespace

void release_leapfrog_state(lora_plan *plan) {
    release_scratch(plan);
    if (plan->cheb_probe) (void) hipFree(plan->cheb_probe);
    plan->cheb_probe = nullptr;
    plan->cheb_bytes = 0;
    plan->cheb_device = -1;
}

namespace {

bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

bool bad_range(const Plan &p, int begin, int end) {
    return begin < 0 || end > p.dims[0] || begin > end || begin % region_granularity(p) != 0;
}

int unsupported(const char *text) {
    set_last_error_text(text);
    return LORA_EUNSUPPORTED;
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
    if (lora_device_count() <= 0) {
        set_last_error_text("no HIP device visible");
        return LORA_ENODEVICE;
    }
    return LORA_EHIP;
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

// whether any two of the n buffers are equal (null entries -- an absent source -- equal nothing)
bool any_equal(const void *const *b, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (b[i] && b[i] == b[j]) return true;
    return false;
}

bool scratch_ready(const lora_plan *plan) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    return plan->leap_scratch[0] && plan->leap_scratch[1] && plan->leap_bytes == lora_plan_padded_bytes(plan) && plan->leap_device == dev;
}

bool ensure_scratch(lora_plan *plan) {
    if (scratch_ready(plan)) return true;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    release_scratch(plan);
    const size_t bytes = lora_plan_padded_bytes(plan);
    for (void *&b : plan->leap_scratch) {
        // (pads beyond the halo ring do not exist; the ring is copied per run, the interior written before it is read)
        if (hipMalloc(&b, bytes) != hipSuccess || hipMemset(b, 0, bytes) != hipSuccess) {
            (void) hipGetLastError();
            release_scratch(plan);
            return false;
        }
    }
    plan->leap_bytes = bytes;
    plan->leap_device = dev;
    return true;
}

// Whether a run of `times` steps takes two-step launches at all: plans of depth 2, a boundary that never writes a halo, the
// scratch grids allowed, at least one pair of launches.
bool run_fuses(const Plan &p, int times) {
    return leapfrog_depth(p) == 2 && p.boundary != LORA_BC_PERIODIC && p.use_scratch != 0 && times >= 4;
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
    if (lora::run_fuses(plan->p, times)) (void) lora::ensure_scratch(plan);  // (without them the run takes single steps)
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
    void *lv[2] = {d_prev, d_cur};  // lv[1] holds the newest level, lv[0] the one before it

    if (p.boundary == LORA_BC_PERIODIC) {
        // the newest level always carries its periodic images; the older one's halo is never read
        auto wrap = [&](void *buf) -> int {
            const int rc = lora_plan_halo(plan, buf, nullptr, LORA_HALO_WRAP, stream);
            if (rc == LORA_EHIP && lora_device_count() <= 0) {
                lora::set_last_error_text("no HIP device visible");
                return LORA_ENODEVICE;
            }
            return rc;
        };
        if (int rc = wrap(lv[1])) return rc;
        for (int i = 0; i < times; ++i) {
            if (int rc = lora::step1(p, lv[1], lv[0], c, 0, m, s)) return rc;
            if (int rc = wrap(lv[0])) return rc;
            std::swap(lv[0], lv[1]);
        }
        return LORA_OK;
    }

    // Pairs of two-step launches through the plan's scratch grids: (prev, cur) -> (s0, s1) -> (prev, cur).  s0 takes levels
    // that live in d_prev under the in-place driver and s1 levels that live in d_cur, so they carry those buffers' halos; four
    // steps later every level is where single steps leave it.
    int done = 0;
    if (lora::run_fuses(p, times) && lora::ensure_scratch(plan)) {
        void *s0 = plan->leap_scratch[0], *s1 = plan->leap_scratch[1];
        if (s0 != d_prev && s0 != d_cur && s1 != d_prev && s1 != d_cur) {
            if (int rc = lora_plan_halo(plan, s0, d_prev, LORA_HALO_COPY, stream)) return rc;
            if (int rc = lora_plan_halo(plan, s1, d_cur, LORA_HALO_COPY, stream)) return rc;
            for (int k = 0; k < times / 4; ++k) {
                if (int rc = lora::step2(p, d_prev, d_cur, s0, s1, c, 0, m, s)) return rc;
                if (int rc = lora::step2(p, s0, s1, d_prev, d_cur, c, 0, m, s)) return rc;
            }
            done = times / 4 * 4;
        }
    }
    for (int i = done; i < times; ++i) {
        if (int rc = lora::step1(p, lv[1], lv[0], c, 0, m, s)) return rc;
        std::swap(lv[0], lv[1]);
    }
    return LORA_OK;
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
    void *lv[2] = {d_prev, d_cur};  // lv[1] holds the newest level, lv[0] the one before it

    if (p.boundary == LORA_BC_PERIODIC) {
        // as lora_plan_run_leapfrog: the newest level always carries its periodic images; the older one's halo is never read
        auto wrap = [&](void *buf) -> int {
            const int rc = lora_plan_halo(plan, buf, nullptr, LORA_HALO_WRAP, stream);
            if (rc == LORA_EHIP && lora_device_count() <= 0) {
                lora::set_last_error_text("no HIP device visible");
                return LORA_ENODEVICE;
            }
            return rc;
        };
        if (int rc = wrap(lv[1])) return rc;
        for (int i = 0; i < times; ++i) {
            if (int rc = lora::step1_src(p, lv[1], lv[0], d_f, A(i), C(i), 0, m, s)) return rc;
            if (int rc = wrap(lv[0])) return rc;
            std::swap(lv[0], lv[1]);
        }
        return LORA_OK;
    }

    // lora_plan_run_leapfrog's schedule and scratch grids: (prev, cur) -> (s0, s1) -> (prev, cur), steps 4k .. 4k + 3
    int done = 0;
    if (lora::run_fuses(p, times) && lora::ensure_scratch(plan)) {
        void *s0 = plan->leap_scratch[0], *s1 = plan->leap_scratch[1];
        const void *all[5] = {d_prev, d_cur, d_f, s0, s1};
        if (!lora::any_equal(all, 5)) {
            if (int rc = lora_plan_halo(plan, s0, d_prev, LORA_HALO_COPY, stream)) return rc;
            if (int rc = lora_plan_halo(plan, s1, d_cur, LORA_HALO_COPY, stream)) return rc;
            for (int k = 0; k < times / 4; ++k) {
                const int i = 4 * k;
                if (int rc = lora::step2_src(p, d_prev, d_cur, d_f, s0, s1, A(i), C(i), A(i + 1), C(i + 1), 0, m, s)) return rc;
                if (int rc = lora::step2_src(p, s0, s1, d_f, d_prev, d_cur, A(i + 2), C(i + 2), A(i + 3), C(i + 3), 0, m, s)) return rc;
            }
            done = times / 4 * 4;
        }
    }
    for (int i = done; i < times; ++i) {
        if (int rc = lora::step1_src(p, lv[1], lv[0], d_f, A(i), C(i), 0, m, s)) return rc;
        std::swap(lv[0], lv[1]);
    }
    return LORA_OK;
}

int lora_run_host_leapfrog(int shape, const double *in_cur, const double *in_prev, double *out, const double *params, double c,
                           int times, const int *dims, int quiet, lora_run_info *info) {
    if (!in_cur || !in_prev || !out || !dims || times < 0 || !std::isfinite(c)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a leapfrog run")) return rc;
    if (lora_device_count() <= 0) {
        lora::set_last_error_text("no HIP device visible");
        return LORA_ENODEVICE;
    }
    lora_plan *plan = nullptr;
    int rc = lora_plan_create(&plan, shape, LORA_F64, dims, params);
    if (rc != LORA_OK) return rc;
    struct Guard {
        lora_plan *p;
        void *b[2] = {nullptr, nullptr};
        hipStream_t s = nullptr;
        ~Guard() {
            if (s) (void) hipStreamDestroy(s);
            for (void *x : b)
                if (x) (void) hipFree(x);
            lora_plan_destroy(p);
        }
    } g{plan};
    auto hip = [&](hipError_t e, const char *what) -> int {
        if (e == hipSuccess) return LORA_OK;
        lora::set_last_error(what, e);
        return LORA_EHIP;
    };
    using clock = std::chrono::steady_clock;
    const size_t bytes = lora_plan_padded_bytes(plan);
    const auto t_total0 = clock::now();
    for (void *&x : g.b)
        if (hipMalloc(&x, bytes) != hipSuccess) {
            (void) hipGetLastError();
            x = nullptr;
            return LORA_ENOMEM;
        }
    void *d_prev = g.b[0], *d_cur = g.b[1];
    if ((rc = hip(hipMemcpy(d_cur, in_cur, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    // set-up outside the timed region: the scratch grids, and one warm-up step (it writes d_prev, which is uploaded after it)
    if ((rc = lora_plan_prepare_leapfrog(plan, times))) return rc;
    if ((rc = hip(hipMemset(d_prev, 0, bytes), "warm-up"))) return rc;
    if (times > 0)
        if ((rc = lora_plan_step_leapfrog(plan, d_cur, d_prev, c, nullptr))) return rc;
    if ((rc = hip(hipDeviceSynchronize(), "warm-up"))) return rc;
    if ((rc = hip(hipMemcpy(d_prev, in_prev, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if ((rc = hip(hipStreamCreateWithFlags(&g.s, hipStreamNonBlocking), "stream"))) return rc;
    if ((rc = hip(hipDeviceSynchronize(), "upload"))) return rc;

    const auto t0 = clock::now();
    if ((rc = lora_plan_run_leapfrog(plan, d_prev, d_cur, c, times, g.s))) return rc;
    if ((rc = hip(hipStreamSynchronize(g.s), "run"))) return rc;
    const auto t1 = clock::now();
    if ((rc = hip(hipMemcpy(out, times % 2 ? d_prev : d_cur, bytes, hipMemcpyDeviceToHost), "download"))) return rc;
    const auto t_total1 = clock::now();

    double points = 1.0;
    for (int d = 0; d < plan->p.ndim; ++d) points *= dims[d];
    const int F = lora_shape_gstencil_factor(shape);
    lora_run_info ri;
    ri.sweep_seconds = std::chrono::duration<double>(t1 - t0).count();
    ri.total_seconds = std::chrono::duration<double>(t_total1 - t_total0).count();
    ri.gstencils = points * times / ri.sweep_seconds / 1e9;
    ri.gstencils_refconv = ri.gstencils * F;
    ri.hbm_gbs = points * times * 3.0 * sizeof(double) / ri.sweep_seconds / 1e9;  // cur and prev read, prev written
    ri.variant = plan->p.variant;
    ri.steps_per_launch = lora::leapfrog_depth(plan->p);
    lora::set_last_run_info(ri);
    if (info) *info = ri;
    if (!quiet) {
        const double secs = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() / 1e6;
        std::printf("%s\n", lora::run_label(shape));
        std::printf("Time = %lld[ms]\n", (long long) std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count());
        std::printf("GStencil/s = %f\n", points * times * F / secs / 1e9);
        std::fflush(stdout);
    }
    return LORA_OK;
}

}  // extern "C"
