// chebyshev.cpp -- the Chebyshev semi-iteration on top of the scaled leapfrog step with a source (leapfrog.cpp:
// lora_plan_run_leapfrog_src):   u(k+1) = w(k+1) (S(u(k)) + f) + (1 - w(k+1)) u(k-1)
// solves u = S(u) + f in O(N) steps on an N-wide grid where Jacobi (lora_plan_run_until with a source) needs O(N^2).
// The coefficient schedule (host only), the run-until driver with a true-residual probe, and the host-buffer operator.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "engine.h"

namespace lora {
namespace {

// w(1) = 1, w(2) = 1 / (1 - rho^2 / 2), w(k+1) = 1 / (1 - rho^2 w(k) / 4): one object, one order of operations -- the driver
// below and lora_chebyshev_coeffs give the same bits for the same step.
struct Omega {
    double rho2;
    int k = 0;  // the step `w` belongs to (0: none yet)
    double w = 0.0;
    explicit Omega(double rho) : rho2(rho * rho) {}
    double next() {
        ++k;
        w = k == 1 ? 1.0 : (k == 2 ? 1.0 / (1.0 - rho2 / 2.0) : 1.0 / (1.0 - rho2 * w / 4.0));
        return w;
    }
};

bool bad_rho(double rho) { return !(rho >= 0.0 && rho < 1.0); }  // (a NaN fails both)

bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int unsupported(const char *text) {
    set_last_error_text(text);
    return LORA_EUNSUPPORTED;
}

bool ensure_probe(lora_plan *plan) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    const size_t bytes = lora_plan_padded_bytes(plan);
    if (plan->cheb_probe && plan->cheb_bytes == bytes && plan->cheb_device == dev) return true;
    if (plan->cheb_probe) (void) hipFree(plan->cheb_probe);
    plan->cheb_probe = nullptr;
    // (only interior cells of it are ever read, each after the probe's sweep wrote it)
    if (hipMalloc(&plan->cheb_probe, bytes) != hipSuccess || hipMemset(plan->cheb_probe, 0, bytes) != hipSuccess) {
        (void) hipGetLastError();
        if (plan->cheb_probe) (void) hipFree(plan->cheb_probe);
        plan->cheb_probe = nullptr;
        return false;
    }
    plan->cheb_bytes = bytes;
    plan->cheb_device = dev;
    return true;
}

bool bad_until(const lora_until *u) {
    if (u->check_every < 2 || u->check_every % 2 || u->max_times < 0) return true;
    if (u->norm != LORA_NORM_MAX && u->norm != LORA_NORM_RMS) return true;
    return !(u->tol >= 0.0) || !(u->rtol >= 0.0);
}

}  // namespace
}  // namespace lora

using lora::Plan;

extern "C" {

int lora_chebyshev_coeffs(double rho, int first_step, int count, double *a, double *c) {
    if (lora::bad_rho(rho) || first_step < 1 || count < 0 || (count > 0 && (!a || !c))) return LORA_EINVAL;
    lora::Omega om(rho);
    for (int k = 1; k < first_step; ++k) (void) om.next();
    for (int i = 0; i < count; ++i) {
        a[i] = om.next();
        c[i] = 1.0 - a[i];
    }
    return LORA_OK;
}

int lora_plan_run_chebyshev_until(lora_plan *plan, void *d_prev, void *d_cur, const void *d_f, double rho, const lora_until *u,
                                  lora_until_result *r, void *stream) {
    if (!plan || !d_prev || !d_cur || !u || !r || lora::bad_rho(rho) || lora::bad_until(u)) return LORA_EINVAL;
    if (d_prev == d_cur || (d_f && (d_f == d_prev || d_f == d_cur))) return LORA_EINVAL;
    if (lora::misaligned(d_prev) || lora::misaligned(d_cur) || lora::misaligned(d_f))
        return lora::unsupported("device buffers must be 16-byte aligned");
    const Plan &p = plan->p;
    if (lora::leapfrog_depth(p) == 0)
        return lora::unsupported(p.source ? "a plan with a source has no leapfrog kernels: the source of a Chebyshev run is a call argument"
                                          : "this plan has no leapfrog kernels (bf16, or the 2D matrix-pipe variant)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_prev, d_cur, s)) return rc;
    *r = {0, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}};
    if (u->max_times < u->check_every) return LORA_OK;
    // under the max norm every deciding field of the fused residual (lora_plan_residual_src) is bit for bit the two-pass
    // probe's; sum_sq -- the RMS norm's -- is summed in another order there, so that norm keeps the two passes and their grid
    const bool fused = u->norm == LORA_NORM_MAX && lora::has_fused_residual(p);
    if (!fused) {
        if (!lora::ensure_probe(plan)) return LORA_ENOMEM;
        if (plan->cheb_probe == d_prev || plan->cheb_probe == d_cur || plan->cheb_probe == d_f) return LORA_EINVAL;
    }
    (void) lora_plan_prepare_leapfrog(plan, u->check_every);

    // the two-pass probe's sweep (unused by the fused one): the plan's own single sweep with f as its source -- a copy of
    // the plan's resolved state, so the caller's plan keeps its options, kernel name, signature and leapfrog depth
    Plan probe = p;
    if (!fused) probe.source = d_f;
    lora::Omega om(rho);
    std::vector<double> a(u->check_every), c(u->check_every);
    while (r->times_done + u->check_every <= u->max_times) {
        for (int i = 0; i < u->check_every; ++i) {
            a[i] = om.next();
            c[i] = 1.0 - a[i];
        }
        // an even run: the newest level is back in d_cur (under the periodic boundary with its images)
        if (int rc = lora_plan_run_leapfrog_src(plan, d_prev, d_cur, d_f, a.data(), c.data(), u->check_every, u->check_every, stream)) return rc;
        r->times_done += u->check_every;
        // the TRUE residual S(u) + f - u of that level, d_prev and d_cur untouched: reduced inside one sweep where the plan has
        // that kernel, else one sweep into the probe grid and one difference
        if (fused) {
            if (int rc = lora::residual_whole(plan, d_cur, d_f, &r->last, s)) return rc;
        } else {
            if (int rc = lora::launch_apps(probe, {1, 0, p.dims[0]}, d_cur, plan->cheb_probe, s)) return rc;
            if (int rc = lora::diff_whole(plan, plan->cheb_probe, d_cur, &r->last, s)) return rc;
        }
        r->checks += 1;
        r->residual = u->norm == LORA_NORM_RMS ? std::sqrt(r->last.sum_sq / (double) r->last.count) : r->last.max_abs;
        if (r->last.nonfinite > 0) {
            r->diverged = 1;
            break;
        }
        if (r->residual <= u->tol + u->rtol * r->last.a_abs_max) {
            r->converged = 1;
            break;
        }
    }
    return LORA_OK;
}

int lora_run_host_chebyshev(int shape, const double *in, const double *source, double *out, const double *params, double rho, int times,
                            const lora_until *u, lora_until_result *r, const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || lora::bad_rho(rho)) return LORA_EINVAL;
    if (u ? (!r || lora::bad_until(u)) : times < 0) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a Chebyshev run (its source is an argument)")) return rc;
    if (lora_device_count() <= 0) {
        lora::set_last_error_text("no HIP device visible");
        return LORA_ENODEVICE;
    }
    lora_plan *plan = nullptr;
    int rc = lora_plan_create(&plan, shape, LORA_F64, dims, params);
    if (rc != LORA_OK) return rc;
    struct Guard {
        lora_plan *p;
        void *b[3] = {nullptr, nullptr, nullptr};
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
    for (int i = 0; i < (source ? 3 : 2); ++i)
        if (hipMalloc(&g.b[i], bytes) != hipSuccess) {
            (void) hipGetLastError();
            g.b[i] = nullptr;
            return LORA_ENOMEM;
        }
    void *d_prev = g.b[0], *d_cur = g.b[1], *d_f = g.b[2];
    if ((rc = hip(hipMemcpy(d_cur, in, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if (source)
        if ((rc = hip(hipMemcpy(d_f, source, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    // set-up outside the timed region: the scratch grids, and one warm-up step (it writes d_prev, which is uploaded after it)
    const int cap = u ? u->max_times : times;
    if ((rc = lora_plan_prepare_leapfrog(plan, u ? u->check_every : times))) return rc;
    if ((rc = hip(hipMemset(d_prev, 0, bytes), "warm-up"))) return rc;
    if (cap > 0)
        if ((rc = lora_plan_step_leapfrog_src(plan, d_cur, d_prev, d_f, 1.0, 0.0, nullptr))) return rc;
    if ((rc = hip(hipDeviceSynchronize(), "warm-up"))) return rc;
    if ((rc = hip(hipMemcpy(d_prev, in, bytes, hipMemcpyHostToDevice), "upload"))) return rc;  // both levels start as `in`
    if ((rc = hip(hipStreamCreateWithFlags(&g.s, hipStreamNonBlocking), "stream"))) return rc;
    if ((rc = hip(hipDeviceSynchronize(), "upload"))) return rc;

    int done = times;
    const auto t0 = clock::now();
    if (u) {
        if ((rc = lora_plan_run_chebyshev_until(plan, d_prev, d_cur, d_f, rho, u, r, g.s))) return rc;
        done = r->times_done;
    } else {
        std::vector<double> a(times > 0 ? times : 1), c(a.size());
        if ((rc = lora_chebyshev_coeffs(rho, 1, times, a.data(), c.data()))) return rc;
        if ((rc = lora_plan_run_leapfrog_src(plan, d_prev, d_cur, d_f, a.data(), c.data(), (int) a.size(), times, g.s))) return rc;
        if (r) *r = {times, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}};
    }
    if ((rc = hip(hipStreamSynchronize(g.s), "run"))) return rc;
    const auto t1 = clock::now();
    if ((rc = hip(hipMemcpy(out, done % 2 ? d_prev : d_cur, bytes, hipMemcpyDeviceToHost), "download"))) return rc;
    const auto t_total1 = clock::now();

    double points = 1.0;
    for (int d = 0; d < plan->p.ndim; ++d) points *= dims[d];
    const int F = lora_shape_gstencil_factor(shape);
    lora_run_info ri;
    ri.sweep_seconds = std::chrono::duration<double>(t1 - t0).count();  // the steps and, with `u`, their probes
    ri.total_seconds = std::chrono::duration<double>(t_total1 - t_total0).count();
    ri.gstencils = points * done / ri.sweep_seconds / 1e9;
    ri.gstencils_refconv = ri.gstencils * F;
    ri.hbm_gbs = points * done * (source ? 4.0 : 3.0) * sizeof(double) / ri.sweep_seconds / 1e9;  // cur, prev (and f) read, prev written
    ri.variant = plan->p.variant;
    ri.steps_per_launch = lora::leapfrog_depth(plan->p);
    lora::set_last_run_info(ri);
    if (info) *info = ri;
    if (!quiet) {
        const double secs = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() / 1e6;
        std::printf("%s\n", lora::run_label(shape));
        std::printf("Time = %lld[ms]\n", (long long) std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count());
        std::printf("GStencil/s = %f\n", points * done * F / secs / 1e9);
        std::fflush(stdout);
    }
    return LORA_OK;
}

}  // extern "C"
