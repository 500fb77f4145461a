// chebyshev.cpp -- the Chebyshev semi-iteration on top of the scaled leapfrog step with a source (leapfrog.cpp:
// lora_plan_run_leapfrog_src):   u(k+1) = w(k+1) (S(u(k)) + f) + (1 - w(k+1)) u(k-1)
// solves u = S(u) + f in O(N) steps on an N-wide grid where Jacobi (lora_plan_run_until with a source) needs O(N^2).
// The coefficient schedule (host only), the run-until driver with the solvers' true-residual probe (reduce.cpp: true_residual;
// its grid here: lora_plan::cheb_probe, allocated only for the two-pass form), and the host-buffer operator (HostRun of
// hostrun.cpp; with its three grids and a warm-up that writes one of them it keeps its own uploads and download).
#include <hip/hip_runtime.h>

#include <cmath>
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
        // (not zeroed: the difference loads whole 16-byte pieces, but selects the halo cells of a piece away before any arithmetic
        // -- kernels_reduce.hip -- and every interior cell is read after the probe's sweep wrote it, on the same stream)
        if (!plan->cheb_probe.ensure(lora_plan_padded_bytes(plan))) return LORA_ENOMEM;
        if (plan->cheb_probe.ptr == d_prev || plan->cheb_probe.ptr == d_cur || plan->cheb_probe.ptr == d_f) return LORA_EINVAL;
    }
    (void) lora_plan_prepare_leapfrog(plan, u->check_every);

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
        if (int rc = lora::true_residual(plan, d_cur, d_f, plan->cheb_probe.ptr, fused, &r->last, s)) return rc;
        if (lora::until_decide(u, r)) break;
    }
    return LORA_OK;
}

int lora_run_host_chebyshev(int shape, const double *in, const double *source, double *out, const double *params, double rho, int times,
                            const lora_until *u, lora_until_result *r, const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || lora::bad_rho(rho)) return LORA_EINVAL;
    if (u ? (!r || lora::bad_until(u)) : times < 0) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a Chebyshev run (its source is an argument)")) return rc;
    lora::HostRun g;
    int rc = g.open(shape, LORA_F64, dims, params);
    if (rc != LORA_OK) return rc;
    lora_plan *plan = g.plan;
    const size_t bytes = g.bytes;
    if (g.alloc(source ? 3 : 2) != hipSuccess) return LORA_ENOMEM;
    void *d_prev = g.b[0], *d_cur = g.b[1], *d_f = g.b[2];
    if ((rc = lora::hip_status(hipMemcpy(d_cur, in, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    if (source)
        if ((rc = lora::hip_status(hipMemcpy(d_f, source, bytes, hipMemcpyHostToDevice), "upload"))) return rc;
    // set-up outside the timed region: the scratch grids, and one warm-up step (it writes d_prev, which is uploaded after it)
    const int cap = u ? u->max_times : times;
    if ((rc = lora_plan_prepare_leapfrog(plan, u ? u->check_every : times))) return rc;
    if ((rc = lora::hip_status(hipMemset(d_prev, 0, bytes), "warm-up"))) return rc;
    if (cap > 0)
        if ((rc = lora_plan_step_leapfrog_src(plan, d_cur, d_prev, d_f, 1.0, 0.0, nullptr))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "warm-up"))) return rc;
    if ((rc = lora::hip_status(hipMemcpy(d_prev, in, bytes, hipMemcpyHostToDevice), "upload"))) return rc;  // both levels start as `in`
    if ((rc = lora::hip_status(g.stream(), "stream"))) return rc;
    if ((rc = lora::hip_status(hipDeviceSynchronize(), "upload"))) return rc;

    int done = times;
    g.tic();
    if (u) {
        if ((rc = lora_plan_run_chebyshev_until(plan, d_prev, d_cur, d_f, rho, u, r, g.s))) return rc;
        done = r->times_done;
    } else {
        std::vector<double> a(times > 0 ? times : 1), c(a.size());
        if ((rc = lora_chebyshev_coeffs(rho, 1, times, a.data(), c.data()))) return rc;
        if ((rc = lora_plan_run_leapfrog_src(plan, d_prev, d_cur, d_f, a.data(), c.data(), (int) a.size(), times, g.s))) return rc;
        if (r) *r = {times, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}};
    }
    if ((rc = lora::hip_status(hipStreamSynchronize(g.s), "run"))) return rc;
    g.toc();  // the steps and, with `u`, their probes
    if ((rc = lora::hip_status(hipMemcpy(out, done % 2 ? d_prev : d_cur, bytes, hipMemcpyDeviceToHost), "download"))) return rc;
    return g.finish(done, source ? 4.0 : 3.0, lora::leapfrog_depth(plan->p), quiet, info);  // cur, prev (and f) read, prev written
}

}  // extern "C"
