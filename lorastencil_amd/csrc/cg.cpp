// cg.cpp -- conjugate gradients for u = S(u) + f on A = I - S (kernels: kernels_cg.hip, the dot reduction:
// kernels_reduce.hip / reduce.cpp).  The public entries of the three kernels, the run-until driver with a true-residual probe
// (its grids: lora_plan::cg, its device-resident scalars: lora_plan::cg_state), the spectrum of a run's Lanczos tridiagonal
// (host only), and the host-buffer operator (its skeleton: hostrun.cpp).
//
// Below them the implicit time stepper (kernels: kernels_theta.hip and the pointwise kernels of kernels_cg.hip):
// theta-scheme steps of du/dt = S(u) + f - u, each a CG solve on sigma I - tau' S started from the level itself, a whole run
// enqueued with no host wait.  Its entries go through the same CgLaunch as everything above, and so does the coarsest level of
// a multigrid cycle (cg_fixed_iterations; the driver: mg.cpp).
//
// At the end the preconditioned drivers: conjugate gradients with z = M r, M one V-cycle of mg.cpp, for u = S(u) + f
// and for the stepper's operator, the fused defect launch's public entry, and their host-buffer operators.
//
// One place per idea (the second anonymous namespace): reduced_entry is the tail of the four public entries that return a
// record; cg_rounds the round loop, stop rule, breakdown rule, history and spectrum of both CG drivers (the probe itself:
// true_residual of reduce.cpp); bad_theta_args and theta_read_back the argument check and the read-back of the steppers.  The
// four host-buffer operators are HostRun's open_solver / ready / timed (hostrun.cpp) round their own prepare, warm-up and call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <vector>

#include "engine.h"
#include "residual_tiles.h"

namespace lora {
namespace {

int no_cg_kernels(const Plan &p) {
    return unsupported(p.source ? "a plan with a source has no conjugate-gradient kernels: the source of a CG run is a call argument"
                                : "this plan has no conjugate-gradient kernels (bf16, the 2D matrix-pipe variant, or an odd innermost extent)");
}

// The launches of the three kernels over [begin, end) (a proper range) -- the ONE place both the public entries and the driver
// go through, so that both run the same kernels at the same geometry.  Records: the plan's.
struct CgLaunch {
    const Plan &p;
    ReduceRecord *records;
    hipStream_t s;
    ResidualTiles rt;
    ReduceArgs a;
    int kind = 0, groups = 0;
    long long count = 0;
    int pcg_cap = -1;  // >= 0: the preconditioned drivers' fold phases (alpha = rz / pq, no beta behind the update), with this history size
    CgLaunch(const Plan &plan, ReduceRecord *rec, hipStream_t stream) : p(plan), records(rec), s(stream) {}
    bool setup(int begin, int end) { return residual_tiles_setup(rt, p, begin, end) && interior_geometry(p, begin, end, a, kind, groups, count); }
    int apply_dot(const void *d_p, void *d_q, CgState *st, int cap) const {
        if (int rc = hip_status(launch_apply_dot(p, rt, static_cast<const double *>(d_p), static_cast<double *>(d_q), st, records, s), "apply_dot launch")) return rc;
        return hip_status(launch_cg_fold(records, rt.groups, st, st ? (pcg_cap >= 0 ? CG_FOLD_PCG_APPLY : CG_FOLD_APPLY) : CG_FOLD_PLAIN, cap, s),
                          "fold launch");
    }
    // sigma p - tau S(p) in place of p - S(p): the same tiles, the same fold
    int apply_dot_shift(const void *d_p, void *d_q, double sigma, double tau, CgState *st) const {
        if (int rc = hip_status(launch_apply_dot_shift(p, rt, static_cast<const double *>(d_p), static_cast<double *>(d_q), sigma, tau, st, records, s),
                                "apply_dot_shift launch"))
            return rc;
        if (st && pcg_cap >= 0) return hip_status(launch_cg_fold(records, rt.groups, st, CG_FOLD_PCG_APPLY, pcg_cap, s), "fold launch");
        return hip_status(launch_cg_fold(records, rt.groups, st, st ? CG_FOLD_APPLY : CG_FOLD_PLAIN, 0, s), "fold launch");
    }
    // r = p = tau (S(u) + f - u) and the fold of r.r; with a state, the step's start behind it
    int theta_start(const void *d_u, const void *d_f, double tau, void *d_r, void *d_p, CgState *st, ThetaState *ts) const {
        if (int rc = hip_status(launch_theta_start(p, rt, static_cast<const double *>(d_u), static_cast<const double *>(d_f), tau,
                                                   static_cast<double *>(d_r), static_cast<double *>(d_p), st, records, s),
                                "theta_start launch"))
            return rc;
        return hip_status(launch_cg_fold(records, rt.groups, st, st ? CG_FOLD_THETA_START : CG_FOLD_PLAIN, 0, s, ts), "fold launch");
    }
    int update(void *d_x, void *d_r, const void *d_p, const void *d_q, double alpha, CgState *st, int cap, ThetaState *ts = nullptr) const {
        if (int rc = hip_status(launch_cg_pointwise(CG_OP_UPDATE, a, kind, groups, static_cast<double *>(d_x), static_cast<double *>(d_r),
                                                    static_cast<const double *>(d_p), static_cast<const double *>(d_q), alpha, st, records, s),
                                "cg_update launch"))
            return rc;
        if (st && pcg_cap >= 0)
            return hip_status(launch_cg_fold(records, groups, st, ts ? CG_FOLD_PCG_THETA_UPDATE : CG_FOLD_PCG_UPDATE, pcg_cap, s, ts), "fold launch");
        return hip_status(launch_cg_fold(records, groups, st, st ? (ts ? CG_FOLD_THETA_UPDATE : CG_FOLD_UPDATE) : CG_FOLD_PLAIN, cap, s, ts), "fold launch");
    }
    // rz = r.z: lora_plan_dot's launches, and behind them the state's (first: CG_FOLD_PCG_RZ0, else beta = rz' / rz)
    int dot_rz(const void *d_r, const void *d_z, CgState *st, bool first) const {
        if (int rc = hip_status(launch_reduce_dot(a, kind, groups, d_r, d_z, records, s), "reduction kernel launch")) return rc;
        return hip_status(launch_cg_fold(records, groups, st, first ? CG_FOLD_PCG_RZ0 : CG_FOLD_PCG_RZ, pcg_cap, s), "fold launch");
    }
    int direction(void *d_p, const void *d_r, double beta, const CgState *st) const {
        return hip_status(launch_cg_pointwise(CG_OP_DIRECTION, a, kind, groups, static_cast<double *>(d_p), nullptr, static_cast<const double *>(d_r),
                                              nullptr, beta, st, records, s),
                          "cg_direction launch");
    }
    int start(void *d_r, void *d_p, const void *d_x) const {  // r = r - x, p = r
        return hip_status(launch_cg_pointwise(CG_OP_START, a, kind, groups, static_cast<double *>(d_r), static_cast<double *>(d_p),
                                              static_cast<const double *>(d_x), nullptr, 0.0, nullptr, records, s),
                          "cg_start launch");
    }
    int result(lora_grid_dot *out) const {  // blocks
        ReduceRecord rec;
        if (int rc = folded_record(records, rec, s)) return rc;
        *out = {rec.f[0], rec.f[1], count, rec.i[0]};
        return LORA_OK;
    }
};

size_t state_bytes(int cap) { return sizeof(CgState) + 2 * sizeof(double) * (size_t) cap + sizeof(PcgState); }  // (engine.h: PcgState)

// the three grids and the state with room for `max_times` coefficients (an earlier, larger history is kept)
int ensure_cg(lora_plan *plan, int max_times) {
    const size_t bytes = lora_plan_padded_bytes(plan);
    for (DeviceGrid &g : plan->cg)
        if (!g.ensure(bytes)) return LORA_ENOMEM;
    const int cap = max_times > 1 ? max_times : 1;
    if (plan->cg_cap >= cap && plan->cg_state.ready(state_bytes(plan->cg_cap))) return LORA_OK;
    if (!plan->cg_state.ensure(state_bytes(cap))) return LORA_ENOMEM;
    plan->cg_cap = cap;
    return LORA_OK;
}

size_t theta_bytes(int cap) { return sizeof(ThetaState) + (sizeof(long long) + sizeof(double)) * (size_t) cap; }

// the stepper's grids and states: the CG set, and the ThetaState with room for `steps` entries (an earlier, larger one is kept)
int ensure_theta(lora_plan *plan, int steps) {
    if (int rc = ensure_cg(plan, 1)) return rc;
    const int cap = steps > 1 ? steps : 1;
    if (plan->theta_cap >= cap && plan->theta_state.ready(theta_bytes(plan->theta_cap))) return LORA_OK;
    if (!plan->theta_state.ensure(theta_bytes(cap))) return LORA_ENOMEM;
    plan->theta_cap = cap;
    return LORA_OK;
}

// eigenvalues of the tridiagonal (d, e2 = squared off-diagonals) below x: the Sturm count
int sturm_count(const std::vector<double> &d, const std::vector<double> &e2, double x, double tiny) {
    int below = 0;
    double q = 1.0;
    for (size_t k = 0; k < d.size(); ++k) {
        q = d[k] - x - (k ? e2[k - 1] / q : 0.0);
        if (q == 0.0) q = -tiny;
        below += q < 0.0;
    }
    return below;
}

// the smallest x in [lo, hi] with at least `want` eigenvalues below it, to the last bit the midpoint still moves
double bisect(const std::vector<double> &d, const std::vector<double> &e2, double lo, double hi, int want, double tiny) {
    for (;;) {
        const double mid = lo + (hi - lo) / 2;
        if (!(mid > lo && mid < hi)) return mid;
        if (sturm_count(d, e2, mid, tiny) >= want)
            hi = mid;
        else
            lo = mid;
    }
}

const double kNaN = std::numeric_limits<double>::quiet_NaN();

}  // namespace

int ensure_cg_grids(lora_plan *plan) { return ensure_cg(plan, 1); }

// The coarsest level of a multigrid cycle (mg.cpp): the iterations of lora_plan_run_cg_until below, through the same CgLaunch,
// from a residual the caller has put into the plan's own r -- no source sweep, no probe, no host wait.
int cg_fixed_iterations(lora_plan *plan, void *d_x, int iters, double sigma, double tau, hipStream_t s, long *launches) {
    const Plan &p = plan->p;
    if (int rc = ensure_cg(plan, 1)) return rc;
    void *d_r = plan->cg[0].ptr, *d_p = plan->cg[1].ptr, *d_q = plan->cg[2].ptr;
    CgState *st = static_cast<CgState *>(plan->cg_state.ptr);
    const int cap = plan->cg_cap;
    ReduceRecord *records = nullptr;
    if (int rc = reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(0, p.dims[0])) return LORA_EINVAL;
    // p = r on the interior, with a zero halo; rr = r.r
    const int *pad = interior_pads(p.ndim);
    if (int rc = hip_status(launch_halo(p, d_p, nullptr, HALO_ZERO, s), "halo launch")) return rc;
    if (int rc = hip_status(launch_copy_interior(p.dtype, p.ndim, p.dims, d_p, pad, d_r, pad, s), "copy launch")) return rc;
    if (int rc = hip_status(launch_reduce_dot(L.a, L.kind, L.groups, d_r, d_r, records, s), "reduction kernel launch")) return rc;
    if (int rc = hip_status(launch_cg_fold(records, L.groups, st, CG_FOLD_START, cap, s), "fold launch")) return rc;
    const bool shifted = !(sigma == 1.0 && tau == 1.0);  // (1, 1) keeps the plain kernel: the same bits on any data
    for (int i = 0; i < iters; ++i) {
        if (int rc = shifted ? L.apply_dot_shift(d_p, d_q, sigma, tau, st) : L.apply_dot(d_p, d_q, st, cap)) return rc;
        if (int rc = L.update(d_x, d_r, d_p, d_q, 0.0, st, cap)) return rc;
        if (int rc = L.direction(d_p, d_r, 0.0, st)) return rc;
    }
    if (launches) *launches += 5 + 5L * iters;  // (the dot is a reduction and its fold)
    return LORA_OK;
}

int defect_whole(const Plan &p, const double *d_u, const double *d_f, double *d_out, hipStream_t s) {
    if (!has_cg(p)) return no_cg_kernels(p);
    ResidualTiles rt;
    if (!residual_tiles_setup(rt, p, 0, p.dims[0])) return LORA_EINVAL;
    return hip_status(launch_defect(p, rt, d_u, d_f, d_out, s), "defect launch");
}

// ---- what the entries below share: the preconditioned drivers' pieces, the reduced public entries' tail, the
// round loop of the two CG drivers, the steppers' argument check and read-back ------------------------------------------------
namespace {

// the drivers need a symmetric preconditioner: as many smoothing applications behind the coarse correction as before it
bool asymmetric(const lora_mg *m) { return m->pre != m->post || m->pre < 1; }

// whether a caller's buffer is one of the plan's own
bool owned(const lora_plan *plan, const void *buf) {
    if (!buf) return false;
    for (const void *own : {plan->cg[0].ptr, plan->cg[1].ptr, plan->cg[2].ptr, plan->cg_state.ptr, plan->theta_state.ptr, plan->pcg_z.ptr})
        if (own == buf) return true;
    return mg_owns(plan, buf);
}

// z = M r, p = z on the interior (the halo of p is the run's zero halo), rz = r.z
int pcg_first_direction(lora_plan *plan, const CgLaunch &L, const lora_mg *m, double sigma, double tau, CgState *st) {
    const Plan &p = plan->p;
    double *d_r = static_cast<double *>(plan->cg[0].ptr), *d_p = static_cast<double *>(plan->cg[1].ptr);
    double *d_z = static_cast<double *>(plan->pcg_z.ptr);
    if (int rc = mg_precondition(plan, d_r, d_z, m, sigma, tau, L.s)) return rc;
    const int *pad = interior_pads(p.ndim);
    if (int rc = hip_status(launch_copy_interior(p.dtype, p.ndim, p.dims, d_p, pad, d_z, pad, L.s), "copy launch")) return rc;
    return L.dot_rz(d_r, d_z, st, true);
}

// behind an iteration's update: z = M r, rz' = r.z, beta = rz' / rz, p = z + beta p
int pcg_next_direction(lora_plan *plan, const CgLaunch &L, const lora_mg *m, double sigma, double tau, CgState *st) {
    double *d_r = static_cast<double *>(plan->cg[0].ptr), *d_p = static_cast<double *>(plan->cg[1].ptr);
    double *d_z = static_cast<double *>(plan->pcg_z.ptr);
    if (int rc = mg_precondition(plan, d_r, d_z, m, sigma, tau, L.s)) return rc;
    if (int rc = L.dot_rz(d_r, d_z, st, false)) return rc;
    return L.direction(d_p, d_z, 0.0, st);
}

// The tail of lora_plan_apply_dot, _cg_update, _apply_dot_shift and _theta_start, behind their own argument checks: the plan's
// kernels, the reduction's admission of (d_a, d_b), the empty record, the launches of `call` (one member of CgLaunch) over
// [begin, end) and the folded record (blocks).  some: reduction_range's answer.
template <class Call>
int reduced_entry(lora_plan *plan, const void *d_a, const void *d_b, int some, int begin, int end, lora_grid_dot *out, void *stream, Call call) {
    const Plan &p = plan->p;
    if (!has_cg(p)) return no_cg_kernels(p);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = admit_reduction(d_a, d_b, s)) return rc;
    *out = {0.0, 0.0, 0, 0};
    if (!some) return LORA_OK;
    ReduceRecord *records = nullptr;
    if (int rc = reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(begin, end)) return LORA_EINVAL;
    if (int rc = call(L)) return rc;
    return L.result(out);
}

// The rounds of lora_plan_run_cg_until and, with `m` (whose V-cycle then gives every next direction), lora_plan_run_pcg_until,
// behind the entry's start-up, into r->until, r->breakdown, r->lambda_min and r->lambda_max.  A round: check_every iterations
// through L, the state back in the probe's wait, the true residual (fused under the max norm, where every deciding field is bit
// for bit the two-pass probe's; else two passes through the plan's q), the stop rule; a breakdown ends the run, as diverged
// unless that check converged.  Then the run's coefficients, the extreme Ritz values of their Lanczos tridiagonal and, where
// lora_cg_spectrum took them, *rho_estimate (the CG result's: nullptr = none, the Ritz values of M A bound no radius of S).
// Nothing is allocated before the history: on small grids the enqueue is the critical path.
template <class Result>
int cg_rounds(lora_plan *plan, const CgLaunch &L, const lora_mg *m, void *d_x, const void *d_f, const lora_until *u, Result *r, double *rho_estimate) {
    void *d_r = plan->cg[0].ptr, *d_p = plan->cg[1].ptr, *d_q = plan->cg[2].ptr;
    CgState *st = static_cast<CgState *>(plan->cg_state.ptr);
    const int cap = plan->cg_cap;
    const bool fused = u->norm == LORA_NORM_MAX;
    CgState now = {};
    lora_until_result &ur = r->until;
    while (ur.times_done + u->check_every <= u->max_times) {
        for (int i = 0; i < u->check_every; ++i) {
            if (int rc = L.apply_dot(d_p, d_q, st, cap)) return rc;
            if (int rc = L.update(d_x, d_r, d_p, d_q, 0.0, st, cap)) return rc;
            if (int rc = m ? pcg_next_direction(plan, L, m, 1.0, 1.0, st) : L.direction(d_p, d_r, 0.0, st)) return rc;
        }
        // the scalars come back in the probe's wait
        if (int rc = hip_status(hipMemcpyAsync(&now, st, sizeof now, hipMemcpyDeviceToHost, L.s), "state download")) return rc;
        if (int rc = true_residual(plan, d_x, d_f, d_q, fused, &ur.last, L.s)) return rc;
        ur.times_done = (int) now.iteration;
        bool stop = until_decide(u, &ur);
        if (now.breakdown) {
            r->breakdown = 1;
            if (!ur.converged) ur.diverged = 1;
            stop = true;
        }
        if (stop) break;
    }
    const int n = ur.times_done;
    if (n > 0) {
        // n alphas and the n - 1 betas between them: lora_cg_spectrum reads no more, so the last beta stays on the device
        std::vector<double> hist(2 * (size_t) n);
        const double *d_hist = reinterpret_cast<const double *>(st + 1);
        if (int rc = hip_status(hipMemcpyAsync(hist.data(), d_hist, sizeof(double) * n, hipMemcpyDeviceToHost, L.s), "history download")) return rc;
        if (n > 1)
            if (int rc = hip_status(hipMemcpyAsync(hist.data() + n, d_hist + cap, sizeof(double) * (n - 1), hipMemcpyDeviceToHost, L.s), "history download"))
                return rc;
        if (int rc = hip_status(hipStreamSynchronize(L.s), "history download")) return rc;
        if (lora_cg_spectrum(hist.data(), hist.data() + n, n, &r->lambda_min, &r->lambda_max) == LORA_OK && rho_estimate)
            *rho_estimate = std::fmax(std::fabs(1.0 - r->lambda_min), std::fabs(1.0 - r->lambda_max));
    }
    return LORA_OK;
}

// what all four stepper entries refuse alike (a NaN fails every comparison)
bool bad_theta_args(double theta, double tau, int steps, int max_iters, double rtol) {
    return !(theta >= 0.0 && theta <= 1.0) || !(tau > 0.0) || !std::isfinite(tau) || steps < 0 || max_iters < 1 || !(rtol >= 0.0) || !std::isfinite(rtol);
}

// The end of lora_plan_run_theta and lora_plan_run_theta_mg, behind their enqueue loops: the two states and the per-step history
// come back behind the steady-state probe's synchronise, then *r and iterations[] (nullptr = not asked for).
int theta_read_back(lora_plan *plan, const void *d_u, const void *d_f, int steps, int *iterations, lora_theta_result *r, hipStream_t s) {
    const CgState *st = static_cast<const CgState *>(plan->cg_state.ptr);
    const ThetaState *ts = static_cast<const ThetaState *>(plan->theta_state.ptr);
    CgState now = {};
    ThetaState tnow = {};
    std::vector<long long> hist((size_t) steps);
    if (int rc = hip_status(hipMemcpyAsync(&now, st, sizeof now, hipMemcpyDeviceToHost, s), "state download")) return rc;
    if (int rc = hip_status(hipMemcpyAsync(&tnow, ts, sizeof tnow, hipMemcpyDeviceToHost, s), "state download")) return rc;
    if (int rc = hip_status(hipMemcpyAsync(hist.data(), ts + 1, sizeof(long long) * steps, hipMemcpyDeviceToHost, s), "history download")) return rc;
    if (int rc = residual_whole(plan, d_u, d_f, &r->steady, s)) return rc;
    r->steps_done = (int) tnow.steps_done;
    r->breakdown = (now.breakdown & CG_HALT_BREAKDOWN) ? 1 : 0;
    r->unconverged_steps = (int) tnow.unconverged;
    r->last_rr0 = tnow.rr0;
    r->last_rr = now.rr;
    for (int step = 0; step < steps; ++step) {
        // a step the breakdown interrupted reports the iterations applied before it; the steps behind it never ran
        const int k = step < r->steps_done ? (int) hist[step] : (step == r->steps_done ? (int) now.iteration : 0);
        if (iterations) iterations[step] = k;
        if (step < r->steps_done) {
            r->iterations_total += k;
            if (k > r->iterations_max) r->iterations_max = k;
        }
    }
    return LORA_OK;
}

}  // namespace
}  // namespace lora

using lora::CgLaunch;
using lora::Plan;

extern "C" {

int lora_plan_apply_dot(lora_plan *plan, const void *d_p, void *d_q, int begin, int end, lora_grid_dot *out, void *stream) {
    if (!plan || !d_p || !d_q || !out) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p) || d_p == d_q) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_p, d_q)) return rc;
    return lora::reduced_entry(plan, d_p, d_q, some, begin, end, out, stream, [&](const CgLaunch &L) { return L.apply_dot(d_p, d_q, nullptr, 0); });
}

int lora_plan_cg_update(lora_plan *plan, void *d_x, void *d_r, const void *d_p, const void *d_q, double alpha, int begin, int end,
                        lora_grid_dot *out_rr, void *stream) {
    if (!plan || !d_x || !d_r || !d_p || !d_q || !out_rr) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p)) return LORA_EINVAL;
    if (d_x == d_r || d_x == d_p || d_x == d_q || d_r == d_p || d_r == d_q || d_p == d_q) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_x, d_r)) return rc;
    if (int rc = lora::check_buffers(d_p, d_q)) return rc;
    return lora::reduced_entry(plan, d_x, d_r, some, begin, end, out_rr, stream,
                               [&](const CgLaunch &L) { return L.update(d_x, d_r, d_p, d_q, alpha, nullptr, 0); });
}

int lora_plan_cg_direction(lora_plan *plan, void *d_p, const void *d_r, double beta, int begin, int end, void *stream) {
    if (!plan || !d_p || !d_r) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p) || d_p == d_r) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_p, d_r)) return rc;
    if (!lora::has_cg(p)) return lora::no_cg_kernels(p);
    if (lora_device_count() <= 0) return lora::no_device();
    if (!some) return LORA_OK;
    CgLaunch L(p, nullptr, static_cast<hipStream_t>(stream));
    if (!L.setup(begin, end)) return LORA_EINVAL;
    return L.direction(d_p, d_r, beta, nullptr);
}

int lora_plan_prepare_cg(lora_plan *plan, int max_times) {
    if (!plan || max_times < 0) return LORA_EINVAL;
    if (!lora::has_cg(plan->p)) return lora::no_cg_kernels(plan->p);
    if (lora_device_count() <= 0) return lora::no_device();
    return lora::ensure_cg(plan, max_times);
}

int lora_plan_run_cg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_until *u, lora_cg_result *r, void *stream) {
    if (!plan || !d_x || !u || !r || lora::bad_until(u) || d_f == d_x) return LORA_EINVAL;
    if (lora::misaligned(d_x) || lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    const Plan &p = plan->p;
    if (!lora::has_cg(p)) return lora::no_cg_kernels(p);
    if (!lora::taps_symmetric(p.w, p.ntaps))
        return lora::unsupported("conjugate gradients need point-symmetric taps, w[t] == w[ntaps - 1 - t]: I - S is not symmetric otherwise");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_x, d_x, s)) return rc;
    *r = {{0, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}}, lora::kNaN, lora::kNaN, lora::kNaN, 0};
    if (u->max_times < u->check_every) return LORA_OK;
    if (int rc = lora::ensure_cg(plan, u->max_times)) return rc;
    void *d_r = plan->cg[0].ptr, *d_p = plan->cg[1].ptr, *d_q = plan->cg[2].ptr;
    for (const void *own : {d_r, d_p, d_q, plan->cg_state.ptr})
        if (own == d_x || own == d_f) return LORA_EINVAL;
    lora::CgState *st = static_cast<lora::CgState *>(plan->cg_state.ptr);
    const int cap = plan->cg_cap;
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(0, p.dims[0])) return LORA_EINVAL;

    // r = fl(fl(S(x) + f) - x), p = r with a zero halo, rr = r.r -- nothing read before this run wrote it, on this stream
    if (int rc = lora::sweep_with_source(p, d_f, d_x, d_r, s)) return rc;
    if (int rc = lora::hip_status(lora::launch_halo(p, d_p, nullptr, lora::HALO_ZERO, s), "halo launch")) return rc;
    if (int rc = L.start(d_r, d_p, d_x)) return rc;
    if (int rc = lora::hip_status(lora::launch_reduce_dot(L.a, L.kind, L.groups, d_r, d_r, records, s), "reduction kernel launch")) return rc;
    if (int rc = lora::hip_status(lora::launch_cg_fold(records, L.groups, st, lora::CG_FOLD_START, cap, s), "fold launch")) return rc;

    return lora::cg_rounds(plan, L, nullptr, d_x, d_f, u, r, &r->rho_estimate);
}

int lora_cg_spectrum(const double *alpha, const double *beta, int n, double *lambda_min, double *lambda_max) {
    if (n < 1 || !alpha || !lambda_min || !lambda_max || (n > 1 && !beta)) return LORA_EINVAL;
    for (int k = 0; k < n; ++k)
        if (!(alpha[k] > 0.0) || !std::isfinite(alpha[k])) return LORA_EINVAL;
    for (int k = 0; k + 1 < n; ++k)
        if (!(beta[k] >= 0.0) || !std::isfinite(beta[k])) return LORA_EINVAL;
    std::vector<double> d(n), e2(n > 1 ? n - 1 : 0);
    for (int k = 0; k < n; ++k) {
        d[k] = 1.0 / alpha[k] + (k ? beta[k - 1] / alpha[k - 1] : 0.0);
        if (k + 1 < n) {
            const double e = std::sqrt(beta[k]) / alpha[k];
            e2[k] = e * e;
        }
    }
    // Gershgorin: every eigenvalue lies in [lo, hi]
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int k = 0; k < n; ++k) {
        const double rad = (k ? std::sqrt(e2[k - 1]) : 0.0) + (k + 1 < n ? std::sqrt(e2[k]) : 0.0);
        lo = std::fmin(lo, d[k] - rad);
        hi = std::fmax(hi, d[k] + rad);
    }
    if (!std::isfinite(lo) || !std::isfinite(hi)) return LORA_EINVAL;  // (a coefficient so small that 1 / alpha overflowed)
    const double scale = std::fmax(std::fabs(lo), std::fabs(hi));
    const double tiny = scale * std::numeric_limits<double>::epsilon() * std::numeric_limits<double>::epsilon();
    const double pad = scale * 4 * std::numeric_limits<double>::epsilon();
    *lambda_min = lora::bisect(d, e2, lo - pad, hi + pad, 1, tiny);
    *lambda_max = lora::bisect(d, e2, lo - pad, hi + pad, n, tiny);
    return LORA_OK;
}

int lora_run_host_cg(int shape, const double *in, const double *source, double *out, const double *params, const lora_until *u,
                     lora_cg_result *r, const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || !u || !r || lora::bad_until(u)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a conjugate-gradient run (its source is an argument)")) return rc;
    lora::HostRun g;
    if (int rc = g.open_solver(shape, dims, params, in, source)) return rc;
    lora_plan *plan = g.plan;
    void *d_x = g.b[0], *d_f = g.b[1];
    // set-up outside the timed region: the plan's grids and state, and one warm-up application into the plan's own q
    if (int rc = lora_plan_prepare_cg(plan, u->max_times)) return rc;
    lora_grid_dot warm;
    if (int rc = lora_plan_apply_dot(plan, d_x, plan->cg[2].ptr, 0, 0, &warm, nullptr)) return rc;
    if (int rc = g.ready()) return rc;
    // timed: the start-up, the iterations and their probes
    if (int rc = g.timed(out, [&] { return lora_plan_run_cg_until(plan, d_x, d_f, u, r, g.s); })) return rc;
    // per iteration: p read, q written; x, r, p, q read, x, r written; r, p read, p written
    return g.finish(r->until.times_done, 11.0, 1, quiet, info);
}

// ---- the implicit stepper ------------------------------------------------------------------------------------------------------
int lora_plan_apply_dot_shift(lora_plan *plan, const void *d_p, void *d_q, double sigma, double tau, int begin, int end, lora_grid_dot *out,
                              void *stream) {
    if (!plan || !d_p || !d_q || !out) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p) || d_p == d_q || !std::isfinite(sigma) || !std::isfinite(tau)) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_p, d_q)) return rc;
    return lora::reduced_entry(plan, d_p, d_q, some, begin, end, out, stream,
                               [&](const CgLaunch &L) { return L.apply_dot_shift(d_p, d_q, sigma, tau, nullptr); });
}

int lora_plan_theta_start(lora_plan *plan, const void *d_u, const void *d_f, double tau, void *d_r, void *d_p, int begin, int end,
                          lora_grid_dot *out_rr, void *stream) {
    if (!plan || !d_u || !d_r || !d_p || !out_rr) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p) || !std::isfinite(tau)) return LORA_EINVAL;
    if (d_u == d_r || d_u == d_p || d_r == d_p || d_f == d_u || d_f == d_r || d_f == d_p) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_u, d_r)) return rc;
    if (int rc = lora::check_buffers(d_p, d_f ? d_f : d_p)) return rc;
    return lora::reduced_entry(plan, d_u, d_r, some, begin, end, out_rr, stream,
                               [&](const CgLaunch &L) { return L.theta_start(d_u, d_f, tau, d_r, d_p, nullptr, nullptr); });
}

int lora_plan_defect(lora_plan *plan, const void *d_u, const void *d_f, void *d_out, int begin, int end, void *stream) {
    if (!plan || !d_u || !d_out) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::reduction_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p)) return LORA_EINVAL;
    if (d_u == d_out || d_f == d_u || d_f == d_out) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_u, d_out)) return rc;
    if (lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (!lora::has_cg(p)) return lora::no_cg_kernels(p);
    if (lora_device_count() <= 0) return lora::no_device();
    if (!some) return LORA_OK;
    lora::ResidualTiles rt;
    if (!lora::residual_tiles_setup(rt, p, begin, end)) return LORA_EINVAL;
    return lora::hip_status(lora::launch_defect(p, rt, static_cast<const double *>(d_u), static_cast<const double *>(d_f),
                                                static_cast<double *>(d_out), static_cast<hipStream_t>(stream)),
                            "defect launch");
}

// ---- the whole small CG in one launch (kernels_cg_small.hip) ------------------------------------------------------
int lora_plan_cg_small(lora_plan *plan, void *d_x, void *d_r, int iters, double sigma, double tau, double *d_info, void *stream) {
    if (!plan || !d_x || !d_r || d_x == d_r || iters < 0 || !std::isfinite(sigma) || !std::isfinite(tau)) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_x, d_r)) return rc;
    const Plan &p = plan->p;
    if (!lora::has_cg_small(p))
        return lora::unsupported("this plan has no one-launch conjugate-gradient kernel (option \"cg_small\"): it takes the 2D and 3D plans "
                                 "with the conjugate-gradient kernels whose interior fits one workgroup");
    if (iters == 0) return LORA_OK;  // nothing to launch: needs no device
    if (lora_device_count() <= 0) return lora::no_device();
    return lora::hip_status(lora::launch_cg_small(p, static_cast<double *>(d_x), static_cast<double *>(d_r), iters, sigma, tau, d_info,
                                                  static_cast<hipStream_t>(stream)),
                            "cg_small launch");
}

int lora_plan_prepare_theta(lora_plan *plan, int steps) {
    if (!plan || steps < 0) return LORA_EINVAL;
    if (!lora::has_cg(plan->p)) return lora::no_cg_kernels(plan->p);
    if (lora_device_count() <= 0) return lora::no_device();
    lora::ReduceRecord *records = nullptr;  // (the run folds into the plan's records: they are part of what it needs)
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    return lora::ensure_theta(plan, steps);
}

int lora_plan_run_theta(lora_plan *plan, void *d_u, const void *d_f, double theta, double tau, int steps, int max_iters, double rtol,
                        int *iterations, lora_theta_result *r, void *stream) {
    if (!plan || !d_u || !r || d_f == d_u || lora::bad_theta_args(theta, tau, steps, max_iters, rtol)) return LORA_EINVAL;
    if (lora::misaligned(d_u) || lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    const Plan &p = plan->p;
    if (!lora::has_cg(p)) return lora::no_cg_kernels(p);
    if (!lora::taps_symmetric(p.w, p.ntaps))
        return lora::unsupported("the implicit stepper needs point-symmetric taps, w[t] == w[ntaps - 1 - t]: sigma I - tau S is not symmetric otherwise");
    *r = {0, 0, 0, 0, 0, lora::kNaN, lora::kNaN, {0.0, 0.0, 0.0, -1, 0, 0}};
    if (steps == 0) return LORA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_u, d_u, s)) return rc;
    if (int rc = lora::ensure_theta(plan, steps)) return rc;
    void *d_r = plan->cg[0].ptr, *d_p = plan->cg[1].ptr, *d_q = plan->cg[2].ptr;
    for (const void *own : {d_r, d_p, d_q, plan->cg_state.ptr, plan->theta_state.ptr})
        if (own == d_u || own == d_f) return LORA_EINVAL;
    lora::CgState *st = static_cast<lora::CgState *>(plan->cg_state.ptr);
    lora::ThetaState *ts = static_cast<lora::ThetaState *>(plan->theta_state.ptr);
    const int cap = plan->theta_cap;
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(0, p.dims[0])) return LORA_EINVAL;

    // the operator of the step and the stop rule's factor, each operation its own rounding
    const double tt = theta * tau, sigma = 1.0 + tt, rtol2 = rtol * rtol;
    // the whole run is enqueued here: nothing below waits for the device before the read-back
    if (int rc = lora::hip_status(lora::launch_cg_fold(records, 0, st, lora::CG_FOLD_THETA_INIT, cap, s, ts, rtol2, max_iters), "fold launch")) return rc;
    if (int rc = lora::hip_status(lora::launch_halo(p, d_p, nullptr, lora::HALO_ZERO, s), "halo launch")) return rc;
    for (int step = 0; step < steps; ++step) {
        if (int rc = L.theta_start(d_u, d_f, tau, d_r, d_p, st, ts)) return rc;
        for (int i = 0; i < max_iters; ++i) {
            if (int rc = L.apply_dot_shift(d_p, d_q, sigma, tt, st)) return rc;
            if (int rc = L.update(d_u, d_r, d_p, d_q, 0.0, st, 0, ts)) return rc;
            if (int rc = L.direction(d_p, d_r, 0.0, st)) return rc;
        }
    }
    return lora::theta_read_back(plan, d_u, d_f, steps, iterations, r, s);  // the one wait
}

int lora_run_host_theta(int shape, const double *in, const double *source, double *out, const double *params, double theta, double tau,
                        int steps, int max_iters, double rtol, const int *dims, int quiet, lora_run_info *info, lora_theta_result *result) {
    if (!in || !out || !dims || !result || lora::bad_theta_args(theta, tau, steps, max_iters, rtol)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("an implicit run (its source is an argument)")) return rc;
    lora::HostRun g;
    if (int rc = g.open_solver(shape, dims, params, in, source)) return rc;
    lora_plan *plan = g.plan;
    void *d_u = g.b[0], *d_f = g.b[1];
    // set-up outside the timed region: the plan's grids and states, and one warm-up application into the plan's own q
    if (int rc = lora_plan_prepare_theta(plan, steps)) return rc;
    lora_grid_dot warm;
    if (int rc = lora_plan_apply_dot_shift(plan, d_u, plan->cg[2].ptr, 1.0, 1.0, 0, 0, &warm, nullptr)) return rc;
    if (int rc = g.ready()) return rc;
    // timed: every step's start and iterations, and the steady-state probe
    if (int rc = g.timed(out, [&] { return lora_plan_run_theta(plan, d_u, d_f, theta, tau, steps, max_iters, rtol, nullptr, result, g.s); })) return rc;
    // per step: u (and f) read, r and p written; per iteration the eleven grids of a CG iteration (lora_run_host_cg)
    const double per_step = (source ? 4.0 : 3.0) + (steps > 0 ? 11.0 * (double) result->iterations_total / steps : 0.0);
    return g.finish(steps, per_step, 1, quiet, info);
}

// ---- multigrid-preconditioned conjugate gradients and the implicit stepper on them ------------------------------
int lora_plan_prepare_pcg(lora_plan *plan, const lora_mg *m, int max_times) {
    if (!plan || !m || max_times < 0 || lora::mg_bad(m, 1.0, 1.0) || lora::asymmetric(m)) return LORA_EINVAL;
    if (int rc = lora::mg_admit(plan, m, 1.0, 1.0, nullptr)) return rc;
    if (lora_device_count() <= 0) return lora::no_device();
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    if (int rc = lora::ensure_cg(plan, max_times)) return rc;
    if (!plan->pcg_z.ensure(lora_plan_padded_bytes(plan))) return LORA_ENOMEM;
    return lora::mg_prepare(plan, m, 1.0, 1.0);
}

int lora_plan_run_pcg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_mg *m, const lora_until *u, lora_pcg_result *r,
                            void *stream) {
    if (!plan || !d_x || !m || !u || !r || lora::bad_until(u) || lora::mg_bad(m, 1.0, 1.0) || lora::asymmetric(m) || d_f == d_x) return LORA_EINVAL;
    if (lora::misaligned(d_x) || lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    int levels = 0;
    if (int rc = lora::mg_admit(plan, m, 1.0, 1.0, &levels)) return rc;
    const Plan &p = plan->p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_x, d_x, s)) return rc;
    *r = {{0, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}}, lora::kNaN, lora::kNaN, 0, levels};
    if (u->max_times < u->check_every) return LORA_OK;
    if (int rc = lora::ensure_cg(plan, u->max_times)) return rc;
    if (!plan->pcg_z.ensure(lora_plan_padded_bytes(plan))) return LORA_ENOMEM;
    if (int rc = lora::mg_prepare(plan, m, 1.0, 1.0)) return rc;
    if (lora::owned(plan, d_x) || lora::owned(plan, d_f)) return LORA_EINVAL;
    double *d_r = static_cast<double *>(plan->cg[0].ptr), *d_p = static_cast<double *>(plan->cg[1].ptr);
    lora::CgState *st = static_cast<lora::CgState *>(plan->cg_state.ptr);
    const int cap = plan->cg_cap;
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(0, p.dims[0])) return LORA_EINVAL;
    L.pcg_cap = cap;

    // r = fl(fl(S(x) + f) - x) in one launch, z = M r, p = z with a zero halo, rz = r.z -- all on this stream
    if (int rc = lora::hip_status(lora::launch_cg_fold(records, 0, st, lora::CG_FOLD_PCG_INIT, cap, s), "fold launch")) return rc;
    if (int rc = lora::defect_whole(p, static_cast<const double *>(d_x), static_cast<const double *>(d_f), d_r, s)) return rc;
    if (int rc = lora::hip_status(lora::launch_halo(p, d_p, nullptr, lora::HALO_ZERO, s), "halo launch")) return rc;
    if (int rc = lora::pcg_first_direction(plan, L, m, 1.0, 1.0, st)) return rc;

    return lora::cg_rounds(plan, L, m, d_x, d_f, u, r, nullptr);
}

int lora_plan_run_theta_mg(lora_plan *plan, void *d_u, const void *d_f, double theta, double tau, int steps, int max_iters, double rtol,
                           const lora_mg *m, int check_every, int *iterations, lora_theta_result *r, void *stream) {
    if (!plan || !d_u || !r || !m || d_f == d_u) return LORA_EINVAL;
    if (lora::bad_theta_args(theta, tau, steps, max_iters, rtol) || check_every < 1) return LORA_EINVAL;
    // the operator of the step and the stop rule's factor, each operation its own rounding
    const double tt = theta * tau, sigma = 1.0 + tt, rtol2 = rtol * rtol;
    if (lora::mg_bad(m, sigma, tt) || lora::asymmetric(m)) return LORA_EINVAL;
    if (lora::misaligned(d_u) || lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::mg_admit(plan, m, sigma, tt, nullptr)) return rc;
    const Plan &p = plan->p;
    *r = {0, 0, 0, 0, 0, lora::kNaN, lora::kNaN, {0.0, 0.0, 0.0, -1, 0, 0}};
    if (steps == 0) return LORA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_u, d_u, s)) return rc;
    if (int rc = lora::ensure_theta(plan, steps)) return rc;
    if (!plan->pcg_z.ensure(lora_plan_padded_bytes(plan))) return LORA_ENOMEM;
    if (int rc = lora::mg_prepare(plan, m, sigma, tt)) return rc;
    if (lora::owned(plan, d_u) || lora::owned(plan, d_f)) return LORA_EINVAL;
    double *d_r = static_cast<double *>(plan->cg[0].ptr), *d_p = static_cast<double *>(plan->cg[1].ptr), *d_q = static_cast<double *>(plan->cg[2].ptr);
    double *d_z = static_cast<double *>(plan->pcg_z.ptr);
    lora::CgState *st = static_cast<lora::CgState *>(plan->cg_state.ptr);
    lora::ThetaState *ts = static_cast<lora::ThetaState *>(plan->theta_state.ptr);
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    CgLaunch L(p, records, s);
    if (!L.setup(0, p.dims[0])) return LORA_EINVAL;
    L.pcg_cap = plan->cg_cap;

    if (int rc = lora::hip_status(lora::launch_cg_fold(records, 0, st, lora::CG_FOLD_THETA_INIT, plan->theta_cap, s, ts, rtol2, max_iters), "fold launch"))
        return rc;
    if (int rc = lora::hip_status(lora::launch_halo(p, d_p, nullptr, lora::HALO_ZERO, s), "halo launch")) return rc;
    lora::CgState now = {};
    for (int step = 0; step < steps; ++step) {
        if (int rc = L.theta_start(d_u, d_f, tau, d_r, d_z, st, ts)) return rc;
        if (int rc = lora::pcg_first_direction(plan, L, m, sigma, tt, st)) return rc;
        // a V-cycle cannot exit early, so the step is enqueued in rounds of check_every iterations with the state read back between
        for (int done = 0; done < max_iters;) {
            const int round = check_every < max_iters - done ? check_every : max_iters - done;
            for (int i = 0; i < round; ++i) {
                if (int rc = L.apply_dot_shift(d_p, d_q, sigma, tt, st)) return rc;
                if (int rc = L.update(d_u, d_r, d_p, d_q, 0.0, st, 0, ts)) return rc;
                if (int rc = lora::pcg_next_direction(plan, L, m, sigma, tt, st)) return rc;
            }
            done += round;
            if (int rc = lora::hip_status(hipMemcpyAsync(&now, st, sizeof now, hipMemcpyDeviceToHost, s), "state download")) return rc;
            if (int rc = lora::hip_status(hipStreamSynchronize(s), "state download")) return rc;
            if (now.breakdown) break;  // the step is done, or the run broke down
        }
        if (now.breakdown & lora::CG_HALT_BREAKDOWN) break;
    }
    return lora::theta_read_back(plan, d_u, d_f, steps, iterations, r, s);
}

int lora_run_host_pcg(int shape, const double *in, const double *source, double *out, const double *params, const lora_mg *m,
                      const lora_until *u, lora_pcg_result *r, const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || !m || !u || !r || lora::bad_until(u) || lora::mg_bad(m, 1.0, 1.0) || lora::asymmetric(m)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a preconditioned conjugate-gradient run (its source is an argument)")) return rc;
    lora::HostRun g;
    if (int rc = g.open_solver(shape, dims, params, in, source)) return rc;
    lora_plan *plan = g.plan;
    void *d_x = g.b[0], *d_f = g.b[1];
    // set-up outside the timed region: the grids, the state, the hierarchy, and one probe as a warm-up (it writes no grid)
    if (int rc = lora_plan_prepare_pcg(plan, m, u->max_times)) return rc;
    lora_grid_diff warm;
    if (int rc = lora_plan_residual_src(plan, d_x, d_f, 0, 0, &warm, nullptr)) return rc;
    if (int rc = g.ready()) return rc;
    // timed: the start-up, the iterations and their probes
    if (int rc = g.timed(out, [&] { return lora_plan_run_pcg_until(plan, d_x, d_f, m, u, r, g.s); })) return rc;
    // per iteration: the cycle's tally in grids of the fine level, and the CG passes -- p read, q written; x, r, p, q read, x, r
    // written; r, z read; z, p read, p written
    long launches = 0;
    double cycle_bytes = 0.0;
    lora::mg_cost(plan, &launches, &cycle_bytes);
    return g.finish(r->until.times_done, cycle_bytes / (8.0 * g.points) + 13.0, 1, quiet, info);
}

int lora_run_host_theta_mg(int shape, const double *in, const double *source, double *out, const double *params, double theta, double tau,
                           int steps, int max_iters, double rtol, const lora_mg *m, int check_every, const int *dims, int quiet,
                           lora_run_info *info, lora_theta_result *result) {
    if (!in || !out || !dims || !result || !m) return LORA_EINVAL;
    if (lora::bad_theta_args(theta, tau, steps, max_iters, rtol) || check_every < 1) return LORA_EINVAL;
    const double tt = theta * tau, sigma = 1.0 + tt;
    if (lora::mg_bad(m, sigma, tt) || lora::asymmetric(m)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("an implicit run (its source is an argument)")) return rc;
    lora::HostRun g;
    if (int rc = g.open_solver(shape, dims, params, in, source)) return rc;
    lora_plan *plan = g.plan;
    void *d_u = g.b[0], *d_f = g.b[1];
    // set-up outside the timed region: the plan's grids and states, the hierarchy for (sigma, tau'), and one warm-up application
    // into the plan's own q
    if (int rc = lora::mg_admit(plan, m, sigma, tt, nullptr)) return rc;
    if (int rc = lora_plan_prepare_theta(plan, steps)) return rc;
    if (!plan->pcg_z.ensure(g.bytes)) return LORA_ENOMEM;
    if (int rc = lora::mg_prepare(plan, m, sigma, tt)) return rc;
    lora_grid_dot warm;
    if (int rc = lora_plan_apply_dot_shift(plan, d_u, plan->cg[2].ptr, 1.0, 1.0, 0, 0, &warm, nullptr)) return rc;
    if (int rc = g.ready()) return rc;
    // timed: every step's start, cycles and iterations, the state read-backs, and the steady-state probe
    if (int rc = g.timed(out, [&] { return lora_plan_run_theta_mg(plan, d_u, d_f, theta, tau, steps, max_iters, rtol, m, check_every, nullptr, result, g.s); }))
        return rc;
    // per step: u (and f) read, r and z written, one cycle, the copy and the dot; per iteration a cycle and the thirteen grids of
    // lora_run_host_pcg (the iterations enqueued past a step's last are not counted)
    long launches = 0;
    double cycle_bytes = 0.0;
    lora::mg_cost(plan, &launches, &cycle_bytes);
    const double cycle = cycle_bytes / (8.0 * g.points);
    const double per_step = (source ? 4.0 : 3.0) + cycle + 4.0 + (steps > 0 ? (cycle + 13.0) * (double) result->iterations_total / steps : 0.0);
    return g.finish(steps, per_step, 1, quiet, info);
}

}  // extern "C"
