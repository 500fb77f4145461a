// mg.cpp -- geometric multigrid for u = S(u) + f (kernels: kernels_mg.hip, the smoother: the source sweeps, the
// coarsest level: the CG launches of cg.cpp).  The host-only geometry (coarse extents, coarse taps), the public entries of the
// two transfer kernels, the level hierarchy a plan owns (lora_plan::mg), the V-cycle driver with the solvers' true-residual
// probe (reduce.cpp: true_residual), and the host-buffer operator (its skeleton: hostrun.cpp).  Shared by every entry here and
// by the PCG entries of cg.cpp: one admission (admit; mg_admit for cg.cpp) and one "cycle into the caller's grid" (cycle_into:
// the driver's cycles and mg_precondition).
//
// Coarsening is boundary-aligned and non-nested (kernels_mg.hip has the geometry): level l + 1 has floor(n / 2) cells per axis,
// the innermost rounded down to even, and the taps of level l rescaled by (h / H)^2 per axis.  On every level but the coarsest
// the smoother is damped Jacobi folded into the taps of an internal plan with the level's right-hand side as its source, so a
// smoothing application is one source sweep and the level's residual one fused defect launch (kernels_theta.hip) -- with plan
// option mgfuse one launch that also restricts it (kernels_mg_fused.hip).  The same
// cycle for A = sigma I - tau S is the preconditioner of the PCG drivers in cg.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "engine.h"

namespace lora {

int mg_coarse_dims(int ndim, const int *dims, int *cdims) {
    if (ndim < 2) return LORA_EUNSUPPORTED;
    for (int d = 0; d < ndim; ++d) {
        int nc = dims[d] / 2;
        if (d == ndim - 1) nc &= ~1;  // the fast kernels need an even innermost extent
        if (nc < 4) return LORA_EUNSUPPORTED;
        cdims[d] = nc;
    }
    return LORA_OK;
}

namespace {

constexpr int kMaxLevels = 16;  // lora_mg_result::level_dims

int centre_tap(int ndim) { return ndim == 2 ? 24 : 13; }

// the offset of tap t along the axes of `dims` (outermost first): 7 x 7 taps of radius 3, 3 x 3 x 3 of radius 1, row-major
void tap_offset(int ndim, int t, int *d) {
    if (ndim == 2) {
        d[0] = t / 7 - 3;
        d[1] = t % 7 - 3;
    } else {
        d[0] = t / 9 - 1;
        d[1] = t / 3 % 3 - 1;
        d[2] = t % 3 - 1;
    }
}

void coarse_taps(int ndim, const double *w, const int *dims, const int *cdims, double *wc) {
    const int ntaps = ndim == 2 ? 49 : 27, c = centre_tap(ndim);
    double q[3];
    for (int a = 0; a < ndim; ++a) {
        const double rho = (double) (cdims[a] + 1) / (double) (dims[a] + 1);
        q[a] = rho * rho;
    }
    double sum = 0.0, others = 0.0;
    for (int t = 0; t < ntaps; ++t) sum += w[t];
    for (int t = 0; t < ntaps; ++t) {
        if (t == c) continue;
        int d[3];
        tap_offset(ndim, t, d);
        double len2 = 0.0;
        for (int a = 0; a < ndim; ++a) len2 += (double) (d[a] * d[a]);
        double f = 1.0;
        for (int a = 0; a < ndim; ++a)
            if (d[a] != 0) f *= (double) (d[a] * d[a]) == len2 ? q[a] : std::pow(q[a], (double) (d[a] * d[a]) / len2);
        wc[t] = w[t] * f;
        others += wc[t];
    }
    wc[c] = sum - others;
}

// any check_every >= 1 counts cycles; the other rules are lora_plan_run_until's
bool bad_mg_until(const lora_until *u) {
    if (u->check_every < 1 || u->max_times < 0 || (u->norm != LORA_NORM_MAX && u->norm != LORA_NORM_RMS)) return true;
    return !(u->tol >= 0.0) || !(u->rtol >= 0.0);
}

bool bad_mg(const lora_mg *m) {
    if (m->pre < 0 || m->post < 0 || (long) m->pre + m->post < 1) return true;
    if (!(m->omega > 0.0 && m->omega < 2.0)) return true;  // (a NaN fails both)
    return m->max_levels < 0 || m->max_levels == 1 || m->coarse_iters < 0;
}

int no_mg_kernels() {
    return unsupported("this plan has no multigrid kernels: they take fp64 plans with the conjugate-gradient kernels (option \"cg\"), of a 2D or "
                       "3D shape, whose extents halve to at least 4 cells per axis");
}

// What a level is on the host: extents, taps, the smoother's factor and taps.
struct LevelDesc {
    int dims[3] = {0, 0, 0};
    double w[49] = {0}, s[49] = {0};
    double d = 0.0, c = 0.0;
};

bool bad_pair(double sigma, double tau) { return !std::isfinite(sigma) || !std::isfinite(tau) || !(tau >= 0.0) || !(sigma > 0.0); }

// The levels of a plan for `m` and A = sigma I - tau S: LORA_OK, or LORA_EUNSUPPORTED for a level whose diagonal
// sigma - tau w[centre] is not positive and finite.  With sigma == tau == 1 every product with 1 is exact: the taps of I - S.
int describe_levels(const Plan &p, const lora_mg *m, double sigma, double tau, std::vector<LevelDesc> &out) {
#pragma clang fp contract(off)
    const int cap = m->max_levels ? (m->max_levels < kMaxLevels ? m->max_levels : kMaxLevels) : kMaxLevels;
    const int c = centre_tap(p.ndim);
    out.clear();
    LevelDesc lv;
    for (int a = 0; a < p.ndim; ++a) lv.dims[a] = p.dims[a];
    std::memcpy(lv.w, p.w, sizeof(double) * p.ntaps);
    for (;;) {
        {
            const double tw = tau * lv.w[c];
            lv.d = sigma - tw;
        }
        if (!(lv.d > 0.0) || !std::isfinite(lv.d))
            return unsupported("a multigrid level's diagonal sigma - tau w[centre] is not positive and finite: damped Jacobi cannot smooth it");
        lv.c = m->omega / lv.d;
        const double ct = lv.c * tau;
        for (int t = 0; t < p.ntaps; ++t) lv.s[t] = ct * lv.w[t];
        {
            const double cs = lv.c * sigma;
            const double keep = 1.0 - cs;
            lv.s[c] = lv.s[c] + keep;
        }
        out.push_back(lv);
        LevelDesc next;
        if ((int) out.size() >= cap || mg_coarse_dims(p.ndim, lv.dims, next.dims) != LORA_OK) break;
        coarse_taps(p.ndim, lv.w, lv.dims, next.dims, next.w);
        lv = next;
    }
    return LORA_OK;
}

struct Level {
    LevelDesc desc;
    lora_plan *smooth = nullptr;  // levels below the coarsest: Dirichlet, taps s, source g
    lora_plan *plain = nullptr;   // the coarsest level: taps w; its CG set holds r (= g), p, q
    DeviceGrid x, spare, g;       // level 0: x is the caller's; the coarsest: x alone
    size_t bytes = 0;             // of a padded grid
    double cells = 0.0;           // of the interior
    double *cur = nullptr, *other = nullptr;  // where the level's iterate is during a cycle, and the level's free grid
};

}  // namespace

struct MgHierarchy {
    std::vector<Level> levels;
    double omega = 0.0, sigma = 1.0, tau = 1.0;
    int max_levels = 0, device = -1;
    unsigned epoch = 0;
    long launches = 0;  // of the last cycle enqueued ...
    double bytes = 0.0; // ... and the bytes its launches move
    ~MgHierarchy() {
        for (Level &lv : levels) {
            lora_plan_destroy(lv.smooth);
            lora_plan_destroy(lv.plain);
            lv.x.release();
            lv.spare.release();
            lv.g.release();
        }
    }
};

void mg_release(lora_plan *plan) {
    delete plan->mg;
    plan->mg = nullptr;
}

namespace {

// an internal plan of the hierarchy: the thread's defaults (boundary, normalised taps, coarse1, mgfuse) must not reach it
int make_plan(lora_plan **out, int shape, const int *dims, const double *taps, int ntaps, int boundary) {
    const int old_bc = lora_set_default_boundary(LORA_BC_REFERENCE), old_norm = lora_set_default_normalize(0);
    const int old_c1 = lora_set_default_coarse1(0), old_fuse = lora_set_default_mgfuse(0);
    int rc = lora_plan_create(out, shape, LORA_F64, dims, nullptr);
    lora_set_default_boundary(old_bc);
    lora_set_default_normalize(old_norm);
    lora_set_default_coarse1(old_c1);
    lora_set_default_mgfuse(old_fuse);
    if (rc == LORA_OK) rc = lora_plan_set_weights(*out, taps, ntaps);
    if (rc == LORA_OK) rc = lora_plan_set_boundary(*out, boundary);
    // launched directly and through two grids alone: no graph, no scratch grid (neither moves a bit)
    if (rc == LORA_OK) rc = lora_plan_set_option(*out, "graph", 0);
    if (rc == LORA_OK) rc = lora_plan_set_option(*out, "scratch", 0);
    return rc;
}

// The plan's hierarchy for `m` and (sigma, tau) on the current device, built or rebuilt when the taps, the damping, the pair, the
// depth or the device changed.
int ensure_hierarchy(lora_plan *plan, const lora_mg *m, double sigma, double tau, bool with_source) {
    const Plan &p = plan->p;
    int device = -1;
    if (int rc = hip_status(hipGetDevice(&device), "hipGetDevice")) return rc;
    MgHierarchy *h = plan->mg;
    if (!(h && h->omega == m->omega && h->sigma == sigma && h->tau == tau && h->max_levels == m->max_levels && h->epoch == p.epoch && h->device == device)) {
        mg_release(plan);
        std::vector<LevelDesc> descs;
        if (int rc = describe_levels(p, m, sigma, tau, descs)) return rc;
        h = new (std::nothrow) MgHierarchy();
        if (!h) return LORA_ENOMEM;
        plan->mg = h;
        h->omega = m->omega;
        h->sigma = sigma;
        h->tau = tau;
        h->max_levels = m->max_levels;
        h->epoch = p.epoch;
        h->device = device;
        h->levels.resize(descs.size());
        const int L = (int) descs.size() - 1;
        for (int l = 0; l <= L; ++l) {
            Level &lv = h->levels[l];
            lv.desc = descs[l];
            lv.bytes = lora_padded_count(p.shape, lv.desc.dims) * sizeof(double);
            lv.cells = 1.0;
            for (int a = 0; a < p.ndim; ++a) lv.cells *= lv.desc.dims[a];
            const int rc = l < L ? make_plan(&lv.smooth, p.shape, lv.desc.dims, lv.desc.s, p.ntaps, LORA_BC_DIRICHLET)
                                 : make_plan(&lv.plain, p.shape, lv.desc.dims, lv.desc.w, p.ntaps, LORA_BC_REFERENCE);
            if (rc != LORA_OK) {
                mg_release(plan);
                return rc;
            }
        }
    }
    const int L = (int) h->levels.size() - 1;
    for (int l = 0; l <= L; ++l) {
        Level &lv = h->levels[l];
        bool ok = true;
        if (l > 0) ok = ok && lv.x.ensure(lv.bytes);
        if (l < L) ok = ok && lv.spare.ensure(lv.bytes);
        if (l < L && (l > 0 || with_source)) ok = ok && lv.g.ensure(lv.bytes);
        if (!ok) return LORA_ENOMEM;
        if (l == L) {
            if (int rc = ensure_cg_grids(lv.plain)) return rc;
            ReduceRecord *records = nullptr;
            if (int rc = reduction_records(lv.plain, &records)) return rc;
        } else if (l > 0) {
            if (int rc = lora_plan_set_source(lv.smooth, lv.g.ptr)) return rc;
        }
    }
    return LORA_OK;
}

// what a cycle enqueues (lora_plan_mg_cycle_cost)
struct Tally {
    long launches = 0;
    double bytes = 0.0;
    void add(int n, double cells, double grids) {  // n launches that move `grids` grids of `cells` cells between them
        launches += n;
        bytes += 8.0 * cells * grids;
    }
};

// `times` applications of the level's smoothing plan from lv.cur, with the values lora_plan_run of that plan gives; the iterate
// ends in lv.cur.  With a source: the launch layer directly, two applications per launch where the plan has them (2D), so that
// an even count never runs as single sweeps and nothing re-copies a halo both grids already share.  Without one (level 0 of a
// run without f) the plan's own fused families apply, whose sums may run in another order than single sweeps: lora_plan_run.
int smooth(Level &lv, int times, hipStream_t s, Tally &tally) {
    if (times <= 0) return LORA_OK;
    const Plan &p = lv.smooth->p;
    if (!p.source) {
        if (int rc = lora_plan_run(lv.smooth, lv.cur, lv.other, times, s)) return rc;
        const int n = dirichlet_run_launches(lv.smooth, times);  // a halo copy, then launches that read one grid and write one
        tally.add(n, lv.cells, 2.0 * (n - 1));
        if (times % 2) std::swap(lv.cur, lv.other);
        return LORA_OK;
    }
    for (int left = times; left > 0;) {
        const int k = (p.steps_per_launch == 2 && left >= 2) ? 2 : 1;
        if (int rc = launch_apps(p, {k, 0, p.dims[0]}, lv.cur, lv.other, s)) return rc;
        tally.add(1, lv.cells, 3.0);
        std::swap(lv.cur, lv.other);
        left -= k;
    }
    return LORA_OK;
}

struct Run {
    lora_plan *plan;
    MgHierarchy *h;
    const lora_mg *m;
    hipStream_t s;
    int ndim, L, coarse_iters;
};

// one V-cycle from level l down and up again; the level's iterate is in levels[l].cur before and after
int cycle(const Run &r, int l, Tally &tally) {
    Level &lv = r.h->levels[l];
    if (l == r.L) {
        // plan option coarse1: a coarsest level that fits one workgroup is ONE launch -- lora_plan_cg_small on the
        // level's plain plan, from the residual the restriction put into its r
        if (r.plan->p.coarse1 && has_cg_small(lv.plain->p)) {
            if (int rc = lora_plan_cg_small(lv.plain, lv.cur, lv.plain->cg[0].ptr, r.coarse_iters, r.h->sigma, r.h->tau, nullptr, r.s)) return rc;
            tally.add(1, lv.cells, 4.0);  // x and r read, x and r written (coarse_iters >= 1: coarse_iterations())
            return LORA_OK;
        }
        if (int rc = cg_fixed_iterations(lv.plain, lv.cur, r.coarse_iters, r.h->sigma, r.h->tau, r.s, &tally.launches)) return rc;
        tally.bytes += 8.0 * lv.cells * (3.0 + 11.0 * r.coarse_iters);  // the copy and the dot; eleven grids an iteration (lora_run_host_cg)
        return LORA_OK;
    }
    Level &co = r.h->levels[l + 1];
    const Plan &sp = lv.smooth->p;
    if (int rc = smooth(lv, r.m->pre, r.s, tally)) return rc;
    // the coarse right-hand side: scaled for the coarse smoother, unscaled for the coarsest level's CG
    const bool last = l + 1 == r.L;
    const double scale = last ? 1.0 / lv.desc.c : co.desc.c / lv.desc.c;
    double *g = static_cast<double *>(last ? co.plain->cg[0].ptr : co.g.ptr);
    Plan bare = sp;
    bare.source = nullptr;
    const double *src = static_cast<const double *>(sp.source);
    if (r.plan->p.mgfuse) {
        // plan option mgfuse: the defect restricted in the launch that computes it, the same bits in g; the level's
        // free grid is not written
        if (int rc = hip_status(launch_mg_defect_restrict(bare, co.desc.dims, lv.cur, src, g, scale, r.s), "fused defect and restriction launch"))
            return rc;
        tally.add(1, lv.cells, src ? 2.0 : 1.0);
        tally.add(0, co.cells, 1.0);
    } else {
        // rs = fl(fl(S_s(x) + g) - x) = c_l times the level's residual, in the level's free grid: one launch, the source its argument
        if (int rc = defect_whole(bare, lv.cur, src, lv.other, r.s)) return rc;
        tally.add(1, lv.cells, src ? 3.0 : 2.0);
        if (int rc = hip_status(launch_mg_restrict(r.ndim, lv.desc.dims, co.desc.dims, lv.other, g, scale, r.s), "restriction launch")) return rc;
        tally.add(1, lv.cells + co.cells, 1.0);
    }
    co.cur = static_cast<double *>(co.x.ptr);
    co.other = static_cast<double *>(co.spare.ptr);
    if (int rc = hip_status(hipMemsetAsync(co.cur, 0, co.bytes, r.s), "coarse start")) return rc;
    tally.add(1, (double) co.bytes / 8.0, 1.0);
    if (int rc = cycle(r, l + 1, tally)) return rc;
    if (int rc = hip_status(launch_mg_prolong_add(r.ndim, lv.desc.dims, co.desc.dims, co.cur, lv.cur, r.s), "prolongation launch")) return rc;
    tally.add(1, 2.0 * lv.cells + co.cells, 1.0);
    return smooth(lv, r.m->post, r.s, tally);
}

void fill_levels(const std::vector<LevelDesc> &descs, lora_mg_result *r) {
    r->levels = (int) descs.size();
    for (int l = 0; l < kMaxLevels; ++l)
        for (int a = 0; a < 3; ++a) r->level_dims[l][a] = l < (int) descs.size() ? descs[l].dims[a] : 0;
}

// What every multigrid entry refuses before a device is asked for, behind its LORA_EINVAL checks: a plan without the kernels,
// taps that are not point-symmetric (`op` names the entry's operator in that text), a level whose diagonal cannot be smoothed.
// descs: the levels of the hierarchy for (m, sigma, tau).
int admit(const lora_plan *plan, const lora_mg *m, double sigma, double tau, const char *op, std::vector<LevelDesc> &descs) {
    const Plan &p = plan->p;
    if (!has_mg(p)) return no_mg_kernels();
    if (!taps_symmetric(p.w, p.ntaps))
        return unsupported((std::string("multigrid needs point-symmetric taps, w[t] == w[ntaps - 1 - t]: ") + op + " is not symmetric otherwise").c_str());
    return describe_levels(p, m, sigma, tau, descs);
}

// the halos every level's free grid shares with its iterate below level 0, and the coarsest level's iterate
int reset_level_halos(MgHierarchy *h, hipStream_t s) {
    const int L = (int) h->levels.size() - 1;
    for (int l = 1; l < L; ++l)
        if (int rc = hip_status(launch_halo(h->levels[l].smooth->p, h->levels[l].spare.ptr, nullptr, HALO_ZERO, s), "halo reset")) return rc;
    h->levels[L].cur = static_cast<double *>(h->levels[L].x.ptr);
    return LORA_OK;
}

int coarse_iterations(const MgHierarchy *h, const lora_mg *m) {
    return m->coarse_iters ? m->coarse_iters : (int) std::fmin(h->levels.back().cells, 64.0);
}

// One V-cycle of level 0 from the iterate in `dst` (the level's free grid: `spare`) that leaves the iterate in `dst`; `tally`
// (what the caller enqueued in front of the cycle) plus the cycle's launches becomes the hierarchy's cost of a cycle.
int cycle_into(const Run &r, double *dst, double *spare, Tally tally = Tally()) {
    const Plan &p = r.plan->p;
    Level &top = r.h->levels[0];
    top.cur = dst;
    top.other = spare;
    if (int rc = cycle(r, 0, tally)) return rc;
    if (top.cur != dst) {  // an odd number of launches moved the iterate: back into the caller's grid, interior cells only
        const int *pad = interior_pads(p.ndim);
        if (int rc = hip_status(launch_copy_interior(LORA_F64, p.ndim, p.dims, dst, pad, top.cur, pad, r.s), "copy launch")) return rc;
        tally.add(1, top.cells, 2.0);
    }
    r.h->launches = tally.launches;
    r.h->bytes = tally.bytes;
    return LORA_OK;
}

}  // namespace

bool mg_bad(const lora_mg *m, double sigma, double tau) { return bad_mg(m) || bad_pair(sigma, tau); }

int mg_admit(const lora_plan *plan, const lora_mg *m, double sigma, double tau, int *levels) {
    if (mg_bad(m, sigma, tau)) return LORA_EINVAL;
    std::vector<LevelDesc> descs;
    if (int rc = admit(plan, m, sigma, tau, "sigma I - tau S", descs)) return rc;
    if (levels) *levels = (int) descs.size();
    return LORA_OK;
}

int mg_prepare(lora_plan *plan, const lora_mg *m, double sigma, double tau) { return ensure_hierarchy(plan, m, sigma, tau, true); }

bool mg_owns(const lora_plan *plan, const void *buf) {
    if (!plan->mg || !buf) return false;
    for (const Level &lv : plan->mg->levels) {
        const void *own[] = {lv.x.ptr, lv.spare.ptr, lv.g.ptr, lv.plain ? lv.plain->cg[0].ptr : nullptr, lv.plain ? lv.plain->cg[1].ptr : nullptr,
                             lv.plain ? lv.plain->cg[2].ptr : nullptr};
        for (const void *o : own)
            if (o && o == buf) return true;
    }
    return false;
}

void mg_cost(const lora_plan *plan, long *launches, double *bytes) {
    *launches = plan->mg ? plan->mg->launches : 0;
    *bytes = plan->mg ? plan->mg->bytes : 0.0;
}

// z = M r: one V-cycle for A z = r from z = 0 (lora_plan_mg_precondition has the contract); the tally counts all of it
int mg_precondition(lora_plan *plan, const double *d_r, double *d_z, const lora_mg *m, double sigma, double tau, hipStream_t s) {
    const Plan &p = plan->p;
    if (int rc = ensure_hierarchy(plan, m, sigma, tau, true)) return rc;
    MgHierarchy *h = plan->mg;
    Level &top = h->levels[0];
    double *spare0 = static_cast<double *>(top.spare.ptr);
    if (int rc = lora_plan_set_source(top.smooth, top.g.ptr)) return rc;
    Tally tally;
    if (int rc = hip_status(launch_mg_scale(p.ndim, p.dims, static_cast<double *>(top.g.ptr), d_r, top.desc.c, s), "source scale launch")) return rc;
    tally.add(1, top.cells, 2.0);
    if (int rc = hip_status(hipMemsetAsync(d_z, 0, top.bytes, s), "zero start")) return rc;
    tally.add(1, (double) top.bytes / 8.0, 1.0);
    if (int rc = hip_status(launch_halo(p, spare0, nullptr, HALO_ZERO, s), "halo reset")) return rc;
    if (int rc = reset_level_halos(h, s)) return rc;
    tally.launches += (long) h->levels.size() - 1;  // (the halo resets: a grid's rim each)
    const Run run = {plan, h, m, s, p.ndim, (int) h->levels.size() - 1, coarse_iterations(h, m)};
    return cycle_into(run, d_z, spare0, tally);
}

}  // namespace lora

using lora::Plan;

extern "C" {

int lora_mg_coarse_dims(int shape, const int *dims, int *cdims) {
    const int nd = lora::shape_ndim(shape);
    if (nd == 0 || !dims || !cdims) return LORA_EINVAL;
    for (int d = 0; d < nd; ++d)
        if (dims[d] < 1) return LORA_EINVAL;
    return lora::mg_coarse_dims(nd, dims, cdims);
}

int lora_mg_coarse_taps(int shape, const double *w, const int *dims, const int *cdims, double *wc) {
    const int nd = lora::shape_ndim(shape);
    if (nd == 0 || !w || !dims || !cdims || !wc) return LORA_EINVAL;
    for (int d = 0; d < nd; ++d)
        if (dims[d] < 1 || cdims[d] < 1) return LORA_EINVAL;
    if (nd < 2) return LORA_EUNSUPPORTED;
    lora::coarse_taps(nd, w, dims, cdims, wc);
    return LORA_OK;
}

int lora_plan_mg_restrict(lora_plan *plan, const void *d_fine, void *d_coarse, double scale, void *stream) {
    if (!plan || !d_fine || !d_coarse || !std::isfinite(scale) || d_fine == d_coarse) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_fine, d_coarse)) return rc;
    const Plan &p = plan->p;
    if (!lora::has_mg(p)) return lora::no_mg_kernels();
    if (lora_device_count() <= 0) return lora::no_device();
    int cdims[3] = {0, 0, 0};
    lora::mg_coarse_dims(p.ndim, p.dims, cdims);
    return lora::hip_status(lora::launch_mg_restrict(p.ndim, p.dims, cdims, static_cast<const double *>(d_fine), static_cast<double *>(d_coarse),
                                                     scale, static_cast<hipStream_t>(stream)),
                            "restriction launch");
}

int lora_plan_mg_defect_restrict(lora_plan *plan, const void *d_u, const void *d_f, void *d_coarse, double scale, void *stream) {
    if (!plan || !d_u || !d_coarse) return LORA_EINVAL;
    if (!std::isfinite(scale)) return LORA_EINVAL;
    if (d_u == d_coarse || d_f == d_u || d_f == d_coarse) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_u, d_coarse)) return rc;
    if (lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    const Plan &p = plan->p;
    if (!lora::has_mg(p)) return lora::no_mg_kernels();
    if (lora_device_count() <= 0) return lora::no_device();
    int cdims[3] = {0, 0, 0};
    lora::mg_coarse_dims(p.ndim, p.dims, cdims);
    return lora::hip_status(lora::launch_mg_defect_restrict(p, cdims, static_cast<const double *>(d_u), static_cast<const double *>(d_f),
                                                            static_cast<double *>(d_coarse), scale, static_cast<hipStream_t>(stream)),
                            "fused defect and restriction launch");
}

int lora_plan_mg_prolong_add(lora_plan *plan, const void *d_coarse, void *d_fine, void *stream) {
    if (!plan || !d_coarse || !d_fine || d_fine == d_coarse) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_coarse, d_fine)) return rc;
    const Plan &p = plan->p;
    if (!lora::has_mg(p)) return lora::no_mg_kernels();
    if (lora_device_count() <= 0) return lora::no_device();
    int cdims[3] = {0, 0, 0};
    lora::mg_coarse_dims(p.ndim, p.dims, cdims);
    return lora::hip_status(lora::launch_mg_prolong_add(p.ndim, p.dims, cdims, static_cast<const double *>(d_coarse), static_cast<double *>(d_fine),
                                                        static_cast<hipStream_t>(stream)),
                            "prolongation launch");
}

int lora_plan_prepare_mg(lora_plan *plan, const lora_mg *m) {
    if (!plan || !m || lora::bad_mg(m)) return LORA_EINVAL;
    std::vector<lora::LevelDesc> descs;
    if (int rc = lora::admit(plan, m, 1.0, 1.0, "I - S", descs)) return rc;
    if (lora_device_count() <= 0) return lora::no_device();
    lora::ReduceRecord *records = nullptr;  // (the probe folds into the plan's records: they are part of what a run needs)
    if (int rc = lora::reduction_records(plan, &records)) return rc;
    return lora::ensure_hierarchy(plan, m, 1.0, 1.0, true);
}

int lora_plan_mg_precondition(lora_plan *plan, const void *d_r, void *d_z, const lora_mg *m, double sigma, double tau, void *stream) {
    if (!plan || !d_r || !d_z || !m || lora::bad_mg(m) || lora::bad_pair(sigma, tau) || d_r == d_z) return LORA_EINVAL;
    if (lora::misaligned(d_r) || lora::misaligned(d_z)) return lora::unsupported("device buffers must be 16-byte aligned");
    if (int rc = lora::mg_admit(plan, m, sigma, tau, nullptr)) return rc;
    if (lora_device_count() <= 0) return lora::no_device();
    if (int rc = lora::mg_prepare(plan, m, sigma, tau)) return rc;
    if (lora::mg_owns(plan, d_r) || lora::mg_owns(plan, d_z)) return LORA_EINVAL;
    return lora::mg_precondition(plan, static_cast<const double *>(d_r), static_cast<double *>(d_z), m, sigma, tau,
                                 static_cast<hipStream_t>(stream));
}

int lora_plan_mg_cycle_cost(const lora_plan *plan, int *launches, double *bytes) {
    if (!plan || !launches || !bytes || !plan->mg || plan->mg->launches == 0) return LORA_EINVAL;
    *launches = (int) plan->mg->launches;
    *bytes = plan->mg->bytes;
    return LORA_OK;
}

int lora_plan_run_mg_until(lora_plan *plan, void *d_x, const void *d_f, const lora_mg *m, const lora_until *u, lora_mg_result *r,
                           void *stream) {
    if (!plan || !d_x || !m || !u || !r || lora::bad_mg_until(u) || lora::bad_mg(m) || d_f == d_x) return LORA_EINVAL;
    if (lora::misaligned(d_x) || lora::misaligned(d_f)) return lora::unsupported("device buffers must be 16-byte aligned");
    const Plan &p = plan->p;
    std::vector<lora::LevelDesc> descs;
    if (int rc = lora::admit(plan, m, 1.0, 1.0, "I - S", descs)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit_reduction(d_x, d_x, s)) return rc;
    *r = {{0, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}}, 0, {{0}}};
    lora::fill_levels(descs, r);
    if (u->max_times < u->check_every) return LORA_OK;
    if (int rc = lora::ensure_hierarchy(plan, m, 1.0, 1.0, d_f != nullptr)) return rc;
    lora::MgHierarchy *h = plan->mg;
    const int L = (int) h->levels.size() - 1;
    if (lora::mg_owns(plan, d_x) || lora::mg_owns(plan, d_f)) return LORA_EINVAL;
    lora::ReduceRecord *records = nullptr;
    if (int rc = lora::reduction_records(plan, &records)) return rc;

    // once per run, on this stream: level 0's source g_0 = fl(c_0 f) and the halos every level's free grid shares with its iterate
    lora::Level &top = h->levels[0];
    double *x0 = static_cast<double *>(d_x), *spare0 = static_cast<double *>(top.spare.ptr);
    if (int rc = lora_plan_set_source(top.smooth, d_f ? top.g.ptr : nullptr)) return rc;
    if (d_f)
        if (int rc = lora::hip_status(lora::launch_mg_scale(p.ndim, p.dims, static_cast<double *>(top.g.ptr), static_cast<const double *>(d_f),
                                                            top.desc.c, s),
                                      "source scale launch"))
            return rc;
    if (int rc = lora::hip_status(lora::launch_halo(p, spare0, d_x, lora::HALO_COPY, s), "halo copy")) return rc;
    if (int rc = lora::reset_level_halos(h, s)) return rc;

    const lora::Run run = {plan, h, m, s, p.ndim, L, lora::coarse_iterations(h, m)};
    // the probe (as lora_plan_run_cg_until): fused under the max norm, else two passes through level 0's free grid
    const bool fused = u->norm == LORA_NORM_MAX;
    lora_until_result &ur = r->until;
    while (ur.times_done + u->check_every <= u->max_times) {
        for (int i = 0; i < u->check_every; ++i)
            if (int rc = lora::cycle_into(run, x0, spare0)) return rc;
        if (int rc = lora::true_residual(plan, d_x, d_f, spare0, fused, &ur.last, s)) return rc;
        ur.times_done += u->check_every;
        if (lora::until_decide(u, &ur)) break;
    }
    return LORA_OK;
}

int lora_run_host_mg(int shape, const double *in, const double *source, double *out, const double *params, const lora_mg *m,
                     const lora_until *u, lora_mg_result *r, const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || !m || !u || !r || lora::bad_mg_until(u) || lora::bad_mg(m)) return LORA_EINVAL;
    if (int rc = lora::default_source_refused("a multigrid run (its source is an argument)")) return rc;
    lora::HostRun g;
    if (int rc = g.open_solver(shape, dims, params, in, source)) return rc;
    lora_plan *plan = g.plan;
    void *d_x = g.b[0], *d_f = g.b[1];
    // set-up outside the timed region: the hierarchy, and one probe as a warm-up (it writes no grid)
    if (int rc = lora_plan_prepare_mg(plan, m)) return rc;
    lora_grid_diff warm;
    if (int rc = lora_plan_residual_src(plan, d_x, d_f, 0, 0, &warm, nullptr)) return rc;
    if (int rc = g.ready()) return rc;
    // timed: the cycles and their probes
    if (int rc = g.timed(out, [&] { return lora_plan_run_mg_until(plan, d_x, d_f, m, u, r, g.s); })) return rc;
    // per cycle: the bytes its launches move (lora_plan_mg_cycle_cost), in grids of the fine level
    const double per_cycle = plan->mg && plan->mg->launches ? plan->mg->bytes / (8.0 * g.points) : 0.0;
    return g.finish(r->until.times_done, per_cycle, 1, quiet, info);
}

}  // extern "C"
