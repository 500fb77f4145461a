// reduce.cpp -- host side of the device-side reductions (kernels_reduce.hip; their records: lora_plan::records) and what is
// built on them: lora_plan_stats, lora_plan_diff, lora_plan_dot, lora_plan_residual and lora_plan_residual_src (kernels_residual.hip),
// lora_grid_stats_merge, the run-until-steady driver lora_plan_run_until, what it shares with the solver drivers (bad_until,
// until_decide), their true-residual probe (true_residual: the CG, PCG, multigrid and Chebyshev drivers) and its group-A form
// (its skeleton: hostrun.cpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "engine.h"
#include "residual_tiles.h"

namespace lora {

#define LORA_HIP_TRY(expr)                    \
    do {                                      \
        hipError_t e__ = (expr);              \
        if (e__ != hipSuccess) {              \
            lora::set_last_error(#expr, e__); \
            return LORA_EHIP;                 \
        }                                     \
    } while (0)

// Launch geometry of a box: everything here follows from the dtype, the extents and the box, never from the device or from
// an earlier call -- which is what makes a reduction return the same bits every time.
bool reduce_geometry(const Plan &p, const int *lo, const int *hi, ReduceArgs &a, int &kind, int &groups) {
    const int *hw = interior_pads(p.ndim);
    long P[3] = {1, 1, 1};
    int l[3] = {0, 0, 0}, h[3] = {1, 1, 1};
    for (int d = 0; d < 3; ++d) {
        const int sd = d - (3 - p.ndim);
        if (sd < 0) continue;
        P[d] = (long) p.dims[sd] + 2 * hw[sd];
        l[d] = lo[sd];
        h[d] = hi[sd];
        if (l[d] < 0 || h[d] > P[d] || h[d] <= l[d]) return false;
    }
    // 16-byte pieces wherever rows start on 16 bytes: a 1D array is one row; bf16 rows are a multiple of 8 cells
    kind = p.dtype == LORA_BF16 ? KIND_BF16X8 : ((p.ndim == 1 || P[2] % 2 == 0) ? KIND_F64X2 : KIND_F64X1);
    const int C = kind == KIND_BF16X8 ? 8 : (kind == KIND_F64X2 ? 2 : 1);
    a.q0 = l[2] / C;
    a.ppr = (h[2] + C - 1) / C - a.q0;  // the last piece ends at most at the row's end: rows are whole pieces (1D: n + 5 <= n + 8)
    a.e1 = h[1] - l[1];
    a.total = (long) (h[0] - l[0]) * a.e1 * a.ppr;
    a.col_lo = l[2];
    a.col_hi = h[2];
    a.row_stride = P[2];
    a.plane_stride = P[1] * P[2];
    a.off0 = ((long) l[0] * P[1] + l[1]) * P[2] + (long) a.q0 * C;
    // at least eight strides of the lanes per workgroup, at most kReduceMaxGroups workgroups (four per CU of 256)
    const long S = reduce_threads();
    long g = (a.total + 8 * S - 1) / (8 * S);
    g = g < 1 ? 1 : (g > kReduceMaxGroups ? kReduceMaxGroups : g);
    a.chunk = ((a.total + g - 1) / g + S - 1) / S * S;
    groups = (int) ((a.total + a.chunk - 1) / a.chunk);
    const long rows = S / a.ppr, d0 = rows / a.e1;
    a.dq = (int) (S % a.ppr);
    a.d1 = (int) (rows % a.e1);
    a.step_off = d0 * a.plane_stride + a.d1 * a.row_stride + (long) a.dq * C;
    a.row_carry = a.row_stride - (long) a.ppr * C;
    a.plane_carry = a.plane_stride - (long) a.e1 * a.row_stride;
    return true;
}

// the interior box of the outermost range [begin, end): its launch geometry and its number of cells
bool interior_geometry(const Plan &p, int begin, int end, ReduceArgs &a, int &kind, int &groups, long long &count) {
    const int *hw = interior_pads(p.ndim);
    int lo[3], hi[3];
    count = 1;
    for (int d = 0; d < p.ndim; ++d) {
        lo[d] = hw[d] + (d == 0 ? begin : 0);
        hi[d] = hw[d] + (d == 0 ? end : p.dims[d]);
        count *= hi[d] - lo[d];
    }
    return reduce_geometry(p, lo, hi, a, kind, groups);
}

// the folded record back on the host (blocks)
int folded_record(const ReduceRecord *records, ReduceRecord &rec, hipStream_t s) {
    LORA_HIP_TRY(hipMemcpyAsync(&rec, records + kReduceMaxGroups, sizeof rec, hipMemcpyDeviceToHost, s));
    LORA_HIP_TRY(hipStreamSynchronize(s));
    return LORA_OK;
}

namespace {

// the plan's records on the current device
int ensure_records(lora_plan *plan, ReduceRecord **out) {
    int dev = 0;
    LORA_HIP_TRY(hipGetDevice(&dev));
    if (!plan->records.ensure(sizeof(ReduceRecord) * (kReduceMaxGroups + 1))) return LORA_ENOMEM;
    *out = static_cast<ReduceRecord *>(plan->records.ptr);
    return LORA_OK;
}

// 1 = whole interior or a proper range, 0 = an empty one, < 0 = a bad one
int resolve_range(const Plan &p, int &begin, int &end) {
    if (begin == 0 && end == 0) end = p.dims[0];
    if (begin < 0 || end > p.dims[0] || begin > end) return LORA_EINVAL;
    return begin < end;
}

// what every reduction entry checks before it touches the device
int admit(const void *a, const void *b, hipStream_t s) {
    if (int rc = check_buffers(a, b)) return rc;
    if (lora_device_count() <= 0) return no_device();
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void) hipGetLastError();
        st = hipStreamCaptureStatusActive;  // (the legacy stream while another stream captures globally)
    }
    if (st != hipStreamCaptureStatusNone) {
        set_last_error_text("a reduction returns its result to the host: the stream must not be capturing");
        return LORA_EUNSUPPORTED;
    }
    return LORA_OK;
}

// launches over the outermost range [begin, end) and the folded record back on the host (blocks)
int reduce_range(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, ReduceRecord &rec, long long &count,
                 hipStream_t s) {
    ReduceArgs a;
    int kind = 0, groups = 0;
    if (!interior_geometry(plan->p, begin, end, a, kind, groups, count)) return LORA_EINVAL;
    ReduceRecord *records = nullptr;
    if (int rc = ensure_records(plan, &records)) return rc;
    const hipError_t e = d_b ? launch_reduce_diff(a, kind, groups, d_a, d_b, records, s) : launch_reduce_stats(a, kind, groups, d_a, records, s);
    if (e != hipSuccess) {
        set_last_error("reduction kernel launch", e);
        return LORA_EHIP;
    }
    return folded_record(records, rec, s);
}

// sum of a * b over [begin, end) (a proper range): the folded record (blocks)
int dot_range(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_dot *out, hipStream_t s) {
    ReduceArgs a;
    int kind = 0, groups = 0;
    long long count = 0;
    if (!interior_geometry(plan->p, begin, end, a, kind, groups, count)) return LORA_EINVAL;
    ReduceRecord *records = nullptr;
    if (int rc = ensure_records(plan, &records)) return rc;
    const hipError_t e = launch_reduce_dot(a, kind, groups, d_a, d_b, records, s);
    if (e != hipSuccess) {
        set_last_error("reduction kernel launch", e);
        return LORA_EHIP;
    }
    ReduceRecord rec;
    if (int rc = folded_record(records, rec, s)) return rc;
    *out = {rec.f[0], rec.f[1], count, rec.i[0]};
    return LORA_OK;
}

const lora_grid_stats kEmptyStats = {HUGE_VAL, -HUGE_VAL, 0.0, 0.0, 0.0, 0, 0};

int diff_range(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_diff *out, hipStream_t s) {
    ReduceRecord rec;
    long long count = 0;
    if (int rc = reduce_range(plan, d_a, d_b, begin, end, rec, count, s)) return rc;
    const bool any = rec.f[0] >= 0.0;  // the kernels' "no finite difference" is max_abs = -1
    *out = {any ? rec.f[0] : 0.0, rec.f[1], rec.f[2], any ? rec.i[0] : -1, count, rec.i[1]};
    return LORA_OK;
}

// one raw sweep of d_in (plus d_f, where given) against d_in over [begin, end) (a proper range of a plan that has the
// kernel): the folded record (blocks)
int residual_range(lora_plan *plan, const void *d_in, const void *d_f, int begin, int end, lora_grid_diff *out, hipStream_t s) {
    const Plan &p = plan->p;
    ResidualTiles rt;
    if (!residual_tiles_setup(rt, p, begin, end)) return LORA_EINVAL;
    ReduceRecord *records = nullptr;
    if (int rc = ensure_records(plan, &records)) return rc;
    const hipError_t e = launch_residual(p, rt, d_in, static_cast<const double *>(d_f), records, s);
    if (e != hipSuccess) {
        set_last_error("residual kernel launch", e);
        return LORA_EHIP;
    }
    ReduceRecord rec;
    LORA_HIP_TRY(hipMemcpyAsync(&rec, records + kReduceMaxGroups, sizeof rec, hipMemcpyDeviceToHost, s));
    LORA_HIP_TRY(hipStreamSynchronize(s));
    long long count = end - begin;
    for (int d = 1; d < p.ndim; ++d) count *= p.dims[d];
    const bool any = rec.f[0] >= 0.0;
    *out = {any ? rec.f[0] : 0.0, rec.f[1], rec.f[2], any ? rec.i[0] : -1, count, rec.i[1]};
    return LORA_OK;
}

int no_residual_kernel() {
    set_last_error_text("this plan has no fused residual kernel (odd innermost extent, or the 2D matrix-pipe variant)");
    return LORA_EUNSUPPORTED;
}

}  // namespace

bool bad_until_schedule(const lora_until *u) { return u->check_every < 2 || u->check_every % 2 || u->max_times < 0; }
bool bad_until(const lora_until *u) {
    if (bad_until_schedule(u) || (u->norm != LORA_NORM_MAX && u->norm != LORA_NORM_RMS)) return true;
    return !(u->tol >= 0.0) || !(u->rtol >= 0.0);  // (a NaN fails both)
}

bool until_decide(const lora_until *u, lora_until_result *r) {
    r->checks += 1;
    r->residual = u->norm == LORA_NORM_RMS ? std::sqrt(r->last.sum_sq / (double) r->last.count) : r->last.max_abs;
    if (r->last.nonfinite > 0)
        r->diverged = 1;
    else if (r->residual <= u->tol + u->rtol * r->last.a_abs_max)
        r->converged = 1;
    return r->diverged || r->converged;
}

int admit_reduction(const void *a, const void *b, hipStream_t s) { return admit(a, b, s); }
int reduction_range(const Plan &p, int &begin, int &end) { return resolve_range(p, begin, end); }
int reduction_records(lora_plan *plan, ReduceRecord **out) { return ensure_records(plan, out); }
int residual_whole(lora_plan *plan, const void *d_in, const void *d_f, lora_grid_diff *out, hipStream_t s) {
    return residual_range(plan, d_in, d_f, 0, plan->p.dims[0], out, s);
}
int diff_whole(lora_plan *plan, const void *d_a, const void *d_b, lora_grid_diff *out, hipStream_t s) {
    return diff_range(plan, d_a, d_b, 0, plan->p.dims[0], out, s);
}
int sweep_with_source(const Plan &p, const void *d_f, const void *d_in, void *d_out, hipStream_t s) {
    Plan with_f = p;
    with_f.source = d_f;
    return launch_apps(with_f, {1, 0, p.dims[0]}, d_in, d_out, s);
}
int true_residual(lora_plan *plan, const void *d_u, const void *d_f, void *d_scratch, bool fused, lora_grid_diff *out, hipStream_t s) {
    if (fused) return residual_whole(plan, d_u, d_f, out, s);
    if (int rc = sweep_with_source(plan->p, d_f, d_u, d_scratch, s)) return rc;
    return diff_whole(plan, d_scratch, d_u, out, s);
}

}  // namespace lora

using lora::Plan;

extern "C" {

int lora_plan_stats(lora_plan *plan, const void *d_buf, int begin, int end, lora_grid_stats *out, void *stream) {
    if (!plan || !d_buf || !out) return LORA_EINVAL;
    const int some = lora::resolve_range(plan->p, begin, end);
    if (some < 0) return some;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_buf, d_buf, s)) return rc;
    *out = lora::kEmptyStats;
    if (!some) return LORA_OK;
    lora::ReduceRecord rec;
    if (int rc = lora::reduce_range(plan, d_buf, nullptr, begin, end, rec, out->count, s)) return rc;
    out->min = rec.f[0];
    out->max = rec.f[1];
    out->sum = rec.f[2];
    out->sum_sq = rec.f[3];
    out->nonfinite = rec.i[0];
    // over one set of finite cells the largest magnitude is at the minimum or at the maximum
    out->abs_max = out->nonfinite < out->count ? std::fmax(std::fabs(out->min), std::fabs(out->max)) : 0.0;
    return LORA_OK;
}

int lora_plan_diff(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_diff *out, void *stream) {
    if (!plan || !d_a || !d_b || !out) return LORA_EINVAL;
    const int some = lora::resolve_range(plan->p, begin, end);
    if (some < 0) return some;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_a, d_b, s)) return rc;
    *out = {0.0, 0.0, 0.0, -1, 0, 0};
    if (!some) return LORA_OK;
    return lora::diff_range(plan, d_a, d_b, begin, end, out, s);
}

int lora_plan_dot(lora_plan *plan, const void *d_a, const void *d_b, int begin, int end, lora_grid_dot *out, void *stream) {
    if (!plan || !d_a || !d_b || !out) return LORA_EINVAL;
    const int some = lora::resolve_range(plan->p, begin, end);
    if (some < 0 || begin % lora::region_granularity(plan->p)) return LORA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_a, d_b, s)) return rc;
    *out = {0.0, 0.0, 0, 0};
    if (!some) return LORA_OK;
    return lora::dot_range(plan, d_a, d_b, begin, end, out, s);
}

int lora_plan_residual(lora_plan *plan, const void *d_in, int begin, int end, lora_grid_diff *out, void *stream) {
    if (!plan || !d_in || !out) return LORA_EINVAL;
    const int some = lora::resolve_range(plan->p, begin, end);
    if (some < 0 || begin % lora::region_granularity(plan->p)) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_in, d_in)) return rc;
    if (!lora::has_fused_residual(plan->p)) return lora::no_residual_kernel();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_in, d_in, s)) return rc;
    *out = {0.0, 0.0, 0.0, -1, 0, 0};
    if (!some) return LORA_OK;
    return lora::residual_range(plan, d_in, nullptr, begin, end, out, s);
}

int lora_plan_residual_src(lora_plan *plan, const void *d_in, const void *d_f, int begin, int end, lora_grid_diff *out, void *stream) {
    if (!d_f) return lora_plan_residual(plan, d_in, begin, end, out, stream);
    if (!plan || !d_in || !out) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::resolve_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p) || d_f == d_in) return LORA_EINVAL;
    if (int rc = lora::check_buffers(d_in, d_f)) return rc;
    // no kernel, bf16, a plan with a source -- all LORA_EUNSUPPORTED.  A plan with a source also reads "fused_residual" 0; it
    // gets the text that names the cause
    if (!p.source && !lora::has_fused_residual(p)) return lora::no_residual_kernel();
    if (p.dtype == LORA_BF16) {
        lora::set_last_error_text("a source is fp64: bf16 plans have no fused residual with a source");
        return LORA_EUNSUPPORTED;
    }
    if (p.source) {
        lora::set_last_error_text("a plan with a source has no fused residual kernel: the source of lora_plan_residual_src is a call argument");
        return LORA_EUNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_in, d_f, s)) return rc;
    *out = {0.0, 0.0, 0.0, -1, 0, 0};
    if (!some) return LORA_OK;
    return lora::residual_range(plan, d_in, d_f, begin, end, out, s);
}

// Test support (no device): which cells the workgroups of lora_plan_residual's launch reduce -- residual_tiles.h replayed.
int lora_debug_residual_cover(const lora_plan *plan, int begin, int end, int *cover, int *workgroups) {
    if (!plan || !cover) return LORA_EINVAL;
    const Plan &p = plan->p;
    const int some = lora::resolve_range(p, begin, end);
    if (some < 0 || begin % lora::region_granularity(p)) return LORA_EINVAL;
    if (!lora::has_fused_residual(p)) return lora::no_residual_kernel();
    if (workgroups) *workgroups = 0;
    lora::ResidualTiles rt;
    if (!some || !lora::residual_tiles_setup(rt, p, begin, end)) return LORA_OK;
    const int *hw = lora::interior_pads(p.ndim);
    int halo[3] = {0, 0, 0};
    long P[3] = {1, 1, 1};
    for (int d = 3 - p.ndim; d < 3; ++d) {
        halo[d] = hw[d - (3 - p.ndim)];
        P[d] = rt.dims[d] + 2L * halo[d];
    }
    for (int g = 0; g < rt.groups; ++g)
        for (long t = g; t < rt.tiles; t += rt.groups) {
            int o[3], n[3];
            lora::residual_tile_box(rt, t, o, n);
            for (int z = o[0]; z < o[0] + n[0]; ++z)
                for (int y = o[1]; y < o[1] + n[1]; ++y)
                    for (int x = o[2]; x < o[2] + n[2]; ++x) cover[((z + halo[0]) * P[1] + (y + halo[1])) * P[2] + (x + halo[2])] += 1;
        }
    if (workgroups) *workgroups = rt.groups;
    return LORA_OK;
}

void lora_grid_stats_merge(lora_grid_stats *into, const lora_grid_stats *part) {
    if (!into || !part) return;
    into->min = part->min < into->min ? part->min : into->min;
    into->max = part->max > into->max ? part->max : into->max;
    into->abs_max = part->abs_max > into->abs_max ? part->abs_max : into->abs_max;
    into->sum += part->sum;
    into->sum_sq += part->sum_sq;
    into->count += part->count;
    into->nonfinite += part->nonfinite;
}

int lora_plan_run_until(lora_plan *plan, void *d_buf0, void *d_buf1, const lora_until *u, lora_until_result *r, void *stream) {
    if (!plan || !d_buf0 || !d_buf1 || !u || !r || d_buf0 == d_buf1 || lora::bad_until(u)) return LORA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lora::admit(d_buf0, d_buf1, s)) return rc;
    const Plan &p = plan->p;
    *r = {0, 0, 0, 0, HUGE_VAL, {0.0, 0.0, 0.0, -1, 0, 0}};
    // under the max norm every deciding field of the fused residual is bit for bit the two-pass probe's; sum_sq -- the RMS
    // norm's -- is summed in another order there, so that norm keeps the two passes
    const bool fused = u->norm == LORA_NORM_MAX && lora::has_fused_residual(p);
    while (r->times_done + u->check_every <= u->max_times) {
        // an even run: the level is back in d_buf0, both halos as a fresh run expects them
        if (int rc = lora_plan_run(plan, d_buf0, d_buf1, u->check_every, stream)) return rc;
        r->times_done += u->check_every;
        // the probe: one raw sweep's change -- reduced inside the sweep where the plan has that kernel, else the sweep into the
        // buffer whose interior a run leaves unspecified anyway and the difference of the two
        if (p.boundary == LORA_BC_PERIODIC)
            if (int rc = lora_plan_halo(plan, d_buf0, nullptr, LORA_HALO_WRAP, stream)) return rc;
        if (fused) {
            if (int rc = lora::residual_range(plan, d_buf0, nullptr, 0, p.dims[0], &r->last, s)) return rc;
        } else {
            if (int rc = lora_plan_step(plan, d_buf0, d_buf1, stream)) return rc;
            if (int rc = lora::diff_range(plan, d_buf1, d_buf0, 0, p.dims[0], &r->last, s)) return rc;
        }
        if (lora::until_decide(u, r)) break;
    }
    return LORA_OK;
}

int lora_run_host_until(int shape, int dtype, const void *in, void *out, const double *params, const int *dims, const lora_until *u,
                        lora_until_result *r, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || !u || !r || lora::bad_until_schedule(u)) return LORA_EINVAL;  // (the rest of `u`: lora_plan_run_until)
    lora::HostRun g;
    int rc = g.open(shape, dtype, dims, params);
    if (rc != LORA_OK) return rc;
    if (dtype == LORA_BF16)
        if (int src_rc = lora::default_source_refused("a bf16 run")) return src_rc;
    lora_plan *plan = g.plan;
    const size_t bytes = g.bytes;
    LORA_HIP_TRY(g.alloc(2));
    LORA_HIP_TRY(hipMemcpy(g.b[0], in, bytes, hipMemcpyHostToDevice));  // whole padded input, halo included
    LORA_HIP_TRY(hipMemset(g.b[1], 0, bytes));
    if (int src_rc = lora::attach_default_source(plan, bytes, &g.src)) return src_rc;  // the thread's default source, beside the grid
    LORA_HIP_TRY(g.stream());
    (void) lora_plan_prepare_run(plan, u->check_every);
    LORA_HIP_TRY(hipDeviceSynchronize());

    g.tic();
    rc = lora_plan_run_until(plan, g.b[0], g.b[1], u, r, g.s);
    if (rc != LORA_OK) return rc;
    LORA_HIP_TRY(hipStreamSynchronize(g.s));
    g.toc();  // the sweeps and their checks

    // 1D copies all but the last element (1d/gpu_1r.cu:134); the level is in buffer 0 (times_done is even)
    LORA_HIP_TRY(hipMemcpy(out, g.b[0], plan->p.ndim == 1 ? bytes - g.esize : bytes, hipMemcpyDeviceToHost));
    return g.finish(r->times_done, plan->p.source ? 3.0 : 2.0, plan->p.steps_per_launch, quiet, info);  // a source is one more read
}

}  // extern "C"
