// capi.cpp -- implementation of the C ABI in include/lorastencil.h: the launch dispatcher, the time-step driver, the holder of
// the grids a plan owns (lora::DeviceGrid) and the plain host-buffer operator that stands in for the reference's gpu_*()
// functions (its skeleton: hostrun.cpp).  (What a plan is and resolves to: plan.cpp.)
//
// Reference behaviour followed (file:line under /root/reference/src/):
//   driver: buf0 <- padded input, buf1 <- 0, `times` launches ping-ponging, result = buf[times % 2]
//           (1d/gpu_1r.cu:103-134, 2d/gpu.cu:392-421, :450-479, :525-554, 3d/gpu_star.cu:158-192,
//            3d/gpu_box.cu:190-223)
// There is deliberately no CPU fallback: without a HIP device every compute entry point fails.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "spans.h"

namespace lora {

static thread_local std::string g_last_error;
static thread_local lora_run_info g_last_info = {};

void set_last_error(const char *what, hipError_t e) {
    g_last_error = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
}

void set_last_error_text(const char *text) { g_last_error = text ? text : ""; }
void set_last_run_info(const lora_run_info &info) { g_last_info = info; }

#define LORA_HIP_TRY(expr)                      \
    do {                                        \
        hipError_t e__ = (expr);                \
        if (e__ != hipSuccess) {                \
            lora::set_last_error(#expr, e__);   \
            return LORA_EHIP;                   \
        }                                       \
    } while (0)

int check_buffers(const void *a, const void *b) {
    if (!a || !b) return LORA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(b) & 15)) {
        g_last_error = "device buffers must be 16-byte aligned";
        return LORA_EUNSUPPORTED;
    }
    return LORA_OK;
}

// Which launches a plan has.  One application: every plan.  lora_plan_step2's two: 2D direct-variant plans whose fused
// kernels apply (odd innermost extents: the row-streaming kernel) and 3D plans with a fused kernel, whatever their depth.
// Otherwise the plan's own kernel family at any depth up to `depth` that it has: 1D the powers of two, 2D the even ones
// (row-streaming kernel 4 / 2, workgroup-row kernel 6 / 4 / 2), 3D the plan's own and 2.
static bool has_apps(const Plan &p, int napps, int depth, bool step2) {
    // a plan with a source has the source kernels only: one application, and two where it resolved to two
    if (p.source) return step2 ? p.steps_per_launch == 2 : (napps == 1 || (napps == 2 && depth >= 2 && p.steps_per_launch == 2));
    if (step2) return p.ndim != 1 && has_fused_kernels(p);  // (1D has no two-application entry of this kind)
    if (napps == 1) return true;
    if (napps < 2 || napps > depth) return false;
    if (p.ndim == 1) return (napps & (napps - 1)) == 0;
    if (p.ndim == 2) return napps % 2 == 0;
    return napps == 2 || napps == depth;
}

bool has_depth(const Plan &p, int napps) { return has_apps(p, napps, p.steps_per_launch, false); }

int launch_apps(const Plan &p, const Apps &a, const void *d_in, void *d_out, hipStream_t s) {
    const int n = a.napps, b = a.begin, e = a.end;
    if (!has_apps(p, n, a.depth ? a.depth : p.steps_per_launch, a.step2)) return LORA_EUNSUPPORTED;
    if (int rc = check_buffers(d_in, d_out)) return rc;
    const int g = region_granularity(p);
    auto bad = [&](int begin, int end) { return begin < 0 || end > p.dims[0] || begin > end || begin % g != 0; };
    if (d_in == d_out || bad(b, e) || bad(a.begin2, a.end2)) return LORA_EINVAL;
    if (p.source && p.source == d_out) return LORA_EINVAL;  // f is read while d_out is written
    const double *in = static_cast<const double *>(d_in);
    double *out = static_cast<double *>(d_out);
    const bool bf16 = p.dtype == LORA_BF16;
    hipError_t err;
    if (p.source)  // (fp64, never the 2D matrix-pipe variant: lora_plan_set_source)
        err = n == 1 ? launch_source(p, in, out, b, e, s) : launch_source2(p, in, out, b, e, s);
    else if (n == 1 && bf16)
        err = launch_3d_bf16(p, d_in, d_out, b, e, s);
    else if (n == 1 && p.generic)
        err = p.ndim == 2 ? launch_2d_generic(p, in, out, b, e, s) : launch_3d_generic(p, in, out, b, e, s);
    else if (n == 1)
        err = p.ndim == 1   ? launch_1d(p, in, out, b, e, s)
              : p.ndim == 3 ? launch_3d(p, in, out, b, e, s)
              : p.variant == LORA_VARIANT_MFMA ? launch_2d_mfma(p, in, out, b, e, s)
                                               : launch_2d_direct(p, in, out, b, e, s);
    else if (p.ndim == 1)
        err = launch_1d_fused(p, n, in, out, b, e, s);
    else if (p.ndim == 2)
        err = (p.wg_active && !a.step2) ? launch_2d_wg(p, n, in, out, b, e, s)
              : p.stream2               ? launch_2d_stream(p, n, in, out, b, e, s)
                                        : launch_2d_fused2(p, in, out, b, e, s);
    else if (n == 3)  // an even global step by default: level 1 has the zero halo, level 2 the source's
        err = launch_3d_stream(p, 3, in, out, static_cast<const double *>(a.halo ? a.halo : d_in), a.parity, b, e, s);
    else if (p.lanes3_active && n == 2 && a.begin2 == a.end2 && !bf16 && !p.generic && p.stream3 != 0 && e - b >= 128)
        // Two sweeps move the same bytes as four, and at that the plane-streaming kernel is the faster of the two (star3d1r
        // 512^3: 475 against 551 us; box3d1r 768^3: 1651 against 1893; tools/tail_time.py) -- same taps in the same order,
        // same bits.  Deep regions of even-extent fp64 grids take it; the rest (thin regions, odd extents, bf16, two ranges)
        // stays with the register-resident kernels.
        err = launch_3d_stream(p, 2, in, out, in, 0, b, e, s);
    else if (p.lanes3_active)
        err = bf16 ? launch_3d_bf16_lanes(p, n, d_in, d_out, b, e, s, a.begin2, a.end2)
                   : launch_3d_lanes(p, n, in, out, b, e, s, a.begin2, a.end2);
    else if (bf16)
        err = p.variant == LORA_VARIANT_MFMA ? launch_3d_bf16_mfma2(p, d_in, d_out, b, e, s)
                                             : launch_3d_bf16_fused2(p, d_in, d_out, b, e, s);
    else
        err = p.stream3_active ? launch_3d_stream(p, 2, in, out, in, 0, b, e, s) : launch_3d_fused2(p, in, out, b, e, s);
    if (err != hipSuccess) {
        set_last_error(n == 1 ? "kernel launch" : "fused kernel launch", err);
        return p.source && lora_device_count() <= 0 ? no_device() : LORA_EHIP;
    }
    return LORA_OK;
}

static thread_local const double *g_default_source = nullptr;

int default_source_refused(const char *who) {
    if (!g_default_source) return LORA_OK;
    g_last_error = std::string(who) + " takes no source (lora_set_default_source)";
    return LORA_EUNSUPPORTED;
}

// The thread's default source uploaded beside the grid and set on the plan of a host-buffer operator (fp64).
int attach_default_source(lora_plan *plan, size_t bytes, void **d_source) {
    if (!g_default_source) return LORA_OK;
    if (hipMalloc(d_source, bytes) != hipSuccess) {
        (void) hipGetLastError();
        *d_source = nullptr;
        return LORA_ENOMEM;
    }
    const hipError_t e = hipMemcpy(*d_source, g_default_source, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_last_error("source upload", e);
        return LORA_EHIP;
    }
    return lora_plan_set_source(plan, *d_source);
}

bool DeviceGrid::ready(size_t want) const {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    return ptr && bytes == want && device == dev;
}

bool DeviceGrid::ensure(size_t want) {
    if (ready(want)) return true;
    release();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipMalloc(&ptr, want) != hipSuccess) {
        (void) hipGetLastError();
        ptr = nullptr;
        return false;
    }
    bytes = want;
    device = dev;
    return true;
}

void DeviceGrid::release() {
    if (ptr) (void) hipFree(ptr);
    *this = DeviceGrid();
}

}  // namespace lora

using lora::g_last_error;
using lora::Plan;

extern "C" {

const char *lora_strerror(int status) {
    switch (status) {
        case LORA_OK:
            return "ok";
        case LORA_EINVAL:
            return "invalid argument";
        case LORA_EUNSUPPORTED:
            return "unsupported size or alignment";
        case LORA_EHIP:
            return "HIP runtime error";
        case LORA_ENOMEM:
            return "out of memory";
        case LORA_ENODEVICE:
            return "no HIP device (this engine has no CPU fallback)";
        default:
            return "unknown status";
    }
}

const char *lora_last_error(void) { return g_last_error.c_str(); }

int lora_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void) hipGetLastError();
        return 0;
    }
    return n;
}

static void torus_drop(lora_plan *plan);

// The public launch entries: each one launch of the dispatcher (lora::launch_apps) at its depth.
int lora_plan_step_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora::launch_apps(plan->p, {1, begin, end}, d_in, d_out, static_cast<hipStream_t>(stream));
}

int lora_plan_step(lora_plan *plan, const void *d_in, void *d_out, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step_region(plan, d_in, d_out, 0, plan->p.dims[0], stream);
}

int lora_plan_step2_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream) {
    if (!plan) return LORA_EINVAL;
    lora::Apps a{2, begin, end};
    a.step2 = true;
    return lora::launch_apps(plan->p, a, d_in, d_out, static_cast<hipStream_t>(stream));
}

int lora_copy_block_f64(void *d_dst, long dst_ld, const void *d_src, long src_ld, long rows, long cols, void *stream) {
    if (!d_dst || !d_src || rows < 0 || cols < 0 || dst_ld < cols || src_ld < cols) return LORA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(d_src)) & 7) return LORA_EUNSUPPORTED;
    const hipError_t e = lora::launch_copy_block(static_cast<double *>(d_dst), dst_ld, static_cast<const double *>(d_src), src_ld,
                                                 rows, cols, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        lora::set_last_error("block copy kernel launch", e);
        return LORA_EHIP;
    }
    return LORA_OK;
}

int lora_plan_halo(lora_plan *plan, void *d_dst, const void *d_src, int mode, void *stream) {
    if (!plan || !d_dst) return LORA_EINVAL;
    if (mode != LORA_HALO_COPY && mode != LORA_HALO_ZERO && mode != LORA_HALO_WRAP) return LORA_EINVAL;
    if (mode == LORA_HALO_COPY && (!d_src || d_src == d_dst)) return LORA_EINVAL;
    const Plan &p = plan->p;
    if (mode == LORA_HALO_WRAP) {
        static const int h1[1] = {4}, h2[2] = {4, 4}, h3[3] = {1, 2, 4};
        const int *h = p.ndim == 1 ? h1 : (p.ndim == 2 ? h2 : h3);
        for (int d = 0; d < p.ndim; ++d)
            if (p.dims[d] < h[d]) return LORA_EUNSUPPORTED;  // the wrap source would be a halo cell itself
    }
    const hipError_t e = lora::launch_halo(p, d_dst, d_src, mode, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        lora::set_last_error("halo kernel launch", e);
        return LORA_EHIP;
    }
    return LORA_OK;
}

int lora_plan_step2(lora_plan *plan, const void *d_in, void *d_out, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_step2_region(plan, d_in, d_out, 0, plan->p.dims[0], stream);
}

int lora_plan_stepk_region(lora_plan *plan, const void *d_in, void *d_out, int begin, int end, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_stepn_region(plan, plan->p.steps_per_launch, d_in, d_out, begin, end, stream);
}

int lora_plan_stepk(lora_plan *plan, const void *d_in, void *d_out, void *stream) {
    if (!plan) return LORA_EINVAL;
    return lora_plan_stepk_region(plan, d_in, d_out, 0, plan->p.dims[0], stream);
}

int lora_plan_stepn_region(lora_plan *plan, int napps, const void *d_in, void *d_out, int begin, int end, void *stream) {
    if (!plan || napps < 1) return LORA_EINVAL;
    return lora::launch_apps(plan->p, {napps, begin, end}, d_in, d_out, static_cast<hipStream_t>(stream));
}

static void drop_graph(lora_plan *plan);

static bool ensure_scratch(lora_plan *plan) {
    const size_t bytes = lora_plan_padded_bytes(plan);
    if (plan->scratch.ready(bytes)) return true;
    drop_graph(plan);  // a captured run holds the old grid's address
    // (not zeroed: every run copies buffer 0's ring into it -- there are no pads beyond the ring -- and a launch writes its whole
    // interior, both on the run's stream, before the next launch reads it)
    return plan->scratch.ensure(bytes);
}

// 1D runs with the automatic launch depth fuse more applications per launch the longer the run is: 8 is the plan's
// own depth (what lora_plan_stepk and the slab drivers use), 16 / 32 pay from 32 / 64 sweeps on (2^20 points: 840 ->
// 999 -> 1066 GStencils/s per launch, 2^28: 1600 -> 1915 -> 1987; tools/k1d.sh) while short runs keep enough fused
// launches.  Every other plan runs at its own depth.
static int run_depth(const Plan &p, int times) {
    if (p.ndim == 1 && p.steps_per_launch_req == 0 && p.steps_per_launch == 8 && p.boundary != LORA_BC_PERIODIC)
        return times >= 64 ? 32 : (times >= 32 ? 16 : 8);
    return p.steps_per_launch;
}

// How lora_plan_run cuts a run of `times` sweeps at depth K into launches: the depths of its fused launches in order (the
// full-depth ones first, then the shallower ones), the rest of the run single sweeps.
struct Schedule {
    std::vector<int> depths;
    bool natural = false;  // three-application 3D form: launch k reads buffer k mod 2 (see run_launches)
    bool scratch = false;  // an odd number of launches: the last two hops go through the plan's scratch grid
};

static Schedule run_schedule(const Plan &p, int times, int K, bool scratch_ok) {
    Schedule sc;
    std::vector<int> &d = sc.depths;
    const bool can_fuse = p.boundary != LORA_BC_PERIODIC && K >= 2 && lora::has_fused_kernels(p);
    if (!can_fuse) return sc;
    if (p.ndim == 3 && K == 3) {
        // What three-application launches leave (1 or 2 sweeps) would be single sweeps at a third of the rate.  When the
        // launches before them end at an even step in buffer 0, two of them are traded for TWO-application launches of
        // the same kernel instead: 3 a + 1 = 3 (a - 1) + 2 + 2, 3 a + 2 = 3 (a - 2) + 4 x 2 (50 sweeps = 14 x 3 + 4 x 2).
        sc.natural = true;
        int nk = times / 3, n2 = 0;
        if (times % 3 == 1 && nk >= 1 && (nk - 1) % 2 == 0) {
            nk -= 1;
            n2 = 2;
        } else if (times % 3 == 2 && nk >= 2 && (nk - 2) % 2 == 0) {
            nk -= 2;
            n2 = 4;
        }
        d.assign(nk, 3);
        d.insert(d.end(), n2, 2);
        return sc;
    }
    // What the full-depth launches leave is covered by shallower ones, so that at most one single sweep remains: 1D K / 2,
    // K / 4, ... 2 applications (100 sweeps at depth 32 = 32 + 32 + 32 + 4); 2D and 3D four and / or two (100 sweeps at
    // depth 6 = 16 x 6 + 4)
    const int nk = times / K;
    int r = times % K;
    d.assign(nk, K);
    if (K == 6 && r >= 2 && r < 4 && nk >= 1) {
        // 6 + 2 as 4 + 4: a two-application launch moves the whole grid for two sweeps (star2d1r 16384^2, us per
        // launch of the workgroup-row kernel at 6 / 4 / 2 applications: 1194 / 944 / 885)
        d.back() = 4;
        d.push_back(4);
        r -= 2;
    }
    for (int t = p.ndim == 1 ? K / 2 : 4; t >= 2; t = p.ndim == 1 ? t / 2 : t - 2)
        if (t < K && r >= t) {
            d.push_back(t);
            r -= t;
        }
    const int n = (int) d.size();
    if (n % 2 == 0) return sc;
    if (n >= 3 && scratch_ok && p.use_scratch != 0) {
        sc.scratch = true;
        return sc;
    }
    // no scratch grid: an even number of launches -- 2D / 3D: one full-depth launch becomes two shallower ones (6 = 4 + 2,
    // 4 = 2 + 2); else the last launch becomes two of half its depth, or (two applications) single sweeps
    int full = 0;  // the full-depth launches
    while (full < n && d[full] == K) ++full;
    if (p.ndim != 1 && full >= 1 && K >= 4) {
        d[full - 1] = K == 6 ? 4 : 2;
        d.insert(d.begin() + full, 2);
    } else if (d.back() >= 4) {
        d.back() /= 2;
        d.push_back(d.back());
    } else {
        d.pop_back();
    }
    return sc;
}

// The run's schedule, its scratch grid allocated now if it asks for one (`allocate`), else taken only if it is there.
static Schedule plan_schedule(lora_plan *plan, int times, bool allocate) {
    const int K = run_depth(plan->p, times);
    Schedule sc = run_schedule(plan->p, times, K, true);
    if (sc.scratch && !(allocate ? ensure_scratch(plan) : plan->scratch.ready(lora_plan_padded_bytes(plan))))
        sc = run_schedule(plan->p, times, K, false);
    return sc;
}

struct RunMarks {  // lora_plan_run_profiled: events around the fused and the single-sweep segment
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start | K-launches | 2-launches | singles
    int fused_launches = 0, two_launches = 0, single_launches = 0;
};

// Test support (no device): the cuts of the register-resident 3D kernels' launches, walked on the host (spans.h: cut3_walk).
// A region of `depth` planes cut into spans (team = 0), team spans as the fp64 kernel launches them (1) or as the bf16
// kernel does (2: column lines with weighted rim rows, the rim columns cut finer), whatever S.
int lora_debug_span_cover(int tiles_x, int tiles_y, int depth, int S, int slots, int team, int *cover, int *workgroups, int *max_steps) {
    if (tiles_x < 1 || tiles_y < 1 || depth < 1 || S < 1 || slots < 1 || !cover) return LORA_EINVAL;
    if (team && tiles_x > slots) return LORA_EUNSUPPORTED;
    constexpr unsigned kTeams2 = lora::bf16_lanes_rules(4).decodes;
    lora::Cut3 c{};
    c.z_end = depth;
    c.tiles_x = tiles_x;
    c.tiles_y = tiles_y;
    const long wgs = team ? lora::cut3_set_teams(c, depth, S, slots, team == 2 ? kTeams2 : 0u) : lora::cut3_set_spans(c, depth, S, slots);
    if (wgs <= 0) return LORA_EUNSUPPORTED;
    if (workgroups) *workgroups = (int) wgs;
    const bool ok = team == 2 ? lora::cut3_walk<kTeams2>(c, S, wgs, depth, cover, max_steps) : lora::cut3_walk<0u>(c, S, wgs, depth, cover, max_steps);
    return ok ? LORA_OK : LORA_EHIP;  // (a segment out of range: a bug)
}

// Test support (no device): the strips and row chunks the workgroup-row 2D kernel's launcher chooses for K applications over
// `rows` rows of the plan's grid (its wg_rows / wg_edge_pct options included) on cus x per_cu resident workgroups.
int lora_debug_wg_layout(lora_plan *plan, int K, int rows, int cus, int per_cu, int *out) {
    if (!plan || !out) return LORA_EINVAL;
    if (plan->p.ndim != 2) return LORA_EUNSUPPORTED;
    return lora::wg_layout_debug(plan->p, K, rows, cus, per_cu, out) ? LORA_OK : LORA_EINVAL;
}

// The cut the fp64 (kernel = 0) or bf16 (1) register-resident kernel's launcher chooses for K applications over planes
// [begin, end) and [begin2, end2) of h, walked the same way; *kind = the layout (enum lora_cut_kind).
int lora_debug_cut_cover(int kernel, int K, int tiles_x, int tiles_y, int h, int begin, int end, int begin2, int end2, int slots,
                         int fused_z_chunk, int spans3, int *cover, int *workgroups, int *max_steps, int *kind) {
    static_assert(LORA_CUT_FIXED == lora::CUT3_KIND_FIXED && LORA_CUT_TEAMS_FINER == lora::CUT3_KIND_TEAMS_FINER, "one list of layouts");
    if ((kernel != 0 && kernel != 1) || (K != 2 && K != 4) || tiles_x < 1 || tiles_y < 1 || slots < 1 || !cover) return LORA_EINVAL;
    if (begin < 0 || end > h || end < begin || (end2 > begin2 && (begin2 < 0 || end2 > h)) || (end == begin && end2 <= begin2)) return LORA_EINVAL;
    const lora::CutRules R = kernel ? lora::bf16_lanes_rules(K) : lora::lanes3_rules(K);
    // (the largest grid of these tiles: 120 output columns and 4 NW - 2 K rows a tile, NW = 8 / 16 waves)
    const long plane = ((long) tiles_y * ((kernel ? 64 : 32) - 2 * K) + 4) * (120L * tiles_x + 8);
    lora::Cut3 c;
    const long wgs = lora::cut3_plan(R, tiles_x, tiles_y, plane, begin, end, begin2, end2, slots, fused_z_chunk, spans3, c, kind);
    if (wgs <= 0) return LORA_EUNSUPPORTED;
    if (workgroups) *workgroups = (int) wgs;
    const bool ok = kernel ? lora::cut3_walk<lora::bf16_lanes_rules(4).decodes>(c, R.S, wgs, h, cover, max_steps)
                           : lora::cut3_walk<lora::lanes3_rules(4).decodes>(c, R.S, wgs, h, cover, max_steps);
    return ok ? LORA_OK : LORA_EHIP;
}

// Two ranges of planes / rows in one call: the two end regions a slab or block driver sweeps behind its deferred wait.
// The register-resident 3D kernels take both in ONE launch (an end region of 4 planes is 13 steps of pipeline whatever it
// computes: 32 us each at 64 x 512^2, tools/region_split_time.py); every other kernel family gets two launches.
int lora_plan_stepn_region2(lora_plan *plan, int napps, const void *d_in, void *d_out, int begin0, int end0, int begin1, int end1,
                            void *stream) {
    if (!plan || napps < 1) return LORA_EINVAL;
    const bool apart = end0 <= begin1 || end1 <= begin0;
    if (plan->p.lanes3_active && (napps == 4 || napps == 2) && end0 > begin0 && end1 > begin1 && apart)
        return lora::launch_apps(plan->p, {napps, begin0, end0, begin1, end1}, d_in, d_out, static_cast<hipStream_t>(stream));
    if (end0 > begin0)
        if (int rc = lora_plan_stepn_region(plan, napps, d_in, d_out, begin0, end0, stream)) return rc;
    return end1 > begin1 ? lora_plan_stepn_region(plan, napps, d_in, d_out, begin1, end1, stream) : LORA_OK;
}

// ---- the periodic option in fused launches: the torus by ghost zones ---------------------------------------------
// A fused launch cannot wrap the halo of its intermediate levels, so rounds 1 - 3 ran periodic grids one sweep at a time
// behind a halo wrap each.  What the slab drivers do for a cut serves for the torus too: extend the grid by a ghost zone
// of radius x applications-per-launch cells on EVERY side, fill it with the periodic images of the interior, and run the
// ordinary fused kernels on the extended grid -- ghost cells are plain interior cells of that problem, computed by the same
// arithmetic on the same values as their originals, so after a launch of K applications everything but the outermost
// radius x K cells is right, the true interior included; wrap the ring again, launch again.  Costs two more buffers and,
// per launch, a wrap of the ring (surface work) and the sweeps' share of the ghost cells (16384^2, K = 6: 0.4 %).
// Bit-identical to wrap + single sweep wherever the fused kernels are bit-identical to single sweeps.
static int torus_radius(int nd) { return nd == 1 ? 4 : (nd == 2 ? 3 : 1); }
static const int *torus_pads(int nd) {
    static const int h1[1] = {4}, h2[2] = {4, 4}, h3[3] = {1, 2, 4};  // (kernels_halo.hip: launch_halo)
    return nd == 1 ? h1 : (nd == 2 ? h2 : h3);
}

static void torus_drop(lora_plan *plan) {
    if (plan->torus) lora_plan_destroy(plan->torus);
    plan->torus = nullptr;
    for (lora::DeviceGrid &b : plan->torus_buf) b.release();
    plan->torus_tried = false;
}

// the extended plan and its buffers, built on first need; nullptr: this plan's periodic runs stay single sweeps
static lora_plan *torus_prepare(lora_plan *plan) {
    Plan &p = plan->p;
    if (p.source) return nullptr;  // the extended plan is built from shape and taps: it would drop the source
    if (p.boundary != LORA_BC_PERIODIC || p.torus == 0 || p.steps_per_launch_req == 1 || p.variant != LORA_VARIANT_DIRECT) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void) hipGetLastError();
        return nullptr;
    }
    if (plan->torus_tried && plan->torus_epoch == p.epoch && plan->torus_device == dev) return plan->torus;
    if (plan->capturing) return nullptr;  // (no allocation inside a stream capture; lora_plan_run prepares before it)
    torus_drop(plan);
    plan->torus_tried = true;
    plan->torus_epoch = p.epoch;
    plan->torus_device = dev;
    const int nd = p.ndim, r = torus_radius(nd), kmax = lora::max_depth(nd);
    const int *pad = torus_pads(nd);
    int ext[3] = {0, 0, 0};
    for (int d = 0; d < nd; ++d) {
        int g = r * kmax;
        if (d == nd - 1 && p.dtype == LORA_BF16) g = (g + 3) / 4 * 4;  // rows stay whole 8-byte units, a multiple of 8 cells
        if (g + pad[d] > p.dims[d]) return nullptr;  // an image of an image: grids this small keep the single sweeps
        plan->torus_ghost[d] = g;
        ext[d] = p.dims[d] + 2 * g;
    }
    lora_plan *tp = nullptr;
    if (lora_plan_create(&tp, p.shape, p.dtype, ext, nullptr) != LORA_OK) return nullptr;
    bool ok = lora_plan_set_boundary(tp, LORA_BC_REFERENCE) == LORA_OK && lora_plan_set_weights(tp, p.w, p.ntaps) == LORA_OK;
    if (ok && p.steps_per_launch_req > 1) (void) lora_plan_set_option(tp, "steps_per_launch", p.steps_per_launch_req);
    ok = ok && tp->p.steps_per_launch >= 2 && tp->p.steps_per_launch <= kmax;
    const size_t bytes = ok ? lora_plan_padded_bytes(tp) : 0;
    ok = ok && plan->torus_buf[0].ensure(bytes) && plan->torus_buf[1].ensure(bytes);
    if (!ok) {
        lora_plan_destroy(tp);
        for (lora::DeviceGrid &b : plan->torus_buf) b.release();
        return nullptr;
    }
    plan->torus = tp;
    return tp;
}

constexpr int kTorusNotTaken = -1000;

static int run_torus(lora_plan *plan, void *d_buf0, void *d_buf1, int times, hipStream_t s, RunMarks *marks) {
    if (times < 2) return kTorusNotTaken;
    lora_plan *tp = torus_prepare(plan);
    if (!tp) return kTorusNotTaken;
    const Plan &p = plan->p;
    const int nd = p.ndim, K = tp->p.steps_per_launch;
    const int *pad = torus_pads(nd);
    int ring[3] = {0, 0, 0};
    for (int d = 0; d < nd; ++d) ring[d] = pad[d] + plan->torus_ghost[d];
    void *buf[2] = {d_buf0, d_buf1};
    void *E[2] = {plan->torus_buf[0].ptr, plan->torus_buf[1].ptr};
    // level 0: the interior into the extended grid's middle, its images into everything around it
    if (int rc = lora::hip_status(lora::launch_copy_interior(p.dtype, nd, p.dims, E[0], ring, buf[0], pad, s), "torus: copy in")) return rc;
    if (int rc = lora::hip_status(lora::launch_ring_wrap(p.dtype, nd, p.dims, ring, E[0], s), "torus: wrap")) return rc;
    int cur = 0, left = times;
    while (left > 0) {
        int d = std::min(left, K);
        while (!lora::has_depth(tp->p, d)) --d;  // the deepest launch the extended plan's kernels have
        if (int rc = lora::launch_apps(tp->p, {d, 0, tp->p.dims[0]}, E[cur], E[1 - cur], s)) return rc;
        if (int rc2 = lora::hip_status(lora::launch_ring_wrap(p.dtype, nd, p.dims, ring, E[1 - cur], s), "torus: wrap")) return rc2;
        if (marks) {
            if (d == K)
                ++marks->fused_launches;
            else if (d > 1)
                ++marks->two_launches;
            else
                ++marks->single_launches;
        }
        cur = 1 - cur;
        left -= d;
    }
    if (marks) {
        (void) hipEventRecord(marks->ev[1], s);
        (void) hipEventRecord(marks->ev[2], s);
    }
    // the result: the extended grid's middle back into the caller's buffer, and that buffer's halo = its periodic images
    if (int rc = lora::hip_status(lora::launch_copy_interior(p.dtype, nd, p.dims, buf[times % 2], pad, E[cur], ring, s), "torus: copy out")) return rc;
    const int rc = lora::hip_status(lora::launch_halo(p, buf[times % 2], nullptr, lora::HALO_WRAP, s), "periodic halo");
    if (marks) (void) hipEventRecord(marks->ev[3], s);
    return rc;
}

static int run_launches(lora_plan *plan, void *d_buf0, void *d_buf1, int times, void *stream, RunMarks *marks = nullptr) {
    const Plan &p = plan->p;
    void *buf[2] = {d_buf0, d_buf1};
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto mark = [&](int k) {
        if (marks) (void) hipEventRecord(marks->ev[k], s);
    };
    mark(0);
    if (times == 0) {
        mark(1);
        mark(2);
        mark(3);
        return LORA_OK;
    }
    auto halo = [&](void *dst, const void *src, int mode, const char *what) -> int {
        const hipError_t e = lora::launch_halo(p, dst, src, mode, s);
        if (e != hipSuccess) {
            lora::set_last_error(what, e);
            return LORA_EHIP;
        }
        return LORA_OK;
    };
    if (p.boundary != LORA_BC_REFERENCE) {
        if (int rc = lora::check_buffers(d_buf0, d_buf1)) return rc;
    }

    if (p.boundary == LORA_BC_PERIODIC) {
        // torus: fused launches on a ghost-extended grid where that applies (run_torus); else refresh the source's halo
        // from the opposite interior edges before every sweep, and once more at the end so that the result is a
        // consistent periodic array
        {
            const int rc = run_torus(plan, d_buf0, d_buf1, times, s, marks);
            if (rc != kTorusNotTaken) return rc;
        }
        mark(1);
        mark(2);
        for (int i = 0; i < times; ++i) {
            if (int rc = halo(buf[i % 2], nullptr, lora::HALO_WRAP, "periodic halo")) return rc;
            if (int rc = lora_plan_step(plan, buf[i % 2], buf[(i + 1) % 2], stream)) return rc;
        }
        if (marks) marks->single_launches = times;
        const int rc = halo(buf[times % 2], nullptr, lora::HALO_WRAP, "periodic halo");
        mark(3);
        return rc;
    }

    const bool dirichlet = p.boundary == LORA_BC_DIRICHLET;
    if (dirichlet) {
        // fixed halo: both buffers carry the caller's halo for the whole run
        if (int rc = halo(buf[1], buf[0], lora::HALO_COPY, "halo copy")) return rc;
    }
    // Temporal fusion.  A fused launch reads a buffer whose halo is the level-0 halo and writes another one, so while
    // fused launches run every physical buffer carries buffer 0's halo; the data must end in buffer 0, after which
    // (reference boundary) buffer 1's halo is put back to 0 and the remaining steps are single sweeps -- the result and
    // its halo end up exactly where the step-by-step driver leaves them.  An EVEN number of launches ping-pongs there by
    // itself; an odd number (>= 3) makes its last two hops through a scratch grid owned by the plan (.. -> buffer 1 ->
    // scratch -> buffer 0), which costs memory -- one more grid of 288 GB -- instead of a four-sweep launch replaced by
    // two two-sweep ones (star2d1r 16384^2, 20 sweeps: 6.2 -> 5.5 ms).  With the Dirichlet boundary all halos simply stay.
    // Three applications per launch (3D fp64, the natural form): launch k covers global steps 3 k + 1 .. 3 k + 3, reading
    // buffer k mod 2 and writing the other one -- exactly where the step-by-step driver has these levels, so the launches
    // run on the reference's own buffer state (buffer 0: the caller's halo, buffer 1: zeros; both the caller's under the
    // Dirichlet option): no halo copies, no parity constraint on the number of launches, no scratch grid.  The kernel is
    // told the parity of its first step (which of its inner levels sees which halo).  The two-application launches after
    // them run like every other fused launch: both buffers carry the caller's halo meanwhile.
    const int K = run_depth(p, times);
    const Schedule sc = plan_schedule(plan, times, /*allocate=*/!plan->capturing);
    const int n = (int) sc.depths.size();
    int full = 0, done = 0;
    for (int d : sc.depths) {
        full += d == K;
        done += d;
    }
    void *scratch = sc.scratch ? plan->scratch.ptr : nullptr;
    if (n > 0) {
        if (int rc = lora::check_buffers(d_buf0, d_buf1)) return rc;
        if (!dirichlet)
            if (int rc = sc.natural ? halo(buf[1], nullptr, lora::HALO_ZERO, "halo reset") : halo(buf[1], buf[0], lora::HALO_COPY, "halo copy"))
                return rc;
        if (scratch)
            if (int rc = halo(scratch, buf[0], lora::HALO_COPY, "halo copy")) return rc;
    }
    for (int k = 0; k < n; ++k) {
        if (k == full) {
            mark(1);
            if (sc.natural && !dirichlet)
                if (int rc = halo(buf[1], buf[0], lora::HALO_COPY, "halo copy")) return rc;
        }
        void *src = buf[k % 2], *dst = buf[(k + 1) % 2];
        if (scratch && k == n - 2) dst = scratch;  // k odd: buffer 1 -> scratch
        if (scratch && k == n - 1) {               // k even: scratch -> buffer 0
            src = scratch;
            dst = buf[0];
        }
        lora::Apps a{sc.depths[k], 0, p.dims[0]};
        a.depth = K;
        a.halo = buf[0];
        a.parity = k & 1;
        if (int rc = lora::launch_apps(p, a, src, dst, s)) return rc;
    }
    if (full == n) mark(1);
    if (!dirichlet && n > (sc.natural ? full : 0))
        if (int rc = halo(buf[1], nullptr, lora::HALO_ZERO, "halo reset")) return rc;
    if (marks) {
        marks->fused_launches = full;
        marks->two_launches = n - full;
    }
    mark(2);
    for (int i = done; i < times; ++i) {  // 2d/gpu.cu:544-546
        const int rc = lora_plan_step(plan, buf[i % 2], buf[(i + 1) % 2], stream);
        if (rc != LORA_OK) return rc;
    }
    if (marks) marks->single_launches = times - done;
    mark(3);
    return LORA_OK;
}

static void drop_graph(lora_plan *plan) {
    if (plan->graph_exec) {
        (void) hipGraphExecDestroy(plan->graph_exec);
        plan->graph_exec = nullptr;
    }
    plan->graph_times = -1;
}

// Everything lora_plan_run(times) would allocate on first need, now: the scratch grid of a schedule with an odd number of
// fused launches (a hipMalloc of one more padded grid -- usually a millisecond or two, but on a fresh device
// it has taken 60 ms, INSIDE whatever region the caller was timing: the "four times slower" runs of DESIGN section 7), the
// extended grid's plan and buffers of a periodic run.  Idempotent; lora_plan_run works without it.
int lora_plan_prepare_run(lora_plan *plan, int times) {
    if (!plan || times < 0) return LORA_EINVAL;
    if (plan->p.boundary == LORA_BC_PERIODIC) {
        if (times >= 2) (void) torus_prepare(plan);
        return LORA_OK;
    }
    (void) plan_schedule(plan, times, true);
    return LORA_OK;
}

int lora_plan_run(lora_plan *plan, void *d_buf0, void *d_buf1, int times, void *stream) {
    if (!plan || times < 0) return LORA_EINVAL;
    if (times == 0) return LORA_OK;  // nothing to launch -- and nothing to capture: an empty graph is not worth a cache entry
    const Plan &p = plan->p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Launch-bound runs (small grids, many steps: the reference's 1D size sweeps in ~2 us per step) are captured
    // once into a hipGraph and replayed; big grids gain nothing and are launched directly.  Capture needs a real
    // stream (not the legacy default one) and no capture already in progress; every kernel takes its taps as launch
    // arguments, so none does host-side work at launch.
    bool want = p.use_graph == 1 || (p.use_graph < 0 && times >= 16 && lora_plan_padded_bytes(plan) <= (64u << 20));
    if (want && s == nullptr) want = false;
    if (want) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
            (void) hipGetLastError();
            want = false;
        }
    }
    if (!want) return run_launches(plan, d_buf0, d_buf1, times, stream);

    if (!(plan->graph_exec && plan->graph_buf[0] == d_buf0 && plan->graph_buf[1] == d_buf1 &&
          plan->graph_times == times && plan->graph_epoch == p.epoch)) {
        drop_graph(plan);
        if (int rc = lora::check_buffers(d_buf0, d_buf1)) return rc;
        // a scratch grid, if this run's schedule wants one, is allocated BEFORE the capture (hipMalloc does not belong inside
        // one); while capturing, run_launches only uses a grid that is already there
        (void) plan_schedule(plan, times, true);
        if (p.boundary == LORA_BC_PERIODIC && times >= 2) (void) torus_prepare(plan);  // (likewise: the extended grid's buffers)
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) {
            (void) hipGetLastError();
            return run_launches(plan, d_buf0, d_buf1, times, stream);
        }
        plan->capturing = true;
        const int rc = run_launches(plan, d_buf0, d_buf1, times, stream);
        plan->capturing = false;
        e = hipStreamEndCapture(s, &graph);
        if (rc != LORA_OK || e != hipSuccess || !graph) {
            if (graph) (void) hipGraphDestroy(graph);
            (void) hipGetLastError();
            return rc != LORA_OK ? rc : run_launches(plan, d_buf0, d_buf1, times, stream);
        }
        e = hipGraphInstantiate(&plan->graph_exec, graph, nullptr, nullptr, 0);
        (void) hipGraphDestroy(graph);
        if (e != hipSuccess) {
            plan->graph_exec = nullptr;
            (void) hipGetLastError();
            return run_launches(plan, d_buf0, d_buf1, times, stream);
        }
        plan->graph_buf[0] = d_buf0;
        plan->graph_buf[1] = d_buf1;
        plan->graph_times = times;
        plan->graph_epoch = p.epoch;
    }
    const hipError_t e = hipGraphLaunch(plan->graph_exec, s);
    if (e != hipSuccess) {
        lora::set_last_error("hipGraphLaunch", e);
        return LORA_EHIP;
    }
    return LORA_OK;
}

int lora_plan_run_profiled(lora_plan *plan, void *d_buf0, void *d_buf1, int times, void *stream,
                           lora_run_profile *profile) {
    if (!plan || times < 0 || !profile) return LORA_EINVAL;
    RunMarks marks;
    struct Guard {
        RunMarks &m;
        ~Guard() {
            for (hipEvent_t e : m.ev)
                if (e) (void) hipEventDestroy(e);
        }
    } guard{marks};
    for (hipEvent_t &e : marks.ev) LORA_HIP_TRY(hipEventCreate(&e));
    const int rc = run_launches(plan, d_buf0, d_buf1, times, stream, &marks);
    if (rc != LORA_OK) return rc;
    LORA_HIP_TRY(hipEventSynchronize(marks.ev[3]));
    profile->fused_launches = marks.fused_launches;
    profile->apps_per_fused_launch = marks.fused_launches ? run_depth(plan->p, times) : 1;
    profile->two_launches = marks.two_launches;
    profile->single_launches = marks.single_launches;
    LORA_HIP_TRY(hipEventElapsedTime(&profile->fused_ms, marks.ev[0], marks.ev[1]));
    LORA_HIP_TRY(hipEventElapsedTime(&profile->two_ms, marks.ev[1], marks.ev[2]));
    LORA_HIP_TRY(hipEventElapsedTime(&profile->single_ms, marks.ev[2], marks.ev[3]));
    return LORA_OK;
}

// ---- group A: host-buffer operators (their skeleton: lora::HostRun, hostrun.cpp) -----------------------------------

int lora_run_host(int shape, const double *in, double *out, const double *params, int times, const int *dims,
                  int quiet, lora_run_info *info) {
    return lora_run_host_dtype(shape, LORA_F64, in, out, params, times, dims, quiet, info);
}

const double *lora_set_default_source(const double *padded_host_source) {
    const double *old = lora::g_default_source;
    lora::g_default_source = padded_host_source;
    return old;
}

int lora_run_host_dtype(int shape, int dtype, const void *in, void *out, const double *params, int times,
                        const int *dims, int quiet, lora_run_info *info) {
    if (!in || !out || !dims || times < 0) return LORA_EINVAL;
    if (dtype == LORA_BF16)
        if (int rc = lora::default_source_refused("a bf16 run")) return rc;
    lora::HostRun dev;
    int rc = dev.open(shape, dtype, dims, params);
    if (rc != LORA_OK) return rc;
    lora_plan *plan = dev.plan;
    const size_t bytes = dev.bytes;
    LORA_HIP_TRY(dev.alloc(2));
    LORA_HIP_TRY(hipMemcpy(dev.b[0], in, bytes, hipMemcpyHostToDevice));  // whole padded input, halo included
    if (int src_rc = lora::attach_default_source(plan, bytes, &dev.src)) return src_rc;  // the thread's default source, beside the grid
    // warm-up (the reference has none): one sweep into buf1, which is then cleared again
    if (times > 0) {
        rc = lora_plan_step(plan, dev.b[0], dev.b[1], nullptr);
        if (rc != LORA_OK) return rc;
    }
    LORA_HIP_TRY(hipMemset(dev.b[1], 0, bytes));
    LORA_HIP_TRY(dev.stream());
    LORA_HIP_TRY(hipDeviceSynchronize());
    if (times >= 16 && bytes <= (64u << 20)) {
        // build (capture + instantiate) the graph outside the timed region, like the reference's setup work
        rc = lora_plan_run(plan, dev.b[0], dev.b[1], times, dev.s);
        if (rc != LORA_OK) return rc;
        LORA_HIP_TRY(hipStreamSynchronize(dev.s));
        LORA_HIP_TRY(hipMemcpy(dev.b[0], in, bytes, hipMemcpyHostToDevice));
        LORA_HIP_TRY(hipMemset(dev.b[1], 0, bytes));
    }
    // (set-up, like the reference's own allocations ahead of its timed loop: the scratch grid / extended grid this run's
    // schedule would otherwise allocate inside the timed region)
    (void) lora_plan_prepare_run(plan, times);
    LORA_HIP_TRY(hipDeviceSynchronize());

    dev.tic();
    rc = lora_plan_run(plan, dev.b[0], dev.b[1], times, dev.s);
    if (rc != LORA_OK) return rc;
    LORA_HIP_TRY(hipStreamSynchronize(dev.s));
    dev.toc();

    // 1D copies all but the last element (1d/gpu_1r.cu:134)
    const size_t copy_bytes = (plan->p.ndim == 1) ? bytes - dev.esize : bytes;
    LORA_HIP_TRY(hipMemcpy(out, dev.b[times % 2], copy_bytes, hipMemcpyDeviceToHost));
    return dev.finish(times, plan->p.source ? 3.0 : 2.0, plan->p.steps_per_launch, quiet, info);  // a source is one more read
}

int lora_last_run_info(lora_run_info *info) {
    if (!info) return LORA_EINVAL;
    *info = lora::g_last_info;
    return LORA_OK;
}

int lora_gpu_1d1r(const double *in, double *out, const double *params, int times, int n) {
    const int dims[1] = {n};
    return lora_run_host(LORA_1D1R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_1d2r(const double *in, double *out, const double *params, int times, int n) {
    const int dims[1] = {n};
    return lora_run_host(LORA_1D2R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_star_2d1r(const double *in, double *out, const double *params, int times, int m, int n) {
    const int dims[2] = {m, n};
    return lora_run_host(LORA_STAR2D1R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_star_2d3r(const double *in, double *out, const double *params, int times, int m, int n) {
    const int dims[2] = {m, n};
    return lora_run_host(LORA_STAR2D3R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_box_2d3r(const double *in, double *out, const double *params, int times, int m, int n) {
    const int dims[2] = {m, n};
    return lora_run_host(LORA_BOX2D3R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_box_3d1r(const double *in, double *out, const double *params, int times, int h, int m, int n) {
    const int dims[3] = {h, m, n};
    return lora_run_host(LORA_BOX3D1R, in, out, params, times, dims, 0, nullptr);
}
int lora_gpu_star_3d1r(const double *in, double *out, const double *params, int times, int h, int m, int n) {
    const int dims[3] = {h, m, n};
    return lora_run_host(LORA_STAR3D1R, in, out, params, times, dims, 0, nullptr);
}

}  // extern "C"

namespace lora {
// What run_launches enqueues for `times` sweeps of a plan under the Dirichlet boundary: the halo copy (and the scratch grid's),
// the schedule's fused launches and the single sweeps behind them (the multigrid driver's tally, mg.cpp).
int dirichlet_run_launches(lora_plan *plan, int times) {
    if (times <= 0) return 0;
    const Schedule sc = plan_schedule(plan, times, false);
    int done = 0;
    for (int d : sc.depths) done += d;
    return 1 + (sc.scratch ? 1 : 0) + (int) sc.depths.size() + (times - done);
}

void release_run_state(lora_plan *plan) {
    drop_graph(plan);
    torus_drop(plan);
    mg_release(plan);
    for (DeviceGrid *g : {&plan->scratch, &plan->records, &plan->leap[0], &plan->leap[1], &plan->cheb_probe, &plan->cg[0], &plan->cg[1],
                          &plan->cg[2], &plan->cg_state, &plan->theta_state, &plan->pcg_z})
        g->release();
}
}  // namespace lora
