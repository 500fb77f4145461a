// hostrun.cpp -- lora::HostRun (engine.h): the skeleton of the host-buffer operators that stand in for the reference's gpu_*()
// functions -- lora_run_host_dtype (capi.cpp), lora_run_host_until (reduce.cpp), lora_run_host_leapfrog (leapfrog.cpp),
// lora_run_host_chebyshev (chebyshev.cpp) -- and, through open_solver / ready / timed, the whole sequence of the five source
// solvers: lora_run_host_cg, _theta, _pcg, _theta_mg (cg.cpp) and lora_run_host_mg (mg.cpp).
//
// Reference behaviour followed (file:line under the reference's src/):
//   timing = steady_clock around the launch loop + one device sync
//           (1d/gpu_1r.cu:103-134, 2d/gpu.cu:392-421, :450-479, :525-554, 3d/gpu_star.cu:158-192, 3d/gpu_box.cu:190-223)
//   stdout: label / "Time = <ms>[ms]" / "GStencil/s = %f" (e.g. 2d/gpu.cu:549-553)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>

#include "engine.h"

namespace lora {

using clock = std::chrono::steady_clock;
static long long now() { return clock::now().time_since_epoch().count(); }

const char *run_label(int shape) {
    switch (shape) {
        case LORA_1D1R:
            return "LoRAStencil(1D 1d1r): ";  // 1d/gpu_1r.cu:127
        case LORA_1D2R:
            return "LoRAStencil(1D 1d2r): ";  // 1d/gpu_2r.cu:129
        case LORA_STAR2D1R:
            return "LoRAStencil(2D star_2d1r): ";  // 2d/gpu.cu:549
        case LORA_STAR2D3R:
            return "LoRAStencil(2D star_2d3r): ";  // 2d/gpu.cu:474
        case LORA_BOX2D1R:
        case LORA_BOX2D3R:
            return "LoRAStencil(2D box_2d3r): ";  // 2d/gpu.cu:415 (one operator serves both box shapes)
        case LORA_STAR3D1R:
            return "LoRAStencil(3D star_3d1r): ";  // 3d/gpu_star.cu:185
        case LORA_BOX3D1R:
            return "LoRAStencil(3D box_3d1r): ";  // 3d/gpu_box.cu:216
        default:
            return "LoRAStencil(?): ";
    }
}

HostRun::~HostRun() {
    if (s) (void) hipStreamDestroy(s);
    if (src) (void) hipFree(src);
    for (void *x : b)
        if (x) (void) hipFree(x);
    lora_plan_destroy(plan);
}

int HostRun::open(int shape, int dtype, const int *dims, const double *params) {
    if (lora_device_count() <= 0) return no_device();
    if (int rc = lora_plan_create(&plan, shape, dtype, dims, params)) return rc;
    this->shape = shape;
    for (int d = 0; d < plan->p.ndim; ++d) points *= dims[d];
    esize = dtype == LORA_BF16 ? 2 : sizeof(double);
    bytes = lora_plan_padded_bytes(plan);
    return LORA_OK;
}

hipError_t HostRun::alloc(int n) {
    ticks[0] = now();
    for (int i = 0; i < n; ++i) {
        const hipError_t e = hipMalloc(&b[i], bytes);
        if (e != hipSuccess) {
            (void) hipGetLastError();
            b[i] = nullptr;
            return e;
        }
    }
    return hipSuccess;
}

hipError_t HostRun::stream() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
void HostRun::tic() { ticks[1] = now(); }
void HostRun::toc() { ticks[2] = now(); }

int HostRun::open_solver(int shape, const int *dims, const double *params, const double *in, const double *source) {
    if (int rc = open(shape, LORA_F64, dims, params)) return rc;
    if (alloc(source ? 2 : 1) != hipSuccess) return LORA_ENOMEM;
    if (int rc = hip_status(hipMemcpy(b[0], in, bytes, hipMemcpyHostToDevice), "upload")) return rc;
    return source ? hip_status(hipMemcpy(b[1], source, bytes, hipMemcpyHostToDevice), "upload") : LORA_OK;
}

int HostRun::ready() {
    if (int rc = hip_status(stream(), "stream")) return rc;
    return hip_status(hipDeviceSynchronize(), "upload");
}

int HostRun::timed_end(double *out) {
    if (int rc = hip_status(hipStreamSynchronize(s), "run")) return rc;
    toc();
    return hip_status(hipMemcpy(out, b[0], bytes, hipMemcpyDeviceToHost), "download");
}

int HostRun::finish(int steps, double grids_moved, int steps_per_launch, int quiet, lora_run_info *info) {
    const clock::duration sweep(ticks[2] - ticks[1]), total(now() - ticks[0]);
    const int F = lora_shape_gstencil_factor(shape);
    lora_run_info ri;
    ri.sweep_seconds = std::chrono::duration<double>(sweep).count();
    ri.total_seconds = std::chrono::duration<double>(total).count();
    ri.gstencils = points * steps / ri.sweep_seconds / 1e9;
    ri.gstencils_refconv = ri.gstencils * F;
    ri.hbm_gbs = points * steps * grids_moved * esize / ri.sweep_seconds / 1e9;
    ri.variant = plan->p.variant;
    ri.steps_per_launch = steps_per_launch;
    set_last_run_info(ri);
    if (info) *info = ri;
    if (!quiet) {
        // byte-compatible with the reference's three lines (2d/gpu.cu:549-553)
        const double secs = std::chrono::duration_cast<std::chrono::microseconds>(sweep).count() / 1e6;
        std::printf("%s\n", run_label(shape));
        std::printf("Time = %lld[ms]\n", (long long) std::chrono::duration_cast<std::chrono::milliseconds>(sweep).count());
        std::printf("GStencil/s = %f\n", points * steps * F / secs / 1e9);
        std::fflush(stdout);
    }
    return LORA_OK;
}

}  // namespace lora
