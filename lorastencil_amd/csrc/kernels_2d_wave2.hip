// kernels_2d_wave2.hip -- TWO variable-coefficient wave steps per launch, 2D fp64: the EPI_WAVE instantiations of
// the one two-step body, stencil2d_step2_kernel<TAPSET, R1, EPI> (step2_body.h), for the three tap sets:
//     out1 = k S(cur) + b cur + c prev,      out2 = k S(out1) + b out1 + c cur
// each level through step_epilogue<EPI_WAVE>: five separate fp64 roundings behind the direct taps, so a launch equals two single
// steps (kernels_step.hip) bit for bit on any data.  The tiles, the boundary rule and the load schedule are EPI_LEAP_SRC's
// (kernels_2d_step2.hip has the table) with k in f's place: on interior level-1 cells as two 8-byte loads, at level 2 as the
// 16-byte piece at the store's address; no halo cell of k is read.  The centre cell the rule multiplies by b is on chip at both
// levels: at level 1 the cell of the input window in A (read before the barrier in front of B's first write), at level 2 the
// level-1 cell that leaves as out1 (mid).  A translation unit of its own: kernels_2d_step2.hip keeps exactly its four rules.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step2_body.h"
#include "step_epilogue.h"

namespace lora {

// Two wave steps (2D plans of wave depth 2; the entries of leapfrog.cpp refuse the others).
hipError_t launch_wave2_2d(const Plan &p, const double *prev, const double *cur, const double *k, double *out1, double *out2, double b,
                           double c, int begin, int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.prev = prev;
    a.cur = cur;
    a.f = k;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = b;
    a.c1 = c;
    a.a2 = b;
    a.c2 = c;
    return launch_step2_e<EPI_WAVE>(p, a, begin, end, s);
}

}  // namespace lora
