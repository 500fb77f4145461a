// kernels_2d_step2.hip -- TWO applications per launch with an update rule at both stores, 2D fp64: ONE kernel
// body, stencil2d_step2_kernel<TAPSET, R1, EPI> (step2_body.h, with its launcher template), whose rule EPI (step_epilogue.h) is a
// template parameter.  This unit instantiates four rules (the fifth, EPI_WAVE, is kernels_2d_wave2.hip's: DESIGN 3.18):
//     EPI_SOURCE        level 1 = S(in) + f,               out  = S(level 1) + f             launch_source2 (plans with a source)
//     EPI_LEAP          out1 = S(cur) + c prev,            out2 = S(out1) + c cur            launch_leapfrog2_2d
//     EPI_LEAP_SCALED   out1 = a1 S(cur) + c1 prev,        out2 = a2 S(out1) + c2 cur        launch_leapfrog2_src_2d, f == nullptr
//     EPI_LEAP_SRC      out1 = a1 (S(cur) + f) + c1 prev,  out2 = a2 (S(out1) + f) + c2 cur  launch_leapfrog2_src_2d
//
// The tile (that of stencil2d_fused2_kernel, kernels_2d_fused.hip):
//   output tile        TH = 4 R1 - 6 rows x 122 columns          (61 lanes x 2 columns; j0 = 122 tx is even)
//   level-1 tile       4 R1 rows      x 128 columns  in LDS (B)  (the output tile plus a ring of 3 cells)
//   input window       4 R1 + 6 rows  x 136 columns  in LDS (A)  (starts 6 left: 16-byte aligned pieces of a row)
// B overwrites A once every wave has consumed its part of it.  R1 = 6 for the star, 10 for the diamond and the box.
//
// Arithmetic: the DIRECT taps of the plan's tap set in row-major order at both levels, always -- never the structured forms of
// rows_2d.h, whatever the plan's fused_eval says -- one fma per tap from an accumulator of 0 (taps_row), then the rule's separate
// fp64 roundings (step_epilogue).  That is the single step's arithmetic (kernels_step.hip) at each level through the same two
// functions, so a launch equals two single steps bit for bit on any data.  Each rule is its own instantiation: "no source" is
// not "add a zero", leapfrog is not "scale by 1", and an operand a rule does not read produces no load and no live register.
//
// What EPI selects, and nothing else (the load schedule and the boundary rule; DESIGN 3.6 has the one complete table, with the
// interior values, which are the formulas above through step_epilogue<EPI>, one column per rule):
//                                  EPI_SOURCE               EPI_LEAP, EPI_LEAP_SCALED       EPI_LEAP_SRC
//   staged grid                    in                       cur                             cur
//   level-1 side loads, per row    f under "cell is         prev under "cell is within 3    prev as left, and f under
//   two 8-byte loads               interior"                of the interior"                "cell is interior"
//   ... asked for at window row    row + 0                  row + 0                         row + 4
//   level-1 cell outside the       Dirichlet: the cell      what prev holds there           what prev holds there
//   interior                       itself from A; else 0
//   level-2 side loads: 16-byte    f, all rows before       cur, in the window loop at      cur and f, as left
//   piece at the store's address   the window loop          window row = output row
//   under the store's predicate
//   out1                           none (B only)            stored by the level-2 lanes     as left
// A level-1 lane owns two columns that start at an ODD padded column (the tiles are shifted by 3), hence two 8-byte loads per
// row there and never a 16-byte one; under "cell is interior" no halo cell of f is loaded at all.  The ring is 3 and the pad 4,
// so a level-1 cell outside the interior is always inside the padded array of prev; a cell further out than 3 is never loaded
// (it feeds no stored result).  Level-1 loads are asked for six window rows before their row completes; with both prev and f
// only two rows before, which keeps the cells in flight within the register budget of three workgroups per CU (no scratch).
// The level-2 piece of cur was staged by this or a neighbouring workgroup just before: it comes from L2.
// out1 passes through the window registers: the level-1 centre cells of a lane's output piece are win[3] and win[4] of window
// row r + 3, so out1 and out2 both leave as 16-byte pieces under one predicate.
// Never written: in / cur, prev, f, and every halo cell of out / out1 / out2.  Never read: halo cells of f; anything outside
// the padded arrays (staged pieces are clamped into them and only feed level-1 cells that the boundary rule replaces).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "step2_body.h"
#include "step_epilogue.h"

namespace lora {

namespace {

// The rule chosen at run time -> its instantiation.  Two applications over the interior rows [begin, end).
hipError_t launch_step2(int epi, const Plan &p, const ArgsStep2 &a, int begin, int end, hipStream_t s) {
    switch (epi) {
        case EPI_SOURCE:
            return launch_step2_e<EPI_SOURCE>(p, a, begin, end, s);
        case EPI_LEAP:
            return launch_step2_e<EPI_LEAP>(p, a, begin, end, s);
        case EPI_LEAP_SCALED:
            return launch_step2_e<EPI_LEAP_SCALED>(p, a, begin, end, s);
        default:
            return launch_step2_e<EPI_LEAP_SRC>(p, a, begin, end, s);
    }
}

}  // namespace

// Two applications with the plan's source.
hipError_t launch_source2(const Plan &p, const double *in, double *out, int begin, int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.cur = in;
    a.f = static_cast<const double *>(p.source);
    a.out2 = out;
    return launch_step2(EPI_SOURCE, p, a, begin, end, s);
}

// Two leapfrog steps (2D plans; launch_leapfrog2 of engine.h dispatches).
hipError_t launch_leapfrog2_2d(const Plan &p, const double *prev, const double *cur, double *out1, double *out2, double c, int begin,
                               int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.prev = prev;
    a.cur = cur;
    a.out1 = out1;
    a.out2 = out2;
    a.c1 = c;
    return launch_step2(EPI_LEAP, p, a, begin, end, s);
}

// Two scaled leapfrog steps; f == nullptr: no source (2D plans; launch_leapfrog2_src of engine.h dispatches).
hipError_t launch_leapfrog2_src_2d(const Plan &p, const double *prev, const double *cur, const double *f, double *out1, double *out2,
                                   double a1, double c1, double a2, double c2, int begin, int end, hipStream_t s) {
    ArgsStep2 a = {};
    a.prev = prev;
    a.cur = cur;
    a.f = f;
    a.out1 = out1;
    a.out2 = out2;
    a.a1 = a1;
    a.c1 = c1;
    a.a2 = a2;
    a.c2 = c2;
    return launch_step2(f ? EPI_LEAP_SRC : EPI_LEAP_SCALED, p, a, begin, end, s);
}

// The name lora_plan_kernel_name reports for a two-application source launch: the EPI_SOURCE instantiation of
// stencil2d_step2_kernel (DESIGN 3.6 maps the reported names to the device symbols).
const char *source2_kernel_name(const Plan &) { return "stencil2d_source2_kernel"; }

}  // namespace lora
