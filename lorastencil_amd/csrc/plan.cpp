// plan.cpp -- what a plan is: its creation, taps, boundary, variant and options (the requested state), and the resolvers
// that derive from them which kernel runs at which depth (struct Resolved, engine.h).  Launching a resolved plan is
// capi.cpp's side; nothing here needs a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "engine.h"

namespace lora {

static thread_local int g_default_boundary = LORA_BC_REFERENCE;
static thread_local int g_default_normalize = 0;
static thread_local int g_default_leap3 = 0;
static thread_local int g_default_wave3 = 0;
static thread_local int g_default_coarse1 = 0;
static thread_local int g_default_mgfuse = 0;

int region_granularity(const Plan &p) { return p.ndim == 1 ? 2 : 1; }  // 2D tiles and 3D chunks may start on any row / plane

// Factors for the MFMA formulation out = sum_t (U_t X) V_t + residual taps, derived from the applied taps W:
//   * c x the star2d1r table  -> the reference's hard-coded rank-1 factor u = v = (0,1,2,4,2,1,0) plus its 8-point
//                                correction (2d/gpu.cu:486-487, :249-264), scaled by c;
//   * star-shaped W           -> vertical band = centre column, horizontal band = centre row without the centre
//                                (2d/gpu.cu:433-444), i.e. two terms with a unit factor each;
//   * anything else           -> pyramid factorisation into three terms (2d/gpu.cu:280-350); what it does not
//                                capture is applied as residual taps if it is sparse enough.
static void derive_lowrank(Plan &p) {
    LowRank2D &lr = p.lowrank;
    lr = LowRank2D{};
    p.lowrank_valid = false;
    const double *W = p.w;
    auto finish_residual = [&](double tol) {
        double wmax = 0.0;
        for (int k = 0; k < 49; ++k) wmax = std::fmax(wmax, std::fabs(W[k]));
        lr.nresid = 0;
        for (int r = 0; r < 7; ++r)
            for (int c = 0; c < 7; ++c) {
                double s = 0.0;
                for (int t = 0; t < lr.rank; ++t) s += lr.u[t][r] * lr.v[t][c];
                const double d = W[r * 7 + c] - s;
                if (!std::isfinite(d)) return false;
                if (std::fabs(d) > tol * wmax) {
                    if (lr.nresid == 16) return false;
                    lr.rdy[lr.nresid] = r - 3;
                    lr.rdx[lr.nresid] = c - 3;
                    lr.rw[lr.nresid] = d;
                    ++lr.nresid;
                }
            }
        return true;
    };
    // (1) scaled star2d1r table
    double ref[49];
    default_params(LORA_STAR2D1R, ref);
    const double c = W[24] / ref[24];
    bool scaled = std::isfinite(c) && c != 0.0;
    for (int k = 0; k < 49 && scaled; ++k) scaled = std::fabs(W[k] - c * ref[k]) <= 1e-14 * std::fabs(c * ref[24]);
    if (scaled) {
        static const double f[7] = {0, 1, 2, 4, 2, 1, 0};
        lr.rank = 1;
        for (int e = 0; e < 7; ++e) {
            lr.u[0][e] = c * f[e];
            lr.v[0][e] = f[e];
        }
        p.lowrank_valid = finish_residual(1e-14);
        return;
    }
    // (2) star-shaped taps
    if (p.tapset == TAPS2D_STAR) {
        lr.rank = 2;
        for (int e = 0; e < 7; ++e) {
            lr.u[0][e] = W[e * 7 + 3];
            lr.v[0][e] = (e == 3) ? 1.0 : 0.0;
            lr.u[1][e] = (e == 3) ? 1.0 : 0.0;
            lr.v[1][e] = (e == 3) ? 0.0 : W[3 * 7 + e];
        }
        p.lowrank_valid = finish_residual(1e-14);
        return;
    }
    // (3) pyramid factorisation (the reference's scheme: exact for its symmetric tables)
    {
        double u[4][7], v[4][7];
        factorize_7x7(W, u, v, nullptr);
        lr.rank = 3;
        bool finite = true;
        for (int t = 0; t < 3; ++t)
            for (int e = 0; e < 7; ++e) {
                finite = finite && std::isfinite(u[t][e]) && std::isfinite(v[t][e]);
                lr.u[t][e] = u[t][e];
                lr.v[t][e] = v[t][e];
            }
        if (finite && finish_residual(1e-13)) {
            p.lowrank_valid = true;
            return;
        }
    }
    // (4) any other taps: truncated SVD, as many terms (<= 3) as the singular values ask for; what three terms do not
    //     capture must be a few isolated taps (applied on the vector pipe) or the taps are refused for this variant
    {
        double u[7][7], v[7][7], sigma[7];
        lr = LowRank2D{};
        if (svd_7x7(W, u, v, sigma) != LORA_OK || !(sigma[0] > 0.0)) return;
        int rank = 1;
        while (rank < 3 && sigma[rank] > 1e-14 * sigma[0]) ++rank;
        lr.rank = rank;
        for (int t = 0; t < rank; ++t)
            for (int e = 0; e < 7; ++e) {
                lr.u[t][e] = u[t][e];
                lr.v[t][e] = v[t][e];
            }
        p.lowrank_valid = finish_residual(1e-13);
    }
}

// ---- the forms of 2D taps the fused kernels evaluate on the vector pipe (rows_2d.h; fused_eval 3..7) ----------------

static bool outside_zero(const LowRank2D &lr, int t, int lo) {
    for (int e = 0; e < 7; ++e)
        if ((e < lo || e > 6 - lo) && (lr.u[t][e] != 0.0 || lr.v[t][e] != 0.0)) return false;
    return true;
}

// Low-rank diamond (fused_eval 3): one term inside the 5 x 5 window plus the 8-point correction +c on (+-3, 0), (0, +-3)
// and -c on (+-2, +-2).  Returns whether the factors have that form; *rc = c.
static bool diamond_form(const LowRank2D &lr, double *rc) {
    if (!(lr.rank == 1 && lr.nresid == 8 && outside_zero(lr, 0, 1))) return false;
    double c = 0.0;
    for (int k = 0; k < 8; ++k) {
        const int ay = lr.rdy[k] < 0 ? -lr.rdy[k] : lr.rdy[k], ax = lr.rdx[k] < 0 ? -lr.rdx[k] : lr.rdx[k];
        const bool tip = (ay == 3 && ax == 0) || (ay == 0 && ax == 3), corner = ay == 2 && ax == 2;
        if (!tip && !corner) return false;
        const double ck = tip ? lr.rw[k] : -lr.rw[k];
        if (k == 0) c = ck;
        if (ck != c) return false;
    }
    *rc = c;
    return true;
}

// Low-rank pyramid (fused_eval 4..6): three terms of shrinking support, no residual.  Returns the form or 0.
static int pyramid_form(const LowRank2D &lr, int lowrank_valu) {
    if (!(lr.rank == 3 && lr.nresid == 0 && outside_zero(lr, 1, 1) && outside_zero(lr, 2, 2))) return 0;
    // mirror-symmetric horizontal profiles (every table the pyramid scheme accepts: it needs a symmetric
    // matrix): the mirrored taps of a row are pre-added once and shared by the three terms
    bool sym = lowrank_valu != 2;  // lowrank_valu = 2 keeps the plain pyramid form (A/B timing)
    for (int t = 0; t < 3 && sym; ++t)
        for (int e = 0; e < 3; ++e)
            if (lr.v[t][e] != lr.v[t][6 - e]) sym = false;
    if (!sym) return 4;
    // the reference table's middle factor (0, 1, 0, -1, 0, 1, 0): zero taps skipped at compile time
    return (lowrank_valu != 3 && lr.u[1][2] == 0.0 && lr.u[1][4] == 0.0 && lr.v[1][2] == 0.0) ? 6 : 5;
}

// Nested-profile form (fused_eval 7; rows_2d.h, EVAL_NEST): row dy of the table = g[k] T_k, k = 3 - |dy - 3|, T_0 = x3,
// T_k = a_k T_(k-1) + (x_(3-k) + x_(3+k)).  Accepted only if the taps it implies are the plan's taps EXACTLY.
static bool nested_form(const double *W, double g[4], double a[4]) {
    a[0] = 0.0;
    for (int k = 0; k < 4; ++k) {
        g[k] = W[k * 7 + (3 - k)];  // outermost tap of row k
        if (!(g[k] != 0.0) || !std::isfinite(g[k])) return false;
    }
    for (int k = 1; k < 4; ++k) {
        a[k] = W[k * 7 + (4 - k)] / g[k];  // next tap inwards / outermost tap
        if (!std::isfinite(a[k])) return false;
    }
    for (int dy = 0; dy < 7; ++dy) {
        const int k = dy <= 3 ? dy : 6 - dy;
        // coefficient of x_(3 +- e) in T_k: prod of a_j for j = e+1 .. k (1 for e = k, absent for e > k)
        for (int dx = 0; dx < 7; ++dx) {
            const int e = dx <= 3 ? 3 - dx : dx - 3;
            double c = 0.0;
            if (e <= k) {
                c = g[k];
                for (int j2 = k; j2 > e; --j2) c *= a[j2];
            }
            if (c != W[dy * 7 + dx]) return false;
        }
    }
    return true;
}

// ---- the resolvers: each a sequence of decisions, the measurements that set a rule next to it -----------------------

static void resolve_1d(Plan &p) {
    // K applications per launch (kernels_1d.hip): 8 by default, the single sweep being launch-latency bound
    p.steps_per_launch = p.steps_per_launch_req == 0 ? 8 : p.steps_per_launch_req;
    p.kernel_name = p.steps_per_launch > 1 ? kernel_name_1d_fused(p) : kernel_name_1d(p);
}

static void resolve_2d(Plan &p) {
    // Tap set: the smallest one that covers the non-zero pattern of the applied taps
    bool diamond = true, star = true;
    for (int r = 0; r < 7; ++r)
        for (int c = 0; c < 7; ++c) {
            if (p.w[r * 7 + c] == 0.0) continue;
            const int ar = r < 3 ? 3 - r : r - 3, ac = c < 3 ? 3 - c : c - 3;
            if (ar != 0 && ac != 0) star = false;
            if (ar + ac > 3) diamond = false;
        }
    p.tapset = star ? TAPS2D_STAR : (diamond ? TAPS2D_DIAMOND : TAPS2D_BOX);

    // Variant: the matrix-pipe one needs a low-rank form of the taps and 16-byte aligned rows
    derive_lowrank(p);
    if (p.variant == LORA_VARIANT_MFMA && !p.lowrank_valid) p.variant = LORA_VARIANT_DIRECT;
    if (p.generic) {
        p.variant = LORA_VARIANT_DIRECT;
        p.lowrank_valid = false;
    }

    // Depth.  Temporal fusion (two applications per launch) wins for every tap set once the tile height is tuned
    // (16384^2 / 8192^2, profiles/r01_sweep_fused_rows.jsonl: 25 taps 602 vs 352 GStencils/s, 13 taps 649 vs
    // 345, 49 taps 400 vs 350); the light 13-tap star prefers the small tile (more workgroups per CU), the
    // FMA-heavier sets the tall one (less recomputed halo).
    // Odd innermost extent (rows only 8-byte aligned): the tiled kernels do not apply, but the row-streaming kernel
    // does -- its 16-byte row pieces need dword alignment only, and the last, half-valid column pair of a row is
    // cut by the store descriptor's per-dword range check -- so fused launches keep their speed and only the
    // single-sweep tail (at most one launch per run) goes through the generic kernel
    const bool stream_ref = p.stream2 && p.boundary == LORA_BC_REFERENCE;  // row-streaming family, the source's own halo
    if (p.variant == LORA_VARIANT_MFMA || (p.generic && !stream_ref))
        p.steps_per_launch = 1;
    else
        p.steps_per_launch = p.steps_per_launch_req == 0 ? max_depth(2) : p.steps_per_launch_req;
    // Temporal fusion wins for every tap set: star2d1r 16384^2 352 (one sweep per launch) -> 593 (tile kernel, 2)
    // -> 591 (row-streaming, 2) -> 843 GStencils/s (row-streaming, 4: profiles/r02_*).  Four applications per launch
    // exist in the row-streaming kernel, reference boundary (the level-2 halo is the source buffer's own; the
    // Dirichlet option would need source rows 11 steps back); six in the workgroup-row kernel (kernels_2d_wg.hip), same
    // conditions; otherwise two
    if (p.steps_per_launch >= 4 && !stream_ref) p.steps_per_launch = 2;
    p.fused_rows = p.fused_rows_req ? p.fused_rows_req : (p.tapset == TAPS2D_STAR ? 6 : 10);

    // Evaluation form: the direct taps of the tap set, or -- fused launches only -- a structured form on the vector pipe
    // (kernels_2d_fused.hip, apply_row) when the taps have the support pattern it is specialised for
    p.fused_eval = p.tapset;
    if (p.steps_per_launch >= 2 && p.lowrank_valid && p.lowrank_valu != 0) {
        if (diamond_form(p.lowrank, &p.lowrank_rc))
            p.fused_eval = 3;
        else if (const int form = pyramid_form(p.lowrank, p.lowrank_valu))
            p.fused_eval = form;
    }
    double g[4], a[4];
    if (p.steps_per_launch >= 2 && p.lowrank_valu != 0 && p.lowrank_valu != 4 && nested_form(p.w, g, a)) {
        p.fused_eval = 7;
        std::memcpy(p.nest_g, g, sizeof g);
        std::memcpy(p.nest_a, a, sizeof a);
    }

    // Kernel family of the fused launches.
    // (49 direct taps -- a table with no low-rank form -- do not fit the scalar registers of the six-application kernel
    // beside its three levels per wave, and rounds 2 - 3 kept such plans at four applications per launch for it.
    // Measured, six win all the same: 395 against 264 - 295 GStencils/s at 8192^2, 432 against 333 at 16384^2
    // (tools/k6_general.py): the taps come from the constant cache, the bytes per sweep are a third less.)
    // The workgroup-row kernel for six applications and, in such plans, for the four- and two-application tails of a
    // run; plans that ask for four or two keep the row-streaming kernel (option wg = 1: the workgroup-row kernel at every
    // depth)
    p.wg_active = stream_ref && p.variant == LORA_VARIANT_DIRECT && p.wg != 0 &&
                  (p.steps_per_launch == 6 || (p.wg == 1 && p.steps_per_launch >= 2));
    if (p.steps_per_launch == 6 && !p.wg_active) p.steps_per_launch = 4;
    // The Dirichlet option: the workgroup-row kernel at FOUR applications per launch (a row of halo values per level;
    // six would need 98 KB of LDS per workgroup), unless the plan asks for two or switches the kernel off
    if (p.boundary == LORA_BC_DIRICHLET && !p.generic && p.stream2 && p.wg != 0 && p.variant == LORA_VARIANT_DIRECT &&
        p.fused_eval != TAPS2D_BOX && (p.steps_per_launch_req == 0 || p.steps_per_launch_req >= 4)) {
        p.steps_per_launch = 4;
        p.wg_active = 1;
    }
    if (p.wg_active) prepare_2d_wg(p);  // kernel resolution + residency query now, not in the first launch of a run

    p.kernel_name = (p.generic && p.steps_per_launch == 1) ? kernel_name_generic(p)
                    : p.variant == LORA_VARIANT_MFMA       ? kernel_name_2d_mfma(p)
                    : p.wg_active                          ? kernel_name_2d_wg(p)
                    : p.steps_per_launch == 1              ? kernel_name_2d_direct(p)
                    : p.stream2                            ? kernel_name_2d_stream(p)
                                                           : kernel_name_2d_fused2(p);
}

// Tap set, and the factors of separable taps.  Returns whether fp64 box taps are exactly separable (cba64: c(x), b(y), a(z)).
static bool taps_3d(Plan &p, double cba64[9]) {
    const bool bf16 = p.dtype == LORA_BF16;
    bool star = true;
    for (int k = 0; k < 27; ++k) {
        if (p.w[k] == 0.0) continue;
        const int dz = k / 9, dy = (k / 3) % 3, dx = k % 3;
        if ((dz != 1) + (dy != 1) + (dx != 1) > 1) star = false;
    }
    p.tapset = star ? TAPS3D_STAR : TAPS3D_BOX;
    // bf16: exactly separable box taps are evaluated as x / y / z passes (option separable = 0: the 27-tap order)
    if (!star && bf16) {
        float w32[27], cba[9];
        for (int k = 0; k < 27; ++k) w32[k] = (float) p.w[k];
        if (separable_27(w32, cba)) {
            if (p.separable != 0) {
                p.tapset = TAPS3D_SEP;
                for (int k = 0; k < 9; ++k) p.sep[k] = cba[k];
            }
            p.mfma3_valid = mfma_factors_27(cba, &p.mfma3_scale, p.mfma3_abc) != 0;
        }
    }
    // Exactly separable fp64 box taps (the reference's: they depend on dx only) can be evaluated as x / y / z passes, 9-10
    // instead of 27 multiply-adds per point (option separable = 0: the 27-tap order)
    return !bf16 && p.tapset == TAPS3D_BOX && p.separable != 0 && separable_27d(p.w, cba64) != 0;
}

// The tile kernel or the plane-streaming kernel, at two or three applications per launch.
static void tiles_or_planes(Plan &p, bool sep_taps, const double *cba64, double npts) {
    const int req = p.steps_per_launch_req;
    // Two applications per launch (kernels_3d_fused.hip): fp64 tiled path; default, as in 2D (star3d1r 512^3
    // 499 vs 288 GStencils/s, box3d1r 768^3 523 vs 300)
    p.steps_per_launch = (!p.generic && req != 1) ? 2 : 1;
    // fp64: THREE applications per launch in the plane-streaming kernel (kernels_3d_planes.hip) -- the grid is read
    // and written once per three sweeps.  An odd count needs no halo copies: launch k starts at global step 3 k and
    // runs on the reference's own buffer state (lora_plan_run)
    // Which fused kernel: the plane-streaming kernel needs a grid that fills its 60 x 60 tiles and 32-plane chunks a few
    // times over (tools/small3d.sh, GStencils/s per launch, tile kernel / planes K = 2 / planes K = 3: star 256^3 496 /
    // 452 / 371, 320^3 458 / 499 / 408, 448^3 562 / 627 / 545, 512^3 497 / 583 / 618, 768^3 530 / 603 / 722; box 256^3
    // 300 / 307, 320^3 307 / 351, 768^3 446 / 499): three applications from ~1.2e8 points (star), two from ~2.4e7,
    // the round-1 tile kernel below.  Option stream3: -1 this rule, 0 tile kernel, 1 plane-streaming kernel always;
    // steps_per_launch = 3 asks for it by itself.  (In its 27-tap order the box stays at two: the third level makes
    // the launch VALU- and LDS-bound; its separable form takes three: that makes a third application per launch pay
    // for the box as well.)
    const bool planes_ok = p.dtype != LORA_BF16 && !p.generic && p.stream3 != 0 && p.boundary != LORA_BC_PERIODIC;
    if (!planes_ok || p.steps_per_launch != 2) return;
    const bool three_pays = p.tapset == TAPS3D_STAR || sep_taps;
    if (req == 3) {
        p.stream3_active = 1;
        p.steps_per_launch = 3;
    } else if (p.stream3 == 1 || npts >= (sep_taps ? 2.0e6 : 2.4e7)) {  // (separable box: from ~128^3, tools/rule3d.sh)
        p.stream3_active = 1;
        // (the separable box: 512^3 two applications 593, three 535-589; 768^3 588 / 673 GStencils/s)
        const double from = p.tapset == TAPS3D_STAR ? 1.2e8 : 3.0e8;
        if (req == 0 && three_pays && (p.stream3 == 1 || npts >= from)) p.steps_per_launch = 3;
    }
    if (p.stream3_active && sep_taps) {
        p.sep64_valid = 1;
        for (int k = 0; k < 9; ++k) p.sep64[k] = cba64[k];
    }
}

// FOUR applications per launch with the levels in registers (kernels_3d_lanes.hip): fp64, the 7-point star or
// exactly separable box taps, reference boundary, any extents (odd innermost ones too: its fused launches replace
// the one-thread-per-point fallback, which then only serves single-sweep tails).  Big grids: a tile is 24 x 120
// output points and a z-chunk re-reads 8 planes, so the launch wants ~256 tiles x long chunks (star3d1r
// GStencils/s per launch, planes kernel / this one: see DESIGN 3.3d); option lanes3 = 1 / 0 forces either,
// steps_per_launch = 4 asks for it by itself.
static bool wants_lanes(const Plan &p, bool sep_taps, double npts) {
    const int req = p.steps_per_launch_req;
    const bool taps = p.dtype != LORA_BF16 && p.boundary == LORA_BC_REFERENCE && (p.tapset == TAPS3D_STAR || sep_taps);
    if (!taps || p.lanes3 == 0 || (req != 0 && req != 4)) return false;
    // (GStencils/s per launch, tile kernels (two per launch) against this one, tools/cube3d_check.py with the kernel's
    // second form: star 192^3 491 / 347, 224^3 498 / 552, 256^3 554 / 678, 320^3 507 / 881, 384^3 610 / 944; box
    // 224^3 504 / 441, 256^3 494 / 558, 320^3 512 / 765, 384^3 607 / 846; 256 x 512 x 128 444 / 532 and 414 / 442; odd
    // innermost extent 512 x 512 x 511: 126 (one thread per point) / 892.  Below ~10 M points there are too few
    // tiles x chunks for the one workgroup per CU this kernel runs.)
    return req == 4 || p.lanes3 == 1 || npts >= (p.generic ? 1.0e7 : (p.tapset == TAPS3D_STAR ? 1.0e7 : 1.4e7));
}

// bf16: FOUR applications per launch with the levels in registers (kernels_3d_bf16_lanes.hip): exactly separable box
// taps on the vector pipe, reference boundary.  A tile is 56 x 120 output points on one 1024-thread workgroup per
// CU, so the launch wants ~256 tiles x long chunks: by grid size (lanes3 = -1), never (0), always (1);
// steps_per_launch = 4 asks for it by itself.
static bool wants_bf16_lanes(const Plan &p, double npts) {
    const int req = p.steps_per_launch_req;
    if (!(p.dtype == LORA_BF16 && p.tapset == TAPS3D_SEP && p.boundary == LORA_BC_REFERENCE && p.variant != LORA_VARIANT_MFMA &&
          p.lanes3 != 0 && !p.generic && (req == 0 || req == 4)))
        return false;
    // (GStencils/s per launch, this kernel / the two-sweep tile kernel, tools/bf16_crossover.py,
    // profiles/r04_bf16_lanes_crossover.jsonl: 192^3 395 / 501, 256^3 891 / 788, 320^3 1487 / 1104, 512^3 1795 / 1345,
    // 48 x 768^2 1243 / 1123, 96 x 768^2 1561 / 1397, 768^3 2090 / 1662)
    return req == 4 || p.lanes3 == 1 || npts >= 1.2e7;
}

static void resolve_3d(Plan &p) {
    const bool bf16 = p.dtype == LORA_BF16;
    const double npts = (double) p.dims[0] * p.dims[1] * p.dims[2];
    double cba64[9];
    const bool sep_taps = taps_3d(p, cba64);
    // Variant: the matrix-pipe one exists for bf16 box taps with bf16-exact factors, reference boundary, fused launches
    if (p.variant == LORA_VARIANT_MFMA && !mfma3_applies(p)) p.variant = LORA_VARIANT_DIRECT;
    tiles_or_planes(p, sep_taps, cba64, npts);
    bool lanes = wants_lanes(p, sep_taps, npts);
    if (lanes) {
        Plan cand = p;  // the residency query reads the plan it is given: the candidate is a copy, committed if it fits
        cand.lanes3_active = 1;
        cand.steps_per_launch = 4;
        cand.stream3_active = 0;
        if (sep_taps) {
            cand.sep64_valid = 1;
            for (int k = 0; k < 9; ++k) cand.sep64[k] = cba64[k];
        }
        lanes = prepare_3d_lanes(cand);  // false: the device has no room for a workgroup of it: the tile kernels stay
        if (lanes) static_cast<Resolved &>(p) = cand;
    }
    const bool blanes = wants_bf16_lanes(p, npts) && prepare_3d_bf16_lanes(p);
    if (blanes) {
        p.lanes3_active = 1;
        p.steps_per_launch = 4;
    }
    const bool mfma = p.variant == LORA_VARIANT_MFMA;
    p.kernel_name = blanes                            ? kernel_name_3d_bf16_lanes(p)
                    : bf16 && p.steps_per_launch == 2 ? (mfma ? kernel_name_3d_bf16_mfma2(p) : kernel_name_3d_bf16_fused2(p))
                    : bf16                            ? kernel_name_3d_bf16(p)
                    : lanes                           ? kernel_name_3d_lanes(p)
                    : p.generic                       ? kernel_name_generic(p)
                    : p.steps_per_launch == 1         ? kernel_name_3d(p)
                    : p.stream3_active                ? kernel_name_3d_stream(p)
                                                      : kernel_name_3d_fused2(p);
}

// A plan that carries a source (lora_plan_set_source) runs the source kernels and nothing else: two applications per launch
// where source_fuses_two says so, single sweeps otherwise.  Everything a fused family of the plain sweeps resolved is switched
// off again, so that no predicate finds a kernel the plan will not run; the tap set and the taps' factor forms stay.
static void resolve_source(Plan &p) {
    p.steps_per_launch = source_fuses_two(p) ? 2 : 1;
    p.wg_active = 0;
    p.stream3_active = 0;
    p.lanes3_active = 0;
    p.kernel_name = p.steps_per_launch == 2 ? source2_kernel_name(p) : source_kernel_name(p);
}

void plan_refresh(Plan &p) {
    ++p.epoch;
    static_cast<Resolved &>(p) = Resolved{};  // nothing a refresh derives outlives the next one
    if (p.ndim == 1)
        resolve_1d(p);
    else if (p.ndim == 2)
        resolve_2d(p);
    else
        resolve_3d(p);
    if (p.source) resolve_source(p);
}

// ---- options: one row per key -------------------------------------------------------------------------------------------

namespace {
enum Check {
    FLAG,      // any value: stored as 0 / 1
    RANGE,     // v[0] <= value <= v[1]
    ONE_OF,    // one of the n values v[]
    DEPTH,     // steps_per_launch: depth_request_status below
    ABLATE,    // diagnostics builds only
    READ_ONLY  // resolved state, not settable
};
struct Option {
    const char *name;
    int Plan::*set;   // what lora_plan_set_option writes (nullptr: READ_ONLY)
    int Plan::*get;   // what lora_plan_get_option reads: the same field, or the resolved value of a request
    Check check;
    int n;
    int v[4];
    int (*derived)(const Plan &) = nullptr;  // READ_ONLY keys that are no field: computed from the plan on every read
};
constexpr Option flag(const char *name, int Plan::*f) { return {name, f, f, FLAG, 0, {}}; }
constexpr Option range(const char *name, int Plan::*f, int lo, int hi) { return {name, f, f, RANGE, 2, {lo, hi}}; }
constexpr Option read_only(const char *name, int Plan::*f) { return {name, nullptr, f, READ_ONLY, 0, {}}; }

const Option kOptions[] = {
    {"rows_per_thread", &Plan::rows_per_thread, &Plan::rows_per_thread, ONE_OF, 3, {4, 8, 16}},
    range("panel_width", &Plan::panel_width, 1, INT_MAX),
    range("z_chunk", &Plan::z_chunk, 1, INT_MAX),
    flag("nt_store", &Plan::nt_store),
    flag("persistent", &Plan::persistent),
    flag("stream", &Plan::stream2),
    range("stream_rows", &Plan::stream_rows, 0, 1 << 20),
    range("wg", &Plan::wg, -1, 1),
    range("wg_rows", &Plan::wg_rows, 0, 1 << 20),
    range("wg_prio", &Plan::wg_prio, 0, 24),
    range("wg_edge_pct", &Plan::wg_edge_pct, -1, 100),
    range("stream_depth", &Plan::stream_depth, 2, 6),
    range("stream3", &Plan::stream3, -1, 1),
    range("lanes3", &Plan::lanes3, -1, 1),
    {"stream3_waves", &Plan::stream3_waves, &Plan::stream3_waves, ONE_OF, 3, {0, 4, 8}},
    flag("stream3_async", &Plan::stream3_async),
    flag("stream3_pipe", &Plan::stream3_pipe),
    // the ring has kStream3Slots slots (deeper ones measured, no gain)
    {"stream3_slots", &Plan::stream3_slots, &Plan::stream3_slots, ONE_OF, 2, {0, kStream3Slots}},
    flag("stream_share", &Plan::stream_share),
    flag("stream_prefetch", &Plan::stream_prefetch),
    range("stream_sync", &Plan::stream_sync, 0, 2),
    range("scratch", &Plan::use_scratch, -1, 1),
    flag("mfma_split", &Plan::mfma_split),
    range("graph", &Plan::use_graph, -1, 1),
    // 2 / 3: plain / symmetric pyramid form, 4: rank-1 + correction instead of the nested-profile form (A/B timing)
    range("lowrank_valu", &Plan::lowrank_valu, -1, 4),
    range("separable", &Plan::separable, -1, 1),
    // wrong-results timing experiments are not part of the shipped library
    {"ablate", &Plan::ablate, &Plan::ablate, ABLATE, 0, {}},
    flag("lds_dma", &Plan::lds_dma),
    {"cols_per_lane", &Plan::cols_per_lane, &Plan::cols_per_lane, ONE_OF, 2, {4, 8}},
    {"fused_rows", &Plan::fused_rows_req, &Plan::fused_rows, ONE_OF, 4, {0, 6, 8, 10}},
    {"steps_per_launch", &Plan::steps_per_launch_req, &Plan::steps_per_launch, DEPTH, 0, {}},
    flag("fused_pipeline", &Plan::fused_pipeline),
    range("fused_z_chunk", &Plan::fused_z_chunk, 0, 4096),
    // 3D fp64 leapfrog: two steps per launch (lora_plan_leapfrog_depth reads 2); chooses no kernel of the plain sweeps
    flag("leap3", &Plan::leap3),
    // 3D fp64 wave steps: two per launch (lora_plan_wave_depth reads 2); chooses no kernel of the plain sweeps or the leapfrog rules
    flag("wave3", &Plan::wave3),
    // multigrid cycles of this plan run a coarsest level that fits as one launch (lora_plan_cg_small); chooses no kernel of a sweep
    flag("coarse1", &Plan::coarse1),
    // multigrid cycles of this plan restrict a level's defect in the launch that computes it (lora_plan_mg_defect_restrict); chooses
    // no kernel of a sweep
    flag("mgfuse", &Plan::mgfuse),
    range("spans3", &Plan::spans3, -1, 2),
    flag("torus", &Plan::torus),
    read_only("tapset", &Plan::tapset),
    read_only("variant", &Plan::variant),
    read_only("fused_eval", &Plan::fused_eval),
    read_only("boundary", &Plan::boundary),
    // whether lora_plan_residual has a kernel for this plan (no part of the kernel signature or of the resolved state)
    {"fused_residual", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return has_fused_residual(q) ? 1 : 0; }},
    // whether the plan has the conjugate-gradient kernels (lora_plan_apply_dot, lora_plan_cg_update, lora_plan_cg_direction)
    {"cg", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return has_cg(q) ? 1 : 0; }},
    // whether the plan has the multigrid transfer kernels and the V-cycle driver (lora_plan_mg_restrict, lora_plan_run_mg_until)
    {"mg", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return has_mg(q) ? 1 : 0; }},
    // whether the plan has the multigrid-preconditioned drivers (lora_plan_mg_precondition, lora_plan_run_pcg_until): as "mg"
    {"pcg", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return has_mg(q) ? 1 : 0; }},
    // whether lora_plan_cg_small takes the plan: a CG plan of a 2D / 3D shape whose cells and LDS need fit one workgroup
    {"cg_small", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return has_cg_small(q) ? 1 : 0; }},
    // whether the plan carries a source (lora_plan_set_source)
    {"source", nullptr, nullptr, READ_ONLY, 0, {}, [](const Plan &q) { return q.source ? 1 : 0; }},
};

const Option *find_option(const char *key) {
    for (const Option &o : kOptions)
        if (!std::strcmp(key, o.name)) return &o;
    return nullptr;
}

// steps_per_launch = value: 0 (auto), 1 and the depths some kernel family has -- powers of two up to max_depth, 3 (3D fp64
// plane-streaming kernel), 6 (2D workgroup-row kernel); 4 in 3D asks for the register-resident kernels
int depth_request_status(const Plan &p, int value) {
    const bool three = value == 3 && p.ndim == 3 && p.dtype != LORA_BF16;
    const bool six = value == 6 && p.ndim == 2;
    if (value < 0 || value > max_depth(1) || ((value & (value - 1)) && !three && !six)) return LORA_EINVAL;
    if (value > max_depth(p.ndim)) return LORA_EUNSUPPORTED;
    // As found, this site judges odd innermost extents by other terms than has_fused_kernels(p) does: in 2D it does not
    // look at the boundary (a Dirichlet plan takes the request and resolves to single sweeps); in 3D it looks at the
    // request (4 turns the register-resident kernels on) where the resolved state may already have them on (2 is refused)
    const bool odd_ok = p.ndim == 2 ? p.stream2 != 0 : value == 4;
    if (value >= 2 && !has_fused_kernels(p, odd_ok)) return LORA_EUNSUPPORTED;
    return LORA_OK;
}
}  // namespace

}  // namespace lora

using lora::Plan;

extern "C" {

int lora_plan_create(lora_plan **out, int shape, int dtype, const int *dims, const double *params) {
    if (!out || !dims) return LORA_EINVAL;
    *out = nullptr;
    const int nd = lora::shape_ndim(shape);
    if (nd == 0 || (dtype != LORA_F64 && dtype != LORA_BF16)) return LORA_EINVAL;
    if (dtype == LORA_BF16 && nd != 3) {
        lora::set_last_error_text("bf16 is implemented for the 3D shapes only");
        return LORA_EUNSUPPORTED;
    }
    if (dtype == LORA_BF16 && (dims[2] & 7)) {
        lora::set_last_error_text("bf16 grids need an innermost extent that is a multiple of 8");
        return LORA_EUNSUPPORTED;
    }
    for (int d = 0; d < nd; ++d)
        if (dims[d] <= 0) return LORA_EINVAL;
    // 2D/3D rows are read and written in 16-byte pieces by the tiled kernels; an odd innermost extent falls back to
    // the generic one-thread-per-point kernels (fp64 only)
    const bool odd_inner = nd >= 2 && (dims[nd - 1] & 1);
    if (odd_inner && dtype != LORA_F64) {
        lora::set_last_error_text("innermost extent must be even");
        return LORA_EUNSUPPORTED;
    }
    if ((double) lora_padded_count(shape, dims) >= 2147483647.0 * 64) return LORA_EUNSUPPORTED;
    if (nd == 1 && dims[0] > 2147483647 - 8) {
        lora::set_last_error_text("1D extent too large (kernels index the padded array with 32-bit integers)");
        return LORA_EUNSUPPORTED;
    }
    lora_plan *pl = new (std::nothrow) lora_plan();
    if (!pl) return LORA_ENOMEM;
    Plan &p = pl->p;
    p.shape = shape;
    p.ndim = nd;
    p.dtype = dtype;
    for (int d = 0; d < nd; ++d) p.dims[d] = dims[d];
    p.ntaps = lora::shape_ntaps(shape);
    double tmp[49];
    if (!params) {
        lora::default_params(shape, tmp);
        params = tmp;
    }
    lora::effective_weights(shape, params, p.w);
    if (lora::g_default_normalize) {  // normalised-weights mode: the operator's taps divided by their sum
        double sum = 0.0;
        for (int k = 0; k < p.ntaps; ++k) sum += p.w[k];
        if (sum != 0.0 && std::isfinite(sum))
            for (int k = 0; k < p.ntaps; ++k) p.w[k] /= sum;
    }
    p.variant = LORA_VARIANT_DIRECT;
    p.generic = odd_inner;
    p.boundary = lora::g_default_boundary;
    p.leap3 = lora::g_default_leap3;
    p.wave3 = lora::g_default_wave3;
    p.coarse1 = lora::g_default_coarse1;
    p.mgfuse = lora::g_default_mgfuse;
    if (nd == 3) {
        // enough workgroups to fill 256 CUs a few times over, chunks as long as that allows
        const long tiles = (long) ((dims[2] + 127) / 128) * ((dims[1] + 15) / 16);
        int zc = 16;
        while (zc > 4 && tiles * ((dims[0] + zc - 1) / zc) < 2048) zc = (zc == 16) ? 7 : 4;
        p.z_chunk = zc;
    }
    lora::plan_refresh(p);
    if (p.boundary == LORA_BC_PERIODIC && lora_plan_set_boundary(pl, LORA_BC_PERIODIC) != LORA_OK) {
        delete pl;
        return LORA_EUNSUPPORTED;
    }
    *out = pl;
    return LORA_OK;
}

void lora_plan_destroy(lora_plan *plan) {
    if (plan) lora::release_run_state(plan);
    delete plan;
}

int lora_plan_set_weights(lora_plan *plan, const double *weights, int count) {
    if (!plan || !weights || count != plan->p.ntaps) return LORA_EINVAL;
    std::memcpy(plan->p.w, weights, sizeof(double) * count);
    lora::plan_refresh(plan->p);
    return LORA_OK;
}

int lora_plan_get_weights(const lora_plan *plan, double *weights, int count) {
    if (!plan || !weights || count != plan->p.ntaps) return LORA_EINVAL;
    std::memcpy(weights, plan->p.w, sizeof(double) * count);
    return LORA_OK;
}

int lora_set_default_boundary(int boundary) {
    const int old = lora::g_default_boundary;
    if (boundary >= LORA_BC_REFERENCE && boundary <= LORA_BC_PERIODIC) lora::g_default_boundary = boundary;
    return old;
}

int lora_set_default_normalize(int on) {
    const int old = lora::g_default_normalize;
    lora::g_default_normalize = on ? 1 : 0;
    return old;
}

int lora_set_default_leap3(int on) {
    const int old = lora::g_default_leap3;
    lora::g_default_leap3 = on ? 1 : 0;
    return old;
}

int lora_set_default_wave3(int on) {
    const int old = lora::g_default_wave3;
    lora::g_default_wave3 = on ? 1 : 0;
    return old;
}

int lora_set_default_coarse1(int on) {
    const int old = lora::g_default_coarse1;
    lora::g_default_coarse1 = on ? 1 : 0;
    return old;
}

int lora_set_default_mgfuse(int on) {
    const int old = lora::g_default_mgfuse;
    lora::g_default_mgfuse = on ? 1 : 0;
    return old;
}

int lora_plan_set_boundary(lora_plan *plan, int boundary) {
    if (!plan || boundary < LORA_BC_REFERENCE || boundary > LORA_BC_PERIODIC) return LORA_EINVAL;
    if (boundary == LORA_BC_PERIODIC) {
        static const int h1[1] = {4}, h2[2] = {4, 4}, h3[3] = {1, 2, 4};
        const int *h = plan->p.ndim == 1 ? h1 : (plan->p.ndim == 2 ? h2 : h3);
        for (int d = 0; d < plan->p.ndim; ++d)
            if (plan->p.dims[d] < h[d]) {
                lora::set_last_error_text("periodic boundary needs every extent >= its halo width");
                return LORA_EUNSUPPORTED;
            }
    }
    plan->p.boundary = boundary;
    lora::plan_refresh(plan->p);  // the boundary option decides how many applications a launch may fuse
    return LORA_OK;
}

int lora_plan_set_variant(lora_plan *plan, int variant) {
    if (!plan) return LORA_EINVAL;
    if (variant == LORA_VARIANT_AUTO) variant = LORA_VARIANT_DIRECT;
    if (variant != LORA_VARIANT_DIRECT && variant != LORA_VARIANT_MFMA) return LORA_EINVAL;
    if (variant == LORA_VARIANT_MFMA && plan->p.source) {
        lora::set_last_error_text("a plan with a source has no matrix-pipe kernels: remove the source first");
        return LORA_EUNSUPPORTED;
    }
    if (variant == LORA_VARIANT_MFMA && plan->p.ndim == 3) {
        // bf16 box taps: in-plane passes on v_mfma_f32_16x16x32_bf16 (kernels_3d_bf16_mfma.hip)
        if (!lora::mfma3_applies(plan->p)) {
            lora::set_last_error_text("the bf16 MFMA variant takes separable box taps with bf16-exact factors, reference boundary, fused launches");
            return LORA_EUNSUPPORTED;
        }
    } else if (variant == LORA_VARIANT_MFMA && plan->p.ndim != 2) {
        return LORA_EUNSUPPORTED;
    } else if (variant == LORA_VARIANT_MFMA && !plan->p.lowrank_valid) {
        lora::set_last_error_text("these taps have no rank<=3 + sparse-residual factorisation");
        return LORA_EUNSUPPORTED;
    }
    plan->p.variant = variant;
    lora::plan_refresh(plan->p);
    return LORA_OK;
}

int lora_plan_set_source(lora_plan *plan, const void *d_source) {
    if (!plan) return LORA_EINVAL;
    Plan &p = plan->p;
    if (d_source) {
        if (reinterpret_cast<uintptr_t>(d_source) & 15) {
            lora::set_last_error_text("device buffers must be 16-byte aligned");
            return LORA_EUNSUPPORTED;
        }
        if (p.dtype == LORA_BF16) {
            lora::set_last_error_text("bf16 plans take no source");
            return LORA_EUNSUPPORTED;
        }
        if (p.ndim == 2 && p.variant == LORA_VARIANT_MFMA) {
            lora::set_last_error_text("the 2D matrix-pipe variant takes no source");
            return LORA_EUNSUPPORTED;
        }
    }
    p.source = d_source;  // borrowed: the plan owns no grid memory
    lora::plan_refresh(p);  // bumps the epoch: a cached graph holds the old pointer
    return LORA_OK;
}

int lora_plan_set_option(lora_plan *plan, const char *key, int value) {
    if (!plan || !key) return LORA_EINVAL;
    Plan &p = plan->p;
    const lora::Option *o = lora::find_option(key);
    if (!o) return LORA_EINVAL;
    switch (o->check) {
        case lora::FLAG:
            value = value ? 1 : 0;
            break;
        case lora::RANGE:
            if (value < o->v[0] || value > o->v[1]) return LORA_EINVAL;
            break;
        case lora::ONE_OF:
            if (std::find(o->v, o->v + o->n, value) == o->v + o->n) return LORA_EINVAL;
            break;
        case lora::DEPTH:
            if (int rc = lora::depth_request_status(p, value)) return rc;
            break;
        case lora::ABLATE:
#ifdef LORA_DIAGNOSTICS
            value &= 63;
            break;
#else
            lora::set_last_error_text("option \"ablate\" exists only in -DLORA_DIAGNOSTICS builds");
            return LORA_EINVAL;
#endif
        case lora::READ_ONLY:
            return LORA_EINVAL;
    }
    p.*(o->set) = value;
    lora::plan_refresh(p);
    return LORA_OK;
}

int lora_plan_get_option(const lora_plan *plan, const char *key, int *value) {
    if (!plan || !key || !value) return LORA_EINVAL;
    const lora::Option *o = lora::find_option(key);
    if (!o) return LORA_EINVAL;
#ifndef LORA_DIAGNOSTICS
    if (o->check == lora::ABLATE) return LORA_EINVAL;
#endif
    *value = o->derived ? o->derived(plan->p) : plan->p.*(o->get);
    return LORA_OK;
}

size_t lora_plan_padded_bytes(const lora_plan *plan) {
    if (!plan) return 0;
    return lora_padded_count(plan->p.shape, plan->p.dims) * (plan->p.dtype == LORA_BF16 ? 2 : sizeof(double));
}

const char *lora_plan_kernel_name(const lora_plan *plan) { return plan ? plan->p.kernel_name.c_str() : ""; }

const char *lora_plan_kernel_signature(const lora_plan *plan) {
    if (!plan) return "";
    const Plan &p = plan->p;
    static thread_local std::string sig;
    char buf[256];
    const std::string &k = p.kernel_name;
    buf[0] = 0;
    if (k == "stencil2d_stream_kernel") {
        const int K = p.steps_per_launch, w = lora::stream_strip_width(K);
        const int depth = p.boundary == LORA_BC_DIRICHLET ? 4 : (K == 4 ? (p.stream_depth == 2 ? 2 : 3) : p.stream_depth);
        std::snprintf(buf, sizeof buf, "eval=%d,k=%d,depth=%d,sync=%d%s,rows=%d,bc=%d", p.fused_eval, K, depth, p.stream_sync,
                      p.stream_share ? ",share=1" : ((K == 4 && p.stream_sync == 1 && p.stream_prefetch) ? ",pf=1" : ""),
                      lora::stream_rows_per_chunk(p, K, p.dims[0], (p.dims[1] + w - 1) / w), p.boundary);
    } else if (k == "stencil2d_wg_kernel")
        std::snprintf(buf, sizeof buf, "eval=%d,k=%d,rows=%d,edge=%d,prio=%d,bc=%d", p.fused_eval, p.steps_per_launch, p.wg_rows,
                      p.wg_edge_pct, p.wg_prio, p.boundary);
    else if (k == "stencil2d_fused2_kernel")
        std::snprintf(buf, sizeof buf, "eval=%d,rows=%d,persist=%d,panel=%d,bc=%d", p.fused_eval, p.fused_rows,
                      p.persistent, p.panel_width, p.boundary);
    else if (k == "stencil2d_direct_kernel")
        std::snprintf(buf, sizeof buf, "taps=%d,rpt=%d,nt=%d,panel=%d", p.tapset, p.rows_per_thread, p.nt_store,
                      p.panel_width);
    else if (k == "stencil2d_mfma_kernel")
        std::snprintf(buf, sizeof buf, "rank=%d,panel=%d", p.lowrank.rank, p.panel_width);
    else if (k == "stencil3d_lanes_kernel")
        std::snprintf(buf, sizeof buf, "taps=%d,k=%d,fzc=%d,sp=%d,bc=%d", p.sep64_valid ? 2 : p.tapset, p.steps_per_launch,
                      p.fused_z_chunk, p.spans3, p.boundary);
    else if (k == "stencil3d_bf16_lanes_kernel")
        std::snprintf(buf, sizeof buf, "taps=%d,k=%d,fzc=%d,sp=%d,bc=%d", p.tapset, p.steps_per_launch, p.fused_z_chunk, p.spans3,
                      p.boundary);
    else if (k == "stencil3d_planes_kernel") {
        const int K = p.steps_per_launch, pipe = (K == 2 || p.stream3_pipe) ? 1 : 0;
        const int nw = lora::stream3_waves(p, K, pipe);
        if (p.stream3_async && (nw == 8 || nw == 4))  // the launcher's own condition (kernels_3d_planes.hip)
            std::snprintf(buf, sizeof buf, "taps=%d,k=%d,waves=%d,async=1,fzc=%d,bc=%d", p.tapset, K, nw, p.fused_z_chunk,
                          p.boundary);
        else
            std::snprintf(buf, sizeof buf, "taps=%d,k=%d,waves=%d,slots=%d,pipe=%d,fzc=%d,bc=%d", p.sep64_valid ? 2 : p.tapset, K,
                          nw, lora::kStream3Slots, pipe, p.fused_z_chunk, p.boundary);
    } else if (p.ndim == 3 && p.dtype == LORA_BF16)
        std::snprintf(buf, sizeof buf, "taps=%d,zc=%d,fzc=%d,cpl=%d,dma=%d,pipe=%d,bc=%d", p.tapset, p.z_chunk,
                      p.fused_z_chunk, p.cols_per_lane, p.lds_dma, p.fused_pipeline, p.boundary);
    else if (p.ndim == 3)
        std::snprintf(buf, sizeof buf, "taps=%d,zc=%d,fzc=%d,bc=%d", p.tapset, p.z_chunk, p.fused_z_chunk, p.boundary);
    else if (p.ndim == 1)
        std::snprintf(buf, sizeof buf, "k=%d", p.steps_per_launch);
    if (p.source) {  // the source kernels: their geometry follows dtype, extents, tap set and boundary alone
        if (p.ndim == 1)
            std::snprintf(buf, sizeof buf, "src=1");
        else if (k == "stencil2d_source2_kernel")
            std::snprintf(buf, sizeof buf, "taps=%d,k=2,bc=%d,src=1", p.tapset, p.boundary);
        else
            std::snprintf(buf, sizeof buf, "taps=%d,src=1", p.tapset);
    }
    sig = k + "[" + buf + "]";
    return sig.c_str();
}

int lora_plan_region_granularity(const lora_plan *plan) { return plan ? lora::region_granularity(plan->p) : 0; }

}  // extern "C"
