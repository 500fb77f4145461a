"""GPU tests that pin which neighbour every tap multiplies, and which halo every intermediate level sees, in every launch of
SEVERAL applications -- the sweep kernels that carry the benchmark -- against the exact integer model of tests/stencil_model.py.

Why.  tests/test_gpu_tap_orientation.py pins the single-launch entries and none of the multi-sweep kernels; the tests of
tests/test_gpu_parity.py that run those use the reference's own taps or a scaling of them, tables that every mirror and
transposition maps to themselves (star2d1r, star2d3r, box2d3r: 7 of 7 symmetries, star3d1r 47 of 47, box3d1r 15 of 47).  A
kernel with a mirrored offset table, swapped separable factors a / b / c, or a window shifted the wrong way at one of its K
levels passes them.  Here the taps are tables that no signed axis permutation maps to themselves (stencil_model.ranked_taps,
mod7_taps, sep_k_taps; fingerprint_taps where it stays exact), the data are small integers over the WHOLE padded array (so
every level's halo rule is exercised with non-zero halos), and every partial sum of every level stays below 2**53 --
``stencil_model.assert_exact`` on ``levels_magnitude`` checks that in integers BEFORE the engine is called -- so the fp64
results are exact whatever the summation order and every comparison is ``stencil_model.exactly`` (==).

Yardstick: ``stencil_model.levels`` -- the contract of lora_plan_stepk / lora_plan_stepn_region as include/lorastencil.h states
it: level k = S(level k - 1) on the whole interior, the halo cells of a level 0 at odd k and the source buffer's at even k
(under the Dirichlet option the source buffer's at every level), the result level K on [begin, end).  It shares no code with
the engine or the oracle; tests/test_stencil_model_host.py ties it to the CPU oracle bit for bit.

Buffers as in tests/test_gpu_tap_orientation.py: carved by tests/arena.py at offsets 16 and 240, guard bands NaN, the output
poisoned before each call; after it the guards are intact, the input unchanged bit for bit, and every cell outside the
region's interior still the poison.  Entries called directly: lora_plan_stepn_region at every depth, lora_plan_stepk_region at
the plan's own, lora_plan_step2_region at two (2D / 3D), lora_plan_stepn_region2 for the two register-resident 3D kernels.

Which kernel a launch runs (lorastencil_amd/csrc/capi.cpp, launch_apps; every test asserts the plan's kernel name and depth):
  2D  a plan of six (default) or, under Dirichlet, four: stencil2d_wg_kernel at 6 / 4 / 2; step2_region of such a plan and every
      depth of a plan that asks for four or two: stencil2d_stream_kernel; option stream = 0: stencil2d_fused2_kernel.  The 49-tap
      box under Dirichlet resolves stencil2d_stream_kernel at two.
  3D  steps_per_launch = 4 with the star or the separable box: stencil3d_lanes_kernel at 4 and 2; = 3: stencil3d_planes_kernel
      at 3 and 2; the default of small grids, and the ranked (not separable) box at steps_per_launch = 4:
      stencil3d_fused2_kernel at 2.  bf16: steps_per_launch = 4 with the separable box: stencil3d_bf16_lanes_kernel (tap set 2) at
      4 and 2; the default: stencil3d_bf16_fused2_kernel at 2.
  1D  stencil1d_fusedk_kernel at 2 .. 32.

Shapes, the smallest that reach each path; the tile extents are read from the files that own the kernels:
  kernels_2d_wg.hip      wg_strip_width: 512 - 6 K output columns per strip (476 / 488 / 500); rows in chunks per resident
                         workgroup, the first and last strip's shorter.  (1, 2); (33, 522) a partial second strip; (45, 1006)
                         three strips at every depth -- an interior strip -- whole and [5, 37); (7, 13) odd
  kernels_2d_stream.hip  stream_out_w: 128 - 6 K columns per strip (104 / 116), chunks of 8 rows.  (1, 2); (33, 130);
                         (70, 258) three strips, whole and [5, 37); (7, 13) odd
  kernels_2d_fused.hip   kOutW = 122 columns x fused_rows (6 star / 10) rows.  (1, 2); (33, 130); (70, 258) with [5, 37)
  kernels_3d_lanes.hip   kOutW = 120 columns x 32 - 2 K rows (24 / 28).  (1, 1, 2); (5, 30, 122) partial second tiles;
                         (9, 58, 244) 3 x 3 tiles at both depths, whole, [3, 5) and two end ranges + the middle; (3, 5, 7) odd;
                         every cut: spans3 = -1, 0, 1, 2 and fused_z_chunk = 3
  kernels_3d_planes.hip  kOutW = 60 columns x 64 - 2 (K - 1) rows (60 / 62; 4 waves: 28 / 30), chunks of planes.  (1, 1, 2);
                         (34, 18, 130) three column tiles, whole and [3, 5), also in chunks of 5 planes; (3, 66, 122) a partial
                         second row tile
  kernels_3d_fused.hip   kOutW = 60 columns x 8 RY - 2 rows, chunks of planes: the same three grids
  kernels_3d_bf16_lanes.hip  kOutW = 120 columns x 64 - 2 K rows (56 / 60); bf16 rows are multiples of 8.  (1, 1, 8);
                         (5, 62, 128) partial second tiles; (3, 122, 248) 3 x 3 tiles
  kernels_1d.hip         kFusedOut = 1024 outputs per workgroup.  (2,); (2051,) three workgroups and an odd tail, whole and
                         [510, 1540)
Nothing has more than 2 * 10**5 cells.

Depths with no exact integer table (1D K = 16 and 32: 28**16 > 2**53): gaussian data, the ranked taps divided by their sum,
against ``stencil_model.levels_real`` (the same model in np.longdouble) cell by cell within the DERIVED bound
2 K (n + 1) 2**-53 M_K, n the number of taps and M_K the model on |w| and |u|: each level's sum of n products errs by at most
(n + 1) 2**-53 of its sum of magnitudes in any order with or without FMA, the errors of K levels add through non-negative
magnitudes, and the factor 2 covers the second-order terms.  A swapped pair of taps misses it by ten orders of magnitude.

bf16: every level rounds, so the yardstick is the oracle's bf16 driver bit for bit (tests/test_stencil_model_host.py anchors its
orientation on this table to the model): sep_k_taps / 4096 on data 0 .. 3.

Periodic: one case per dimension, lora_plan_run of 4 + 2 + 1 sweeps with torus = 1 (ghost-extended grid) and 0 (a halo wrap per
sweep) against ``stencil_model.periodic`` (np.roll of the interior).

Negative control, no kernel changed: once per kernel family the engine gets a MIRRORED table (``stencil_model.transform``) and
the comparison with the model of the unmirrored one must fail.

Not here: the structured 2D evaluations (fused_eval 3, 6, 7) accept symmetric tables only -- their orientation cannot be
fingerprinted this way (the asymmetric tables resolve fused_eval 0 / 1 / 2, asserted); the MFMA variants; the slab and block
drivers, which launch these same entries.

MEASURED on the MI355X.  Every case agrees with the model with the kernels as they are (no kernel changed); the file takes about
2 s of wall time; the largest error / bound of the long-double cases is 0.0049.  What the cases resolved
(test_report_what_the_cases_resolved prints it; kernel signature, then the depths launched under that plan):
  wg      diamond, star  reference  stencil2d_wg_kernel[eval=0 | 1,k=6,rows=0,edge=-1,prio=12,bc=0]      6, 4, 2
          box (mod-7)    reference  stencil2d_wg_kernel[eval=2,k=6,...,bc=0]                              6
          box (1 + t)    reference  stencil2d_wg_kernel[eval=2,k=6,...,bc=0]                              4, 2
          diamond, star  dirichlet  stencil2d_wg_kernel[eval=0 | 1,k=4,...,bc=1]                          4, 2
  stream  all three      reference  stencil2d_stream_kernel[eval=0 | 1 | 2,k=4,depth=3,sync=1,rows=8,bc=0]  4, 2
          all three      reference  stencil2d_stream_kernel[eval=...,k=2,depth=4,sync=1,rows=8,bc=0]      2
          all three      dirichlet  stencil2d_stream_kernel[eval=...,k=2,depth=4,sync=1,rows=8,bc=1]      2  (star, diamond: wg = 0)
  tile    all three      both       stencil2d_fused2_kernel[eval=...,rows=10 | 6,persist=0 | 1,panel=32,bc=0 | 1]  2
  lanes   star           reference  stencil3d_lanes_kernel[taps=0,k=4,fzc=0 | 3,sp=-1 | 0 | 1 | 2,bc=0]   4, 2
          separable box  reference  stencil3d_lanes_kernel[taps=2,k=4,...]                                4, 2
  planes  star           both       stencil3d_planes_kernel[taps=0,k=3,waves=8,slots=2,pipe=0,fzc=0 | 5,bc=0 | 1]  3, 2
          ranked box     both       stencil3d_planes_kernel[taps=1,k=3,waves=8,...]                       3, 2
          separable box  both       stencil3d_planes_kernel[taps=2,k=3,waves=4,...]                       3, 2
  fused3  all three      both       stencil3d_fused2_kernel[taps=0 | 1,zc=4,fzc=0 | 5,bc=0 | 1]           2
  1d      1d1r, 1d2r     both       stencil1d_fusedk_kernel[k=8]  8, 4, 2;   stencil1d_fusedk_kernel[k=32]  32, 16
  bf16    separable box  reference  stencil3d_bf16_lanes_kernel[taps=2,k=4,fzc=0,sp=-1,bc=0]              4, 2
                                    stencil3d_bf16_fused2_kernel[taps=2 | 1,zc=4,fzc=0,cpl=4,dma=0,pipe=0,bc=0]  2
With the y and z factors handed to kernels_3d_lanes.hip's separable path swapped in a scratch build, the four separable-box
cases of that kernel here fail, while test_3d_register_resident_kernel_equals_step_by_step and
test_3d_register_resident_kernel_real_data_and_regions of tests/test_gpu_parity.py pass on box3d1r (a = b there).
"""
import functools
import time

import numpy as np
import pytest

import stencil_model as SM
import test_gpu_tap_orientation as T

pytestmark = pytest.mark.gpu

OFFSETS = T.OFFSETS
REF, DIRI = "reference", "dirichlet"


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


@pytest.fixture(scope="module")
def O(engine_built):
    from oracle import oracle

    return oracle


WORST = {"ratio": 0.0}


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_gpu_multisweep_taps.py: {time.perf_counter() - t0:.1f} s wall time; "
          f"largest error / bound of the long-double cases {WORST['ratio']:.3g}")


# ---- tables and data ---------------------------------------------------------------------------------------------------------------
def table(L, shape, name):
    """"ranked": 1 .. n on the support of the shape's own taps; "mod7": the 49-tap box at K = 6; "sepk": the separable box"""
    if name == "mod7":
        return SM.mod7_taps()
    if name == "sepk":
        return SM.sep_k_taps()
    assert name == "ranked"
    return SM.ranked_taps(L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0)


def top_of(w, depth):
    """the largest datum, at most 9, that keeps `depth` applications exact: top * (tap sum) ** depth < 2**53"""
    top = min(9, (SM.EXACT - 1) // int(np.abs(w).sum()) ** depth)
    assert top >= 1, f"tap sum {int(w.sum())} is not exact at depth {depth}"
    return int(top)


@functools.lru_cache(maxsize=None)
def data(shape, dims, top):
    return SM.data_small(shape, dims, SM.seed_of("multisweep", shape, dims, top), top)


_MODEL = {}


def model(shape, dims, w, top, K, dirichlet):
    """level K of the contract on the whole interior, computed once per case and shared; exactness checked first"""
    key = (shape, dims, tuple(int(x) for x in w), top, K, dirichlet)
    if key not in _MODEL:
        u = data(shape, dims, top)
        SM.assert_exact(f"{shape} {dims} K = {K}", SM.levels_magnitude(shape, u, w, K, dirichlet))
        whole = SM.stepn(shape, u, w, K, 0, None, dirichlet)
        whole.setflags(write=False)
        _MODEL[key] = whole
    return _MODEL[key]


def make_plan(L, shape, dims, w, options=(), boundary=REF, dtype="f64"):
    p = L.Plan(shape, dims, dtype=dtype)
    if boundary != REF:
        p.set_boundary(boundary)
    for key, value in options:
        p.set_option(key, value)
    return p.set_weights(np.asarray(w, dtype=np.float64))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# (family, shape, table, dims, regions, options, boundary, depths, kernel name, the plan's own depth)
def _c(family, shape, tname, dims, regions, options, boundary, depths, kernel, kplan):
    return (family, shape, tname, tuple(dims), tuple(regions), tuple(options), boundary, tuple(depths), kernel, kplan)


SHAPES_2D = ("star2d1r", "star2d3r", "box2d3r")  # diamond, star, box
EVAL = {"star2d1r": 0, "star2d3r": 1, "box2d3r": 2}  # fused_eval of the asymmetric tables: the direct taps of the tap set
WG, STREAM, TILE = "stencil2d_wg_kernel", "stencil2d_stream_kernel", "stencil2d_fused2_kernel"
LANES, PLANES, FUSED3 = "stencil3d_lanes_kernel", "stencil3d_planes_kernel", "stencil3d_fused2_kernel"
BLANES, BFUSED = "stencil3d_bf16_lanes_kernel", "stencil3d_bf16_fused2_kernel"
K1D = "stencil1d_fusedk_kernel"

GRIDS_WG = (((1, 2), ((0, 1),)), ((33, 522), ((0, 33),)), ((45, 1006), ((0, 45), (5, 37))), ((7, 13), ((0, 7),)))
GRIDS_STREAM = (((1, 2), ((0, 1),)), ((33, 130), ((0, 33),)), ((70, 258), ((0, 70), (5, 37))), ((7, 13), ((0, 7),)))
GRIDS_TILE = GRIDS_STREAM[:3]
GRIDS_LANES = (((1, 1, 2), ((0, 1),)), ((5, 30, 122), ((0, 5),)), ((9, 58, 244), ((0, 9), (3, 5))), ((3, 5, 7), ((0, 3),)))
GRIDS_PLANES = (((1, 1, 2), ((0, 1),)), ((34, 18, 130), ((0, 34), (3, 5))), ((3, 66, 122), ((0, 3),)))
GRIDS_1D = (((2,), ((0, 2),)), ((2051,), ((0, 2051), (510, 1540))))


def even(dims):
    return dims[-1] % 2 == 0


CASES = []
for s in SHAPES_2D:
    for d, r in GRIDS_WG:
        # the workgroup-row kernel under a plan of six: the box at six on the mod-7 table, at four and two on `1 + t`
        if s == "box2d3r":
            CASES.append(_c("wg", s, "mod7", d, r, (), REF, (6,), WG, 6))
            CASES.append(_c("wg", s, "ranked", d, r, (), REF, (4, 2), WG, 6))
        else:
            CASES.append(_c("wg", s, "ranked", d, r, (), REF, (6, 4, 2), WG, 6))
        if even(d):  # (odd innermost extents under Dirichlet: single sweeps of the one-thread-per-point kernel)
            if s == "box2d3r":  # the 49-tap box under Dirichlet: the row-streaming kernel at two
                CASES.append(_c("stream", s, "ranked", d, r, (), DIRI, (2,), STREAM, 2))
            else:
                CASES.append(_c("wg", s, "ranked", d, r, (), DIRI, (4, 2), WG, 4))
    for d, r in GRIDS_STREAM:
        CASES.append(_c("stream", s, "ranked", d, r, (("steps_per_launch", 4),), REF, (4, 2), STREAM, 4))
        CASES.append(_c("stream", s, "ranked", d, r, (("steps_per_launch", 2),), REF, (2,), STREAM, 2))
        if even(d) and s != "box2d3r":
            CASES.append(_c("stream", s, "ranked", d, r, (("wg", 0),), DIRI, (2,), STREAM, 2))
    for d, r in GRIDS_TILE:
        for persistent in (0, 1):
            opts = (("stream", 0), ("steps_per_launch", 2), ("persistent", persistent))
            CASES.append(_c("tile", s, "ranked", d, r, opts, REF, (2,), TILE, 2))
        CASES.append(_c("tile", s, "ranked", d, r, (("stream", 0), ("steps_per_launch", 2)), DIRI, (2,), TILE, 2))
for s, t in (("star3d1r", "ranked"), ("box3d1r", "sepk")):
    for d, r in GRIDS_LANES:
        CASES.append(_c("lanes", s, t, d, r, (("steps_per_launch", 4),), REF, (4, 2), LANES, 4))
for s, t in (("star3d1r", "ranked"), ("box3d1r", "ranked"), ("box3d1r", "sepk")):
    for d, r in GRIDS_PLANES:
        for bc in (REF, DIRI):
            CASES.append(_c("planes", s, t, d, r, (("steps_per_launch", 3),), bc, (3, 2), PLANES, 3))
            CASES.append(_c("fused3", s, t, d, r, (("stream3", 0),), bc, (2,), FUSED3, 2))
    if (s, t) == ("box3d1r", "ranked"):  # not separable: steps_per_launch = 4 must land on the tile kernel at two
        CASES.append(_c("fused3", s, t, (34, 18, 130), ((0, 34),), (("steps_per_launch", 4),), REF, (2,), FUSED3, 2))
    CASES.append(_c("planes", s, t, (34, 18, 130), ((0, 34), (3, 5)), (("steps_per_launch", 3), ("fused_z_chunk", 5)), REF, (3, 2), PLANES, 3))
    CASES.append(_c("fused3", s, t, (34, 18, 130), ((0, 34), (3, 5)), (("stream3", 0), ("fused_z_chunk", 5)), REF, (2,), FUSED3, 2))
for s in ("1d1r", "1d2r"):
    for d, r in GRIDS_1D:
        for bc in (REF, DIRI):
            CASES.append(_c("1d", s, "ranked", d, r, (("steps_per_launch", 8),), bc, (8, 4, 2), K1D, 8))

# how a launch of the register-resident kernels is cut along z: the plan's own rule, equal chunks, spans, team spans, fixed chunks
CUTS = ((("spans3", -1), ("fused_z_chunk", 0)), (("spans3", 0), ("fused_z_chunk", 0)), (("spans3", 1), ("fused_z_chunk", 0)),
        (("spans3", 2), ("fused_z_chunk", 0)), (("spans3", -1), ("fused_z_chunk", 3)))


def case_id(c):
    opts = ",".join(f"{k}={v}" for k, v in c[5])
    return f"{c[0]}-{c[1]}-{c[2]}-{'x'.join(map(str, c[3]))}-{c[6]}" + (f"-{opts}" if opts else "")


def entries(plan, K, kplan, nd):
    """(name, call) of the entries that launch K applications of this plan over [lo, hi)"""
    out = [("stepn_region", lambda src, dst, lo, hi: plan.stepn_region(K, src, dst, lo, hi))]
    if K == kplan:
        out.append(("stepk_region", lambda src, dst, lo, hi: plan.stepk_region(src, dst, lo, hi)))
    if K == 2 and nd != 1:
        out.append(("step2_region", lambda src, dst, lo, hi: plan.step2_region(src, dst, lo, hi)))
    return out


def check_launch(g, call, lo, hi, want, what):
    g.arena.fill_poison(1)
    call(g.v[0], g.v[1], lo, hi)
    g.guards(what)
    T.inputs_unchanged(g, (0,), what)
    T.check_cells(g, 1, lo, hi, want, what)


RESOLVED_SEEN = {}


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_k_applications_in_one_launch(L, case):
    family, shape, tname, dims, regions, options, boundary, depths, kernel, kplan = case
    nd = len(dims)
    w = table(L, shape, tname)
    top = top_of(w, max(depths))
    u = data(shape, dims, top)
    plan = make_plan(L, shape, dims, w, options, boundary)
    resolved = (plan.kernel_name, plan.get_option("steps_per_launch"))
    assert resolved == (kernel, kplan), f"{case_id(case)}: the plan resolved {plan.kernel_signature} at depth {resolved[1]}"
    if nd == 2:
        assert plan.get_option("fused_eval") == EVAL[shape], "an asymmetric table must resolve the direct taps of its tap set"
    if (shape, tname) == ("box3d1r", "sepk") and family in ("lanes", "planes"):
        assert "taps=2" in plan.kernel_signature, f"the separable path was not taken: {plan.kernel_signature}"
    RESOLVED_SEEN.setdefault((family, shape, tname, boundary, plan.kernel_signature), depths)
    dirichlet = boundary == DIRI
    want = {K: model(shape, dims, w, top, K, dirichlet) for K in depths}
    for cut in (CUTS if family == "lanes" else ((),)):
        for key, value in cut:
            plan.set_option(key, value)
        assert plan.kernel_name == kernel and plan.get_option("steps_per_launch") == kplan
        for off in OFFSETS:
            g = T.grids(L, shape, dims, off, [u, None])
            for K in depths:
                for lo, hi in regions:
                    for name, call in entries(plan, K, kplan, nd):
                        what = f"{name} K = {K} {case_id(case)} {dict(cut)} [{lo}, {hi}) offset {off}"
                        check_launch(g, call, lo, hi, want[K][lo:hi], what)
                if family == "lanes" and dims[0] >= 9:
                    # two end ranges in ONE launch of the register-resident kernel, then the middle
                    h = dims[0]
                    for b0, e0, b1, e1 in ((0, 2, h - 3, h), (h - 4, h, 0, 1)):
                        what = f"stepn_region2 K = {K} {case_id(case)} {dict(cut)} [{b0}, {e0}) + [{b1}, {e1}) offset {off}"
                        g.arena.fill_poison(1)
                        plan.stepn_region2(K, g.v[0], g.v[1], b0, e0, b1, e1)
                        plan.stepn_region(K, g.v[0], g.v[1], min(e0, e1), max(b0, b1))
                        g.guards(what)
                        T.inputs_unchanged(g, (0,), what)
                        T.check_cells(g, 1, 0, h, want[K], what)


# ---- 1D at sixteen and thirty-two applications: no integer table stays exact --------------------------------------------------------
@pytest.mark.parametrize("boundary", [REF, DIRI])
@pytest.mark.parametrize("shape", ["1d1r", "1d2r"])
def test_1d_deep_launches_against_the_long_double_model(L, shape, boundary):
    dims, regions = GRIDS_1D[1]
    wi = table(L, shape, "ranked")
    ntaps = int(np.count_nonzero(wi))
    w = wi.astype(np.float64) / float(wi.sum())
    u = np.random.default_rng(SM.seed_of("1d deep", shape)).standard_normal(SM.padded_shape(shape, dims))
    plan = make_plan(L, shape, dims, w, (("steps_per_launch", 32),), boundary)
    assert (plan.kernel_name, plan.get_option("steps_per_launch")) == (K1D, 32)
    dirichlet = boundary == DIRI
    for K in (32, 16):
        exact = SM.levels_real(shape, u, w, K, dirichlet)
        bound = 2.0 * K * (ntaps + 1) * 2.0 ** -53 * SM.levels_real(shape, np.abs(u), np.abs(w), K, dirichlet).astype(np.float64)
        assert (bound > 0).all()
        for off in OFFSETS:
            g = T.grids(L, shape, dims, off, [u, None])
            for lo, hi in regions:
                what = f"stepn_region K = {K} {shape} {dims} {boundary} [{lo}, {hi}) offset {off}"
                g.arena.fill_poison(1)
                plan.stepn_region(K, g.v[0], g.v[1], lo, hi)
                g.guards(what)
                T.inputs_unchanged(g, (0,), what)
                m = g.region(lo, hi)
                got = g.v[1][m].cpu().numpy()
                assert bool(g.arena.is_poison(1)[~m].all()), f"{what}: a cell outside the region's interior was written"
                assert np.isfinite(got).all(), f"{what}: a NaN reached a result"
                err = np.abs(got.astype(np.longdouble) - exact[lo:hi]).astype(np.float64)
                ratio = float((err / bound[lo:hi]).max())
                WORST["ratio"] = max(WORST["ratio"], ratio)
                print(what, "largest error / bound", ratio)
                assert ratio <= 1.0, f"{what}: {int((err > bound[lo:hi]).sum())} cells are further from the long-double model than the bound"
        # the comparison has teeth: the model of the mirrored table is far outside the bound
        mirrored = SM.levels_real(shape, u, w[::-1].copy(), K, dirichlet)
        assert float((np.abs(mirrored - exact).astype(np.float64) / bound).max()) > 1e6


# ---- bf16: bit for bit against the oracle's bf16 driver ---------------------------------------------------------------------------
class Bf16Grids:
    """a source and an output grid of bf16 bit patterns carved from one poisoned allocation"""

    def __init__(self, L, shape, dims, off, bits):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, tuple(dims)
        self.arena = carve(L.padded_shape(shape, dims), "bf16", n_buffers=2, offset_bytes=off)
        self.v = self.arena.views
        self.arena.bits(0).copy_(torch.from_numpy(bits.view(np.int16).copy()))
        self.before = self.arena.bits(0).clone()
        self.mask = torch.zeros(self.v[0].shape, dtype=torch.bool, device="cuda")

    def region(self, lo, hi):
        self.mask.zero_()
        self.L.interior(self.shape, self.mask)[lo:hi] = True
        return self.mask

    def check(self, lo, hi, want_padded, what):
        """after a launch into grid 1: guards, input, the cells of [lo, hi) against the oracle's padded result, the rest poison"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        assert torch.equal(self.arena.bits(0), self.before), f"{what}: the input grid was written"
        m = self.region(lo, hi)
        got = self.arena.bits(1)[m].cpu().numpy().view(np.uint16)
        want = want_padded[m.cpu().numpy()]
        assert bool(self.arena.is_poison(1)[~m].all()), f"{what}: a cell outside the region's interior was written"
        return got, want


GRIDS_BF16 = (((1, 1, 8), ((0, 1),)), ((5, 62, 128), ((0, 5),)), ((3, 122, 248), ((0, 3), (1, 2))))
# (options, depths, kernel, plan depth, the oracle's `separable`)
BF16 = [((("steps_per_launch", 4),), (4, 2), BLANES, 4, True), ((), (2,), BFUSED, 2, True), ((("separable", 0),), (2,), BFUSED, 2, False)]


def bf16_taps():
    return SM.sep_k_taps().astype(np.float64) / 4096.0  # sum 0.75: the levels stay of order one


@pytest.mark.parametrize("options,depths,kernel,kplan,separable", BF16, ids=["lanes", "fused2", "fused2-tap-order"])
@pytest.mark.parametrize("dims,regions", GRIDS_BF16, ids=["x".join(map(str, d)) for d, _ in GRIDS_BF16])
def test_bf16_k_applications_against_the_oracle(L, O, dims, regions, options, depths, kernel, kplan, separable):
    shape = "box3d1r"
    w = bf16_taps()
    bits = O.to_bf16(data(shape, dims, 3))
    plan = make_plan(L, shape, dims, w, options, dtype="bf16")
    assert (plan.kernel_name, plan.get_option("steps_per_launch")) == (kernel, kplan), plan.kernel_signature
    assert plan.get_option("tapset") == (2 if separable else 1), plan.kernel_signature
    RESOLVED_SEEN.setdefault(("bf16", shape, "sepk / 4096", REF, plan.kernel_signature), depths)
    for K in depths:
        want = O.run_bf16(shape, bits, K, weights=w, separable=separable)
        for off in OFFSETS:
            g = Bf16Grids(L, shape, dims, off, bits)
            for lo, hi in regions:
                for name, call in entries(plan, K, kplan, 3):
                    what = f"{name} K = {K} bf16 {dims} {dict(options)} [{lo}, {hi}) offset {off}"
                    g.arena.fill_poison(1)
                    call(g.v[0], g.v[1], lo, hi)
                    got, exp = g.check(lo, hi, want, what)
                    assert np.array_equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.size} cells differ from the bf16 oracle"
            if kernel == BLANES and dims[0] >= 3:
                h = dims[0]
                what = f"stepn_region2 K = {K} bf16 {dims} [0, 1) + [{h - 1}, {h}) offset {off}"
                g.arena.fill_poison(1)
                plan.stepn_region2(K, g.v[0], g.v[1], 0, 1, h - 1, h)
                plan.stepn_region(K, g.v[0], g.v[1], 1, h - 1)
                got, exp = g.check(0, h, want, what)
                assert np.array_equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.size} cells differ from the bf16 oracle"


# ---- periodic runs: one full launch, one tail, one single sweep ------------------------------------------------------------------------
PERIODIC = [("1d1r", (2051,)), ("star2d3r", (33, 130)), ("star3d1r", (9, 18, 130))]


@pytest.mark.parametrize("torus", [1, 0])
@pytest.mark.parametrize("shape,dims", PERIODIC, ids=[s for s, _ in PERIODIC])
def test_periodic_runs_against_the_rolled_model(L, shape, dims, torus):
    """lora_plan_run of 4 + 2 + 1 sweeps under the periodic boundary with steps_per_launch = 4 (the ranked tables stay exact for
    seven sweeps, not for the 6 + 4 + 1 of the 2D default): fused launches on the ghost-extended grid (torus = 1) or a halo wrap
    per sweep (0).  The interior against np.roll of the interior, seven times."""
    import torch
    from arena import assert_guards_intact

    times = 7
    w = table(L, shape, "ranked")
    top = top_of(w, times)
    u = data(shape, dims, top)
    SM.assert_exact(f"{shape} {dims} periodic", SM.periodic_magnitude(shape, u, w, times))
    want = SM.periodic(shape, u, w, times)
    plan = make_plan(L, shape, dims, w, (("steps_per_launch", 4), ("torus", torus)), "periodic")
    assert plan.get_option("boundary") == 2 and plan.get_option("torus") == torus, plan.kernel_signature
    for off in OFFSETS:
        g = T.grids(L, shape, dims, off, [u, None])
        what = f"run {times} periodic torus = {torus} {shape} {dims} offset {off}"
        plan.run(g.v[0], g.v[1], times)
        torch.cuda.synchronize()
        assert_guards_intact(g.arena, what)
        got = g.host(times % 2)
        if not SM.exactly(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what}: {len(bad)} of {want.size} cells differ from the periodic model, the first at {tuple(bad[0])}: "
                                 f"engine {got[tuple(bad[0])]!r}, model {int(want[tuple(bad[0])])}")


# ---- negative control: the comparison is not vacuous ---------------------------------------------------------------------------------
def _mirror(w):
    nd = {9: 1, 49: 2, 27: 3}[w.size]
    return SM.transform(w, tuple(range(nd)), (0,) * (nd - 1) + (1,))  # the innermost axis mirrored


def _first(family, tname, dims):
    return next(c for c in CASES if (c[0], c[2], c[3], c[6]) == (family, tname, dims, REF))


# one case per kernel family, the register-resident and plane-streaming kernels on both of their evaluations
CONTROL = [_first("wg", "ranked", (33, 522)), _first("stream", "ranked", (33, 130)), _first("tile", "ranked", (33, 130)),
           _first("lanes", "ranked", (5, 30, 122)), _first("lanes", "sepk", (5, 30, 122)), _first("planes", "ranked", (34, 18, 130)),
           _first("planes", "sepk", (34, 18, 130)), _first("fused3", "ranked", (34, 18, 130)), _first("1d", "ranked", (2051,))]


@pytest.mark.parametrize("case", CONTROL, ids=[case_id(c) for c in CONTROL])
def test_a_mirrored_table_fails_the_comparison(L, case):
    family, shape, tname, dims, regions, options, boundary, depths, kernel, kplan = case
    w = table(L, shape, tname)
    mirrored = _mirror(w)
    assert not np.array_equal(mirrored, w)
    top = top_of(w, max(depths))
    u = data(shape, dims, top)
    plan = make_plan(L, shape, dims, mirrored, options, boundary)
    assert (plan.kernel_name, plan.get_option("steps_per_launch")) == (kernel, kplan), plan.kernel_signature
    g = T.grids(L, shape, dims, OFFSETS[0], [u, None])
    for K in depths:
        g.arena.fill_poison(1)
        plan.stepn_region(K, g.v[0], g.v[1], 0, dims[0])
        g.guards(case_id(case))
        got = g.host(1)
        assert not SM.exactly(got, model(shape, dims, w, top, K, False)), f"{case_id(case)} K = {K}: a mirrored table went unnoticed"
        assert SM.exactly(got, SM.stepn(shape, u, mirrored, K, 0, None)), f"{case_id(case)} K = {K}: not the mirrored table's result either"


def test_a_mirrored_table_fails_the_bf16_comparison(L, O):
    shape, (dims, _) = "box3d1r", GRIDS_BF16[1]
    w = bf16_taps()
    mirrored = _mirror(SM.sep_k_taps()).astype(np.float64) / 4096.0
    bits = O.to_bf16(data(shape, dims, 3))
    for options, depths, kernel, kplan, separable in BF16[:2]:
        plan = make_plan(L, shape, dims, mirrored, options, dtype="bf16")
        assert (plan.kernel_name, plan.get_option("steps_per_launch")) == (kernel, kplan), plan.kernel_signature
        g = Bf16Grids(L, shape, dims, OFFSETS[0], bits)
        for K in depths:
            g.arena.fill_poison(1)
            plan.stepn_region(K, g.v[0], g.v[1], 0, dims[0])
            got, exp = g.check(0, dims[0], O.run_bf16(shape, bits, K, weights=w, separable=separable), f"control bf16 K = {K}")
            assert not np.array_equal(got, exp), f"bf16 {kernel} K = {K}: a mirrored table went unnoticed"


def test_report_what_the_cases_resolved():
    """prints the record the header keeps (runs last: the cases above fill it)"""
    for (family, shape, tname, boundary, signature), depths in sorted(RESOLVED_SEEN.items()):
        print(f"{family:7s} {shape:9s} {tname:12s} {boundary:10s} depths {depths}: {signature}")
    assert RESOLVED_SEEN
