"""Hostile memory and plan reuse (GPU): the existing comparisons once more, but on grids that are sub-arrays of one poisoned
allocation (tests/arena.py: 16-byte aligned and no more, NaN guard bands all round), with a poisoned second buffer, with the
written set of every direct launch checked cell by cell, with ONE plan driven through a long sequence of option / tap /
boundary changes and runs, and with two plans in flight at once.

ROWS is the table of configurations; together they reach every kernel the library can launch, and every test asserts through
``kernel_name`` / ``kernel_signature`` that a row lands where it says before it runs.  Each row has a RAGGED size (last tile,
strip or chunk partial in every dimension; taken from the parametrisations of test_gpu_parity.py) and an EXACT one (the
extents end on the kernel's tile boundary: the tile sizes are quoted per row from the kernel sources).

What a result must equal is what test_gpu_parity.py demands of the same configuration: the oracle bit for bit on its integer
inputs while sums are exact (|values| < 2^50) and on bf16 grids, the relative bound of the existing tests afterwards.
A NaN from a guard band fails either comparison.
"""
import threading

import numpy as np
import pytest

import arena as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    assert L.device_count() >= 1
    return L


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O

    return O


def rel_err(got, exp):
    """test_gpu_parity.rel_err: point-wise relative error with a floor of 1e-2 x the largest |exp|."""
    exp = np.asarray(exp, dtype=np.float64)
    scale = np.abs(exp).max()
    if not scale > 0:
        return float(np.abs(got - exp).max())
    return float((np.abs(got - exp) / np.maximum(np.abs(exp), 1e-2 * scale)).max())


MFMA = 2  # LORA_VARIANT_MFMA


class Row:
    def __init__(self, id, shape, ragged, exact, kernel, sig=(), opts=None, dtype="f64", bc=None, variant=None, taps=None,
                 times=(1, 3), step2=True, fused_direct=True):
        self.id, self.shape, self.ragged, self.exact, self.kernel, self.sig = id, shape, ragged, exact, kernel, tuple(sig)
        self.opts, self.dtype, self.bc, self.variant, self.taps, self.times = dict(opts or {}), dtype, bc, variant, taps, times
        self.step2 = step2                # lora_plan_step2 exists for the plan (capi.cpp: has_apps)
        self.fused_direct = fused_direct  # stepk / stepn_region have stated semantics for the plan
        self.ndim = {"1": 1, "2": 2, "3": 3}[[c for c in shape if c.isdigit()][0]]

    def __repr__(self):
        return self.id


# Step counts per depth K of a plan (capi.cpp: run_schedule): full-depth launches, the shallower tails, a single sweep, and an
# odd number (>= 3) of launches, which goes through the plan's scratch grid.
T1 = (1, 3)            # single sweeps
T2 = (4, 7)            # 2 + 2 | 2 + 2 + 2 (scratch) + 1
T3 = (7, 10)           # 3D natural form: 3 + 3 + 1 | 3 + 3 + 2 + 2
T4 = (11, 13)          # 4 + 4 + 2 (scratch) + 1 | 4 + 4 + 4 (scratch) + 1
T4L = (6, 13)          # register-resident kernels: 4 + 2 (their two-application form) | 4 + 4 + 4 (scratch) + 1
T6 = (14, 19, 23)      # 6 + 6 + 2 (scratch) | 6 + 6 + 6 (scratch) + 1 | 6 + 6 + 6 + 4 + 1
T4D = (13, 14)         # Dirichlet, four per launch: 4 + 4 + 4 (scratch) + 1 | 4 + 4 + 4 + 2


def _t1d(k):           # 3 K (scratch) | 4 K + 3: four launches, a tail of two where K > 2, a single sweep
    return (3 * k, 4 * k + 3)


ROWS = [
    # ---- 1D (kernels_1d.hip: a workgroup owns kFusedOut = 1024 outputs; exact: 2048) ----
    Row("1d_single", "1d1r", (4097,), (2048,), "stencil1d_kernel", ["k=1"], {"steps_per_launch": 1}, step2=False),
    *[Row(f"1d_fused{k}", "1d1r" if k != 4 else "1d2r", (5000,), (2048,), "stencil1d_fusedk_kernel", [f"k={k}]"],
          {"steps_per_launch": k}, times=_t1d(k), step2=False) for k in (2, 4, 8, 16, 32)],
    # the run-length dependent depth (8 / 16 from 32 sweeps / 32 from 64): 16 + 16 + 8 (scratch) | 32 + 32 + 32 + 4
    Row("1d_auto", "1d2r", (4097,), (4096,), "stencil1d_fusedk_kernel", ["k=8]"], times=(40, 100), step2=False),
    # ---- 2D single sweeps ----
    # kernels_2d.hip: tile 4 RPT rows x 128 columns (RPT = 8: 32 x 128; 16: 64 x 128, the tallest window staged anywhere)
    Row("2d_direct", "star2d1r", (40, 130), (64, 256), "stencil2d_direct_kernel", ["rpt=8"], {"steps_per_launch": 1}),
    Row("2d_direct_rpt16", "box2d3r", (33, 254), (64, 128), "stencil2d_direct_kernel", ["rpt=16"],
        {"steps_per_launch": 1, "rows_per_thread": 16}),
    # kernels_generic.hip: one thread per point, 64 columns per block; an odd extent cannot end on a column boundary
    Row("2d_generic", "star2d3r", (33, 65), (64, 127), "stencil2d_generic_kernel", [], {"steps_per_launch": 1}),
    # kernels_2d_mfma.hip: 32 x 128 output tile; no fused launches in this variant
    Row("2d_mfma", "box2d3r", (40, 130), (64, 256), "stencil2d_mfma_kernel", [], variant=MFMA, step2=False),
    # ---- 2D tile kernel (kernels_2d_fused.hip: 4 R1 - 6 = 34 rows at fused_rows = 10, 122 columns) ----
    Row("2d_tile", "star2d1r", (53, 246), (68, 244), "stencil2d_fused2_kernel", ["persist=0", "rows=10"],
        {"stream": 0, "steps_per_launch": 2}, times=T2),
    Row("2d_tile_persistent", "box2d3r", (90, 250), (68, 244), "stencil2d_fused2_kernel", ["persist=1"],
        {"stream": 0, "steps_per_launch": 2, "persistent": 1}, times=T2),
    # ---- 2D row-streaming kernel (kernels_2d_stream.hip: strips of 128 - 6 K columns, chunks of 8 rows) ----
    Row("2d_stream4_even", "star2d1r", (53, 246), (64, 208), "stencil2d_stream_kernel", ["k=4"], {"steps_per_launch": 4},
        times=T4),
    # (odd extents: 207 ends one column short of the second strip: the half-valid last pair cut by the store descriptor)
    Row("2d_stream4_odd", "box2d3r", (33, 65), (64, 207), "stencil2d_stream_kernel", ["k=4"], {"steps_per_launch": 4},
        times=T4),
    Row("2d_stream2_even", "star2d3r", (27, 124), (64, 232), "stencil2d_stream_kernel", ["k=2"], {"steps_per_launch": 2},
        times=T2),
    Row("2d_stream2_odd", "star2d1r", (129, 233), (64, 231), "stencil2d_stream_kernel", ["k=2"], {"steps_per_launch": 2},
        times=T2),
    # ---- 2D workgroup-row kernel (kernels_2d_wg.hip: strips of 512 - 6 K columns: 476 / 488 / 500) ----
    Row("2d_wg6", "star2d1r", (53, 246), (64, 476), "stencil2d_wg_kernel", ["k=6", "bc=0"], times=T6),
    Row("2d_wg6_odd", "box2d3r", (20, 131), (64, 475), "stencil2d_wg_kernel", ["k=6"], times=T6),
    Row("2d_wg4", "star2d3r", (53, 246), (64, 488), "stencil2d_wg_kernel", ["k=4", "bc=0"], {"wg": 1, "steps_per_launch": 4},
        times=T4),
    Row("2d_wg2", "star2d1r", (40, 130), (64, 500), "stencil2d_wg_kernel", ["k=2"], {"wg": 1, "steps_per_launch": 2}, times=T2),
    # (lora_plan_step2 is defined on the reference state only -- level-1 halo = 0 -- so it is not launched on this plan)
    Row("2d_wg4_dirichlet", "star2d1r", (53, 246), (64, 488), "stencil2d_wg_kernel", ["k=4", "bc=1"], bc="dirichlet", times=T4D,
        step2=False),
    Row("2d_wg6_short_chunks", "star2d1r", (90, 250), (80, 952), "stencil2d_wg_kernel", ["k=6", "rows=20", "edge=0"],
        {"wg_rows": 20, "wg_edge_pct": 0}, times=T6),
    # a full-rank 49-tap table: the taps one by one (eval = 2), six applications per launch
    Row("2d_wg6_49_taps", "box2d3r", (13, 233), (64, 476), "stencil2d_wg_kernel", ["k=6", "eval=2"], taps="w49", times=(7, 8, 14)),
    # ---- 3D fp64 single sweeps (kernels_3d.hip: 16 x 128 tile, z_chunk planes; kernels_generic.hip) ----
    Row("3d_single", "star3d1r", (33, 19, 258), (8, 16, 128), "stencil3d_stream_kernel", [], {"steps_per_launch": 1, "z_chunk": 4}),
    Row("3d_generic", "box3d1r", (7, 9, 33), (8, 16, 63), "stencil3d_generic_kernel", [], step2=False),
    # ---- 3D tile kernel (kernels_3d_fused.hip: 30 x 60 tile, chunks of up to 32 planes) ----
    Row("3d_tile", "star3d1r", (37, 29, 190), (32, 30, 120), "stencil3d_fused2_kernel", [], {"stream3": 0, "steps_per_launch": 2},
        times=T2),
    # ---- 3D plane-streaming kernel (kernels_3d_planes.hip: 8 NW - 2 (K - 1) rows x 60 columns, ring two planes ahead) ----
    Row("3d_planes_k3_w4", "star3d1r", (37, 29, 190), (32, 28, 120), "stencil3d_planes_kernel", ["k=3", "waves=4"],
        {"steps_per_launch": 3, "stream3_waves": 4}, times=T3),
    Row("3d_planes_k3_w8", "box3d1r", (9, 31, 62), (32, 60, 120), "stencil3d_planes_kernel", ["k=3", "waves=8", "taps=2"],
        {"steps_per_launch": 3, "stream3_waves": 8}, times=T3),
    Row("3d_planes_k2_w4", "box3d1r", (37, 29, 190), (32, 30, 120), "stencil3d_planes_kernel", ["k=2", "waves=4", "taps=2"],
        {"stream3": 1, "steps_per_launch": 2, "stream3_waves": 4}, times=T2),
    Row("3d_planes_k2_w8", "star3d1r", (9, 31, 62), (32, 62, 120), "stencil3d_planes_kernel", ["k=2", "waves=8"],
        {"stream3": 1, "steps_per_launch": 2, "stream3_waves": 8}, times=T2),
    # (the pipelined three-level form fits with 6 waves only: 44 rows)
    Row("3d_planes_pipe", "star3d1r", (37, 29, 190), (32, 44, 120), "stencil3d_planes_kernel", ["k=3", "pipe=1", "waves=6"],
        {"steps_per_launch": 3, "stream3_pipe": 1}, times=T3),
    Row("3d_planes_async", "box3d1r", (37, 29, 190), (32, 28, 120), "stencil3d_planes_kernel", ["k=3", "async=1", "waves=4"],
        {"steps_per_launch": 3, "stream3_async": 1, "stream3_waves": 4}, times=T3),
    Row("3d_planes_27_tap_order", "box3d1r", (9, 31, 62), (32, 62, 120), "stencil3d_planes_kernel", ["k=2", "taps=1", "waves=8"],
        {"stream3": 1, "steps_per_launch": 2, "separable": 0, "stream3_waves": 8}, times=T2),
    # ---- 3D register-resident kernel (kernels_3d_lanes.hip: 24 x 120 tile at K = 4, z streamed one plane ahead) ----
    Row("3d_lanes", "star3d1r", (37, 29, 190), (32, 24, 120), "stencil3d_lanes_kernel", ["k=4", "sp=-1"], {"steps_per_launch": 4},
        times=T4L),
    *[Row(f"3d_lanes_spans{sp}", "box3d1r", (37, 29, 190), (32, 24, 120), "stencil3d_lanes_kernel", ["k=4", f"sp={sp}"],
          {"steps_per_launch": 4, "spans3": sp}, times=T4L) for sp in (0, 1, 2)],
    Row("3d_lanes_z_chunk", "star3d1r", (40, 60, 128), (32, 24, 120), "stencil3d_lanes_kernel", ["k=4", "fzc=3"],
        {"steps_per_launch": 4, "fused_z_chunk": 3}, times=T4L),
    Row("3d_lanes_odd", "box3d1r", (12, 24, 121), (32, 24, 119), "stencil3d_lanes_kernel", ["k=4"], {"steps_per_launch": 4},
        times=T4L),
    # ---- 3D bf16 (kernels_3d_bf16*.hip).  Single sweeps: 16 x 128 tile (256 columns at 8 per lane); fused2: 30 x 120;
    # register-resident: 56 x 120; matrix pipe: 28 x 60 ----
    Row("bf16_single_lds_dma", "box3d1r", (9, 21, 264), (8, 16, 128), "stencil3d_bf16_kernel", ["dma=1", "cpl=4"],
        {"steps_per_launch": 1, "lds_dma": 1}, dtype="bf16"),
    Row("bf16_single_cpl8", "star3d1r", (9, 21, 264), (8, 16, 256), "stencil3d_bf16_kernel", ["dma=0", "cpl=8"],
        {"steps_per_launch": 1, "cols_per_lane": 8}, dtype="bf16"),
    Row("bf16_fused2", "box3d1r", (9, 31, 248), (32, 30, 120), "stencil3d_bf16_fused2_kernel", ["taps=2"], dtype="bf16", times=T2),
    Row("bf16_fused2_star", "star3d1r", (37, 61, 136), (32, 30, 120), "stencil3d_bf16_fused2_kernel", ["taps=0"], dtype="bf16",
        times=T2),
    Row("bf16_lanes", "box3d1r", (9, 31, 248), (32, 56, 120), "stencil3d_bf16_lanes_kernel", ["k=4"], {"steps_per_launch": 4},
        dtype="bf16", times=T4L),
    Row("bf16_mfma", "box3d1r", (9, 31, 248), (32, 28, 120), "stencil3d_bf16_mfma2_kernel", [], dtype="bf16", variant=MFMA,
        times=(4, 5, 9)),
    # ---- periodic runs: fused launches on the ghost-extended grid (torus = 1) and single sweeps behind a wrap (0).  The
    # raw launch entries of a periodic plan other than the single sweep have no stated halo semantics: not launched. ----
    Row("periodic_torus_2d", "star2d1r", (53, 246), (64, 476), "stencil2d_stream_kernel", ["bc=2"], bc="periodic", times=(2, 7, 13),
        step2=False, fused_direct=False),
    Row("periodic_wrap_2d", "box2d3r", (40, 130), (64, 256), "stencil2d_stream_kernel", ["bc=2"], {"torus": 0}, bc="periodic",
        times=(2, 7), step2=False, fused_direct=False),
    Row("periodic_torus_3d", "star3d1r", (9, 20, 136), (32, 24, 120), "stencil3d_fused2_kernel", ["bc=2"], bc="periodic",
        times=(2, 7, 13), step2=False, fused_direct=False),
    Row("periodic_torus_1d", "1d1r", (4097,), (4096,), "stencil1d_fusedk_kernel", ["k=8]"], bc="periodic", times=(7, 40),
        step2=False, fused_direct=False),
]
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROWS)


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _weights(O, row):
    """The taps given to set_weights (None: the plan's own, from the reference harness's params table)."""
    if row.dtype == "bf16":  # (the reference taps overflow bf16 within a few sweeps: normalised, as the existing bf16 tests)
        w = O.effective_weights(row.shape)
        return w / w.sum()
    if row.taps == "w49":  # full rank, dyadic: exact sums on small integers (test_general_49_tap_tables_...)
        return np.random.default_rng(49).integers(-2, 3, 49).astype(np.float64) / 64.0
    return None


def _input(O, row, dims, seed=0):
    ps = O.padded_shape(row.shape, dims)
    if row.dtype == "bf16":
        rng = np.random.default_rng(41 + seed)
        if row.variant == MFMA:  # small integers: the regime the matrix-pipe contract is stated for
            return O.to_bf16(rng.integers(0, 100, ps).astype(np.float64))
        return O.to_bf16(rng.standard_normal(ps))
    if row.taps == "w49":
        return np.random.default_rng(dims[0] + seed).integers(-2, 3, ps).astype(np.float64)
    return O.reference_input(row.shape, dims)


def _expected(O, row, a, t, raw=False):
    """The oracle's grid after t sweeps of the row's driver; raw: of the plain sweep, whatever the plan's boundary option
    (include/lorastencil.h: "lora_plan_step* stay raw sweeps" -- no halo copy, no wrap)."""
    w = _weights(O, row)
    if row.dtype == "bf16":
        sep = "mfma" if row.variant == MFMA else (row.opts.get("separable", -1) != 0)
        return O.run_bf16(row.shape, a, t, weights=w, separable=sep)
    if row.bc and not raw:
        return O.run_bc(row.shape, a, t, row.bc, weights=w)
    return O.run(row.shape, a, t, weights=w)


def _check(row, got, exp, t, what, whole_1d=True):
    """The demand of the existing tests for this kind of configuration (see the module docstring)."""
    if row.ndim == 1 and whole_1d:  # the last element of a 1D array is not compared, as everywhere (1d/gpu_1r.cu:134)
        got, exp = got[:-1], exp[:-1]
    if row.dtype == "bf16" and row.variant == MFMA:
        # test_bf16_matrix_pipe_variant_matches_its_contract: within one bf16 ulp of the largest value, nearly all identical
        from oracle import oracle as O

        g, e = O.from_bf16(got), O.from_bf16(exp)
        assert np.isfinite(g).all(), what
        assert np.abs(g - e).max() <= 2.0 ** -7 * np.abs(e).max(), what
        assert (got != exp).mean() < 0.02, what
    elif row.dtype == "bf16":
        assert np.array_equal(got, exp), what
    elif row.taps == "w49" and t > 8:  # (past 2^52 in the numerators: to rounding, test_general_49_tap_tables_...)
        assert rel_err(got, exp) < 1e-12, what
    elif np.abs(exp).max() < 2.0 ** 50:
        assert np.array_equal(got, exp), what
    else:
        assert rel_err(got, exp) < 1e-13, what


def _make_plan(L, O, row, dims):
    plan = L.Plan(row.shape, dims, dtype=row.dtype)
    w = _weights(O, row)
    if w is not None:
        plan.set_weights(w)
    if row.bc:
        plan.set_boundary(row.bc)
    for k, v in row.opts.items():
        plan.set_option(k, v)
    if row.variant is not None:
        plan.set_variant(row.variant)
    # the row lands where the table says -- or the table has rotted
    sig = plan.kernel_signature
    assert plan.kernel_name == row.kernel, (row.id, dims, sig)
    for piece in row.sig:
        assert piece in sig, (row.id, dims, piece, sig)
    return plan


def _load(view, a):
    import torch

    if view.dtype == torch.bfloat16:
        view.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int16)))
    else:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _host(view):
    import torch

    if view.dtype == torch.bfloat16:
        return view.view(torch.int16).cpu().numpy().view(np.uint16)
    return view.cpu().numpy()


def _interior(L, shape, t):
    return L.ops.interior(shape, t)


def _fill_second(L, ar, shape, boundary, poisoned):
    """Buffer 1 before a run.  Reference boundary: its halo is part of the contract (odd sweeps read it: zeros); its interior
    is not -- poison.  Dirichlet / periodic: lora_plan_run rewrites its halo before anything reads it -- poison everywhere."""
    if not poisoned:
        ar.views[1].zero_()
    elif boundary in (None, "reference"):
        ar.views[1].zero_()
        _interior(L, shape, ar.bits(1)).fill_(ar.poison)
    else:
        ar.fill_poison(1)


def _run_carved(L, O, row, plan, dims, a, t, offset, poisoned=False):
    import torch

    ar = A.carve(O.padded_shape(row.shape, dims), row.dtype, 2, offset)
    _load(ar.views[0], a)
    _fill_second(L, ar, row.shape, row.bc, poisoned)
    torch.cuda.synchronize()
    plan.run(ar.views[0], ar.views[1], t)
    torch.cuda.synchronize()
    A.assert_guards_intact(ar, f"{row.id} {dims} t={t} offset={offset}")
    return ar


def _offsets(row):
    i = ROW_IDS.index(row.id)
    return A.OFFSETS[i % 5], A.OFFSETS[(i + 2) % 5]


# ---------------------------------------------------------------------------------------------------------------------------
# a. carved buffers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["ragged", "exact"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_carved_buffers_match_the_oracle_and_leave_the_guards_alone(L, O, row, size):
    dims = getattr(row, size)
    a = _input(O, row, dims)
    plan = _make_plan(L, O, row, dims)
    if row.bc == "periodic":  # the launches behind a periodic row: fused ones on the extended grid, or none of them
        import torch

        ar = A.carve(O.padded_shape(row.shape, dims), row.dtype, 2, 16)
        _load(ar.views[0], a)
        prof = plan.run_profiled(ar.views[0], ar.views[1], row.times[-1])
        torch.cuda.synchronize()
        fused = prof.fused_launches + prof.two_launches
        assert (fused > 0) if row.opts.get("torus", 1) else (fused == 0 and prof.single_launches == row.times[-1]), row.id
        A.assert_guards_intact(ar, row.id)
    for t in row.times:
        exp = _expected(O, row, a, t)
        for offset in _offsets(row):
            ar = _run_carved(L, O, row, plan, dims, a, t, offset)
            _check(row, _host(ar.views[t % 2]), exp, t, f"{row.id} {dims} t={t} offset={offset}")


# ---------------------------------------------------------------------------------------------------------------------------
# b. poisoned second buffer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["ragged", "exact"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_the_second_buffers_interior_is_never_read(L, O, row, size):
    """lora_plan_run's precondition on buffer 1 (include/lorastencil.h): only its halo under the reference boundary, nothing
    otherwise.  Poison wherever the contract allows it: the result must be the bits of the run on a zeroed buffer 1."""
    import torch

    dims = getattr(row, size)
    a = _input(O, row, dims)
    plan = _make_plan(L, O, row, dims)
    offset = A.OFFSETS[(ROW_IDS.index(row.id) + 4) % 5]
    cut = slice(None, -1) if row.ndim == 1 else Ellipsis
    for t in row.times:
        zeroed = _run_carved(L, O, row, plan, dims, a, t, offset, poisoned=False)
        poisoned = _run_carved(L, O, row, plan, dims, a, t, offset, poisoned=True)
        got, ref = poisoned.bits(t % 2)[cut], zeroed.bits(t % 2)[cut]
        assert not bool((got == poisoned.poison).any()), f"{row.id} {dims} t={t}: poison in the result"
        assert torch.equal(got, ref), f"{row.id} {dims} t={t}: {int((got != ref).sum())} cells differ"


# ---------------------------------------------------------------------------------------------------------------------------
# c. written set of the direct launches
# ---------------------------------------------------------------------------------------------------------------------------
def _direct_launches(row, plan):
    """[(label, applications, launch(src, dst, begin, end))] -- every direct entry the plan has (capi.cpp: has_apps)."""
    K = plan.get_option("steps_per_launch")
    out = [("step_region", 1, plan.step_region)]
    if row.step2:
        out.append(("step2_region", 2, plan.step2_region))
    if row.fused_direct and K > 1:
        out.append(("stepk_region", K, plan.stepk_region))
        if row.ndim == 1:
            tails = [n for n in (2, 4, 8, 16) if n < K]
        elif row.ndim == 2:
            tails = [n for n in (2, 4) if n < K]
        else:
            tails = [2] if K > 2 else []
        for n in tails:
            out.append((f"stepn_region({n})", n, lambda s, d, b, e, n=n: plan.stepn_region(n, s, d, b, e)))
    return out


def _ranges(n, g):
    """Ranges of the outermost interior index: whole grid, empty ones, ranges that start and end inside a tile / chunk, the
    first and the last row alone; begins are multiples of the region granularity g."""
    def dn(x):
        return max(0, min(n, x)) // g * g

    cand = [(0, n), (0, 0), (dn(n // 2), dn(n // 2)), (dn(n), dn(n)), (dn(n // 3 + 1), min(n, 2 * n // 3 + 2)), (0, min(n, 1)),
            (dn(n - 1), n), (dn(3), min(n, 11))]
    out = []
    for b, e in cand:
        if 0 <= b <= e <= n and (b, e) not in out:
            out.append((b, e))
    return out


@pytest.mark.parametrize("size", ["ragged", "exact"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_direct_launches_write_exactly_the_interior_of_their_range(L, O, row, size):
    """The destination starts as poison everywhere.  After a launch over [begin, end) the cells that are no longer poison are
    EXACTLY the interior cells of those rows / planes / points -- no halo cell, nothing outside the range (the slab and block
    drivers keep ghost rows there), no guard byte -- and each holds the oracle's value."""
    import torch

    dims = getattr(row, size)
    a = _input(O, row, dims)
    plan = _make_plan(L, O, row, dims)
    g = plan.region_granularity
    assert g == (2 if row.ndim == 1 else 1)
    h0 = L.ops.halo(row.shape)[0]
    ar = A.carve(O.padded_shape(row.shape, dims), row.dtype, 2, _offsets(row)[0])
    src, dst = ar.views
    _load(src, a)
    inner = torch.zeros(ar.padded_shape, dtype=torch.bool, device=dst.device)
    _interior(L, row.shape, inner).fill_(True)
    oracle = {}  # applications -> the oracle's grid after that many sweeps

    def verify(label, napps, ranges):
        what = f"{row.id} {dims} {label} {ranges}"
        A.assert_guards_intact(ar, what)
        want = torch.zeros_like(inner)
        for b, e in ranges:
            want[h0 + b:h0 + e] = inner[h0 + b:h0 + e]
        written = ~ar.is_poison(1)
        extra, missing = written & ~want, want & ~written
        assert not bool(extra.any()), f"{what}: {int(extra.sum())} cells written outside the range, first at " \
                                      f"{tuple(int(x) for x in extra.nonzero()[0])}"
        assert not bool(missing.any()), f"{what}: {int(missing.sum())} cells of the range not written, first at " \
                                        f"{tuple(int(x) for x in missing.nonzero()[0])}"
        if bool(want.any()):
            if napps not in oracle:
                oracle[napps] = _expected(O, row, a, napps, raw=napps == 1)  # (one application: the raw sweep)
            exp = oracle[napps]
            mask = want.cpu().numpy()
            got = _host(dst)
            # (the written cells only, as flat arrays: the last element of a 1D array is a halo cell, never among them)
            _check(row, got[mask], exp[mask], napps, what, whole_1d=False)

    for label, napps, launch in _direct_launches(row, plan):
        for b, e in _ranges(dims[0], g):
            ar.fill_poison(1)
            torch.cuda.synchronize()
            launch(src, dst, b, e)
            torch.cuda.synchronize()
            verify(label, napps, [(b, e)])
    # the whole-grid entries
    whole = [("step", 1, plan.step)]
    if row.step2:
        whole.append(("step2", 2, plan.step2))
    if row.fused_direct:
        whole.append(("stepk", plan.get_option("steps_per_launch"), plan.stepk))
    for label, napps, launch in whole:
        ar.fill_poison(1)
        torch.cuda.synchronize()
        launch(src, dst)
        torch.cuda.synchronize()
        verify(label, napps, [(0, dims[0])])
    # two ranges in one call (one launch in the register-resident 3D kernels, two launches elsewhere; an empty range is skipped)
    n = dims[0]
    K = plan.get_option("steps_per_launch") if row.fused_direct else 1
    lo, hi = max(g, (n // 4) // g * g), max(n // 2, (n - n // 4)) // g * g
    pairs = [((0, lo), (hi, n)), ((hi, n), (0, lo)), ((0, 0), (hi, n)), ((0, lo), (n // g * g, n // g * g))]
    depths = [K] + ([2] if row.ndim == 3 and K == 4 else [])
    for napps in depths:
        for (b0, e0), (b1, e1) in pairs:
            if not (0 <= b0 <= e0 <= n and 0 <= b1 <= e1 <= n and (e0 <= b1 or e1 <= b0)):
                continue
            ar.fill_poison(1)
            torch.cuda.synchronize()
            plan.stepn_region2(napps, src, dst, b0, e0, b1, e1)
            torch.cuda.synchronize()
            verify(f"stepn_region2({napps})", napps, [(b0, e0), (b1, e1)])
    assert np.array_equal(_host(src), a)  # the source is only read


# ---------------------------------------------------------------------------------------------------------------------------
# bookkeeping kernels: lora_plan_halo and lora_copy_block_f64 on carved memory
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,dtype", [("1d1r", (37,), "f64"), ("star2d1r", (9, 14), "f64"), ("box2d3r", (40, 131), "f64"),
                                              ("box3d1r", (5, 6, 16), "f64"), ("star3d1r", (7, 9, 33), "f64"),
                                              ("box3d1r", (5, 6, 16), "bf16"), ("box3d1r", (9, 31, 248), "bf16")])
@pytest.mark.parametrize("offset", [48, 496])
def test_halo_kernel_touches_halo_cells_only(L, O, shape, dims, dtype, offset):
    """lora_plan_halo COPY / ZERO / WRAP: every cell outside the interior gets its value, the interior keeps its bits (poison
    included: the kernel must not read it into anything), the guards stay."""
    import torch

    rng = np.random.default_rng(3)
    h = L.ops.halo(shape)
    ps = O.padded_shape(shape, dims)
    plan = L.Plan(shape, dims, dtype=dtype)
    inner = tuple(slice(k, -k) for k in h)
    a = rng.integers(1, 90, ps).astype(np.float64)
    b = rng.integers(1, 90, ps).astype(np.float64)
    enc = (lambda x: O.to_bf16(x)) if dtype == "bf16" else (lambda x: x)
    dec = (lambda x: O.from_bf16(x)) if dtype == "bf16" else (lambda x: x)
    ar = A.carve(ps, dtype, 2, offset)
    src, dst = ar.views
    _load(src, enc(a))
    # COPY from a source whose INTERIOR is poison (only its halo is the kernel's business) into a destination full of data
    _interior(L, shape, ar.bits(0)).fill_(ar.poison)
    _load(dst, enc(b))
    torch.cuda.synchronize()
    plan.halo(dst, "copy", src)
    torch.cuda.synchronize()
    exp = a.copy()
    exp[inner] = b[inner]
    assert np.array_equal(dec(_host(dst)), exp), (shape, "copy")
    # ZERO, the destination's interior poisoned: it must come out bit for bit as it went in
    _interior(L, shape, ar.bits(1)).fill_(ar.poison)
    plan.halo(dst, "zero")
    torch.cuda.synchronize()
    assert bool(_interior(L, shape, ar.is_poison(1)).all()), (shape, "zero: interior")
    outside = ~ar.is_poison(1)
    assert int(outside.sum()) == int(np.prod(ps)) - int(np.prod(dims)) and bool((ar.bits(1)[outside] == 0).all()), (shape, "zero")
    # WRAP from the destination's own interior
    _load(dst, enc(b))
    torch.cuda.synchronize()
    plan.halo(dst, "wrap")
    torch.cuda.synchronize()
    assert np.array_equal(dec(_host(dst)), np.pad(b[inner], [(k, k) for k in h], mode="wrap")), (shape, "wrap")
    A.assert_guards_intact(ar, f"halo {shape} {dims} {dtype}")


@pytest.mark.parametrize("rows,cols,dst_ld,src_ld,dst_col,src_col", [
    (7, 10, 24, 18, 4, 2),     # even everything, 16-byte aligned block starts: the 16-byte path
    (7, 10, 24, 18, 3, 2),     # destination starts on an odd column: 8-byte path
    (5, 9, 21, 40, 6, 7),      # odd extent and leading dimensions
    (64, 130, 138, 138, 4, 4),  # the interior of a padded 2D grid into another one
    (1, 1, 8, 8, 7, 0), (3, 258, 258, 300, 0, 42),
])
@pytest.mark.parametrize("offset", [16, 112])
def test_block_copy_kernel_writes_its_block_only(L, O, rows, cols, dst_ld, src_ld, dst_col, src_col, offset):
    """lora_copy_block_f64 with leading dimensions larger than `cols`: the block arrives, every other cell of the destination
    array keeps its poison, the guards stay."""
    import torch
    from lorastencil_amd import _lib

    rng = np.random.default_rng(rows * 1000 + cols)
    extra = 3  # rows of the arrays above and below the block
    dst_ar = A.carve((rows + 2 * extra, dst_ld), "f64", 1, offset)
    src_ar = A.carve((rows + 2 * extra, src_ld), "f64", 1, offset)
    data = rng.standard_normal((rows + 2 * extra, src_ld))
    _load(src_ar.views[0], data)
    d_ptr = dst_ar.views[0].data_ptr() + (extra * dst_ld + dst_col) * 8
    s_ptr = src_ar.views[0].data_ptr() + (extra * src_ld + src_col) * 8
    torch.cuda.synchronize()
    _lib.check(_lib.lib().lora_copy_block_f64(d_ptr, dst_ld, s_ptr, src_ld, rows, cols, None), "lora_copy_block_f64")
    torch.cuda.synchronize()
    want = torch.zeros((rows + 2 * extra, dst_ld), dtype=torch.bool, device="cuda")
    want[extra:extra + rows, dst_col:dst_col + cols] = True
    written = ~dst_ar.is_poison(0)
    assert torch.equal(written, want), f"{int((written ^ want).sum())} cells off the block"
    got = dst_ar.views[0].cpu().numpy()[extra:extra + rows, dst_col:dst_col + cols]
    assert np.array_equal(got, data[extra:extra + rows, src_col:src_col + cols])
    A.assert_guards_intact(dst_ar, "block copy destination")
    A.assert_guards_intact(src_ar, "block copy source")


# ---------------------------------------------------------------------------------------------------------------------------
# d. one plan, many runs
# ---------------------------------------------------------------------------------------------------------------------------
def _taps_menu(O, case):
    if case == "1d":
        w = O.effective_weights("1d1r")
        w2 = O.effective_weights("1d2r")
        return [w / w.sum(), w2 / w2.sum(), 0.5 * w / w.sum()]
    if case == "2d":  # each with a low-rank form, so that the matrix-pipe variant is valid under any of them
        out = []
        for s in ("star2d1r", "box2d3r", "star2d3r"):
            w = O.effective_weights(s)
            out.append(w / w.sum())
        return out
    if case == "3d":
        ws, wb = O.effective_weights("star3d1r"), O.effective_weights("box3d1r")
        rng = np.random.default_rng(27)
        g = rng.standard_normal(27)  # general taps: no separable form
        return [ws / ws.sum(), wb / wb.sum(), g / np.abs(g).sum()]
    wb = O.effective_weights("box3d1r")
    aniso = np.einsum("k,i,j->kij", [0.25, 0.5, 0.125], [1.0, 2.0, 1.0], [0.0625, 0.125, 0.03125]).ravel()
    ws = O.effective_weights("star3d1r")
    return [wb / wb.sum(), aniso, ws / ws.sum()]


LIFECYCLES = {
    # case: shape, dims, dtype, option menu, run lengths, (short run, long run, run without / with the scratch grid)
    "1d": ("1d1r", (5000,), "f64",
           {"steps_per_launch": (0, 1, 2, 4, 8, 16, 32), "scratch": (-1, 0, 1), "graph": (-1, 0, 1), "torus": (0, 1)},
           (0, 1, 2, 7, 16, 17, 24, 31, 40, 67, 100), (17, 40, 16, 24)),
    "2d": ("star2d1r", (53, 246), "f64",
           {"steps_per_launch": (0, 1, 2, 4, 6), "stream": (0, 1), "wg": (-1, 0, 1), "wg_rows": (0, 20), "lowrank_valu": (-1, 0, 4),
            "persistent": (0, 1), "fused_rows": (0, 6, 8, 10), "rows_per_thread": (4, 8, 16), "stream_depth": (2, 4, 6),
            "scratch": (-1, 0, 1), "graph": (-1, 0, 1), "torus": (0, 1)},
           (0, 1, 2, 5, 6, 8, 13, 14, 18, 19, 23), (7, 20, 12, 18)),
    "3d": ("box3d1r", (37, 29, 190), "f64",
           {"steps_per_launch": (0, 1, 2, 3, 4), "stream3": (-1, 0, 1), "lanes3": (-1, 0, 1), "stream3_waves": (0, 4, 8),
            "stream3_pipe": (0, 1), "spans3": (-1, 0, 1, 2), "fused_z_chunk": (0, 3, 9), "z_chunk": (1, 4, 7), "separable": (-1, 0),
            "scratch": (-1, 0, 1), "graph": (-1, 0, 1), "torus": (0, 1)},
           (0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13, 17), (5, 17, 4, 6)),
    "3d_bf16": ("box3d1r", (9, 31, 248), "bf16",
                {"steps_per_launch": (0, 1, 2, 4), "lanes3": (-1, 0, 1), "spans3": (-1, 0, 1, 2), "fused_z_chunk": (0, 3, 9),
                 "z_chunk": (1, 4, 7), "separable": (-1, 0), "lds_dma": (0, 1), "cols_per_lane": (4, 8), "fused_pipeline": (0, 1),
                 "scratch": (-1, 0, 1), "graph": (-1, 0, 1), "torus": (0, 1)},
                (0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13, 17), (5, 17, 4, 6)),
}


@pytest.mark.parametrize("case", list(LIFECYCLES))
def test_one_plan_through_many_runs_equals_fresh_plans(L, O, case):
    """A plan carries state across runs -- the cached hipGraph (keyed on buffers, times, epoch), the scratch grid, the two
    ghost-extended periodic grids (keyed on the epoch), the resolved options.  ONE plan goes through a scripted prefix that
    forces every cache transition and a seeded random tail; after every run its signature and its result must be those of a
    FRESH plan given the same requested settings: the same kernel, so the same bits."""
    import torch

    shape, dims, dtype, menu, lengths, (t_short, t_long, t_plain, t_scratch) = LIFECYCLES[case]
    nd = len(dims)
    bf16 = dtype == "bf16"
    ps = O.padded_shape(shape, dims)
    taps = _taps_menu(O, case)
    rng = np.random.default_rng({"1d": 101, "2d": 202, "3d": 303, "3d_bf16": 404}[case])
    plan = L.Plan(shape, dims, dtype=dtype).set_weights(taps[0])
    model = {"taps": 0, "bc": "reference", "opts": {}, "variant": L.VARIANT_DIRECT}
    pairs = [A.carve(ps, dtype, 2, 48), A.carve(ps, dtype, 2, 240)]
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
    padded_bytes = int(np.prod(ps)) * (2 if bf16 else 8)

    def fresh_plan():
        p = L.Plan(shape, dims, dtype=dtype).set_weights(taps[model["taps"]]).set_boundary(model["bc"])
        for k, v in model["opts"].items():
            p.set_option(k, v)
        if model["variant"] == L.VARIANT_MFMA:
            p.set_variant(L.VARIANT_MFMA)
        return p

    def mfma_valid():
        # (lora_plan_set_variant: 2D taps with a low-rank form -- all of the menu's; 3D: bf16 box taps with bf16-exact factors
        # -- the menu's first two --, reference boundary, fused launches)
        if case == "2d":
            return True
        return case == "3d_bf16" and model["taps"] in (0, 1) and model["bc"] == "reference" and \
            model["opts"].get("steps_per_launch", 0) != 1

    def new_input():
        if bf16:
            return O.to_bf16(rng.standard_normal(ps))
        return rng.integers(0, 100, ps).astype(np.float64)

    def fill(ar, a, poison_dst=False):
        _load(ar.views[0], a)
        if poison_dst:
            ar.fill_poison(1)
        else:
            _fill_second(L, ar, shape, model["bc"], poisoned=True)

    counts = {"runs": 0, "graph_runs": 0, "replay": 0, "graph_new_buffers": 0, "graph_new_times": 0, "graph_new_taps": 0,
              "to_periodic": 0, "from_periodic": 0, "scratch_after_none": 0, "stepk": 0, "zero_sweeps": 0, "side_streams": set()}
    state = {"epoch": 0, "graph_key": None, "taps_epoch": 0, "last_bc": None, "last_scratch": None}
    cut = slice(None, -1) if nd == 1 else Ellipsis

    def apply(op):
        kind = op[0]
        if kind == "opt":
            plan.set_option(op[1], op[2])
            model["opts"].pop(op[1], None)
            model["opts"][op[1]] = op[2]  # (re-inserted: the fresh plan replays the last settings in their order)
        elif kind == "taps":
            plan.set_weights(taps[op[1]])
            model["taps"] = op[1]
            state["taps_epoch"] = state["epoch"] + 1
        elif kind == "bc":
            plan.set_boundary(op[1])
            model["bc"] = op[1]
        elif kind == "variant":
            plan.set_variant(op[1])
        elif kind == "prepare":
            plan.prepare_run(op[1])
            return
        elif kind == "stepk":
            do_stepk(op[1], op[2])
            return
        elif kind == "run":
            do_run(op[1], op[2], op[3])
            return
        state["epoch"] += 1
        # the resolver may take a variant back (taps / boundary / depth it does not exist for): the plan says what it holds
        model["variant"] = plan.get_option("variant")

    def do_stepk(pi, si):
        ar = pairs[pi]
        a = new_input()
        fill(ar, a, poison_dst=True)
        torch.cuda.synchronize()
        plan.stepk(ar.views[0], ar.views[1], stream=streams[si])
        torch.cuda.synchronize()
        f = fresh_plan()
        assert f.kernel_signature == plan.kernel_signature, (case, counts, model)
        far = A.carve(ps, dtype, 2, 112)
        fill(far, a, poison_dst=True)
        torch.cuda.synchronize()
        f.stepk(far.views[0], far.views[1])
        torch.cuda.synchronize()
        assert torch.equal(ar.bits(1), far.bits(1)), (case, "stepk", counts, model)
        A.assert_guards_intact(ar, f"{case} stepk")
        A.assert_guards_intact(far, f"{case} stepk (fresh plan)")
        counts["stepk"] += 1

    def do_run(t, pi, si):
        ar = pairs[pi]
        a = new_input()
        fill(ar, a)
        torch.cuda.synchronize()
        plan.run(ar.views[0], ar.views[1], t, stream=streams[si])
        torch.cuda.synchronize()
        what = f"{case} run #{counts['runs']} t={t} pair={pi} stream={si} {model}"
        A.assert_guards_intact(ar, what)
        f = fresh_plan()
        assert f.kernel_signature == plan.kernel_signature, what
        far = A.carve(ps, dtype, 2, 112)
        fill(far, a)
        torch.cuda.synchronize()
        prof = f.run_profiled(far.views[0], far.views[1], t)  # (direct launches, no graph; blocks until done)
        torch.cuda.synchronize()
        A.assert_guards_intact(far, what + " (fresh plan)")
        got, ref = ar.bits(t % 2)[cut], far.bits(t % 2)[cut]
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} cells differ from the fresh plan's"
        assert bool(torch.isfinite(ar.views[t % 2].double()[cut]).all()), what
        # ---- what this run exercised (mirrors of lora_plan_run's own decisions, capi.cpp) ----
        counts["runs"] += 1
        counts["zero_sweeps"] += t == 0
        if si:
            counts["side_streams"].add(si)
        g = model["opts"].get("graph", -1)
        graph = si != 0 and t > 0 and (g == 1 or (g < 0 and t >= 16 and padded_bytes <= (64 << 20)))
        if graph:
            key = (pi, t, state["epoch"])
            last = state["graph_key"]
            counts["graph_runs"] += 1
            if last is not None:
                counts["replay"] += key == last
                counts["graph_new_buffers"] += key[0] != last[0]
                counts["graph_new_times"] += key[1] != last[1]
                counts["graph_new_taps"] += state["taps_epoch"] > last[2]
            state["graph_key"] = key
        if t > 0:
            if state["last_bc"] == "reference" and model["bc"] == "periodic":
                counts["to_periodic"] += 1
            if state["last_bc"] == "periodic" and model["bc"] == "reference":
                counts["from_periodic"] += 1
            state["last_bc"] = model["bc"]
            launches = prof.fused_launches + prof.two_launches
            natural = nd == 3 and plan.get_option("steps_per_launch") == 3
            scratch = model["bc"] != "periodic" and not natural and launches >= 3 and launches % 2 == 1 and \
                model["opts"].get("scratch", -1) != 0
            if scratch and state["last_scratch"] is False:
                counts["scratch_after_none"] += 1
            state["last_scratch"] = scratch

    script = [
        ("opt", "graph", 1),
        ("run", t_long, 0, 1),          # captured
        ("run", t_long, 0, 1),          # the cached graph replayed
        ("run", t_long, 1, 1),          # graph = 1, other buffers
        ("run", t_short, 1, 2),         # other times, other side stream
        ("taps", 1),
        ("run", t_short, 1, 2),         # other taps
        ("bc", "periodic"),
        ("run", t_long, 0, 1),          # a periodic run after reference runs ...
        ("run", t_long, 0, 1),          # ... replayed
        ("bc", "reference"),
        ("run", t_long, 0, 0),          # ... and back, on the null stream
        ("opt", "graph", -1),
        ("run", t_plain, 0, 0),         # a schedule with an even number of launches ...
        ("prepare", t_scratch),
        ("run", t_scratch, 1, 2),       # ... then one that goes through the scratch grid
        ("stepk", 0, 1),
        ("run", 0, 0, 2),
        ("bc", "dirichlet"),
        ("run", t_scratch, 0, 1),
        ("bc", "reference"),
        ("variant", L.VARIANT_DIRECT),
        ("run", t_long, 1, 0),
    ]
    for op in script:
        apply(op)
    keys = list(menu)
    n_ops = len(script)
    while n_ops < 64:
        r = rng.random()
        if r < 0.40:
            op = ("run", int(rng.choice(lengths)), int(rng.integers(2)), int(rng.integers(3)))
        elif r < 0.70:
            k = keys[int(rng.integers(len(keys)))]
            values = menu[k]
            if k == "steps_per_launch" and case == "2d" and model["variant"] == L.VARIANT_MFMA:
                values = (0, 1)  # (the matrix-pipe variant has no fused launches: deeper requests are refused)
            op = ("opt", k, int(values[int(rng.integers(len(values)))]))
        elif r < 0.78:
            op = ("taps", int(rng.integers(len(taps))))
        elif r < 0.86:
            op = ("bc", ("reference", "dirichlet", "periodic")[int(rng.integers(3))])
        elif r < 0.91:
            want = L.VARIANT_MFMA if (rng.random() < 0.6 and mfma_valid()) else L.VARIANT_DIRECT
            op = ("variant", want)
        elif r < 0.95:
            op = ("prepare", int(rng.choice(lengths)))
        else:
            if model["bc"] == "periodic":
                continue  # (the fused entries of a periodic plan have no stated halo semantics)
            op = ("stepk", int(rng.integers(2)), int(rng.integers(3)))
        apply(op)
        n_ops += 1
    assert n_ops >= 40 and counts["runs"] >= 15, counts
    for k in ("replay", "graph_new_buffers", "graph_new_times", "graph_new_taps", "to_periodic", "from_periodic",
              "scratch_after_none", "stepk", "zero_sweeps"):
        assert counts[k] >= 1, (k, counts)
    assert counts["side_streams"] == {1, 2}, counts


# ---------------------------------------------------------------------------------------------------------------------------
# e. two plans at once
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_plans_in_flight_equal_their_solo_runs(L, O):
    """include/lorastencil.h: "Different plans may be used from different threads at the same time".  Two plans of different
    shapes and taps, each on its own stream and its own carved pair: launches interleaved from one host thread, then issued
    from two threads -- each result the bits of the plan running alone."""
    import torch

    rng = np.random.default_rng(5)
    w2 = O.effective_weights("star2d1r")
    w3 = O.effective_weights("box3d1r")
    jobs = [  # (shape, dims, dtype, taps, sweeps per call: 2D one launch of four + one of two, 3D two launches of two)
        ("star2d1r", (150, 380), "f64", w2 / w2.sum(), 6),
        ("box3d1r", (21, 37, 136), "bf16", w3 / w3.sum(), 4),
    ]
    rounds = 4
    state = []
    for i, (shape, dims, dtype, w, per_call) in enumerate(jobs):
        ps = O.padded_shape(shape, dims)
        a = O.to_bf16(rng.standard_normal(ps)) if dtype == "bf16" else rng.standard_normal(ps)
        plan = L.Plan(shape, dims, dtype=dtype).set_weights(w)
        ar = A.carve(ps, dtype, 2, A.OFFSETS[1 + 2 * i])
        state.append({"plan": plan, "ar": ar, "a": a, "stream": torch.cuda.Stream(), "per_call": per_call, "shape": shape})

    def reset(s):
        _load(s["ar"].views[0], s["a"])
        _fill_second(L, s["ar"], s["shape"], "reference", poisoned=True)

    def call(s):  # an even number of sweeps: the data is back in buffer 0 and buffer 1's halo is zero again
        s["plan"].run(s["ar"].views[0], s["ar"].views[1], s["per_call"], stream=s["stream"])

    solo = []
    for s in state:
        reset(s)
        torch.cuda.synchronize()
        for _ in range(rounds):
            call(s)
        torch.cuda.synchronize()
        A.assert_guards_intact(s["ar"], "solo")
        solo.append(s["ar"].bits(0).clone())
        assert bool(torch.isfinite(s["ar"].views[0].double()).all())

    # one host thread, launches interleaved, no synchronisation in between
    for s in state:
        reset(s)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for s in state:
            call(s)
    torch.cuda.synchronize()
    for s, ref in zip(state, solo):
        A.assert_guards_intact(s["ar"], "interleaved")
        assert torch.equal(s["ar"].bits(0), ref), (s["shape"], "interleaved")

    # two host threads
    for s in state:
        reset(s)
    torch.cuda.synchronize()
    errors = []
    start = threading.Barrier(len(state))

    def worker(s):
        try:
            torch.cuda.set_device(0)
            start.wait(timeout=60)
            for _ in range(rounds):
                call(s)
            s["stream"].synchronize()
        except Exception as e:  # noqa: BLE001 -- reported below, in the test's own thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(s,)) for s in state]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads) and not errors, errors
    torch.cuda.synchronize()
    for s, ref in zip(state, solo):
        A.assert_guards_intact(s["ar"], "two threads")
        assert torch.equal(s["ar"].bits(0), ref), (s["shape"], "two threads")
