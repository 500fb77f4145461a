"""GPU tests that pin which neighbour every tap multiplies, in every single-launch entry, against the exact integer model of
tests/stencil_model.py.

Why.  The solver-side kernels are tested by a chain -- kernel == ``plan.step_region`` plus one numpy operation, bit for bit --
on tap tables that a transposition, a mirror or a point reflection maps to themselves and that hold many equal pairs
(tests/test_stencil_model_host.py pins which).  A kernel with its own offset table (kernels_cg_small.hip's ringed LDS array,
kernels_mg_fused.hip's window, the row policies of tile_walk.h, the plane ring in 3D) can mix up two neighbours and pass.  Here
the taps are ``stencil_model.fingerprint_taps``: pairwise distinct positive integers that no signed axis permutation maps to
themselves; the data are integers (u, u_prev in 0..99 with values in their halos, f in 0..9 with NaN in its halo).  Every
intermediate stays below 2**53 -- ``stencil_model.assert_exact`` checks that in integers BEFORE the engine is called -- so the
engine's fp64 results are exact whatever its summation order, and every comparison is ``==`` on values or on record fields.  The
one entry that rounds, lora_plan_cg_small, gets a derived allowance (see there).

Yardstick per entry: the model, which shares no code with the engine or the oracle and whose orientation the host test ties to
the CPU oracle.  No entry is compared with another entry of the engine, except where the header promises the same bits
(mg_defect_restrict against defect + mg_restrict).

Buffers: carved by tests/arena.py (through tests/test_gpu_pcg.py's Grids) at offsets 16 and 240, guard bands NaN; output grids
poisoned before each call; after it the guards are intact, the inputs unchanged bit for bit, and every cell outside the region's
interior still holds what it held.

Shapes, the smallest that reach each path (from the files that own the kernels):
  1D   (1027,) whole and [510, 1027): two tiles of 512 and the odd tail point
  2D   (1, 2) a single tiny grid; (33, 130) one row and one column pair spill into second tiles; (70, 258) with [5, 37): a region
       that begins and ends inside a tile; (7, 13) odd innermost extent: the one-thread-per-point kernels (sweeps only)
  3D   (1, 1, 2); (34, 18, 130) whole and with [3, 5): partial tiles on all three axes, the plane ring ends mid-phase; (3, 5, 7)
  cg_small            (5, 6), (4, 130), (5, 7, 6): non-square, so a transposition cannot hide
  mg_defect_restrict  (16, 20) -> (8, 10) and (9, 10, 12) -> (4, 5, 6)
Tap sets: 2D diamond / star / box through star2d1r / star2d3r / box2d3r; 3D star and the 27-tap box, the box with three tables:
"direct" (1 + t), "sep" (the outer product (1, 2, 3) x (1, 5, 7) x (1, 11, 13)) and "sep0" ("direct" with option separable = 0).
The fp64 single-launch entries have no separable evaluation (plan.cpp keeps the factors for the plane-streaming and
register-resident multi-sweep kernels only), so all three run the 27-tap order; test_cases_reach_every_tap_set says what the
plans resolve.  Those multi-sweep kernels are pinned the same way by tests/test_gpu_multisweep_taps.py.

MEASURED on the MI355X: every entry agrees with the model as it is (no kernel changed); cg_small's one iteration gives numpy's
bits (0 of the 2 units allowed); the file takes about 3 s.  With the two inner offsets of kernels_cg_small.hip's host-built table
swapped in a scratch build, all 20 cg_small tests here fail, while tests/test_gpu_coarse1.py notices on box3d1r only.
"""
import functools
import time

import numpy as np
import pytest

import stencil_model as SM
import test_gpu_coarse1 as C
import test_gpu_mg as M
import test_gpu_pcg as P

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
A, CC = 2, -1                      # the leapfrog coefficients of a single step: a (S(u) + f) + c u_prev
A1, C1, A2, C2 = 2, -1, 3, -2      # two steps per launch: another pair for the second step, so a swap shows
SIGMA, TAU = 9, 8                  # apply_dot_shift
THETA_TAU = 4                      # theta_start

SHAPES_2D = ("star2d1r", "star2d3r", "box2d3r")
TABLES_3D = (("star3d1r", "direct"), ("box3d1r", "direct"), ("box3d1r", "sep"), ("box3d1r", "sep0"))

# (shape, form, dims, regions as [lo, hi) of the outermost axis)
D1 = [(s, "direct", (1027,), ((0, 1027), (510, 1027))) for s in ("1d1r", "1d2r")]
D2 = [(s, "direct", d, r) for s in SHAPES_2D for d, r in (((1, 2), ((0, 1),)), ((33, 130), ((0, 33),)), ((70, 258), ((5, 37),)))]
D3 = [(s, f, d, r) for s, f in TABLES_3D for d, r in (((1, 1, 2), ((0, 1),)), ((34, 18, 130), ((0, 34), (3, 5))))]
ODD = [(s, "direct", (7, 13), ((0, 7),)) for s in SHAPES_2D] + [(s, f, (3, 5, 7), ((0, 3),)) for s, f in TABLES_3D]
WALK = D1 + D2 + D3        # the plans of the shared tile walk: residual, apply_dot, theta_start, defect
SWEEPS = WALK + ODD        # step_region, with a source, the single leapfrog steps
# theta_start squares r = 4 (S(u) + f - u).  With the "sep" table (tap sum 1950) r is about 3.9e5 per cell, and over the 79 560
# cells of the whole 34 x 18 x 130 grid the sum of squares is about 1.2e16 > 2**53: not exact, so that table keeps the [3, 5)
# region there (4 680 cells, 7e14) and the whole grid runs with the other three tables.
THETA = [(s, f, d, tuple(r for r in rs if not (f == "sep" and r == (0, 34)))) for s, f, d, rs in WALK]
CG_SMALL = [(s, "direct", d) for s in SHAPES_2D for d in ((5, 6), (4, 130))] + [(s, f, (5, 7, 6)) for s, f in TABLES_3D]
MG = [(s, "direct", (16, 20)) for s in SHAPES_2D] + [(s, f, (9, 10, 12)) for s, f in TABLES_3D]


def ids(cases):
    return [f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}" for c in cases]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_gpu_tap_orientation.py: {time.perf_counter() - t0:.1f} s wall time")


def taps(L, shape, form):
    """the integer fingerprint table of a case, on the support of the shape's own taps (the plan resolves the same tap set)"""
    support = L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0
    return SM.fingerprint_taps(support, "sep" if form == "sep" else "direct")


def make_plan(L, shape, form, dims, options=()):
    p = L.Plan(shape, dims)
    if form == "sep0":
        p.set_option("separable", 0)
    for key, value in options:
        p.set_option(key, value)
    return p.set_weights(taps(L, shape, form).astype(np.float64))


@functools.lru_cache(maxsize=None)
def model_data(shape, dims):
    return SM.data(shape, dims, SM.seed_of("tap orientation", SM.ndim_of(shape), dims))


def grids(L, shape, dims, off, values):
    """tests/test_gpu_pcg.py's carved grids with the bits every input held"""
    g = P.Grids(L, shape, dims, off, values)
    g.before = [g.bits(i) for i in range(len(values))]
    return g


def inputs_unchanged(g, which, what):
    import torch

    for i in which:
        assert torch.equal(g.arena.bits(i), g.before[i]), f"{what}: input grid {i} was written"


def check_cells(g, i, lo, hi, want, what, untouched=None):
    """grid i holds the model's integers on the interior cells of [lo, hi), value for value, and every other cell of it the
    poison (or, for an in-place entry, the bits `untouched` held)"""
    import torch

    m = g.region(lo, hi)
    got = g.v[i][m].cpu().numpy().reshape(want.shape)
    if not SM.exactly(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} cells differ from the integer model, the first at {tuple(bad[0])}: "
                             f"engine {got[tuple(bad[0])]!r}, model {int(want[tuple(bad[0])])}")
    if untouched is None:
        assert bool(g.arena.is_poison(i)[~m].all()), f"{what}: a cell outside the region's interior was written"
    else:
        assert torch.equal(g.arena.bits(i)[~m], untouched[~m]), f"{what}: a cell outside the region's interior was written"


def diff_tuple(L, rec):
    return L.GridDiff(float(rec[0]), float(rec[1]), float(rec[2]), rec[3], rec[4], rec[5])


def dot_tuple(L, rec):
    return L.GridDot(float(rec[0]), float(rec[1]), rec[2], rec[3])


# ---- which tap sets the cases reach ------------------------------------------------------------------------------------------------
def test_cases_reach_every_tap_set(L):
    seen = {1: set(), 2: set(), 3: set()}
    for shape, form, dims, _ in SWEEPS:
        seen[len(dims)].add(make_plan(L, shape, form, dims).get_option("tapset"))
    assert seen[2] == {0, 1, 2}  # diamond, star, box
    assert seen[3] == {0, 1}     # star, box
    # the three tables of the 27-tap box: all of them the box, in the 27-tap order
    direct, sep = taps(L, "box3d1r", "direct"), taps(L, "box3d1r", "sep")
    a, b, c = (np.array(v) for v in SM.SEP_FACTORS)
    assert np.array_equal(sep, np.einsum("i,j,k->ijk", a, b, c).ravel()) and not np.array_equal(sep, direct)
    for form in ("direct", "sep", "sep0"):
        p = make_plan(L, "box3d1r", form, (34, 18, 130))
        assert p.get_option("tapset") == 1 and p.get_option("cg") == 1 and p.get_option("fused_residual") == 1
        assert p.get_option("separable") == (0 if form == "sep0" else -1)
    # (the engine's exact rank-1 test reads the factors through the centre tap, b = (1, 5, 7) / 5, which does not round-trip:
    # it does not take the "sep" table for separable -- and no entry tested here would evaluate it that way if it did)
    print("lora_separable_3x3x3 of the 'sep' table:", L.separable_3x3x3(sep.astype(np.float64)))


# ---- 1, 2. step_region, plain and with a source ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", SWEEPS, ids=ids(SWEEPS))
def test_step_region_and_source(L, shape, form, dims, regions):
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    SM.assert_exact(f"{shape} {dims}", [SM.magnitude(shape, u, w, f)])
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [u, f, None])
        plain, src = make_plan(L, shape, form, dims), make_plan(L, shape, form, dims).set_source(g.v[1])
        assert src.get_option("source") == 1
        for lo, hi in regions:
            for plan, ff, name in ((plain, None, "step_region"), (src, f, "set_source + step_region")):
                what = f"{name} {shape} {form} {dims} [{lo}, {hi}) offset {off}"
                g.arena.fill_poison(2)
                plan.step_region(g.v[0], g.v[2], lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0, 1), what)
                check_cells(g, 2, lo, hi, SM.source(shape, u, w, ff, lo, hi), what)


# ---- 3. two applications with a source in one launch (2D, even innermost extent) ------------------------------------------------
def run_default_and_direct(L, shape, form, dims, extra, call):
    """call(plan, exact) with option lowrank_valu = 0 (direct tap order: exact) and with the plan's default evaluation: exact
    unless that resolves a structured form, whose products round (then rint(got) == model and |got - model| <= 0.25)"""
    for opts in ([("lowrank_valu", 0)], []):
        plan = make_plan(L, shape, form, dims, list(extra) + opts)
        call(plan, bool(opts) or plan.get_option("fused_eval") in (0, 1, 2) or len(dims) == 3, "lowrank_valu = 0" if opts else "default")


def check_two_level(g, i, lo, hi, want, exact, what):
    if exact:
        check_cells(g, i, lo, hi, want, what)
        return 0.0
    got = g.v[i][g.region(lo, hi)].cpu().numpy().reshape(want.shape)
    dev = float(np.abs(got - want.astype(np.float64)).max())
    assert np.array_equal(np.rint(got), want.astype(np.float64)) and dev <= 0.25, f"{what}: {dev} from the integer model"
    assert bool(g.arena.is_poison(i)[~g.region(lo, hi)].all()), f"{what}: a cell outside the region's interior was written"
    return dev


@pytest.mark.parametrize("shape,form,dims,regions", D2, ids=ids(D2))
def test_step2_region_with_a_source(L, shape, form, dims, regions):
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    SM.assert_exact(f"{shape} {dims}", [SM.source2_magnitude(shape, u, w, f)])
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [u, f, None])

        def call(plan, exact, name):
            plan.set_source(g.v[1])
            assert plan.get_option("steps_per_launch") == 2 and plan.kernel_name == "stencil2d_source2_kernel"
            for lo, hi in regions:
                what = f"step2_region {shape} {dims} [{lo}, {hi}) offset {off} {name}"
                g.arena.fill_poison(2)
                plan.step2_region(g.v[0], g.v[2], lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0, 1), what)
                dev = check_two_level(g, 2, lo, hi, SM.source2(shape, u, w, f, lo, hi), exact, what)
                print(what, "exact" if exact else "structured form", "largest deviation", dev)

        run_default_and_direct(L, shape, form, dims, (), call)


# ---- 4. single leapfrog steps, in place ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", SWEEPS, ids=ids(SWEEPS))
def test_leapfrog_steps(L, shape, form, dims, regions):
    cur, f, prev = model_data(shape, dims)
    w = taps(L, shape, form)
    SM.assert_exact(f"{shape} {dims}", [abs(A) * SM.magnitude(shape, cur, w, f) + abs(CC) * SM.interior(shape, SM.ints(prev))])
    plan = make_plan(L, shape, form, dims)
    assert plan.leapfrog_depth >= 1
    import torch

    prev_host = torch.from_numpy(np.array(prev))
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [cur, f, prev])
        for lo, hi in regions:
            for name in ("step_leapfrog_region", "step_leapfrog_src_region"):
                what = f"{name} {shape} {form} {dims} [{lo}, {hi}) offset {off}"
                g.v[2].copy_(prev_host)  # in place: the oldest level is overwritten
                if name == "step_leapfrog_region":
                    plan.step_leapfrog_region(g.v[0], g.v[2], float(CC), lo, hi)
                    want = SM.leapfrog(shape, cur, prev, w, None, 1, CC, lo, hi)
                else:
                    plan.step_leapfrog_src_region(g.v[0], g.v[2], g.v[1], float(A), float(CC), lo, hi)
                    want = SM.leapfrog(shape, cur, prev, w, f, A, CC, lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0, 1), what)
                check_cells(g, 2, lo, hi, want, what, untouched=g.before[2])


# ---- 5, 6. two leapfrog steps in one launch: 2D, and 3D behind option leap3 ---------------------------------------------------------
LEAP2 = D2 + D3


@pytest.mark.parametrize("shape,form,dims,regions", LEAP2, ids=ids(LEAP2))
def test_two_leapfrog_steps_in_one_launch(L, shape, form, dims, regions):
    cur, f, prev = model_data(shape, dims)
    w = taps(L, shape, form)
    SM.assert_exact(f"{shape} {dims}", [SM.leapfrog2_magnitude(shape, prev, cur, w, f, A1, C1, A2, C2)])
    extra = [("leap3", 1)] if len(dims) == 3 else []
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [prev, cur, f, None, None])

        def call(plan, exact, name):
            assert plan.leapfrog_depth == 2
            for lo, hi in regions:
                for entry in ("step2_leapfrog_region", "step2_leapfrog_src_region"):
                    what = f"{entry} {shape} {form} {dims} [{lo}, {hi}) offset {off} {name}"
                    g.arena.fill_poison(3)
                    g.arena.fill_poison(4)
                    if entry == "step2_leapfrog_region":
                        plan.step2_leapfrog_region(g.v[0], g.v[1], g.v[3], g.v[4], float(CC), lo, hi)
                        want1, want2 = SM.leapfrog2(shape, prev, cur, w, None, 1, CC, 1, CC, lo, hi)
                    else:
                        plan.step2_leapfrog_src_region(g.v[0], g.v[1], g.v[2], g.v[3], g.v[4], float(A1), float(C1), float(A2), float(C2), lo, hi)
                        want1, want2 = SM.leapfrog2(shape, prev, cur, w, f, A1, C1, A2, C2, lo, hi)
                    g.guards(what)
                    inputs_unchanged(g, (0, 1, 2), what)
                    dev = max(check_two_level(g, 3, lo, hi, want1, exact, what + " out1"), check_two_level(g, 4, lo, hi, want2, exact, what + " out2"))
                    print(what, "exact" if exact else "structured form", "largest deviation", dev)

        run_default_and_direct(L, shape, form, dims, extra, call)


# ---- 7. residual and residual_src: the whole record ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", WALK, ids=ids(WALK))
def test_residual_records(L, shape, form, dims, regions):
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    plan = make_plan(L, shape, form, dims)
    assert plan.get_option("fused_residual") == 1
    b = SM.interior(shape, SM.ints(u))
    want = {}
    for lo, hi in regions:
        for ff in (None, f):
            rec = SM.diff_record(shape, dims, SM.source(shape, u, w, ff, lo, hi), b[lo:hi], lo)
            SM.assert_exact(f"{shape} {dims} [{lo}, {hi})", [SM.magnitude(shape, u, w, ff), rec[1]])
            want[(lo, hi, ff is None)] = diff_tuple(L, rec)
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [u, f])
        for lo, hi in regions:
            what = f"{shape} {form} {dims} [{lo}, {hi}) offset {off}"
            got, got_f = plan.residual(g.v[0], lo, hi), plan.residual_src(g.v[0], g.v[1], lo, hi)
            g.guards(what)
            inputs_unchanged(g, (0, 1), what)
            print(what, got, got_f)
            assert got == want[(lo, hi, True)], f"residual {what}: the model's record is {want[(lo, hi, True)]}"
            assert got_f == want[(lo, hi, False)], f"residual_src {what}: the model's record is {want[(lo, hi, False)]}"


# ---- 8. apply_dot and apply_dot_shift --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", WALK, ids=ids(WALK))
def test_apply_dot_and_shift(L, shape, form, dims, regions):
    p_host, _, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    plan = make_plan(L, shape, form, dims)
    assert plan.get_option("cg") == 1
    pi = SM.interior(shape, SM.ints(p_host))
    model = {}
    for lo, hi in regions:
        for sigma, tau in ((1, 1), (SIGMA, TAU)):
            q = SM.shifted(shape, p_host, w, sigma, tau, lo, hi)
            rec = SM.dot_record(pi[lo:hi], q)
            SM.assert_exact(f"{shape} {dims} [{lo}, {hi})", [sigma * pi + tau * SM.magnitude(shape, p_host, w), rec[1]])
            model[(lo, hi, sigma)] = (q, dot_tuple(L, rec))
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [p_host, None])
        for lo, hi in regions:
            for sigma, tau in ((1, 1), (SIGMA, TAU)):
                name = "apply_dot" if sigma == 1 else "apply_dot_shift"
                what = f"{name} {shape} {form} {dims} [{lo}, {hi}) offset {off}"
                g.arena.fill_poison(1)
                if sigma == 1:
                    got = plan.apply_dot(g.v[0], g.v[1], lo, hi)
                else:
                    got = plan.apply_dot_shift(g.v[0], g.v[1], float(sigma), float(tau), lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0,), what)
                q, rec = model[(lo, hi, sigma)]
                check_cells(g, 1, lo, hi, q, what)
                assert got == rec, f"{what}: record {got}, the model's {rec}"


# ---- 9. theta_start ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", THETA, ids=ids(THETA))
def test_theta_start(L, shape, form, dims, regions):
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    plan = make_plan(L, shape, form, dims)
    assert plan.get_option("cg") == 1 and regions
    model = {}
    for lo, hi in regions:
        for ff in (None, f):
            r = SM.theta_r(shape, u, w, ff, THETA_TAU, lo, hi)
            rec = SM.dot_record(r, r)
            SM.assert_exact(f"{shape} {dims} [{lo}, {hi})", [THETA_TAU * (SM.magnitude(shape, u, w, ff) + SM.interior(shape, SM.ints(u))), rec[1]])
            model[(lo, hi, ff is None)] = (r, dot_tuple(L, rec))
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [u, f, None, None])
        for lo, hi in regions:
            for ff in (None, f):
                what = f"theta_start {shape} {form} {dims} [{lo}, {hi}) f {ff is not None} offset {off}"
                g.arena.fill_poison(2)
                g.arena.fill_poison(3)
                got = plan.theta_start(g.v[0], None if ff is None else g.v[1], float(THETA_TAU), g.v[2], g.v[3], lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0, 1), what)
                r, rec = model[(lo, hi, ff is None)]
                check_cells(g, 2, lo, hi, r, what + " r")
                check_cells(g, 3, lo, hi, r, what + " p")
                assert got == rec, f"{what}: record {got}, the model's {rec}"


# ---- 10. defect ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims,regions", WALK, ids=ids(WALK))
def test_defect(L, shape, form, dims, regions):
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    plan = make_plan(L, shape, form, dims)
    SM.assert_exact(f"{shape} {dims}", [SM.magnitude(shape, u, w, f) + SM.interior(shape, SM.ints(u))])
    for off in OFFSETS:
        g = grids(L, shape, dims, off, [u, f, None])
        for lo, hi in regions:
            for ff in (None, f):
                what = f"defect {shape} {form} {dims} [{lo}, {hi}) f {ff is not None} offset {off}"
                g.arena.fill_poison(2)
                plan.defect(g.v[0], None if ff is None else g.v[1], g.v[2], lo, hi)
                g.guards(what)
                inputs_unchanged(g, (0, 1), what)
                check_cells(g, 2, lo, hi, SM.defect(shape, u, w, ff, lo, hi), what)


# ---- 11. mg_defect_restrict ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims", MG, ids=ids(MG))
def test_mg_defect_restrict(L, shape, form, dims):
    """The model's exact defect through the dense per-axis matrices in long double, judged by the bound of
    tests/test_gpu_mg.py::test_restriction_against_the_dense_matrices -- (terms + 4) u times the restricted |defect| -- with that
    file's matrices, pattern and u; and bit for bit against defect + mg_restrict, as the header promises."""
    import torch

    cdims = L.mg_coarse_dims(shape, dims)
    u, f, _ = model_data(shape, dims)
    w = taps(L, shape, form)
    plan = make_plan(L, shape, form, dims)
    assert plan.get_option("mg") == 1
    Pm, pattern, rho = M.transfer_yardstick(dims, cdims)
    LD = np.longdouble
    terms = M.apply_axes([q.T for q in pattern], np.ones(dims))
    SM.assert_exact(f"{shape} {dims}", [SM.magnitude(shape, u, w, f) + SM.interior(shape, SM.ints(u))])
    for off, scale in zip(OFFSETS, (1.0, -0.37)):
        fine = grids(L, shape, dims, off, [u, f, None])
        coarse = P.Grids(L, shape, cdims, off, [None, None])
        cmask = coarse.interior_mask()
        for ff in (f, None):
            what = f"mg_defect_restrict {shape} {form} {dims} -> {cdims} f {ff is not None} scale {scale} offset {off}"
            d = SM.defect(shape, u, w, ff, 0, None)
            coarse.arena.fill_poison(0)
            plan.mg_defect_restrict(fine.v[0], None if ff is None else fine.v[1], coarse.v[0], scale)
            fine.guards(what)
            coarse.guards(what)
            inputs_unchanged(fine, (0, 1), what)
            assert bool(coarse.arena.is_poison(0)[~cmask].all()), what + ": a halo cell of the coarse grid was written"
            got = coarse.host(0)
            exact = LD(scale) * LD(rho) * M.apply_axes([p.T for p in Pm], d.astype(LD))
            mass = abs(scale) * rho * M.apply_axes([p.T.astype(np.float64) for p in Pm], np.abs(d).astype(np.float64))
            bound = (terms + 4) * M.U * mass
            err = np.abs(got.astype(LD) - exact).astype(np.float64)
            print(what, "max |coarse|", np.abs(got).max(), "max err / bound", np.max(err / np.maximum(bound, 1e-300)))
            assert np.isfinite(got).all() and np.abs(got).max() > 0.0
            assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} coarse cells are further from the restricted model defect than the bound"
            # the composition the header names: the defect is the model's, the restriction of it has the same bits
            fine.arena.fill_poison(2)
            coarse.arena.fill_poison(1)
            plan.defect(fine.v[0], None if ff is None else fine.v[1], fine.v[2])
            plan.mg_restrict(fine.v[2], coarse.v[1], scale)
            torch.cuda.synchronize()
            check_cells(fine, 2, 0, dims[0], d, what + ": defect")
            assert np.array_equal(got.view(np.uint64), coarse.host(1).view(np.uint64)), what + ": differs from defect + mg_restrict"


# ---- 12. cg_small ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form,dims", CG_SMALL, ids=ids(CG_SMALL))
def test_cg_small_one_iteration_on_integers(L, shape, form, dims):
    """One iteration from integer x0, r0 (stencil_model.cg_start) with the integer taps.  q = A r0 and both dots are exact in
    the model, so rr0 is compared with ==.  alpha = rr0 / pq is ONE correctly rounded division of two exact integers, so
    x = fl(x0 + fl(alpha p)) and r = fl(r0 - fl(alpha q)) are determined up to one rounding of the product and one of the sum;
    numpy computes them the same way, and the allowance is two units in the last place of the larger operand.  That allowance
    is DERIVED from the header's rounding rule, not measured; a wrong tap moves q by an integer and r by alpha times it, about
    1e-3, against an allowance of about 1e-14."""
    w = taps(L, shape, form)
    x0, r0 = SM.cg_start(shape, dims, w, SM.seed_of("cg_small", shape, form, dims))
    plan = make_plan(L, shape, form, dims)
    assert plan.get_option("cg_small") == 1
    x0f, r0f = x0.astype(np.float64), r0.astype(np.float64)
    worst = 0.0
    for (sigma, tau), off in zip(((1, 1), (SIGMA, TAU)), OFFSETS):
        what = f"cg_small {shape} {form} {dims} ({sigma}, {tau}) offset {off}"
        padded = SM.with_halo(shape, r0, 0)
        q = SM.shifted(shape, padded, w, sigma, tau, 0, None)
        rr, pq = SM.dot_record(r0, r0), SM.dot_record(r0, q)
        assert pq[0] > 0 and rr[0] > 0, f"{what}: the model's p.q = {pq[0]}: the kernel would halt before its first update"
        SM.assert_exact(what, [sigma * np.abs(r0) + tau * SM.magnitude(shape, padded, w), rr[1], pq[1]])
        alpha = np.float64(rr[0]) / np.float64(pq[0])
        ap, aq = alpha * r0f, alpha * q.astype(np.float64)
        want_x, want_r = x0f + ap, r0f - aq
        x, r, info = C.Solve(L, shape, dims, x0f, r0f, off).run(plan, 1, float(sigma), float(tau), what=what)
        ulps_x = np.abs(x - want_x) / np.spacing(np.maximum(np.abs(x0f), np.abs(ap)))
        ulps_r = np.abs(r - want_r) / np.spacing(np.maximum(np.abs(r0f), np.abs(aq)))
        worst = max(worst, float(ulps_x.max()), float(ulps_r.max()))
        print(what, "rr0", info[0], "model", rr[0], "alpha", alpha, "x, r: units in the last place from numpy", ulps_x.max(), ulps_r.max())
        assert info[0] == float(rr[0]) and info[2] == 1 and info[3] == 0, f"{what}: d_info {info}, the model's rr0 {rr[0]}"
        assert np.isfinite(x).all() and np.isfinite(r).all()
        assert ulps_x.max() <= 2.0, f"{what}: x is {ulps_x.max()} units in the last place from x0 + alpha p"
        assert ulps_r.max() <= 2.0, f"{what}: r is {ulps_r.max()} units in the last place from r0 - alpha q"
    print(shape, form, dims, "largest deviation seen:", worst, "units in the last place")


@pytest.mark.parametrize("shape,form,dims", CG_SMALL, ids=ids(CG_SMALL))
def test_cg_small_four_iterations_against_the_numpy_model(L, shape, form, dims):
    """tests/test_gpu_coarse1.py's model and allowance scheme (the model against itself with its sums in the opposite order,
    tenfold, floor of ten units in the last place) on the fingerprint taps divided by their sum: not point-symmetric, so A is
    not symmetric -- the recurrences are plain arithmetic either way, and p.A p = p.(A + A^T) p / 2 > 0 because the symmetric
    part of S has non-negative entries and row sums of at most 1."""
    wi = taps(L, shape, form)
    w = wi.astype(np.float64) / float(wi.sum())
    x0, r0 = C.data(shape, dims)
    plan = L.Plan(shape, dims)
    if form == "sep0":
        plan.set_option("separable", 0)
    plan.set_weights(w)
    assert plan.get_option("cg_small") == 1
    iters = 4
    for (sigma, tau), off in zip(C.PAIRS, OFFSETS):
        a, b = (C.model_cg(w, x0, r0, iters, sigma, tau, order) for order in (1, -1))
        dev_x = np.abs(a[0] - b[0]).max() / np.abs(a[0]).max()
        dev_r = np.abs(a[1] - b[1]).max() / np.abs(r0).max()
        dev_rr0 = abs(a[2] - b[2]) / a[2]
        allow = dict(x=max(10.0 * dev_x, C.FLOOR), r=max(10.0 * dev_r, C.FLOOR), rr0=max(10.0 * dev_rr0, C.FLOOR))
        mx, mr, mrr0, _, mdone, mhalt = a
        assert mdone == iters and mhalt == 0
        what = f"cg_small {shape} {form} {dims} ({sigma}, {tau}) iters {iters}"
        x, r, info = C.Solve(L, shape, dims, x0, r0, off).run(plan, iters, sigma, tau, what=what)
        err_x = np.abs(x - mx).max() / np.abs(mx).max()
        err_r = np.abs(r - mr).max() / np.abs(r0).max()
        err_rr0 = abs(info[0] - mrr0) / mrr0
        print(what, "model's two orders differ by", (dev_x, dev_r), "allow", allow, "engine against model: x", err_x, "r", err_r, "rr0", err_rr0)
        assert np.isfinite(x).all() and np.isfinite(r).all(), what + ": a NaN of a halo reached a result"
        assert err_x <= allow["x"], f"{what}: x is {err_x} from the model's, allowed {allow['x']}"
        assert err_r <= allow["r"], f"{what}: r is {err_r} of max |r0| from the model's, allowed {allow['r']}"
        assert err_rr0 <= allow["rr0"] and info[2] == iters and info[3] == 0, f"{what}: d_info {info}"
