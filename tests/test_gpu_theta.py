"""GPU tests of the implicit time stepper (kernels_theta.hip, the stepper's phases of kernels_cg.hip's fold, cg.cpp).

Yardsticks: ``plan.step_region`` into a spare grid and numpy's elementwise fp64 arithmetic (one rounding per operation, as the
kernels') for the bits of the two stencil launches; exact integer sums and ``math.fsum`` for the records; a Python loop over
the public entries for the driver; a numpy restatement of the whole algorithm (start, CG, stop rule), the closed-form decay of
an eigenmode and ``numpy.linalg.solve`` for what the stepper computes.

Grids, regions, taps, buffers: those of tests/test_gpu_cg.py (its CASES and SEVERAL, ``symmetric_taps``, tests/arena.py at
offsets 16 and 240 with NaN guard bands).
"""
import math
import zlib

import numpy as np
import pytest

from test_gpu_cg import (CASES, IDS, OFFSETS, SEVERAL, SEVERAL_IDS, Grids, check_record, dense_problem, fbits, host_data, make_plan,
                         padded_with_interior, same_bits, span, symmetric_taps)
from test_gpu_stream_order import Job, _bits, ctx  # noqa: F401  (ctx: the gate fixture, one instance for this module)

pytestmark = pytest.mark.gpu

SHIFTS = [(1.0, 1.0), (9.0, 8.0), (1.37, 0.61)]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def sweep_into_spare(g, plan, i_in, lo, hi):
    """the older code: step_region of grid i_in into a zeroed spare grid (a plan with a source stores fl(acc + f))"""
    import torch

    spare = torch.zeros_like(g.v[i_in])
    if hi > lo:
        plan.step_region(g.v[i_in], spare, lo, hi)
    torch.cuda.synchronize()
    return spare


def region_cells(g, t, lo, hi):
    """the interior cells of the outermost range [lo, hi) of a device grid as a flat host vector"""
    return g.L.interior(g.shape, t).cpu().numpy()[lo:hi].ravel()


# ---- 1. apply_dot_shift ----------------------------------------------------------------------------------------------------
def check_shift(g, p, sigma, tau, begin, end, what):
    """one apply_dot_shift from grid 0 into grid 1 (whole grid NaN before): q bit for bit numpy's fl(fl(sigma p) - fl(tau
    spare)) on the region's interior, every other cell of q still the NaN it was, p unchanged, the guards intact"""
    import torch

    lo, hi = span(p, begin, end)
    g.arena.fill_poison(1)
    before = g.bits(0)
    got = p.apply_dot_shift(g.v[0], g.v[1], sigma, tau, begin, end)
    g.guards(what)
    assert torch.equal(g.arena.bits(0), before), what + ": p changed"
    spare = sweep_into_spare(g, p, 0, lo, hi)
    with np.errstate(invalid="ignore"):
        want = np.float64(sigma) * region_cells(g, g.v[0], lo, hi) - np.float64(tau) * region_cells(g, spare, lo, hi)
    have = region_cells(g, g.v[1], lo, hi)
    assert np.array_equal(have.view(np.int64), want.view(np.int64)), what + ": q differs from numpy on step_region's sweep"
    m = g.region(lo, hi)
    assert bool(g.arena.is_poison(1)[~m].all()), what + ": a cell of q outside the region's interior was written"
    return got


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_apply_dot_shift_bits_and_records(L, shape, dims, regions):
    """integer data with the integer pairs: p <= 99, |q| <= 9 x 99 + 8 x 49 x 3 x 99, every product below 1.2e7 and their sum over
    at most 79560 cells below 2**53 -- exact in any order; real data and (1.37, 0.61): the bound of test_gpu_cg.check_record"""
    ints, real = host_data(shape, dims)[:2]
    for kind, data in (("int", ints), ("normalised", real)):
        p = make_plan(L, shape, dims, kind)
        for off in OFFSETS:
            g = Grids(L, shape, dims, off, [data, None])
            for begin, end in regions:
                lo, hi = span(p, begin, end)
                for sigma, tau in SHIFTS:
                    what = f"{shape} {dims} {kind} ({sigma}, {tau}) [{begin}, {end}) offset {off}"
                    got = check_shift(g, p, sigma, tau, begin, end, what)
                    if hi == lo:
                        assert got == L.GridDot(0.0, 0.0, 0, 0), what
                        continue
                    a, b = g.host(0, lo, hi), g.host(1, lo, hi)
                    if kind == "int" and sigma != 1.37:
                        ia, ib = a.astype(np.int64), b.astype(np.int64)
                        assert np.array_equal(ib, b) and got == L.GridDot(float((ia * ib).sum()), float(np.abs(ia * ib).sum()), a.size, 0), what
                    else:
                        check_record(got, a, b, what)
                    if (sigma, tau) == (1.0, 1.0):  # the operator I - S: lora_plan_apply_dot, in q and in all four fields
                        q = g.bits(1)
                        g.arena.fill_poison(1)
                        plain = p.apply_dot(g.v[0], g.v[1], begin, end)
                        assert tuple(map(fbits, plain)) == tuple(map(fbits, got)), (what, plain, got)
                        assert np.array_equal(q.cpu().numpy(), g.bits(1).cpu().numpy()), what + ": q differs from apply_dot's"


# ---- 2. theta_start --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_theta_start_bits_and_records(L, shape, dims, regions):
    """grids: 0 = u (its halo holds values: the stencil reads it), 1 = f with a NaN halo, 2 = r, 3 = p, both NaN everywhere
    before each call.  The yardstick sweeps with a clean copy of f as a plan's source.  Integer data, tau = 8: |r| <= 8 x (49 x
    3 x 99 + 99), r squared below 1.4e10 and the sum over 79560 cells below 2**53; real data: check_record's bound."""
    import torch

    ints, real, real2 = host_data(shape, dims)[:3]
    ints2 = ints[::-1].copy() if len(dims) == 1 else ints.T.copy().reshape(ints.shape)
    for kind, u0, f0, tau in (("int", ints, ints2, 8.0), ("normalised", real, real2, 8.0), ("normalised", real, real2, 0.61)):
        w = symmetric_taps(L, shape, kind)
        p = make_plan(L, shape, dims, kind)
        for off in OFFSETS:
            g = Grids(L, shape, dims, off, [u0, None, None, None])
            every = g.region(0, p.dims[0]).clone()
            f_clean = torch.from_numpy(np.array(f0)).cuda()
            g.v[1][every] = f_clean[every]  # the halo of f stays NaN
            with_f = L.Plan(shape, dims).set_weights(w).set_source(f_clean)
            before = (g.bits(0), g.bits(1))
            for begin, end in regions:
                lo, hi = span(p, begin, end)
                m = g.region(lo, hi).clone()
                for use_f in (True, False):
                    what = f"{shape} {dims} {kind} tau {tau} f {use_f} [{begin}, {end}) offset {off}"
                    g.arena.fill_poison(2)
                    g.arena.fill_poison(3)
                    got = p.theta_start(g.v[0], g.v[1] if use_f else None, tau, g.v[2], g.v[3], begin, end)
                    g.guards(what)
                    assert torch.equal(g.arena.bits(0), before[0]) and torch.equal(g.arena.bits(1), before[1]), what + ": u or f changed"
                    spare = sweep_into_spare(g, with_f if use_f else p, 0, lo, hi)
                    want = np.float64(tau) * (region_cells(g, spare, lo, hi) - region_cells(g, g.v[0], lo, hi))
                    for i in (2, 3):
                        have = region_cells(g, g.v[i], lo, hi)
                        assert np.array_equal(have.view(np.int64), want.view(np.int64)), f"{what}: grid {i} differs from numpy on the sweep"
                        assert bool(g.arena.is_poison(i)[~m].all()), f"{what}: a cell of grid {i} outside the region's interior was written"
                    if hi == lo:
                        assert got == L.GridDot(0.0, 0.0, 0, 0), what
                    elif kind == "int":
                        iw = want.astype(np.int64)
                        assert np.array_equal(iw, want) and got == L.GridDot(float((iw * iw).sum()), float((iw * iw).sum()), iw.size, 0), what
                    else:
                        check_record(got, want, want, what)


# ---- the driver --------------------------------------------------------------------------------------------------------------
def theta_by_public_entries(plan, u, f, theta, tau, steps, max_iters, rtol):
    """the loop of the header's bit contract on the device grid u (in place); alpha, beta, thresh and the stop test in host
    fp64.  Returns (iterations of every finished step, breakdown, iterations applied in the step that broke down)."""
    import torch

    r, p, q = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    tt = theta * tau
    sigma, rtol2 = 1.0 + tt, rtol * rtol
    counts = []
    for _ in range(steps):
        start = plan.theta_start(u, f, tau, r, p)
        rr = start.dot
        if start.nonfinite > 0 or not math.isfinite(rr):
            return counts, True, 0
        thresh, k = rtol2 * rr, 0
        while rr != 0.0:
            d = plan.apply_dot_shift(p, q, sigma, tt)
            if d.nonfinite > 0 or not math.isfinite(d.dot) or not d.dot > 0.0 or not math.isfinite(rr):
                return counts, True, k
            e = plan.cg_update(u, r, p, q, rr / d.dot)
            k += 1
            if e.nonfinite > 0 or not math.isfinite(e.dot):
                return counts, True, k
            beta, rr = e.dot / rr, e.dot
            if rr <= thresh or k == max_iters:
                break
            plan.cg_direction(p, r, beta)
        counts.append(k)
    return counts, False, 0


def run_and_compare(L, plan, g, u0, f, theta, tau, steps, max_iters, rtol, what):
    """the driver on grid 0 (f: a device grid or None) against the loop over the public entries from the same level: d_u bit
    for bit, the iterations, the counts of the result; f and the halo of u untouched, the guards intact.  Returns (result,
    counts of the host loop, its breakdown flag)."""
    import torch

    g.v[0].copy_(torch.from_numpy(np.array(u0)))
    halo = ~g.region(0, plan.dims[0]).clone()
    before_u, before_f = g.bits(0), g.bits(1)
    res = plan.run_theta(g.v[0], f, tau, steps, theta=theta, max_iters=max_iters, rtol=rtol)
    g.guards(what)
    assert torch.equal(g.arena.bits(1), before_f), what + ": d_f was written"
    assert torch.equal(g.arena.bits(0)[halo], before_u[halo]), what + ": a halo cell of d_u was written"
    got = g.v[0].clone()
    g.v[0].copy_(torch.from_numpy(np.array(u0)))
    counts, broke, partial = theta_by_public_entries(plan, g.v[0], f, theta, tau, steps, max_iters, rtol)
    print(what, "driver:", res, "host loop:", counts, broke, partial)
    assert same_bits(got, g.v[0]), what + ": d_u differs from the loop over the public entries"
    assert res.breakdown == broke and res.steps_done == len(counts), what
    assert list(res.iterations) == counts + ([partial] + [0] * (steps - len(counts) - 1) if broke else []), what
    assert res.iterations_total == sum(counts) and res.iterations_max == max(counts, default=0), what
    assert res.unconverged_steps <= sum(k == max_iters for k in counts), what
    steady = plan.residual_src(g.v[0], f) if f is not None else plan.residual(g.v[0])
    assert tuple(map(fbits, res.steady)) == tuple(map(fbits, steady)), what + ": steady is not residual_src of the last level"
    return res, counts, broke


@pytest.mark.parametrize("shape,dims,regions", SEVERAL, ids=SEVERAL_IDS)
def test_driver_equals_the_composition_of_the_public_entries(L, shape, dims, regions):
    """Normalised taps, random u and f with random halos of u, 3 steps at tau = 8, at most 12 iterations to rtol = 1e-2.  The
    stop rule must fire, and not always at the same place: over a case's two runs the host loop's counts take more than one
    value and at least one is below 12 -- asserted of the host loop, so a rule that never fires cannot pass."""
    _, u0, f0 = host_data(shape, dims)[:3]
    plan = make_plan(L, shape, dims, "normalised")
    seen = []
    for off, theta in zip(OFFSETS, (1.0, 0.5)):
        g = Grids(L, shape, dims, off, [u0, f0])
        res, counts, broke = run_and_compare(L, plan, g, u0, g.v[1], theta, 8.0, 3, 12, 1e-2, f"{shape} {dims} theta {theta}")
        assert not broke and res.steps_done == 3
        assert res.unconverged_steps == 0 or max(counts) == 12
        seen += counts
    assert len(set(seen)) > 1 and min(seen) < 12, seen


def test_max_iters_exhausted_is_counted_not_an_error(L):
    shape, dims = "star2d1r", (70, 260)
    _, u0, f0 = host_data(shape, dims)[:3]
    plan = make_plan(L, shape, dims, "normalised")
    g = Grids(L, shape, dims, 16, [u0, f0])
    res, counts, broke = run_and_compare(L, plan, g, u0, g.v[1], 1.0, 8.0, 2, 3, 0.0, "rtol = 0, max_iters = 3")
    assert list(res.iterations) == [3, 3] == counts and res.unconverged_steps == 2 and res.steps_done == 2 and not broke
    assert res.iterations_total == 6 and res.iterations_max == 3


def test_breakdown_is_a_numeric_outcome(L):
    """Integer taps of sum 9 -- the centre 1, the four neighbours 2 -- at theta = 1, tau = 8: A = 9 I - 8 S has the eigenvalues
    9 - 8 (1 + 4 c), c in (-1, 1), so it is indefinite and p.Ap < 0 on smooth directions.  The level is a smooth positive field:
    the first direction already has p.q < 0.  No fault is provoked: this is the arithmetic path of tests/test_gpu_cg.py's
    test of the same name.  The same plan then runs a clean problem: the flag does not outlive its run."""
    import torch

    shape, dims = "star2d1r", (6, 10)
    w = np.zeros(49)
    w[24] = 1.0
    w[[17, 23, 25, 31]] = 2.0
    plan = L.Plan(shape, dims).set_weights(w)
    rng = np.random.default_rng(5)
    u0 = padded_with_interior(L, shape, dims, rng.integers(5, 9, dims).astype(np.float64), halo=1.0)
    f0 = padded_with_interior(L, shape, dims, rng.integers(-2, 3, dims).astype(np.float64))
    g = Grids(L, shape, dims, 16, [u0, f0])
    res, counts, broke = run_and_compare(L, plan, g, u0, g.v[1], 1.0, 8.0, 3, 6, 1e-6, "indefinite A")
    assert broke and res.breakdown and res.steps_done == len(counts) < 3
    # a NaN in an interior cell of f: the start's dot is not finite -- breakdown before anything is stored into d_u
    f1 = f0.copy()
    L.interior(shape, f1)[2, 3] = float("nan")
    g = Grids(L, shape, dims, 240, [u0, f1])
    before = g.bits(0)
    res = plan.run_theta(g.v[0], g.v[1], 8.0, 2, max_iters=4)
    g.guards("NaN in f")
    assert res.breakdown and res.steps_done == 0 and torch.equal(g.arena.bits(0), before) and res.steady.nonfinite > 0
    # the same plan afterwards, on Jacobi taps
    w = np.zeros(49)
    w[[17, 23, 25, 31]] = 0.25
    plan.set_weights(w)
    g = Grids(L, shape, dims, 16, [u0, f0])
    res, counts, broke = run_and_compare(L, plan, g, u0, g.v[1], 1.0, 8.0, 2, 40, 1e-8, "after the breakdown")
    assert not broke and res.steps_done == 2 and res.unconverged_steps == 0


def test_theta_zero_is_the_explicit_step(L):
    """theta = 0: A = I, q = p bit for bit, pq = rr0 in the same order of summation, alpha = 1: one iteration per step, and the
    level is fl(u + fl(tau fl(fl(S(u) + f) - u))).  The yardstick: the source sweep of a plan that carries f, numpy for the
    rest, level by level from the yardstick's own levels; 4 ulp of each value are allowed."""
    import torch

    for shape, dims in (("star2d1r", (70, 260)), ("box3d1r", (35, 17, 130)), ("1d2r", (1027,))):
        _, u0, f0 = host_data(shape, dims)[:3]
        w = symmetric_taps(L, shape, "normalised")
        plan = make_plan(L, shape, dims, "normalised")
        g = Grids(L, shape, dims, 16, [u0, f0])
        res = plan.run_theta(g.v[0], g.v[1], 0.5, 3, theta=0.0, max_iters=5, rtol=1e-8)
        g.guards(f"theta = 0 {shape}")
        assert list(res.iterations) == [1, 1, 1] and res.steps_done == 3 and not res.breakdown and res.unconverged_steps == 0
        with_f = L.Plan(shape, dims).set_weights(w).set_source(g.v[1])
        level, spare = torch.from_numpy(np.array(u0)).cuda(), torch.zeros_like(g.v[0])
        inner = lambda t: L.interior(shape, t)
        for _ in range(3):
            with_f.step(level, spare)
            torch.cuda.synchronize()
            a, b = inner(spare).cpu().numpy(), inner(level).cpu().numpy()
            inner(level).copy_(torch.from_numpy(b + np.float64(0.5) * (a - b)).cuda())
        want, got = inner(level).cpu().numpy(), inner(g.v[0]).cpu().numpy()
        ulps = np.abs(got - want) / np.spacing(np.abs(want))
        print("theta = 0", shape, "largest difference in ulp:", ulps.max())
        assert ulps.max() <= 4.0


# ---- what it computes: a numpy restatement of the algorithm ------------------------------------------------------------------
JACOBI = [17, 23, 25, 31]


def jacobi_sweep(a):
    """S of the star2d1r Jacobi taps on a padded array: the interior's new values"""
    c = a[4:-4, 4:-4]
    return 0.25 * a[3:-5, 4:-4] + 0.25 * a[4:-4, 3:-5] + 0.25 * a[4:-4, 5:-3] + 0.25 * a[5:-3, 4:-4] + 0.0 * c


def numpy_theta(u0, f, theta, tau, steps, max_iters, rtol):
    """start, CG and stop rule as the header states them, in numpy on padded arrays (its dots are numpy's pairwise sums).
    Returns (the last level as a padded array, the iterations of every step)."""
    u = u0.copy()
    tt = theta * tau
    sigma, rtol2 = 1.0 + tt, rtol * rtol
    counts = []
    p = np.zeros_like(u)
    inner = lambda a: a[4:-4, 4:-4]
    for _ in range(steps):
        t = jacobi_sweep(u) + inner(f) if f is not None else jacobi_sweep(u)
        r = tau * (t - inner(u))
        inner(p)[...] = r
        rr = float((r * r).sum())
        thresh, k = rtol2 * rr, 0
        while rr != 0.0:
            q = sigma * inner(p) - tt * jacobi_sweep(p)
            alpha = rr / float((inner(p) * q).sum())
            inner(u)[...] += alpha * inner(p)
            r -= alpha * q
            new = float((r * r).sum())
            k += 1
            beta, rr = new / rr, new
            if rr <= thresh or k == max_iters:
                break
            inner(p)[...] = r + beta * inner(p)
        counts.append(k)
    return u, counts


def jacobi_plan(L, dims):
    w = np.zeros(49)
    w[JACOBI] = 0.25
    return L.Plan("star2d1r", dims).set_weights(w), w


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("dims", [(6, 10), (33, 34)])
def test_an_eigenmode_decays_by_the_schemes_factor(L, dims, theta):
    """u = sin(pi i / (m + 1)) sin(2 pi j / (n + 1)) with a zero halo is an eigenvector of the Jacobi sweep, lambda = (cos(pi /
    (m + 1)) + cos(2 pi / (n + 1))) / 2, so every theta step multiplies it by g = (1 - (1 - theta) tau (1 - lambda)) / (1 + theta
    tau (1 - lambda)).  The bound is the numpy restatement's own distance from g^5 u0, relative to g^5; the engine may be 10
    times as far: its dots are summed in another order.  (A numpy model of this setup: 1e-13 .. 8e-13, at most 3 iterations.)"""
    m, n = dims
    tau, steps = 8.0, 5
    i, j = np.meshgrid(np.arange(1, m + 1), np.arange(1, n + 1), indexing="ij")
    u0 = padded_with_interior(L, "star2d1r", dims, np.sin(math.pi * i / (m + 1)) * np.sin(2 * math.pi * j / (n + 1)))
    lam = (math.cos(math.pi / (m + 1)) + math.cos(2 * math.pi / (n + 1))) / 2
    gf = (1 - (1 - theta) * tau * (1 - lam)) / (1 + theta * tau * (1 - lam))
    exact = gf ** steps * u0
    model, model_counts = numpy_theta(u0, None, theta, tau, steps, 60, 1e-12)
    model_err = np.abs(model - exact).max() / abs(gf ** steps)
    plan, _ = jacobi_plan(L, dims)
    g = Grids(L, "star2d1r", dims, 240, [u0, None])
    res = plan.run_theta(g.v[0], None, tau, steps, theta=theta, max_iters=60, rtol=1e-12)
    g.guards(f"eigenmode {dims} theta {theta}")
    err = np.abs(g.v[0].cpu().numpy() - exact).max() / abs(gf ** steps)
    print("eigenmode", dims, "theta", theta, "g", gf, "numpy restatement:", model_err, model_counts, "engine:", err, res.iterations)
    assert res.unconverged_steps == 0 and res.steps_done == steps and not res.breakdown
    assert err <= 10 * model_err


def test_rough_data_converges_and_leaves_the_rest_of_its_launches_unused(L):
    """(33, 34), random u with a random halo, random f, backward Euler at tau = 8, rtol = 1e-10 with room for 200 iterations a
    step.  The numpy restatement's counts come first and must be at most 100 (a CPU model with a slightly different rule: 52
    .. 56), so at least half of every step's launches are the early exit; the engine's counts within 2 of them, and the three
    levels those of a dense solve of (9 I - 8 S) u+ = u + 8 (f + the boundary's share) to 100 rtol max |u|."""
    dims, tau, rtol = (33, 34), 8.0, 1e-10
    rng = np.random.default_rng(zlib.crc32(b"theta rough"))
    plan, w = jacobi_plan(L, dims)
    u0 = rng.standard_normal(L.padded_shape("star2d1r", dims)) * 3.0
    f0 = padded_with_interior(L, "star2d1r", dims, rng.standard_normal(dims))
    model, k = numpy_theta(u0, f0, 1.0, tau, 3, 200, rtol)
    print("numpy restatement:", k)
    assert max(k) <= 100
    g = Grids(L, "star2d1r", dims, 16, [u0, f0])
    res = plan.run_theta(g.v[0], g.v[1], tau, 3, theta=1.0, max_iters=200, rtol=rtol)
    g.guards("rough data")
    print("engine:", res)
    assert res.unconverged_steps == 0 and res.steps_done == 3 and not res.breakdown
    assert all(abs(a - b) <= 2 for a, b in zip(res.iterations, k)), (res.iterations, k)
    A, b = dense_problem(L, "star2d1r", dims, w, f0, u0)  # A = I - S, b = f + S(the halo of u)
    M = (1 + tau) * np.eye(len(b)) - tau * (np.eye(len(b)) - A)
    level = L.interior("star2d1r", u0).ravel().copy()
    for _ in range(3):
        level = np.linalg.solve(M, level + tau * b)
    err = np.abs(L.interior("star2d1r", g.v[0]).cpu().numpy().ravel() - level).max()
    print("against the dense solve:", err, "bound", 100 * rtol * np.abs(level).max())
    assert err <= 100 * rtol * np.abs(level).max()
    assert np.abs(L.interior("star2d1r", model).ravel() - level).max() <= 100 * rtol * np.abs(level).max()


# ---- tuning options, streams, the host form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", SEVERAL, ids=SEVERAL_IDS)
def test_no_tuning_option_moves_a_bit(L, shape, dims, regions):
    import torch
    from test_gpu_residual import TUNING

    _, u0, f0 = host_data(shape, dims)[:3]
    g = Grids(L, shape, dims, 16, [u0, f0])
    ref = make_plan(L, shape, dims, "normalised").run_theta(g.v[0], g.v[1], 8.0, 2, theta=0.5, max_iters=6, rtol=1e-2)
    want = g.bits(0)
    tried = 0
    for key, value in TUNING[len(dims)]:
        t = make_plan(L, shape, dims, "normalised")
        if L._lib.lib().lora_plan_set_option(t._h, key.encode(), value) != 0:
            continue  # (not an option of this plan)
        g.v[0].copy_(torch.from_numpy(np.array(u0)))
        res = t.run_theta(g.v[0], g.v[1], 8.0, 2, theta=0.5, max_iters=6, rtol=1e-2)
        g.guards(f"{shape} {key}={value}")
        assert repr(res) == repr(ref) and torch.equal(g.bits(0), want), (shape, key, value)
        tried += 1
    assert tried > 0


@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("shape,dims", [("star2d1r", (70, 260)), ("box3d1r", (35, 17, 130))])
def test_a_run_is_ordered_on_its_stream(ctx, shape, dims, scenario):
    """tests/test_gpu_stream_order.py's gate: the run on a non-blocking stream while that stream (A) or the null stream (B)
    holds work -- cold (the grids, the states, the records are allocated inside the gated call), then prepared."""
    import arena as A

    L = ctx.L
    ar = A.carve(L.padded_shape(shape, dims), "f64", 2, 240)
    u, f = ar.views
    _, u0, f0 = host_data(shape, dims)[:3]
    w = symmetric_taps(L, shape, "normalised")
    job = Job("run_theta", [ar], [(ar.bits(0), _bits(ctx.torch, u0)), (ar.bits(1), _bits(ctx.torch, f0))],
              lambda: L.Plan(shape, dims).set_weights(w),
              lambda p, s: p.run_theta(u, f, 8.0, 2, theta=0.5, max_iters=6, rtol=1e-2, stream=s),
              prepare=lambda p: p.prepare_theta(2), blocking=True)
    key = ("theta", shape, scenario)
    try:
        ref = ctx.reference(key, job)
        assert ref.ret.steps_done == 2 and not ref.ret.breakdown, ref.ret
        ctx.check(key, job, scenario, "cold")
        ctx.check(key, job, scenario, "prepared")
    finally:
        ctx.torch.cuda.synchronize()
        ctx.refs.pop(key, None)


def test_run_host_theta_is_the_plan_driver(L):
    """the shape's own taps divided by their sum (the thread's normalise default): symmetric, non-negative"""
    import torch

    lib = L._lib.lib()
    shape, dims = "star2d3r", (6, 10)
    rng = np.random.default_rng(9)
    x = rng.integers(-3, 4, L.padded_shape(shape, dims)).astype(np.float64)
    f = padded_with_interior(L, shape, dims, rng.integers(-8, 9, dims).astype(np.float64))
    old = lib.lora_set_default_normalize(1)
    try:
        out, res, info = L.run_host_theta(shape, x, 8.0, 3, source=f, theta=0.5, max_iters=40, rtol=1e-8)
        plan = L.Plan(shape, dims)
    finally:
        lib.lora_set_default_normalize(old)
    dx, df = torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()
    ref = plan.run_theta(dx, df, 8.0, 3, theta=0.5, max_iters=40, rtol=1e-8)
    print("run_host_theta:", res, info.sweep_seconds)
    assert res.steps_done == 3 and res.unconverged_steps == 0
    assert res == ref._replace(iterations=()) and np.array_equal(out.view(np.int64), dx.cpu().numpy().view(np.int64))
    assert info.steps_per_launch == 1 and info.hbm_gbs > 0
    assert info.hbm_gbs == pytest.approx(60 * 3 * (4 + 11 * res.iterations_total / 3) * 8 / info.sweep_seconds / 1e9)


def test_the_cli_prints_its_four_lines(L):
    """the reference's three lines, counting steps, then the stepper's own (starting the tool is what this test is about)"""
    import os
    import re
    import subprocess
    from conftest import ROOT

    p = subprocess.run([os.path.join(ROOT, "lorastencil_amd", "bin", "lorastencil_2d"), "star2d1r", "256", "256", "4", "--normalize", "--bc=dirichlet",
                        "--implicit=64", "--iters=80", "--source=const:1"], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and lines[0].startswith("INFO: shape = star_2d1r, m = 256, n = 256, times = 4")
    assert lines[1] == "LoRAStencil(2D star_2d1r): " and lines[2].startswith("Time = ") and lines[3].startswith("GStencil/s = ")
    m = re.match(r"Implicit: theta = 1, tau = 64, steps = 4, iterations = (\d+) \(max (\d+) of 80 a step, rtol 1e-08\), unconverged steps = (\d+), "
                 r"steady residual = (\S+) \(max \|S\(u\) \+ f - u\|\)$", lines[4])
    assert m, lines[4]
    assert 4 <= int(m.group(1)) <= 320 and int(m.group(2)) <= 80 and math.isfinite(float(m.group(4)))
    assert any(s.startswith("Source: f = 1 on every interior cell (du/dt = S(u) + f - u)") for s in lines)
