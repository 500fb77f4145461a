"""GPU tests of the one-launch small CG (kernels_cg_small.hip, lora_plan_cg_small) and of plan option "coarse1", which puts it on
the coarsest level of the multigrid cycle (mg.cpp).

Yardsticks, none of them the code under test: a numpy model of the header's per-iteration formulas written here, one numpy
operation per rounding, which never calls the engine; ``numpy.linalg.solve`` on dense systems; Python loops over the public
entries (the classes of tests/test_gpu_mg.py and tests/test_gpu_pcg.py with ``Plan.cg_small`` on the coarsest level) for the
bits of a cycle; the numpy V-cycle model and the bounds of those two files for the drivers.

Engine against model.  Both are fp64 runs of one algorithm that differ in summation order (the kernel's tap sum is a chain of
fused multiply-adds, its dots fold lane by lane, wave by wave), so the yardstick for "how far apart may two such runs be" is the
model against itself with its tap sums and dots in the opposite order, with a tenfold margin, computed in the test and never
taken from the engine's output.  x is measured relative to max |x|, r relative to max |r0|: once a solve has converged the two
orders' residuals differ by as little as 1e-52 of |r0|, which is why the allowance has a floor of ten units in the last place,
10 * 2**-52.  CHECKED in numpy before the engine ran: on the shapes below the two orders differ by 7e-18 to 6.5e-16 in x and by
6.6e-16 down to 1e-82 in r.  MEASURED on the MI355X afterwards, over the 72 cases: the kernel is at most 6.5e-16 from the model
in x, 5.2e-16 in r and 1.6e-16 in rr0, and with as many iterations as cells 2.5e-16 to 7.2e-16 from numpy.linalg.solve.

Buffers are carved by tests/arena.py at offsets 16 and 240: NaN guard bands, NaN in every halo cell of x and r.
"""
import functools
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

import test_gpu_mg as M
import test_gpu_pcg as P

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
PAIRS = [(1.0, 1.0), (9.0, 8.0)]
FLOOR = 10.0 * 2.0 ** -52

DIMS_2D = [(4, 4), (5, 6), (7, 6), (4, 130), (12, 34), (32, 32)]
DIMS_3D = [(4, 4, 4), (5, 7, 6), (4, 6, 34)]
KERNEL_CASES = [(s, d) for s in ("star2d1r", "box2d3r") for d in DIMS_2D] + [(s, d) for s in ("star3d1r", "box3d1r") for d in DIMS_3D]
KERNEL_IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d in KERNEL_CASES]
DENSE_DIMS = [(4, 4), (5, 6), (7, 6)]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


@functools.lru_cache(maxsize=None)
def normalised_taps(shape):
    """the shape's own taps divided by their sum (what --normalize runs): point-symmetric, every tap of the support"""
    import lorastencil_amd as L
    from lorastencil_amd import _lib

    old = _lib.lib().lora_set_default_normalize(1)
    try:
        w = L.Plan(shape, (4, 4) if "2d" in shape else (4, 4, 4)).weights.copy()
    finally:
        _lib.lib().lora_set_default_normalize(old)
    assert abs(w.sum() - 1.0) < 1e-12 and np.array_equal(w, w[::-1])
    w.setflags(write=False)
    return w


# ---- the model: the header's formulas, one numpy operation per rounding ------------------------------------------------------------
def model_dot(a, b, order):
    prod = (a * b).ravel()
    return float(np.sum(prod if order > 0 else prod[::-1]))


def model_cg(w, x0, r0, iters, sigma, tau, order):
    """(x, r, rr0, rr, iterations done, halt) of lora_plan_cg_small on interior arrays with a zero halo"""
    x, r = x0.copy(), r0.copy()
    p = r.copy()
    rr = model_dot(r, r, order)
    rr0, done, halt = rr, 0, 0
    for _ in range(iters):
        if rr == 0.0:
            halt = 1
            break
        acc = P.model_sweep(w, p, order)
        q = p - acc if (sigma, tau) == (1.0, 1.0) else sigma * p - tau * acc
        pq = model_dot(p, q, order)
        if not (math.isfinite(pq) and pq > 0.0):
            halt = 2
            break
        alpha = rr / pq
        x = x + alpha * p
        r = r - alpha * q
        rr_new = model_dot(r, r, order)
        done += 1
        if not math.isfinite(rr_new):
            rr, halt = rr_new, 2
            break
        beta = rr_new / rr
        rr = rr_new
        p = r + beta * p
    return x, r, rr0, rr, done, halt


@functools.lru_cache(maxsize=None)
def data(shape, dims):
    rng = np.random.default_rng(zlib.crc32(repr(("cg_small", shape, dims)).encode()))
    x0, r0 = rng.standard_normal(dims) * 2.0, rng.standard_normal(dims)
    x0.setflags(write=False)
    r0.setflags(write=False)
    return x0, r0


@functools.lru_cache(maxsize=None)
def reference(shape, dims, sigma, tau, iters):
    """the model in both summation orders, made once, and the allowances it gives for x, r and rr0"""
    w = normalised_taps(shape)
    x0, r0 = data(shape, dims)
    a, b = (model_cg(w, x0, r0, iters, sigma, tau, order) for order in (1, -1))
    dev_x = np.abs(a[0] - b[0]).max() / np.abs(a[0]).max()
    dev_r = np.abs(a[1] - b[1]).max() / np.abs(r0).max()
    dev_rr0 = abs(a[2] - b[2]) / a[2]
    return a, dict(x=max(10.0 * dev_x, FLOOR), r=max(10.0 * dev_r, FLOOR), rr0=max(10.0 * dev_rr0, FLOOR)), (dev_x, dev_r)


def iteration_counts(dims):
    return (4, min(64, int(np.prod(dims))))


class Solve:
    """x and r carved with NaN halos, the four doubles of d_info NaN; one call; the checks every call must pass"""

    def __init__(self, L, shape, dims, x0, r0, offset):
        import torch

        self.L, self.shape, self.dims = L, shape, dims
        self.g = P.Grids(L, shape, dims, offset, [P.padded(L, shape, dims, x0, np.nan), P.padded(L, shape, dims, r0, np.nan)])
        self.info = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
        self.halo = ~self.g.interior_mask()
        self.before = (self.g.bits(0), self.g.bits(1))

    def run(self, plan, iters, sigma=1.0, tau=1.0, with_info=True, what=""):
        import torch

        plan.cg_small(self.g.v[0], self.g.v[1], iters, sigma, tau, self.info if with_info else None)
        self.g.guards(what)
        for i in (0, 1):
            assert torch.equal(self.g.arena.bits(i)[self.halo], self.before[i][self.halo]), what + f": a halo cell of grid {i} was written"
        return self.g.host(0), self.g.host(1), self.info.cpu().numpy()


# ---- 1. the kernel against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_against_the_numpy_model(L, shape, dims):
    w = normalised_taps(shape)
    x0, r0 = data(shape, dims)
    plan = L.Plan(shape, dims).set_weights(w)
    assert plan.get_option("cg_small") == 1
    for (sigma, tau), off in zip(PAIRS, OFFSETS):
        for iters in iteration_counts(dims):
            (mx, mr, mrr0, mrr, mdone, mhalt), allow, dev = reference(shape, dims, sigma, tau, iters)
            what = f"{shape} {dims} ({sigma}, {tau}) iters {iters}"
            x, r, info = Solve(L, shape, dims, x0, r0, off).run(plan, iters, sigma, tau, what=what)
            err_x = np.abs(x - mx).max() / np.abs(mx).max()
            err_r = np.abs(r - mr).max() / np.abs(r0).max()
            err_rr0 = abs(info[0] - mrr0) / mrr0
            print(what, "model's two orders differ by", dev, "allow", allow, "engine against model: x", err_x, "r", err_r, "rr0", err_rr0,
                  "info", info, "model rr", mrr)
            assert mdone == iters and mhalt == 0
            assert np.isfinite(x).all() and np.isfinite(r).all(), what + ": a NaN of a halo reached a result"
            assert err_x <= allow["x"], f"{what}: x is {err_x} from the model's, allowed {allow['x']}"
            assert err_r <= allow["r"], f"{what}: r is {err_r} of max |r0| from the model's, allowed {allow['r']}"
            assert err_rr0 <= allow["rr0"] and info[2] == iters and info[3] == 0, f"{what}: d_info {info}"


def dense_A(w, dims, sigma, tau):
    n = int(np.prod(dims))
    eye = np.eye(n).reshape((n,) + tuple(dims))
    return np.stack([(sigma * e - tau * P.model_sweep(w, e)).ravel() for e in eye], axis=1)


@pytest.mark.parametrize("shape", ["star2d1r", "box2d3r"])
@pytest.mark.parametrize("dims", DENSE_DIMS, ids=["4x4", "5x6", "7x6"])
def test_as_many_iterations_as_cells_is_the_dense_solve(L, shape, dims):
    w = normalised_taps(shape)
    x0, r0 = data(shape, dims)
    cells = int(np.prod(dims))
    plan = L.Plan(shape, dims).set_weights(w)
    for (sigma, tau), off in zip(PAIRS, OFFSETS):
        A = dense_A(w, dims, sigma, tau)
        want = np.linalg.solve(A, r0.ravel() + A @ x0.ravel()).reshape(dims)  # r0 = b - A x0
        model = model_cg(w, x0, r0, cells, sigma, tau, 1)[0]
        what = f"{shape} {dims} ({sigma}, {tau}) iters {cells}"
        x, _, info = Solve(L, shape, dims, x0, r0, off).run(plan, cells, sigma, tau, what=what)
        err, merr = np.abs(x - want).max() / np.abs(want).max(), np.abs(model - want).max() / np.abs(want).max()
        print(what, "against numpy.linalg.solve: engine", err, "model", merr, "info", info)
        assert err <= 1e-13, f"{what}: x is {err} from the dense solve"


# ---- 2. determinism and memory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", [("box2d3r", (12, 34)), ("star2d1r", (4, 130)), ("box3d1r", (5, 7, 6))])
def test_same_bits_every_time_and_nothing_else_is_touched(L, shape, dims):
    import torch

    w = normalised_taps(shape)
    x0, r0 = data(shape, dims)
    plan = L.Plan(shape, dims).set_weights(w)
    iters = 7
    runs = []
    for off, with_info in ((16, True), (240, True), (16, False)):
        s = Solve(L, shape, dims, x0, r0, off)
        s.run(plan, iters, 9.0, 8.0, with_info=with_info, what=f"{shape} {dims} offset {off} info {with_info}")
        runs.append((s.g.bits(0), s.g.bits(1), s.info.clone()))
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1]), "the same call gave other bits"
    assert torch.equal(runs[0][2].view(torch.int64), runs[1][2].view(torch.int64))
    assert bool(torch.isnan(runs[2][2]).all()), "d_info was NULL: nothing may have written the four doubles"
    (_, _, mrr0, mrr, _, _), allow, _ = reference(shape, dims, 9.0, 8.0, iters)
    info = runs[0][2].cpu().numpy()
    print(shape, dims, "info", info, "model rr0, rr", mrr0, mrr)
    assert abs(info[0] - mrr0) / mrr0 <= allow["rr0"] and info[2] == iters and info[3] == 0
    # rr = r.r moves with r: |d rr| <= 2 |r|_2 |d r|_2 <= 2 sqrt(rr) sqrt(cells) max |d r| (Cauchy-Schwarz), and the fold's own rounding
    cells = int(np.prod(dims))
    bound = 2.0 * math.sqrt(mrr * cells) * allow["r"] * np.abs(r0).max() + cells * 2.0 ** -52 * mrr
    assert abs(info[1] - mrr) <= bound, f"rr {info[1]} is {abs(info[1] - mrr)} from the model's {mrr}, allowed {bound}"


# ---- 3. halting -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", [("star2d1r", (4, 4)), ("box2d3r", (12, 34)), ("star3d1r", (4, 6, 34))])
def test_halting(L, shape, dims):
    import torch

    w = normalised_taps(shape)
    x0, r0 = data(shape, dims)
    plan = L.Plan(shape, dims).set_weights(w)
    # a residual that is zero: converged before the first iteration
    s = Solve(L, shape, dims, x0, np.zeros(dims), 16)
    _, r, info = s.run(plan, 5, what=f"{shape} {dims} r0 = 0")
    print(shape, dims, "r0 = 0: info", info)
    assert torch.equal(s.g.arena.bits(0), s.before[0]) and not r.any()
    assert info[0] == 0.0 and info[1] == 0.0 and info[2] == 0 and info[3] == 1
    # a negative definite operator, -I - S: p.q < 0 in the first iteration, a breakdown that leaves x and r alone
    s = Solve(L, shape, dims, x0, r0, 240)
    s.run(plan, 5, -1.0, 1.0, what=f"{shape} {dims} sigma = -1")
    info = s.info.cpu().numpy()
    print(shape, dims, "sigma = -1: info", info)
    assert torch.equal(s.g.arena.bits(0), s.before[0]) and torch.equal(s.g.arena.bits(1), s.before[1])
    assert info[2] == 0 and info[3] == 2 and info[0] == info[1] > 0.0
    assert model_cg(w, x0, r0, 5, -1.0, 1.0, 1)[4:] == (0, 2)


# ---- 4. the cycle -----------------------------------------------------------------------------------------------------------------
class MgCycle1(M.PublicCycle):
    """tests/test_gpu_mg.py's loop over the public entries with Plan.cg_small standing for the coarsest level's CG"""

    def cycle(self, l, cur, other):
        if l == self.last:
            self.plain[l].cg_small(cur, self.g[l], self.iters)
            return cur
        return super().cycle(l, cur, other)


class PcgCycle1(P.PublicCycle):
    """tests/test_gpu_pcg.py's z = M r for (sigma, tau) with Plan.cg_small on the coarsest level"""

    def cycle(self, l, cur, other):
        if l == self.last:
            self.plain[l].cg_small(cur, self.g[l], self.iters, self.sigma, self.tau)
            return cur
        return super().cycle(l, cur, other)


def cycle_problem(L, shape, dims):
    rng = np.random.default_rng(zlib.crc32(repr(("coarse1 cycle", shape, dims)).encode()))
    w = M.jacobi_taps(2) if shape == "star2d1r" else P.symmetric_random_taps(L, shape, rng)
    ps = L.padded_shape(shape, dims)
    return w, rng.standard_normal(ps), rng.standard_normal(ps)  # non-zero halo values in x0: the boundary


CYCLE_CASES = [("star2d1r", (64, 64), (4, 4)), ("box3d1r", (16, 24, 32), (4, 6, 8))]
CYCLE_IDS = ["64x64", "16x24x32"]


@pytest.mark.parametrize("shape,dims,coarsest", CYCLE_CASES, ids=CYCLE_IDS)
def test_cycles_equal_the_loop_over_the_public_entries(L, shape, dims, coarsest):
    import torch

    w, x0, f = cycle_problem(L, shape, dims)
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    ref = MgCycle1(L, shape, dims, w, 0.8, 2, 2, True)
    assert ref.tab[-1][0] == coarsest and ref.plain[-1].get_option("cg_small") == 1
    for cycles, off in zip((1, 2, 3), (16, 240, 16)):
        g = M.Grids(L, shape, dims, off, [x0, f])
        before_x, before_f, halo = g.bits(0), g.bits(1), ~g.interior_mask()
        res = plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=cycles)
        g.guards(f"{shape} {dims} coarse1 x{cycles}")
        assert res.until.times_done == cycles and res.level_dims[-1] == coarsest
        assert torch.equal(g.arena.bits(1), before_f) and torch.equal(g.arena.bits(0)[halo], before_x[halo])
        expect = ref.run(x0, f, cycles)
        assert M.same_bits(g.v[0], expect), f"{shape} {dims}: d_x after {cycles} cycle(s) differs from the loop with Plan.cg_small"
    # the one launch folds its sums in another order than the launches it replaces: the cycles agree to rounding level
    off_plan = L.Plan(shape, dims).set_weights(w)
    g_off, g_on = (M.Grids(L, shape, dims, 16, [x0, f]) for _ in range(2))
    off_plan.run_mg_until(g_off.v[0], g_off.v[1], tol=0.0, check_every=1, max_times=1)
    plan.run_mg_until(g_on.v[0], g_on.v[1], tol=0.0, check_every=1, max_times=1)
    a, b = g_off.host(0), g_on.host(0)
    print(shape, dims, "one cycle, option off against on: max difference", np.abs(a - b).max(), "of", np.abs(a).max())
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()


@pytest.mark.parametrize("shape,dims,coarsest", CYCLE_CASES, ids=CYCLE_IDS)
def test_preconditioner_equals_the_composition_of_the_public_entries(L, shape, dims, coarsest):
    import torch

    w, r0, _ = cycle_problem(L, shape, dims)
    sigma, tau = 9.0, 8.0
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    ref = PcgCycle1(L, shape, dims, w, 0.8, 2, 2, sigma, tau)
    assert ref.tab[-1][0] == coarsest
    g = P.Grids(L, shape, dims, 240, [None, None])  # r: its halo stays NaN; z: NaN everywhere
    every = g.interior_mask()
    g.v[0][every] = torch.from_numpy(r0).cuda()[every]
    before_r = g.bits(0)
    plan.mg_precondition(g.v[0], g.v[1], sigma, tau, pre=2, post=2, omega=0.8)
    g.guards(f"{shape} {dims} precondition")
    assert torch.equal(g.arena.bits(0), before_r), "d_r was written"
    expect = ref.apply(g.v[0])
    assert P.same_bits(L.interior(shape, g.v[1]), expect), f"{shape} {dims}: d_z differs from the composition with Plan.cg_small"
    assert float(expect.abs().max()) > 0.0


def one_cycle_cost(L, shape, dims, w, x0, f, coarse1, **kw):
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", coarse1)
    g = M.Grids(L, shape, dims, 16, [x0, f])
    res = plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=1, **kw)
    g.guards(f"{shape} {dims} coarse1 {coarse1}")
    return plan.mg_cycle_cost(), res


def test_cycle_cost_counts_the_level_as_one_launch(L):
    """V(2,2) with f.  TODAY'S COUNT from the header: a 2D level below the coarsest is six launches (two smoothing applications
    in one launch, the defect, the restriction, the zeroing, the prolongation, two applications in one launch), a 3D level
    eight (single sweeps), the coarsest 5 + 5 iters: 4 x 6 + 85 = 109 at 64 x 64, 2 x 8 + 325 = 341 at 16 x 24 x 32."""
    for (shape, dims, coarsest), today in zip(CYCLE_CASES, (109, 341)):
        w, x0, f = cycle_problem(L, shape, dims)
        iters = min(64, int(np.prod(coarsest)))
        (n_off, b_off), _ = one_cycle_cost(L, shape, dims, w, x0, f, 0)
        (n_on, b_on), _ = one_cycle_cost(L, shape, dims, w, x0, f, 1)
        print(shape, dims, "launches per cycle: off", n_off, "on", n_on, "bytes: off", b_off, "on", b_on)
        assert n_off == today
        assert n_off - n_on == 5 + 5 * iters - 1
        cells = float(np.prod(coarsest))
        assert b_off - b_on == 8.0 * cells * (3.0 + 11.0 * iters) - 8.0 * cells * 4.0
        # a shallower hierarchy whose coarsest level still fits: 32 x 32 in 2D
        if shape == "star2d1r":
            (m_off, _), res = one_cycle_cost(L, shape, dims, w, x0, f, 0, max_levels=2)
            (m_on, _), _ = one_cycle_cost(L, shape, dims, w, x0, f, 1, max_levels=2)
            assert res.level_dims[-1] == (32, 32) and m_off - m_on == 5 + 5 * 64 - 1


def test_a_coarsest_level_that_does_not_fit_changes_nothing(L):
    shape, dims = "star2d1r", (16, 4096)
    w = M.jacobi_taps(2)
    rng = np.random.default_rng(11)
    ps = L.padded_shape(shape, dims)
    x0, f = rng.standard_normal(ps), rng.standard_normal(ps)
    coarsest = dims
    while True:
        try:
            coarsest = L.mg_coarse_dims(shape, coarsest)
        except L.LoraError:
            break
    fits = L.Plan(shape, coarsest).get_option("cg_small")
    plan_off, plan_on = L.Plan(shape, dims).set_weights(w), L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    g_off, g_on = (M.Grids(L, shape, dims, 240, [x0, f]) for _ in range(2))
    r_off = plan_off.run_mg_until(g_off.v[0], g_off.v[1], tol=0.0, check_every=1, max_times=1)
    r_on = plan_on.run_mg_until(g_on.v[0], g_on.v[1], tol=0.0, check_every=1, max_times=1)
    g_on.guards("16 x 4096 coarse1")
    n_off, n_on = plan_off.mg_cycle_cost()[0], plan_on.mg_cycle_cost()[0]
    print(shape, dims, "coarsest", coarsest, "cg_small", fits, "launches off", n_off, "on", n_on)
    assert r_on.level_dims[-1] == coarsest == r_off.level_dims[-1]
    assert (n_on == n_off) == (fits == 0)
    if fits == 0:
        assert M.same_bits(g_off.v[0], g_on.v[0]), "the level does not fit: the existing launches run, the same bits"


def test_the_thread_default_reaches_the_drivers_plan_and_comes_back(L):
    shape, dims, coarsest = CYCLE_CASES[0]
    w, x0, f = cycle_problem(L, shape, dims)
    (n_on, _), _ = one_cycle_cost(L, shape, dims, w, x0, f, 1)
    assert L.set_default_coarse1(1) == 0
    try:
        plan = L.Plan(shape, dims).set_weights(w)
        assert plan.get_option("coarse1") == 1
        g = M.Grids(L, shape, dims, 16, [x0, f])
        plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=1)  # builds the hierarchy's internal plans
        assert plan.mg_cycle_cost()[0] == n_on
        assert L.set_default_coarse1(1) == 1, "building the hierarchy changed the thread's default"
    finally:
        L.set_default_coarse1(0)


# ---- 5. the drivers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def independence_on(n):
    """tests/test_gpu_mg.py's independence(n) for the engine with coarse1 on: the residual after every cycle until it is <= 1e-8 |f|"""
    import lorastencil_amd as L

    shape, dims = "star2d1r", (n, n)
    w = M.jacobi_taps(2)
    f = np.random.default_rng(5).standard_normal(dims)
    target = 1e-8 * np.abs(f).max()
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    g = M.Grids(L, shape, dims, 16, [M.padded(L, shape, dims, np.zeros(dims), 0.0), M.padded(L, shape, dims, f, 0.0)])
    engine = []
    while not engine or (engine[-1] > target and len(engine) < 40):
        engine.append(plan.run_mg_until(g.v[0], g.v[1], tol=0.0, pre=2, post=2, omega=0.8, check_every=1, max_times=1).until.residual)
    g.guards(f"grid independence {dims} coarse1")
    return engine


def test_multigrid_keeps_the_models_residuals(L):
    deviation = 0.0
    for n in (64, 256):
        model, _, _ = M.independence(n)
        deviation = max([deviation] + [max(a / b, b / a) - 1.0 for a, b in zip(model[0][:6], model[1][:6])])
    factor = 1.0 + 10.0 * deviation
    print("the model's two tap orders differ by a factor of", 1.0 + deviation, "-> allowed factor", factor)
    for n in (64, 256):
        model, off, _ = M.independence(n)
        on = independence_on(n)
        ratios = [max(a / b, b / a) for a, b in zip(on[:6], model[0][:6])]
        print(n, "cycles to 1e-8: option off", len(off), "on", len(on), "; on / model over the first six cycles:",
              " ".join(f"{r - 1:.2e}" for r in ratios))
        assert len(ratios) == 6 and all(r <= factor for r in ratios), f"{n}: a residual of the first six cycles is a factor {max(ratios)} from the model's"
        assert on[-1] <= 1e-8 * np.abs(np.random.default_rng(5).standard_normal((n, n))).max()
        assert abs(len(on) - len(off)) <= 1, f"{n}: {len(on)} cycles with the option, {len(off)} without"


def test_pcg_solves_the_jacobi_problem(L):
    """tests/test_gpu_pcg.py's problem, cap and bound at 64 x 64"""
    shape, dims = "star2d1r", (64, 64)
    w = P.jacobi_taps(2)
    rng = np.random.default_rng(zlib.crc32(repr(("solve", dims)).encode()))
    ps = L.padded_shape(shape, dims)
    f = P.padded(L, shape, dims, rng.standard_normal(dims), 0.0)
    x = P.padded(L, shape, dims, np.zeros(dims), rng.standard_normal(ps))
    S, b = P.dense_operator(L, shape, dims, w, x)
    n = S.shape[0]
    tol = 1e-12 * np.abs(f).max()
    rho = P.jacobi_rho(dims)
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    g = P.Grids(L, shape, dims, 240, [x, f])
    res = plan.run_pcg_until(g.v[0], g.v[1], tol=tol, check_every=2, max_times=40)
    g.guards(f"{shape} {dims} pcg coarse1")
    err = np.abs(g.host(0).ravel() - np.linalg.solve(np.eye(n) - S, L.interior(shape, f).ravel() + b)).max()
    print(shape, dims, res, "error against numpy.linalg.solve:", err, "bound", tol / (1 - rho))
    assert res.until.converged and not res.until.diverged and not res.breakdown and res.until.residual <= tol
    assert err <= tol / (1 - rho)


@pytest.mark.parametrize("shape,dims", [("star2d1r", (16, 16)), ("star3d1r", (8, 8, 8))])
def test_each_implicit_step_is_the_dense_solve(L, shape, dims):
    """tests/test_gpu_pcg.py's test_each_step_is_the_dense_solve at tau = 64: its cap of 40 iterations, its bound 2 rtol |r0|_2"""
    w = P.jacobi_taps(len(dims))
    rng = np.random.default_rng(zlib.crc32(repr(("theta dense", dims)).encode()))
    ps = L.padded_shape(shape, dims)
    u0, f = rng.standard_normal(ps), P.padded(L, shape, dims, rng.standard_normal(dims), 0.0)
    S, halo_part = P.dense_operator(L, shape, dims, w, u0)
    n, rtol, tau = S.shape[0], 1e-10, 64.0
    fi = L.interior(shape, f).ravel()
    plan = L.Plan(shape, dims).set_weights(w).set_option("coarse1", 1)
    g = P.Grids(L, shape, dims, 16, [u0, f])
    for step in range(2):
        u = g.host(0).ravel()
        r0 = tau * (S @ u + halo_part + fi - u)
        want = np.linalg.solve((1.0 + tau) * np.eye(n) - tau * S, u + tau * fi + tau * halo_part)
        res = plan.run_theta_mg(g.v[0], g.v[1], tau, 1, theta=1.0, max_iters=40, rtol=rtol, check_every=2)
        err = np.abs(g.host(0).ravel() - want).max()
        bound = 2.0 * rtol * float(np.sqrt((r0 * r0).sum()))
        print(shape, dims, "tau", tau, "step", step, "iterations", res.iterations, "error", err, "bound", bound)
        assert res.steps_done == 1 and res.unconverged_steps == 0 and not res.breakdown
        assert err <= bound
    g.guards(f"{shape} {dims} theta_mg coarse1")


def test_cli_flag_coarse1(L):
    """starting the tools is what this test is about"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe2, exe3 = (os.path.join(root, "lorastencil_amd", "bin", f"lorastencil_{d}d") for d in (2, 3))
    run = lambda *a: subprocess.run(list(a), capture_output=True, text=True, timeout=120)
    r = run(exe2, "star2d1r", "64", "64", "40", "--mg", "--normalize", "--source=point:1", "--until=1e-9", "--coarse1")
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert any(ln.startswith("Multigrid: V(2,2) cycles = ") and ln.endswith("levels = 5, coarsest = 4 x 4") for ln in r.stdout.splitlines())
    assert any(", converged, " in ln for ln in r.stdout.splitlines())
    r = run(exe3, "star3d1r", "16", "16", "16", "40", "--pcg=1", "--normalize", "--until=1e-9", "--coarse1")
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and any(", converged, " in ln for ln in r.stdout.splitlines())
    r = run(exe2, "star2d1r", "64", "64", "3", "--normalize", "--bc=dirichlet", "--implicit=64", "--precond=mg", "--iters=30", "--source=const:1",
            "--coarse1")
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and any("unconverged steps = 0" in ln for ln in r.stdout.splitlines())


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------
def test_the_launch_is_ordered_behind_a_long_sweep_on_its_stream(L):
    """tests/test_gpu_stream_order.py's scenario A for one entry: a gate (one workgroup spinning for a bounded time), then a long
    run of sweeps that produces the residual, then lora_plan_cg_small, all on one non-blocking stream.  A launch that did not wait
    for its stream would read the residual before the sweeps wrote it."""
    import torch

    shape, dims, iters, sweeps = "star2d1r", (32, 32), 12, 400
    w = normalised_taps(shape)
    x0, r_in = data(shape, dims)
    sweep = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_option("graph", 0)
    plan = L.Plan(shape, dims).set_weights(w)

    def sequence(stream, wait):
        g = P.Grids(L, shape, dims, 16, [P.padded(L, shape, dims, x0, 0.0), P.padded(L, shape, dims, r_in * 1e3, 0.0),
                                         P.padded(L, shape, dims, np.zeros(dims), 0.0)])
        torch.cuda.synchronize()
        busy = None
        with torch.cuda.stream(stream):
            if not wait:
                torch.cuda._sleep(40_000_000)  # 20 ms at a 2 GHz counter, 400 ms at 100 MHz: longer than the enqueueing below
            sweep.run(g.v[1], g.v[2], sweeps, stream=stream)  # an even count: the result is back in grid 1
            if wait:
                torch.cuda.synchronize()
            plan.cg_small(g.v[0], g.v[1], iters, stream=stream)
            busy = not stream.query()
        torch.cuda.synchronize()
        g.guards(f"stream order, wait {wait}")
        return g, busy

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.zeros(8, device="cuda").add_(1.0)  # the first use of a stream sets up its queue
    torch.cuda.synchronize()
    ref, _ = sequence(s, True)
    got, busy = sequence(s, False)
    assert busy, "the stream had drained when the call returned: the gate was too short to show anything"
    assert float(ref.v[1].abs().max()) > 0.0 and not P.same_bits(ref.v[0], torch.from_numpy(P.padded(L, shape, dims, x0, 0.0)).cuda())
    assert P.same_bits(ref.v[0], got.v[0]) and P.same_bits(ref.v[1], got.v[1])
