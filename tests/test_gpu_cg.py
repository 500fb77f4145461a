"""GPU tests of the conjugate-gradient kernels and driver (kernels_cg.hip, cg.cpp; the dot reduction: kernels_reduce.hip).

Yardsticks: the engine's older code -- ``plan.step_region`` into a spare grid, then an elementwise subtraction -- for the bits
of q; exact integer sums and ``math.fsum`` on host copies for the records; numpy, which rounds ``x + alpha * p`` twice, for the
pointwise kernels; a Python loop over the public entries for the driver; ``numpy.linalg.solve`` and the header's closed form of
rho for the solver.

Grids: the fp64 cases of tests/test_gpu_residual.py with their regions -- the smallest that reach every path of the tile walk
apply_dot inherits (one cell; a partial tile and two tiles per direction; regions that begin and end inside a tile; the empty
one; 1027 = 2 x 512 + 3: the odd tail point; 33 x 130: one row and one column pair in second tiles; 70 x 258 with [5, 37); 34 x
18 x 130 whole and with regions of 1, 2 and 3 planes, which end the plane ring in each of its three phases).  Taps are set
explicitly: small symmetric integers, and non-negative symmetric taps divided by their sum.  Buffers are carved by tests/arena.py at offsets 16 and 240, the guard bands NaN.
"""
import functools
import itertools
import math
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
U = 2.0 ** -53

CASES = [
    ("1d1r", (1,), [(0, 0)]),
    ("1d2r", (1027,), [(0, 0), (2, 515), (510, 1027), (4, 4)]),
    ("star2d1r", (1, 2), [(0, 0)]),
    ("star2d1r", (70, 260), [(0, 0), (5, 37), (33, 70), (7, 7)]),
    ("star2d3r", (70, 260), [(0, 0), (5, 37)]),
    ("box2d3r", (70, 260), [(0, 0), (33, 70)]),
    ("star3d1r", (1, 1, 2), [(0, 0)]),
    ("box3d1r", (35, 17, 130), [(0, 0), (1, 34), (33, 35), (9, 9)]),
    ("star3d1r", (35, 17, 130), [(0, 0), (1, 34)]),
    # the edges of the shared walk (csrc/tile_walk.h), as in tests/test_gpu_residual.py
    ("star2d1r", (33, 130), [(0, 0)]),
    ("star2d3r", (33, 130), [(0, 0)]),
    ("box2d3r", (33, 130), [(0, 0)]),
    ("star2d1r", (70, 258), [(5, 37)]),
    ("star2d3r", (70, 258), [(5, 37)]),
    ("box2d3r", (70, 258), [(5, 37)]),
    ("box3d1r", (34, 18, 130), [(0, 0), (3, 4), (3, 5), (3, 6)]),
    ("star3d1r", (34, 18, 130), [(0, 0), (3, 4), (3, 5), (3, 6)]),
]
IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d, _ in CASES]
SEVERAL = [c for c in CASES if c[1] in ((1027,), (70, 260), (35, 17, 130))]
SEVERAL_IDS = [IDS[CASES.index(c)] for c in SEVERAL]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def symmetric_taps(L, shape, kind):
    """point-symmetric taps on the support of the shape's own: small integers 1..3, or the same divided by their sum"""
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    t = np.arange(w.size)
    ints = np.where(w != 0, 1.0 + np.minimum(t, w.size - 1 - t) % 3, 0.0)
    assert np.array_equal(ints, ints[::-1])
    return ints if kind == "int" else ints / ints.sum()


def make_plan(L, shape, dims, kind):
    p = L.Plan(shape, dims).set_weights(symmetric_taps(L, shape, kind))
    assert p.get_option("cg") == 1
    return p


@functools.lru_cache(maxsize=None)
def host_data(shape, dims):
    """whole padded arrays every test of a case starts from, made once, read-only: integers 0..99 and seeded normal values"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("cg", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    out = [rng.integers(0, 100, ps).astype(np.float64)] + [rng.standard_normal(ps) * 3.0 for _ in range(4)]
    for a in out:
        a.setflags(write=False)
    return out


def span(p, begin, end):
    return (0, p.dims[0]) if (begin, end) == (0, 0) else (begin, end)


class Grids:
    """n grids carved from one poisoned allocation; grid i starts as values[i] (whole padded array) or stays NaN (None)"""

    def __init__(self, L, shape, dims, offset, values):
        import torch
        from arena import carve

        self.L, self.shape = L, shape
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=len(values), offset_bytes=offset)
        self.v = self.arena.views
        for view, a in zip(self.v, values):
            if a is not None:
                view.copy_(torch.from_numpy(np.array(a)))
        self.mask = torch.zeros(self.v[0].shape, dtype=torch.bool, device="cuda")

    def region(self, lo, hi):
        """boolean mask of the interior cells of the outermost range [lo, hi)"""
        self.mask.zero_()
        self.L.interior(self.shape, self.mask)[lo:hi] = True
        return self.mask

    def bits(self, i):
        return self.arena.bits(i).clone()

    def guards(self, what):
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)

    def host(self, i, lo, hi):
        return self.L.interior(self.shape, self.v[i]).cpu().numpy()[lo:hi].ravel()


def same_bits(a, b):
    import torch

    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def fbits(x):
    return np.float64(x).tobytes()


def check_record(got, a, b, what):
    """the record of the products of two host vectors within the bound that holds for ANY summation order:
    |dot - fsum| <= (count + 1) u sum |a b|, and sum_abs within the same bound"""
    prod = a * b
    ok = np.isfinite(prod)
    exact, exact_abs = math.fsum(prod[ok]), math.fsum(np.abs(prod[ok]))
    bound = (prod.size + 1) * U * exact_abs
    print(what, "dot", got.dot, "fsum", exact, "sum_abs", got.sum_abs, "fsum", exact_abs, "bound", bound)
    assert got.count == prod.size and got.nonfinite == int((~ok).sum()), what
    assert abs(got.dot - exact) <= bound and abs(got.sum_abs - exact_abs) <= bound, what


def apply_reference(g, p, i_p, lo, hi):
    """q as the older code gives it: step_region into a spare grid, then p - spare, elementwise in fp64"""
    import torch

    spare = torch.zeros_like(g.v[i_p])
    if hi > lo:
        p.step_region(g.v[i_p], spare, lo, hi)
    return g.v[i_p] - spare


def check_apply(g, p, begin, end, what):
    """one apply_dot from grid 0 into grid 1 (whole grid NaN before): q bit for bit the reference on the region's interior,
    every other cell of q -- its halo -- still the NaN it was, p unchanged, the guards intact; returns the record"""
    import torch

    lo, hi = span(p, begin, end)
    g.arena.fill_poison(1)
    before = g.bits(0)
    got = p.apply_dot(g.v[0], g.v[1], begin, end)
    g.guards(what)
    assert torch.equal(g.arena.bits(0), before), what + ": p changed"
    ref = apply_reference(g, p, 0, lo, hi)
    m = g.region(lo, hi)
    assert same_bits(g.v[1][m], ref[m]), what + ": q differs from step_region and a subtraction"
    assert bool(g.arena.is_poison(1)[~m].all()), what + ": a cell of q outside the region's interior was written"
    return got


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_apply_dot_integer_data(L, shape, dims, regions):
    """integers 0..99 and integer taps 1..3: |acc| <= 49 x 3 x 99, every product below 1.5e6 x 99 and their sum over at most
    79560 cells below 2**53 -- exact in any order"""
    ints = host_data(shape, dims)[0]
    p = make_plan(L, shape, dims, "int")
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, [ints, None])
        for begin, end in regions:
            what = f"{shape} {dims} [{begin}, {end}) offset {off}"
            got = check_apply(g, p, begin, end, what)
            lo, hi = span(p, begin, end)
            if hi == lo:
                assert got == L.GridDot(0.0, 0.0, 0, 0), what
                continue
            a, b = g.host(0, lo, hi).astype(np.int64), g.host(1, lo, hi).astype(np.int64)
            assert got == L.GridDot(float((a * b).sum()), float(np.abs(a * b).sum()), a.size, 0), what


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_apply_dot_real_data(L, shape, dims, regions):
    from test_gpu_residual import TUNING

    real = host_data(shape, dims)[1]
    p = make_plan(L, shape, dims, "normalised")
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, [real, None])
        for begin, end in regions:
            what = f"{shape} {dims} [{begin}, {end}) offset {off}"
            got = check_apply(g, p, begin, end, what)
            lo, hi = span(p, begin, end)
            if hi == lo:
                assert got == L.GridDot(0.0, 0.0, 0, 0), what
                continue
            check_record(got, g.host(0, lo, hi), g.host(1, lo, hi), what)
            q = g.bits(1)
            again = check_apply(g, p, begin, end, what + " again")
            assert tuple(map(fbits, again)) == tuple(map(fbits, got)) and np.array_equal(q.cpu().numpy(), g.bits(1).cpu().numpy()), what
            if off == OFFSETS[0] and (begin, end) == regions[0]:  # no tuning option moves a bit
                for key, value in TUNING[len(dims)]:
                    t = make_plan(L, shape, dims, "normalised")
                    if L._lib.lib().lora_plan_set_option(t._h, key.encode(), value) != 0:
                        continue  # (not an option of this plan)
                    tuned = check_apply(g, t, begin, end, f"{what} {key}={value}")
                    assert tuple(map(fbits, tuned)) == tuple(map(fbits, got)), (what, key, value)
                    assert np.array_equal(q.cpu().numpy(), g.bits(1).cpu().numpy()), (what, key, value)


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_dot(L, shape, dims, regions):
    """both grids NaN outside their interiors: no halo cell reaches a result; a NaN interior cell is counted and left out"""
    import torch

    ints, real, real2 = host_data(shape, dims)[:3]
    p = make_plan(L, shape, dims, "normalised")
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, [None, None])
        every = g.region(0, p.dims[0]).clone()
        for values, exact in (((ints, ints[::-1].copy() if len(dims) == 1 else ints.T.copy().reshape(ints.shape)), True), ((real, real2), False)):
            for i in (0, 1):
                g.arena.fill_poison(i)
                g.v[i][every] = torch.from_numpy(np.array(values[i])).cuda()[every]
            before = (g.bits(0), g.bits(1))
            for begin, end in regions:
                what = f"{shape} {dims} [{begin}, {end}) offset {off}"
                lo, hi = span(p, begin, end)
                got, same = p.dot(g.v[0], g.v[1], begin, end), p.dot(g.v[1], g.v[1], begin, end)
                g.guards(what)
                if hi == lo:
                    assert got == same == L.GridDot(0.0, 0.0, 0, 0), what
                    continue
                a, b = g.host(0, lo, hi), g.host(1, lo, hi)
                if exact:  # integers below 100: every sum is exact
                    assert got == L.GridDot(float((a * b).sum()), float(np.abs(a * b).sum()), a.size, 0), what
                    assert same == L.GridDot(float((b * b).sum()), float((b * b).sum()), a.size, 0), what
                else:
                    check_record(got, a, b, what)
                    check_record(same, b, b, what + " a == b")
                    assert tuple(map(fbits, p.dot(g.v[0], g.v[1], begin, end))) == tuple(map(fbits, got)), what
            assert torch.equal(g.arena.bits(0), before[0]) and torch.equal(g.arena.bits(1), before[1])
        # a NaN and an infinity in interior cells of the last region that has cells
        begin, end = [r for r in regions if span(p, *r)[1] > span(p, *r)[0]][-1]
        lo, hi = span(p, begin, end)
        cells = torch.nonzero(g.region(lo, hi).ravel()).ravel()
        g.v[0].view(-1)[cells[0]] = float("nan")
        if len(cells) > 1:
            g.v[1].view(-1)[cells[-1]] = float("inf")
        with np.errstate(invalid="ignore"):
            check_record(p.dot(g.v[0], g.v[1], begin, end), g.host(0, lo, hi), g.host(1, lo, hi), f"{shape} {dims} non-finite cells")


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_cg_update_and_direction_against_numpy(L, shape, dims, regions):
    """x + alpha * p in numpy is two roundings, as the kernel's; cells outside the region's interior keep their bits -- the
    halos of all four grids are NaN"""
    import torch

    ints, x0, r0, p0, q0 = host_data(shape, dims)
    plan = make_plan(L, shape, dims, "normalised")
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, [None] * 4)
        every = g.region(0, plan.dims[0]).clone()

        def load(values):
            for i, a in enumerate(values):
                g.arena.fill_poison(i)
                g.v[i][every] = torch.from_numpy(np.array(a)).cuda()[every]
            return [g.bits(i) for i in range(4)]

        for begin, end in regions:
            what = f"{shape} {dims} [{begin}, {end}) offset {off}"
            lo, hi = span(plan, begin, end)
            m = g.region(lo, hi).clone()
            # real data, an alpha with a full mantissa
            alpha, beta = 0.37 + 2.0 ** -40, -1.0 / 3.0
            before = load([x0, r0, p0, q0])
            h = [g.host(i, lo, hi) for i in range(4)]
            got = plan.cg_update(*g.v, alpha, begin, end)
            g.guards(what)
            want_x, want_r = h[0] + alpha * h[2], h[1] - alpha * h[3]
            assert np.array_equal(g.host(0, lo, hi).view(np.int64), want_x.view(np.int64)), what + ": x"
            assert np.array_equal(g.host(1, lo, hi).view(np.int64), want_r.view(np.int64)), what + ": r"
            for i in range(4):
                assert torch.equal(g.arena.bits(i)[~m], before[i][~m]), f"{what}: grid {i} changed outside the region's interior"
            assert torch.equal(g.arena.bits(2), before[2]) and torch.equal(g.arena.bits(3), before[3]), what + ": p or q changed"
            if hi == lo:
                assert got == L.GridDot(0.0, 0.0, 0, 0), what
            else:
                check_record(got, want_r, want_r, what + " rr")
            # direction: p = r + beta p
            before = [g.bits(i) for i in range(4)]
            h = [g.host(i, lo, hi) for i in range(4)]
            plan.cg_direction(g.v[2], g.v[1], beta, begin, end)
            g.guards(what + " direction")
            assert np.array_equal(g.host(2, lo, hi).view(np.int64), (h[1] + beta * h[2]).view(np.int64)), what + ": p"
            assert torch.equal(g.arena.bits(2)[~m], before[2][~m]), what + ": p changed outside the region's interior"
            for i in (0, 1, 3):
                assert torch.equal(g.arena.bits(i), before[i]), f"{what}: direction changed grid {i}"
            # integer data, alpha = 0.5: every value a multiple of 0.5 below 200, rr exact in any order
            if hi > lo:
                load([ints, ints[::-1].copy() if len(dims) == 1 else ints.T.copy().reshape(ints.shape), ints, ints])
                h = [g.host(i, lo, hi) for i in range(4)]
                got = plan.cg_update(*g.v, 0.5, begin, end)
                r_new = h[1] - 0.5 * h[3]
                assert got == L.GridDot(float((r_new * r_new).sum()), float((r_new * r_new).sum()), r_new.size, 0), what + ": exact rr"


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def padded_with_interior(L, shape, dims, interior, halo=0.0):
    a = np.full(L.padded_shape(shape, dims), float(halo))
    L.interior(shape, a)[...] = interior
    return a


def cg_by_public_entries(L, plan, w, shape, dims, g, iterations, with_f=True, norm="max"):
    """grids of g: 0 = x, 1 = f; the loop of the header's bit contract.  Returns the true residual record of the result as the
    driver's probe takes it: in one pass under the max norm, by a source sweep and a difference under the RMS norm."""
    import torch

    x, f = g.v[0], g.v[1] if with_f else None
    r, p, q = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    sweep = L.Plan(shape, dims).set_weights(w)
    if with_f:
        sweep.set_source(f)
    sweep.step(x, r)  # fl(S(x) + f)
    torch.cuda.synchronize()
    inner = lambda t: L.interior(shape, t)
    inner(r).copy_(inner(r) - inner(x))
    inner(p).copy_(inner(r))
    rr = plan.dot(r, r).dot
    for _ in range(iterations):
        pq = plan.apply_dot(p, q).dot
        alpha = rr / pq
        rr_new = plan.cg_update(x, r, p, q, alpha).dot
        beta = rr_new / rr
        plan.cg_direction(p, r, beta)
        rr = rr_new
    if norm == "max":
        return plan.residual_src(x, f)
    sweep.step(x, q)
    return plan.diff(q, x)


@pytest.mark.parametrize("shape,dims,regions", SEVERAL, ids=SEVERAL_IDS)
def test_driver_equals_the_composition_of_the_public_entries(L, shape, dims, regions):
    """every combination of the probe's two forms (the max norm: fused; the RMS norm: two passes) with and without f"""
    import torch

    _, x0, f0 = host_data(shape, dims)[:3]
    w = symmetric_taps(L, shape, "normalised")
    plan = make_plan(L, shape, dims, "normalised")
    for norm, with_f in itertools.product(("max", "rms"), (True, False)):
        for off, iterations in zip((16, 240, 16), (2, 4, 6)):
            what = f"{shape} {dims} run_cg_until x{iterations} norm {norm} f {with_f}"
            g = Grids(L, shape, dims, off, [x0, f0])
            before_f, halo = g.bits(1), ~g.region(0, plan.dims[0]).clone()
            before_x = g.bits(0)
            res = plan.run_cg_until(g.v[0], g.v[1] if with_f else None, tol=0.0, norm=norm, check_every=2, max_times=iterations)
            g.guards(what)
            assert torch.equal(g.arena.bits(1), before_f), what + ": d_f was written"
            assert torch.equal(g.arena.bits(0)[halo], before_x[halo]), what + ": a halo cell of d_x was written"
            got_x = g.v[0].clone()
            g.v[0].copy_(torch.from_numpy(np.array(x0)))
            last = cg_by_public_entries(L, plan, w, shape, dims, g, iterations, with_f, norm)
            assert same_bits(got_x, g.v[0]), what + ": x differs from the loop over the public entries"
            assert res.until.times_done == iterations and res.until.checks == iterations // 2 and not res.breakdown
            assert tuple(map(fbits, res.until.last)) == tuple(map(fbits, last)), what
            assert fbits(res.until.residual) == fbits(last.max_abs if norm == "max" else math.sqrt(last.sum_sq / last.count)), what
            assert not res.until.converged and not res.until.diverged
            assert res.lambda_min > 0 and res.lambda_max >= res.lambda_min and res.rho_estimate == max(abs(1 - res.lambda_min), abs(1 - res.lambda_max))


def jacobi(L, dims):
    """1/4 on the four neighbours through set_weights on star2d1r; f = integers in [-8, 8], x = 0 with a non-zero integer halo"""
    w = np.zeros(L.ops.ntaps("star2d1r"))
    assert w.size == 49
    w[[24 - 7, 24 - 1, 24 + 1, 24 + 7]] = 0.25
    rng = np.random.default_rng(zlib.crc32(repr(("jacobi", dims)).encode()))
    f = padded_with_interior(L, "star2d1r", dims, rng.integers(-8, 9, dims).astype(np.float64))
    x = rng.integers(-3, 4, f.shape).astype(np.float64)
    L.interior("star2d1r", x)[...] = 0.0
    rho = (math.cos(math.pi / (dims[0] + 1)) + math.cos(math.pi / (dims[1] + 1))) / 2
    return w, f, x, rho


def dense_problem(L, shape, dims, w, f, x):
    """A = I - S on the interior as a dense matrix and b = f + S(the halo of x): A u = b is u = S(u) + f with x's boundary"""
    nd, side = len(dims), {2: 7, 3: 3}[len(dims)]
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims)
    taps = np.asarray(w).reshape((side,) * nd)
    halo = [(a - b) // 2 for a, b in zip(x.shape, dims)]
    S, b = np.zeros((n, n)), L.interior(shape, f).astype(np.float64).ravel().copy()
    for cell in np.ndindex(*dims):
        for t in zip(*np.nonzero(taps)):
            nb = tuple(c + k - side // 2 for c, k in zip(cell, t))
            if all(0 <= c < d for c, d in zip(nb, dims)):
                S[idx[cell], idx[nb]] += taps[t]
            else:
                b[idx[cell]] += taps[t] * x[tuple(c + h for c, h in zip(nb, halo))]
    return np.eye(n) - S, b


def numpy_cg_iterations(A, b, tol):
    x, r = np.zeros_like(b), b.copy()
    p, rr, k = r.copy(), r @ r, 0
    while np.abs(r).max() > tol and k < 10 * b.size:
        q = A @ p
        alpha = rr / (p @ q)
        x += alpha * p
        r -= alpha * q
        rr, old = r @ r, rr
        p = r + (rr / old) * p
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def solved(dims):
    """one run of the driver per Jacobi grid, shared by the tests below"""
    import lorastencil_amd as L
    import torch

    w, f, x, rho = jacobi(L, dims)
    A, b = dense_problem(L, "star2d1r", dims, w, f, x)
    tol = 1e-9
    need = numpy_cg_iterations(A, b, 1e-12)
    plan = L.Plan("star2d1r", dims).set_weights(w)
    g = Grids(L, "star2d1r", dims, 240, [x, f])
    res = plan.run_cg_until(g.v[0], g.v[1], tol=tol, norm="max", check_every=2, max_times=2 * need)
    g.guards(f"jacobi {dims}")
    print("jacobi", dims, "numpy CG to 1e-12:", need, "iterations; the driver:", res)
    return plan, g, res, A, b, rho, tol, x


@pytest.mark.parametrize("dims", [(6, 10), (33, 34)])
def test_it_solves_the_jacobi_problem(L, dims):
    plan, g, res, A, b, rho, tol, x0 = solved(dims)
    assert res.until.converged and not res.until.diverged and not res.breakdown
    assert plan.residual_src(g.v[0], g.v[1]).max_abs <= tol
    got = g.v[0].cpu().numpy()
    halo = np.ones(got.shape, dtype=bool)
    L.interior("star2d1r", halo)[...] = False
    assert np.array_equal(got[halo], x0[halo])
    if dims == (6, 10):
        err = np.abs(L.interior("star2d1r", got).ravel() - np.linalg.solve(A, b)).max()
        print("error against numpy.linalg.solve:", err, "bound", 2 * math.sqrt(60) * tol / (1 - rho))
        assert err <= 2 * math.sqrt(60) * tol / (1 - rho)


@pytest.mark.parametrize("dims", [(6, 10), (33, 34)])
def test_rho_estimate_against_the_closed_form(L, dims):
    _, _, res, _, _, rho, _, _ = solved(dims)
    print("rho", rho, "estimate", res.rho_estimate, "difference", res.rho_estimate - rho, "lambda", res.lambda_min, res.lambda_max)
    assert rho - 1e-8 <= res.rho_estimate <= rho + 1e-12
    # Ritz values lie inside the spectrum [1 - rho, 1 + rho]
    assert 1 - rho - 1e-12 <= res.lambda_min <= res.lambda_max <= 1 + rho + 1e-12


def test_it_solves_a_3d_box_problem(L):
    shape, dims, tol = "box3d1r", (4, 4, 8), 1e-9
    w = symmetric_taps(L, shape, "normalised")
    w[13] = 0.0  # without the centre tap rho(S) < 1 - w_centre: A = I - S is positive definite with room
    rng = np.random.default_rng(11)
    f = padded_with_interior(L, shape, dims, rng.integers(-8, 9, dims).astype(np.float64))
    x = rng.integers(-3, 4, f.shape).astype(np.float64)
    L.interior(shape, x)[...] = 0.0
    A, b = dense_problem(L, shape, dims, w, f, x)
    need = numpy_cg_iterations(A, b, 1e-12)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 16, [x, f])
    res = plan.run_cg_until(g.v[0], g.v[1], tol=tol, check_every=2, max_times=2 * need)
    g.guards("box3d1r (4, 4, 8)")
    print("box3d1r", dims, "numpy CG:", need, "the driver:", res)
    assert res.until.converged and plan.residual_src(g.v[0], g.v[1]).max_abs <= tol
    err = np.abs(L.interior(shape, g.v[0]).cpu().numpy().ravel() - np.linalg.solve(A, b)).max()
    rho = np.abs(np.linalg.eigvalsh(np.eye(len(b)) - A)).max()
    assert err <= 2 * math.sqrt(len(b)) * tol / (1 - rho)
    assert res.rho_estimate <= rho + 1e-12


def test_breakdown_is_a_numeric_outcome(L):
    import torch

    dims = (6, 10)
    _, f, x, _ = jacobi(L, dims)
    # centre 2 and nothing else: S = 2 I, A = -I is not positive definite -- p.q < 0 at the first application
    w = np.zeros(49)
    w[24] = 2.0
    plan = L.Plan("star2d1r", dims).set_weights(w)
    x = x + padded_with_interior(L, "star2d1r", dims, 1.0)
    g = Grids(L, "star2d1r", dims, 16, [x, f])
    before = g.bits(0)
    res = plan.run_cg_until(g.v[0], g.v[1], tol=1e-9, check_every=2, max_times=8)
    g.guards("A = -I")
    print("A = -I:", res)
    assert res.until.diverged and res.breakdown and not res.until.converged
    assert res.until.times_done == 0 and res.until.checks == 1
    assert torch.equal(g.arena.bits(0), before), "x is not the last good iterate"
    assert math.isnan(res.rho_estimate) and math.isnan(res.lambda_min) and math.isnan(res.lambda_max)
    # a NaN in an interior cell of f
    w, f, x, _ = jacobi(L, dims)
    f = f.copy()
    L.interior("star2d1r", f)[2, 3] = float("nan")
    plan = L.Plan("star2d1r", dims).set_weights(w)
    g = Grids(L, "star2d1r", dims, 16, [x, f])
    res = plan.run_cg_until(g.v[0], g.v[1], tol=1e-9, check_every=2, max_times=8)
    g.guards("NaN in f")
    print("NaN in f:", res)
    assert res.until.diverged and not res.until.converged and res.until.last.nonfinite > 0
    # the same plan solves the clean problem afterwards: the flag does not outlive its run
    clean = solved(dims)
    w, f, x, _ = jacobi(L, dims)
    g = Grids(L, "star2d1r", dims, 240, [x, f])
    res = plan.run_cg_until(g.v[0], g.v[1], tol=1e-9, check_every=2, max_times=200)
    assert res.until.converged and same_bits(g.v[0], clean[1].v[0])


def test_run_host_cg_is_the_plan_driver(L):
    """the shape's own taps divided by their sum (the thread's normalise default): symmetric, non-negative, rho(S) < 1 under a
    zero boundary"""
    import torch

    lib = L._lib.lib()
    shape, dims = "star2d3r", (6, 10)
    _, f, x, _ = jacobi(L, dims)
    old = lib.lora_set_default_normalize(1)
    try:
        out, res, info = L.run_host_cg(shape, x, 1e-9, source=f, check_every=2, max_times=200)
        plan = L.Plan(shape, dims)
    finally:
        lib.lora_set_default_normalize(old)
    dx, df = torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()
    ref = plan.run_cg_until(dx, df, tol=1e-9, check_every=2, max_times=200)
    print("run_host_cg:", res, info.sweep_seconds)
    assert res.until.converged and res == ref and np.array_equal(out.view(np.int64), dx.cpu().numpy().view(np.int64))
    assert info.steps_per_launch == 1 and info.hbm_gbs > 0
    assert info.hbm_gbs == pytest.approx(60 * res.until.times_done * 11 * 8 / info.sweep_seconds / 1e9)
