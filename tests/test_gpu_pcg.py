"""GPU tests of the fused defect kernel, the V-cycle for A = sigma I - tau S as a preconditioner, the PCG driver and the
implicit stepper built on it (kernels_theta.hip: the defect modes; mg.cpp; cg.cpp; the PCG phases of kernels_cg.hip's fold).

Yardsticks, none of them the code under test: ``plan.step_region`` of a plan that carries f followed by one numpy subtraction
for the defect; Python loops over the public entries, the level plans built from the header's formulas, for the bits of the
preconditioner and of the two drivers; a numpy model of the cycle and of PCG written here from the same formulas (its own
coarsening rule and coarse taps), which never calls the engine; ``numpy.linalg.solve`` on dense systems.

Engine against model.  Both are fp64 runs of one algorithm that differ in summation order, so the yardstick for "how far apart
may two such runs be" is the model against itself with its taps summed in the opposite order, with a tenfold margin, computed
in the test and never taken from the engine's output (the scheme of tests/test_gpu_mg.py).

Buffers are carved by tests/arena.py at offsets 16 and 240, the guard bands NaN.
"""
import functools
import itertools
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
PAIRS = [(1.0, 1.0), (9.0, 8.0)]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


# ---- the closed forms of the header, in numpy ------------------------------------------------------------------------------------
def tap_offsets(nd):
    if nd == 1:
        return [(t - 4,) for t in range(9)]
    if nd == 2:
        return [(t // 7 - 3, t % 7 - 3) for t in range(49)]
    return [(t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1) for t in range(27)]


def jacobi_taps(nd):
    offs = tap_offsets(nd)
    w = np.zeros(len(offs))
    for t, d in enumerate(offs):
        if sum(abs(x) for x in d) == 1:
            w[t] = 1.0 / (2 * nd)
    return w


def jacobi_rho(dims):
    return sum(math.cos(math.pi / (n + 1)) for n in dims) / len(dims)


def smoother_pair(w, omega, sigma, tau):
    """(s, c) of the header for A = sigma I - tau S, one numpy operation per rounding"""
    ct = len(w) // 2
    d = sigma - tau * w[ct]
    c = omega / d
    cp = c * tau
    s = cp * w
    s[ct] = s[ct] + (1.0 - c * sigma)
    return s, c


def P_axis(n, nc):
    i = np.arange(n, dtype=np.int64)[:, None] + 1
    j = np.arange(nc, dtype=np.int64)[None, :] + 1
    num = (n + 1) - np.abs(i * (nc + 1) - j * (n + 1))
    return np.maximum(num, 0).astype(np.float64) / np.float64(n + 1)


def apply_axes(mats, x):
    for a, m in enumerate(mats):
        x = np.moveaxis(np.tensordot(m, x, axes=(1, a)), 0, a)
    return x


# ---- grids --------------------------------------------------------------------------------------------------------------------
class Grids:
    """n grids of one padded shape carved from one poisoned allocation; grid i starts as values[i] or stays NaN (None)"""

    def __init__(self, L, shape, dims, offset, values):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, tuple(dims)
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

    def interior_mask(self):
        return self.region(0, self.dims[0]).clone()

    def bits(self, i):
        return self.arena.bits(i).clone()

    def guards(self, what):
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)

    def host(self, i):
        return self.L.interior(self.shape, self.v[i]).cpu().numpy().copy()


def padded(L, shape, dims, interior, halo):
    a = np.array(halo, dtype=np.float64) if isinstance(halo, np.ndarray) else np.full(L.padded_shape(shape, dims), float(halo))
    L.interior(shape, a)[...] = interior
    return a


def same_bits(a, b):
    import torch

    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def symmetric_random_taps(L, shape, rng, total=0.9):
    """every tap of the shape's support, point-symmetric, positive, the sum `total`"""
    support = L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0
    w = np.where(support, rng.uniform(0.2, 1.0, support.size), 0.0)
    w = (w + w[::-1]) / 2
    return w * (total / w.sum())


# ---- 1. the defect kernel --------------------------------------------------------------------------------------------------------
DEFECT_CASES = [
    ("1d1r", (37,), (2, 36)),                # the odd tail point; a sub-range that begins on an even point
    ("star2d1r", (16, 20), (3, 11)),
    ("box2d3r", (70, 260), (33, 70)),        # more than one 128-column tile with a partial one, two row tiles
    ("star3d1r", (8, 8, 8), (1, 7)),
    ("box3d1r", (35, 17, 130), (1, 34)),     # two plane tiles, two row tiles, two column tiles
]
DEFECT_IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d, _ in DEFECT_CASES]
DEFECT_EDGES = [  # the edges of the shared walk (csrc/tile_walk.h), as in tests/test_gpu_residual.py
    ("1d2r", (1027,), (510, 1027)),          # two full tiles and one of three points: the odd tail point in the last piece
    ("star2d1r", (33, 130), (1, 33)),        # one row and one column pair in second tiles
    ("star2d3r", (33, 130), (1, 33)),
    ("box2d3r", (33, 130), (1, 33)),
    ("star2d1r", (70, 258), (5, 37)),        # a region that begins and ends inside a tile
    ("star2d3r", (70, 258), (5, 37)),
    ("box2d3r", (70, 258), (5, 37)),
] + [(s, (34, 18, 130), (3, 3 + k)) for s in ("box3d1r", "star3d1r") for k in (1, 2, 3)]  # the plane ring ends in each of its phases
DEFECT_IDS += [f"{s}-{'x'.join(map(str, d))}-{b}-{e}" for s, d, (b, e) in DEFECT_EDGES]
DEFECT_CASES += DEFECT_EDGES


@pytest.mark.parametrize("shape,dims,sub", DEFECT_CASES, ids=DEFECT_IDS)
def test_defect_is_a_source_sweep_and_one_subtraction(L, shape, dims, sub):
    """grids: 0 = u (values in its halo: the stencil reads it), 1 = f with a NaN halo, 2 = out, NaN everywhere before each
    call.  The yardstick sweeps with a clean copy of f as a plan's source."""
    import torch

    rng = np.random.default_rng(zlib.crc32(repr(("defect", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    w = rng.uniform(-1.0, 1.0, L.ops.ntaps(shape)) * (L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0)
    u0, f0 = rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 3.0
    p = L.Plan(shape, dims).set_weights(w)
    assert p.get_option("cg") == 1
    f_clean = torch.from_numpy(f0).cuda()
    with_f = L.Plan(shape, dims).set_weights(w).set_source(f_clean)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, [u0, None, None])
        every = g.interior_mask()
        g.v[1][every] = f_clean[every]  # the halo of f stays NaN
        before = (g.bits(0), g.bits(1))
        for begin, end in [(0, 0), sub]:
            lo, hi = (0, dims[0]) if (begin, end) == (0, 0) else (begin, end)
            m = g.region(lo, hi).clone()
            for use_f in (True, False):
                what = f"{shape} {dims} f {use_f} [{begin}, {end}) offset {off}"
                g.arena.fill_poison(2)
                p.defect(g.v[0], g.v[1] if use_f else None, g.v[2], begin, end)
                g.guards(what)
                assert torch.equal(g.arena.bits(0), before[0]) and torch.equal(g.arena.bits(1), before[1]), what + ": u or f changed"
                spare = torch.zeros_like(g.v[0])
                (with_f if use_f else p).step_region(g.v[0], spare, lo, hi)
                torch.cuda.synchronize()
                want = spare[m].cpu().numpy() - g.v[0][m].cpu().numpy()  # one fp64 subtraction
                have = g.v[2][m].cpu().numpy()
                assert np.isfinite(have).all(), what + ": a NaN of a halo reached a result"
                assert np.array_equal(have.view(np.int64), want.view(np.int64)), what + ": out differs from step_region and a subtraction"
                assert bool(g.arena.is_poison(2)[~m].all()), what + ": a cell of out outside the region's interior was written"


def test_defect_takes_a_capturing_stream(L):
    import torch

    shape, dims = "star2d1r", (16, 20)
    rng = np.random.default_rng(3)
    ps = L.padded_shape(shape, dims)
    p = L.Plan(shape, dims).set_weights(jacobi_taps(2))
    u, f = torch.from_numpy(rng.standard_normal(ps)).cuda(), torch.from_numpy(rng.standard_normal(ps)).cuda()
    direct, replayed = torch.zeros_like(u), torch.zeros_like(u)
    p.defect(u, f, direct)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        p.defect(u, f, replayed, stream=s)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(direct, replayed) and float(direct.abs().max()) > 0.0


# ---- 2. the preconditioner, bit for bit ------------------------------------------------------------------------------------------
def level_tables(L, shape, dims, w, omega, sigma, tau):
    """[(dims, w, s, c)] per level from the header's formulas; the coarse taps through the public host entry"""
    out = []
    while True:
        s, c = smoother_pair(w.copy(), omega, sigma, tau)
        out.append((tuple(dims), w, s, c))
        try:
            nxt = L.mg_coarse_dims(shape, dims)
        except L.LoraError:
            break
        w = L.mg_coarse_taps(shape, w, dims, nxt)
        dims = nxt
    return out


class PublicCycle:
    """z = M r as the header's bit contract composes it: level plans built with Plan + set_weights (+ set_boundary + set_source
    for the smoothing sweeps), lora_plan_defect for the level's residual, the transfers, the CG entries with the scalars divided
    in host fp64."""

    def __init__(self, L, shape, dims, w, omega, pre, post, sigma, tau):
        import torch

        self.L, self.shape, self.pre, self.post, self.sigma, self.tau = L, shape, pre, post, sigma, tau
        self.tab = level_tables(L, shape, dims, w, omega, sigma, tau)
        self.last = len(self.tab) - 1
        self.plain, self.smooth, self.bare, self.x, self.spare, self.g = [], [], [], [], [], []
        for l, (d, wl, sl, cl) in enumerate(self.tab):
            z = lambda: torch.zeros(L.padded_shape(shape, d), dtype=torch.float64, device="cuda")
            self.plain.append(L.Plan(shape, d).set_weights(wl))
            self.x.append(z())
            self.spare.append(z())
            self.g.append(z())
            if l < self.last:
                self.smooth.append(L.Plan(shape, d).set_weights(sl).set_boundary("dirichlet").set_source(self.g[l]))
                self.bare.append(L.Plan(shape, d).set_weights(sl))
        self.iters = min(64, int(np.prod(self.tab[-1][0])))
        self.p, self.q = torch.zeros_like(self.x[-1]), torch.zeros_like(self.x[-1])

    def inner(self, t):
        return self.L.interior(self.shape, t)

    def cycle(self, l, cur, other):
        if l == self.last:
            plan, x, r, p, q = self.plain[l], cur, self.g[l], self.p, self.q
            p.zero_()
            self.inner(p).copy_(self.inner(r))
            rr = plan.dot(r, r).dot
            for _ in range(self.iters):
                if (self.sigma, self.tau) == (1.0, 1.0):
                    pq = plan.apply_dot(p, q).dot
                else:
                    pq = plan.apply_dot_shift(p, q, self.sigma, self.tau).dot
                if not (math.isfinite(pq) and pq > 0.0 and math.isfinite(rr)):
                    break  # the sticky halt: the residual vanished exactly
                rr_new = plan.cg_update(x, r, p, q, rr / pq).dot
                beta = rr_new / rr
                rr = rr_new
                if not math.isfinite(rr_new):
                    break
                plan.cg_direction(p, r, beta)
            return cur
        sm, c = self.smooth[l], self.tab[l][3]
        if self.pre:
            sm.run(cur, other, self.pre)
            if self.pre % 2:
                cur, other = other, cur
        self.bare[l].defect(cur, self.g[l], other)
        nxt_c = self.tab[l + 1][3]
        scale = 1.0 / c if l + 1 == self.last else nxt_c / c
        self.plain[l].mg_restrict(other, self.g[l + 1], scale)
        self.x[l + 1].zero_()
        coarse = self.cycle(l + 1, self.x[l + 1], self.spare[l + 1])
        self.plain[l].mg_prolong_add(coarse, cur)
        if self.post:
            sm.run(cur, other, self.post)
            if self.post % 2:
                cur, other = other, cur
        return cur

    def apply(self, r):
        """M r for a padded device grid r (only its interior is read); the result's interior as a device tensor"""
        import torch

        self.g[0].zero_()
        self.inner(self.g[0]).copy_(self.inner(r) * self.tab[0][3])  # g_0 = fl(c_0 r): one multiplication
        self.x[0].zero_()
        self.spare[0].zero_()
        out = self.cycle(0, self.x[0], self.spare[0])
        torch.cuda.synchronize()
        return self.inner(out)


def cycle_taps(L, shape, rng):
    return jacobi_taps(2) if shape == "star2d1r" else symmetric_random_taps(L, shape, rng)


@pytest.mark.parametrize("shape,dims,levels", [("star2d1r", (16, 20), 3), ("box3d1r", (8, 8, 16), 2)])
@pytest.mark.parametrize("sigma,tau", PAIRS, ids=["1-1", "9-8"])
def test_preconditioner_equals_the_composition_of_the_public_entries(L, shape, dims, levels, sigma, tau):
    import torch

    rng = np.random.default_rng(zlib.crc32(repr(("precondition", shape, dims)).encode()))
    w = cycle_taps(L, shape, rng)
    ps = L.padded_shape(shape, dims)
    r0 = rng.standard_normal(ps)
    plan = L.Plan(shape, dims).set_weights(w)
    for off, smooth in zip(OFFSETS, (1, 2)):
        ref = PublicCycle(L, shape, dims, w, 0.8, smooth, smooth, sigma, tau)
        assert len(ref.tab) == levels
        g = Grids(L, shape, dims, off, [None, None])  # r: its halo stays NaN; z: NaN everywhere
        every = g.interior_mask()
        g.v[0][every] = torch.from_numpy(r0).cuda()[every]
        before_r = g.bits(0)
        plan.mg_precondition(g.v[0], g.v[1], sigma, tau, pre=smooth, post=smooth, omega=0.8)
        what = f"{shape} {dims} ({sigma}, {tau}) V({smooth},{smooth})"
        g.guards(what)
        assert torch.equal(g.arena.bits(0), before_r), what + ": d_r was written"
        assert bool((g.v[1][~every] == 0.0).all()), what + ": the halo of d_z is not the zero halo of a correction"
        expect = ref.apply(g.v[0])
        assert same_bits(L.interior(shape, g.v[1]), expect), what + ": d_z differs from the composition of the public entries"
        assert float(expect.abs().max()) > 0.0
        launches, nbytes = plan.mg_cycle_cost()
        print(what, "launches", launches, "bytes", nbytes)
        assert launches > 5 * ref.iters and nbytes > 0


# ---- 3. the model ---------------------------------------------------------------------------------------------------------------
def model_coarse_dims(dims):
    c = [n // 2 for n in dims]
    c[-1] &= ~1
    return None if len(dims) < 2 or min(c) < 4 else tuple(c)


def model_coarse_taps(w, dims, cdims):
    nd = len(dims)
    offs = tap_offsets(nd)
    ct = len(offs) // 2
    q = [((cdims[a] + 1) / (dims[a] + 1)) ** 2 for a in range(nd)]
    wc = np.zeros_like(w)
    for t, d in enumerate(offs):
        if t != ct:
            l2 = float(sum(x * x for x in d))
            wc[t] = w[t] * np.prod([q[a] ** (d[a] * d[a] / l2) for a in range(nd)])
    wc[ct] = w.sum() - np.delete(wc, ct).sum()
    return wc


def model_sweep(w, x, order=1):
    """S(x) of an interior array with a zero halo, the taps summed in ascending (1) or descending (-1) order"""
    offs = tap_offsets(x.ndim)
    r = 3 if x.ndim == 2 else 1
    xp = np.pad(x, r)
    acc = np.zeros_like(x)
    for t in (range(len(offs)) if order > 0 else range(len(offs) - 1, -1, -1)):
        if w[t] != 0.0:
            acc = acc + w[t] * xp[tuple(slice(r + d, r + d + n) for d, n in zip(offs[t], x.shape))]
    return acc


class Model:
    """M of the header in numpy on interior arrays with a zero halo: the V-cycle for sigma I - tau S, the coarsest level the
    engine's fixed count of CG iterations from zero (halting like the engine when the residual vanishes)."""

    def __init__(self, w, dims, omega, smooth, order, sigma=1.0, tau=1.0):
        self.smooth, self.order, self.sigma, self.tau, self.lv = smooth, order, sigma, tau, []
        dims = tuple(dims)
        while True:
            s, c = smoother_pair(w.copy(), omega, sigma, tau)
            self.lv.append(dict(dims=dims, w=w, s=s, c=c))
            nxt = model_coarse_dims(dims)
            if nxt is None:
                break
            self.lv[-1]["P"] = [P_axis(n, nc) for n, nc in zip(dims, nxt)]
            self.lv[-1]["rho"] = float(np.prod([(nc + 1) / (n + 1) for n, nc in zip(dims, nxt)]))
            w, dims = model_coarse_taps(w, dims, nxt), nxt
        self.iters = min(64, int(np.prod(self.lv[-1]["dims"])))

    def A(self, l, x):
        return self.sigma * x - self.tau * model_sweep(self.lv[l]["w"], x, self.order)

    def coarsest(self, b):
        l = len(self.lv) - 1
        x, r = np.zeros_like(b), b.copy()
        p, rr = r.copy(), float((r * r).sum())
        for _ in range(self.iters):
            q = self.A(l, p)
            pq = float((p * q).sum())
            if not (math.isfinite(pq) and pq > 0.0 and math.isfinite(rr)):
                break
            alpha = rr / pq
            x, r = x + alpha * p, r - alpha * q
            rr_new = float((r * r).sum())
            p, rr = r + (rr_new / rr) * p, rr_new
        return x

    def cycle(self, l, x, g):
        lv = self.lv[l]
        if l == len(self.lv) - 1:
            return self.coarsest(g)
        for _ in range(self.smooth):
            x = model_sweep(lv["s"], x, self.order) + g
        rs = (model_sweep(lv["s"], x, self.order) + g) - x
        nxt = self.lv[l + 1]
        scale = 1.0 / lv["c"] if l + 2 == len(self.lv) else nxt["c"] / lv["c"]
        gc = scale * lv["rho"] * apply_axes([p.T for p in lv["P"]], rs)
        x = x + apply_axes(lv["P"], self.cycle(l + 1, np.zeros(nxt["dims"]), gc))
        for _ in range(self.smooth):
            x = model_sweep(lv["s"], x, self.order) + g
        return x

    def M(self, r):
        return self.cycle(0, np.zeros_like(r), self.lv[0]["c"] * r)

    def pcg_residuals(self, f, tol, check_every, cap=60):
        """PCG for u = S(u) + f from u = 0 (sigma = tau = 1): max |S(u) + f - u| after every round until it is <= tol"""
        w = self.lv[0]["w"]
        x, r = np.zeros_like(f), f.copy()
        z = self.M(r)
        p, rz, out = z.copy(), float((r * z).sum()), []
        while len(out) * check_every < cap:
            for _ in range(check_every):
                q = self.A(0, p)
                alpha = rz / float((p * q).sum())
                x, r = x + alpha * p, r - alpha * q
                z = self.M(r)
                rz_new = float((r * z).sum())
                p, rz = z + (rz_new / rz) * p, rz_new
            out.append(np.abs((model_sweep(w, x) + f) - x).max())
            if out[-1] <= tol:
                break
        return out


@pytest.mark.parametrize("shape,dims", [("star2d1r", (16, 16)), ("star3d1r", (8, 8, 8))])
@pytest.mark.parametrize("sigma,tau", PAIRS, ids=["1-1", "9-8"])
def test_the_preconditioner_is_the_models_and_symmetric(L, shape, dims, sigma, tau):
    import torch

    nd = len(dims)
    w = jacobi_taps(nd)
    rng = np.random.default_rng(zlib.crc32(repr(("model", dims)).encode()))
    x, y = rng.standard_normal(dims), rng.standard_normal(dims)
    models = [Model(w, dims, 0.8, 2, order, sigma, tau) for order in (1, -1)]
    zs = [[m.M(v) for v in (x, y)] for m in models]
    deviation = max(np.abs(a - b).max() / np.abs(a).max() for a, b in zip(zs[0], zs[1]))
    allow = 10.0 * deviation
    print(shape, dims, (sigma, tau), "the model's two tap orders differ by", deviation, "(relative, max norm) -> allowance", allow)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 16, [padded(L, shape, dims, x, np.nan), None, padded(L, shape, dims, y, np.nan), None])
    plan.mg_precondition(g.v[0], g.v[1], sigma, tau)
    plan.mg_precondition(g.v[2], g.v[3], sigma, tau)
    g.guards(f"{shape} {dims} model")
    Mx, My = g.host(1), g.host(3)
    for have, want, name in ((Mx, zs[0][0], "x"), (My, zs[0][1], "y")):
        err = np.abs(have - want).max() / np.abs(want).max()
        print("  M", name, "engine against model:", err)
        assert err <= allow, f"M {name} is {err} from the model's, allowed {allow}"
    asym = abs(float((x * My).sum()) - float((Mx * y).sum()))
    scale = float(np.sqrt((x * x).sum()) * np.sqrt((My * My).sum()))
    print("  |<x, M y> - <M x, y>| =", asym, "allowed", allow * scale)
    assert asym <= allow * scale


# ---- 4. the PCG driver ------------------------------------------------------------------------------------------------------------
def pcg_by_public_entries(L, plan, shape, x, f, iters, smooth):
    """the loop of the header's bit contract on the device grid x (in place); alpha and beta divided in host fp64"""
    import torch

    r, z, p, q = (torch.zeros_like(x) for _ in range(4))
    inner = lambda t: L.interior(shape, t)
    plan.defect(x, f, r)
    plan.mg_precondition(r, z, pre=smooth, post=smooth)
    inner(p).copy_(inner(z))
    rz = plan.dot(r, z).dot
    for _ in range(iters):
        pq = plan.apply_dot(p, q).dot
        plan.cg_update(x, r, p, q, rz / pq)
        plan.mg_precondition(r, z, pre=smooth, post=smooth)
        rz_new = plan.dot(r, z).dot
        plan.cg_direction(p, z, rz_new / rz)
        rz = rz_new
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,dims", [("star2d1r", (16, 20)), ("box3d1r", (8, 8, 16))])
@pytest.mark.parametrize("with_f", [True, False], ids=["f", "nof"])
def test_pcg_driver_equals_the_host_loop(L, shape, dims, with_f):
    import torch

    rng = np.random.default_rng(zlib.crc32(repr(("pcg", shape, dims)).encode()))
    w = cycle_taps(L, shape, rng)
    ps = L.padded_shape(shape, dims)
    x0 = rng.standard_normal(ps)  # non-zero halo values: the boundary
    f0 = rng.standard_normal(ps) if with_f else None
    plan = L.Plan(shape, dims).set_weights(w)
    # both forms of the probe: fused under the max norm, a source sweep and a difference under the RMS norm
    for (off, smooth), norm in itertools.product(zip(OFFSETS, (1, 2)), ("max", "rms")):
        g = Grids(L, shape, dims, off, [x0, f0])
        halo = ~g.interior_mask()
        before_x, before_f = g.bits(0), g.bits(1)
        f = g.v[1] if with_f else None
        res = plan.run_pcg_until(g.v[0], f, tol=0.0, smooth=smooth, norm=norm, check_every=2, max_times=4)
        what = f"{shape} {dims} V({smooth},{smooth}) f {with_f} norm {norm}"
        g.guards(what)
        assert torch.equal(g.arena.bits(1), before_f), what + ": d_f was written"
        assert torch.equal(g.arena.bits(0)[halo], before_x[halo]), what + ": a halo cell of d_x was written"
        print(what, res)
        assert res.until.times_done == 4 and res.until.checks == 2 and not res.breakdown and not res.until.diverged
        assert res.levels == len(level_tables(L, shape, dims, w, 0.8, 1.0, 1.0))
        assert 0.0 < res.lambda_min <= res.lambda_max < 2.0  # M A of a convergent stationary method has its spectrum in (0, 2)
        expect = torch.from_numpy(x0).cuda()
        pcg_by_public_entries(L, L.Plan(shape, dims).set_weights(w), shape, expect, f, 4, smooth)
        assert same_bits(g.v[0], expect), what + ": d_x after 4 iterations differs from the host loop over the public entries"
        last = plan.residual_src(g.v[0], f)
        if norm == "rms":
            sweep, q = L.Plan(shape, dims).set_weights(w), torch.zeros_like(g.v[0])
            if with_f:
                sweep.set_source(f)
            sweep.step(g.v[0], q)
            two_pass = plan.diff(q, g.v[0])
            assert res.until.last == two_pass and res.until.residual == math.sqrt(two_pass.sum_sq / two_pass.count), what
        else:
            assert res.until.last == last, what
        assert res.until.last.max_abs == last.max_abs and (norm == "rms" or res.until.residual == last.max_abs)


def dense_operator(L, shape, dims, w, x):
    """S on the interior as a dense matrix and S(the halo of x) as a vector"""
    nd, side = len(dims), {2: 7, 3: 3}[len(dims)]
    n = int(np.prod(dims))
    idx = np.arange(n).reshape(dims)
    taps = np.asarray(w).reshape((side,) * nd)
    halo = [(a - b) // 2 for a, b in zip(x.shape, dims)]
    S, b = np.zeros((n, n)), np.zeros(n)
    for cell in np.ndindex(*dims):
        for t in zip(*np.nonzero(taps)):
            nb = tuple(c + k - side // 2 for c, k in zip(cell, t))
            if all(0 <= c < d for c, d in zip(nb, dims)):
                S[idx[cell], idx[nb]] += taps[t]
            else:
                b[idx[cell]] += taps[t] * x[tuple(c + h for c, h in zip(nb, halo))]
    return S, b


@pytest.mark.parametrize("shape,dims", [("star2d1r", (16, 16)), ("star3d1r", (8, 8, 8))])
def test_pcg_solves_the_jacobi_problem(L, shape, dims):
    """the problem and the bound of tests/test_gpu_mg.py's test_it_solves_the_jacobi_problem"""
    import torch

    w = jacobi_taps(len(dims))
    rng = np.random.default_rng(zlib.crc32(repr(("solve", dims)).encode()))
    ps = L.padded_shape(shape, dims)
    f = padded(L, shape, dims, rng.standard_normal(dims), 0.0)
    x = padded(L, shape, dims, np.zeros(dims), rng.standard_normal(ps))  # zero start, non-zero boundary values
    S, b = dense_operator(L, shape, dims, w, x)
    n = S.shape[0]
    tol = 1e-12 * np.abs(f).max()
    rho = jacobi_rho(dims)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 240, [x, f])
    before_x, halo = g.bits(0), ~g.interior_mask()
    res = plan.run_pcg_until(g.v[0], g.v[1], tol=tol, check_every=2, max_times=40)
    g.guards(f"{shape} {dims} solve")
    assert torch.equal(g.arena.bits(0)[halo], before_x[halo]), "a halo cell of d_x was written"
    err = np.abs(g.host(0).ravel() - np.linalg.solve(np.eye(n) - S, L.interior(shape, f).ravel() + b)).max()
    print(shape, dims, res, "error against numpy.linalg.solve:", err, "bound", tol / (1 - rho))
    assert res.until.converged and not res.until.diverged and res.until.residual <= tol
    assert plan.residual_src(g.v[0], g.v[1]).max_abs <= tol
    assert err <= tol / (1 - rho)


@functools.lru_cache(maxsize=None)
def independence(n):
    """the model in both tap orders and the engine on the n x n Jacobi problem: zero start, random f, max norm, rounds of 2"""
    import lorastencil_amd as L

    shape, dims = "star2d1r", (n, n)
    w = jacobi_taps(2)
    f = np.random.default_rng(5).standard_normal(dims)
    tol = 1e-8 * np.abs(f).max()
    model = [Model(w, dims, 0.8, 2, order).pcg_residuals(f, tol, 2) for order in (1, -1)]
    plan = L.Plan(shape, dims).set_weights(w)
    zero, fp = padded(L, shape, dims, np.zeros(dims), 0.0), padded(L, shape, dims, f, 0.0)
    rounds = []
    for k in (1, 2, 3):  # a restart would lose the directions: each prefix is a run of its own from the zero start
        g = Grids(L, shape, dims, 16, [zero, fp])
        rounds.append(plan.run_pcg_until(g.v[0], g.v[1], tol=0.0, check_every=2, max_times=2 * k).until.residual)
    g = Grids(L, shape, dims, 16, [zero, fp])
    full = plan.run_pcg_until(g.v[0], g.v[1], tol=tol, check_every=2, max_times=60)
    g.guards(f"grid independence {dims}")
    return model, rounds, full


def test_pcg_iterations_do_not_grow_with_the_grid(L):
    counts, deviation = {}, 0.0
    for n in (64, 256):
        model, rounds, full = independence(n)
        assert full.until.converged, full
        counts[n] = (2 * len(model[0]), full.until.times_done)
        deviation = max([deviation] + [max(a / b, b / a) - 1.0 for a, b in zip(model[0][:3], model[1][:3])])
        print(n, "iterations under the max-norm rule, rounds of 2: model", counts[n][0], "engine", counts[n][1], "lambda(M A) in",
              (full.lambda_min, full.lambda_max))
        print("  model ", " ".join(f"{r:.3e}" for r in model[0]))
        print("  engine", " ".join(f"{r:.3e}" for r in rounds), "... final", f"{full.until.residual:.3e}")
    print("(a CPU prototype of the design under a 2-norm stop, |r|_2 <= 1e-8 |r0|_2, counted 8 and 8; under this test's max-norm rule:", counts, ")")
    factor = 1.0 + 10.0 * deviation
    print("the model's two tap orders differ by a factor of", 1.0 + deviation, "-> allowed factor", factor)
    for n in (64, 256):
        model, rounds, _ = independence(n)
        assert abs(counts[n][1] - counts[n][0]) <= 2, f"{n}: the engine needs {counts[n][1]} iterations, the model {counts[n][0]}"
        ratios = [max(a / b, b / a) for a, b in zip(rounds, model[0][:3])]
        print(n, "engine / model over the first three rounds:", " ".join(f"{r - 1:.2e}" for r in ratios))
        assert len(ratios) == 3 and all(r <= factor for r in ratios), f"{n}: a residual of the first three rounds is a factor {max(ratios)} from the model's"
    assert abs(counts[64][1] - counts[256][1]) <= 2, f"iterations grow with the grid: {counts}"


def small_problem(L, seed=1):
    shape, dims = "star2d1r", (16, 16)
    rng = np.random.default_rng(seed)
    ps = L.padded_shape(shape, dims)
    f = padded(L, shape, dims, rng.standard_normal(dims), 0.0)
    x = padded(L, shape, dims, np.zeros(dims), rng.standard_normal(ps))
    return shape, dims, jacobi_taps(2), x, f


def test_nan_in_the_source_is_reported_as_divergence(L):
    import torch

    shape, dims, w, x, f = small_problem(L)
    f = f.copy()
    L.interior(shape, f)[5, 7] = np.nan
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 240, [x, f])
    before_x, before_f = g.bits(0), g.bits(1)
    res = plan.run_pcg_until(g.v[0], g.v[1], tol=1e-9, check_every=2, max_times=6)
    g.guards("NaN in f")
    print(res)
    assert res.until.diverged and not res.until.converged and res.breakdown and res.until.checks == 1
    # every launch that could move x exited: d_x is the start iterate
    assert torch.equal(g.arena.bits(0), before_x) and torch.equal(g.arena.bits(1), before_f)


def test_fewer_times_than_a_round_touches_nothing(L):
    import torch

    shape, dims, w, x, f = small_problem(L)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 16, [x, f])
    before = (g.bits(0), g.bits(1))
    res = plan.run_pcg_until(g.v[0], g.v[1], tol=1e-9, check_every=4, max_times=3)
    g.guards("max_times < check_every")
    assert res.until.times_done == 0 and res.until.checks == 0 and math.isnan(res.lambda_min) and res.levels == 3
    assert torch.equal(g.arena.bits(0), before[0]) and torch.equal(g.arena.bits(1), before[1])


def test_a_run_on_a_busy_devices_other_stream_gives_the_same_bits(L):
    import torch

    shape, dims, w, x, f = small_problem(L)
    plan = L.Plan(shape, dims).set_weights(w)
    g0 = Grids(L, shape, dims, 16, [x, f])
    plan.run_pcg_until(g0.v[0], g0.v[1], tol=0.0, check_every=2, max_times=4)  # torch's current stream: the null stream
    torch.cuda.synchronize()
    g1 = Grids(L, shape, dims, 16, [x, f])
    mine, busy = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(20):
            a = (a @ a).clamp_(-1.0, 1.0)
    res = L.Plan(shape, dims).set_weights(w).run_pcg_until(g1.v[0], g1.v[1], tol=0.0, check_every=2, max_times=4, stream=mine)
    g1.guards("run on a non-blocking stream")
    assert res.until.times_done == 4
    assert same_bits(g0.v[0], g1.v[0])


# ---- 5. the implicit stepper on it ----------------------------------------------------------------------------------------------
def theta_mg_by_public_entries(L, plan, shape, u, f, theta, tau, steps, max_iters, rtol, smooth):
    """the loop of the header's bit contract on the device grid u (in place); returns the iterations of every step"""
    import torch

    r, z, p, q = (torch.zeros_like(u) for _ in range(4))
    inner = lambda t: L.interior(shape, t)
    tt = theta * tau
    sigma, rtol2 = 1.0 + tt, rtol * rtol
    M = lambda: plan.mg_precondition(r, z, sigma, tt, pre=smooth, post=smooth)
    counts = []
    for _ in range(steps):
        rr = plan.theta_start(u, f, tau, r, z).dot
        thresh, k = rtol2 * rr, 0
        M()
        inner(p).copy_(inner(z))
        rz = plan.dot(r, z).dot
        while rr != 0.0:
            pq = plan.apply_dot_shift(p, q, sigma, tt).dot
            rr = plan.cg_update(u, r, p, q, rz / pq).dot
            k += 1
            if rr <= thresh or k == max_iters:
                break
            M()
            rz_new = plan.dot(r, z).dot
            plan.cg_direction(p, z, rz_new / rz)
            rz = rz_new
        counts.append(k)
    torch.cuda.synchronize()
    return counts


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("check_every", [1, 3])
def test_stepper_equals_the_host_loop(L, theta, check_every):
    import torch

    shape, dims, tau, steps = "star2d1r", (16, 20), 8.0, 2
    rng = np.random.default_rng(zlib.crc32(repr(("theta_mg", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    w = jacobi_taps(2)
    u0, f0 = rng.standard_normal(ps), rng.standard_normal(ps)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 16 if check_every == 1 else 240, [u0, f0])
    halo = ~g.interior_mask()
    before_u, before_f = g.bits(0), g.bits(1)
    res = plan.run_theta_mg(g.v[0], g.v[1], tau, steps, theta=theta, max_iters=30, rtol=1e-6, smooth=2, check_every=check_every)
    what = f"theta {theta} check_every {check_every}"
    g.guards(what)
    assert torch.equal(g.arena.bits(1), before_f), what + ": d_f was written"
    assert torch.equal(g.arena.bits(0)[halo], before_u[halo]), what + ": a halo cell of d_u was written"
    expect = torch.from_numpy(u0).cuda()
    counts = theta_mg_by_public_entries(L, L.Plan(shape, dims).set_weights(w), shape, expect, g.v[1], theta, tau, steps, 30, 1e-6, 2)
    print(what, res, "host loop:", counts)
    assert list(res.iterations) == counts and res.steps_done == steps and not res.breakdown and res.unconverged_steps == 0
    assert res.iterations_total == sum(counts) and res.iterations_max == max(counts) and 1 <= min(counts) and max(counts) < 30
    assert same_bits(g.v[0], expect), what + ": d_u differs from the host loop over the public entries"
    steady = plan.residual_src(g.v[0], g.v[1])
    assert res.steady.max_abs == steady.max_abs and res.steady.argmax == steady.argmax


@pytest.mark.parametrize("shape,dims", [("star2d1r", (16, 16)), ("star3d1r", (8, 8, 8))])
def test_each_step_is_the_dense_solve(L, shape, dims):
    """Backward Euler with normalised taps: A = sigma I - tau S has lambda_min(A) >= sigma - tau = 1 because the taps sum to 1,
    so |e|_inf <= |e|_2 <= |r|_2 / lambda_min <= rtol |r0|_2 for the recursive residual; the factor 2 covers the recursive against
    the true residual."""
    import torch

    w = jacobi_taps(len(dims))
    rng = np.random.default_rng(zlib.crc32(repr(("theta dense", dims)).encode()))
    ps = L.padded_shape(shape, dims)
    u0, f = rng.standard_normal(ps), padded(L, shape, dims, rng.standard_normal(dims), 0.0)
    S, halo_part = dense_operator(L, shape, dims, w, u0)
    n, rtol, most = S.shape[0], 1e-10, {}
    fi = L.interior(shape, f).ravel()
    plan = L.Plan(shape, dims).set_weights(w)
    for tau in (64.0, 4096.0):
        g = Grids(L, shape, dims, 16, [u0, f])
        most[tau] = 0
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
            most[tau] = max(most[tau], res.iterations_max)
        g.guards(f"{shape} {dims} tau {tau}")
        gc = Grids(L, shape, dims, 16, [u0, f])
        cg = plan.run_theta(gc.v[0], gc.v[1], tau, 2, theta=1.0, max_iters=400, rtol=rtol)
        print("   the CG stepper's iterations for the same two steps:", cg.iterations, "unconverged", cg.unconverged_steps)
    assert most[4096.0] <= most[64.0] + 2, most


def test_no_steps_touches_nothing_and_too_few_iterations_are_counted(L):
    import torch

    shape, dims, w, x, f = small_problem(L)
    plan = L.Plan(shape, dims).set_weights(w)
    g = Grids(L, shape, dims, 240, [x, f])
    before = (g.bits(0), g.bits(1))
    res = plan.run_theta_mg(g.v[0], g.v[1], 64.0, 0)
    g.guards("steps == 0")
    assert res.steps_done == 0 and res.iterations == () and math.isnan(res.last_rr0)
    assert torch.equal(g.arena.bits(0), before[0]) and torch.equal(g.arena.bits(1), before[1])
    res = plan.run_theta_mg(g.v[0], g.v[1], 64.0, 2, max_iters=2, rtol=1e-12, check_every=3)
    g.guards("max_iters too low")
    print(res)
    assert res.steps_done == 2 and res.unconverged_steps == 2 and res.iterations == (2, 2) and not res.breakdown
    assert torch.equal(g.arena.bits(1), before[1])


# ---- 6. the layers above ---------------------------------------------------------------------------------------------------------
def test_the_host_operators_are_the_plan_drivers(L):
    from lorastencil_amd import _lib

    shape, dims, w, x, f = small_problem(L)
    # the host operators build their plan from the shape's own taps: integers that sum to 100, so both sides run in
    # normalised-weights mode, taps / 100 -- point-symmetric, the centre 0.16
    old = _lib.lib().lora_set_default_normalize(1)
    try:
        plan = L.Plan(shape, dims)
        g = Grids(L, shape, dims, 16, [x, f, x])
        res = plan.run_pcg_until(g.v[0], g.v[1], tol=0.0, check_every=2, max_times=4)
        out, hres, info = L.run_host_pcg(shape, x, 0.0, source=f, check_every=2, max_times=4)
        tres = plan.run_theta_mg(g.v[2], g.v[1], 8.0, 2, theta=0.5, max_iters=30, rtol=1e-8, check_every=2)
        tout, htres, tinfo = L.run_host_theta_mg(shape, x, 8.0, 2, source=f, theta=0.5, max_iters=30, rtol=1e-8, check_every=2)
    finally:
        _lib.lib().lora_set_default_normalize(old)
    assert abs(plan.weights.sum() - 1.0) < 1e-12 and np.isfinite(res.until.residual)
    assert hres.until.times_done == 4 and hres.levels == res.levels and hres.until.residual == res.until.residual
    assert np.array_equal(out.view(np.int64), g.v[0].cpu().numpy().view(np.int64))
    assert info.sweep_seconds > 0 and info.hbm_gbs > 0 and info.steps_per_launch == 1
    assert htres == tres._replace(iterations=()) and htres.steps_done == 2 and htres.unconverged_steps == 0
    assert np.array_equal(tout.view(np.int64), g.v[2].cpu().numpy().view(np.int64))
    assert tinfo.sweep_seconds > 0 and tinfo.hbm_gbs > 0


def test_cli_flags(L):
    """starting the tools is what this test is about"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe2, exe3 = (os.path.join(root, "lorastencil_amd", "bin", f"lorastencil_{d}d") for d in (2, 3))
    run = lambda *a: subprocess.run(list(a), capture_output=True, text=True, timeout=120)
    r = run(exe2, "star2d1r", "64", "64", "40", "--pcg", "--normalize", "--source=point:1", "--until=1e-9")
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[0] == "INFO: shape = star_2d1r, m = 64, n = 64, times = 40"
    assert lines[1] == "LoRAStencil(2D star_2d1r): " and lines[2].startswith("Time = ") and lines[3].startswith("GStencil/s = ")
    assert any(ln.startswith("Preconditioned conjugate gradients on I - S: V(2,2), omega = 0.8, levels = 5, iterations = ") for ln in lines)
    assert any(ln.startswith("Until: times_done = ") and ", converged, residual = " in ln and "checked every 2 steps" in ln for ln in lines)
    r = run(exe3, "star3d1r", "16", "16", "16", "40", "--pcg=1", "--normalize", "--until=1e-9", "--check-every=4")
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert any(ln.startswith("Preconditioned conjugate gradients on I - S: V(1,1), omega = 0.8, levels = 3,") for ln in r.stdout.splitlines())
    assert any(", converged, " in ln and "checked every 4 steps" in ln for ln in r.stdout.splitlines())
    r = run(exe2, "star2d1r", "64", "64", "3", "--normalize", "--bc=dirichlet", "--implicit=64", "--precond=mg", "--iters=30", "--source=const:1",
            "--check-every=3")
    print(r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and any(ln.startswith("Implicit: theta = 1, tau = 64, steps = 3, iterations = ") and "unconverged steps = 0" in ln for ln in lines)
    assert "Preconditioner: one V(2,2) cycle a solve, omega = 0.8, state read back every 3 iterations" in lines
    r = run(exe3, "star3d1r", "16", "16", "16", "2", "--normalize", "--implicit=64", "--precond=mg:1", "--iters=30")
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "Preconditioner: one V(1,1) cycle a solve, omega = 0.8, state read back every 2 iterations" in r.stdout.splitlines()
    # the reference's integer taps leave no positive diagonal: refused, not run
    r = run(exe2, "star2d1r", "64", "64", "40", "--pcg", "--until=1e-9")
    assert r.returncode == 1 and "diagonal" in r.stdout
    # exclusive the way --mg is, and it needs --until; --precond only with --implicit
    for extra in ("--mg", "--cg", "--chebyshev=0.5", "--implicit=2", "--leapfrog", "--gpus=2", "--grid=1x2"):
        r = run(exe2, "star2d1r", "64", "64", "40", "--pcg", "--normalize", "--until=1e-9", extra)
        assert r.returncode == 1 and ("--pcg runs on one GPU" in r.stderr or "--mg runs on one GPU" in r.stderr), extra
    r = run(exe2, "star2d1r", "64", "64", "40", "--pcg", "--normalize")
    assert r.returncode == 1 and "needs --until" in r.stderr
    r = run(exe2, "star2d1r", "64", "64", "40", "--pcg=0", "--normalize", "--until=1e-9")
    assert r.returncode == 1 and "--pcg=N" in r.stderr
    r = run(exe2, "star2d1r", "64", "64", "40", "--pcg", "--normalize", "--until=1e-9", "--check-every=3")
    assert r.returncode == 1 and "even" in r.stderr
    r = run(exe2, "star2d1r", "64", "64", "40", "--precond=mg", "--normalize")
    assert r.returncode == 1 and "only with --implicit" in r.stderr
    r = run(exe2, "star2d1r", "64", "64", "40", "--implicit=8", "--precond=jacobi", "--normalize")
    assert r.returncode == 1 and "Unknown option" in r.stderr
