"""GPU tests of the scaled leapfrog step with a source and of the Chebyshev semi-iteration built on it (lora_plan_step_leapfrog_src
... lora_run_host_chebyshev; kernels_step.hip, kernels_2d_step2.hip, chebyshev.cpp):
u+ = a (S(u) + f) + c u-, the new level stored over the oldest one.

Contract under test: one step is t = fl(acc + f) (no f: t = acc), prev = fl(fl(a t) + fl(c prev)) on the interior cells of the swept
range, acc the bits of the plan's plain single sweep of cur; halo cells of prev never written and never used, cur and f never
written; the 2D two-step launch equals two single steps bit for bit; run_leapfrog_src equals that many single steps whatever its
schedule; the Chebyshev schedule on top of it meets the bound of the Chebyshev theorem where plain source sweeps are nowhere near.

Memory: the grids are FOUR or FIVE buffers carved by tests/arena.py out of one poisoned allocation, at offsets 16 and 240.  prev,
cur and f hold different seeded values in their halos too, so a mixed-up halo or a used halo of f shows.  After every call the
guard bands are intact and every read-only buffer is unchanged bit for bit.

Shapes: the cases, regions and offsets of tests/test_gpu_leapfrog.py -- the kernels have the tiles of the leapfrog kernels.
"""
import functools
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
FILL = -7.0  # what an output buffer holds before a launch: a cell the launch must not write keeps it
COEFS = ((1.0, -1.0), (0.7, 0.3), (1.9, -0.9))  # 0.7 * t and 0.3 * prev round, so a contracted fused multiply-add shows

# (shape, dims, regions): (0, n) the whole interior; 1D regions begin on an even point (the plan's region granularity)
CASES = [
    ("1d1r", (1,), [(0, 1)]),
    ("1d2r", (1027,), [(0, 1027), (2, 515), (510, 1027), (4, 4)]),
    ("star2d1r", (1, 2), [(0, 1)]),
    ("star2d1r", (70, 260), [(0, 70), (5, 37), (33, 70), (7, 7)]),
    ("star2d3r", (70, 260), [(0, 70), (5, 37), (33, 70)]),
    ("box2d3r", (70, 260), [(0, 70), (5, 37), (33, 70)]),
    ("star2d1r", (7, 13), [(0, 7), (2, 5)]),
    ("box2d3r", (7, 13), [(0, 7)]),
    ("star3d1r", (1, 1, 2), [(0, 1)]),
    ("box3d1r", (35, 17, 130), [(0, 35), (1, 34), (33, 35), (9, 9)]),
    ("star3d1r", (35, 17, 130), [(0, 35), (1, 34)]),
    ("star3d1r", (3, 5, 7), [(0, 3), (1, 2)]),
    ("box3d1r", (3, 5, 7), [(0, 3)]),
]
IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d, _ in CASES]
FUSED = [c for c in CASES if len(c[1]) == 2 and c[1][1] % 2 == 0]  # the plans that have the two-step launch
FUSED_IDS = [IDS[CASES.index(c)] for c in FUSED]
RUNS = [CASES[i] for i in (1, 3, 4, 5, 6, 9, 10, 11)]
RUN_IDS = [IDS[CASES.index(c)] for c in RUNS]
TIMES = (0, 1, 2, 3, 4, 5, 7, 8, 12, 13)


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def support(L, shape):
    return L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0


def real_taps(L, shape):
    """small integers on the shape's own support (the plan resolves the same tap set), divided by their sum: taps that round"""
    on = support(L, shape)
    w = np.where(on, 1.0 + np.arange(on.size) % 3, 0.0)
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def host_data(shape, dims):
    """per case, made once, read-only: three seeded real grids (prev, cur, f), whole padded arrays (so their halos differ)"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("leapfrog_src", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    out = (rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 2.0, rng.standard_normal(ps) * 1.5)
    for a in out:
        a.setflags(write=False)
    return out


def bits_of(t):
    return t.view(__import__("torch").int64)


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


class Grids:
    """prev, cur, f and one or two more buffers carved out of one poisoned allocation"""

    def __init__(self, L, shape, dims, offset, prev, cur, f, n_buffers=4):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, dims
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=n_buffers, offset_bytes=offset)
        self.prev, self.cur, self.f = self.arena.views[0], self.arena.views[1], self.arena.views[2]
        self.spare = self.arena.views[3:]
        self.h_prev = torch.from_numpy(np.array(prev)).cuda()
        self.h_cur = torch.from_numpy(np.array(cur)).cuda()
        self.h_f = torch.from_numpy(np.array(f)).cuda()
        self.f.copy_(self.h_f)
        self.reset()

    def reset(self, spare=FILL):
        self.prev.copy_(self.h_prev)
        self.cur.copy_(self.h_cur)
        for s in self.spare:
            s.fill_(spare)

    def check(self, what, kept=()):
        """guards intact; f, and every buffer of `kept` (pairs of a view and what it held), unchanged bit for bit"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i, (view, was) in enumerate(((self.f, self.h_f),) + tuple(kept)):
            assert torch.equal(bits_of(view), bits_of(was)), f"{what}: read-only buffer {i} was written"


def single_steps(p, prev, cur, f, a, c, times, periodic=False):
    """the engine's own loop of single in-place steps with coefficient i clamped to the arrays' end; returns the buffers of
    (level times - 1, level times)"""
    lv = [prev, cur]
    if periodic and times:
        p.halo(lv[1], "wrap")
    for i in range(times):
        k = min(i, len(a) - 1)
        p.step_leapfrog_src(lv[1], lv[0], f, float(a[k]), float(c[k]))
        if periodic:
            p.halo(lv[0], "wrap")
        lv.reverse()
    return lv


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_single_step_is_the_plain_sweep_then_separate_operations(L, shape, dims, regions):
    """bit for bit on seeded real data: every cell of prev, so the halo and the rows outside the region too.  Expected: the plain
    step_region into a spare buffer, then spare + f, a * ., c * prev, + as separate eager torch operations on the region's interior;
    with and without f; without f and with a = 1 also the bits of lora_plan_step_leapfrog"""
    prev, cur, f = host_data(shape, dims)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, f)
        p = L.Plan(shape, dims).set_weights(real_taps(L, shape))
        sig = p.kernel_signature
        tmp = g.spare[0]
        for a, c in COEFS:
            for src in (g.f, None):
                for begin, end, whole in [(b, e, False) for b, e in regions] + [(0, dims[0], True)]:  # (last: the whole-grid entry)
                    g.reset()
                    p.step_region(g.cur, tmp, begin, end)
                    want = g.h_prev.clone()
                    t = L.interior(shape, tmp)[begin:end]
                    if src is not None:
                        t = t + L.interior(shape, g.h_f)[begin:end]  # one rounding
                    x = a * t                                         # another
                    y = c * L.interior(shape, g.h_prev)[begin:end]    # another
                    L.interior(shape, want)[begin:end] = x + y        # and the last
                    if whole:
                        p.step_leapfrog_src(g.cur, g.prev, src, a, c)
                    else:
                        p.step_leapfrog_src_region(g.cur, g.prev, src, a, c, begin, end)
                    g.check(f"{shape} {dims} a={a} c={c} f={src is not None} [{begin}, {end})", kept=[(g.cur, g.h_cur)])
                    bad = int((bits_of(g.prev) != bits_of(want)).sum())
                    assert bad == 0, (off, a, c, src is not None, begin, end, whole, bad)
                    if src is None and a == 1.0 and not whole:
                        leap = g.h_prev.clone()
                        p.step_leapfrog_region(g.h_cur, leap, c, begin, end)
                        assert same_bits(g.prev, leap), (off, c, begin, end)
        assert p.kernel_signature == sig and p.leapfrog_depth == (2 if len(dims) == 2 and dims[1] % 2 == 0 else 1)


@pytest.mark.parametrize("shape,dims,regions", FUSED, ids=FUSED_IDS)
def test_two_step_launch_is_two_single_steps(L, shape, dims, regions):
    """out1 and out2 on the rows of the region against whole-grid single steps with (a1, c1) != (a2, c2), so a swap shows; cells
    outside the region keep the fill value; also with the structured evaluation forms requested or forbidden -- the launch
    evaluates direct taps whatever lowrank_valu says"""
    import torch

    prev, cur, f = host_data(shape, dims)
    w = real_taps(L, shape)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, f, n_buffers=5)
        o1, o2 = g.spare
        base = L.Plan(shape, dims).set_weights(w)
        assert base.leapfrog_depth == 2
        for k, (a1, c1) in enumerate(COEFS):
            a2, c2 = COEFS[(k + 1) % len(COEFS)]
            for src, h_src in ((g.f, g.h_f), (None, None)):
                l1 = g.h_prev.clone()
                base.step_leapfrog_src(g.h_cur, l1, h_src, a1, c1)   # level 1, prev's halo
                l2 = g.h_cur.clone()
                base.step_leapfrog_src(l1, l2, h_src, a2, c2)        # level 2, cur's halo
                for begin, end in regions:
                    want1, want2 = torch.full_like(l1, FILL), torch.full_like(l2, FILL)
                    L.interior(shape, want1)[begin:end] = L.interior(shape, l1)[begin:end]
                    L.interior(shape, want2)[begin:end] = L.interior(shape, l2)[begin:end]
                    for lowrank in (None, 0, 1, 4) if k == 0 else (None,):
                        q = base if lowrank is None else L.Plan(shape, dims).set_weights(w).set_option("lowrank_valu", lowrank)
                        g.reset()
                        q.step2_leapfrog_src_region(g.prev, g.cur, src, o1, o2, a1, c1, a2, c2, begin, end)
                        g.check(f"{shape} two steps {a1} {c1} {a2} {c2} [{begin}, {end})", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                        where = (off, k, src is not None, begin, end, lowrank)
                        assert same_bits(o1, want1), where + (int((bits_of(o1) != bits_of(want1)).sum()),)
                        assert same_bits(o2, want2), where + (int((bits_of(o2) != bits_of(want2)).sum()),)
                if (0, dims[0]) in regions:  # the whole-grid entry is the same launch
                    g.reset()
                    base.step2_leapfrog_src(g.prev, g.cur, src, o1, o2, a1, c1, a2, c2)
                    g.check("whole grid", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                    assert same_bits(L.interior(shape, o1), L.interior(shape, l1)) and same_bits(L.interior(shape, o2), L.interior(shape, l2))
                    assert bool((o1 == FILL).any()) and bool((o2 == FILL).any())  # (the halos)


@pytest.mark.parametrize("bc", ["reference", "dirichlet", "periodic"])
@pytest.mark.parametrize("shape,dims,regions", RUNS, ids=RUN_IDS)
def test_run_is_that_many_single_steps(L, shape, dims, regions, bc):
    """both final levels, in the buffers the contract names: constant coefficients, three that are clamped, and one per step; with
    and without the scratch grids, and a second time on the same plan"""
    prev, cur, f = host_data(shape, dims)
    w = real_taps(L, shape)
    rng = np.random.default_rng(17)
    per_step_a, per_step_c = rng.uniform(0.5, 1.5, 16), rng.uniform(-1.0, 0.5, 16)
    coefs = {1: (per_step_a[:1], per_step_c[:1]), 3: (per_step_a[:3], per_step_c[:3]), 16: (per_step_a, per_step_c)}
    g = Grids(L, shape, dims, OFFSETS[0], prev, cur, f)
    ref = L.Plan(shape, dims).set_weights(w).set_boundary(bc)
    want = {}
    for n, (a, c) in coefs.items():
        for times in TIMES:
            g.reset()
            lv = single_steps(ref, g.prev, g.cur, g.f, a, c, times, periodic=bc == "periodic")
            assert (lv[1] is g.cur) == (times % 2 == 0)
            want[n, times] = (g.prev.clone(), g.cur.clone())
    for scratch in (0, 1):
        p = L.Plan(shape, dims).set_weights(w).set_boundary(bc).set_option("scratch", scratch)
        sig = p.kernel_signature
        for n, (a, c) in coefs.items():
            for times in TIMES + (8, 13):
                g.reset()
                p.run_leapfrog_src(g.prev, g.cur, g.f, a, c, times)
                g.check(f"{shape} {bc} scratch={scratch} ncoef={n} run_leapfrog_src({times})")
                for name, got, exp in zip(("prev", "cur"), (g.prev, g.cur), want[n, times]):
                    assert same_bits(got, exp), (bc, scratch, n, times, name, int((bits_of(got) != bits_of(exp)).sum()))
        assert p.kernel_signature == sig
    # without a source, through the same schedule
    a, c = coefs[3]
    for times in (5, 13):
        g.reset()
        single_steps(ref, g.prev, g.cur, None, a, c, times, periodic=bc == "periodic")
        exp = (g.prev.clone(), g.cur.clone())
        g.reset()
        ref.run_leapfrog_src(g.prev, g.cur, None, a, c, times)
        g.check(f"{shape} {bc} no source run_leapfrog_src({times})")
        assert same_bits(g.prev, exp[0]) and same_bits(g.cur, exp[1]), (bc, times)


# ---- convergence: u = S(u) + f with S = the mean of the 2 d neighbours, zero halos ------------------------------------------
def jacobi_problem(L, shape, dims):
    """taps 1 / (2 d) on the 2 d neighbours and 0 at the centre; f = integers in [-8, 8] / 64 on the interior, zero halo;
    returns (taps, padded f, rho) with rho the spectral radius of S under zero halos"""
    d = len(dims)
    side = {1: 9, 2: 7, 3: 3}[d]  # the tap table: 9 taps, 7 x 7, 3 x 3 x 3
    w = np.zeros(L.ops.ntaps(shape))
    assert w.size == side ** d
    centre = w.size // 2
    for ax in range(d):
        w[centre - side ** ax] = w[centre + side ** ax] = 1.0 / (2 * d)
    assert support(L, shape)[w != 0].all()
    rng = np.random.default_rng(zlib.crc32(repr(("poisson", shape, dims)).encode()))
    f = np.zeros(L.padded_shape(shape, dims))
    L.interior(shape, f)[...] = rng.integers(-8, 9, dims) / 64.0
    rho = sum(math.cos(math.pi / (m + 1)) for m in dims) / d
    return w, f, rho


def true_residual(L, shape, u, f):
    """S(u) + f - u on the interior, in numpy from the padded host arrays (zero halos)"""
    ui = L.interior(shape, u)
    d = ui.ndim
    p = np.pad(ui, 1)
    s = np.zeros_like(ui)
    for ax in range(d):
        lo, hi = [slice(1, -1)] * d, [slice(1, -1)] * d
        lo[ax], hi[ax] = slice(0, -2), slice(2, None)
        s += (p[tuple(lo)] + p[tuple(hi)]) / (2 * d)
    return s + L.interior(shape, f) - ui


def rms(x):
    return math.sqrt(float((x * x).mean()))


def theorem_bound(rho, k):
    """2 s^k / (1 + s^2k), s = rho / (1 + sqrt(1 - rho^2)): the Chebyshev theorem's reduction of the 2-norm of the residual of a
    symmetric S with spectrum in [-rho, rho] after k steps from u(0)"""
    s = rho / (1.0 + math.sqrt(1.0 - rho * rho))
    return 2.0 * s ** k / (1.0 + s ** (2 * k))


@pytest.mark.parametrize("shape,dims,steps", [("star2d1r", (62, 64), 300), ("1d1r", (1027,), 4000), ("star3d1r", (35, 17, 130), 120)],
                         ids=["2d", "1d", "3d"])
def test_chebyshev_meets_the_theorem_bound_where_plain_sweeps_do_not(L, shape, dims, steps):
    """u0 = 0, so the first residual is f: after `steps` Chebyshev steps RMS(S(u) + f - u) / RMS(f) <= 1.01 x the theorem's bound
    (2D, 300 steps: 7.95e-7; emulated in numpy 5.7e-7.  1D, 4000: 9.8e-6; numpy 7.0e-6.  3D, 120: 2.4e-6; numpy 1.7e-6) -- derived,
    not tuned; the 1 % is for the rounding of the residual's own evaluation.  As many plain source sweeps from the same start
    leave the ratio >= 1e-3 (numpy: 1.7e-2, 5.9e-2, 6.1e-3)."""
    import torch

    w, f, rho = jacobi_problem(L, shape, dims)
    bound = theorem_bound(rho, steps)
    assert bound >= 1e-8
    if shape == "star2d1r":
        assert abs(bound - 7.95e-7) < 0.01e-7
    zero = np.zeros_like(f)
    g = Grids(L, shape, dims, OFFSETS[0], zero, zero, f)
    p = L.Plan(shape, dims).set_weights(w)
    a, c = L.chebyshev_coeffs(rho, 1, steps)
    p.run_leapfrog_src(g.prev, g.cur, g.f, a, c, steps)
    g.check("chebyshev run")
    u = (g.cur if steps % 2 == 0 else g.prev).cpu().numpy()
    ratio = rms(true_residual(L, shape, u, f)) / rms(L.interior(shape, f))
    print(shape, dims, steps, "chebyshev: RMS residual / RMS f =", ratio, "bound", bound)
    # the same number of plain sweeps with the source
    q = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(g.f)
    b0, b1 = torch.zeros_like(g.h_cur), torch.zeros_like(g.h_cur)
    q.run(b0, b1, steps)
    torch.cuda.synchronize()
    plain = rms(true_residual(L, shape, (b0 if steps % 2 == 0 else b1).cpu().numpy(), f)) / rms(L.interior(shape, f))
    print(shape, dims, steps, "plain sweeps: RMS residual / RMS f =", plain)
    assert ratio <= 1.01 * bound
    assert plain >= 1e-3


def test_run_chebyshev_until_converges_where_run_until_does_not(L):
    """star2d1r (62, 64), tol 1e-10 on the max norm, a check every 20 steps, 600 at most: Chebyshev converges (numpy: max residual
    8.7e-12 at step 500), plain source sweeps do not (numpy: 2.0e-3 at step 600).  `last` is the two-pass record of a plan that
    carries f as its source, the levels are those of run_leapfrog_src(times_done), the plan is what it was."""
    import torch

    shape, dims = "star2d1r", (62, 64)
    w, f, rho = jacobi_problem(L, shape, dims)
    zero = np.zeros_like(f)
    g = Grids(L, shape, dims, OFFSETS[1], zero, zero, f, n_buffers=5)
    p = L.Plan(shape, dims).set_weights(w)
    sig, depth = p.kernel_signature, p.leapfrog_depth
    r = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-10, rtol=0.0, norm="max", check_every=20, max_times=600)
    g.check("run_chebyshev_until")
    print("chebyshev until:", r)
    assert r.converged and not r.diverged and r.times_done % 20 == 0 and 0 < r.times_done <= 600
    assert r.checks == r.times_done // 20 and r.residual == r.last.max_abs and r.residual <= 1e-10
    assert p.kernel_signature == sig and p.leapfrog_depth == depth and p.get_option("source") == 0
    got_prev, got_cur = g.prev.clone(), g.cur.clone()
    # the probe's record: a source sweep into a spare grid plus lora_plan_diff
    q = L.Plan(shape, dims).set_weights(w).set_source(g.f)
    q.step(g.cur, g.spare[0])
    two = q.diff(g.spare[0], g.cur)
    for field in ("max_abs", "a_abs_max", "argmax", "count", "nonfinite"):
        a, b = getattr(r.last, field), getattr(two, field)
        assert np.array(a).tobytes() == np.array(b).tobytes(), (field, a, b)
    assert r.last.count == dims[0] * dims[1] and r.last.nonfinite == 0
    # the levels: run_leapfrog_src(times_done) with the schedule's coefficients
    a, c = L.chebyshev_coeffs(rho, 1, r.times_done)
    g.reset()
    p.run_leapfrog_src(g.prev, g.cur, g.f, a, c, r.times_done)
    g.check("run_leapfrog_src(times_done)")
    assert same_bits(g.cur, got_cur) and same_bits(g.prev, got_prev)
    # a second time on the same plan, from a d_prev whose interior is finite rubbish: step 1 has c = 0
    g.reset()
    L.interior(shape, g.prev).fill_(123.25)
    r2 = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-10, check_every=20, max_times=600)
    g.check("run_chebyshev_until again")
    assert r2.times_done == r.times_done and same_bits(g.cur, got_cur) and same_bits(g.prev, got_prev)
    # plain sweeps with the source and the same limits
    plain = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(g.f)
    b0, b1 = torch.zeros_like(g.h_cur), torch.zeros_like(g.h_cur)
    rp = plain.run_until(b0, b1, tol=1e-10, rtol=0.0, norm="max", check_every=20, max_times=600)
    print("plain until:", rp)
    assert not rp.converged and rp.times_done == 600 and rp.residual > 1e-6
    # the cap: not converging is no error
    g.reset()
    r3 = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-10, check_every=20, max_times=59)
    assert not r3.converged and r3.times_done == 40 and r3.checks == 2


def test_host_entry_and_cli_agree(L):
    shape, dims = "star2d1r", (62, 64)
    rho = sum(math.cos(math.pi / (m + 1)) for m in dims) / 2
    grid = L.reference_input(shape, dims)
    src = np.zeros_like(grid)
    L.interior(shape, src)[...] = 0.125
    out, r, info = L.run_host_chebyshev(shape, grid, rho, source=src, tol=1e-10, check_every=60, max_times=600)
    assert info.steps_per_launch == 2 and info.hbm_gbs > 0 and out.shape == grid.shape
    assert r.times_done % 60 == 0 and 0 < r.times_done <= 600
    # a fixed number of steps: the plan's run
    import torch

    out7, r7, _ = L.run_host_chebyshev(shape, grid, rho, times=7, source=src)
    assert r7.times_done == 7
    p = L.Plan(shape, dims)
    d_prev, d_cur, d_f = torch.from_numpy(grid).cuda(), torch.from_numpy(grid).cuda(), torch.from_numpy(src).cuda()
    a, c = L.chebyshev_coeffs(rho, 1, 7)
    p.run_leapfrog_src(d_prev, d_cur, d_f, a, c, 7)
    torch.cuda.synchronize()
    assert np.array_equal(out7.view(np.int64), d_prev.cpu().numpy().view(np.int64))  # times is odd: level 7 is in prev

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_2d")
    run = subprocess.run([exe, "star2d1r", "62", "64", "600", f"--chebyshev={rho!r}", "--until=1e-10", "--source=const:0.125",
                          "--bc=dirichlet"], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    lines = run.stdout.splitlines()
    assert lines[0] == "INFO: shape = star_2d1r, m = 62, n = 64, times = 600"
    assert lines[1] == "LoRAStencil(2D star_2d1r): " and lines[2].startswith("Time = ") and lines[3].startswith("GStencil/s = ")
    assert any(ln.startswith("Chebyshev: ") for ln in lines)
    m = [re.match(r"Until: times_done = (\d+), ", ln) for ln in lines]
    done = [int(x.group(1)) for x in m if x]
    assert done == [r.times_done]
