"""GPU tests of the 3D two-step leapfrog launch behind plan option "leap3" (kernels_3d_step2.hip).  Every comparison
is bit for bit.

Contract under test: with the option on, a 3D fp64 plan with an even innermost extent has lora_plan_leapfrog_depth 2; one launch
of lora_plan_step2_leapfrog[_src][_region] equals two single steps (lora_plan_step_leapfrog_src) on any data, for the three rules
(c alone; a and c; a, c and f); it writes the interior cells of the region's planes of out1 and out2 and nothing else, reads no halo
cell of f and nothing outside the padded arrays; runs and Chebyshev solves give the bits they give without the option.

Memory: prev, cur, f, out1, out2 are five buffers carved by tests/arena.py out of one poisoned allocation, at every offset of
arena.OFFSETS.  prev and cur hold different seeded values in their halos too; the halo of f is NaN, so a halo cell of f that is
read shows in the results.  After every call the guard bands are intact and prev, cur and f are unchanged bit for bit.

Shapes: the smallest that reach each way the kernel can go wrong -- (1, 1, 2) the smallest grid; (3, 2, 8) a small grid in one
tile; (12, 30, 60) exactly one output tile of 30 x 60; (19, 33, 62) with fused_z_chunk = 8: 2 x 2 ragged tiles, three chunks along
z, the last one short; (9, 31, 124): three column tiles, rim tiles only in y.
"""
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = -7.0  # what an output buffer holds before a launch: a cell the launch must not write keeps it
COEFS = ((1.0, -1.0), (0.7, 0.3), (1.9, -0.9))  # 0.7 * t and 0.3 * prev round, so a contracted fused multiply-add shows
SHAPES = ("star3d1r", "box3d1r")
# (dims, options beside leap3)
GRIDS = [((1, 1, 2), {}), ((3, 2, 8), {}), ((12, 30, 60), {}), ((19, 33, 62), {"fused_z_chunk": 8}), ((9, 31, 124), {})]
CASES = [(s, d, o) for d, o in GRIDS for s in SHAPES]
IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d, _ in CASES]
BIG = (19, 33, 62)
TIMES = (0, 1, 3, 4, 5, 8, 11)


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def real_taps(L, shape):
    """small integers on the shape's own support (the plan resolves the same tap set), divided by their sum: taps that round"""
    on = L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0
    w = np.where(on, 1.0 + np.arange(on.size) % 3, 0.0)
    return w / w.sum()


def regions_of(h):
    """the whole range, one that starts and ends inside chunks, the last plane, an empty one"""
    inner = (3, 14) if h > 14 else ((1, h - 1) if h >= 3 else None)
    out = [(0, h)] + ([inner] if inner else []) + [(h - 1, h), (h // 2, h // 2)]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def host_data(dims):
    """per grid, made once, read-only: seeded non-integer prev, cur (whole padded arrays, so their halos differ) and f, whose halo
    is NaN"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("leap3", dims)).encode()))
    ps = L.padded_shape("star3d1r", dims)
    prev, cur = rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 2.0
    f = np.full(ps, np.nan)
    L.interior("star3d1r", f)[...] = rng.standard_normal(dims) * 1.5
    for a in (prev, cur, f):
        a.setflags(write=False)
    return prev, cur, f


def bits_of(t):
    return t.view(__import__("torch").int64)


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


class Grids:
    """prev, cur, f and two or one more buffers carved out of one poisoned allocation"""

    def __init__(self, L, dims, offset, prev, cur, f, n_buffers=5):
        import torch
        from arena import carve

        self.arena = carve(L.padded_shape("star3d1r", dims), "f64", n_buffers=n_buffers, offset_bytes=offset)
        self.prev, self.cur, self.f = self.arena.views[0], self.arena.views[1], self.arena.views[2]
        self.spare = self.arena.views[3:]
        self.h_prev = torch.from_numpy(np.array(prev)).cuda()
        self.h_cur = torch.from_numpy(np.array(cur)).cuda()
        self.h_f = torch.from_numpy(np.array(f)).cuda()
        self.f.copy_(self.h_f)
        self.reset()

    def reset(self):
        self.prev.copy_(self.h_prev)
        self.cur.copy_(self.h_cur)
        for s in self.spare:
            s.fill_(FILL)

    def check(self, what, kept=()):
        """guards intact; f, and every buffer of `kept` (pairs of a view and what it held), unchanged bit for bit"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i, (view, was) in enumerate(((self.f, self.h_f),) + tuple(kept)):
            assert torch.equal(bits_of(view), bits_of(was)), f"{what}: read-only buffer {i} was written"


def rules(g, k):
    """the three rules with coefficient pair k for the first step and k + 1 for the second: (name, f buffer, its pristine copy,
    a1, c1, a2, c2); the rule that has c alone takes one c for both steps and a = 1"""
    a1, c1 = COEFS[k]
    a2, c2 = COEFS[(k + 1) % len(COEFS)]
    return [("c", None, None, 1.0, c1, 1.0, c1), ("a,c", None, None, a1, c1, a2, c2), ("a,c,f", g.f, g.h_f, a1, c1, a2, c2)]


def two_single_steps(ref, g, h_src, a1, c1, a2, c2):
    """whole-grid single steps on copies: level 1 carries prev's halo, level 2 cur's"""
    l1 = g.h_prev.clone()
    ref.step_leapfrog_src(g.h_cur, l1, h_src, a1, c1)
    l2 = g.h_cur.clone()
    ref.step_leapfrog_src(l1, l2, h_src, a2, c2)
    return l1, l2


def launch(q, g, name, src, o1, o2, a1, c1, a2, c2, region):
    if name == "c":
        if region is None:
            q.step2_leapfrog(g.prev, g.cur, o1, o2, c1)
        else:
            q.step2_leapfrog_region(g.prev, g.cur, o1, o2, c1, *region)
    elif region is None:
        q.step2_leapfrog_src(g.prev, g.cur, src, o1, o2, a1, c1, a2, c2)
    else:
        q.step2_leapfrog_src_region(g.prev, g.cur, src, o1, o2, a1, c1, a2, c2, *region)


@pytest.mark.parametrize("shape,dims,opts", CASES, ids=IDS)
def test_two_step_launch_is_two_single_steps(L, shape, dims, opts):
    """out1 and out2 on the planes of the region against whole-grid single steps with (a1, c1) != (a2, c2), so a swap shows; cells
    outside the region and all halo cells keep the fill value; the whole-grid entry is the same launch"""
    import torch
    from arena import OFFSETS

    prev, cur, f = host_data(dims)
    w = real_taps(L, shape)
    ref = L.Plan(shape, dims).set_weights(w)
    assert ref.leapfrog_depth == 1
    q = L.Plan(shape, dims).set_weights(w).set_option("leap3", 1)
    for key, value in opts.items():
        q.set_option(key, value)
    assert q.leapfrog_depth == 2
    sig = q.kernel_signature
    for n, off in enumerate(OFFSETS):
        g = Grids(L, dims, off, prev, cur, f)
        o1, o2 = g.spare
        k = n % len(COEFS)
        for name, src, h_src, a1, c1, a2, c2 in rules(g, k):
            l1, l2 = two_single_steps(ref, g, h_src, a1, c1, a2, c2)
            assert not bool(torch.isnan(L.interior(shape, l2)).any())  # (no halo cell of f got in on the reference's side either)
            for region in regions_of(dims[0]) + [None]:
                begin, end = region if region else (0, dims[0])
                want1, want2 = torch.full_like(l1, FILL), torch.full_like(l2, FILL)
                L.interior(shape, want1)[begin:end] = L.interior(shape, l1)[begin:end]
                L.interior(shape, want2)[begin:end] = L.interior(shape, l2)[begin:end]
                g.reset()
                launch(q, g, name, src, o1, o2, a1, c1, a2, c2, region)
                g.check(f"{shape} {dims} rule {name} {region}", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                where = (off, name, region)
                assert same_bits(o1, want1), where + ("out1", int((bits_of(o1) != bits_of(want1)).sum()))
                assert same_bits(o2, want2), where + ("out2", int((bits_of(o2) != bits_of(want2)).sum()))
    assert q.kernel_signature == sig and q.leapfrog_depth == 2


@pytest.mark.parametrize("shape", SHAPES)
def test_non_finite_data_gives_the_bits_of_two_single_steps(L, shape):
    """NaN, +inf and -inf in interior cells of cur, prev and f -- at tile corners, tile seams, chunk seams and the grid's faces:
    the same positions and the same bit patterns as two single steps"""
    import torch

    dims = BIG
    prev, cur, f = (np.array(x) for x in host_data(dims))
    h, m, n = dims
    spots = [(0, 0, 0), (h - 1, m - 1, n - 1), (7, 29, 59), (8, 30, 60), (15, 31, 61), (16, 0, 30), (9, 15, 1), (18, 32, 0), (4, 30, 59)]
    vals = [np.nan, np.inf, -np.inf]
    for i, s in enumerate(spots):
        (L.interior(shape, cur), L.interior(shape, prev), L.interior(shape, f))[i % 3][s] = vals[(i // 3) % 3]
    L.interior(shape, cur)[10, 3, 40:44] = [np.inf, -np.inf, np.nan, np.inf]  # inf - inf inside one window
    w = real_taps(L, shape)
    ref = L.Plan(shape, dims).set_weights(w)
    q = L.Plan(shape, dims).set_weights(w).set_option("leap3", 1).set_option("fused_z_chunk", 8)
    g = Grids(L, dims, 48, prev, cur, f)
    o1, o2 = g.spare
    for k in range(len(COEFS)):
        for name, src, h_src, a1, c1, a2, c2 in rules(g, k):
            l1, l2 = two_single_steps(ref, g, h_src, a1, c1, a2, c2)
            assert bool(torch.isnan(L.interior(shape, l2)).any()) and bool(torch.isfinite(L.interior(shape, l2)).any())
            for region in ((0, h), (3, 14)):
                g.reset()
                launch(q, g, name, src, o1, o2, a1, c1, a2, c2, region)
                g.check(f"{shape} non-finite rule {name} {region}", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                b, e = region
                for got, exp, what in ((o1, l1, "out1"), (o2, l2, "out2")):
                    gi, ei = L.interior(shape, got)[b:e], L.interior(shape, exp)[b:e]
                    assert same_bits(gi, ei), (k, name, region, what, int((bits_of(gi.contiguous()) != bits_of(ei.contiguous())).sum()))


@pytest.mark.parametrize("bc", ["reference", "dirichlet"])
@pytest.mark.parametrize("shape", SHAPES)
def test_runs_equal_the_runs_without_the_option(L, shape, bc):
    """run_leapfrog and run_leapfrog_src, per-step Chebyshev coefficients: both buffers, against the same plan with leap3 = 0"""
    dims = BIG
    prev, cur, f = host_data(dims)
    w = real_taps(L, shape)
    a, c = L.chebyshev_coeffs(0.95, 1, max(TIMES))
    g = Grids(L, dims, 112, prev, cur, f, n_buffers=3)
    off_plan = L.Plan(shape, dims).set_weights(w).set_boundary(bc)
    on_plan = L.Plan(shape, dims).set_weights(w).set_boundary(bc).set_option("leap3", 1).set_option("fused_z_chunk", 8)
    assert off_plan.leapfrog_depth == 1 and on_plan.leapfrog_depth == 2
    for times in TIMES:
        for src in (g.f, None):
            g.reset()
            off_plan.run_leapfrog_src(g.prev, g.cur, src, a, c, times)
            g.check("reference run")
            want = (g.prev.clone(), g.cur.clone())
            g.reset()
            on_plan.run_leapfrog_src(g.prev, g.cur, src, a, c, times)
            g.check(f"{shape} {bc} run_leapfrog_src({times}) f={src is not None}")
            assert same_bits(g.prev, want[0]) and same_bits(g.cur, want[1]), (times, src is not None)
        g.reset()
        off_plan.run_leapfrog(g.prev, g.cur, -0.9, times)
        want = (g.prev.clone(), g.cur.clone())
        g.reset()
        on_plan.run_leapfrog(g.prev, g.cur, -0.9, times)
        g.check(f"{shape} {bc} run_leapfrog({times})")
        assert same_bits(g.prev, want[0]) and same_bits(g.cur, want[1]), times
    assert on_plan.leapfrog_depth == 2


@pytest.mark.parametrize("how", ["periodic", "scratch=0"])
def test_runs_that_take_single_steps_only(L, how):
    """the periodic boundary and scratch = 0 run single steps whatever the option says: equal as well"""
    shape, dims = "star3d1r", BIG
    prev, cur, f = host_data(dims)
    w = real_taps(L, shape)
    a, c = L.chebyshev_coeffs(0.95, 1, 8)
    g = Grids(L, dims, 240, prev, cur, f, n_buffers=3)

    def plan(leap3):
        p = L.Plan(shape, dims).set_weights(w).set_option("leap3", leap3)
        return p.set_boundary("periodic") if how == "periodic" else p.set_option("scratch", 0)

    for times in (5, 8):
        got = []
        for leap3 in (0, 1):
            for run in (lambda p: p.run_leapfrog_src(g.prev, g.cur, g.f, a, c, times), lambda p: p.run_leapfrog(g.prev, g.cur, -0.9, times)):
                g.reset()
                run(plan(leap3))
                g.check(f"{how} leap3={leap3} times={times}")
                got.append((g.prev.clone(), g.cur.clone()))
        for i in (0, 1):
            assert same_bits(got[i][0], got[i + 2][0]) and same_bits(got[i][1], got[i + 2][1]), (times, i)


@pytest.mark.parametrize("norm", ["max", "rms"])
def test_run_chebyshev_until_with_and_without_the_option(L, norm):
    """star3d1r (35, 17, 130), the Jacobi problem of tests/test_gpu_leapfrog_src.py: the same times_done, checks and converged, and the
    same bits in both buffers"""
    import math

    shape, dims = "star3d1r", (35, 17, 130)
    w = np.zeros(L.ops.ntaps(shape))
    for ax in range(3):
        w[13 - 3 ** ax] = w[13 + 3 ** ax] = 1.0 / 6
    rng = np.random.default_rng(5)
    f = np.zeros(L.padded_shape(shape, dims))
    L.interior(shape, f)[...] = rng.integers(-8, 9, dims) / 64.0
    rho = sum(math.cos(math.pi / (m + 1)) for m in dims) / 3
    zero = np.zeros_like(f)
    g = Grids(L, dims, 16, zero, zero, f, n_buffers=3)
    seen = []
    for leap3 in (0, 1):
        p = L.Plan(shape, dims).set_weights(w).set_option("leap3", leap3)
        assert p.leapfrog_depth == 1 + leap3
        g.reset()
        r = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-9, rtol=0.0, norm=norm, check_every=20, max_times=400)
        g.check(f"run_chebyshev_until leap3={leap3}")
        print(norm, leap3, r)
        seen.append((r, g.prev.clone(), g.cur.clone()))
    (r0, p0, c0), (r1, p1, c1) = seen
    assert r0.converged and 0 < r0.times_done <= 400
    assert (r1.times_done, r1.checks, r1.converged, r1.diverged) == (r0.times_done, r0.checks, r0.converged, r0.diverged)
    assert np.array(r1.residual).tobytes() == np.array(r0.residual).tobytes()
    assert same_bits(p0, p1) and same_bits(c0, c1)


def test_host_entry_and_cli(L):
    """run_host_leapfrog under set_default_leap3(1) equals the default run bit for bit; the CLI prints the same lines"""
    shape, dims = "star3d1r", (12, 30, 60)
    rng = np.random.default_rng(11)
    ps = L.padded_shape(shape, dims)
    cur, prev = rng.standard_normal(ps), rng.standard_normal(ps)
    out0, info0 = L.run_host_leapfrog(shape, cur, prev, c=-0.9, times=9)
    assert info0.steps_per_launch == 1
    assert L.set_default_leap3(1) == 0
    try:
        out1, info1 = L.run_host_leapfrog(shape, cur, prev, c=-0.9, times=9)
    finally:
        assert L.set_default_leap3(0) == 1
    assert info1.steps_per_launch == 2
    assert np.array_equal(out0.view(np.int64), out1.view(np.int64))

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_3d")
    timing = ("Time = ", "GStencil/s = ", "GStencils/s ", "Algorithmic HBM traffic", "Total incl. transfers")
    seen = []
    for extra in ([], ["--leap3"]):
        run = subprocess.run([exe, "star3d1r", "12", "30", "60", "9", "--leapfrog=-0.9", "--normalize", *extra], capture_output=True,
                             text=True, timeout=120)
        print(run.stdout, run.stderr)
        assert run.returncode == 0
        lines = run.stdout.splitlines()
        assert lines[0] == "INFO: shape = star_3d1r, h = 12, m = 30, n = 60, times = 9"
        assert sum(ln.startswith(timing) for ln in lines) == len(timing)
        assert any(ln.startswith("Result range = [") for ln in lines)
        seen.append([ln for ln in lines if not ln.startswith(timing)])
    assert seen[0] == seen[1]
