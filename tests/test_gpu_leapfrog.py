"""GPU tests of leapfrog stepping (lora_plan_step_leapfrog ... lora_run_host_leapfrog; kernels_step.hip,
kernels_2d_step2.hip): u(t+1) = S(u(t)) + c u(t-1), the new level stored over the oldest one.

Contract under test: one step is prev = fl(acc + fl(c * prev)) on the interior cells of the swept range, acc the bits of the
plan's plain single sweep of cur, in two roundings; halo cells of prev never written and never used, cur never written; the 2D
two-step launch equals two single steps bit for bit, level-1 cells outside the interior taking prev's halo; run_leapfrog
equals that many single steps whatever its schedule.

Memory: the grids are THREE or FOUR buffers carved by tests/arena.py out of one poisoned allocation, at offsets 16 and 240.
prev and cur hold different seeded values in their halos too, so a mixed-up halo shows.  After every call the guard bands
are intact and every read-only buffer is unchanged bit for bit.

Shapes: the cases, regions and offsets of tests/test_gpu_source.py -- the single-step kernels have the tiles of the source
kernels (1D 512 points per workgroup; 2D 32 rows x 128 columns; 3D 16 rows x 128 columns x chunks of 4 planes; odd innermost
extents one thread per point) and the two-step kernel those of the source rule's (4 R1 - 6 rows x 122 columns, R1 = 6
for the star, 10 for diamond and box):
  one cell                      (1,)       (1, 2)       (1, 1, 2)
  partial tile + two tiles per direction, regions that begin and end inside a tile, the empty region
                                (1027,) = 2 x 512 + 3, with the odd tail point
                                (70, 260) = 2 x 32 + 6 rows, 2 x 128 + 4 columns; 3 x 18 + 16 and 2 x 34 + 2 rows, 2 x 122 + 16 columns
                                (35, 17, 130) = 8 x 4 + 3 planes, 16 + 1 rows, 128 + 2 columns
  odd innermost extent          (7, 13)    (3, 5, 7)
"""
import functools
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
FILL = -7.0  # what an output buffer holds before a launch: a cell the launch must not write keeps it
CS = (-1.0, 0.7)  # 0.7 * prev rounds, so a contracted fused multiply-add shows

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
# one plan per kernel family: 1D, 2D tiled (and the two-step launch), 3D tiled, one thread per point in 2D and 3D
FAMILIES = [("1d1r", (1027,)), ("star2d1r", (70, 260)), ("star3d1r", (35, 17, 130)), ("star2d1r", (7, 13)), ("star3d1r", (3, 5, 7))]
FAMILY_IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d in FAMILIES]


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


def equal_dyadic_taps(L, shape):
    """2**-a on the shape's support, a the least exponent with a tap sum <= 1: returns (taps, a)"""
    on = support(L, shape)
    a = math.ceil(math.log2(on.sum()))
    return np.where(on, 2.0 ** -a, 0.0), a


@functools.lru_cache(maxsize=None)
def host_data(shape, dims):
    """per case, made once, read-only: two seeded real grids and two of integers 0..7, whole padded arrays (so the halos of a
    pair differ)"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("leapfrog", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    out = (rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 2.0, rng.integers(0, 8, ps).astype(np.float64),
           rng.integers(0, 8, ps).astype(np.float64))
    for a in out:
        a.setflags(write=False)
    return out


def bits_of(t):
    return t.view(__import__("torch").int64)


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


class Grids:
    """prev, cur and one or two more buffers carved out of one poisoned allocation"""

    def __init__(self, L, shape, dims, offset, prev, cur, n_buffers=3):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, dims
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=n_buffers, offset_bytes=offset)
        self.prev, self.cur = self.arena.views[0], self.arena.views[1]
        self.spare = self.arena.views[2:]
        self.h_prev = torch.from_numpy(np.array(prev)).cuda()
        self.h_cur = torch.from_numpy(np.array(cur)).cuda()
        self.reset()

    def reset(self, spare=FILL):
        self.prev.copy_(self.h_prev)
        self.cur.copy_(self.h_cur)
        for s in self.spare:
            s.fill_(spare)

    def check(self, what, kept=()):
        """guards intact; every buffer of `kept` (pairs of a view and what it held) unchanged bit for bit"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i, (view, was) in enumerate(kept):
            assert torch.equal(bits_of(view), bits_of(was)), f"{what}: read-only buffer {i} was written"


def single_steps(p, prev, cur, c, times, periodic=False):
    """the engine's own loop of single in-place steps; returns the buffers of (level times - 1, level times)"""
    lv = [prev, cur]
    if periodic and times:
        p.halo(lv[1], "wrap")
    for _ in range(times):
        p.step_leapfrog(lv[1], lv[0], c)
        if periodic:
            p.halo(lv[0], "wrap")
        lv.reverse()
    return lv


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_single_step_is_the_plain_sweep_then_plus_c_prev(L, shape, dims, regions):
    """bit for bit on seeded real data: every cell of prev, so the halo and the rows outside the region too.  Expected: the plain
    step_region into a spare buffer, then tmp + (c * prev) as two separate numpy operations on the host"""
    prev, cur, _, _ = host_data(shape, dims)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur)
        p = L.Plan(shape, dims).set_weights(real_taps(L, shape))
        assert p.leapfrog_depth == (2 if len(dims) == 2 and dims[1] % 2 == 0 else 1)
        sig = p.kernel_signature
        tmp = g.spare[0]
        for c in CS:
            for begin, end, whole in [(b, e, False) for b, e in regions] + [(0, dims[0], True)]:  # (last: the whole-grid entry)
                g.reset()
                p.step_region(g.cur, tmp, begin, end)
                want = np.array(prev)
                swept = L.interior(shape, tmp.cpu().numpy())[begin:end]
                scaled = c * L.interior(shape, np.array(prev))[begin:end]  # one rounding
                L.interior(shape, want)[begin:end] = swept + scaled        # ... and another
                if whole:
                    p.step_leapfrog(g.cur, g.prev, c)
                else:
                    p.step_leapfrog_region(g.cur, g.prev, c, begin, end)
                g.check(f"{shape} {dims} c={c} [{begin}, {end})", kept=[(g.cur, g.h_cur)])
                got = g.prev.cpu().numpy()
                bad = int((got.view(np.int64) != want.view(np.int64)).sum())
                assert bad == 0, (off, c, begin, end, whole, bad)
        assert p.kernel_signature == sig


@pytest.mark.parametrize("shape,dims,regions", FUSED, ids=FUSED_IDS)
def test_two_step_launch_is_two_single_steps(L, shape, dims, regions):
    """out1 and out2 on the rows of the region against whole-grid single steps (level 1 lives in prev's buffer, so it has
    prev's halo); cells outside the region keep the fill value; also with the structured evaluation forms requested or
    forbidden -- the launch evaluates direct taps whatever lowrank_valu says"""
    import torch

    prev, cur, _, _ = host_data(shape, dims)
    w = real_taps(L, shape)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, n_buffers=4)
        o1, o2 = g.spare
        base = L.Plan(shape, dims).set_weights(w)
        assert base.leapfrog_depth == 2
        for c in CS:
            l1 = g.h_prev.clone()
            base.step_leapfrog(g.h_cur, l1, c)   # level 1, prev's halo
            l2 = g.h_cur.clone()
            base.step_leapfrog(l1, l2, c)        # level 2, cur's halo
            for begin, end in regions:
                want1, want2 = torch.full_like(l1, FILL), torch.full_like(l2, FILL)
                L.interior(shape, want1)[begin:end] = L.interior(shape, l1)[begin:end]
                L.interior(shape, want2)[begin:end] = L.interior(shape, l2)[begin:end]
                for lowrank in (None, 0, 1, 4):
                    q = base if lowrank is None else L.Plan(shape, dims).set_weights(w).set_option("lowrank_valu", lowrank)
                    g.reset()
                    q.step2_leapfrog_region(g.prev, g.cur, o1, o2, c, begin, end)
                    g.check(f"{shape} two steps c={c} [{begin}, {end})", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                    assert same_bits(o1, want1), (off, c, begin, end, lowrank, int((bits_of(o1) != bits_of(want1)).sum()))
                    assert same_bits(o2, want2), (off, c, begin, end, lowrank, int((bits_of(o2) != bits_of(want2)).sum()))
            if (0, dims[0]) in regions:  # the whole-grid entry is the same launch
                g.reset()
                base.step2_leapfrog(g.prev, g.cur, o1, o2, c)
                g.check("whole grid", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                assert same_bits(L.interior(shape, o1), L.interior(shape, l1)) and same_bits(L.interior(shape, o2), L.interior(shape, l2))


@pytest.mark.parametrize("bc", ["reference", "periodic"])
@pytest.mark.parametrize("shape,dims,regions", RUNS, ids=RUN_IDS)
def test_run_is_that_many_single_steps(L, shape, dims, regions, bc):
    """both final levels, in the buffers the contract names, with and without the scratch grids, and a second time on the
    same plan"""
    prev, cur, _, _ = host_data(shape, dims)
    c = -0.7
    w = real_taps(L, shape)
    g = Grids(L, shape, dims, OFFSETS[0], prev, cur)
    ref = L.Plan(shape, dims).set_weights(w).set_boundary(bc)
    want = {}
    for times in TIMES:
        g.reset()
        lv = single_steps(ref, g.prev, g.cur, c, times, periodic=bc == "periodic")
        assert (lv[1] is g.cur) == (times % 2 == 0)
        want[times] = (g.prev.clone(), g.cur.clone())
    for scratch in (0, 1):
        p = L.Plan(shape, dims).set_weights(w).set_boundary(bc).set_option("scratch", scratch)
        sig = p.kernel_signature
        for times in TIMES + (8, 13):
            g.reset()
            if times == 12:
                p.prepare_leapfrog(times)
            p.run_leapfrog(g.prev, g.cur, c, times)
            g.check(f"{shape} {bc} scratch={scratch} run_leapfrog({times})")
            for name, got, exp in zip(("prev", "cur"), (g.prev, g.cur), want[times]):
                assert same_bits(got, exp), (bc, scratch, times, name, int((bits_of(got) != bits_of(exp)).sum()))
        assert p.kernel_signature == sig


@pytest.mark.parametrize("shape,dims", FAMILIES, ids=FAMILY_IDS)
def test_time_reversal_is_exact(L, shape, dims):
    """c = -1, integers 0..7, taps 2**-a on the support: six steps forward, the two levels swapped, six steps more, and the start
    is back.  Exactness: |u(t+1)| <= |u(t)| + |u(t-1)| (tap sum <= 1), so every value on the way is below 7 * 21 < 2**8
    (Fibonacci numbers up to step 7), and every value and partial sum is a multiple of 2**(-a (t + 1)) with t <= 5: at most
    8 + 6 a bits, which the assertion keeps under 53."""
    _, _, ip, ic = host_data(shape, dims)
    w, a = equal_dyadic_taps(L, shape)
    assert 8 + 6 * a <= 53
    g = Grids(L, shape, dims, OFFSETS[1], ip, ic)
    p = L.Plan(shape, dims).set_weights(w)
    p.run_leapfrog(g.prev, g.cur, -1.0, 6)
    g.check("forward")
    assert not same_bits(g.cur, g.h_cur)
    p.run_leapfrog(g.cur, g.prev, -1.0, 6)  # cur's buffer holds level 6, prev's level 5: swapped
    g.check("backward")
    got_prev, got_cur = g.prev.cpu().numpy(), g.cur.cpu().numpy()
    # level 5 of the way back is the start's level 0 and ends in the buffer that plays prev there, level 6 is level -1
    assert np.all(got_cur == np.array(ic)) and np.all(got_prev == np.array(ip))


def standing_wave(L, shape, dims, modes, r2):
    """taps centre 2 - 2 d r2, neighbours r2; u(0) = product of sines (zero halo); returns (taps, u0, cos w)"""
    d = len(dims)
    side = {1: 9, 2: 7, 3: 3}[d]  # the tap table: 9 taps, 7 x 7, 3 x 3 x 3
    w = np.zeros(L.ops.ntaps(shape))
    assert w.size == side ** d
    centre = w.size // 2
    for ax in range(d):  # the two neighbours along every axis
        w[centre - side ** ax] = w[centre + side ** ax] = r2
    w[centre] = 2.0 - 2.0 * d * r2
    assert support(L, shape)[w != 0].all()  # inside the shape's own support
    u0 = np.ones(dims)
    lam = 2.0 - 2.0 * d * r2
    for ax, (m, pm) in enumerate(zip(dims, modes)):
        s = np.sin(np.pi * pm * np.arange(1, m + 1) / (m + 1))
        u0 = u0 * s.reshape([-1 if k == ax else 1 for k in range(d)])
        lam += 2.0 * r2 * np.cos(np.pi * pm / (m + 1))
    return w, u0, lam / 2.0


@pytest.mark.parametrize("shape,dims,modes,r2", [("star2d1r", (70, 260), (3, 5), 0.25), ("1d1r", (1027,), (7,), 0.5),
                                                 ("star3d1r", (35, 17, 130), (2, 3, 5), 0.125)], ids=["2d", "1d", "3d"])
def test_standing_wave_against_the_closed_form(L, shape, dims, modes, r2):
    """zero halos, c = -1, u(-1) = cos(w) u(0): after T = 200 steps u(T) = cos(w T) u(0) to 1e-11.  The yardstick is the same
    recurrence in plain numpy on the CPU: 8.3e-14 for (70, 260) mode (3, 5), 3.9e-13 for mode (1, 1), 1.4e-13 for (1027,) mode 7;
    the bar leaves 25 x over the worst of those for the kernels' different summation order, and a wrong c, a swapped level or a
    wrong halo gives an error of order 1."""
    T = 200
    w, u0, cosw = standing_wave(L, shape, dims, modes, r2)
    assert abs(cosw) < 1.0
    ps = L.padded_shape(shape, dims)
    cur, prev = np.zeros(ps), np.zeros(ps)
    L.interior(shape, cur)[...] = u0
    L.interior(shape, prev)[...] = cosw * u0
    g = Grids(L, shape, dims, OFFSETS[0], prev, cur)
    p = L.Plan(shape, dims).set_weights(w)
    p.run_leapfrog(g.prev, g.cur, -1.0, T)
    g.check("standing wave")
    got = L.interior(shape, g.cur.cpu().numpy())
    err = float(np.abs(got - math.cos(math.acos(cosw) * T) * u0).max())
    print(shape, dims, modes, "max |u(T) - cos(w T) u(0)| =", err)
    assert err <= 1e-11


def test_host_entry_equals_the_plan_and_the_cli_runs(L):
    import torch

    shape, dims, times, c = "star2d1r", (64, 128), 7, -1.0
    rng = np.random.default_rng(11)
    ps = L.padded_shape(shape, dims)
    cur, prev = rng.integers(0, 100, ps).astype(np.float64), rng.integers(0, 100, ps).astype(np.float64)
    out, info = L.run_host_leapfrog(shape, cur, prev, c=c, times=times)
    assert info.steps_per_launch == 2 and info.hbm_gbs > 0
    p = L.Plan(shape, dims)
    d_prev, d_cur = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
    p.run_leapfrog(d_prev, d_cur, c, times)
    torch.cuda.synchronize()
    assert np.array_equal(out.view(np.int64), d_prev.cpu().numpy().view(np.int64))  # times is odd: level 7 is in prev
    out2, _ = L.run_host_leapfrog(shape, cur, prev, c=-0.5, times=4)
    d_prev, d_cur = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
    p.run_leapfrog(d_prev, d_cur, -0.5, 4)
    torch.cuda.synchronize()
    assert np.array_equal(out2.view(np.int64), d_cur.cpu().numpy().view(np.int64))

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_2d")
    r = subprocess.run([exe, "star2d1r", "64", "128", "7", "--leapfrog"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[0] == "INFO: shape = star_2d1r, m = 64, n = 128, times = 7"
    assert lines[1] == "LoRAStencil(2D star_2d1r): " and lines[2].startswith("Time = ") and lines[2].endswith("[ms]")
    assert lines[3].startswith("GStencil/s = ")
    assert any(ln.startswith("Leapfrog: u(t+1) = S(u(t)) + -1 u(t-1)") for ln in lines)
