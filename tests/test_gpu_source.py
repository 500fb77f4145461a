"""GPU tests of the source term (lora_plan_set_source; kernels_step.hip, kernels_2d_step2.hip): u <- S(u) + f.

Contract under test: out = fl(acc + f) on the interior cells of the swept range, acc the bits of the plan's plain single sweep;
halo cells of out never written, halo cells of f never used, f never written; two applications per launch (2D) equal two single
source sweeps bit for bit.

Memory: the two grids and f are THREE buffers carved by tests/arena.py out of one poisoned allocation, at offsets 16 and 240.
The whole padded view of f is NaN except its interior, so a halo cell of f that reached a result would show.  After every call
the guard bands are intact and f -- and, for the launch entries, the input -- is unchanged bit for bit.

Shapes, from the tile constants as built:
  single sweep   1D: 256 lanes x 2 points = 512 points per workgroup.  2D: 32 rows x 128 columns (kernels_step.hip: kRPT = 8,
                 kTileW = 128).  3D: 16 rows x 128 columns x chunks of 4 planes on grids this small (kRY = 4; the chunk rule
                 16 -> 7 -> 4 of launch_step3d).  Odd innermost extents: one thread per point, blocks of 4 rows x 64 columns.
  two per launch 2D: 4 R1 - 6 rows x 122 columns, R1 = 6 for the star (18 rows), 10 for diamond and box (34 rows)
                 (kernels_2d_step2.hip: launch_source2).
  one cell                      (1,)       (1, 2)       (1, 1, 2)
  partial tile + two tiles per direction, regions that begin and end inside a tile, the empty region
                                (1027,) = 2 x 512 + 3, with the odd tail point
                                (70, 260) = 2 x 32 + 6 rows, 2 x 128 + 4 columns; 3 x 18 + 16 and 2 x 34 + 2 rows, 2 x 122 + 16 columns
                                (35, 17, 130) = 8 x 4 + 3 planes, 16 + 1 rows, 128 + 2 columns
  odd innermost extent          (7, 13)    (3, 5, 7)
Tap sets: 2D diamond / star / box through star2d1r / star2d3r / box2d3r, 3D star / box (test_cases_reach_every_tap_set).
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
FUSED = [c for c in CASES if len(c[1]) == 2 and c[1][1] % 2 == 0]  # the plans that fuse two applications
FUSED_IDS = [IDS[CASES.index(c)] for c in FUSED]
RUNS = [CASES[i] for i in (1, 3, 4, 5, 6, 9, 10, 11)]
RUN_IDS = [IDS[CASES.index(c)] for c in RUNS]
TIMES = (0, 1, 2, 3, 4, 5, 7, 12)
SEVEN = [("1d1r", (1027,)), ("1d2r", (1027,)), ("star2d1r", (70, 260)), ("star2d3r", (70, 260)), ("box2d3r", (70, 260)),
         ("star3d1r", (35, 17, 130)), ("box3d1r", (35, 17, 130))]


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


def manufactured_taps(L, shape):
    """centre 0.25, every other tap of the support the largest power of two that keeps their sum <= 0.5: (taps, tap sum)"""
    on = support(L, shape)
    centre = on.size // 2
    others = int(on.sum()) - 1
    w = np.where(on, 2.0 ** math.floor(math.log2(0.5 / others)), 0.0)
    w[centre] = 0.25
    return w, float(w.sum())


@functools.lru_cache(maxsize=None)
def host_data(shape, dims):
    """per case, made once, read-only: seeded real data and integers 0..7 for the grid (whole padded array), real values and
    integers 0..1 for f (interior; its halo is NaN)"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr((shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    real = rng.standard_normal(ps) * 3.0
    ints = rng.integers(0, 8, ps).astype(np.float64)
    f_real = np.full(ps, np.nan)
    L.interior(shape, f_real)[...] = rng.standard_normal(dims) * 2.0
    f_ints = np.full(ps, np.nan)
    L.interior(shape, f_ints)[...] = rng.integers(0, 2, dims).astype(np.float64)
    for a in (real, ints, f_real, f_ints):
        a.setflags(write=False)
    return real, ints, f_real, f_ints


def bits_of(t):
    return t.view(__import__("torch").int64)


class Grids:
    """buffers 0 and 1 and f carved out of one poisoned allocation; f's halo is NaN"""

    def __init__(self, L, shape, dims, offset, u, f):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, dims
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=3, offset_bytes=offset)
        self.b0, self.b1, self.f = self.arena.views
        self.u = torch.from_numpy(np.ascontiguousarray(u)).cuda()
        self.set_f(f)
        self.reset()

    def set_f(self, f):
        import torch

        self.f.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        self.f_before = self.arena.bits(2).clone()

    def reset(self, second=0.0):
        self.b0.copy_(self.u)
        self.b1.fill_(second)

    def check(self, what, input_kept=False):
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        assert torch.equal(self.arena.bits(2), self.f_before), f"{what}: f was written"
        if input_kept:
            assert torch.equal(bits_of(self.b0), bits_of(self.u)), f"{what}: the input was written"


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


def plain_and_source(L, shape, dims, w, g, bc="reference", options=()):
    """a plan without a source and one with g.f, otherwise alike"""
    plans = []
    for src in (None, g.f):
        p = L.Plan(shape, dims).set_weights(w).set_boundary(bc)
        for k, v in options:
            p.set_option(k, v)
        if src is not None:
            p.set_source(src)
            assert p.get_option("source") == 1 and "src=1" in p.kernel_signature
        plans.append(p)
    return plans


def test_cases_reach_every_tap_set(L):
    seen = {2: set(), 3: set()}
    for shape, dims, _ in CASES:
        if len(dims) > 1:
            seen[len(dims)].add(L.Plan(shape, dims).set_weights(real_taps(L, shape)).get_option("tapset"))
    assert seen[2] == {0, 1, 2} and seen[3] == {0, 1}  # diamond, star, box; star, box


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_single_sweep_is_the_plain_sweep_plus_f(L, shape, dims, regions):
    """bit for bit on seeded real data: every cell of the output buffer, so the halo and the rows outside the region too"""
    import torch

    real, _, f_real, _ = host_data(shape, dims)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, real, f_real)
        plain, src = plain_and_source(L, shape, dims, real_taps(L, shape), g)
        assert src.get_option("fused_residual") == 0
        f_in = L.interior(shape, g.f)
        for begin, end in regions:
            g.reset(FILL)
            plain.step_region(g.b0, g.b1, begin, end)
            want = g.b1.clone()
            L.interior(shape, want)[begin:end] += f_in[begin:end]  # one fp64 addition per cell
            g.reset(FILL)
            src.step_region(g.b0, g.b1, begin, end)
            g.check(f"{shape} {dims} [{begin}, {end})", input_kept=True)
            assert same_bits(g.b1, want), (off, begin, end, int((bits_of(g.b1) != bits_of(want)).sum()))
            assert not torch.isnan(g.b1).any()
        # the whole-grid entry, and a zero source: the plain sweep as numbers
        g.reset(FILL)
        plain.step(g.b0, g.b1)
        want = g.b1.clone()
        g.set_f(np.where(np.isnan(f_real), np.nan, 0.0))
        g.reset(FILL)
        src.step(g.b0, g.b1)
        g.check("zero source", input_kept=True)
        assert torch.equal(g.b1, want)


@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_nonfinite_source_cells_change_exactly_those_cells(L, shape, dims, regions):
    import torch

    real, _, f_real, _ = host_data(shape, dims)
    g = Grids(L, shape, dims, OFFSETS[1], real, f_real)
    _, src = plain_and_source(L, shape, dims, real_taps(L, shape), g)
    g.reset(FILL)
    src.step(g.b0, g.b1)
    finite = g.b1.clone()
    f = f_real.copy()
    inner = L.interior(shape, f)
    n = inner.size
    cells = {pos: v for pos, v in zip(sorted({0, n // 2, n - 1}), (np.nan, np.inf, -np.inf))}
    for pos, v in cells.items():
        inner[np.unravel_index(pos, inner.shape)] = v
    g.set_f(f)
    g.reset(FILL)
    src.step(g.b0, g.b1)
    g.check("non-finite f", input_kept=True)
    got, was = L.interior(shape, g.b1).cpu().numpy(), L.interior(shape, finite).cpu().numpy()
    changed = np.flatnonzero(got.view(np.int64).ravel() != was.view(np.int64).ravel())
    assert set(changed) == set(cells), (changed, sorted(cells))
    for pos, v in cells.items():
        x = got.ravel()[pos]
        assert np.isnan(x) if np.isnan(v) else x == v
    halo_got, halo_was = g.b1.clone(), finite.clone()
    L.interior(shape, halo_got)[...] = 0
    L.interior(shape, halo_was)[...] = 0
    assert same_bits(halo_got, halo_was)


@pytest.mark.parametrize("bc", ["reference", "dirichlet"])
@pytest.mark.parametrize("shape,dims,regions", FUSED, ids=FUSED_IDS)
def test_two_application_launch_is_two_single_source_sweeps(L, shape, dims, regions, bc):
    """stepn_region(2) from an even level: the input carries the caller's halo, level 1 is a whole single source sweep into a
    buffer whose halo is 0 (reference) or the input's (Dirichlet), level 2 a single source sweep of the region; also with the
    structured evaluation forms requested or forbidden -- the source kernels evaluate direct taps whatever lowrank_valu says"""
    import torch

    real, _, f_real, _ = host_data(shape, dims)
    w = real_taps(L, shape)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, real, f_real)
        _, src = plain_and_source(L, shape, dims, w, g, bc)
        assert src.get_option("steps_per_launch") == 2 and src.kernel_name == "stencil2d_source2_kernel"
        mid = torch.zeros_like(g.u)
        if bc == "dirichlet":
            src.halo(mid, "copy", g.u)
        src.step(g.u, mid)
        for begin, end in regions:
            want = torch.full_like(g.u, FILL)
            src.step_region(mid, want, begin, end)
            for lowrank in (None, 0, 1, 4):
                q = src if lowrank is None else plain_and_source(L, shape, dims, w, g, bc, [("lowrank_valu", lowrank)])[1]
                g.reset(FILL)
                q.stepn_region(2, g.b0, g.b1, begin, end)
                g.check(f"{shape} {bc} two applications [{begin}, {end})", input_kept=True)
                assert same_bits(g.b1, want), (off, bc, begin, end, lowrank, int((bits_of(g.b1) != bits_of(want)).sum()))
        if (0, dims[0]) in regions:  # the other two-application entries are the same launch
            for call in (src.step2, src.stepk):
                g.reset(FILL)
                call(g.b0, g.b1)
                want = torch.full_like(g.u, FILL)
                src.step(mid, want)
                assert same_bits(g.b1, want)


def test_depths_a_source_plan_does_not_have_are_refused(L):
    import torch
    from lorastencil_amd import _lib

    for shape, dims, depths in [("1d1r", (64,), (2, 8)), ("star2d1r", (16, 24), (4, 6)), ("star2d1r", (7, 13), (2,)),
                                ("box3d1r", (6, 6, 8), (2, 3, 4))]:
        a = torch.zeros(L.padded_shape(shape, dims), dtype=torch.float64, device="cuda")
        b, f = torch.zeros_like(a), torch.zeros_like(a)
        p = L.Plan(shape, dims).set_source(f)
        for d in depths:
            with pytest.raises(L.LoraError) as e:
                p.stepn_region(d, a, b, 0, dims[0])
            assert e.value.status == _lib.LORA_EUNSUPPORTED, (shape, d)
        if p.get_option("steps_per_launch") == 1:
            with pytest.raises(L.LoraError) as e:
                p.step2(a, b)
            assert e.value.status == _lib.LORA_EUNSUPPORTED
        with pytest.raises(L.LoraError) as e:  # f is read while the output is written
            p.step(a, f)
        assert e.value.status == _lib.LORA_EINVAL
        with pytest.raises(L.LoraError) as e:
            p.residual(a)
        assert e.value.status == _lib.LORA_EUNSUPPORTED


def step_loop(p, g, times, bc):
    """the engine's own step-by-step loop of single sweeps from (b0, b1 = 0): the result buffer"""
    buf = (g.b0, g.b1)
    if bc == "dirichlet":
        p.halo(g.b1, "copy", g.b0)
    for i in range(times):
        if bc == "periodic":
            p.halo(buf[i % 2], "wrap")
        p.step(buf[i % 2], buf[(i + 1) % 2])
    if bc == "periodic" and times:
        p.halo(buf[times % 2], "wrap")
    return buf[times % 2]


def exact_sweeps(a, u_max, f_max):
    """How many sweeps with taps 2**-a of sum <= 1 stay exact in fp64 on non-negative integer data: level t is a multiple of
    2**(-a t) and at most u_max + t f_max (the tap sum is <= 1), every partial sum of a sweep likewise, so level t and
    everything on the way to it is exact while (u_max + t f_max) 2**(a t) <= 2**53"""
    t = 0
    while (u_max + (t + 1) * f_max) * 2.0 ** (a * (t + 1)) <= 2.0 ** 53:
        t += 1
    return t


@pytest.mark.parametrize("bc", ["reference", "dirichlet", "periodic"])
@pytest.mark.parametrize("shape,dims,regions", RUNS, ids=RUN_IDS)
def test_run_is_the_step_by_step_loop_and_the_oracle(L, shape, dims, regions, bc):
    """run(times) -- two-application launches in 2D, an odd number of them (7 sweeps: three) through the scratch grid -- against
    the engine's loop of single source sweeps on real data, and under the reference and Dirichlet boundaries against a host loop
    of oracle.step + f on integers 0..7 with f in 0..1 and taps 2**-a, as far as that loop is exact (exact_sweeps)"""
    import torch
    from oracle import oracle as O

    real, ints, f_real, f_ints = host_data(shape, dims)
    g = Grids(L, shape, dims, OFFSETS[0], real, f_real)
    _, p = plain_and_source(L, shape, dims, real_taps(L, shape), g, bc)
    fuses = len(dims) == 2 and dims[1] % 2 == 0 and bc != "periodic"
    assert p.get_option("steps_per_launch") == (2 if fuses else 1)
    for times in TIMES:
        g.reset()
        want = step_loop(p, g, times, bc).clone()
        g.reset()
        p.run(g.b0, g.b1, times)
        g.check(f"{shape} {bc} run({times})")
        got = (g.b0, g.b1)[times % 2]
        assert same_bits(got, want), (bc, times, int((bits_of(got) != bits_of(want)).sum()))
    if bc == "periodic":
        return
    w, a = equal_dyadic_taps(L, shape)
    horizon = exact_sweeps(a, 7, 1)
    assert horizon >= 7, (shape, a, horizon)  # the three-launch run is inside it for every shape
    g = Grids(L, shape, dims, OFFSETS[1], ints, f_ints)
    _, p = plain_and_source(L, shape, dims, w, g, bc)
    f_in = O.interior(shape, np.array(f_ints))
    checked = []
    for times in [t for t in TIMES if t <= horizon]:
        host = [np.array(ints), np.zeros_like(ints)]
        if bc == "dirichlet":
            host[1] = np.array(ints)  # both buffers carry the caller's halo; the interior is overwritten before it is read
        for i in range(times):
            O.step(shape, host[i % 2], w, out=host[(i + 1) % 2])
            O.interior(shape, host[(i + 1) % 2])[...] += f_in
        g.reset()
        p.run(g.b0, g.b1, times)
        g.check(f"{shape} {bc} integer run({times})")
        got = (g.b0, g.b1)[times % 2].cpu().numpy()
        want = host[times % 2]
        if bc == "dirichlet":  # what the untouched second buffer's halo holds after a run is the driver's business: interiors
            got, want = O.interior(shape, got), O.interior(shape, want)
        assert np.array_equal(got, want), (bc, times)
        checked.append(times)
    assert 7 in checked


@pytest.mark.parametrize("shape,dims", SEVEN, ids=[f"{s}-{'x'.join(map(str, d))}" for s, d in SEVEN])
def test_manufactured_solution(L, shape, dims):
    """u* = integers 0..99, f = u* - S(u*) on the interior, Dirichlet: u* is an exact fixed point (all values dyadic), and from
    a zero interior the iteration contracts to it: max|u - u*| <= residual / (1 - s) + 1e-11 (the contraction bound in the max
    norm; the last term covers rounding at values <= 100)"""
    import torch
    from oracle import oracle as O

    w, s = manufactured_taps(L, shape)
    assert s in (0.625, 0.75, 0.65625), s
    rng = np.random.default_rng(zlib.crc32(repr(("u*", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    ustar = rng.integers(0, 100, ps).astype(np.float64)
    f = np.full(ps, np.nan)
    O.interior(shape, f)[...] = O.interior(shape, ustar) - O.interior(shape, O.step(shape, ustar, w))
    g = Grids(L, shape, dims, OFFSETS[1], ustar, f)
    p = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_source(g.f)
    if len(dims) == 2:
        assert p.get_option("steps_per_launch") == 2
    g.reset()
    r = p.run_until(g.b0, g.b1, 0.0, check_every=2)
    g.check("run_until at u*")
    print(shape, dims, "at u*:", r)
    assert r.checks == 1 and r.times_done == 2 and r.converged and r.residual == 0.0
    assert same_bits(g.b0, g.u)
    start = ustar.copy()
    O.interior(shape, start)[...] = 0.0
    g.b0.copy_(torch.from_numpy(start))
    g.b1.zero_()
    r = p.run_until(g.b0, g.b1, 1e-9, check_every=2, max_times=400)
    g.check("run_until from zero")
    err = float((L.interior(shape, g.b0) - L.interior(shape, g.u)).abs().max())
    print(shape, dims, "from zero:", r.times_done, "sweeps, residual", r.residual, "max|u - u*|", err, "bound", r.residual / (1 - s) + 1e-11)
    assert r.converged and not r.diverged and r.times_done <= 400
    assert err <= r.residual / (1 - s) + 1e-11
    # A run of two sweeps is two single launches (one fused launch would leave the level in the wrong buffer), so the calls
    # above, as specified, never fuse.  The same iteration checked every FOUR sweeps runs two two-application launches per
    # check in 2D: same bound.
    g.b0.copy_(torch.from_numpy(start))
    g.b1.zero_()
    r4 = p.run_until(g.b0, g.b1, 1e-9, check_every=4, max_times=400)
    g.check("run_until from zero, every four sweeps")
    err4 = float((L.interior(shape, g.b0) - L.interior(shape, g.u)).abs().max())
    print(shape, dims, "every four:", r4.times_done, "sweeps, residual", r4.residual, "max|u - u*|", err4)
    assert r4.converged and err4 <= r4.residual / (1 - s) + 1e-11
    if len(dims) == 2:
        prof = p.run_profiled(g.b0, g.b1, 4)
        assert (prof.fused_launches, prof.apps_per_fused_launch, prof.single_launches) == (2, 2, 0)


def test_graph_replay_takes_the_new_source(L):
    import torch

    shape, dims, times = "star2d1r", (16, 24), 6
    real, _, f_real, _ = host_data(shape, dims)
    g = Grids(L, shape, dims, OFFSETS[0], real, f_real)
    f2 = torch.from_numpy(np.where(np.isnan(f_real), np.nan, f_real * 0.5 + 1.0)).cuda()
    p = L.Plan(shape, dims).set_weights(real_taps(L, shape)).set_option("graph", 1).set_source(g.f)
    stream = torch.cuda.Stream()
    results = []
    for src in (g.f, f2, g.f):
        p.set_source(src)
        g.reset()
        torch.cuda.synchronize()
        p.run(g.b0, g.b1, times, stream=stream)
        stream.synchronize()
        g.check("graph run")
        results.append((g.b0, g.b1)[times % 2].clone())
        q = L.Plan(shape, dims).set_weights(real_taps(L, shape)).set_option("graph", 0).set_source(src)
        g.reset()
        want = step_loop(q, g, times, "reference").clone()
        assert same_bits(results[-1], want)
    assert not same_bits(results[0], results[1]) and same_bits(results[0], results[2])


@pytest.mark.parametrize("shape,dims", [("star2d1r", (70, 260)), ("box3d1r", (35, 17, 130)), ("1d2r", (1027,))], ids=["2d", "3d", "1d"])
def test_plan_without_its_source_again_runs_like_a_fresh_plan(L, shape, dims):
    real, _, f_real, _ = host_data(shape, dims)
    g = Grids(L, shape, dims, OFFSETS[0], real, f_real)
    w = real_taps(L, shape)
    fresh = L.Plan(shape, dims).set_weights(w)
    used = L.Plan(shape, dims).set_weights(w).set_source(g.f)
    g.reset()
    used.run(g.b0, g.b1, 7)
    used.set_source(None)
    assert (used.kernel_signature, used.get_option("steps_per_launch"), used.get_option("fused_residual")) == (
        fresh.kernel_signature, fresh.get_option("steps_per_launch"), fresh.get_option("fused_residual"))
    for times in (7, 12):
        g.reset()
        fresh.run(g.b0, g.b1, times)
        want = (g.b0, g.b1)[times % 2].clone()
        g.reset()
        used.run(g.b0, g.b1, times)
        g.check("run without the source")
        assert same_bits((g.b0, g.b1)[times % 2], want)


@pytest.mark.parametrize("shape,dims,bc", [("star2d1r", (70, 260), "reference"), ("box3d1r", (12, 9, 16), "dirichlet"), ("1d2r", (300,), "reference")],
                         ids=["2d", "3d", "1d"])
def test_host_operators_with_a_source_equal_the_plan(L, shape, dims, bc):
    import torch
    from lorastencil_amd import _lib

    rng = np.random.default_rng(5)
    a = rng.integers(0, 100, L.padded_shape(shape, dims)).astype(np.float64)
    f = np.zeros_like(a)
    L.interior(shape, f)[...] = rng.standard_normal(dims)
    old_bc = _lib.lib().lora_set_default_boundary(L.ops.BOUNDARIES[bc])
    try:
        # (the host operators map params to taps; the plan side uses the same params)
        out, info = L.run_host(shape, a, times=5, source=f)
        until = L.run_host_until(shape, a, 1e300, check_every=4, max_times=8, source=f)
        p = L.Plan(shape, dims).set_source(torch.from_numpy(f).cuda())
    finally:
        _lib.lib().lora_set_default_boundary(old_bc)
        L.ops.set_default_source(None)
    assert p.get_option("boundary") == L.ops.BOUNDARIES[bc]
    b0 = torch.from_numpy(a).cuda()
    b1 = torch.zeros_like(b0)
    p.run(b0, b1, 5)
    want = (b0, b1)[1].cpu().numpy()
    n = want.size - 1 if len(dims) == 1 else want.size  # (the 1D operators copy all but the last element)
    assert np.array_equal(out.ravel()[:n], want.ravel()[:n])
    assert info.steps_per_launch == p.get_option("steps_per_launch")
    b0 = torch.from_numpy(a).cuda()
    b1 = torch.zeros_like(b0)
    r = p.run_until(b0, b1, 1e300, check_every=4, max_times=8)
    assert (until[1].times_done, until[1].checks, until[1].converged) == (r.times_done, r.checks, r.converged) == (4, 1, True)
    assert np.float64(until[1].residual).tobytes() == np.float64(r.residual).tobytes()
    assert np.array_equal(until[0].ravel()[:n], b0.cpu().numpy().ravel()[:n])


def test_cli_point_source_until_steady(L):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_2d")
    r = subprocess.run([exe, "star2d1r", "64", "64", "400", "--bc=dirichlet", "--normalize", "--source=point:1", "--until=1e-9"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert lines[0] == "INFO: shape = star_2d1r, m = 64, n = 64, times = 400"
    assert lines[1] == "LoRAStencil(2D star_2d1r): " and lines[2].startswith("Time = ") and lines[2].endswith("[ms]")
    assert lines[3].startswith("GStencil/s = ")
    assert any(ln.startswith("Source: f = 1 on the interior centre cell") for ln in lines)
    r = subprocess.run([exe, "star2d1r", "64", "64", "6", "--source=const:0.5", "--no-extra"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 4
