"""GPU tests of lora_plan_residual (kernels_residual.hip): one sweep's change, reduced inside the sweep.

Yardstick: the engine's older code -- ``plan.step_region`` into a second buffer followed by ``plan.diff`` -- and, for sum_sq,
numpy and ``math.fsum`` on host copies of the two grids.

Memory: the grid is ONE buffer carved by tests/arena.py (``n_buffers=1``: the call has no second buffer to hand over) at
offsets 16 and 240.  The whole padded view is filled with finite data, halo included -- the stencil reads it --; the guard
bands stay NaN.  After every call the guards must be intact and the grid's bits unchanged.

Shapes, from the constants as built (csrc/residual_tiles.h).  Tiles: 1D 512 points; 2D 32 rows x 128 columns; 3D fp64
32 planes x 16 rows x 128 columns; 3D bf16 32 x 16 x 256.  Workgroups: min(tiles, cap), cap 1024 (2D: 768); workgroup g walks
tiles g, g + G, ...  Per family, the smallest grids that reach each path:
  one cell                                  (1,)        (1, 2)       (1, 1, 2)       (1, 1, 8)   [rows are 16-byte pieces]
  a partial tile in each direction and two tiles per direction, regions that begin and end inside a tile, the empty one
                                            (1027,)     (70, 260)    (35, 17, 130)   (35, 17, 264)
      1027 = 2 x 512 + 3: the odd tail point, a third tile of three points
  more tiles than workgroups, so that some workgroup walks a second tile
                                            (2**19 + 515,): 1026 tiles     (801, 3970): 26 x 32 = 832 tiles, 25.7 MB
                                            (3, 16401, 2) and (3, 16401, 8): 1026 tiles of one or two rows' width
  the edges of the fp64 walk that the solvers' kernels share (csrc/tile_walk.h)
                                            (33, 130): one row and one column pair spill into second tiles
                                            (70, 258) with [5, 37): a region that begins and ends inside a tile
                                            (34, 18, 130), whole and with regions of 1, 2 and 3 planes: the last consume() falls
                                            in each of the three phases; with one plane the p >= 2 barrier is the only one reached
Tap sets: 2D diamond / star / box through star2d1r / star2d3r / box2d3r; 3D fp64 star / box; bf16 star, separable box and the
27-tap box (option separable = 0, and taps that do not factor) -- test_cases_reach_every_tap_set asserts it.
"""
import functools
import math
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
U = 2.0 ** -53

# (shape, dtype, dims, regions, taps): taps = "" the shape's own support, "sep0" bf16 with option separable = 0, "nosep" box
# taps that do not factor
CASES = [
    ("1d1r", "f64", (1,), [(0, 0)], ""),
    ("1d2r", "f64", (1027,), [(0, 0), (2, 515), (510, 1027), (4, 4)], ""),
    ("1d1r", "f64", (2**19 + 515,), [(0, 0)], ""),
    ("star2d1r", "f64", (1, 2), [(0, 0)], ""),
    ("star2d1r", "f64", (70, 260), [(0, 0), (5, 37), (33, 70), (7, 7)], ""),
    ("star2d3r", "f64", (70, 260), [(0, 0), (5, 37)], ""),
    ("box2d3r", "f64", (70, 260), [(0, 0), (33, 70)], ""),
    ("star2d1r", "f64", (801, 3970), [(0, 0)], ""),
    ("star3d1r", "f64", (1, 1, 2), [(0, 0)], ""),
    ("box3d1r", "f64", (35, 17, 130), [(0, 0), (1, 34), (33, 35), (9, 9)], ""),
    ("star3d1r", "f64", (35, 17, 130), [(0, 0), (1, 34)], ""),
    ("box3d1r", "f64", (3, 16401, 2), [(0, 0)], ""),
    ("box3d1r", "bf16", (1, 1, 8), [(0, 0)], ""),
    ("box3d1r", "bf16", (35, 17, 264), [(0, 0), (1, 34), (33, 35), (9, 9)], ""),
    ("star3d1r", "bf16", (35, 17, 264), [(0, 0), (1, 34)], ""),
    ("box3d1r", "bf16", (35, 17, 264), [(0, 0), (33, 35)], "sep0"),
    ("box3d1r", "bf16", (35, 17, 264), [(0, 0)], "nosep"),
    ("box3d1r", "bf16", (3, 16401, 8), [(0, 0)], ""),
    # the edges of the fp64 walk the solvers' kernels share (csrc/tile_walk.h); appended, so that the indices above stay
    ("star2d1r", "f64", (33, 130), [(0, 0)], ""),
    ("star2d3r", "f64", (33, 130), [(0, 0)], ""),
    ("box2d3r", "f64", (33, 130), [(0, 0)], ""),
    ("star2d1r", "f64", (70, 258), [(5, 37)], ""),
    ("star2d3r", "f64", (70, 258), [(5, 37)], ""),
    ("box2d3r", "f64", (70, 258), [(5, 37)], ""),
    ("box3d1r", "f64", (34, 18, 130), [(0, 0), (3, 4), (3, 5), (3, 6)], ""),
    ("star3d1r", "f64", (34, 18, 130), [(0, 0), (3, 4), (3, 5), (3, 6)], ""),
]
IDS = [f"{s}-{t}-{'x'.join(map(str, d))}{'-' + k if k else ''}" for s, t, d, _, k in CASES]
SEVERAL_TILES = [c for c in CASES if c[2] in ((1027,), (70, 260), (35, 17, 130), (35, 17, 264))]
SEVERAL_IDS = [IDS[CASES.index(c)] for c in SEVERAL_TILES]
TUNING = {1: [("steps_per_launch", 2)], 2: [("rows_per_thread", 4), ("rows_per_thread", 16), ("panel_width", 1), ("nt_store", 1)],
          3: [("z_chunk", 3), ("cols_per_lane", 8), ("lds_dma", 1), ("fused_z_chunk", 8)]}


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def integer_taps(L, shape, dtype, taps):
    """small integer taps on the support of the shape's own taps (so the plan resolves the same tap set); for the bf16 box
    an exact product a (x) b (x) c, one tap more for "nosep" """
    w = L.effective_weights(shape)[:L.ops.ntaps(shape)]
    ints = np.where(w != 0, 1.0 + np.arange(w.size) % 3, 0.0)
    if dtype == "bf16" and shape == "box3d1r":
        a, b, c = np.array([1.0, 2, 1]), np.array([2.0, 1, 1]), np.array([1.0, 1, 2])  # z, y, x
        ints = np.einsum("i,j,k->ijk", a, b, c).ravel()
        if taps == "nosep":
            ints[13] += 1
    return ints


def make_plan(L, shape, dtype, dims, taps, weights):
    p = L.Plan(shape, dims, dtype=dtype)
    if taps == "sep0":
        p.set_option("separable", 0)
    if weights == "int":
        p.set_weights(integer_taps(L, shape, dtype, taps))
    elif weights == "normalised":
        w = integer_taps(L, shape, dtype, taps)
        p.set_weights(w / w.sum())
    assert p.get_option("fused_residual") == 1
    return p


@functools.lru_cache(maxsize=None)
def host_data(shape, dtype, dims):
    """Whole padded arrays every test of a case starts from, made once: integers 0..99 and seeded normal values (as the dtype
    holds them); read-only."""
    import lorastencil_amd as L
    import torch

    rng = np.random.default_rng(zlib.crc32(repr((shape, dtype, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    ints = rng.integers(0, 100, ps).astype(np.float64)
    real = rng.standard_normal(ps) * 3.0
    if dtype == "bf16":
        real = torch.from_numpy(real).to(torch.bfloat16).double().numpy()
    for a in (ints, real):
        a.setflags(write=False)
    return ints, real


class Grid:
    """one carved grid holding `values` (whole padded array), a plain second buffer for the yardstick"""

    def __init__(self, L, shape, dtype, dims, offset, values):
        import torch
        from arena import carve

        self.L, self.shape = L, shape
        self.arena = carve(L.padded_shape(shape, dims), dtype, n_buffers=1, offset_bytes=offset)
        self.view = self.arena.views[0]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(self.view.dtype))
        self.before = self.arena.bits(0).clone()
        self.scratch = torch.zeros_like(self.view)

    def residual(self, p, begin=0, end=0):
        import torch
        from arena import assert_guards_intact

        got = p.residual(self.view, begin, end)
        torch.cuda.synchronize()
        assert_guards_intact(self.arena, f"{self.shape} [{begin}, {end})")
        assert torch.equal(self.arena.bits(0), self.before), "lora_plan_residual wrote into the grid"
        return got

    def two_pass(self, p, begin=0, end=0):
        """the yardstick: step_region into the second buffer, then diff"""
        lo, hi = (0, p.dims[0]) if (begin, end) == (0, 0) else (begin, end)
        self.scratch.zero_()
        p.step_region(self.view, self.scratch, lo, hi)
        return p.diff(self.scratch, self.view, begin, end)

    def host_d(self, p, begin=0, end=0):
        """d of the region from host copies of the two grids (after two_pass)"""
        lo, hi = (0, p.dims[0]) if (begin, end) == (0, 0) else (begin, end)
        a = self.L.interior(self.shape, self.scratch).double().cpu().numpy()[lo:hi]
        b = self.L.interior(self.shape, self.view).double().cpu().numpy()[lo:hi]
        with np.errstate(invalid="ignore"):
            return (a - b).ravel()


def bits(t):
    return tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in t)


def exact_fields(t):
    return bits((t.max_abs, t.a_abs_max, t.argmax, t.count, t.nonfinite))


def test_cases_reach_every_tap_set(L):
    seen = {}
    for shape, dtype, dims, _, taps in CASES:
        for weights in ("int", "normalised"):
            seen.setdefault((len(dims), dtype, weights), set()).add(make_plan(L, shape, dtype, dims, taps, weights).get_option("tapset"))
    for weights in ("int", "normalised"):
        assert seen[(2, "f64", weights)] == {0, 1, 2}  # diamond, star, box
        assert seen[(3, "f64", weights)] == {0, 1}     # star, box
    assert seen[(3, "bf16", "int")] == {0, 1, 2}       # star, box, separable
    assert {0, 1} <= seen[(3, "bf16", "normalised")]


def test_plans_without_the_kernel_are_refused_on_the_device(L):
    import torch
    from lorastencil_amd import _lib

    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    for p in [L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9)), mfma]:
        buf = torch.zeros(p.padded_shape, dtype=torch.float64, device="cuda")
        assert p.get_option("fused_residual") == 0
        with pytest.raises(L.LoraError) as e:
            p.residual(buf)
        assert e.value.status == _lib.LORA_EUNSUPPORTED
        # run_until still runs on them: the two-pass probe
        r = p.run_until(buf, torch.zeros_like(buf), 1e-9, check_every=2, max_times=2)
        assert r.checks == 1 and r.converged and r.last.count == p.dims[0] * p.dims[1] * (p.dims[2] if len(p.dims) == 3 else 1)


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", CASES, ids=IDS)
def test_integer_data_whole_record_is_the_two_pass_record(L, shape, dtype, dims, regions, taps):
    """integer data 0..99, small integer taps: every d is an integer and the sum of squares is below 2**53 (at most 27 or 49
    taps of at most 4, 3.2 M cells: < 1e15), so sum_sq is exact in any order"""
    ints, _ = host_data(shape, dtype, dims)
    p = make_plan(L, shape, dtype, dims, taps, "int")
    for off in OFFSETS:
        g = Grid(L, shape, dtype, dims, off, ints)
        for begin, end in regions:
            got, want = g.residual(p, begin, end), g.two_pass(p, begin, end)
            print(dims, (begin, end), got)
            assert bits(got) == bits(want), (off, begin, end, want)
            if begin == end != 0:
                assert got == L.GridDiff(0.0, 0.0, 0.0, -1, 0, 0)
            else:
                assert got.nonfinite == 0 and got.sum_sq < 2.0 ** 53 and got.max_abs > 0


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", CASES, ids=IDS)
def test_real_data_exact_fields_and_the_summation_bound(L, shape, dtype, dims, regions, taps):
    """The five exact fields are the two-pass record's.  sum_sq: a sum of n squares in fp64 in ANY order is within
    (n - 1) u of the exact sum of the rounded squares (relative; every term is positive), each square has one rounding more,
    and math.fsum is within 2 u of the exact sum: (n + 2) u, u = 2**-53 -- the bound derived in test_gpu_reduce.py, not
    measured."""
    _, real = host_data(shape, dtype, dims)
    p = make_plan(L, shape, dtype, dims, taps, "normalised")
    for off in OFFSETS:
        g = Grid(L, shape, dtype, dims, off, real)
        for begin, end in regions:
            got, want = g.residual(p, begin, end), g.two_pass(p, begin, end)
            d = g.host_d(p, begin, end)
            fs = math.fsum(d * d)
            print(dims, (begin, end), got, "two-pass sum_sq", want.sum_sq, "fsum", fs,
                  "error / bound", abs(got.sum_sq - fs) / max((d.size + 2) * U * fs, 1e-300))
            assert exact_fields(got) == exact_fields(want), (off, begin, end, want)
            assert got.count == d.size and got.nonfinite == 0
            assert abs(got.sum_sq - fs) <= (got.count + 2) * U * fs


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", SEVERAL_TILES, ids=SEVERAL_IDS)
def test_equal_maxima_in_different_tiles_take_the_lower_index(L, shape, dtype, dims, regions, taps):
    """two equal spikes on a zero field, one in the first tile and one in the last (other tile in every direction, other
    workgroup), each far enough from the edge to see its whole stencil: the same |d| around both"""
    import lorastencil_amd as LL

    r = {1: 4, 2: 3, 3: 1}[len(dims)]
    field = np.zeros(LL.padded_shape(shape, dims))
    inner = LL.interior(shape, field)
    inner[tuple(r for _ in dims)] = 8.0
    inner[tuple(n - 1 - r for n in dims)] = 8.0
    p = make_plan(L, shape, dtype, dims, taps, "int")
    index = LL.interior(shape, np.arange(field.size, dtype=np.int64).reshape(field.shape)).ravel()
    for off in OFFSETS:
        g = Grid(L, shape, dtype, dims, off, field)
        got, want = g.residual(p), g.two_pass(p)
        d = np.abs(g.host_d(p))
        at = index[d == d.max()]
        half = index[index.size // 2]
        print(dims, got, "cells at the maximum:", at)
        assert at.size >= 2 and at.min() < half < at.max()  # the maximum is reached around both spikes
        assert bits(got) == bits(want) and got.argmax == at.min() and got.max_abs == d.max() > 0


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", CASES, ids=IDS)
def test_nonfinite_data_gives_the_two_pass_record(L, shape, dtype, dims, regions, taps):
    """a NaN, a +inf and a -inf in the interior and a NaN in the halo cell left of the first interior cell, on integer data:
    every field, sum_sq included (integers), is the two-pass record's"""
    import lorastencil_amd as LL

    ints, _ = host_data(shape, dtype, dims)
    a = ints.copy()
    inner = LL.interior(shape, a)
    flat = inner.size
    for pos, v in zip(sorted({flat // 4, flat // 2, (3 * flat) // 4}), (np.nan, np.inf, -np.inf)):
        inner[np.unravel_index(pos, inner.shape)] = v
    h = LL.ops.halo(shape)
    a[tuple(h[:-1]) + (h[-1] - 1,)] = np.nan
    p = make_plan(L, shape, dtype, dims, taps, "int")
    for off in OFFSETS:
        g = Grid(L, shape, dtype, dims, off, a)
        for begin, end in regions:
            got, want = g.residual(p, begin, end), g.two_pass(p, begin, end)
            print(dims, (begin, end), got)
            assert bits(got) == bits(want), (off, begin, end, want)
        assert g.residual(p).nonfinite > 0


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", SEVERAL_TILES + [CASES[7]], ids=SEVERAL_IDS + [IDS[7]])
def test_same_call_same_bits_whatever_the_tuning_options(L, shape, dtype, dims, regions, taps):
    _, real = host_data(shape, dtype, dims)
    p = make_plan(L, shape, dtype, dims, taps, "normalised")
    g = Grid(L, shape, dtype, dims, OFFSETS[1], real)
    first = [g.residual(p, b, e) for b, e in regions]
    assert [bits(g.residual(p, b, e)) for b, e in regions] == [bits(x) for x in first]
    for key, value in TUNING[len(dims)]:
        q = make_plan(L, shape, dtype, dims, taps, "normalised").set_option(key, value)
        assert q.get_option(key) == value and q.get_option("tapset") == p.get_option("tapset")
        assert [bits(g.residual(q, b, e)) for b, e in regions] == [bits(x) for x in first], (key, value)


# ---- run_until: the probe is the fused residual under the max norm, the two passes under the RMS norm ------------------
def taps_2d():
    w = np.zeros(49)
    w[[24, 23, 25, 17, 31]] = 0.2  # the centre and its four neighbours
    return w


UNTIL = [("star2d1r", "f64", (16, 24), "dirichlet", 4, 1e-9), ("star2d1r", "f64", (16, 24), "periodic", 1, 1e-9),
         ("box3d1r", "bf16", (12, 16, 24), "dirichlet", 2, 0.0)]


@pytest.mark.parametrize("shape,dtype,dims,bc,seed,tol", UNTIL, ids=["2d-dirichlet", "2d-periodic", "3d-bf16"])
def test_run_until_probes_with_the_fused_residual(L, shape, dtype, dims, bc, seed, tol):
    """the inputs of test_gpu_run_until.py"""
    import torch

    a = L.reference_input(shape, dims, rng=L.GlibcRand(seed))
    if shape == "star2d1r":
        w = taps_2d()
    else:
        w = L.effective_weights(shape)
        w = w / w.sum()
    p = L.Plan(shape, dims, dtype=dtype).set_boundary(bc).set_weights(w)
    assert p.get_option("fused_residual") == 1
    check_every, max_times = 50, 6000

    def pair():
        b0 = torch.from_numpy(a).to(torch.bfloat16 if dtype == "bf16" else torch.float64).cuda()
        return b0, torch.zeros_like(b0)

    def by_hand(norm):
        """run(check_every), step, diff through the public calls: the loop as it was before the fused probe"""
        b0, b1 = pair()
        T, residual, conv, div, last = 0, math.inf, 0, 0, None
        while T + check_every <= max_times:
            p.run(b0, b1, check_every)
            T += check_every
            if bc == "periodic":
                p.halo(b0, "wrap")
            p.step(b0, b1)
            last = p.diff(b1, b0)
            residual = math.sqrt(last.sum_sq / last.count) if norm == "rms" else last.max_abs
            if last.nonfinite > 0:
                div = 1
                break
            if residual <= tol:
                conv = 1
                break
        return T, residual, conv, div, last

    for norm in ("max", "rms"):
        b0, b1 = pair()
        r = p.run_until(b0, b1, tol, norm=norm, check_every=check_every, max_times=max_times)
        torch.cuda.synchronize()
        T, residual, conv, div, last = by_hand(norm)
        print(shape, bc, norm, r, "by hand:", T, residual, conv, div)
        assert (r.times_done, r.converged, r.diverged, r.checks) == (T, conv, div, T // check_every)
        assert np.float64(r.residual).tobytes() == np.float64(residual).tobytes()
        assert exact_fields(r.last) == exact_fields(last)
        if norm == "max":
            assert bits(r.last) == bits(p.residual(b0))  # d_buf0 is level times_done, its halo as the probe saw it
        else:
            s = torch.zeros_like(b0)
            p.step(b0, s)
            assert bits(r.last) == bits(p.diff(s, b0)) == bits(last)
