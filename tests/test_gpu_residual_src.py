"""GPU tests of lora_plan_residual_src (kernels_residual.hip with a source operand): the true residual S(u) + f - u in one pass.

Yardstick: a second plan with the same weights that carries f as its source -- ``set_source(f)`` + ``step_region`` into a spare
grid, then ``diff`` -- and, for sum_sq, ``math.fsum`` on host copies of the two grids.

Cases, tap helpers and the tuning table are those of tests/test_gpu_residual.py (its fp64 cases: the smallest grids that reach
each path of these kernels; that file's docstring derives them).

Memory: the grid and f are TWO buffers carved by tests/arena.py at offsets 16 and 240, guard bands NaN.  The grid's whole
padded view holds finite data; the HALO CELLS OF f HOLD NaN, so a kernel that reads one into a result shows up as
nonfinite > 0 or a NaN field.  After every call the guards must be intact and the bits of both buffers unchanged.
"""
import functools
import math
import zlib

import numpy as np
import pytest

import test_gpu_leapfrog_src as lf
import test_gpu_residual as base
from test_gpu_residual import OFFSETS, TUNING, U, bits, exact_fields, host_data, make_plan

pytestmark = pytest.mark.gpu

CASES = [c for c in base.CASES if c[1] == "f64"]
IDS = [base.IDS[base.CASES.index(c)] for c in CASES]
SEVERAL = [c for c in CASES if c[2] in ((1027,), (70, 260), (35, 17, 130))]
SEVERAL_IDS = [base.IDS[base.CASES.index(c)] for c in SEVERAL]
TILE = {1: (512,), 2: (32, 128), 3: (32, 16, 128)}  # csrc/residual_tiles.h


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


@functools.lru_cache(maxsize=None)
def source_data(shape, dims):
    """padded f, made once per case, read-only: integers in [-8, 8] and seeded normal values on the interior, NaN in every
    halo cell"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("residual_src", shape, dims)).encode()))
    out = []
    for interior in (rng.integers(-8, 9, dims).astype(np.float64), rng.standard_normal(dims) * 1.5):
        f = np.full(L.padded_shape(shape, dims), np.nan)
        L.interior(shape, f)[...] = interior
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


class Pair:
    """the grid and f carved out of one poisoned allocation; a plain spare grid for the yardstick"""

    def __init__(self, L, shape, dims, offset, values, f):
        import torch
        from arena import carve

        self.L, self.shape = L, shape
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=2, offset_bytes=offset)
        self.view, self.f = self.arena.views
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values)))
        self.f.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        self.before = [self.arena.bits(i).clone() for i in (0, 1)]
        self.spare = torch.zeros_like(self.view)

    def check(self, what):
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i in (0, 1):
            assert torch.equal(self.arena.bits(i), self.before[i]), f"{what}: buffer {i} was written"

    def residual_src(self, p, begin=0, end=0, f=True):
        got = p.residual_src(self.view, self.f if f else None, begin, end)
        self.check(f"{self.shape} residual_src [{begin}, {end})")
        return got

    def two_pass(self, q, begin=0, end=0):
        """the yardstick: q carries self.f as its source; one sweep into the spare grid, then diff"""
        lo, hi = (0, q.dims[0]) if (begin, end) == (0, 0) else (begin, end)
        self.spare.zero_()
        if hi > lo:
            q.step_region(self.view, self.spare, lo, hi)
        got = q.diff(self.spare, self.view, begin, end)
        self.check("two-pass")
        return got

    def host_d(self, q, begin=0, end=0):
        """d of the region from host copies of the two grids (after two_pass)"""
        lo, hi = (0, q.dims[0]) if (begin, end) == (0, 0) else (begin, end)
        a = self.L.interior(self.shape, self.spare).cpu().numpy()[lo:hi]
        b = self.L.interior(self.shape, self.view).cpu().numpy()[lo:hi]
        with np.errstate(invalid="ignore"):
            return (a - b).ravel()


def plans(L, shape, dims, weights, g):
    """the plan under test (no source) and the yardstick's (the same weights, g.f as its source)"""
    p = make_plan(L, shape, "f64", dims, "", weights)
    q = make_plan(L, shape, "f64", dims, "", weights).set_source(g.f)
    assert p.get_option("source") == 0 and q.get_option("source") == 1
    return p, q


def test_cases_reach_every_tap_set(L):
    seen = {}
    for shape, _, dims, _, taps in CASES:
        for weights in ("int", "normalised"):
            seen.setdefault((len(dims), weights), set()).add(make_plan(L, shape, "f64", dims, taps, weights).get_option("tapset"))
    for weights in ("int", "normalised"):
        assert seen[(2, weights)] == {0, 1, 2}  # diamond, star, box
        assert seen[(3, weights)] == {0, 1}     # star, box


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", CASES, ids=IDS)
def test_integer_data_whole_record_is_the_two_pass_record(L, shape, dtype, dims, regions, taps):
    """integer data 0..99, small integer taps, integer f in [-8, 8]: every d is an integer and the sum of squares is below 2**53
    (as in test_gpu_residual.py; f adds at most 8 to |d| < 2e4), so sum_sq is exact in any order"""
    ints, _ = host_data(shape, dtype, dims)
    f_int, _ = source_data(shape, dims)
    for off in OFFSETS:
        g = Pair(L, shape, dims, off, ints, f_int)
        p, q = plans(L, shape, dims, "int", g)
        for begin, end in regions:
            got, want = g.residual_src(p, begin, end), g.two_pass(q, begin, end)
            print(dims, (begin, end), got)
            assert bits(got) == bits(want), (off, begin, end, want)
            if begin == end != 0:
                assert got == L.GridDiff(0.0, 0.0, 0.0, -1, 0, 0)
            else:
                assert got.nonfinite == 0 and got.sum_sq < 2.0 ** 53 and got.max_abs > 0


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", SEVERAL, ids=SEVERAL_IDS)
def test_real_data_exact_fields_summation_bound_and_same_bits(L, shape, dtype, dims, regions, taps):
    """The five exact fields are the two-pass record's; sum_sq within (count + 2) u of math.fsum (the bound derived in
    test_gpu_reduce.py, not measured); the same call gives the same six fields, also after each tuning option is set."""
    _, real = host_data(shape, dtype, dims)
    _, f_real = source_data(shape, dims)
    for off in OFFSETS:
        g = Pair(L, shape, dims, off, real, f_real)
        p, q = plans(L, shape, dims, "normalised", g)
        first = []
        for begin, end in regions:
            got, want = g.residual_src(p, begin, end), g.two_pass(q, begin, end)
            d = g.host_d(q, begin, end)
            fs = math.fsum(d * d)
            print(dims, (begin, end), got, "two-pass sum_sq", want.sum_sq, "fsum", fs,
                  "error / bound", abs(got.sum_sq - fs) / max((d.size + 2) * U * fs, 1e-300))
            assert exact_fields(got) == exact_fields(want), (off, begin, end, want)
            assert got.count == d.size and got.nonfinite == 0
            assert abs(got.sum_sq - fs) <= (got.count + 2) * U * fs
            first.append(got)
        assert [bits(g.residual_src(p, b, e)) for b, e in regions] == [bits(x) for x in first]
        if off == OFFSETS[1]:
            for key, value in TUNING[len(dims)]:
                t = make_plan(L, shape, "f64", dims, "", "normalised").set_option(key, value)
                assert t.get_option(key) == value and t.get_option("tapset") == p.get_option("tapset")
                assert [bits(g.residual_src(t, b, e)) for b, e in regions] == [bits(x) for x in first], (key, value)


@pytest.mark.parametrize("shape,dtype,dims,regions,taps", CASES, ids=IDS)
def test_no_source_is_the_plain_residual(L, shape, dtype, dims, regions, taps):
    """d_f = None: all six fields of lora_plan_residual bit for bit; f of all zeros: the same record as numbers"""
    _, real = host_data(shape, dtype, dims)
    g = Pair(L, shape, dims, OFFSETS[1], real, np.zeros(L.padded_shape(shape, dims)))
    p = make_plan(L, shape, "f64", dims, "", "normalised")
    for begin, end in regions:
        plain = p.residual(g.view, begin, end)
        assert bits(g.residual_src(p, begin, end, f=False)) == bits(plain), (begin, end)
        assert g.residual_src(p, begin, end) == plain, (begin, end)


def test_no_source_is_the_plain_residual_on_bf16(L):
    shape, dims = "box3d1r", (35, 17, 264)
    _, real = host_data(shape, "bf16", dims)
    g = base.Grid(L, shape, "bf16", dims, OFFSETS[1], real)
    p = make_plan(L, shape, "bf16", dims, "", "normalised")
    for begin, end in [(0, 0), (1, 34), (9, 9)]:
        assert bits(p.residual_src(g.view, None, begin, end)) == bits(g.residual(p, begin, end))


@pytest.mark.parametrize("where", ["f", "grid", "both"])
@pytest.mark.parametrize("shape,dtype,dims,regions,taps", SEVERAL, ids=SEVERAL_IDS)
def test_nonfinite_operands_give_the_two_pass_record(L, shape, dtype, dims, regions, taps, where):
    """+inf, -inf and NaN in a tile's first cell, its last cell and a cell of the second tile, in f, in the grid or in both, on
    real data: the five exact fields are the two-pass record's and nonfinite counts the cells whose difference is not finite"""
    import lorastencil_amd as LL

    _, real = host_data(shape, dtype, dims)
    _, f_real = source_data(shape, dims)
    ext = TILE[len(dims)]
    last = tuple(min(e, n) - 1 for e, n in zip(ext, dims))
    second = tuple(0 for _ in dims[:-1]) + (ext[-1],)
    assert dims[-1] > ext[-1]
    cells = [tuple(0 for _ in dims), last, second]
    a, f = real.copy(), f_real.copy()
    for arr, on in ((f, where in ("f", "both")), (a, where in ("grid", "both"))):
        if on:
            for cell, v in zip(cells, (np.inf, -np.inf, np.nan)):
                LL.interior(shape, arr)[cell] = v
    for off in OFFSETS:
        g = Pair(L, shape, dims, off, a, f)
        p, q = plans(L, shape, dims, "normalised", g)
        for begin, end in regions:
            got, want = g.residual_src(p, begin, end), g.two_pass(q, begin, end)
            d = g.host_d(q, begin, end)
            print(dims, where, (begin, end), got)
            assert exact_fields(got) == exact_fields(want), (off, begin, end, want)
            assert got.nonfinite == np.count_nonzero(~np.isfinite(d)) and got.count == d.size
            assert math.isfinite(got.sum_sq) and math.isfinite(got.max_abs) and math.isfinite(got.a_abs_max)
        assert g.residual_src(p).nonfinite >= 3


def test_plans_that_take_no_source_operand_are_refused_on_the_device(L):
    import torch
    from lorastencil_amd import _lib

    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    sourced = L.Plan("star2d1r", (32, 64))
    for p in [L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9)), mfma, bf, sourced]:
        buf = torch.zeros(p.padded_shape, dtype=torch.bfloat16 if p is bf else torch.float64, device="cuda")
        f = torch.zeros(p.padded_shape, dtype=torch.float64, device="cuda")
        if p is sourced:
            p.set_source(torch.zeros_like(f))
        with pytest.raises(L.LoraError) as e:
            p.residual_src(buf, f)
        assert e.value.status == _lib.LORA_EUNSUPPORTED


def test_the_chebyshev_driver_probes_with_the_fused_residual(L):
    """the problem of test_run_chebyshev_until_converges_where_run_until_does_not (tests/test_gpu_leapfrog_src.py)"""
    shape, dims = "star2d1r", (62, 64)
    w, f, rho = lf.jacobi_problem(L, shape, dims)
    zero = np.zeros_like(f)
    g = lf.Grids(L, shape, dims, OFFSETS[1], zero, zero, f, n_buffers=5)
    p = L.Plan(shape, dims).set_weights(w)
    keys = ["fused_residual", "source", "steps_per_launch", "variant", "tapset", "boundary", "scratch"]
    state = lambda: (p.kernel_signature, p.kernel_name, p.leapfrog_depth, [p.get_option(k) for k in keys])  # noqa: E731
    before = state()
    assert p.get_option("fused_residual") == 1
    q = L.Plan(shape, dims).set_weights(w).set_source(g.f)

    def two_pass():
        q.step(g.cur, g.spare[0])
        return q.diff(g.spare[0], g.cur)

    r = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-10, rtol=0.0, norm="max", check_every=20, max_times=600)
    g.check("run_chebyshev_until, max norm")
    print("max norm:", r)
    assert r.converged and not r.diverged and r.times_done % 20 == 0 and 0 < r.times_done <= 600
    assert r.checks == r.times_done // 20 and r.residual == r.last.max_abs <= 1e-10
    for s in g.spare:
        assert bool((s == lf.FILL).all()), "the probe touched a grid that is not its own"
    assert bits(r.last) == bits(p.residual_src(g.cur, g.f))
    assert exact_fields(r.last) == exact_fields(two_pass())
    got_prev, got_cur = g.prev.clone(), g.cur.clone()
    a, c = L.chebyshev_coeffs(rho, 1, r.times_done)
    g.reset()
    p.run_leapfrog_src(g.prev, g.cur, g.f, a, c, r.times_done)
    g.check("run_leapfrog_src(times_done)")
    assert lf.same_bits(g.cur, got_cur) and lf.same_bits(g.prev, got_prev)
    assert state() == before

    # the RMS norm keeps the two passes: all six fields
    g.reset()
    rr = p.run_chebyshev_until(g.prev, g.cur, g.f, rho, tol=1e-10, rtol=0.0, norm="rms", check_every=20, max_times=600)
    g.check("run_chebyshev_until, rms norm")
    print("rms norm:", rr)
    assert rr.converged and bits(rr.last) == bits(two_pass())
    assert state() == before

    # no source, a non-zero first level: the plain fused residual
    u0 = np.zeros_like(f)
    L.interior(shape, u0)[...] = L.interior(shape, f) * 4.0
    g0 = lf.Grids(L, shape, dims, OFFSETS[0], zero, u0, f, n_buffers=4)
    r0 = p.run_chebyshev_until(g0.prev, g0.cur, None, rho, tol=1e-10, rtol=0.0, norm="max", check_every=20, max_times=600)
    g0.check("run_chebyshev_until, no source")
    print("no source:", r0)
    assert r0.checks >= 1 and r0.last.max_abs > 0 and bits(r0.last) == bits(p.residual(g0.cur))
    assert state() == before

    # a plan without the kernel: the two passes, all six fields
    dims1 = (62, 63)
    w1, f1, rho1 = lf.jacobi_problem(L, shape, dims1)
    z1 = np.zeros_like(f1)
    g1 = lf.Grids(L, shape, dims1, OFFSETS[1], z1, z1, f1, n_buffers=5)
    p1 = L.Plan(shape, dims1).set_weights(w1)
    assert p1.get_option("fused_residual") == 0
    sig1 = (p1.kernel_signature, p1.leapfrog_depth)
    r1 = p1.run_chebyshev_until(g1.prev, g1.cur, g1.f, rho1, tol=1e-10, rtol=0.0, norm="max", check_every=20, max_times=600)
    g1.check("run_chebyshev_until, no kernel")
    print("no kernel:", r1)
    q1 = L.Plan(shape, dims1).set_weights(w1).set_source(g1.f)
    q1.step(g1.cur, g1.spare[0])
    assert r1.converged and bits(r1.last) == bits(q1.diff(g1.spare[0], g1.cur))
    assert (p1.kernel_signature, p1.leapfrog_depth) == sig1
