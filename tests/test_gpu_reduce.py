"""GPU tests of the device-side reductions (lora_plan_stats / lora_plan_diff; kernels_reduce.hip) against numpy on the host
copy of the same grids.

The grids are carved by tests/arena.py at offsets 16 and 240: every halo cell and every byte around a grid is a NaN, so a halo
or guard value that reached a result would show as a NaN or as a non-zero `nonfinite`.

Shapes: the smallest that reach every path of the kernel -- one cell, rows of one piece, odd rows (8-byte pieces), rows that
are no multiple of the lanes' stride, and per family one grid that spans several workgroups of the kernel as built (2048
pieces per workgroup at these sizes, reduce.cpp: reduce_geometry): 1D 2**17 + 3 -> 65538 pieces, 33 workgroups; 2D
(257, 1030) -> 132355 pieces, 65; (64, 1031), 8-byte pieces -> 65984, 33; 3D fp64 (20, 33, 72) -> 23760, 12; 3D bf16
(20, 33, 72) -> 6600 pieces of 8 cells, 4 workgroups of 1792.
"""
import functools
import math
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = (
    [("1d1r", "f64", (n,)) for n in (1, 9, 4099, 2**17 + 3)]
    + [("star2d1r", "f64", d) for d in ((1, 1), (5, 7), (33, 130), (257, 1030), (64, 1031))]
    + [("box3d1r", "f64", d) for d in ((1, 1, 2), (3, 5, 9), (9, 17, 40), (20, 33, 72))]
    + [("box3d1r", "bf16", d) for d in ((1, 1, 8), (3, 5, 16), (20, 33, 72))]
)
IDS = [f"{s}-{t}-{'x'.join(map(str, d))}" for s, t, d in CASES]
OFFSETS = (16, 240)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


@functools.lru_cache(maxsize=None)
def plan_of(shape, dtype, dims):
    import lorastencil_amd as L

    return L.Plan(shape, dims, dtype=dtype)


@functools.lru_cache(maxsize=None)
def host_data(shape, dtype, dims):
    """The interiors every test of a case starts from, made once: integers 0..99 and seeded normal values (as the dtype
    holds them), and the padded linear index of every interior cell."""
    import lorastencil_amd as L
    import torch

    rng = np.random.default_rng(zlib.crc32(repr((shape, dtype, dims)).encode()))
    ints = rng.integers(0, 100, dims).astype(np.float64)
    real = rng.standard_normal(dims) * 3.0
    if dtype == "bf16":
        real = torch.from_numpy(real).to(torch.bfloat16).double().numpy()
    ps = L.padded_shape(shape, dims)
    index = L.interior(shape, np.arange(int(np.prod(ps)), dtype=np.int64).reshape(ps)).copy()
    for a in (ints, real, index):
        a.setflags(write=False)
    return ints, real, index


def arenas(L, shape, dtype, dims):
    from arena import carve

    return [carve(L.padded_shape(shape, dims), dtype, n_buffers=2, offset_bytes=off) for off in OFFSETS]


def put(L, shape, view, values):
    """interior of a carved grid <- values; its halo keeps the poison"""
    import torch

    L.interior(shape, view).copy_(torch.from_numpy(np.array(values, dtype=np.float64, order="C")).to(view.dtype))


def host(L, shape, view):
    return L.interior(shape, view).double().cpu().numpy()


def np_stats(L, x):
    x = np.asarray(x, dtype=np.float64).ravel()
    f = x[np.isfinite(x)]
    if f.size == 0:
        return L.GridStats(math.inf, -math.inf, 0.0, 0.0, 0.0, x.size, x.size)
    return L.GridStats(f.min(), f.max(), np.abs(f).max(), f.sum(), (f * f).sum(), x.size, x.size - f.size)


def np_diff(L, a, b, index):
    """lora_plan_diff by numpy: float64 subtraction, the lowest padded index among the equal maxima"""
    with np.errstate(invalid="ignore"):
        d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    ok = np.isfinite(d)
    if not ok.any():
        return L.GridDiff(0.0, 0.0, 0.0, -1, d.size, d.size)
    ad = np.abs(d[ok])
    return L.GridDiff(ad.max(), (d[ok] * d[ok]).sum(), np.abs(np.asarray(a)[ok]).max(), int(index[ok][ad == ad.max()].min()), d.size,
                      int(d.size - ok.sum()))


def bits(t):
    return tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in t)


@pytest.mark.parametrize("shape,dtype,dims", CASES, ids=IDS)
def test_exact_data_is_bit_for_bit_numpy(L, shape, dtype, dims):
    from arena import assert_guards_intact

    ints, _, index = host_data(shape, dtype, dims)
    p = plan_of(shape, dtype, dims)
    want = np_stats(L, ints)  # integer sums below 2**53: exact in any order
    for ar in arenas(L, shape, dtype, dims):
        put(L, shape, ar.views[0], ints)
        put(L, shape, ar.views[1], ints)
        got = p.stats(ar.views[0])
        print(dims, got)
        assert bits(got) == bits(want)
        assert got.nonfinite == 0 and got.count == ints.size  # no halo or guard value reached the result
        same = p.diff(ar.views[0], ar.views[1])
        print(dims, same)
        assert bits(same) == bits(L.GridDiff(0.0, 0.0, ints.max(), int(index.ravel()[0]), ints.size, 0))
        assert_guards_intact(ar, f"{shape} {dims}")


@pytest.mark.parametrize("shape,dtype,dims", CASES, ids=IDS)
def test_real_data_within_the_summation_bound(L, shape, dtype, dims):
    """min / max / abs_max are exact; a sum of n terms in fp64 in ANY order is within (n - 1) u sum|x_i| of the exact one
    (u = 2**-53, first order; every partial sum is bounded by sum|x_i|), sum_sq has one more rounding per square; math.fsum of
    the rounded squares is itself within 2 u of the exact sum.  (n + 2) u covers all of it and is derived, not measured."""
    _, real, _ = host_data(shape, dtype, dims)
    p = plan_of(shape, dtype, dims)
    x = real.ravel()
    n = x.size
    for ar in arenas(L, shape, dtype, dims):
        put(L, shape, ar.views[0], real)
        assert np.array_equal(host(L, shape, ar.views[0]), real)
        got = p.stats(ar.views[0])
        print(dims, got, math.fsum(x), math.fsum(x * x))
        assert (got.min, got.max, got.abs_max) == (x.min(), x.max(), np.abs(x).max())
        assert (got.count, got.nonfinite) == (n, 0)
        assert abs(got.sum - math.fsum(x)) <= (n + 2) * U * math.fsum(np.abs(x))
        assert abs(got.sum_sq - math.fsum(x * x)) <= (n + 2) * U * math.fsum(x * x)
        # the same call returns the same bits every time
        again = [p.stats(ar.views[0]) for _ in range(5)]
        assert all(bits(a) == bits(got) for a in again)
        put(L, shape, ar.views[1], real[::-1] if real.ndim == 1 else np.flip(real, axis=-1))
        first = p.diff(ar.views[0], ar.views[1])
        assert all(bits(p.diff(ar.views[0], ar.views[1])) == bits(first) for _ in range(5))


@pytest.mark.parametrize("shape,dtype,dims", CASES, ids=IDS)
def test_regions_merge_to_the_whole(L, shape, dtype, dims):
    ints, _, index = host_data(shape, dtype, dims)
    p = plan_of(shape, dtype, dims)
    d0 = dims[0]
    cut_sets = [sorted({c for c in cs if 0 < c < d0}) for cs in ((1, d0 - 1), (d0 // 2,), (1, d0 // 2, d0 - 1))]
    ar = arenas(L, shape, dtype, dims)[1]
    put(L, shape, ar.views[0], ints)
    whole = p.stats(ar.views[0])
    assert bits(whole) == bits(p.stats(ar.views[0], 0, d0)) == bits(np_stats(L, ints))
    for cuts in cut_sets:
        edges = [0] + cuts + [d0]
        parts = [p.stats(ar.views[0], b, e) for b, e in zip(edges[:-1], edges[1:])]
        for (b, e), part in zip(zip(edges[:-1], edges[1:]), parts):
            assert bits(part) == bits(np_stats(L, ints[b:e])), (b, e)
        assert bits(L.stats_merge(*parts)) == bits(whole), cuts
    assert bits(p.stats(ar.views[0], d0, d0)) == bits(L.EMPTY_STATS)  # an empty range: no launch, the empty record
    if d0 < 2:
        return
    # diff on a piece sees only that piece: differences planted in the first and the last row (plane, point)
    b = ints.copy()
    b[0] = b[0] + 5.0
    b[d0 - 1] = b[d0 - 1] - 7.0
    put(L, shape, ar.views[1], b)
    for lo, hi in [(0, 1), (d0 - 1, d0)] + ([(1, d0 - 1)] if d0 >= 3 else []):
        got = p.diff(ar.views[0], ar.views[1], lo, hi)
        assert bits(got) == bits(np_diff(L, ints[lo:hi], b[lo:hi], index[lo:hi])), (lo, hi)
        assert got.max_abs == (5.0 if lo == 0 else 7.0 if hi == d0 else 0.0)
    assert p.diff(ar.views[0], ar.views[1]).max_abs == 7.0


@pytest.mark.parametrize("shape,dtype,dims", CASES, ids=IDS)
def test_diff_finds_planted_differences(L, shape, dtype, dims):
    from arena import assert_guards_intact

    ints, _, index = host_data(shape, dtype, dims)
    p = plan_of(shape, dtype, dims)
    n = ints.size
    b = ints.copy()
    flat = b.reshape(-1)  # (a view: dims is contiguous)
    corners = sorted({int(np.ravel_multi_index([(d - 1) * k for d, k in zip(dims, ends)], dims))
                      for ends in np.ndindex(*(2,) * len(dims))})
    for k, at in enumerate(corners):  # every interior corner: the first and the last interior cell among them
        flat[at] += k + 1
    assert flat[0] != ints.reshape(-1)[0] and flat[n - 1] != ints.reshape(-1)[n - 1]
    twins = sorted({n // 3, (2 * n) // 3} - set(corners))
    for at in twins:  # two equal maxima in the middle
        flat[at] -= 50.0
    want = np_diff(L, ints, b, index)
    if len(twins) == 2:
        assert want.max_abs == 50.0 and want.argmax == index.reshape(-1)[twins[0]]
    for ar in arenas(L, shape, dtype, dims):
        put(L, shape, ar.views[0], ints)
        put(L, shape, ar.views[1], b)
        got = p.diff(ar.views[0], ar.views[1])
        print(dims, got)
        assert bits(got) == bits(want)  # max_abs, sum_sq (integers) and a_abs_max exact, the LOWER index of the equal maxima
        back = p.diff(ar.views[1], ar.views[0])
        assert (back.max_abs, back.sum_sq, back.argmax, back.a_abs_max) == (want.max_abs, want.sum_sq, want.argmax, np.abs(b).max())
        assert_guards_intact(ar, f"{shape} {dims}")


@pytest.mark.parametrize("dims", [(1, 1, 8), (3, 5, 16), (20, 33, 72)], ids=lambda d: "x".join(map(str, d)))
def test_bf16_values_with_distant_exponents(L, dims):
    """(double) a - (double) b with one rounding: 1 - 2**-100 rounds to 1 in fp64 as in fp32, 1 - 2**-30 is exact in fp64 only."""
    shape = "box3d1r"
    p = plan_of(shape, "bf16", dims)
    ar = arenas(L, shape, "bf16", dims)[0]
    for small in (2.0 ** -100, 2.0 ** -30):
        put(L, shape, ar.views[0], np.full(dims, 1.0))
        put(L, shape, ar.views[1], np.full(dims, small))
        assert np.array_equal(host(L, shape, ar.views[1]), np.full(dims, small))  # bf16 holds it
        got = p.diff(ar.views[0], ar.views[1])
        want = float(np.float64(1.0) - np.float64(small))
        assert got.max_abs == want and got.a_abs_max == 1.0 and got.nonfinite == 0
        assert got.sum_sq == want * want * got.count or abs(got.sum_sq - want * want * got.count) <= (got.count + 2) * U * got.sum_sq
        back = p.diff(ar.views[1], ar.views[0])
        assert back.max_abs == want and back.a_abs_max == small


@pytest.mark.parametrize("shape,dtype,dims", CASES, ids=IDS)
def test_nonfinite_cells_are_counted_and_ignored(L, shape, dtype, dims):
    ints, _, index = host_data(shape, dtype, dims)
    p = plan_of(shape, dtype, dims)
    n = ints.size
    a = ints.copy()
    flat = a.reshape(-1)
    planted = dict(zip(sorted({n // 2, 0, n - 1}), (np.nan, np.inf, -np.inf)))  # as many of the three as the grid has cells
    for at, v in planted.items():
        flat[at] = v
    ar = arenas(L, shape, dtype, dims)[0]
    put(L, shape, ar.views[0], a)
    put(L, shape, ar.views[1], a)  # the same infinities in both: inf - inf is not finite either
    got = p.stats(ar.views[0])
    print(dims, got)
    assert got.nonfinite == len(planted) and bits(got) == bits(np_stats(L, a))
    df = p.diff(ar.views[0], ar.views[1])
    print(dims, df)
    assert df.nonfinite == len(planted) and bits(df) == bits(np_diff(L, a, a, index))
    # nothing finite at all: the empty record
    put(L, shape, ar.views[0], np.full(dims, np.nan))
    assert bits(p.stats(ar.views[0])) == bits(L.GridStats(math.inf, -math.inf, 0.0, 0.0, 0.0, n, n))
    assert bits(p.diff(ar.views[0], ar.views[1])) == bits(L.GridDiff(0.0, 0.0, 0.0, -1, n, n))
    assert bits(p.diff(ar.views[1], ar.views[0])) == bits(L.GridDiff(0.0, 0.0, 0.0, -1, n, n))


def test_capturing_stream_and_misaligned_buffers_are_refused(L):
    import torch
    from lorastencil_amd import _lib

    p = plan_of("star2d1r", "f64", (33, 130))
    a = torch.zeros(L.padded_shape("star2d1r", (33, 130)), dtype=torch.float64, device="cuda")
    with pytest.raises(L.LoraError) as e:
        p.stats(a.data_ptr() + 8)
    assert e.value.status == _lib.LORA_EUNSUPPORTED
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(L.LoraError) as e:
            p.stats(a, stream=s)
        a.add_(1.0)  # (something to capture)
    assert e.value.status == _lib.LORA_EUNSUPPORTED
    assert p.stats(a).max == 0.0
