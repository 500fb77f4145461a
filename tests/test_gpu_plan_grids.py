"""GPU test of the grids a plan allocates on first need (lora::DeviceGrid in csrc/engine.h: the sweep scratch grid, the two
leapfrog scratch grids, the Chebyshev probe grid, the reductions' records): ONE plan object goes through every driver that owns
one, in turn, and after each call its result equals a fresh plan's for the same call on the same inputs, bit for bit -- each
grid is keyed on its own size and device, and no driver frees or reuses another's.

Shapes: the ragged grids tests/test_gpu_leapfrog.py and tests/test_gpu_leap3.py use for the two-step launch, the smallest with
interior, rim and ragged tiles of it: star2d1r (70, 260), direct variant; star3d1r (19, 33, 62), fp64, leap3 = 1, chunks of 8
planes.  Both have an even innermost extent and the reference boundary.

Memory: five caller buffers (two pairs of levels and f) carved by tests/arena.py out of one poisoned allocation; the guard bands
are intact at the end and f is never written.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (shape, dims, options)
CASES = [("star2d1r", (70, 260), {}), ("star3d1r", (19, 33, 62), {"leap3": 1, "fused_z_chunk": 8})]
IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d, _ in CASES]
RHO = 0.9


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def taps(L, shape, k):
    """small integers on the shape's own support, divided by their sum (taps that round); k picks another set"""
    on = L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0
    w = np.where(on, 1.0 + (np.arange(on.size) + k) % 3, 0.0)
    return w / w.sum()


def bits_of(t):
    return t.view(__import__("torch").int64)


class Grids:
    """prev, cur, f and a second pair of levels on `device`, each with its pristine copy"""

    def __init__(self, L, shape, dims, device="cuda"):
        import torch
        from arena import carve

        rng = np.random.default_rng(zlib.crc32(repr(("plan grids", shape, dims)).encode()))
        ps = L.padded_shape(shape, dims)
        host = [rng.standard_normal(ps) * s for s in (3.0, 2.0, 1.5, 2.5)]
        host.insert(2, np.zeros(ps))  # f: its halo is zero
        L.interior(shape, host[2])[...] = rng.standard_normal(dims) * 1.5
        self.arena = carve(ps, "f64", n_buffers=5, offset_bytes=240, device=device)
        self.prev, self.cur, self.f, self.prev2, self.cur2 = self.arena.views
        self.pristine = [torch.from_numpy(h).to(device) for h in host]
        self.reset()

    def reset(self):
        for view, was in zip(self.arena.views, self.pristine):
            view.copy_(was)

    def snapshot(self):
        import torch

        torch.cuda.synchronize(self.f.device)
        assert torch.equal(bits_of(self.f), bits_of(self.pristine[2])), "f was written"
        return [bits_of(v).clone() for v in self.arena.views]


def same_as_fresh(g, what, used, fresh, call):
    """`call(plan, g)` on the plan under test and on a fresh one, each from the pristine inputs: the same return value and the
    same bits in all five buffers"""
    import torch

    seen = []
    for plan in (used, fresh):
        g.reset()
        r = call(plan, g)
        seen.append((r, g.snapshot()))
    (r0, b0), (r1, b1) = seen
    assert repr(r0) == repr(r1), (what, r0, r1)  # (an UntilResult: its fields as printed, a NaN residual included)
    for i, (x, y) in enumerate(zip(b0, b1)):
        assert torch.equal(x, y), (what, "buffer", i, int((x != y).sum()))


def make_plan(L, shape, dims, opts, w):
    p = L.Plan(shape, dims).set_weights(w)
    for key, value in opts.items():
        p.set_option(key, value)
    return p


def step1(p, g):
    p.run_leapfrog(g.prev, g.cur, -0.9, 9)  # the scratch pair (two pairs of two-step launches) and one tail step


@pytest.mark.parametrize("shape,dims,opts", CASES, ids=IDS)
def test_one_plan_through_every_grid_it_owns(L, shape, dims, opts):
    from arena import assert_guards_intact

    w0, w1 = taps(L, shape, 0), taps(L, shape, 1)
    assert not np.array_equal(w0, w1)
    g = Grids(L, shape, dims)
    p = make_plan(L, shape, dims, opts, w0)
    assert p.leapfrog_depth == 2
    K = p.get_option("steps_per_launch")
    assert K >= 2 and K != 3  # (three applications per launch is the one form that needs no scratch grid)
    a, c = L.chebyshev_coeffs(RHO, 1, 8)
    fresh = lambda w=w0: make_plan(L, shape, dims, opts, w)

    same_as_fresh(g, "1 run_leapfrog(9)", p, fresh(), step1)
    # three launches of the plan's depth: an odd number, so the last two hops go through the sweep scratch grid
    def step2(q, g):
        q.run(g.cur, g.prev, 3 * K)

    def step4(q, g):
        q.run_leapfrog_src(g.prev2, g.cur2, g.f, a, c, 8)

    same_as_fresh(g, "2 run", p, fresh(), step2)
    # the RMS norm keeps the two-pass probe: the probe grid and the records
    until = dict(tol=1e-12, rtol=0.0, check_every=4, max_times=8)
    same_as_fresh(g, "3 run_chebyshev_until", p, fresh(), lambda q, g: q.run_chebyshev_until(g.prev, g.cur, g.f, RHO, norm="rms", **until))
    same_as_fresh(g, "4 run_leapfrog_src(8)", p, fresh(), step4)
    p.set_weights(w1)
    same_as_fresh(g, "5 run_leapfrog(9), other taps", p, fresh(w1), step1)
    same_as_fresh(g, "6 run_until", p, fresh(w1), lambda q, g: q.run_until(g.cur, g.prev, norm="max", **until))
    assert_guards_intact(g.arena, f"{shape} {dims}")


def test_one_plan_on_two_devices(L):
    """the grids are keyed on the device: device 0, device 1 with that device's buffers, device 0 again"""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from arena import assert_guards_intact

    shape, dims, opts = CASES[0]
    w = taps(L, shape, 0)
    grids = [Grids(L, shape, dims, device=f"cuda:{d}") for d in (0, 1)]
    p = make_plan(L, shape, dims, opts, w)
    for d in (0, 1, 0):
        with torch.cuda.device(d):
            same_as_fresh(grids[d], f"device {d}", p, make_plan(L, shape, dims, opts, w), step1)
    for g in grids:
        assert_guards_intact(g.arena, "two devices")
