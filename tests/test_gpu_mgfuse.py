"""GPU tests of the fused defect-and-restrict launch (kernels_mg_fused.hip, lora_plan_mg_defect_restrict) and of plan option
"mgfuse", which puts it into the multigrid cycle in place of lora_plan_defect and lora_plan_mg_restrict (mg.cpp).

The yardstick is the composition the header names, through two public entries that have bit contracts and tests of their own
(tests/test_gpu_pcg.py, tests/test_gpu_mg.py): ``Plan.defect`` into a spare grid, then ``Plan.mg_restrict``.  Every comparison
is ``np.array_equal`` / ``torch.equal`` on integer views: there is no tolerance anywhere in this file.

The kernel's tile, which the extents below are chosen around: a workgroup owns 11 coarse rows x 60 coarse columns in 2D (a
window of 24 x 128 fine cells), 16 coarse planes x 5 coarse rows x 60 coarse columns in 3D (12 x 128 fine cells per plane);
at the 2.2 ratio of the innermost axis the host narrows the tile to 56 columns.

Buffers are carved by tests/arena.py: NaN guard bands around every grid, NaN in the halo of f and in the whole of the coarse
grid before each call; the halo of u is random, it holds the boundary values.
"""
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import test_gpu_mg as M
import test_gpu_pcg as P

pytestmark = pytest.mark.gpu

SCALE = 0.37
TILE_2D = (11, 60)      # coarse rows x coarse columns of a workgroup
TILE_3D = (16, 5, 60)   # coarse planes x rows x columns

SHAPES_2D = ["star2d1r", "box2d1r", "star2d3r", "box2d3r"]
SHAPES_3D = ["star3d1r", "box3d1r"]
DIMS_2D = [
    (9, 10),      # -> (4, 4): the 2.2 ratio on the innermost axis, a single pair
    (14, 14),
    (70, 260),
    (250, 250),   # -> (125, 124): twelve tiles of rows, three of columns
    (33, 1030),
    (300, 24),
    (24, 124),    # -> (12, 62): one full tile plus one coarse row, one full tile plus one pair
]
DIMS_3D = [
    (9, 9, 10),     # -> (4, 4, 4)
    (35, 17, 130),
    (20, 40, 264),
    (34, 12, 124),  # -> (17, 6, 62): one full tile plus one cell on every axis
    (66, 22, 244),  # -> (33, 11, 122): three tiles on every axis
]
CASES = [(s, d) for s in SHAPES_2D for d in DIMS_2D] + [(s, d) for s in SHAPES_3D for d in DIMS_3D]
IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d in CASES]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def _the_tiles_named_above_are_crossed():
    """the extents hold, per axis, one full tile plus one cell (one pair on the innermost axis) and at least three tiles"""
    for tile, dims_list in ((TILE_2D, DIMS_2D), (TILE_3D, DIMS_3D)):
        for axis, t in enumerate(tile):
            coarse = [(d[axis] // 2) & (~1 if axis == len(tile) - 1 else ~0) for d in dims_list]
            step = 2 if axis == len(tile) - 1 else 1
            assert any(c == t + step for c in coarse), (tile, axis, "one full tile plus one cell")
            assert any(c > 2 * t for c in coarse), (tile, axis, "three tiles")


_the_tiles_named_above_are_crossed()


@functools.lru_cache(maxsize=None)
def own_taps(shape):
    """the shape's own table, normalised (what --normalize runs)"""
    import lorastencil_amd as L
    from lorastencil_amd import _lib

    old = _lib.lib().lora_set_default_normalize(1)
    try:
        w = L.Plan(shape, (8, 8) if "2d" in shape else (8, 8, 8)).weights.copy()
    finally:
        _lib.lib().lora_set_default_normalize(old)
    w.setflags(write=False)
    return w


def random_taps(L, shape):
    """normalised random point-symmetric taps on the shape's support"""
    rng = np.random.default_rng(zlib.crc32(repr(("mgfuse taps", shape)).encode()))
    return P.symmetric_random_taps(L, shape, rng, total=1.0)


@functools.lru_cache(maxsize=None)
def fields(shape, dims):
    """u with a random halo, f: random normals, so that the order of every sum shows"""
    import lorastencil_amd as L

    rng = np.random.default_rng(zlib.crc32(repr(("mgfuse", shape, dims)).encode()))
    ps = L.padded_shape(shape, dims)
    u, f = rng.standard_normal(ps) * 3.0, rng.standard_normal(ps)
    u.setflags(write=False)
    f.setflags(write=False)
    return u, f


class Pair:
    """fine grids u, f (NaN halo), spare and coarse grids `fused`, `composed` carved from poisoned arenas; one fused call and the
    composition, and everything a call must leave alone"""

    def __init__(self, L, shape, dims, offset):
        import torch

        self.L, self.shape, self.dims = L, shape, dims
        self.cdims = L.mg_coarse_dims(shape, dims)
        u, f = fields(shape, dims)
        self.fine = P.Grids(L, shape, dims, offset, [u, None, None])
        every = self.fine.interior_mask()
        self.fine.v[1][every] = torch.from_numpy(f.copy()).cuda()[every]  # the halo of f stays NaN
        self.coarse = P.Grids(L, shape, self.cdims, offset, [None, None])  # NaN everywhere
        self.cmask = self.coarse.interior_mask()
        self.before = (self.fine.bits(0), self.fine.bits(1))

    def fused(self, plan, use_f, what):
        import torch

        g, c = self.fine, self.coarse
        c.arena.fill_poison(0)
        plan.mg_defect_restrict(g.v[0], g.v[1] if use_f else None, c.v[0], SCALE)
        g.guards(what)
        c.guards(what)
        assert torch.equal(g.arena.bits(0), self.before[0]) and torch.equal(g.arena.bits(1), self.before[1]), what + ": u or f was written"
        assert bool(c.arena.is_poison(0)[~self.cmask].all()), what + ": a halo cell of the coarse grid was written"
        got = c.host(0)
        assert np.isfinite(got).all(), what + ": a NaN of a halo, a guard or the coarse grid reached a result"
        return got

    def composed(self, plan, use_f):
        g, c = self.fine, self.coarse
        g.arena.fill_poison(2)
        c.arena.fill_poison(1)
        plan.defect(g.v[0], g.v[1] if use_f else None, g.v[2])
        plan.mg_restrict(g.v[2], c.v[1], SCALE)
        return c.host(1)


def same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. the launch is the composition, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", CASES, ids=IDS)
def test_the_launch_is_defect_then_restrict_bit_for_bit(L, shape, dims):
    pair = Pair(L, shape, dims, 16)
    for kind, w in (("random", random_taps(L, shape)), ("own", own_taps(shape))):
        plan = L.Plan(shape, dims).set_weights(w)
        assert plan.get_option("mg") == 1
        for use_f in (True, False):
            what = f"{shape} {dims} -> {pair.cdims} {kind} taps f {use_f}"
            got, want = pair.fused(plan, use_f, what), pair.composed(plan, use_f)
            differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
            print(what, "cells that differ:", differ, "of", got.size, "max |value|", np.abs(want).max())
            assert np.abs(want).max() > 0.0
            assert same(got, want), f"{what}: {differ} coarse cells differ from Plan.defect + Plan.mg_restrict"


# ---- 2. nothing else is touched, hostile memory reaches nothing, the same bits every time ---------------------------------------
@pytest.mark.parametrize("shape,dims", [("box2d3r", (70, 260)), ("star2d1r", (9, 10)), ("star2d3r", (24, 124)), ("box3d1r", (35, 17, 130)),
                                        ("star3d1r", (34, 12, 124))])
def test_nothing_else_is_touched_and_two_calls_give_the_same_bits(L, shape, dims):
    plan = L.Plan(shape, dims).set_weights(random_taps(L, shape))
    runs = []
    for off in (240, 496):
        pair = Pair(L, shape, dims, off)  # Pair.fused checks u, f, the guards, the coarse halo and that the interior is finite
        for use_f in (True, False):
            first = pair.fused(plan, use_f, f"{shape} {dims} offset {off} f {use_f}")
            again = pair.fused(plan, use_f, f"{shape} {dims} offset {off} f {use_f}, second call")
            assert same(first, again), "the same call gave other bits"
            assert same(first, pair.composed(plan, use_f))
            runs.append(first)
    assert same(runs[0], runs[2]) and same(runs[1], runs[3]), "the bits depend on where the buffers lie"
    assert not same(runs[0], runs[1]), "f reached nothing"


# ---- 3. whole cycles ----------------------------------------------------------------------------------------------------------
CYCLE_CASES = [("star2d1r", (70, 260)), ("box2d3r", (64, 64)), ("star3d1r", (35, 17, 130)), ("box3d1r", (16, 16, 32))]
CYCLE_IDS = [f"{s}-{'x'.join(map(str, d))}" for s, d in CYCLE_CASES]


def cycle_problem(L, shape, dims):
    rng = np.random.default_rng(zlib.crc32(repr(("mgfuse cycle", shape, dims)).encode()))
    w = P.symmetric_random_taps(L, shape, rng)
    ps = L.padded_shape(shape, dims)
    return w, rng.standard_normal(ps), rng.standard_normal(ps)  # non-zero halo values in x0: the boundary


def plans(L, shape, dims, w, coarse1=0):
    off = L.Plan(shape, dims).set_weights(w).set_option("coarse1", coarse1)
    on = L.Plan(shape, dims).set_weights(w).set_option("coarse1", coarse1).set_option("mgfuse", 1)
    assert off.get_option("mgfuse") == 0 and on.get_option("mgfuse") == 1
    return off, on


def drive(L, shape, dims, plan, x0, f, what):
    """every driver that goes through the cycle, each from fresh grids; the results as integer tensors"""
    import torch

    out = {}
    for cycles in (1, 3):
        g = M.Grids(L, shape, dims, 16, [x0, f])
        res = plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=cycles)
        g.guards(f"{what} run_mg_until x{cycles}")
        assert res.until.times_done == cycles
        out[f"run_mg_until x{cycles}"] = g.bits(0)
        if cycles == 1:
            out["cost"], out["level_dims"] = plan.mg_cycle_cost(), res.level_dims
    for sigma, tau in ((1.0, 1.0), (1.5, 0.5)):
        g = P.Grids(L, shape, dims, 240, [None, None])  # r: its halo stays NaN; z: NaN everywhere
        every = g.interior_mask()
        g.v[0][every] = torch.from_numpy(f).cuda()[every]
        plan.mg_precondition(g.v[0], g.v[1], sigma, tau, pre=2, post=2, omega=0.8)
        g.guards(f"{what} mg_precondition ({sigma}, {tau})")
        out[f"mg_precondition ({sigma}, {tau})"] = g.bits(1)[every]
    g = P.Grids(L, shape, dims, 16, [x0, f])
    # (a round of lora_plan_run_pcg_until is an even number of iterations: four is the least count that holds three)
    res = plan.run_pcg_until(g.v[0], g.v[1], tol=0.0, check_every=2, max_times=4)
    g.guards(f"{what} run_pcg_until")
    assert res.until.times_done == 4
    out["run_pcg_until x4"] = g.bits(0)
    g = P.Grids(L, shape, dims, 16, [x0, f])
    res = plan.run_theta_mg(g.v[0], g.v[1], 64.0, 2, theta=1.0, max_iters=4, rtol=1e-10, check_every=2)
    g.guards(f"{what} run_theta_mg")
    assert res.steps_done == 2
    out["run_theta_mg x2"] = g.bits(0)
    return out


def compare_drivers(L, shape, dims, coarse1):
    import torch

    w, x0, f = cycle_problem(L, shape, dims)
    off, on = plans(L, shape, dims, w, coarse1)
    a = drive(L, shape, dims, off, x0, f, f"{shape} {dims} mgfuse off")
    b = drive(L, shape, dims, on, x0, f, f"{shape} {dims} mgfuse on")
    start = M.Grids(L, shape, dims, 16, [x0, f]).bits(0)
    assert not torch.equal(a["run_mg_until x1"], start), "a cycle changed nothing: the comparison would show nothing"
    for key in a:
        if key in ("cost", "level_dims"):
            continue
        assert torch.equal(a[key], b[key]), f"{shape} {dims} coarse1 {coarse1}: {key} with mgfuse on differs from mgfuse off"
    return a, b


@pytest.mark.parametrize("shape,dims", CYCLE_CASES, ids=CYCLE_IDS)
def test_the_drivers_give_the_same_bits_with_the_option_on(L, shape, dims):
    compare_drivers(L, shape, dims, 0)


def test_the_drivers_give_the_same_bits_with_coarse1_on_as_well(L):
    compare_drivers(L, "box2d3r", (64, 64), 1)


# ---- 4. the cycle's cost --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", CYCLE_CASES, ids=CYCLE_IDS)
def test_cycle_cost_counts_one_launch_and_two_passes_fewer_per_level(L, shape, dims):
    w, x0, f = cycle_problem(L, shape, dims)
    for coarse1 in (0, 1):
        costs = []
        for plan in plans(L, shape, dims, w, coarse1):
            g = M.Grids(L, shape, dims, 16, [x0, f])
            res = plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=1)
            costs.append(plan.mg_cycle_cost())
        (n_off, b_off), (n_on, b_on) = costs
        levels = len(res.level_dims)
        cells = sum(float(np.prod(d)) for d in res.level_dims[:-1])
        print(shape, dims, "coarse1", coarse1, "levels", levels, "launches off", n_off, "on", n_on, "bytes off", b_off, "on", b_on)
        assert levels >= 2 and n_off - n_on == levels - 1
        assert b_off - b_on == 16.0 * cells


def test_the_option_changes_nothing_on_a_plan_whose_cycles_never_run(L):
    import torch

    shape, dims = "star2d1r", (70, 260)
    w, x0, _ = cycle_problem(L, shape, dims)
    off, on = plans(L, shape, dims, w)
    assert (off.kernel_name, off.kernel_signature) == (on.kernel_name, on.kernel_signature)
    results = []
    for plan in (off, on):
        a, b = torch.from_numpy(x0).cuda(), torch.from_numpy(x0).cuda()
        plan.run(a, b, 6)
        torch.cuda.synchronize()
        results.append(a.clone())
    assert P.same_bits(results[0], results[1])


# ---- 5. the thread default and the CLI ------------------------------------------------------------------------------------------
def test_the_thread_default_reaches_the_plan_of_run_host_mg_and_comes_back(L):
    """lora_run_host_mg reports the bytes of a cycle through its hbm_gbs: bytes per cycle = hbm_gbs x seconds / cycles.  They are
    the plan's lora_plan_mg_cycle_cost, which differs between off and on by 16 bytes per cell of every level below the coarsest."""
    from lorastencil_amd import _lib

    shape, dims = "star2d1r", (64, 64)
    u, f = fields(shape, dims)
    w = own_taps(shape)
    want = {}
    for key, plan in zip((0, 1), plans(L, shape, dims, w)):
        g = M.Grids(L, shape, dims, 16, [u, f])
        plan.run_mg_until(g.v[0], g.v[1], tol=0.0, check_every=1, max_times=1)
        want[key] = plan.mg_cycle_cost()[1]
    assert want[0] > want[1]
    old_norm = _lib.lib().lora_set_default_normalize(1)
    assert L.set_default_mgfuse(0) == 0
    try:
        outs = {}
        for key in (0, 1):
            assert L.set_default_mgfuse(key) == 0
            out, res, info = L.run_host_mg(shape, u, 0.0, source=f, check_every=1, max_times=2)
            assert L.set_default_mgfuse(0) == key, "the run changed the thread's default"
            per_cycle = info.hbm_gbs * 1e9 * info.sweep_seconds / res.until.times_done
            print("default", key, "bytes per cycle from the run info", per_cycle, "from the plan", want[key])
            assert abs(per_cycle - want[key]) <= 1e-9 * want[key]
            outs[key] = out
        assert same(outs[0], outs[1])
        assert L.Plan(shape, dims).get_option("mgfuse") == 0
    finally:
        L.set_default_mgfuse(0)
        _lib.lib().lora_set_default_normalize(old_norm)


def test_cli_flag_mgfuse(L):
    """starting the tool is what this test is about"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_2d")
    args = [exe, "star2d1r", "64", "64", "20", "--normalize", "--bc=dirichlet", "--mg", "--until=1e-9"]  # (--mg needs --until)
    timed = ("Time = ", "GStencil/s = ", "GStencils/s ", "Algorithmic HBM traffic", "Total incl. transfers")
    lines = []
    for extra in ([], ["--mgfuse"], ["--mgfuse", "--coarse1"]):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0
        lines.append([ln for ln in r.stdout.splitlines() if not ln.startswith(timed)])
    assert any(ln.startswith("Multigrid: V(2,2) cycles = ") for ln in lines[0]) and any(ln.startswith("Until: ") for ln in lines[0])
    assert any(ln.startswith("Result range = [") for ln in lines[0])
    assert lines[0] == lines[1], "--mgfuse changed a result line"
    assert len(lines[2]) == len(lines[0])


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------
def test_the_launch_is_ordered_behind_a_long_sweep_on_its_stream(L):
    """tests/test_gpu_stream_order.py's scenario A for one entry: a gate (one workgroup spinning for a bounded time), then a long
    run of sweeps that produces u, then lora_plan_mg_defect_restrict, all on one non-blocking stream.  A launch that did not wait
    for its stream would read u before the sweeps wrote it."""
    import torch

    shape, dims, sweeps = "star2d1r", (70, 260), 400
    w = own_taps(shape)
    u0, f = fields(shape, dims)
    cdims = L.mg_coarse_dims(shape, dims)
    sweep = L.Plan(shape, dims).set_weights(w).set_boundary("dirichlet").set_option("graph", 0)
    plan = L.Plan(shape, dims).set_weights(w)

    def sequence(stream, wait):
        g = P.Grids(L, shape, dims, 16, [u0 * 1e3, f, u0 * 1e3])
        c = P.Grids(L, shape, cdims, 16, [None])
        torch.cuda.synchronize()
        busy = None
        with torch.cuda.stream(stream):
            if not wait:
                torch.cuda._sleep(40_000_000)  # 20 ms at a 2 GHz counter, 400 ms at 100 MHz: longer than the enqueueing below
            sweep.run(g.v[0], g.v[2], sweeps, stream=stream)  # an even count: the result is back in grid 0
            if wait:
                torch.cuda.synchronize()
            plan.mg_defect_restrict(g.v[0], g.v[1], c.v[0], SCALE, stream=stream)
            busy = not stream.query()
        torch.cuda.synchronize()
        g.guards(f"stream order, wait {wait}")
        c.guards(f"stream order, wait {wait}")
        return g, c, busy

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.zeros(8, device="cuda").add_(1.0)  # the first use of a stream sets up its queue
    torch.cuda.synchronize()
    ref_g, ref_c, _ = sequence(s, True)
    got_g, got_c, busy = sequence(s, False)
    assert busy, "the stream had drained when the call returned: the gate was too short to show anything"
    # the sweeps moved u, and the launch's result depends on it
    start = P.Grids(L, shape, dims, 16, [u0 * 1e3])
    stale = P.Grids(L, shape, cdims, 16, [None])
    plan.mg_defect_restrict(start.v[0], ref_g.v[1], stale.v[0], SCALE)
    torch.cuda.synchronize()
    assert not same(stale.host(0), ref_c.host(0))
    assert P.same_bits(ref_g.v[0], got_g.v[0]) and same(ref_c.host(0), got_c.host(0))
