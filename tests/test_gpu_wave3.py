"""GPU tests of the 3D two-step wave launch behind plan option "wave3" (kernels_3d_step2.hip, EPI_WAVE).  Every
comparison is bit for bit.

Contract under test: with the option on, a 3D fp64 plan with an even innermost extent has lora_plan_wave_depth 2; one launch of
lora_plan_step2_wave[_region] equals two single steps (lora_plan_step_wave) on any data: out1 = k S(cur) + b cur + c prev,
out2 = k S(out1) + b out1 + c cur, five separate roundings per level; it writes the interior cells of the region's planes of out1
and out2 and nothing else, reads no halo cell of k and nothing outside the padded arrays; runs give the bits they give without the
option.

Memory: prev, cur, k, out1, out2 are five buffers carved by tests/arena.py out of one poisoned allocation, at every offset of
arena.OFFSETS.  prev and cur hold different seeded values in their halos too; the halo of k is NaN, so a halo cell of k that is
read shows in the results.  After every call the guard bands are intact and prev, cur and k are unchanged bit for bit.

Shapes: those of tests/test_gpu_leap3.py, the kernel's geometry -- (1, 1, 2) the smallest grid; (3, 2, 8) a small grid in one
tile; (12, 30, 60) exactly one output tile of 30 x 60; (19, 33, 62) with fused_z_chunk = 8: 2 x 2 ragged tiles, three chunks along
z, the last one short, so the centre cells a lane carries from one plane iteration to the next start afresh in every chunk;
(9, 31, 124): three column tiles, rim tiles only in y.
"""
import functools
import os
import subprocess
import time
import zlib

import numpy as np
import pytest

import stencil_model as M
from test_gpu_wave import GATE_MS, _independent_stream, _spin_cycles_per_ms

pytestmark = pytest.mark.gpu

FILL = -7.0  # what an output buffer holds before a launch: a cell the launch must not write keeps it
COEFS = ((2.0, -1.0), (1.9, -0.9), (0.7, 0.3))  # 1.9 * u, 0.7 * u and 0.3 * prev round, so a contracted fused multiply-add shows
INT_COEFS = ((2, -1), (-3, 2))
SHAPES = ("star3d1r", "box3d1r")
# (dims, options beside wave3)
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


def support(L, shape):
    return L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0


def real_taps(L, shape):
    """small integers on the shape's own support (the plan resolves the same tap set), divided by their sum: taps that round"""
    on = support(L, shape)
    w = np.where(on, 1.0 + np.arange(on.size) % 3, 0.0)
    return w / w.sum()


def regions_of(h):
    """the whole range, one that starts and ends inside chunks, the last plane, an empty one"""
    inner = (3, 14) if h > 14 else ((1, h - 1) if h >= 3 else None)
    out = [(0, h)] + ([inner] if inner else []) + [(h - 1, h), (h // 2, h // 2)]
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def host_data(dims):
    """per grid, made once, read-only: seeded non-integer prev, cur (whole padded arrays, so their halos differ) and k, whose halo
    is NaN"""
    rng = np.random.default_rng(zlib.crc32(repr(("wave3", dims)).encode()))
    ps = M.padded_shape("star3d1r", dims)
    prev, cur = rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 2.0
    k = np.full(ps, np.nan)
    M.interior("star3d1r", k)[...] = rng.uniform(0.05, 0.45, dims)
    for a in (prev, cur, k):
        a.setflags(write=False)
    return prev, cur, k


@functools.lru_cache(maxsize=None)
def int_data(dims):
    """per grid, made once, read-only: integer prev and cur in -4 .. 4 over the whole padded arrays, integer k in 0 .. 3 that
    differs from cell to cell on the interior (the rule of tests/test_gpu_wave.py), NaN in k's halo"""
    rng = np.random.default_rng(zlib.crc32(repr(("wave3-int", dims)).encode()))
    ps = M.padded_shape("star3d1r", dims)
    prev = rng.integers(-4, 5, ps).astype(np.float64)
    cur = rng.integers(-4, 5, ps).astype(np.float64)
    k = np.full(ps, np.nan)
    M.interior("star3d1r", k)[...] = (np.indices(dims).sum(axis=0) + np.arange(int(np.prod(dims))).reshape(dims) // 7) % 4
    for a in (prev, cur, k):
        a.setflags(write=False)
    return prev, cur, k


def bits_of(t):
    return t.view(__import__("torch").int64)


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


class Grids:
    """prev, cur, k and two or no more buffers carved out of one poisoned allocation"""

    def __init__(self, L, dims, offset, prev, cur, k, n_buffers=5):
        import torch
        from arena import carve

        self.arena = carve(L.padded_shape("star3d1r", dims), "f64", n_buffers=n_buffers, offset_bytes=offset)
        self.prev, self.cur, self.k = self.arena.views[0], self.arena.views[1], self.arena.views[2]
        self.spare = self.arena.views[3:]
        self.h_prev = torch.from_numpy(np.array(prev)).cuda()
        self.h_cur = torch.from_numpy(np.array(cur)).cuda()
        self.h_k = torch.from_numpy(np.array(k)).cuda()
        self.k.copy_(self.h_k)
        self.reset()

    def reset(self):
        self.prev.copy_(self.h_prev)
        self.cur.copy_(self.h_cur)
        for s in self.spare:
            s.fill_(FILL)

    def check(self, what, kept=()):
        """guards intact; k, and every buffer of `kept` (pairs of a view and what it held), unchanged bit for bit"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i, (view, was) in enumerate(((self.k, self.h_k),) + tuple(kept)):
            assert torch.equal(bits_of(view), bits_of(was)), f"{what}: read-only buffer {i} was written"


def two_single_steps(ref, g, b, c):
    """whole-grid single steps on copies: level 1 carries prev's halo, level 2 cur's"""
    l1 = g.h_prev.clone()
    ref.step_wave(g.h_cur, l1, g.h_k, b, c)
    l2 = g.h_cur.clone()
    ref.step_wave(l1, l2, g.h_k, b, c)
    return l1, l2


def launch(q, g, o1, o2, b, c, region):
    if region is None:
        q.step2_wave(g.prev, g.cur, g.k, o1, o2, b, c)
    else:
        q.step2_wave_region(g.prev, g.cur, g.k, o1, o2, b, c, *region)


def plan_with(L, shape, dims, w, opts, **more):
    q = L.Plan(shape, dims).set_weights(w).set_option("wave3", 1)
    for key, value in {**opts, **more}.items():
        q.set_option(key, value)
    return q


def assert_region(L, shape, o1, o2, want1, want2, where):
    assert same_bits(o1, want1), where + ("out1", int((bits_of(o1) != bits_of(want1)).sum()))
    assert same_bits(o2, want2), where + ("out2", int((bits_of(o2) != bits_of(want2)).sum()))


# ---- 1. the bit contract on real data -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,opts", CASES, ids=IDS)
def test_two_step_launch_is_two_single_steps(L, shape, dims, opts):
    """out1 and out2 on the planes of the region against whole-grid single steps of a plan without the option; cells outside the
    region and all halo cells keep the fill value; the whole-grid entry is the same launch"""
    import torch
    from arena import OFFSETS

    prev, cur, k = host_data(dims)
    w = real_taps(L, shape)
    ref = L.Plan(shape, dims).set_weights(w)
    assert ref.wave_depth == 1
    q = plan_with(L, shape, dims, w, opts)
    assert q.wave_depth == 2 and q.leapfrog_depth == 1
    sig = q.kernel_signature
    for n, off in enumerate(OFFSETS):
        g = Grids(L, dims, off, prev, cur, k)
        o1, o2 = g.spare
        b, c = COEFS[n % len(COEFS)]
        l1, l2 = two_single_steps(ref, g, b, c)
        assert not bool(torch.isnan(L.interior(shape, l2)).any())  # (no halo cell of k got in on the reference's side either)
        for region in regions_of(dims[0]) + [None]:
            begin, end = region if region else (0, dims[0])
            want1, want2 = torch.full_like(l1, FILL), torch.full_like(l2, FILL)
            L.interior(shape, want1)[begin:end] = L.interior(shape, l1)[begin:end]
            L.interior(shape, want2)[begin:end] = L.interior(shape, l2)[begin:end]
            g.reset()
            launch(q, g, o1, o2, b, c, region)
            g.check(f"{shape} {dims} b={b} c={c} {region}", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
            assert_region(L, shape, o1, o2, want1, want2, (off, b, c, region))
    assert q.kernel_signature == sig and q.wave_depth == 2


# ---- 2. the exact integer model -----------------------------------------------------------------------------------------------
def model(shape, prev, cur, k, w, b, c, u2_from_cur=False, k2_shift=None):
    """int64: level 1 = k S(cur) + b cur + c prev on the whole interior inside prev's halo; out2 = k S(level 1) + b level 1 + c cur.
    The two wrong models a test on this data must tell from the right one: level 2's centre term read from cur, and level 2's k
    read at the level-1 cell's place in the tile (k2_shift = (rows, columns) the k grid is rolled by)."""
    ki = M.ints(M.interior(shape, k))
    ui, pi = M.interior(shape, M.ints(cur)), M.interior(shape, M.ints(prev))
    out1 = ki * M.apply(shape, cur, w) + b * ui + c * pi
    level1 = M.with_halo(shape, out1, M.ints(prev))
    k2 = ki if k2_shift is None else np.roll(ki, k2_shift, axis=(1, 2))
    out2 = k2 * M.apply(shape, level1, w) + b * (ui if u2_from_cur else out1) + c * ui
    return out1, out2


def model_bound(shape, prev, cur, k, w, b, c):
    """no partial sum of either level, in any order, exceeds these"""
    ki = M.ints(M.interior(shape, k))
    ua, pa = np.abs(M.interior(shape, M.ints(cur))), np.abs(M.interior(shape, M.ints(prev)))
    m1 = ki * M.magnitude(shape, cur, w) + abs(b) * ua + abs(c) * pa
    m2 = ki * M.magnitude(shape, M.with_halo(shape, m1, np.abs(M.ints(prev))), w) + abs(b) * m1 + abs(c) * ua
    return [m1, m2]


@pytest.mark.parametrize("shape,dims,opts", CASES, ids=IDS)
def test_two_step_launch_equals_the_integer_model(L, shape, dims, opts):
    """fingerprint taps (pairwise distinct, no symmetry left), small integers, k in 0 .. 3 that differs per cell with NaN in its
    halo: both levels equal the int64 model with ==.  On every grid of more than one cell the model with level 2's u taken from
    cur, and the one with level 2's k taken one row and two columns away, give other numbers: either mistake fails this test"""
    from arena import OFFSETS

    prev, cur, k = int_data(dims)
    w = M.fingerprint_taps(support(L, shape))
    q = plan_with(L, shape, dims, w.astype(np.float64), opts)
    h = dims[0]
    for n, off in enumerate(OFFSETS[:2]):
        g = Grids(L, dims, off, prev, cur, k)
        o1, o2 = g.spare
        b, c = INT_COEFS[n % len(INT_COEFS)]
        M.assert_exact(f"{shape} {dims}", model_bound(shape, prev, cur, k, w, b, c))
        want1, want2 = model(shape, prev, cur, k, w, b, c)
        assert not np.array_equal(model(shape, prev, cur, k, w, b, c, u2_from_cur=True)[1], want2)
        if dims[1] > 1:
            assert not np.array_equal(model(shape, prev, cur, k, w, b, c, k2_shift=(1, 2))[1], want2)
            assert not np.array_equal(model(shape, prev, cur, k, w, b, c, k2_shift=(-1, -2))[1], want2)
        for begin, end in regions_of(h):
            g.reset()
            q.step2_wave_region(g.prev, g.cur, g.k, o1, o2, b, c, begin, end)
            g.check(f"{shape} {dims} b={b} c={c} [{begin}, {end})", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
            got1, got2 = o1.cpu().numpy(), o2.cpu().numpy()
            assert M.exactly(M.interior(shape, got1)[begin:end], want1[begin:end]), (off, b, c, begin, end, "out1")
            assert M.exactly(M.interior(shape, got2)[begin:end], want2[begin:end]), (off, b, c, begin, end, "out2")
            for got in (got1, got2):
                keep = np.ones(got.shape, dtype=bool)
                M.interior(shape, keep)[begin:end] = False
                assert (got[keep] == FILL).all(), (off, b, c, begin, end, "a cell outside the region")


# ---- 3. non-finite data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_non_finite_data_gives_the_bits_of_two_single_steps(L, shape):
    """NaN, +inf and -inf in interior cells of cur, prev and k -- at tile corners, tile seams, chunk seams and the grid's faces:
    the same positions and the same bit patterns as two single steps"""
    import torch

    dims = BIG
    prev, cur, k = (np.array(x) for x in host_data(dims))
    h, m, n = dims
    spots = [(0, 0, 0), (h - 1, m - 1, n - 1), (7, 29, 59), (8, 30, 60), (15, 31, 61), (16, 0, 30), (9, 15, 1), (18, 32, 0), (4, 30, 59)]
    vals = [np.nan, np.inf, -np.inf]
    for i, s in enumerate(spots):
        (L.interior(shape, cur), L.interior(shape, prev), L.interior(shape, k))[i % 3][s] = vals[(i // 3) % 3]
    L.interior(shape, cur)[10, 3, 40:44] = [np.inf, -np.inf, np.nan, np.inf]  # inf - inf inside one window
    w = real_taps(L, shape)
    ref = L.Plan(shape, dims).set_weights(w)
    q = plan_with(L, shape, dims, w, {"fused_z_chunk": 8})
    g = Grids(L, dims, 48, prev, cur, k)
    o1, o2 = g.spare
    for b, c in COEFS:
        l1, l2 = two_single_steps(ref, g, b, c)
        assert bool(torch.isnan(L.interior(shape, l2)).any()) and bool(torch.isfinite(L.interior(shape, l2)).any())
        for region in ((0, h), (3, 14)):
            g.reset()
            launch(q, g, o1, o2, b, c, region)
            g.check(f"{shape} non-finite b={b} c={c} {region}", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
            lo, hi = region
            for got, exp, what in ((o1, l1, "out1"), (o2, l2, "out2")):
                gi, ei = L.interior(shape, got)[lo:hi], L.interior(shape, exp)[lo:hi]
                assert same_bits(gi, ei), (b, c, region, what, int((bits_of(gi.contiguous()) != bits_of(ei.contiguous())).sum()))


# ---- 4. runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reference", "dirichlet", "periodic", "scratch=0", "leap3"])
@pytest.mark.parametrize("shape", SHAPES)
def test_runs_equal_the_runs_without_the_option(L, shape, how):
    """run_wave, both buffers, against the same plan with wave3 = 0; k is a buffer of its own, equal to no scratch grid"""
    dims = BIG
    prev, cur, k = host_data(dims)
    w = real_taps(L, shape)
    g = Grids(L, dims, 112, prev, cur, k, n_buffers=3)

    def plan(wave3):
        p = L.Plan(shape, dims).set_weights(w).set_option("wave3", wave3).set_option("fused_z_chunk", 8)
        if how in ("reference", "dirichlet", "periodic"):
            return p.set_boundary(how)
        return p.set_option("scratch", 0) if how == "scratch=0" else p.set_option("leap3", 1)

    off_plan, on_plan = plan(0), plan(1)
    assert off_plan.wave_depth == 1 and on_plan.wave_depth == 2
    for n, times in enumerate(TIMES):
        b, c = COEFS[n % len(COEFS)]
        g.reset()
        off_plan.run_wave(g.prev, g.cur, g.k, b, c, times)
        g.check("reference run")
        want = (g.prev.clone(), g.cur.clone())
        g.reset()
        on_plan.run_wave(g.prev, g.cur, g.k, b, c, times)
        g.check(f"{shape} {how} run_wave({times})")
        assert same_bits(g.prev, want[0]) and same_bits(g.cur, want[1]), times
    assert on_plan.wave_depth == 2 and off_plan.wave_depth == 1


# ---- 5. the host entry and the CLI --------------------------------------------------------------------------------------------
def test_host_entry_and_cli(L):
    """run_host_wave under set_default_wave3(1) equals the default run bit for bit; the CLI prints the same lines"""
    shape, dims = "star3d1r", BIG
    rng = np.random.default_rng(11)
    ps = L.padded_shape(shape, dims)
    cur, prev = rng.standard_normal(ps), rng.standard_normal(ps)
    kappa = np.full(ps, np.nan)
    L.interior(shape, kappa)[...] = rng.uniform(0.01, 0.03, dims)
    out0, info0 = L.run_host_wave(shape, cur, prev, kappa, b=1.9, c=-0.9, laplacian=True, times=9)
    assert info0.steps_per_launch == 1
    assert L.set_default_wave3(1) == 0
    try:
        out1, info1 = L.run_host_wave(shape, cur, prev, kappa, b=1.9, c=-0.9, laplacian=True, times=9)
    finally:
        assert L.set_default_wave3(0) == 1
    assert info1.steps_per_launch == 2
    assert np.isfinite(L.interior(shape, out0)).all()
    assert np.array_equal(out0.view(np.int64), out1.view(np.int64))

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "lorastencil_amd", "bin", "lorastencil_3d")
    timing = ("Time = ", "GStencil/s = ", "GStencils/s ", "Algorithmic HBM traffic", "Total incl. transfers")
    seen = []
    for extra in ([], ["--wave3"]):
        run = subprocess.run([exe, "star3d1r", "20", "34", "64", "8", "--wave=0.1,0.2", *extra], capture_output=True, text=True,
                             timeout=120)
        print(run.stdout, run.stderr)
        assert run.returncode == 0
        lines = run.stdout.splitlines()
        assert lines[0] == "INFO: shape = star_3d1r, h = 20, m = 34, n = 64, times = 8"
        assert any(ln.startswith("Result range = [") for ln in lines)
        seen.append([ln for ln in lines if not ln.startswith(timing)])
    assert seen[0] == seen[1] and len(seen[0]) >= 2


# ---- 6. stream ordering -------------------------------------------------------------------------------------------------------
def test_step2_wave_is_ordered_on_its_stream(L):
    """One call on a non-blocking stream S while a gate (a bounded spin) is pending on S: then on S the uploads over poisoned
    grids, the call, a snapshot, poison again -- work that is not ordered on S runs before the input exists.  The snapshot equals the
    ungated call of a twin plan bit for bit; afterwards the grids hold nothing but poison; the call did not block."""
    import torch
    from arena import assert_guards_intact, carve

    shape, dims = "star3d1r", BIG
    b, c = 1.9, -0.9
    staged = [torch.from_numpy(np.array(x)).cuda() for x in host_data(dims)]
    ar = carve(L.padded_shape(shape, dims), "f64", n_buffers=5, offset_bytes=16)
    v = ar.views

    def make_plan():
        return plan_with(L, shape, dims, real_taps(L, shape), {"fused_z_chunk": 8})

    def call(p, stream):
        p.step2_wave(v[0], v[1], v[2], v[3], v[4], b, c, stream=stream)

    def upload():
        for view, src in zip(v[:3], staged):
            view.copy_(src, non_blocking=True)

    null = torch.cuda.default_stream()
    per_ms = _spin_cycles_per_ms(torch)
    S = _independent_stream(torch, null, per_ms)
    # the ungated call of a twin plan on an idle device: the expected bits (it also loads the kernel's code object)
    twin, plan = make_plan(), make_plan()
    expected = None
    for q in (twin, plan):
        ar.flat.fill_(ar.poison)
        with torch.cuda.stream(S):
            upload()
            call(q, S)
        torch.cuda.synchronize()
        if expected is None:
            expected = ar.flat.clone()
        assert torch.equal(ar.flat, expected), "the ungated call is not deterministic"
    assert_guards_intact(ar, "ungated")
    for i in (3, 4):  # out1 and out2 were written
        assert not bool((expected[ar.spans[i][0]:ar.spans[i][1]] == ar.poison).all())

    snap = torch.empty_like(ar.flat)
    ar.flat.fill_(ar.poison)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(GATE_MS * per_ms))
    t_gate = time.perf_counter()
    with torch.cuda.stream(S):
        upload()
        call(plan, S)
        busy_after = not S.query()
        host_ms = (time.perf_counter() - t_gate) * 1e3
        snap.copy_(ar.flat, non_blocking=True)
        ar.flat.fill_(ar.poison)
    torch.cuda.synchronize()
    print(f"stream-order step2_wave 3D: host {host_ms:.2f} ms behind the gate, busy after: {busy_after}")
    assert host_ms < GATE_MS / 2, "the host was held up for longer than half the gate: the case shows nothing"
    assert busy_after, "the call blocked until the gated stream had drained"
    bad = snap != expected
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ from the ungated call's"
    assert bool((ar.flat == ar.poison).all()), "something wrote into the grids after the caller's stream had put the poison back"
