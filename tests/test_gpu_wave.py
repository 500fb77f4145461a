"""GPU tests of the variable-coefficient wave step (lora_plan_step_wave ... lora_run_host_wave; kernels_step.hip,
kernels_2d_wave2.hip, leapfrog.cpp): u+ = k(x) S(u) + b u + c u-, the new level stored over the oldest one.

Contract under test: one step is prev = fl(fl(fl(k acc) + fl(b u)) + fl(c prev)) on the interior cells of the swept range, acc the
bits of the plan's plain single sweep of cur, u the centre cell of cur, k the cell of the coefficient grid; halo cells of prev never
written, halo cells of k never read, cur and k never written; the 2D two-step launch equals two single steps bit for bit; run_wave
equals that many single steps whatever its schedule, also on a 3D plan with option leap3 (which has no two-step wave launch).

Memory: the grids are FOUR or FIVE buffers carved by tests/arena.py out of one poisoned allocation, at offsets 16 and 240.  prev,
cur and k hold different seeded values in their halos too (the integer test puts NaN into k's halo), so a mixed-up halo or a used
halo of k shows.  After every call the guard bands are intact and every read-only buffer is unchanged bit for bit.

Shapes: the cases, regions and offsets of tests/test_gpu_leapfrog_src.py -- the kernels have the tiles of the leapfrog kernels:
two 2D tile columns of 122, a ragged last tile, several z chunks, the odd-extent generic kernels, the one-cell grids.
"""
import functools
import time
import zlib

import numpy as np
import pytest

import stencil_model as M

pytestmark = pytest.mark.gpu

OFFSETS = (16, 240)
FILL = -7.0  # what an output buffer holds before a launch: a cell the launch must not write keeps it
COEFS = ((2.0, -1.0), (1.9, -0.9), (0.7, 0.3))  # 1.9 * u, 0.7 * u and 0.3 * prev round, so a contracted fused multiply-add shows
INT_COEFS = ((2, -1), (-3, 2))

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
RUNS = [CASES[i] for i in (1, 3, 4, 5, 6, 9, 10, 11)]  # (every extent reaches the halo width: the periodic wrap takes them)
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


def wave_depth_of(dims):
    return 2 if len(dims) == 2 and dims[1] % 2 == 0 else 1


@functools.lru_cache(maxsize=None)
def host_data(shape, dims):
    """per case, made once, read-only: three seeded real grids (prev, cur, k), whole padded arrays (so their halos differ)"""
    rng = np.random.default_rng(zlib.crc32(repr(("wave", shape, dims)).encode()))
    ps = M.padded_shape(shape, dims)
    out = (rng.standard_normal(ps) * 3.0, rng.standard_normal(ps) * 2.0, rng.uniform(0.05, 0.45, ps))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def int_data(shape, dims):
    """per case, made once, read-only: integer prev and cur in -4 .. 4 over the whole padded arrays, integer k in 0 .. 3 that
    differs from cell to cell on the interior, NaN in k's halo"""
    rng = np.random.default_rng(zlib.crc32(repr(("wave-int", shape, dims)).encode()))
    ps = M.padded_shape(shape, dims)
    prev = rng.integers(-4, 5, ps).astype(np.float64)
    cur = rng.integers(-4, 5, ps).astype(np.float64)
    k = np.full(ps, np.nan)
    # neighbours along the innermost axis differ by 1 or 2 (mod 4), every value occurs
    inner = (np.indices(dims).sum(axis=0) + np.arange(int(np.prod(dims))).reshape(dims) // 7) % 4
    M.interior(shape, k)[...] = inner
    for a in (prev, cur, k):
        a.setflags(write=False)
    return prev, cur, k


def bits_of(t):
    return t.view(__import__("torch").int64)


def same_bits(a, b):
    import torch

    return torch.equal(bits_of(a.contiguous()), bits_of(b.contiguous()))


class Grids:
    """prev, cur, k and one or two more buffers carved out of one poisoned allocation"""

    def __init__(self, L, shape, dims, offset, prev, cur, k, n_buffers=4):
        import torch
        from arena import carve

        self.L, self.shape, self.dims = L, shape, dims
        self.arena = carve(L.padded_shape(shape, dims), "f64", n_buffers=n_buffers, offset_bytes=offset)
        self.prev, self.cur, self.k = self.arena.views[0], self.arena.views[1], self.arena.views[2]
        self.spare = self.arena.views[3:]
        self.h_prev = torch.from_numpy(np.array(prev)).cuda()
        self.h_cur = torch.from_numpy(np.array(cur)).cuda()
        self.h_k = torch.from_numpy(np.array(k)).cuda()
        self.k.copy_(self.h_k)
        self.reset()

    def reset(self, spare=FILL):
        self.prev.copy_(self.h_prev)
        self.cur.copy_(self.h_cur)
        for s in self.spare:
            s.fill_(spare)

    def check(self, what, kept=()):
        """guards intact; k, and every buffer of `kept` (pairs of a view and what it held), unchanged bit for bit"""
        import torch
        from arena import assert_guards_intact

        torch.cuda.synchronize()
        assert_guards_intact(self.arena, what)
        for i, (view, was) in enumerate(((self.k, self.h_k),) + tuple(kept)):
            assert torch.equal(bits_of(view), bits_of(was)), f"{what}: read-only buffer {i} was written"


def single_steps(p, prev, cur, k, b, c, times, periodic=False):
    """the engine's own loop of single in-place steps; returns the buffers of (level times - 1, level times)"""
    lv = [prev, cur]
    if periodic and times:
        p.halo(lv[1], "wrap")
    for _ in range(times):
        p.step_wave(lv[1], lv[0], k, b, c)
        if periodic:
            p.halo(lv[0], "wrap")
        lv.reverse()
    return lv


# ---- 1. the exact integer model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_single_step_equals_the_integer_model(L, shape, dims, regions):
    """fingerprint taps (pairwise distinct, no symmetry left), small integers, k in 0 .. 3 that differs per cell with NaN in its
    halo: the region equals k * apply(cur) + b * cur + c * prev in int64 with ==; every other cell of prev keeps its value"""
    import torch

    prev, cur, k = int_data(shape, dims)
    w = M.fingerprint_taps(support(L, shape))
    s_cur = M.apply(shape, cur, w)
    ki, ui, pi = M.ints(M.interior(shape, k)), M.interior(shape, M.ints(cur)), M.interior(shape, M.ints(prev))
    assert len(np.unique(ki)) == min(4, ki.size) and (ki.size < 2 or (np.diff(ki.ravel()) != 0).any())
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, k)
        p = L.Plan(shape, dims).set_weights(w.astype(np.float64))
        sig = p.kernel_signature
        for b, c in INT_COEFS:
            M.assert_exact(f"{shape} {dims}", [3 * M.magnitude(shape, cur, w) + abs(b) * np.abs(ui) + abs(c) * np.abs(pi)])
            whole = ki * s_cur + b * ui + c * pi
            for begin, end, entry in [(x, y, "region") for x, y in regions] + [(0, dims[0], "whole")]:
                g.reset()
                if entry == "whole":
                    p.step_wave(g.cur, g.prev, g.k, b, c)
                else:
                    p.step_wave_region(g.cur, g.prev, g.k, b, c, begin, end)
                g.check(f"{shape} {dims} b={b} c={c} [{begin}, {end})", kept=[(g.cur, g.h_cur)])
                got = g.prev.cpu().numpy()
                assert M.exactly(M.interior(shape, got)[begin:end], whole[begin:end]), (off, b, c, begin, end, entry)
                keep = torch.ones_like(g.prev, dtype=torch.bool)
                L.interior(shape, keep)[begin:end] = False
                assert torch.equal(bits_of(g.prev)[keep], bits_of(g.h_prev)[keep]), (off, b, c, begin, end, "a cell outside the region")
        assert p.kernel_signature == sig and p.wave_depth == wave_depth_of(dims)


# ---- 2. the bit contract on real data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_single_step_is_the_plain_sweep_then_five_separate_operations(L, shape, dims, regions):
    """bit for bit on seeded real data: every cell of prev, so the halo and the rows outside the region too.  Expected: the plain
    step_region into a spare buffer, then k * spare, b * cur, their sum, c * prev and the last sum as separate eager torch
    operations on the region's interior"""
    prev, cur, k = host_data(shape, dims)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, k)
        p = L.Plan(shape, dims).set_weights(real_taps(L, shape))
        sig = p.kernel_signature
        tmp = g.spare[0]
        for b, c in COEFS:
            for begin, end, whole in [(x, y, False) for x, y in regions] + [(0, dims[0], True)]:  # (last: the whole-grid entry)
                g.reset()
                p.step_region(g.cur, tmp, begin, end)
                want = g.h_prev.clone()
                x = L.interior(shape, g.h_k)[begin:end] * L.interior(shape, tmp)[begin:end]  # one rounding
                y = b * L.interior(shape, g.h_cur)[begin:end]                                  # another
                s = x + y                                                                      # another
                z = c * L.interior(shape, g.h_prev)[begin:end]                                 # another
                L.interior(shape, want)[begin:end] = s + z                                     # and the last
                if whole:
                    p.step_wave(g.cur, g.prev, g.k, b, c)
                else:
                    p.step_wave_region(g.cur, g.prev, g.k, b, c, begin, end)
                g.check(f"{shape} {dims} b={b} c={c} [{begin}, {end})", kept=[(g.cur, g.h_cur)])
                bad = int((bits_of(g.prev) != bits_of(want)).sum())
                assert bad == 0, (off, b, c, begin, end, whole, bad)
        assert p.kernel_signature == sig and p.wave_depth == wave_depth_of(dims)


# ---- 3. the two-step launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", FUSED, ids=FUSED_IDS)
def test_two_step_launch_is_two_single_steps(L, shape, dims, regions):
    """out1 and out2 on the rows of the region against whole-grid single steps; cells outside the region and every halo cell of both
    outputs keep the fill value; prev, cur and k are unchanged"""
    import torch

    prev, cur, k = host_data(shape, dims)
    w = real_taps(L, shape)
    for off in OFFSETS:
        g = Grids(L, shape, dims, off, prev, cur, k, n_buffers=5)
        o1, o2 = g.spare
        p = L.Plan(shape, dims).set_weights(w)
        assert p.wave_depth == 2
        for b, c in COEFS:
            l1 = g.h_prev.clone()
            p.step_wave(g.h_cur, l1, g.h_k, b, c)   # level 1, prev's halo
            l2 = g.h_cur.clone()
            p.step_wave(l1, l2, g.h_k, b, c)        # level 2, cur's halo
            for begin, end in regions:
                want1, want2 = torch.full_like(l1, FILL), torch.full_like(l2, FILL)
                L.interior(shape, want1)[begin:end] = L.interior(shape, l1)[begin:end]
                L.interior(shape, want2)[begin:end] = L.interior(shape, l2)[begin:end]
                g.reset()
                p.step2_wave_region(g.prev, g.cur, g.k, o1, o2, b, c, begin, end)
                g.check(f"{shape} two steps {b} {c} [{begin}, {end})", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                where = (off, b, c, begin, end)
                assert same_bits(o1, want1), where + (int((bits_of(o1) != bits_of(want1)).sum()),)
                assert same_bits(o2, want2), where + (int((bits_of(o2) != bits_of(want2)).sum()),)
            if (0, dims[0]) in regions:  # the whole-grid entry is the same launch
                g.reset()
                p.step2_wave(g.prev, g.cur, g.k, o1, o2, b, c)
                g.check("whole grid", kept=[(g.prev, g.h_prev), (g.cur, g.h_cur)])
                assert same_bits(L.interior(shape, o1), L.interior(shape, l1)) and same_bits(L.interior(shape, o2), L.interior(shape, l2))
                halo = torch.ones_like(o1, dtype=torch.bool)
                L.interior(shape, halo)[...] = False
                assert bool((o1[halo] == FILL).all()) and bool((o2[halo] == FILL).all())


# ---- 4. the run -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["reference", "dirichlet", "periodic"])
@pytest.mark.parametrize("shape,dims,regions", RUNS, ids=RUN_IDS)
def test_run_is_that_many_single_steps(L, shape, dims, regions, bc):
    """both final levels, in the buffers the contract names; with and without the scratch grids, a second time on the same plan, and
    on 3D plans also with option leap3 = 1, under which the wave run still takes single steps"""
    prev, cur, k = host_data(shape, dims)
    w = real_taps(L, shape)
    b, c = 1.9, -0.9
    g = Grids(L, shape, dims, OFFSETS[0], prev, cur, k)
    ref = L.Plan(shape, dims).set_weights(w).set_boundary(bc)
    want = {}
    for times in TIMES:
        g.reset()
        lv = single_steps(ref, g.prev, g.cur, g.k, b, c, times, periodic=bc == "periodic")
        assert (lv[1] is g.cur) == (times % 2 == 0)
        want[times] = (g.prev.clone(), g.cur.clone())
    for leap3 in (0, 1) if len(dims) == 3 else (0,):
        for scratch in (0, 1):
            p = L.Plan(shape, dims).set_weights(w).set_boundary(bc).set_option("scratch", scratch)
            if leap3:
                p.set_option("leap3", 1)
                assert p.wave_depth == 1 and p.leapfrog_depth == (2 if dims[2] % 2 == 0 else 1)  # (leap3 moves the leapfrog depth alone)
            sig, depth = p.kernel_signature, p.leapfrog_depth
            for times in TIMES + (8, 13):
                g.reset()
                p.run_wave(g.prev, g.cur, g.k, b, c, times)
                g.check(f"{shape} {bc} scratch={scratch} leap3={leap3} run_wave({times})")
                for name, got, exp in zip(("prev", "cur"), (g.prev, g.cur), want[times]):
                    assert same_bits(got, exp), (bc, scratch, leap3, times, name, int((bits_of(got) != bits_of(exp)).sum()))
            assert p.kernel_signature == sig and p.leapfrog_depth == depth


# ---- 5. the cross-check with an existing kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,regions", CASES, ids=IDS)
def test_constant_k_and_no_centre_term_is_the_scaled_leapfrog_step(L, shape, dims, regions):
    """k = a on every cell and b = 0: on finite data the step equals step_leapfrog_src(d_f=None, a, c) as numbers (==: the b * u
    term is a signed zero, which may turn a -0.0 into 0.0 and moves nothing else)"""
    import torch

    prev, cur, _ = host_data(shape, dims)
    p = L.Plan(shape, dims).set_weights(real_taps(L, shape))
    for a, c in ((0.7, 0.3), (1.0, -1.0)):
        g = Grids(L, shape, dims, OFFSETS[1], prev, cur, np.full(M.padded_shape(shape, dims), a))
        for begin, end in regions:
            g.reset()
            want = g.h_prev.clone()
            p.step_leapfrog_src_region(g.h_cur, want, None, a, c, begin, end)
            p.step_wave_region(g.cur, g.prev, g.k, 0.0, c, begin, end)
            g.check(f"{shape} {dims} a={a} c={c} [{begin}, {end})", kept=[(g.cur, g.h_cur)])
            assert bool(torch.isfinite(want).all()) and bool((g.prev == want).all()), (a, c, begin, end, int((g.prev != want).sum()))


# ---- 6. the host-buffer operator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims", [("1d1r", (37,)), ("1d2r", (64,)), ("star2d1r", (20, 130)), ("box2d3r", (9, 14)), ("star2d3r", (9, 13)),
                                        ("star3d1r", (5, 6, 10)), ("box3d1r", (4, 5, 7))],
                         ids=["1d1r", "1d2r", "star2d1r", "box2d3r", "star2d3r-odd", "star3d1r", "box3d1r-odd"])
def test_run_host_wave_equals_the_integer_model_loop(L, shape, dims):
    """laplacian = 1, default params (integer tables), 3 steps, integer kappa <= 2, data <= 3 in magnitude: level 3 equals the int64
    loop new = kappa * apply(cur, w') + 2 cur - prev with w' the zero-sum taps, every level inside the halo of the buffer it lives in"""
    rng = np.random.default_rng(M.seed_of("host-wave", shape, dims))
    ps = M.padded_shape(shape, dims)
    cur = rng.integers(-3, 4, ps).astype(np.float64)
    prev = rng.integers(-3, 4, ps).astype(np.float64)
    kappa = np.full(ps, np.nan)  # (the halo of kappa is never read)
    M.interior(shape, kappa)[...] = rng.integers(0, 3, dims)
    w = M.ints(L.effective_weights(shape)[:L.ops.ntaps(shape)]).copy()
    total = 0
    for t in w:  # sequentially, in table order
        total += int(t)
    assert abs(total) < 2 ** 20  # (so the fp64 sum the operator forms is this integer)
    w[w.size // 2] -= total
    assert w.sum() == 0
    ki = M.ints(M.interior(shape, kappa))
    lv = [M.ints(prev), M.ints(cur)]             # lv[1] the newest level
    mag = [np.abs(lv[0]), np.abs(lv[1])]         # the same loop on absolute values: bounds every partial sum
    for _ in range(3):
        new = ki * M.apply(shape, lv[1], w) + 2 * M.interior(shape, lv[1]) - M.interior(shape, lv[0])
        bound = ki * M.magnitude(shape, mag[1], w) + 2 * M.interior(shape, mag[1]) + M.interior(shape, mag[0])
        M.assert_exact(f"{shape} {dims}", [bound])
        lv = [lv[1], M.with_halo(shape, new, lv[0])]
        mag = [mag[1], M.with_halo(shape, bound, mag[0])]
    out, info = L.run_host_wave(shape, cur, prev, kappa, b=2.0, c=-1.0, laplacian=True, times=3)
    assert M.exactly(out, lv[1]), (shape, dims)
    assert info.steps_per_launch == wave_depth_of(dims) and info.hbm_gbs > 0 and out.shape == ps
    # without the zero-sum form the raw taps run: another result on this data
    raw, _ = L.run_host_wave(shape, cur, prev, kappa, b=2.0, c=-1.0, laplacian=False, times=3)
    assert not np.array_equal(M.interior(shape, raw), M.interior(shape, out))


# ---- 7. stream ordering -----------------------------------------------------------------------------------------------------------
GATE_MS = 60.0


def _spin_cycles_per_ms(torch):
    def timed(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(1000)  # (the spin kernel's code object)
    cycles = 10_000_000
    ms = timed(cycles)
    if ms < 20.0:
        cycles = int(cycles * 40.0 / max(ms, 0.01))
        ms = timed(cycles)
    assert 1.0 < ms < 2000.0, f"torch.cuda._sleep({cycles}) took {ms} ms: not a usable gate"
    return cycles / ms


def _independent_stream(torch, null, per_ms):
    """a side stream that is served while a gate is pending on the null stream and the other way round (streams that share a
    hardware queue run one behind the other whatever the code does: such a pair shows nothing); every stream has run something
    before its first gate"""
    tiny = (torch.arange(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda"))

    def passes(gated, other):
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        with torch.cuda.stream(gated):
            torch.cuda._sleep(int(GATE_MS * per_ms))
        t0 = time.perf_counter()
        with torch.cuda.stream(other):
            tiny[1].copy_(tiny[0])
            done.record()
        done.synchronize()
        ok = (not gated.query()) and (time.perf_counter() - t0) * 1e3 < GATE_MS / 4
        torch.cuda.synchronize()
        return ok

    for _ in range(8):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            tiny[1].copy_(tiny[0])
        torch.cuda.synchronize()
        if passes(s, null) and passes(null, s):
            return s
    raise AssertionError("no side stream is served independently of the null stream: the gate would show nothing")


@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("entry", ["step_wave", "step2_wave", "run_wave"])
def test_calls_are_ordered_on_their_stream_and_on_nothing_else(L, scenario, entry):
    """One call on a non-blocking stream S while a gate (a bounded spin) is pending.  A: the gate on S, then on S the uploads over
    poisoned grids, the call, a snapshot, poison again -- work that is not ordered on S runs before the input exists.  B: the gate on
    the null stream, the same sequence on S -- work left on the null stream lands on the poison S has put back.  The snapshot
    equals the ungated call of a twin plan bit for bit; afterwards the grids hold nothing but poison; the call did not block."""
    import torch
    from arena import assert_guards_intact, carve

    shape, dims, times = "star2d1r", (70, 260), 9
    b, c = 1.9, -0.9
    prev, cur, k = host_data(shape, dims)
    staged = [torch.from_numpy(np.array(x)).cuda() for x in (prev, cur, k)]
    ar = carve(L.padded_shape(shape, dims), "f64", n_buffers=5, offset_bytes=OFFSETS[0])
    v = ar.views

    def make_plan():
        p = L.Plan(shape, dims).set_weights(real_taps(L, shape))
        p.prepare_wave(times)
        return p

    def call(p, stream):
        if entry == "step_wave":
            p.step_wave(v[1], v[0], v[2], b, c, stream=stream)
        elif entry == "step2_wave":
            p.step2_wave(v[0], v[1], v[2], v[3], v[4], b, c, stream=stream)
        else:
            p.run_wave(v[0], v[1], v[2], b, c, times, stream=stream)

    def upload():
        for view, src in zip(v[:3], staged):
            view.copy_(src, non_blocking=True)

    null = torch.cuda.default_stream()
    per_ms = _spin_cycles_per_ms(torch)
    S = _independent_stream(torch, null, per_ms)
    # the ungated call of a twin plan on an idle device: the expected bits (it also loads the kernels' code objects and, on the
    # plan under test, makes the first-need allocations before any gate is pending)
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
    assert not bool((expected[ar.spans[0][0]:ar.spans[0][1]] == ar.poison).all())

    snap = torch.empty_like(ar.flat)
    ar.flat.fill_(ar.poison)
    torch.cuda.synchronize()
    gated = S if scenario == "A" else null
    with torch.cuda.stream(gated):
        torch.cuda._sleep(int(GATE_MS * per_ms))
    t_gate = time.perf_counter()
    with torch.cuda.stream(S):
        upload()
        call(plan, S)
        busy_after = not gated.query()
        host_ms = (time.perf_counter() - t_gate) * 1e3
        snap.copy_(ar.flat, non_blocking=True)
        ar.flat.fill_(ar.poison)
    if scenario == "B":
        S.synchronize()  # (bounded: at the latest when the gate has run out)
        assert not null.query() and (time.perf_counter() - t_gate) * 1e3 < GATE_MS / 2, \
            "S did not drain while the null stream's gate was pending: the case shows nothing about the library"
    torch.cuda.synchronize()
    print(f"stream-order {entry} {scenario}: host {host_ms:.2f} ms behind the gate, busy after: {busy_after}")
    assert host_ms < GATE_MS / 2, "the host was held up for longer than half the gate: the case shows nothing"
    assert busy_after, "the call blocked until the gated stream had drained"
    bad = snap != expected
    assert not bool(bad.any()), f"{int(bad.sum())} elements differ from the ungated call's, {int((snap == ar.poison).sum() - (expected == ar.poison).sum())} more of them poison"
    assert bool((ar.flat == ar.poison).all()), "something wrote into the grids after the caller's stream had put the poison back"
