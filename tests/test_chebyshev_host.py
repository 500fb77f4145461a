"""CPU tests of the scaled leapfrog step with a source and of the Chebyshev entries built on it (lora_plan_step_leapfrog_src ...
lora_run_host_chebyshev; include/lorastencil.h): the symbols, the status codes in their documented order on addresses
nobody dereferences, the coefficient schedule against its recurrence, that no call changes what a plan resolves to, the loud
failure without a device, and the CLI's --chebyshev flag.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C, D, F = A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (4 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

ENTRIES = ["lora_plan_step_leapfrog_src", "lora_plan_step_leapfrog_src_region", "lora_plan_step2_leapfrog_src",
           "lora_plan_step2_leapfrog_src_region", "lora_plan_run_leapfrog_src", "lora_chebyshev_coeffs", "lora_plan_run_chebyshev_until",
           "lora_run_host_chebyshev"]

# every key lora_plan_get_option answers in the shipped library
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "spans3", "torus", "tapset", "variant",
        "fused_eval", "boundary", "fused_residual", "source"]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature, p.leapfrog_depth


def dp(x):
    return x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def until(L, tol=1e-6, rtol=0.0, norm=0, check_every=20, max_times=100):
    from lorastencil_amd import _lib

    return _lib.Until(tol, rtol, norm, check_every, max_times)


def test_symbols_are_exported(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    for name in ENTRIES:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert ("int lora_plan_step_leapfrog_src(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_f, double a, double c, "
            "void *stream);") in header
    assert "int lora_chebyshev_coeffs(double rho, int first_step, int count, double *a, double *c);" in header
    for name in ("step_leapfrog_src", "step_leapfrog_src_region", "step2_leapfrog_src", "step2_leapfrog_src_region", "run_leapfrog_src",
                 "run_chebyshev_until"):
        assert callable(getattr(L.Plan, name)), name
    assert callable(L.chebyshev_coeffs) and callable(L.run_host_chebyshev)


def test_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    p = L.Plan("star2d1r", (32, 64))
    h = p._h
    one, two = np.array([1.0]), np.array([1.0, nan, 0.5])
    neg = np.array([-1.0])
    r = _lib.UntilResult()
    u = until(L)
    # -- LORA_EINVAL: null plan / pointer (d_f may be null), non-finite a or c, bad range, times < 0, ncoef < 1, equal buffers
    assert lib.lora_plan_step_leapfrog_src(None, A, B, F, 1.0, -1.0, None) == E
    assert lib.lora_plan_step_leapfrog_src_region(None, A, B, F, 1.0, -1.0, 0, 1, None) == E
    assert lib.lora_plan_step2_leapfrog_src(None, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, None) == E
    assert lib.lora_plan_step2_leapfrog_src_region(None, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, 0, 1, None) == E
    assert lib.lora_plan_run_leapfrog_src(None, A, B, F, dp(one), dp(neg), 1, 1, None) == E
    assert lib.lora_plan_run_chebyshev_until(None, A, B, F, 0.5, ctypes.byref(u), ctypes.byref(r), None) == E
    for f in (F, None):
        for cur, prev in ((None, B), (A, None), (A, A)):
            assert lib.lora_plan_step_leapfrog_src(h, cur, prev, f, 1.0, -1.0, None) == E
            assert lib.lora_plan_run_leapfrog_src(h, prev, cur, f, dp(one), dp(neg), 1, 3, None) == E
            assert lib.lora_plan_run_chebyshev_until(h, prev, cur, f, 0.5, ctypes.byref(u), ctypes.byref(r), None) == E
    # d_f equal to another buffer of the call
    assert lib.lora_plan_step_leapfrog_src(h, A, B, B, 1.0, -1.0, None) == E   # d_f == d_prev
    assert lib.lora_plan_step_leapfrog_src(h, A, B, A, 1.0, -1.0, None) == E   # d_f == d_cur
    assert lib.lora_plan_run_leapfrog_src(h, A, B, A, dp(one), dp(neg), 1, 3, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, B, dp(one), dp(neg), 1, 3, None) == E
    assert lib.lora_plan_run_chebyshev_until(h, A, B, A, 0.5, ctypes.byref(u), ctypes.byref(r), None) == E
    assert lib.lora_plan_run_chebyshev_until(h, A, B, B, 0.5, ctypes.byref(u), ctypes.byref(r), None) == E
    for bad in (inf, -inf, nan):
        assert lib.lora_plan_step_leapfrog_src(h, A, B, F, bad, -1.0, None) == E
        assert lib.lora_plan_step_leapfrog_src(h, A, B, F, 1.0, bad, None) == E
        for k in range(4):
            coef = [1.0, -1.0, 1.0, -1.0]
            coef[k] = bad
            assert lib.lora_plan_step2_leapfrog_src(h, A, B, F, C, D, *coef, None) == E
        assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(np.array([bad])), dp(neg), 1, 3, None) == E
        assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(one), dp(np.array([bad])), 1, 3, None) == E
    # a non-finite entry counts only among those that will be used: two[1] is step 1's (a run of no steps uses none)
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(two), dp(two), 3, 2, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(two), dp(two), 3, 0, None) == 0
    for begin, end in ((-1, 4), (0, 33), (5, 4)):
        assert lib.lora_plan_step_leapfrog_src_region(h, A, B, F, 1.0, -1.0, begin, end, None) == E
        assert lib.lora_plan_step2_leapfrog_src_region(h, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, begin, end, None) == E
    p1 = L.Plan("1d1r", (300,))
    assert lib.lora_plan_step_leapfrog_src_region(p1._h, A, B, F, 1.0, -1.0, 3, 10, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(one), dp(neg), 1, -1, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(one), dp(neg), 0, 1, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, None, dp(neg), 1, 1, None) == E
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(one), None, 1, 1, None) == E
    bufs = [A, B, F, C, D]
    for i in range(5):
        for j in range(i + 1, 5):
            args = list(bufs)
            args[j] = args[i]
            assert lib.lora_plan_step2_leapfrog_src(h, *args, 1.0, -1.0, 0.5, 0.5, None) == E, (i, j)
    for i in (0, 1, 3, 4):
        args = list(bufs)
        args[i] = None
        assert lib.lora_plan_step2_leapfrog_src(h, *args, 1.0, -1.0, 0.5, 0.5, None) == E, i
    # run_chebyshev_until: rho outside [0, 1), the rules of lora_until, null u / r
    for rho in (-0.1, 1.0, nan, inf):
        assert lib.lora_plan_run_chebyshev_until(h, A, B, F, rho, ctypes.byref(u), ctypes.byref(r), None) == E
    for bad_u in (until(L, check_every=3), until(L, check_every=0), until(L, max_times=-1), until(L, norm=7), until(L, tol=nan),
                  until(L, rtol=-1.0)):
        assert lib.lora_plan_run_chebyshev_until(h, A, B, F, 0.5, ctypes.byref(bad_u), ctypes.byref(r), None) == E
    assert lib.lora_plan_run_chebyshev_until(h, A, B, F, 0.5, None, ctypes.byref(r), None) == E
    assert lib.lora_plan_run_chebyshev_until(h, A, B, F, 0.5, ctypes.byref(u), None, None) == E
    # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument on a plan without the kernels, with a misaligned buffer
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    assert lib.lora_plan_step_leapfrog_src(bf._h, A + 8, A + 8, F, 1.0, -1.0, None) == E
    assert lib.lora_plan_step_leapfrog_src(bf._h, A, B, F + 8, nan, -1.0, None) == E
    assert lib.lora_plan_run_leapfrog_src(bf._h, A, B, F, dp(one), dp(neg), 1, -1, None) == E
    assert lib.lora_plan_run_chebyshev_until(bf._h, A, B + 8, F, 1.0, ctypes.byref(u), ctypes.byref(r), None) == E
    # -- LORA_EUNSUPPORTED: a misaligned buffer
    for cur, prev, f in ((A + 8, B, F), (A, B + 8, F), (A, B, F + 8)):
        assert lib.lora_plan_step_leapfrog_src(h, cur, prev, f, 1.0, -1.0, None) == U and "16-byte" in lib.lora_last_error().decode()
        assert lib.lora_plan_run_leapfrog_src(h, prev, cur, f, dp(one), dp(neg), 1, 2, None) == U
        assert lib.lora_plan_run_chebyshev_until(h, prev, cur, f, 0.5, ctypes.byref(u), ctypes.byref(r), None) == U
    for i in range(5):
        args = list(bufs)
        args[i] += 8
        assert lib.lora_plan_step2_leapfrog_src(h, *args, 1.0, -1.0, 0.5, 0.5, None) == U, i
    # -- LORA_EUNSUPPORTED: the plans without the kernels -- a plan on which set_source was called among them
    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    src = L.Plan("star2d1r", (32, 64)).set_source(D)
    for q in (bf, mfma, src):
        n = q.dims[0]
        for f in (F, None):
            assert lib.lora_plan_step_leapfrog_src(q._h, A, B, f, 1.0, -1.0, None) == U
            assert lib.lora_plan_step_leapfrog_src_region(q._h, A, B, f, 1.0, -1.0, 0, n, None) == U
            assert lib.lora_plan_run_leapfrog_src(q._h, A, B, f, dp(one), dp(neg), 1, 4, None) == U
            assert lib.lora_plan_run_leapfrog_src(q._h, A, B, f, dp(one), dp(neg), 1, 0, None) == U
            assert lib.lora_plan_run_chebyshev_until(q._h, A, B, f, 0.5, ctypes.byref(u), ctypes.byref(r), None) == U
            if len(q.dims) == 2:
                assert lib.lora_plan_step2_leapfrog_src(q._h, A, B, f, C, D, 1.0, -1.0, 0.5, 0.5, None) == U
    assert src.leapfrog_depth == 0 and src.get_option("source") == 1
    # -- the two-step entries on plans that have no two-step kernel
    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8))]:
        q = L.Plan(shape, dims)
        assert q.leapfrog_depth == 1
        assert lib.lora_plan_step2_leapfrog_src(q._h, A, B, F, C, D, 1.0, -1.0, 0.5, 0.5, None) == U, shape
        assert lib.lora_plan_step2_leapfrog_src_region(q._h, A, B, None, C, D, 1.0, -1.0, 0.5, 0.5, 0, 2, None) == U, shape
    # -- nothing to do is no error and needs no device
    assert lib.lora_plan_run_leapfrog_src(h, A, B, F, dp(one), dp(neg), 1, 0, None) == 0
    assert lib.lora_plan_step_leapfrog_src_region(h, A, B, F, 1.0, -1.0, 7, 7, None) == 0
    assert lib.lora_plan_step_leapfrog_src_region(h, A, B, None, 1.0, -1.0, 7, 7, None) == 0
    assert lib.lora_plan_step2_leapfrog_src_region(h, A, B, F, C, D, 1.0, -1.0, 0.5, 0.5, 7, 7, None) == 0


def omegas(rho, n):
    """the recurrence in Python floats: w(1) .. w(n)"""
    w = [1.0]
    if n > 1:
        w.append(1.0 / (1.0 - rho * rho / 2.0))
    while len(w) < n:
        w.append(1.0 / (1.0 - rho * rho * w[-1] / 4.0))
    return w[:n]


@pytest.mark.parametrize("rho", [0.0, 0.3, 0.9, 0.99882, 0.9999999])
def test_coefficients_follow_the_recurrence(L, rho):
    n = 400
    a, c = L.chebyshev_coeffs(rho, 1, n)
    assert a.shape == c.shape == (n,)
    assert a[0] == 1.0 and c[0] == 0.0 and math.copysign(1.0, c[0]) == 1.0
    want = np.array(omegas(rho, n))
    assert np.all(np.abs(a - want) <= 1e-15 * np.abs(want))
    assert np.array_equal(c, 1.0 - a)
    # w decreases from w(2) on towards 2 / (1 + sqrt(1 - rho^2))
    limit = 2.0 / (1.0 + math.sqrt(1.0 - rho * rho))
    assert np.all(np.diff(a[1:]) <= 0.0)
    assert np.all(a[1:] >= limit * (1.0 - 1e-15))
    if rho > 0.0:
        assert a[1] > a[-1] and a[1] > limit
    else:
        assert np.all(a == 1.0)
    # a window equals the tail of the full schedule, bit for bit
    a7, c7 = L.chebyshev_coeffs(rho, 7, 50)
    assert np.array_equal(a7, a[6:56]) and np.array_equal(c7, c[6:56])
    a0, c0 = L.chebyshev_coeffs(rho, 3, 0)
    assert a0.size == 0 and c0.size == 0


def test_coefficients_status_codes(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E = _lib.LORA_EINVAL
    a, c = np.zeros(4), np.zeros(4)
    for rho in (-0.1, 1.0, float("nan"), float("inf"), 1.5):
        assert lib.lora_chebyshev_coeffs(rho, 1, 4, dp(a), dp(c)) == E, rho
    assert lib.lora_chebyshev_coeffs(0.5, 0, 4, dp(a), dp(c)) == E
    assert lib.lora_chebyshev_coeffs(0.5, -3, 4, dp(a), dp(c)) == E
    assert lib.lora_chebyshev_coeffs(0.5, 1, -1, dp(a), dp(c)) == E
    assert lib.lora_chebyshev_coeffs(0.5, 1, 4, None, dp(c)) == E
    assert lib.lora_chebyshev_coeffs(0.5, 1, 4, dp(a), None) == E
    assert lib.lora_chebyshev_coeffs(0.5, 1, 0, None, None) == 0
    assert np.all(a == 0.0) and np.all(c == 0.0)  # a refused call writes nothing
    assert lib.lora_chebyshev_coeffs(0.5, 1, 4, dp(a), dp(c)) == 0 and a[0] == 1.0
    with pytest.raises(L.LoraError):
        L.chebyshev_coeffs(1.0, 1, 3)


def test_host_entry_status_codes(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    a = np.zeros(L.padded_shape("star2d1r", (8, 16)))
    out = np.zeros_like(a)
    dims, sid = L.ops._dims_arg((8, 16)), L.ops.shape_id("star2d1r")
    r = _lib.UntilResult()
    u = until(L)
    run = lib.lora_run_host_chebyshev
    assert run(sid, None, dp(a), dp(out), None, 0.5, 1, None, None, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), None, None, 0.5, 1, None, None, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(out), None, 0.5, 1, None, None, None, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(out), None, 0.5, -1, None, None, dims, 1, None) == E
    for rho in (-0.1, 1.0, float("nan")):
        assert run(sid, dp(a), None, dp(out), None, rho, 1, None, None, dims, 1, None) == E
    assert run(sid, dp(a), None, dp(out), None, 0.5, 1, ctypes.byref(u), None, dims, 1, None) == E  # `u` needs `r`
    assert run(sid, dp(a), None, dp(out), None, 0.5, 1, ctypes.byref(until(L, check_every=3)), ctypes.byref(r), dims, 1, None) == E
    assert L.set_default_source(a) is None
    try:
        assert run(sid, dp(a), None, dp(out), None, 0.5, 1, None, None, dims, 1, None) == U
        assert "source" in lib.lora_last_error().decode()
    finally:
        assert L.set_default_source(None) is a
    with pytest.raises(ValueError):
        L.run_host_chebyshev("star2d1r", a, 0.5, times=1, source=np.zeros((3, 3)))


@pytest.mark.parametrize("shape,dims", [("1d2r", (300,)), ("star2d1r", (64, 128)), ("box2d3r", (64, 127)), ("box3d1r", (16, 16, 32))],
                         ids=["1d", "2d", "2d-odd", "3d"])
def test_calls_leave_the_plan_as_it_was(L, shape, dims):
    """f, a, c and the buffers are call arguments: every key's value, the kernel name, the signature and the leapfrog depth stay"""
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p = L.Plan(shape, dims)
    before = state(p)
    n = dims[0]
    a, c = L.chebyshev_coeffs(0.9, 1, 9)
    r, u = _lib.UntilResult(), until(L)
    if not has_gpu():  # (with a device these would launch on addresses nobody owns; tests/test_gpu_leapfrog_src.py covers them there)
        lib.lora_plan_step_leapfrog_src(p._h, A, B, F, 1.0, -1.0, None)
        lib.lora_plan_step_leapfrog_src_region(p._h, A, B, None, 0.7, 0.3, 0, n, None)
        lib.lora_plan_step2_leapfrog_src(p._h, A, B, F, C, D, 1.0, -1.0, 0.7, 0.3, None)
        lib.lora_plan_step2_leapfrog_src_region(p._h, A, B, None, C, D, 1.0, -1.0, 0.7, 0.3, 0, n, None)
        lib.lora_plan_run_leapfrog_src(p._h, A, B, F, dp(a), dp(c), 9, 9, None)
        lib.lora_plan_run_chebyshev_until(p._h, A, B, F, 0.9, ctypes.byref(u), ctypes.byref(r), None)
    assert lib.lora_plan_step_leapfrog_src_region(p._h, A, B, F, 0.7, 0.3, 2, 2, None) == 0
    assert lib.lora_plan_run_leapfrog_src(p._h, A, B, F, dp(a), dp(c), 9, 0, None) == 0
    assert state(p) == before
    assert state(p) == state(L.Plan(shape, dims))


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    a, c = L.chebyshev_coeffs(0.9, 1, 9)
    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8)), ("star3d1r", (3, 5, 7))]:
        for bc in ("reference", "periodic"):
            for f in (F, None):
                p = L.Plan(shape, dims).set_boundary(bc)
                calls = [lambda: p.step_leapfrog_src(A, B, f), lambda: p.step_leapfrog_src_region(A, B, f, 0.7, 0.3, 0, 2),
                         lambda: p.run_leapfrog_src(A, B, f, 1.0, -1.0, 1), lambda: p.run_leapfrog_src(A, B, f, a, c, 9),
                         lambda: p.run_chebyshev_until(A, B, f, 0.9, 1e-6, check_every=2, max_times=4)]
                if p.leapfrog_depth == 2:
                    calls.append(lambda: p.step2_leapfrog_src(A, B, f, C, D, 1.0, -1.0, 0.7, 0.3))
                for i, call in enumerate(calls):
                    with pytest.raises(L.LoraError) as e:
                        call()
                    assert e.value.status == _lib.LORA_ENODEVICE, (shape, bc, i)
    g = np.zeros(L.padded_shape("star2d1r", (32, 64)))
    for kw in ({"times": 1}, {"times": 1, "source": g}, {"tol": 1e-6, "check_every": 2, "max_times": 4}):
        with pytest.raises(L.LoraError) as e:
            L.run_host_chebyshev("star2d1r", g, 0.9, **kw)
        assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_chebyshev_parse_errors_and_refusals(engine_built):
    need = "Invalid argument: --chebyshev=RHO needs a number RHO with 0 <= RHO < 1.\n"
    for bad in ("--chebyshev=", "--chebyshev=abc", "--chebyshev=0.5x", "--chebyshev=1", "--chebyshev=1.0", "--chebyshev=-0.1",
                "--chebyshev=nan", "--chebyshev=inf", "--chebyshev=2"):
        rc, out, err = cli(2, "star2d1r", "64", "64", "4", bad)
        assert rc == 1 and err == need and out == "", bad
    rc, out, err = cli(2, "star2d1r", "64", "64", "4", "--chebyshev")
    assert rc == 1 and err == "Unknown option: --chebyshev\n" and out == ""
    refused = "--chebyshev runs on one GPU in fp64"
    for extra in (["--gpus=2"], ["--gpus=1"], ["--grid=1x2"], ["--check"], ["--leapfrog"], ["--leapfrog=-0.5"]):
        # (with --leapfrog, --until and --source meet --leapfrog's own, older refusal first: checked below)
        for more in ([], ["--until=1e-9"], ["--source=const:1"]) if "leapfrog" not in extra[0] else ([],):
            rc, out, err = cli(2, "star2d1r", "64", "64", "4", "--chebyshev=0.9", *extra, *more)
            assert rc == 1 and err.startswith(refused) and err.count("\n") == 1 and out == "", (extra, more)
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--chebyshev=0.9")
    assert rc == 1 and err.startswith(refused) and err.count("\n") == 1 and out == ""
    # the --leapfrog refusals are what they were
    rc, out, err = cli(2, "star2d1r", "64", "64", "4", "--leapfrog", "--until=1e-9", "--chebyshev=0.9")
    assert rc == 1 and err.startswith("--leapfrog runs on one GPU in fp64") and err.count("\n") == 1 and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_chebyshev_reaches_the_operator(engine_built):
    for dim, args in ((2, ["star2d1r", "62", "64", "600", "--chebyshev=0.99882", "--until=1e-10", "--source=const:0.125", "--bc=dirichlet"]),
                      (1, ["1d1r", "64", "3", "--chebyshev=0"]),
                      (3, ["box3d1r", "8", "8", "8", "2", "--chebyshev=0.5", "--source=point:1", "--bc=periodic"])):
        rc, out, _ = cli(dim, *args)
        assert out.startswith("INFO: shape = ")
        assert rc == 1 and "no HIP device" in out
