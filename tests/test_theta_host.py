"""CPU tests of the implicit stepper's boundary (include/lorastencil.h, group B "implicit time stepping"): the symbols and their
mirrors, the order of the status codes without a device, the argument rules of the driver, the refusal of taps that are not
point-symmetric, and steps == 0."""
import ctypes
import math

import numpy as np
import pytest
from conftest import has_gpu

A, B, C, D = 4096, 8192, 12288, 16384  # four distinct 16-byte aligned "device" addresses: nothing is dereferenced before a device is asked for


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def plans(L):
    from lorastencil_amd import _lib

    yes = [L.Plan("1d2r", (1027,)), L.Plan("star2d1r", (6, 10)), L.Plan("box2d3r", (70, 260)), L.Plan("box3d1r", (35, 17, 130))]
    no = [L.Plan("box3d1r", (4, 4, 8), dtype="bf16"), L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA), L.Plan("star2d1r", (32, 63))]
    return yes, no


def jacobi_plan(L):
    w = np.zeros(L.ops.ntaps("star2d1r"))
    w[[17, 23, 25, 31]] = 0.25
    return L.Plan("star2d1r", (6, 10)).set_weights(w), w


def test_every_new_symbol_is_exported_and_mirrored(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    for name in ["lora_plan_apply_dot_shift", "lora_plan_theta_start", "lora_plan_run_theta", "lora_plan_prepare_theta", "lora_run_host_theta"]:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ["ThetaResult", "run_host_theta"]:
        assert hasattr(L, name) and name in L.__all__, name
    for name in ["apply_dot_shift", "theta_start", "run_theta", "prepare_theta"]:
        assert callable(getattr(L.Plan, name)), name
    fields = ["steps_done", "breakdown", "unconverged_steps", "iterations_total", "iterations_max", "last_rr0", "last_rr", "steady"]
    assert [f[0] for f in _lib.ThetaResult._fields_] == fields
    # three ints and padding, a long long, an int and padding, two doubles, the lora_grid_diff
    assert ctypes.sizeof(_lib.ThetaResult) == 16 + 8 + 8 + 16 + ctypes.sizeof(_lib.GridDiff)
    assert L.ThetaResult._fields == tuple(fields) + ("iterations",)


def test_status_codes_come_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    yes, no = plans(L)
    p, one_d = yes[2], yes[0]
    out = _lib.GridDot()
    o = ctypes.byref(out)
    shift = lambda plan, a, b, sg=1.0, t=1.0, lo=0, hi=0, rec=o: lib.lora_plan_apply_dot_shift(plan._h if plan else None, a, b, sg, t, lo, hi, rec, None)
    start = lambda plan, u, f, r, q, t=8.0, lo=0, hi=0, rec=o: lib.lora_plan_theta_start(plan._h if plan else None, u, f, t, r, q, lo, hi, rec, None)
    # 1. null pointers, bad ranges, a begin off the granularity, equal buffers of different roles, non-finite factors: LORA_EINVAL
    assert shift(None, A, B) == E and shift(p, None, B) == E and shift(p, A, None) == E and shift(p, A, B, rec=None) == E
    assert shift(p, A, A) == E and shift(p, A, B, hi=71) == E and shift(p, A, B, lo=5, hi=3) == E and shift(one_d, A, B, lo=3, hi=9) == E
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert shift(p, A, B, sg=bad) == E and shift(p, A, B, t=bad) == E and start(p, A, B, C, D, t=bad) == E
    assert start(None, A, B, C, D) == E and start(p, None, B, C, D) == E and start(p, A, B, None, D) == E and start(p, A, B, C, None) == E
    assert start(p, A, B, C, D, rec=None) == E and start(p, A, B, C, D, hi=71) == E and start(one_d, A, B, C, D, lo=3, hi=9) == E
    bufs = [A, B, C, D]
    for i in range(4):
        for j in range(i + 1, 4):
            same = list(bufs)
            same[j] = same[i]
            assert start(p, *same) == E, (i, j)
    assert start(p, A, None, C, C) == E
    # ... also on a plan without the kernels, and with a misaligned buffer: LORA_EINVAL comes first
    assert shift(no[0], A + 8, A + 8) == E and start(no[0], A + 8, None, A + 8, D) == E
    # 2. a misaligned buffer: LORA_EUNSUPPORTED, also on a plan without the kernels
    for q in (p, no[2]):
        assert shift(q, A + 8, B) == U and shift(q, A, B + 8) == U
        for k in range(4):
            mis = list(bufs)
            mis[k] += 8
            assert start(q, *mis) == U, k
    # 3. a plan without the kernels: LORA_EUNSUPPORTED, also for the empty range
    for q in no:
        assert shift(q, A, B) == U and shift(q, A, B, lo=2, hi=2) == U
        assert start(q, A, B, C, D) == U and start(q, A, None, C, D, lo=2, hi=2) == U
        assert lib.lora_plan_prepare_theta(q._h, 3) == U
        assert "conjugate-gradient" in lib.lora_last_error().decode()
    assert lib.lora_plan_prepare_theta(p._h, -1) == E and lib.lora_plan_prepare_theta(None, 4) == E
    # a plan that carries a source has no kernels either: the source is a call argument
    s = yes[1]
    assert lib.lora_plan_set_source(s._h, A) == 0 and shift(s, B, C) == U and start(s, B, None, C, D) == U
    assert lib.lora_plan_set_source(s._h, None) == 0
    # 4. then the device: without one, LORA_ENODEVICE -- the empty range included, like the reductions
    if not has_gpu():
        N = _lib.LORA_ENODEVICE
        assert shift(p, A, B) == N and shift(p, A, B, lo=2, hi=2) == N and shift(p, A, B, 9.0, 8.0) == N
        assert start(p, A, B, C, D) == N and start(p, A, None, C, D) == N and start(p, A, B, C, D, lo=2, hi=2) == N
        assert lib.lora_plan_prepare_theta(p._h, 3) == N


def test_the_driver_checks_its_arguments_and_refuses_unsymmetric_taps(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p, w = jacobi_plan(L)
    r = _lib.ThetaResult()

    def run(plan, u, f, theta=1.0, tau=8.0, steps=3, max_iters=12, rtol=1e-2, res=r):
        return lib.lora_plan_run_theta(plan._h if plan else None, u, f, theta, tau, steps, max_iters, rtol, None,
                                       ctypes.byref(res) if res is not None else None, None)

    # the refusals the issue names, and their neighbours
    assert run(p, A, B, theta=1.5) == E and run(p, A, B, theta=-0.1) == E and run(p, A, B, theta=float("nan")) == E
    assert run(p, A, B, tau=0.0) == E and run(p, A, B, tau=-1.0) == E and run(p, A, B, tau=float("inf")) == E and run(p, A, B, tau=float("nan")) == E
    assert run(p, A, B, rtol=float("nan")) == E and run(p, A, B, rtol=-1e-3) == E and run(p, A, B, rtol=float("inf")) == E
    assert run(p, A, B, max_iters=0) == E and run(p, A, B, steps=-1) == E
    assert run(p, A, A) == E
    assert run(None, A, B) == E and run(p, None, B) == E and run(p, A, B, res=None) == E
    # the arguments come before everything else: a bad theta on a plan without the kernels with a misaligned buffer
    yes, no = plans(L)
    assert run(no[0], A + 8, B, theta=1.5) == E
    assert run(p, A + 8, B) == U and run(p, A, B + 8) == U
    for q in no:
        assert run(q, A, B) == U
    # taps that are not point-symmetric: decided on the host, before any device is asked for
    lop = w.copy()
    lop[17] = 0.125
    assert run(L.Plan("star2d1r", (6, 10)).set_weights(lop), A, B) == U
    assert "point-symmetric" in lib.lora_last_error().decode()
    for shape, dims in [("1d2r", (1027,)), ("box3d1r", (4, 4, 8))]:
        v = np.arange(1.0, L.ops.ntaps(shape) + 1)
        assert run(L.Plan(shape, dims).set_weights(v), A, None) == U
        assert run(L.Plan(shape, dims).set_weights(v), A, None, steps=0) == U  # steps == 0 excuses no refusal
        if not has_gpu():
            assert run(L.Plan(shape, dims).set_weights(v + v[::-1]), A, None) == _lib.LORA_ENODEVICE
    if not has_gpu():
        assert run(p, A, B) == _lib.LORA_ENODEVICE and run(p, A, None) == _lib.LORA_ENODEVICE
        # the host operator: arguments first, then the device, and a default source is refused
        a = np.zeros(L.padded_shape("star2d1r", (6, 10)))
        for kw in ({"theta": 1.5}, {"tau": 0.0}, {"rtol": float("nan")}, {"max_iters": 0}):
            args = {"tau": 8.0, "steps": 2}
            args.update(kw)
            with pytest.raises(L.LoraError) as e:
                L.run_host_theta("star2d1r", a, **args)
            assert e.value.status == E, kw
        with pytest.raises(L.LoraError) as e:
            L.run_host_theta("star2d1r", a, 8.0, 2)
        assert e.value.status == _lib.LORA_ENODEVICE
        old = L.set_default_source(a)
        try:
            with pytest.raises(L.LoraError) as e:
                L.run_host_theta("star2d1r", a, 8.0, 2)
            assert e.value.status == U
        finally:
            L.set_default_source(old)


def test_no_steps_is_ok_and_touches_nothing(L):
    """steps == 0 returns LORA_OK before any device is asked for -- the made-up addresses are never dereferenced -- with an
    empty result; the iteration array is not written"""
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p, _ = jacobi_plan(L)
    r = _lib.ThetaResult()
    r.steps_done = r.breakdown = r.unconverged_steps = r.iterations_max = 7
    r.iterations_total = 7
    its = (ctypes.c_int * 2)(41, 42)
    for f in (B, None):
        assert lib.lora_plan_run_theta(p._h, A, f, 0.5, 8.0, 0, 12, 1e-2, its, ctypes.byref(r), None) == _lib.LORA_OK
        assert (r.steps_done, r.breakdown, r.unconverged_steps, r.iterations_total, r.iterations_max) == (0, 0, 0, 0, 0)
        assert math.isnan(r.last_rr0) and math.isnan(r.last_rr)
        assert (r.steady.max_abs, r.steady.count, r.steady.argmax, r.steady.nonfinite) == (0.0, 0, -1, 0)
        assert list(its) == [41, 42]
    if not has_gpu():  # the wrapper, which passes a fresh iteration array
        res = p.run_theta(A, None, 8.0, 0)
        assert res.steps_done == 0 and res.iterations == () and not res.breakdown


def test_the_cli_refuses_what_an_implicit_run_cannot_be_combined_with(engine_built):
    """starting the command-line tool is what this test is about; every refusal comes before a device is asked for"""
    import os
    import subprocess
    from conftest import ROOT

    def run(dim, *args):
        p = subprocess.run([os.path.join(ROOT, "lorastencil_amd", "bin", f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=60)
        return p.returncode, p.stdout, p.stderr

    base = ("star2d1r", "64", "128", "4", "--normalize", "--bc=dirichlet", "--implicit=8")
    for other in ("--cg", "--chebyshev=0.5", "--leapfrog", "--until=1e-6", "--gpus=1", "--grid=1x1", "--check"):
        rc, _, err = run(2, *base, other)
        assert rc == 1 and err.startswith("--implicit runs a fixed number of implicit steps on one GPU in fp64: not with"), (other, err)
    rc, _, err = run(3, "box3d1r", "8", "8", "8", "2", "--implicit=8", "--dtype=bf16")
    assert rc == 1 and err.startswith("--implicit runs a fixed number")
    for bad, text in (("--implicit=0", "--implicit=TAU needs"), ("--implicit=abc", "--implicit=TAU needs"), ("--implicit=inf", "--implicit=TAU needs")):
        rc, _, err = run(2, "star2d1r", "64", "128", "4", bad)
        assert rc == 1 and text in err, (bad, err)
    for bad, text in (("--theta=1.5", "--theta=TH needs"), ("--iters=0", "--iters=N needs"), ("--rtol=-1", "--rtol=R needs"), ("--rtol=nan", "--rtol=R needs")):
        rc, _, err = run(2, *base, bad)
        assert rc == 1 and text in err, (bad, err)
    rc, _, err = run(2, "star2d1r", "64", "128", "4", "--theta=0.5")
    assert rc == 1 and "only with --implicit=TAU" in err
    if not has_gpu():
        rc, out, _ = run(2, *base, "--theta=0.5", "--iters=20", "--rtol=1e-6", "--source=const:1")
        assert rc == 1 and out.startswith("INFO: shape = star_2d1r, m = 64, n = 128, times = 4\n") and "no HIP device" in out
