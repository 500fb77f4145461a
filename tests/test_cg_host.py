"""CPU tests of the conjugate-gradient boundary (include/lorastencil.h, group B "conjugate gradients"): the symbols and their
mirrors, the order of the status codes without a device, which plans read option "cg" 1, the refusal of taps that are not
point-symmetric, and lora_cg_spectrum against numpy on the same tridiagonal."""
import ctypes

import numpy as np
import pytest
from conftest import has_gpu

A, B, C, D = 4096, 8192, 12288, 16384  # four distinct 16-byte aligned "device" addresses: nothing is dereferenced before a device is asked for


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def test_every_new_symbol_is_exported_and_mirrored(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    for name in ["lora_plan_dot", "lora_plan_apply_dot", "lora_plan_cg_update", "lora_plan_cg_direction", "lora_plan_run_cg_until",
                 "lora_plan_prepare_cg", "lora_cg_spectrum", "lora_run_host_cg"]:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ["GridDot", "CgResult", "cg_spectrum", "run_host_cg"]:
        assert hasattr(L, name) and name in L.__all__, name
    for name in ["dot", "apply_dot", "cg_update", "cg_direction", "run_cg_until", "prepare_cg"]:
        assert callable(getattr(L.Plan, name)), name
    # the C structs as the header lays them out
    assert [f[0] for f in _lib.GridDot._fields_] == ["dot", "sum_abs", "count", "nonfinite"] and ctypes.sizeof(_lib.GridDot) == 32
    assert [f[0] for f in _lib.CgResult._fields_] == ["until", "lambda_min", "lambda_max", "rho_estimate", "breakdown"]
    assert ctypes.sizeof(_lib.CgResult) == ctypes.sizeof(_lib.UntilResult) + 32
    assert L.GridDot._fields == ("dot", "sum_abs", "count", "nonfinite")
    assert L.CgResult._fields == ("until", "lambda_min", "lambda_max", "rho_estimate", "breakdown")


def plans(L):
    from lorastencil_amd import _lib

    yes = [L.Plan("1d1r", (9,)), L.Plan("1d2r", (1027,)), L.Plan("star2d1r", (6, 10)), L.Plan("box2d3r", (70, 260)),
           L.Plan("star3d1r", (1, 1, 2)), L.Plan("box3d1r", (35, 17, 130))]
    no = [L.Plan("box3d1r", (4, 4, 8), dtype="bf16"), L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA),
          L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9))]
    return yes, no


def test_option_cg_reads_one_on_the_right_plans(L):
    from lorastencil_amd import _lib

    yes, no = plans(L)
    for p in yes:
        assert p.get_option("cg") == 1 and p.get_option("fused_residual") == 1
        for v in (0, 1):
            assert _lib.lib().lora_plan_set_option(p._h, b"cg", v) == _lib.LORA_EINVAL  # read-only
    for p in no:
        assert p.get_option("cg") == 0
    s = yes[2]
    assert _lib.lib().lora_plan_set_source(s._h, A) == 0 and s.get_option("cg") == 0
    assert _lib.lib().lora_plan_set_source(s._h, None) == 0 and s.get_option("cg") == 1


def test_status_codes_come_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    after = (_lib.LORA_OK,) if has_gpu() else (_lib.LORA_ENODEVICE,)
    yes, no = plans(L)
    p = yes[3]
    out = _lib.GridDot()
    o = ctypes.byref(out)
    # 1. null pointers, bad ranges, a begin off the granularity, equal buffers of different roles: LORA_EINVAL
    assert lib.lora_plan_dot(None, A, B, 0, 0, o, None) == E and lib.lora_plan_dot(p._h, None, B, 0, 0, o, None) == E
    assert lib.lora_plan_dot(p._h, A, B, 0, 0, None, None) == E and lib.lora_plan_dot(p._h, A, B, 0, 71, o, None) == E
    assert lib.lora_plan_dot(p._h, A, B, 5, 3, o, None) == E and lib.lora_plan_dot(p._h, A, B, -1, 3, o, None) == E
    assert lib.lora_plan_apply_dot(p._h, A, None, 0, 0, o, None) == E and lib.lora_plan_apply_dot(p._h, A, A, 0, 0, o, None) == E
    assert lib.lora_plan_apply_dot(p._h, A, B, 0, 71, o, None) == E
    one_d = yes[1]
    assert one_d.region_granularity == 2
    for call in (lambda b: lib.lora_plan_dot(one_d._h, A, B, b, 9, o, None), lambda b: lib.lora_plan_apply_dot(one_d._h, A, B, b, 9, o, None),
                 lambda b: lib.lora_plan_cg_update(one_d._h, A, B, C, D, 0.5, b, 9, o, None),
                 lambda b: lib.lora_plan_cg_direction(one_d._h, A, B, 0.5, b, 9, None)):
        assert call(3) == E
    bufs = [A, B, C, D]
    for i in range(4):
        for j in range(i + 1, 4):
            same = list(bufs)
            same[j] = same[i]
            assert lib.lora_plan_cg_update(p._h, *same, 0.5, 0, 0, o, None) == E, (i, j)
    assert lib.lora_plan_cg_update(p._h, A, B, C, D, 0.5, 0, 0, None, None) == E
    assert lib.lora_plan_cg_direction(p._h, A, A, 0.5, 0, 0, None) == E and lib.lora_plan_cg_direction(p._h, A, None, 0.5, 0, 0, None) == E
    # ... also on a plan without the kernels, and with a misaligned buffer: LORA_EINVAL comes first
    assert lib.lora_plan_apply_dot(no[0]._h, A + 8, A + 8, 0, 0, o, None) == E
    # 2. a misaligned buffer: LORA_EUNSUPPORTED, also on a plan without the kernels
    for q in (p, no[2]):
        assert lib.lora_plan_apply_dot(q._h, A + 8, B, 0, 0, o, None) == U and lib.lora_plan_apply_dot(q._h, A, B + 8, 0, 0, o, None) == U
        for k in range(4):
            mis = list(bufs)
            mis[k] += 8
            assert lib.lora_plan_cg_update(q._h, *mis, 0.5, 0, 0, o, None) == U
        assert lib.lora_plan_cg_direction(q._h, A, B + 8, 0.5, 0, 0, None) == U
    assert lib.lora_plan_dot(p._h, A + 8, B, 0, 0, o, None) == U
    # 3. a plan without the kernels: LORA_EUNSUPPORTED, also for the empty range; lora_plan_dot takes every plan
    for q in no:
        assert lib.lora_plan_apply_dot(q._h, A, B, 0, 0, o, None) == U and lib.lora_plan_apply_dot(q._h, A, B, 2, 2, o, None) == U
        assert lib.lora_plan_cg_update(q._h, A, B, C, D, 0.5, 0, 0, o, None) == U
        assert lib.lora_plan_cg_direction(q._h, A, B, 0.5, 0, 0, None) == U
        assert lib.lora_plan_prepare_cg(q._h, 10) == U
        assert "conjugate-gradient" in lib.lora_last_error().decode()
    assert lib.lora_plan_prepare_cg(p._h, -1) == E and lib.lora_plan_prepare_cg(None, 4) == E
    # 4. then the device: without one, LORA_ENODEVICE -- the empty range included, like the reductions
    if not has_gpu():
        for q in no[:1] + [p]:
            assert lib.lora_plan_dot(q._h, A, B, 0, 0, o, None) in after and lib.lora_plan_dot(q._h, A, A, 2, 2, o, None) in after
        assert lib.lora_plan_apply_dot(p._h, A, B, 0, 0, o, None) in after and lib.lora_plan_apply_dot(p._h, A, B, 2, 2, o, None) in after
        assert lib.lora_plan_cg_update(p._h, A, B, C, D, 0.5, 0, 0, o, None) in after
        assert lib.lora_plan_cg_direction(p._h, A, B, 0.5, 0, 0, None) in after
        assert lib.lora_plan_prepare_cg(p._h, 10) in after


def test_the_driver_checks_its_arguments_and_refuses_unsymmetric_taps(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (6, 10))
    w = np.zeros(L.ops.ntaps("star2d1r"))
    w[[17, 23, 25, 31]] = 0.25
    p.set_weights(w)
    r = _lib.CgResult()
    good = _lib.Until(1e-9, 0.0, _lib.NORM_MAX, 2, 40)
    run = lambda plan, x, f, u: lib.lora_plan_run_cg_until(plan._h if plan else None, x, f, ctypes.byref(u) if u else None, ctypes.byref(r), None)
    assert run(None, A, B, good) == E and run(p, None, B, good) == E and run(p, A, B, None) == E and run(p, A, A, good) == E
    assert lib.lora_plan_run_cg_until(p._h, A, B, ctypes.byref(good), None, None) == E
    for bad in [_lib.Until(1e-9, 0.0, 0, 3, 40), _lib.Until(1e-9, 0.0, 0, 0, 40), _lib.Until(-1.0, 0.0, 0, 2, 40),
                _lib.Until(float("nan"), 0.0, 0, 2, 40), _lib.Until(1e-9, 0.0, 7, 2, 40), _lib.Until(1e-9, 0.0, 0, 2, -1)]:
        assert run(p, A, B, bad) == E  # lora_plan_run_until's rules, unchanged
    assert run(p, A + 8, B, good) == U and run(p, A, B + 8, good) == U
    for q in plans(L)[1]:
        assert run(q, A, B, good) == U
    # taps that are not point-symmetric: decided on the host, before any device is asked for
    lop = w.copy()
    lop[17] = 0.125
    assert L.Plan("star2d1r", (6, 10)).set_weights(lop).get_option("cg") == 1
    assert run(L.Plan("star2d1r", (6, 10)).set_weights(lop), A, B, good) == U
    assert "point-symmetric" in lib.lora_last_error().decode()
    for shape, dims in [("1d2r", (1027,)), ("box3d1r", (4, 4, 8))]:
        v = np.arange(1.0, L.ops.ntaps(shape) + 1)
        assert run(L.Plan(shape, dims).set_weights(v), A, None, good) == U
        if not has_gpu():  # (with a device the symmetric table would be launched on these made-up addresses)
            assert run(L.Plan(shape, dims).set_weights(v + v[::-1]), A, None, good) == _lib.LORA_ENODEVICE
    if not has_gpu():
        assert run(p, A, B, good) == _lib.LORA_ENODEVICE and run(p, A, None, good) == _lib.LORA_ENODEVICE
        # the host operator: arguments first, then the device
        a = np.zeros(L.padded_shape("star2d1r", (6, 10)))
        with pytest.raises(L.LoraError) as e:
            L.run_host_cg("star2d1r", a, 1e-9, check_every=3)
        assert e.value.status == E
        with pytest.raises(L.LoraError) as e:
            L.run_host_cg("star2d1r", a, 1e-9)
        assert e.value.status == _lib.LORA_ENODEVICE
        old = L.set_default_source(a)
        try:
            with pytest.raises(L.LoraError) as e:
                L.run_host_cg("star2d1r", a, 1e-9)
            assert e.value.status == U
        finally:
            L.set_default_source(old)


def lanczos(alpha, beta):
    n = len(alpha)
    d = 1.0 / alpha
    d[1:] += beta[:-1] / alpha[:-1]
    e = np.sqrt(beta[:-1]) / alpha[:-1]
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1) if n > 1 else np.array([[d[0]]])


@pytest.mark.parametrize("n", [1, 2, 40])
def test_cg_spectrum_agrees_with_eigvalsh(L, n):
    rng = np.random.default_rng(n)
    alpha, beta = rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 0.9, n)
    ev = np.linalg.eigvalsh(lanczos(alpha, beta))
    lo, hi = L.cg_spectrum(alpha, beta)
    print(n, "lambda_min", lo, ev[0], "lambda_max", hi, ev[-1])
    assert abs(lo - ev[0]) <= 1e-12 * abs(ev[0]) and abs(hi - ev[-1]) <= 1e-12 * abs(ev[-1])
    # the last beta is not read
    beta2 = beta.copy()
    beta2[-1] = -5.0
    assert L.cg_spectrum(alpha, beta2) == (lo, hi)


def test_cg_spectrum_refuses_bad_histories(L):
    from lorastencil_amd import _lib

    lib, E = _lib.lib(), _lib.LORA_EINVAL
    lo, hi = ctypes.c_double(), ctypes.c_double()
    dp = lambda a: np.asarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda a, b, n: lib.lora_cg_spectrum(dp(a), dp(b), n, ctypes.byref(lo), ctypes.byref(hi))
    assert call([1.0, 2.0], [0.5, 0.5], 2) == _lib.LORA_OK
    assert call([1.0, 2.0], [0.5, 0.5], 0) == E and call([1.0, 2.0], [0.5, 0.5], -3) == E
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call([1.0, bad], [0.5, 0.5], 2) == E and call([bad], [0.5], 1) == E
    assert call([1.0, 2.0], [-0.5, 0.5], 2) == E and call([1.0, 2.0], [float("nan"), 0.5], 2) == E
    assert lib.lora_cg_spectrum(None, dp([0.5]), 1, ctypes.byref(lo), ctypes.byref(hi)) == E
    assert lib.lora_cg_spectrum(dp([1.0]), dp([0.5]), 1, None, ctypes.byref(hi)) == E
    assert lib.lora_cg_spectrum(dp([1.0]), None, 1, ctypes.byref(lo), ctypes.byref(hi)) == _lib.LORA_OK and lo.value == 1.0 == hi.value
