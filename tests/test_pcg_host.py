"""CPU tests of the multigrid-preconditioned boundary (include/lorastencil.h, group B "multigrid-preconditioned conjugate
gradients"): the symbols and their mirrors, the struct layout, option "pcg", the smoother formulas for A = sigma I - tau S
restated in numpy, and the order of the status codes on addresses that are never dereferenced."""
import ctypes

import numpy as np
import pytest
from conftest import has_gpu

A, B, C = 4096, 8192, 12288  # distinct 16-byte aligned "device" addresses: nothing is dereferenced before a device is asked for


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def offsets(nd):
    if nd == 2:
        return [(t // 7 - 3, t % 7 - 3) for t in range(49)]
    return [(t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1) for t in range(27)]


def jacobi(nd):
    w = np.zeros(len(offsets(nd)))
    for t, d in enumerate(offsets(nd)):
        if sum(abs(x) for x in d) == 1:
            w[t] = 1.0 / (2 * nd)
    return w


def plans(L):
    """(plans whose option "cg" reads 1, plans without the CG kernels)"""
    from lorastencil_amd import _lib

    yes = [L.Plan("1d1r", (9,)), L.Plan("1d2r", (1027,)), L.Plan("star2d1r", (6, 10)), L.Plan("box2d3r", (70, 260)),
           L.Plan("star3d1r", (1, 1, 2)), L.Plan("box3d1r", (35, 17, 130))]
    no = [L.Plan("box3d1r", (4, 4, 8), dtype="bf16"), L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA),
          L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9))]
    return yes, no


def test_every_new_symbol_is_exported_and_mirrored(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    for name in ["lora_plan_defect", "lora_plan_mg_precondition", "lora_plan_run_pcg_until", "lora_plan_prepare_pcg", "lora_plan_run_theta_mg",
                 "lora_run_host_pcg", "lora_run_host_theta_mg"]:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ["PcgResult", "run_host_pcg", "run_host_theta_mg"]:
        assert hasattr(L, name) and name in L.__all__, name
    for name in ["defect", "mg_precondition", "run_pcg_until", "prepare_pcg", "run_theta_mg"]:
        assert callable(getattr(L.Plan, name)), name


def test_struct_layout_is_the_headers(L):
    from lorastencil_amd import _lib

    # lora_pcg_result {lora_until_result until; double lambda_min, lambda_max; int breakdown, levels;}
    assert [f[0] for f in _lib.PcgResult._fields_] == ["until", "lambda_min", "lambda_max", "breakdown", "levels"]
    u = ctypes.sizeof(_lib.UntilResult)
    assert _lib.PcgResult.lambda_min.offset == u and _lib.PcgResult.breakdown.offset == u + 16 and _lib.PcgResult.levels.offset == u + 20
    assert ctypes.sizeof(_lib.PcgResult) == u + 24
    assert L.PcgResult._fields == ("until", "lambda_min", "lambda_max", "breakdown", "levels")


def test_option_pcg_reads_what_mg_reads(L):
    from lorastencil_amd import _lib

    yes, no = plans(L)
    extra = [L.Plan(s, d) for s, d in [("star2d1r", (8, 8)), ("star2d1r", (9, 10)), ("star3d1r", (8, 8, 8)), ("star2d3r", (64, 64))]]
    for p in yes + no + extra:
        assert p.get_option("pcg") == p.get_option("mg")
    assert [p.get_option("pcg") for p in yes] == [0, 0, 0, 1, 0, 1] and all(p.get_option("pcg") == 1 for p in extra)
    for v in (0, 1):
        assert _lib.lib().lora_plan_set_option(yes[3]._h, b"pcg", v) == _lib.LORA_EINVAL  # read-only
    p = yes[3]
    assert _lib.lib().lora_plan_set_source(p._h, A) == 0 and p.get_option("pcg") == 0
    assert _lib.lib().lora_plan_set_source(p._h, None) == 0 and p.get_option("pcg") == 1


def smoother_11(w, omega):
    """the smoother of lora_plan_run_mg_until: d = fl(1 - w[centre]), c = fl(omega / d), s[t] = fl(c w[t]), s[centre] += fl(1 - c)"""
    ct = len(w) // 2
    d = 1.0 - w[ct]
    c = omega / d
    s = c * w
    s[ct] = s[ct] + (1.0 - c)
    return d, c, s


def smoother_pair(w, omega, sigma, tau):
    """the header's formulas for A = sigma I - tau S, one numpy operation per rounding"""
    ct = len(w) // 2
    d = sigma - tau * w[ct]
    c = omega / d
    cp = c * tau
    s = cp * w
    s[ct] = s[ct] + (1.0 - c * sigma)
    return d, c, s


@pytest.mark.parametrize("nd", [2, 3])
def test_the_pair_one_one_gives_todays_smoother_bit_for_bit(nd):
    rng = np.random.default_rng(nd)
    tables = [jacobi(nd)]
    for _ in range(20):
        w = rng.uniform(-0.3, 1.0, len(offsets(nd)))
        w = (w + w[::-1]) / 2
        tables.append(w * (0.97 / w.sum()))
    for w in tables:
        for omega in (0.8, 2.0 / 3.0, 1.0, 1.3):
            d0, c0, s0 = smoother_11(w.copy(), omega)
            d1, c1, s1 = smoother_pair(w.copy(), omega, 1.0, 1.0)
            assert d0 == d1 and c0 == c1 and np.array_equal(s0.view(np.int64), s1.view(np.int64))
    # and a pair that is not (1, 1) is the damped Jacobi sweep of sigma I - tau S: s = I - c A on the taps
    w, sigma, tau, omega = jacobi(nd), 9.0, 8.0, 0.8
    d, c, s = smoother_pair(w.copy(), omega, sigma, tau)
    a_taps = -tau * w
    a_taps[len(w) // 2] += sigma
    ident = np.zeros_like(w)
    ident[len(w) // 2] = 1.0
    assert d == sigma and np.allclose(s, ident - c * a_taps, rtol=0, atol=4 * 2.0 ** -53)


def test_defect_checks_its_arguments_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    yes, no = plans(L)
    p = yes[3]  # box2d3r (70, 260)
    f = lambda plan, u, src, out, b=0, e=0: lib.lora_plan_defect(plan._h if plan else None, u, src, out, b, e, None)
    # 1. LORA_EINVAL: a null plan, d_u or d_out; a bad range or begin; any two buffers equal -- also on a plan without the
    # kernels and with misaligned buffers
    assert f(None, A, B, C) == E and f(p, None, B, C) == E and f(p, A, B, None) == E
    assert f(p, A, B, C, 10, 5) == E and f(p, A, B, C, -1, 5) == E and f(p, A, B, C, 0, 71) == E
    assert f(p, A, B, A) == E and f(p, A, A, C) == E and f(p, A, C, C) == E
    assert f(no[0], A + 8, A + 8, A + 8) == E and f(no[2], A + 8, None, A + 8) == E
    # 2. LORA_EUNSUPPORTED: a misaligned buffer, also on a plan without the kernels
    for q in (p, no[2]):
        assert f(q, A + 8, B, C) == U and f(q, A, B + 8, C) == U and f(q, A, B, C + 8) == U and f(q, A + 8, None, C) == U
        assert "aligned" in lib.lora_last_error().decode()
    # 3. then a plan without the kernels: bf16, the matrix-pipe variant, an odd innermost extent, a plan with a source
    for q in no:
        assert f(q, A, B, C) == U and f(q, A, None, C) == U
    assert lib.lora_plan_set_source(p._h, A) == 0
    assert f(p, B, None, C) == U and "source" in lib.lora_last_error().decode()
    assert lib.lora_plan_set_source(p._h, None) == 0
    # 4. then the device; 1D plans have the kernel
    if not has_gpu():
        for q in yes:
            assert f(q, A, B, C) == _lib.LORA_ENODEVICE and f(q, A, None, C) == _lib.LORA_ENODEVICE


BAD_MG = [(-1, 2, 0.8, 0, 0), (2, -1, 0.8, 0, 0), (0, 0, 0.8, 0, 0), (2, 2, 0.0, 0, 0), (2, 2, 2.0, 0, 0), (2, 2, -0.5, 0, 0),
          (2, 2, float("nan"), 0, 0), (2, 2, float("inf"), 0, 0), (2, 2, 0.8, -1, 0), (2, 2, 0.8, 1, 0), (2, 2, 0.8, 0, -1)]
BAD_PAIRS = [(1.0, float("nan")), (1.0, float("inf")), (1.0, -1.0), (0.0, 1.0), (-2.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0)]


def refused_plans(L):
    yes, no = plans(L)
    return no + [yes[0], yes[2], yes[4]]  # without the CG kernels; 1D; extents that do not halve to 4


def odd_taps():
    lop = jacobi(2)
    lop[17] = 0.125
    return lop


def test_the_preconditioner_checks_its_arguments_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (16, 16)).set_weights(jacobi(2))
    good = _lib.Mg(2, 2, 0.8, 0, 0)
    f = lambda plan, r, z, m, sigma=1.0, tau=1.0: lib.lora_plan_mg_precondition(plan._h if plan else None, r, z, ctypes.byref(m) if m else None,
                                                                                sigma, tau, None)
    assert f(None, A, B, good) == E and f(p, None, B, good) == E and f(p, A, None, good) == E and f(p, A, B, None) == E and f(p, A, A, good) == E
    for bad in BAD_MG:
        assert f(p, A, B, _lib.Mg(*bad)) == E, bad
    for sigma, tau in BAD_PAIRS:
        assert f(p, A, B, good, sigma, tau) == E, (sigma, tau)
    assert f(plans(L)[1][0], A + 8, A + 8, good) == E  # ... before alignment and the plan are looked at
    # any m is legal here: the public entry does not ask for a symmetric cycle
    assert f(p, A + 8, B, _lib.Mg(1, 2, 0.8, 0, 0)) == U and f(p, A, B + 8, _lib.Mg(0, 1, 0.8, 0, 0)) == U
    assert "aligned" in lib.lora_last_error().decode()
    for q in refused_plans(L):
        assert f(q, A, B, good) == U and "multigrid" in lib.lora_last_error().decode()
    q = L.Plan("star2d1r", (16, 16)).set_weights(odd_taps())
    assert f(q, A, B, good) == U and "point-symmetric" in lib.lora_last_error().decode()
    # a level diagonal <= 0: the reference's integer star2d1r taps (the plan's defaults), and sigma - tau w[centre] <= 0
    q = L.Plan("star2d1r", (16, 16))
    assert f(q, A, B, good) == U and "diagonal" in lib.lora_last_error().decode()
    centre = jacobi(2)
    centre[24] = 0.5
    q = L.Plan("star2d1r", (16, 16)).set_weights(centre)
    assert f(q, A, B, good, 1.0, 2.0) == U and "diagonal" in lib.lora_last_error().decode()
    if not has_gpu():
        for pair in [(1.0, 1.0), (9.0, 8.0), (1.0, 0.0), (4097.0, 4096.0)]:
            assert f(p, A, B, good, *pair) == _lib.LORA_ENODEVICE, pair


def test_the_pcg_driver_checks_its_arguments_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (16, 16)).set_weights(jacobi(2))
    r = _lib.PcgResult()
    good_m, good_u = _lib.Mg(2, 2, 0.8, 0, 0), _lib.Until(1e-9, 0.0, _lib.NORM_MAX, 2, 20)

    def run(plan, x, f, m, u, res=r):
        return lib.lora_plan_run_pcg_until(plan._h if plan else None, x, f, ctypes.byref(m) if m else None, ctypes.byref(u) if u else None,
                                           ctypes.byref(res) if res is not None else None, None)

    prep = lambda plan, m, n=20: lib.lora_plan_prepare_pcg(plan._h if plan else None, ctypes.byref(m) if m else None, n)
    assert run(None, A, B, good_m, good_u) == E and run(p, None, B, good_m, good_u) == E and run(p, A, B, None, good_u) == E
    assert run(p, A, B, good_m, None) == E and run(p, A, B, good_m, good_u, None) == E and run(p, A, A, good_m, good_u) == E
    # check_every is even and >= 2, as in lora_plan_run_cg_until
    for bad in [_lib.Until(1e-9, 0.0, 0, 0, 20), _lib.Until(1e-9, 0.0, 0, 1, 20), _lib.Until(1e-9, 0.0, 0, 3, 20), _lib.Until(-1.0, 0.0, 0, 2, 20),
                _lib.Until(float("nan"), 0.0, 0, 2, 20), _lib.Until(1e-9, -1.0, 0, 2, 20), _lib.Until(1e-9, 0.0, 7, 2, 20),
                _lib.Until(1e-9, 0.0, 0, 2, -1)]:
        assert run(p, A, B, good_m, bad) == E
    for bad in BAD_MG + [(1, 2, 0.8, 0, 0), (2, 1, 0.8, 0, 0), (0, 1, 0.8, 0, 0), (1, 0, 0.8, 0, 0)]:  # ... and pre == post >= 1
        assert run(p, A, B, _lib.Mg(*bad), good_u) == E, bad
        assert prep(p, _lib.Mg(*bad)) == E, bad
    assert prep(None, good_m) == E and prep(p, None) == E and prep(p, good_m, -1) == E
    assert run(plans(L)[1][0], A + 8, A + 8, good_m, good_u) == E
    assert run(p, A + 8, B, good_m, good_u) == U and run(p, A, B + 8, good_m, good_u) == U
    for q in refused_plans(L):
        assert run(q, A, B, good_m, good_u) == U and "multigrid" in lib.lora_last_error().decode()
        assert prep(q, good_m) == U
    q = L.Plan("star2d1r", (16, 16)).set_weights(odd_taps())
    assert run(q, A, B, good_m, good_u) == U and "point-symmetric" in lib.lora_last_error().decode()
    q = L.Plan("star2d1r", (16, 16))  # the reference's integer taps: 1 - w[centre] <= 0
    assert run(q, A, None, good_m, good_u) == U and "diagonal" in lib.lora_last_error().decode()
    assert prep(q, good_m) == U
    if not has_gpu():
        assert run(p, A, B, good_m, good_u) == _lib.LORA_ENODEVICE and run(p, A, None, good_m, good_u) == _lib.LORA_ENODEVICE
        assert prep(p, good_m) == _lib.LORA_ENODEVICE
        a = np.zeros(L.padded_shape("star2d1r", (16, 16)))
        with pytest.raises(L.LoraError) as e:
            L.run_host_pcg("star2d1r", a, 1e-9, check_every=3)
        assert e.value.status == E
        with pytest.raises(L.LoraError) as e:
            L.run_host_pcg("star2d1r", a, 1e-9)
        assert e.value.status == _lib.LORA_ENODEVICE


def test_the_preconditioned_stepper_checks_its_arguments_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (16, 16)).set_weights(jacobi(2))
    r = _lib.ThetaResult()
    good = _lib.Mg(2, 2, 0.8, 0, 0)

    def run(plan, u, f, theta=1.0, tau=8.0, steps=2, iters=10, rtol=1e-8, m=good, ce=1, res=r):
        return lib.lora_plan_run_theta_mg(plan._h if plan else None, u, f, theta, tau, steps, iters, rtol, ctypes.byref(m) if m else None, ce,
                                          None, ctypes.byref(res) if res is not None else None, None)

    assert run(None, A, B) == E and run(p, None, B) == E and run(p, A, B, res=None) == E and run(p, A, B, m=None) == E and run(p, A, A) == E
    for kw in [dict(theta=-0.1), dict(theta=1.1), dict(theta=float("nan")), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")),
               dict(tau=float("nan")), dict(steps=-1), dict(iters=0), dict(rtol=-1.0), dict(rtol=float("inf")), dict(ce=0), dict(ce=-3)]:
        assert run(p, A, B, **kw) == E, kw
    for bad in BAD_MG + [(1, 2, 0.8, 0, 0), (2, 1, 0.8, 0, 0), (0, 1, 0.8, 0, 0)]:
        assert run(p, A, B, m=_lib.Mg(*bad)) == E, bad
    assert run(plans(L)[1][0], A + 8, A + 8) == E
    assert run(p, A + 8, B) == U and run(p, A, B + 8) == U and "aligned" in lib.lora_last_error().decode()
    for q in refused_plans(L):
        assert run(q, A, B) == U and "multigrid" in lib.lora_last_error().decode()
    q = L.Plan("star2d1r", (16, 16)).set_weights(odd_taps())
    assert run(q, A, B) == U and "point-symmetric" in lib.lora_last_error().decode()
    q = L.Plan("star2d1r", (16, 16))  # integer taps: sigma - tau' w[centre] <= 0 for tau = 8
    assert run(q, A, B) == U and "diagonal" in lib.lora_last_error().decode()
    # steps == 0 touches nothing, with or without a device; theta == 0 and any check_every >= 1 are legal
    assert run(p, A, B, steps=0) == _lib.LORA_OK and r.steps_done == 0
    if not has_gpu():
        for kw in [dict(), dict(theta=0.0), dict(ce=3), dict(theta=0.5, tau=4096.0)]:
            assert run(p, A, B, **kw) == _lib.LORA_ENODEVICE, kw
        a = np.zeros(L.padded_shape("star2d1r", (16, 16)))
        with pytest.raises(L.LoraError) as e:
            L.run_host_theta_mg("star2d1r", a, 8.0, 2, check_every=0)
        assert e.value.status == E
        with pytest.raises(L.LoraError) as e:
            L.run_host_theta_mg("star2d1r", a, 8.0, 2)
        assert e.value.status == _lib.LORA_ENODEVICE
