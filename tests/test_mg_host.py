"""CPU tests of the multigrid boundary (include/lorastencil.h, group B "geometric multigrid"): the symbols and their mirrors, the
struct layouts, the coarsening rule and its refusals, the coarse taps against a numpy restatement, which plans read option "mg"
1, and the order of the status codes on addresses that are never dereferenced."""
import ctypes

import numpy as np
import pytest
from conftest import has_gpu

A, B, C = 4096, 8192, 12288  # distinct 16-byte aligned "device" addresses: nothing is dereferenced before a device is asked for


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def test_every_new_symbol_is_exported_and_mirrored(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    for name in ["lora_mg_coarse_dims", "lora_mg_coarse_taps", "lora_plan_mg_restrict", "lora_plan_mg_prolong_add", "lora_plan_run_mg_until",
                 "lora_plan_prepare_mg", "lora_plan_mg_cycle_cost", "lora_run_host_mg"]:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ["MgResult", "mg_coarse_dims", "mg_coarse_taps", "run_host_mg"]:
        assert hasattr(L, name) and name in L.__all__, name
    for name in ["mg_restrict", "mg_prolong_add", "run_mg_until", "prepare_mg", "mg_cycle_cost"]:
        assert callable(getattr(L.Plan, name)), name


def test_struct_layouts_are_the_headers(L):
    from lorastencil_amd import _lib

    # lora_mg {int pre, post; double omega; int max_levels, coarse_iters;}
    assert [f[0] for f in _lib.Mg._fields_] == ["pre", "post", "omega", "max_levels", "coarse_iters"]
    assert ctypes.sizeof(_lib.Mg) == 24 and _lib.Mg.omega.offset == 8 and _lib.Mg.max_levels.offset == 16
    # lora_mg_result {lora_until_result until; int levels; int level_dims[16][3];}
    assert [f[0] for f in _lib.MgResult._fields_] == ["until", "levels", "level_dims"]
    u = ctypes.sizeof(_lib.UntilResult)
    assert _lib.MgResult.levels.offset == u and _lib.MgResult.level_dims.offset == u + 4
    assert ctypes.sizeof(_lib.MgResult) == u + 200  # 4 + 192, padded to the struct's 8-byte alignment
    assert L.MgResult._fields == ("until", "levels", "level_dims")


@pytest.mark.parametrize("shape,dims,expect", [("star2d1r", (70, 260), (35, 130)), ("star2d1r", (9, 10), (4, 4)),
                                               ("box2d3r", (250, 250), (125, 124)), ("box3d1r", (35, 17, 130), (17, 8, 64)),
                                               ("star2d1r", (8, 8), (4, 4)), ("star3d1r", (8, 8, 8), (4, 4, 4)),
                                               ("star2d1r", (16384, 16384), (8192, 8192))])
def test_coarse_dims_table(L, shape, dims, expect):
    assert L.mg_coarse_dims(shape, dims) == expect


def test_coarse_dims_refusals(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    out = (ctypes.c_int * 3)()
    call = lambda shape, dims, o=out: lib.lora_mg_coarse_dims(L.ops.shape_id(shape), (ctypes.c_int * len(dims))(*dims) if dims else None, o)
    # any n_c < 4: the outer axis, the inner one (10 -> 5 -> 4 is fine, 8 -> 4 is fine, 9 odd outer -> 4 is fine)
    for shape, dims in [("star2d1r", (7, 64)), ("star2d1r", (64, 6)), ("star2d1r", (6, 10)), ("star2d1r", (64, 7)),
                        ("star3d1r", (8, 7, 8)), ("star3d1r", (7, 8, 8)), ("star3d1r", (8, 8, 6)), ("star3d1r", (1, 1, 2))]:
        assert call(shape, dims) == U, (shape, dims)
    assert call("star2d1r", (8, 9)) == _lib.LORA_OK and tuple(out[:2]) == (4, 4)  # (an odd innermost extent coarsens; its plan has no kernels)
    # 1D shapes
    assert call("1d1r", (1024,)) == U and call("1d2r", (4096,)) == U
    # arguments
    assert call("star2d1r", None) == E and call("star2d1r", (64, 64), None) == E and call("star2d1r", (0, 64)) == E
    assert lib.lora_mg_coarse_dims(99, (ctypes.c_int * 2)(64, 64), out) == E
    with pytest.raises(L.LoraError) as e:
        L.mg_coarse_dims("1d1r", (64,))
    assert e.value.status == U


def offsets(nd):
    if nd == 2:
        return [(t // 7 - 3, t % 7 - 3) for t in range(49)]
    return [(t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1) for t in range(27)]


def numpy_coarse_taps(w, dims, cdims):
    """the header's rule restated: wc = w prod_a q_a^(d_a^2 / |d|^2), the centre keeps the tap sum"""
    nd = len(dims)
    offs = offsets(nd)
    c = len(offs) // 2
    q = [((cdims[a] + 1) / (dims[a] + 1)) ** 2 for a in range(nd)]
    wc = np.zeros(len(offs))
    for t, d in enumerate(offs):
        if t != c:
            l2 = float(sum(x * x for x in d))
            wc[t] = w[t] * np.prod([q[a] ** (d[a] * d[a] / l2) for a in range(nd)])
    wc[c] = w.sum() - np.delete(wc, c).sum()
    return wc


def test_coarse_taps_are_exact_per_axis_for_star_taps(L):
    # a tap along one axis is w q_a, one multiplication by the squared ratio: bit for bit
    for shape, dims in [("star2d3r", (70, 260)), ("star2d1r", (9, 10)), ("star3d1r", (35, 17, 130))]:
        nd = len(dims)
        cd = L.mg_coarse_dims(shape, dims)
        offs = offsets(nd)
        rng = np.random.default_rng(3)
        w = np.array([rng.uniform(0.01, 0.2) if sum(1 for x in d if x) == 1 else 0.0 for d in offs])
        w = (w + w[::-1]) / 2
        wc = L.mg_coarse_taps(shape, w, dims, cd)
        for t, d in enumerate(offs):
            axes = [a for a in range(nd) if d[a]]
            if len(axes) == 1:
                rho = (cd[axes[0]] + 1) / (dims[axes[0]] + 1)
                assert wc[t] == w[t] * (rho * rho), (shape, t)
            elif axes:
                assert wc[t] == 0.0
        assert np.array_equal(wc, wc[::-1])
        assert abs(wc.sum() - w.sum()) <= 4 * np.finfo(float).eps * np.abs(wc).sum()


@pytest.mark.parametrize("shape,dims", [("box2d3r", (250, 96)), ("box2d3r", (70, 260)), ("box3d1r", (24, 40, 64)), ("box3d1r", (35, 17, 130))])
def test_coarse_taps_of_full_tables_match_numpy_and_keep_symmetry_and_sum(L, shape, dims):
    nd = len(dims)
    cd = L.mg_coarse_dims(shape, dims)
    rng = np.random.default_rng(11)
    w = rng.uniform(0.0, 1.0, L.ops.ntaps(shape))
    w = (w + w[::-1]) / 2
    w /= 1.5 * w.sum()
    wc = L.mg_coarse_taps(shape, w, dims, cd)
    ref = numpy_coarse_taps(w, dims, cd)
    eps = np.finfo(float).eps
    print(shape, dims, cd, "max |wc - numpy| / ulp", np.max(np.abs(wc - ref) / (eps * np.maximum(np.abs(ref), 1e-300))))
    c = len(w) // 2
    off = np.arange(len(w)) != c
    assert np.all(np.abs(wc - ref)[off] <= 4 * eps * np.abs(ref)[off])            # pow against numpy's power: a few ulps
    assert abs(wc[c] - ref[c]) <= 4 * eps * np.abs(ref).sum()                      # a difference of sums
    assert np.array_equal(wc, wc[::-1])                                            # point symmetry, exactly
    assert abs(wc.sum() - w.sum()) <= 4 * eps * np.abs(wc).sum()                   # the tap sum
    assert np.all(wc[off] <= w[off]) and np.all(wc[off] > 0.0)                     # every q < 1: the coupling weakens


def test_coarse_taps_arguments(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda *v: (ctypes.c_int * len(v))(*v)
    w, out = np.zeros(49), np.zeros(49)
    sid = L.ops.shape_id("star2d1r")
    assert lib.lora_mg_coarse_taps(sid, dp(w), ip(64, 64), ip(32, 32), dp(out)) == _lib.LORA_OK
    assert lib.lora_mg_coarse_taps(sid, None, ip(64, 64), ip(32, 32), dp(out)) == E
    assert lib.lora_mg_coarse_taps(sid, dp(w), None, ip(32, 32), dp(out)) == E
    assert lib.lora_mg_coarse_taps(sid, dp(w), ip(64, 64), None, dp(out)) == E
    assert lib.lora_mg_coarse_taps(sid, dp(w), ip(64, 64), ip(32, 32), None) == E
    assert lib.lora_mg_coarse_taps(sid, dp(w), ip(64, 0), ip(32, 32), dp(out)) == E
    assert lib.lora_mg_coarse_taps(99, dp(w), ip(64, 64), ip(32, 32), dp(out)) == E
    assert lib.lora_mg_coarse_taps(L.ops.shape_id("1d1r"), dp(w), ip(64), ip(32), dp(out)) == U


def plans(L):
    """the yes / no lists of tests/test_cg_host.py"""
    from lorastencil_amd import _lib

    yes = [L.Plan("1d1r", (9,)), L.Plan("1d2r", (1027,)), L.Plan("star2d1r", (6, 10)), L.Plan("box2d3r", (70, 260)),
           L.Plan("star3d1r", (1, 1, 2)), L.Plan("box3d1r", (35, 17, 130))]
    no = [L.Plan("box3d1r", (4, 4, 8), dtype="bf16"), L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA),
          L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9))]
    return yes, no


def test_option_mg_reads_one_on_the_right_plans(L):
    from lorastencil_amd import _lib

    yes, no = plans(L)
    # of the CG plans: the 2D and 3D ones whose extents halve to at least 4
    assert [p.get_option("mg") for p in yes] == [0, 0, 0, 1, 0, 1]
    assert [p.get_option("cg") for p in yes] == [1] * 6
    for p in no:
        assert p.get_option("mg") == 0
    assert L.Plan("star2d1r", (6, 10)).get_option("mg") == 0
    for shape, dims in [("star2d1r", (8, 8)), ("star2d1r", (9, 10)), ("star3d1r", (8, 8, 8)), ("star2d3r", (64, 64))]:
        assert L.Plan(shape, dims).get_option("mg") == 1, (shape, dims)
    p = yes[3]
    for v in (0, 1):
        assert _lib.lib().lora_plan_set_option(p._h, b"mg", v) == _lib.LORA_EINVAL  # read-only
    # a plan that carries a source has no CG kernels, so none of these either
    assert _lib.lib().lora_plan_set_source(p._h, A) == 0 and p.get_option("mg") == 0
    assert _lib.lib().lora_plan_set_source(p._h, None) == 0 and p.get_option("mg") == 1


def test_transfer_status_codes_come_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    yes, no = plans(L)
    p = yes[3]
    refused = no + [yes[0], yes[2], yes[4]]
    # 1. a null plan or buffer, a non-finite scale, equal buffers: LORA_EINVAL -- also on a plan without the kernels and with a misaligned buffer
    assert lib.lora_plan_mg_restrict(None, A, B, 1.0, None) == E and lib.lora_plan_mg_restrict(p._h, None, B, 1.0, None) == E
    assert lib.lora_plan_mg_restrict(p._h, A, None, 1.0, None) == E and lib.lora_plan_mg_restrict(p._h, A, A, 1.0, None) == E
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.lora_plan_mg_restrict(p._h, A, B, bad, None) == E
    assert lib.lora_plan_mg_prolong_add(None, A, B, None) == E and lib.lora_plan_mg_prolong_add(p._h, None, B, None) == E
    assert lib.lora_plan_mg_prolong_add(p._h, A, None, None) == E and lib.lora_plan_mg_prolong_add(p._h, A, A, None) == E
    assert lib.lora_plan_mg_restrict(no[0]._h, A + 8, A + 8, 1.0, None) == E and lib.lora_plan_mg_prolong_add(no[0]._h, A + 8, A + 8, None) == E
    assert lib.lora_plan_mg_restrict(no[0]._h, A + 8, B, float("nan"), None) == E
    # 2. a misaligned buffer: LORA_EUNSUPPORTED, also on a plan without the kernels
    for q in (p, no[2]):
        assert lib.lora_plan_mg_restrict(q._h, A + 8, B, 1.0, None) == U and lib.lora_plan_mg_restrict(q._h, A, B + 8, 1.0, None) == U
        assert lib.lora_plan_mg_prolong_add(q._h, A + 8, B, None) == U and lib.lora_plan_mg_prolong_add(q._h, A, B + 8, None) == U
        assert "aligned" in lib.lora_last_error().decode()
    # 3. a plan whose option "mg" reads 0: LORA_EUNSUPPORTED
    for q in refused:
        assert lib.lora_plan_mg_restrict(q._h, A, B, 1.0, None) == U and lib.lora_plan_mg_prolong_add(q._h, A, B, None) == U
        assert "multigrid" in lib.lora_last_error().decode()
    # 4. then the device
    if not has_gpu():
        assert lib.lora_plan_mg_restrict(p._h, A, B, 1.0, None) == _lib.LORA_ENODEVICE
        assert lib.lora_plan_mg_prolong_add(p._h, A, B, None) == _lib.LORA_ENODEVICE


def jacobi(L, shape):
    offs = offsets(L.ops.ndim(shape))
    w = np.zeros(len(offs))
    for t, d in enumerate(offs):
        if sum(abs(x) for x in d) == 1:
            w[t] = 1.0 / (2 * len(d))
    return w


def test_the_driver_checks_its_arguments_in_the_documented_order(L):
    from lorastencil_amd import _lib

    lib, E, U = _lib.lib(), _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (16, 16)).set_weights(jacobi(L, "star2d1r"))
    r = _lib.MgResult()
    good_m, good_u = _lib.Mg(2, 2, 0.8, 0, 0), _lib.Until(1e-9, 0.0, _lib.NORM_MAX, 1, 20)

    def run(plan, x, f, m, u, res=r):
        return lib.lora_plan_run_mg_until(plan._h if plan else None, x, f, ctypes.byref(m) if m else None, ctypes.byref(u) if u else None,
                                          ctypes.byref(res) if res is not None else None, None)

    # LORA_EINVAL: null pointers, a bad until, a bad cycle, d_f == d_x
    assert run(None, A, B, good_m, good_u) == E and run(p, None, B, good_m, good_u) == E and run(p, A, B, None, good_u) == E
    assert run(p, A, B, good_m, None) == E and run(p, A, B, good_m, good_u, None) == E and run(p, A, A, good_m, good_u) == E
    for bad in [_lib.Until(1e-9, 0.0, 0, 0, 20), _lib.Until(1e-9, 0.0, 0, -2, 20), _lib.Until(-1.0, 0.0, 0, 1, 20),
                _lib.Until(float("nan"), 0.0, 0, 1, 20), _lib.Until(1e-9, -1.0, 0, 1, 20), _lib.Until(1e-9, 0.0, 7, 1, 20),
                _lib.Until(1e-9, 0.0, 0, 1, -1)]:
        assert run(p, A, B, good_m, bad) == E
    for bad in [_lib.Mg(-1, 2, 0.8, 0, 0), _lib.Mg(2, -1, 0.8, 0, 0), _lib.Mg(0, 0, 0.8, 0, 0), _lib.Mg(2, 2, 0.0, 0, 0), _lib.Mg(2, 2, 2.0, 0, 0),
                _lib.Mg(2, 2, -0.5, 0, 0), _lib.Mg(2, 2, float("nan"), 0, 0), _lib.Mg(2, 2, float("inf"), 0, 0), _lib.Mg(2, 2, 0.8, -1, 0),
                _lib.Mg(2, 2, 0.8, 1, 0), _lib.Mg(2, 2, 0.8, 0, -1)]:
        assert run(p, A, B, bad, good_u) == E, (bad.pre, bad.post, bad.omega, bad.max_levels, bad.coarse_iters)
        assert lib.lora_plan_prepare_mg(p._h, ctypes.byref(bad)) == E
    assert lib.lora_plan_prepare_mg(None, ctypes.byref(good_m)) == E and lib.lora_plan_prepare_mg(p._h, None) == E
    # ... before the buffers' alignment and the plan are looked at
    assert run(plans(L)[1][0], A + 8, A + 8, good_m, good_u) == E
    # LORA_EUNSUPPORTED: a misaligned buffer, then a plan whose "mg" reads 0, then taps that are not point-symmetric, then a
    # level whose diagonal is not positive
    assert run(p, A + 8, B, good_m, good_u) == U and run(p, A, B + 8, good_m, good_u) == U
    yes, no = plans(L)
    for q in no + [yes[0], yes[2], yes[4]]:
        assert run(q, A, B, good_m, good_u) == U and "multigrid" in lib.lora_last_error().decode()
        assert lib.lora_plan_prepare_mg(q._h, ctypes.byref(good_m)) == U
    lop = jacobi(L, "star2d1r")
    lop[17] = 0.125
    q = L.Plan("star2d1r", (16, 16)).set_weights(lop)
    assert q.get_option("mg") == 1 and run(q, A, B, good_m, good_u) == U and "point-symmetric" in lib.lora_last_error().decode()
    one = jacobi(L, "star2d1r")
    one[24] = 1.0
    q = L.Plan("star2d1r", (16, 16)).set_weights(one)
    assert run(q, A, None, good_m, good_u) == U and "diagonal" in lib.lora_last_error().decode()
    assert lib.lora_plan_prepare_mg(q._h, ctypes.byref(good_m)) == U
    # one tap table every level can carry: any check_every >= 1 is legal, odd ones included
    if not has_gpu():
        for ce in (1, 2, 3):
            assert run(p, A, B, good_m, _lib.Until(1e-9, 0.0, 0, ce, 20)) == _lib.LORA_ENODEVICE
        assert run(p, A, None, good_m, good_u) == _lib.LORA_ENODEVICE
        assert lib.lora_plan_prepare_mg(p._h, ctypes.byref(good_m)) == _lib.LORA_ENODEVICE
        n, b = ctypes.c_int(), ctypes.c_double()
        assert lib.lora_plan_mg_cycle_cost(p._h, ctypes.byref(n), ctypes.byref(b)) == E  # no cycle has run
        a = np.zeros(L.padded_shape("star2d1r", (16, 16)))
        with pytest.raises(L.LoraError) as e:
            L.run_host_mg("star2d1r", a, 1e-9, check_every=0)
        assert e.value.status == E
        with pytest.raises(L.LoraError) as e:
            L.run_host_mg("star2d1r", a, 1e-9)
        assert e.value.status == _lib.LORA_ENODEVICE
        old = L.set_default_source(a)
        try:
            with pytest.raises(L.LoraError) as e:
                L.run_host_mg("star2d1r", a, 1e-9)
            assert e.value.status == U
        finally:
            L.set_default_source(old)
