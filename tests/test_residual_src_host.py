"""CPU tests of lora_plan_residual_src's boundary (include/lorastencil.h): the symbol and its mirrors, the order of the status
codes on addresses nobody dereferences, which plans refuse a source operand, the loud failure without a device, and that no
call changes the plan (the source is a call argument, never plan state).
"""
import ctypes
import os

import pytest
from conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 16-byte aligned addresses nobody owns.  Every call made on them is refused before a launch; the good calls, which stop at
# LORA_ENODEVICE only where there is no device, are made under `not has_gpu()` alone.
A, F = 4096, 8192

# what of a plan must be what it was after a call: the kernel's name and signature (every option that picks or tunes a kernel
# is part of the signature), the leapfrog depth, and the keys a source or this entry could have touched
KEYS = ["fused_residual", "source", "steps_per_launch", "variant", "tapset", "boundary"]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature, p.leapfrog_depth


def plans_without_the_kernel(L):
    from lorastencil_amd import _lib

    return [L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9)), L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)]


def test_symbol_prototype_and_method_exist(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    assert lib.lora_plan_residual_src and "lora_plan_residual_src" in _lib.SIGNATURES
    assert ("int lora_plan_residual_src(lora_plan *plan, const void *d_in, const void *d_f, int begin, int end, lora_grid_diff *out, "
            "void *stream);") in header
    restype, argtypes = _lib.SIGNATURES["lora_plan_residual_src"]
    assert restype is ctypes.c_int and len(argtypes) == 7
    assert callable(L.Plan.residual_src)


def test_status_codes_come_in_the_stated_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    df = ctypes.byref(_lib.GridDiff())
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    call = lib.lora_plan_residual_src
    p = L.Plan("star2d1r", (32, 64))
    before = state(p)
    # 1. LORA_EINVAL: null pointers, bad ranges, a bad begin, d_f == d_in -- with and without a source
    for f in (F, None):
        assert call(None, A, f, 0, 0, df, None) == E
        assert call(p._h, None, f, 0, 0, df, None) == E
        assert call(p._h, A, f, 0, 0, None, None) == E
        for begin, end in [(-1, 4), (0, 33), (5, 4), (33, 33)]:
            assert call(p._h, A, f, begin, end, df, None) == E, (begin, end)
    assert call(p._h, A, A, 0, 0, df, None) == E
    p1 = L.Plan("1d1r", (300,))
    assert call(p1._h, A, F, 1, 300, df, None) == E and call(p1._h, A, F, 3, 3, df, None) == E  # an odd begin in 1D
    # ... all of it before alignment and before "no kernel": a plan without the kernel, misaligned buffers
    for q in plans_without_the_kernel(L):
        assert call(None, A + 8, F + 8, 0, 0, df, None) == E
        assert call(q._h, A + 8, A + 8, 0, 0, df, None) == E        # d_f == d_in
        assert call(q._h, A + 8, F + 8, 0, q.dims[0] + 1, df, None) == E  # a bad range
        assert call(q._h, A + 8, F + 8, 3, 2, df, None) == E
    # 2. LORA_EUNSUPPORTED: a misaligned d_in or d_f
    for q in [p, p1] + plans_without_the_kernel(L):
        assert call(q._h, A + 8, F, 0, 0, df, None) == U
        assert call(q._h, A, F + 8, 0, 0, df, None) == U
        assert "aligned" in lib.lora_last_error().decode()
    assert state(p) == before


def test_plans_that_take_no_source_operand_are_refused(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    df = ctypes.byref(_lib.GridDiff())
    U = _lib.LORA_EUNSUPPORTED
    for q in plans_without_the_kernel(L):
        before = state(q)
        assert q.get_option("fused_residual") == 0
        assert lib.lora_plan_residual_src(q._h, A, F, 0, 0, df, None) == U
        assert "fused residual" in lib.lora_last_error().decode()
        assert lib.lora_plan_residual_src(q._h, A, None, 0, 0, df, None) == U  # (as lora_plan_residual)
        assert state(q) == before
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    before = state(bf)
    assert bf.get_option("fused_residual") == 1
    assert lib.lora_plan_residual_src(bf._h, A, F, 0, 0, df, None) == U
    assert "bf16" in lib.lora_last_error().decode()
    assert lib.lora_plan_residual_src(bf._h, A, F, 2, 2, df, None) == U  # also for the empty range
    assert state(bf) == before
    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("box3d1r", (4, 6, 8))]:
        s = L.Plan(shape, dims)
        assert lib.lora_plan_set_source(s._h, F) == 0
        before = state(s)
        assert s.get_option("source") == 1 and s.get_option("fused_residual") == 0
        assert lib.lora_plan_residual_src(s._h, A, F, 0, 0, df, None) == U
        assert "source" in lib.lora_last_error().decode()
        assert lib.lora_plan_residual_src(s._h, A, F + 4096, 0, 0, df, None) == U  # another grid than the plan's source, too
        assert state(s) == before
        assert lib.lora_plan_set_source(s._h, None) == 0 and s.get_option("fused_residual") == 1


def test_the_key_stays_read_only_and_the_plan_unchanged(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    df = ctypes.byref(_lib.GridDiff())
    for shape, dtype, dims in [("1d2r", "f64", (300,)), ("box2d3r", "f64", (33, 130)), ("star3d1r", "f64", (3, 5, 8)),
                               ("box3d1r", "bf16", (3, 5, 8))]:
        p = L.Plan(shape, dims, dtype=dtype)
        before = state(p)
        for f in (F, None):  # refused before a launch, with or without a device: a bad range, a misaligned grid
            assert lib.lora_plan_residual_src(p._h, A, f, 0, dims[0] + 1, df, None) == _lib.LORA_EINVAL
            assert lib.lora_plan_residual_src(p._h, A + 8, f, 0, 0, df, None) == _lib.LORA_EUNSUPPORTED
            if not has_gpu():  # with a device these would launch on addresses nobody owns
                assert lib.lora_plan_residual_src(p._h, A, f, 0, 0, df, None) in (_lib.LORA_ENODEVICE, _lib.LORA_EUNSUPPORTED)
                assert lib.lora_plan_residual_src(p._h, A, f, 2, 2, df, None) in (_lib.LORA_ENODEVICE, _lib.LORA_EUNSUPPORTED)
        for v in (0, 1):
            assert lib.lora_plan_set_option(p._h, b"fused_residual", v) == _lib.LORA_EINVAL
        assert state(p) == before and "residual" not in p.kernel_signature
        assert p.get_option("source") == 0 and p.get_option("fused_residual") == 1


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_residual_src_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("box2d3r", (32, 64)), ("box3d1r", (4, 6, 8))]:
        p = L.Plan(shape, dims)
        before = state(p)
        for call in [lambda: p.residual_src(A, F), lambda: p.residual_src(A, F, 2, 2), lambda: p.residual_src(A, F, 0, 2),
                     lambda: p.residual_src(A, None)]:
            with pytest.raises(L.LoraError) as e:
                call()
            assert e.value.status == _lib.LORA_ENODEVICE
        assert state(p) == before
