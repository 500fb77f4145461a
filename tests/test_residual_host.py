"""CPU tests of lora_plan_residual's boundary (include/lorastencil.h): argument validation on addresses nobody dereferences,
which plans have the kernel (read-only option "fused_residual"), the loud failure without a device, and -- through
lora_debug_residual_cover, which replays csrc/residual_tiles.h on the host -- that the launch's workgroups reduce every
interior cell of the region exactly once, no other cell, and the same cells whatever the plan's tuning options say.

Shapes: per family one cell, a grid with partial tiles in every direction and two tiles per direction, and one with more
tiles than the family's workgroup cap (1D 512 points a tile, cap 1024; 2D 32 x 128, cap 768; 3D 32 x 16 x 128, bf16
32 x 16 x 256, cap 1024), so that some workgroup walks a second tile.
"""
import ctypes

import numpy as np
import pytest
from conftest import has_gpu

A = 4096  # a 16-byte aligned address nobody dereferences: every call below is refused before a launch
MAX_GROUPS = 1024  # kReduceMaxGroups (csrc/engine.h)

# (shape, dtype, dims, regions): (0, 0) is the whole interior; the others begin and end inside a tile, or are empty
COVER_CASES = [
    ("1d1r", "f64", (1,), [(0, 0)]),
    ("1d1r", "f64", (1027,), [(0, 0), (2, 515), (510, 1027), (4, 4)]),
    ("1d2r", "f64", (2**19 + 515,), [(0, 0), (1000, 2**19 + 1)]),  # 1026 tiles
    ("star2d1r", "f64", (1, 2), [(0, 0)]),
    ("star2d3r", "f64", (70, 260), [(0, 0), (5, 37), (33, 70), (7, 7)]),
    ("box2d3r", "f64", (801, 3970), [(0, 0), (3, 800)]),  # 26 x 32 = 832 tiles
    ("star3d1r", "f64", (1, 1, 2), [(0, 0)]),
    ("box3d1r", "f64", (35, 17, 130), [(0, 0), (1, 34), (33, 35), (9, 9)]),
    ("box3d1r", "f64", (3, 16401, 2), [(0, 0), (1, 2)]),  # 1026 tiles
    ("box3d1r", "bf16", (1, 1, 8), [(0, 0)]),
    ("star3d1r", "bf16", (35, 17, 264), [(0, 0), (1, 34), (33, 35), (9, 9)]),
    ("box3d1r", "bf16", (3, 16401, 8), [(0, 0), (1, 2)]),  # 1026 tiles
]
TUNING = {1: [("steps_per_launch", 2)], 2: [("rows_per_thread", 4), ("rows_per_thread", 16), ("panel_width", 1), ("nt_store", 1)],
          3: [("z_chunk", 3), ("cols_per_lane", 8), ("lds_dma", 1), ("fused_z_chunk", 8)]}


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def cover_of(L, plan, begin, end):
    from lorastencil_amd import _lib

    cover = np.zeros(L.padded_shape(plan.shape, plan.dims), dtype=np.int32)
    groups = ctypes.c_int(-1)
    rc = _lib.lib().lora_debug_residual_cover(plan._h, begin, end, cover.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(groups))
    assert rc == 0, rc
    return cover, groups.value


def test_arguments_are_checked_before_anything_is_launched(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    df = _lib.GridDiff()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    p = L.Plan("star2d1r", (32, 64))
    assert lib.lora_plan_residual(None, A, 0, 0, ctypes.byref(df), None) == E
    assert lib.lora_plan_residual(p._h, None, 0, 0, ctypes.byref(df), None) == E
    assert lib.lora_plan_residual(p._h, A, 0, 0, None, None) == E
    for begin, end in [(-1, 4), (0, 33), (5, 4), (33, 33)]:
        assert lib.lora_plan_residual(p._h, A, begin, end, ctypes.byref(df), None) == E, (begin, end)
    p1 = L.Plan("1d1r", (300,))
    assert p1.region_granularity == 2
    assert lib.lora_plan_residual(p1._h, A, 1, 300, ctypes.byref(df), None) == E  # an odd begin is a bad range in 1D
    assert lib.lora_plan_residual(p1._h, A, 3, 3, ctypes.byref(df), None) == E
    assert lib.lora_plan_residual(p._h, A + 8, 0, 0, ctypes.byref(df), None) == U
    assert lib.lora_plan_residual(p1._h, A + 8, 0, 0, ctypes.byref(df), None) == U
    cover = (ctypes.c_int * 8)()
    assert lib.lora_debug_residual_cover(None, 0, 0, cover, None) == E
    assert lib.lora_debug_residual_cover(p._h, 0, 0, None, None) == E
    assert lib.lora_debug_residual_cover(p._h, 0, 33, cover, None) == E
    assert lib.lora_debug_residual_cover(p1._h, 1, 5, cover, None) == E


def test_plans_without_the_kernel_are_refused(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    df = _lib.GridDiff()
    U = _lib.LORA_EUNSUPPORTED
    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    assert mfma.get_option("variant") == _lib.VARIANT_MFMA
    cover = (ctypes.c_int * (48 * 80))()
    for p in [L.Plan("star2d1r", (32, 63)), L.Plan("box3d1r", (4, 6, 9)), mfma]:
        assert p.get_option("fused_residual") == 0
        assert lib.lora_plan_residual(p._h, A, 0, 0, ctypes.byref(df), None) == U
        assert "fused residual" in lib.lora_last_error().decode()
        assert lib.lora_debug_residual_cover(p._h, 0, 0, cover, None) == U
        # ... and the answer to a bad argument stays the reductions': it comes first
        assert lib.lora_plan_residual(p._h, None, 0, 0, ctypes.byref(df), None) == _lib.LORA_EINVAL
    # back on the direct variant the 2D plan has it again
    assert mfma.set_variant(_lib.VARIANT_DIRECT).get_option("fused_residual") == 1


def test_eligible_plans_say_so_and_the_key_is_read_only(L):
    from lorastencil_amd import _lib

    for shape, dtype, dims in [("1d1r", "f64", (7,)), ("1d2r", "f64", (300,)), ("star2d1r", "f64", (5, 8)), ("box2d3r", "f64", (33, 130)),
                               ("star3d1r", "f64", (3, 5, 8)), ("box3d1r", "f64", (3, 5, 8)), ("box3d1r", "bf16", (3, 5, 8)),
                               ("star3d1r", "bf16", (3, 5, 16))]:
        p = L.Plan(shape, dims, dtype=dtype)
        sig, name = p.kernel_signature, p.kernel_name
        assert p.get_option("fused_residual") == 1, (shape, dtype, dims)
        for v in (0, 1):
            assert _lib.lib().lora_plan_set_option(p._h, b"fused_residual", v) == _lib.LORA_EINVAL
        assert "residual" not in sig and (p.kernel_signature, p.kernel_name) == (sig, name)


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_residual_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dtype, dims in [("1d1r", "f64", (300,)), ("star2d1r", "f64", (32, 64)), ("box3d1r", "f64", (4, 6, 8)),
                               ("box3d1r", "bf16", (4, 6, 8))]:
        p = L.Plan(shape, dims, dtype=dtype)
        for call in [lambda: p.residual(A), lambda: p.residual(A, 2, 2), lambda: p.residual(A, 0, 2)]:
            with pytest.raises(L.LoraError) as e:
                call()
            assert e.value.status == _lib.LORA_ENODEVICE


@pytest.mark.parametrize("shape,dtype,dims,regions", COVER_CASES, ids=[f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}" for c in COVER_CASES])
def test_every_cell_of_the_region_is_reduced_once(L, shape, dtype, dims, regions):
    p = L.Plan(shape, dims, dtype=dtype)
    for begin, end in regions:
        cover, groups = cover_of(L, p, begin, end)
        want = np.zeros_like(cover)
        lo, hi = (0, dims[0]) if (begin, end) == (0, 0) else (begin, end)
        L.interior(shape, want)[lo:hi] = 1
        assert np.array_equal(cover, want), (begin, end)
        assert (groups == 0) if lo == hi else (1 <= groups <= MAX_GROUPS), (begin, end, groups)
    # more tiles than workgroups: the cap is reached (and the cover above shows the later tiles were walked)
    if max(dims) > 3000:
        _, groups = cover_of(L, p, 0, 0)
        assert groups in (768, 1024)


@pytest.mark.parametrize("shape,dtype,dims,regions", [COVER_CASES[i] for i in (1, 4, 7, 10)], ids=["1d", "2d", "3d", "3d-bf16"])
def test_tuning_options_do_not_move_a_cell(L, shape, dtype, dims, regions):
    p = L.Plan(shape, dims, dtype=dtype)
    before = [cover_of(L, p, b, e) for b, e in regions]
    for key, value in TUNING[len(dims)]:
        q = L.Plan(shape, dims, dtype=dtype).set_option(key, value)
        assert q.get_option(key) == value
        for (b, e), (cover, groups) in zip(regions, before):
            got, g = cover_of(L, q, b, e)
            assert g == groups and np.array_equal(got, cover), (key, value, b, e)
