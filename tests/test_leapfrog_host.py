"""CPU tests of the leapfrog entries' boundary (lora_plan_step_leapfrog ... lora_run_host_leapfrog; include/lorastencil.h): the
symbols, the status codes in their documented order on addresses nobody dereferences, which plans have which depth, that no
leapfrog call changes what a plan resolves to, the loud failure without a device, and the CLI's --leapfrog flag.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C, D = A + (1 << 20), A + (2 << 20), A + (3 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

ENTRIES = ["lora_plan_leapfrog_depth", "lora_plan_step_leapfrog", "lora_plan_step_leapfrog_region", "lora_plan_step2_leapfrog",
           "lora_plan_step2_leapfrog_region", "lora_plan_run_leapfrog", "lora_plan_prepare_leapfrog", "lora_run_host_leapfrog"]

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
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature


def test_symbols_are_exported(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    for name in ENTRIES:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert "int lora_plan_step_leapfrog(lora_plan *plan, const void *d_cur, void *d_prev, double c, void *stream);" in header
    assert "int lora_plan_run_leapfrog(lora_plan *plan, void *d_prev, void *d_cur, double c, int times, void *stream);" in header
    for name in ("step_leapfrog", "step_leapfrog_region", "step2_leapfrog", "step2_leapfrog_region", "run_leapfrog", "prepare_leapfrog"):
        assert callable(getattr(L.Plan, name)), name
    assert isinstance(L.Plan.leapfrog_depth, property) and callable(L.run_host_leapfrog)


def test_depth_table(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    assert lib.lora_plan_leapfrog_depth(None) == 0
    assert L.Plan("1d1r", (300,)).leapfrog_depth == 1
    assert L.Plan("star2d1r", (64, 128)).leapfrog_depth == 2
    assert L.Plan("star2d1r", (64, 127)).leapfrog_depth == 1
    box = L.Plan("box2d3r", (64, 128))
    assert box.leapfrog_depth == 2
    box.set_variant(_lib.VARIANT_MFMA)
    assert box.get_option("variant") == _lib.VARIANT_MFMA and box.leapfrog_depth == 0
    assert L.Plan("box3d1r", (16, 16, 32)).leapfrog_depth == 1
    assert L.Plan("box3d1r", (16, 16, 32), dtype="bf16").leapfrog_depth == 0
    for shape, dims, depth in [("1d1r", (300,), 1), ("star2d1r", (64, 128), 2), ("star2d1r", (64, 127), 1), ("box3d1r", (16, 16, 32), 1)]:
        p = L.Plan(shape, dims).set_source(A)
        assert p.leapfrog_depth == 0, shape
        p.set_source(None)
        assert p.leapfrog_depth == depth, shape
    # neither the boundary nor the scratch option moves it: they choose the run's schedule, not the kernels a plan has
    assert L.Plan("star2d1r", (64, 128)).set_boundary("periodic").set_option("scratch", 0).leapfrog_depth == 2


def test_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    p = L.Plan("star2d1r", (32, 64))
    h = p._h
    # -- LORA_EINVAL: null plan / pointer, non-finite c, bad range, times < 0, equal buffers
    assert lib.lora_plan_step_leapfrog(None, A, B, -1.0, None) == E
    assert lib.lora_plan_step_leapfrog_region(None, A, B, -1.0, 0, 1, None) == E
    assert lib.lora_plan_step2_leapfrog(None, A, B, C, D, -1.0, None) == E
    assert lib.lora_plan_step2_leapfrog_region(None, A, B, C, D, -1.0, 0, 1, None) == E
    assert lib.lora_plan_run_leapfrog(None, A, B, -1.0, 1, None) == E
    assert lib.lora_plan_prepare_leapfrog(None, 1) == E
    for cur, prev in ((None, B), (A, None), (A, A)):
        assert lib.lora_plan_step_leapfrog(h, cur, prev, -1.0, None) == E
        assert lib.lora_plan_run_leapfrog(h, prev, cur, -1.0, 3, None) == E
    for c in (inf, -inf, nan):
        assert lib.lora_plan_step_leapfrog(h, A, B, c, None) == E
        assert lib.lora_plan_step2_leapfrog(h, A, B, C, D, c, None) == E
        assert lib.lora_plan_run_leapfrog(h, A, B, c, 3, None) == E
    for begin, end in ((-1, 4), (0, 33), (5, 4)):
        assert lib.lora_plan_step_leapfrog_region(h, A, B, -1.0, begin, end, None) == E
        assert lib.lora_plan_step2_leapfrog_region(h, A, B, C, D, -1.0, begin, end, None) == E
    p1 = L.Plan("1d1r", (300,))
    assert p1.region_granularity == 2
    assert lib.lora_plan_step_leapfrog_region(p1._h, A, B, -1.0, 3, 10, None) == E
    assert lib.lora_plan_run_leapfrog(h, A, B, -1.0, -1, None) == E
    assert lib.lora_plan_prepare_leapfrog(h, -1) == E
    bufs = [A, B, C, D]
    for i in range(4):
        for j in range(i + 1, 4):
            args = list(bufs)
            args[j] = args[i]
            assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == E, (i, j)
    for i in range(4):
        args = list(bufs)
        args[i] = None
        assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == E, i
    # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument on a plan without the kernels, with a misaligned buffer
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    assert lib.lora_plan_step_leapfrog(bf._h, A + 8, A + 8, -1.0, None) == E
    assert lib.lora_plan_step_leapfrog(bf._h, A, B, nan, None) == E
    assert lib.lora_plan_run_leapfrog(bf._h, A, B, -1.0, -1, None) == E
    # -- LORA_EUNSUPPORTED: a misaligned buffer
    for cur, prev in ((A + 8, B), (A, B + 8)):
        assert lib.lora_plan_step_leapfrog(h, cur, prev, -1.0, None) == U and "16-byte" in lib.lora_last_error().decode()
        assert lib.lora_plan_run_leapfrog(h, prev, cur, -1.0, 2, None) == U
    for i in range(4):
        args = list(bufs)
        args[i] += 8
        assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == U, i
    # -- LORA_EUNSUPPORTED: the plans without the kernels
    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    src = L.Plan("star2d1r", (32, 64)).set_source(D)
    for q in (bf, mfma, src):
        n = q.dims[0]
        assert lib.lora_plan_step_leapfrog(q._h, A, B, -1.0, None) == U
        assert lib.lora_plan_step_leapfrog_region(q._h, A, B, -1.0, 0, n, None) == U
        assert lib.lora_plan_run_leapfrog(q._h, A, B, -1.0, 4, None) == U
        assert lib.lora_plan_run_leapfrog(q._h, A, B, -1.0, 0, None) == U
        assert lib.lora_plan_prepare_leapfrog(q._h, 4) == U
        if len(q.dims) == 2:
            assert lib.lora_plan_step2_leapfrog(q._h, A, B, C, D, -1.0, None) == U
    # -- the two-step entries on plans that have no two-step kernel
    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8))]:
        q = L.Plan(shape, dims)
        assert q.leapfrog_depth == 1
        assert lib.lora_plan_step2_leapfrog(q._h, A, B, C, D, -1.0, None) == U, shape
        assert lib.lora_plan_step2_leapfrog_region(q._h, A, B, C, D, -1.0, 0, 2, None) == U, shape
    # -- nothing to do is no error and needs no device
    assert lib.lora_plan_run_leapfrog(h, A, B, -1.0, 0, None) == 0
    assert lib.lora_plan_step_leapfrog_region(h, A, B, -1.0, 7, 7, None) == 0
    assert lib.lora_plan_step2_leapfrog_region(h, A, B, C, D, 0.5, 7, 7, None) == 0


def test_host_entry_status_codes(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    a = np.zeros(L.padded_shape("star2d1r", (8, 16)))
    out = np.zeros_like(a)
    dims, sid = L.ops._dims_arg((8, 16)), L.ops.shape_id("star2d1r")
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    assert lib.lora_run_host_leapfrog(sid, None, dp(a), dp(out), None, -1.0, 1, dims, 1, None) == E
    assert lib.lora_run_host_leapfrog(sid, dp(a), None, dp(out), None, -1.0, 1, dims, 1, None) == E
    assert lib.lora_run_host_leapfrog(sid, dp(a), dp(a), None, None, -1.0, 1, dims, 1, None) == E
    assert lib.lora_run_host_leapfrog(sid, dp(a), dp(a), dp(out), None, -1.0, 1, None, 1, None) == E
    assert lib.lora_run_host_leapfrog(sid, dp(a), dp(a), dp(out), None, -1.0, -1, dims, 1, None) == E
    assert lib.lora_run_host_leapfrog(sid, dp(a), dp(a), dp(out), None, float("nan"), 1, dims, 1, None) == E
    assert L.set_default_source(a) is None
    try:
        assert lib.lora_run_host_leapfrog(sid, dp(a), dp(a), dp(out), None, -1.0, 1, dims, 1, None) == U
        assert "source" in lib.lora_last_error().decode()
    finally:
        assert L.set_default_source(None) is a
    with pytest.raises(ValueError):
        L.run_host_leapfrog("star2d1r", a, np.zeros((3, 3)))


@pytest.mark.parametrize("shape,dims", [("1d2r", (300,)), ("star2d1r", (64, 128)), ("box2d3r", (64, 127)), ("box3d1r", (16, 16, 32))],
                         ids=["1d", "2d", "2d-odd", "3d"])
def test_leapfrog_calls_leave_the_plan_as_it_was(L, shape, dims):
    """c and the buffers are call arguments: every key's value, the kernel name and the signature stay"""
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p = L.Plan(shape, dims)
    before = state(p)
    n = dims[0]
    if not has_gpu():  # (with a device these would launch on addresses nobody owns; tests/test_gpu_leapfrog.py covers them there)
        lib.lora_plan_step_leapfrog(p._h, A, B, -1.0, None)
        lib.lora_plan_step_leapfrog_region(p._h, A, B, 0.7, 0, n, None)
        lib.lora_plan_step2_leapfrog(p._h, A, B, C, D, -1.0, None)
        lib.lora_plan_step2_leapfrog_region(p._h, A, B, C, D, 0.7, 0, n, None)
        lib.lora_plan_run_leapfrog(p._h, A, B, -0.5, 9, None)
    assert lib.lora_plan_step_leapfrog_region(p._h, A, B, 0.7, 2, 2, None) == 0
    assert lib.lora_plan_run_leapfrog(p._h, A, B, -0.5, 0, None) == 0
    assert lib.lora_plan_prepare_leapfrog(p._h, 9) == 0
    assert p.leapfrog_depth in (1, 2)
    assert state(p) == before
    assert state(p) == state(L.Plan(shape, dims))


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_leapfrog_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8)), ("star3d1r", (3, 5, 7))]:
        for bc in ("reference", "periodic"):
            p = L.Plan(shape, dims).set_boundary(bc)
            calls = [lambda: p.step_leapfrog(A, B), lambda: p.step_leapfrog_region(A, B, 0.7, 0, 2), lambda: p.run_leapfrog(A, B, -1.0, 1),
                     lambda: p.run_leapfrog(A, B, -1.0, 9)]
            if p.leapfrog_depth == 2:
                calls.append(lambda: p.step2_leapfrog(A, B, C, D))
            for i, call in enumerate(calls):
                with pytest.raises(L.LoraError) as e:
                    call()
                assert e.value.status == _lib.LORA_ENODEVICE, (shape, bc, i)
            p.prepare_leapfrog(9)  # allocates nothing here, and says so by staying quiet
    a = np.zeros(L.padded_shape("star2d1r", (32, 64)))
    with pytest.raises(L.LoraError) as e:
        L.run_host_leapfrog("star2d1r", a, a, times=1)
    assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_leapfrog_parse_errors_and_refusals(engine_built):
    need = "Invalid argument: --leapfrog=C needs a finite number C.\n"
    for bad in ("--leapfrog=", "--leapfrog=abc", "--leapfrog=1x", "--leapfrog=inf", "--leapfrog=nan", "--leapfrog=-1e999"):
        rc, out, err = cli(2, "star2d1r", "64", "64", "4", bad)
        assert rc == 1 and err == need and out == "", bad
    refused = "--leapfrog runs on one GPU in fp64"
    for extra in (["--gpus=2"], ["--gpus=1"], ["--grid=1x2"], ["--check"], ["--until=1e-9"], ["--source=const:1"]):
        for flag in ("--leapfrog", "--leapfrog=-0.5"):
            rc, out, err = cli(2, "star2d1r", "64", "64", "4", flag, *extra)
            assert rc == 1 and err.startswith(refused) and err.count("\n") == 1 and out == "", (flag, extra)
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--leapfrog")
    assert rc == 1 and err.startswith(refused) and out == ""
    rc, out, err = cli(1, "1d1r", "64", "4", "--source=point:2", "--leapfrog=0.25")
    assert rc == 1 and err.startswith(refused) and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_leapfrog_reaches_the_operator(engine_built):
    for dim, args in ((2, ["star2d1r", "64", "128", "7", "--leapfrog"]), (1, ["1d1r", "64", "3", "--leapfrog=-0.5"]),
                      (3, ["box3d1r", "8", "8", "8", "2", "--leapfrog=-1", "--bc=periodic"])):
        rc, out, _ = cli(dim, *args)
        assert out.startswith("INFO: shape = ")
        assert rc == 1 and "no HIP device" in out
