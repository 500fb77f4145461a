"""CPU tests of the source term's boundary (lora_plan_set_source, lora_set_default_source; include/lorastencil.h): the symbols,
the status codes on addresses nobody dereferences, what a plan with a source resolves to -- and that it resolves exactly as
before once the source is gone --, kernel name and signature, the loud failure without a device, and the CLI's --source flag.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT, has_gpu

A = 4096  # a 16-byte aligned address nobody dereferences
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

# every key lora_plan_get_option answers in the shipped library
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "spans3", "torus", "tapset", "variant",
        "fused_eval", "boundary", "fused_residual", "source"]

# (shape, dims, boundary, requested depth or None) -> steps_per_launch with a source, kernel with a source
FAMILIES = [
    ("1d1r", (300,), "reference", None, 1, "stencil1d_source_kernel"),
    ("1d2r", (300,), "periodic", 8, 1, "stencil1d_source_kernel"),
    ("star2d1r", (64, 128), "reference", None, 2, "stencil2d_source2_kernel"),
    ("star2d3r", (64, 128), "dirichlet", None, 2, "stencil2d_source2_kernel"),
    ("box2d3r", (64, 128), "reference", 6, 2, "stencil2d_source2_kernel"),
    ("box2d3r", (64, 128), "dirichlet", 4, 2, "stencil2d_source2_kernel"),
    ("star2d1r", (64, 128), "reference", 1, 1, "stencil2d_source_kernel"),
    ("star2d1r", (64, 128), "periodic", None, 1, "stencil2d_source_kernel"),
    ("star2d1r", (64, 127), "reference", None, 1, "stencil2d_generic_source_kernel"),
    ("star2d1r", (16384, 16384), "reference", None, 2, "stencil2d_source2_kernel"),
    ("star3d1r", (16, 16, 32), "reference", None, 1, "stencil3d_source_kernel"),
    ("box3d1r", (16, 16, 32), "dirichlet", 2, 1, "stencil3d_source_kernel"),
    ("star3d1r", (512, 512, 512), "reference", None, 1, "stencil3d_source_kernel"),
    ("box3d1r", (16, 16, 31), "reference", None, 1, "stencil3d_generic_source_kernel"),
]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def make(L, shape, dims, bc, depth):
    p = L.Plan(shape, dims).set_boundary(bc)
    if depth is not None:
        p.set_option("steps_per_launch", depth)
    return p


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature


def test_symbols_are_exported(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    assert lib.lora_plan_set_source and lib.lora_set_default_source
    assert "lora_plan_set_source" in _lib.SIGNATURES and "lora_set_default_source" in _lib.SIGNATURES
    assert callable(L.Plan.set_source) and callable(L.set_default_source)
    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    assert "int lora_plan_set_source(lora_plan *plan, const void *d_source);" in header
    assert "const double *lora_set_default_source(const double *padded_host_source);" in header


def test_set_source_status_codes(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    assert lib.lora_plan_set_source(None, A) == E
    p = L.Plan("star2d1r", (32, 64))
    before = state(p)
    assert lib.lora_plan_set_source(p._h, A + 8) == U and "16-byte" in lib.lora_last_error().decode()
    assert state(p) == before and p.get_option("source") == 0
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    assert lib.lora_plan_set_source(bf._h, A) == U
    assert lib.lora_plan_set_source(bf._h, None) == 0 and bf.get_option("source") == 0
    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    assert mfma.get_option("variant") == _lib.VARIANT_MFMA
    assert lib.lora_plan_set_source(mfma._h, A) == U and mfma.get_option("source") == 0
    # ... and the other way round: the variant is refused on a plan that has a source, which stays as it was
    q = L.Plan("box2d3r", (32, 64)).set_source(A)
    with_source = state(q)
    assert lib.lora_plan_set_variant(q._h, _lib.VARIANT_MFMA) == U
    assert state(q) == with_source and q.get_option("variant") == _lib.VARIANT_DIRECT
    assert lib.lora_plan_set_variant(q._h, _lib.VARIANT_DIRECT) == 0
    q.set_source(None)
    assert q.set_variant(_lib.VARIANT_MFMA).get_option("variant") == _lib.VARIANT_MFMA
    # the key is read-only
    assert lib.lora_plan_set_option(p._h, b"source", 1) == E


@pytest.mark.parametrize("shape,dims,bc,depth,want_depth,want_kernel", FAMILIES,
                         ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}" for c in FAMILIES])
def test_resolution_with_a_source_and_after_it_is_removed(L, shape, dims, bc, depth, want_depth, want_kernel):
    fresh = make(L, shape, dims, bc, depth)
    p = make(L, shape, dims, bc, depth)
    plain_name, plain_sig = p.kernel_name, p.kernel_signature
    assert p.get_option("source") == 0 and "src=" not in plain_sig
    p.set_source(A)
    assert p.get_option("source") == 1
    assert p.get_option("steps_per_launch") == want_depth
    assert p.get_option("fused_residual") == 0
    assert p.kernel_name == want_kernel != plain_name
    sig = p.kernel_signature
    assert sig.startswith(want_kernel + "[") and "src=1" in sig and sig != plain_sig
    # every option set while the source is there keeps the depth; the tuning keys do not reach the signature
    for key, value in [("rows_per_thread", 16), ("panel_width", 1), ("nt_store", 1), ("z_chunk", 3), ("lowrank_valu", 0)]:
        p.set_option(key, value)
        assert (p.get_option("steps_per_launch"), p.kernel_signature) == (want_depth, sig), key
        fresh.set_option(key, value)
    p.set_source(A + 16)
    assert (p.get_option("steps_per_launch"), p.kernel_signature) == (want_depth, sig)
    p.set_source(None)
    assert state(p) == state(fresh)
    assert "src=" not in p.kernel_signature


def test_source_and_output_must_differ_and_other_depths_are_refused(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    B, C = A + 65536, A + 131072
    p2 = L.Plan("star2d1r", (32, 64)).set_source(C)
    assert lib.lora_plan_step(p2._h, A, C, None) == E
    assert lib.lora_plan_stepn_region(p2._h, 2, A, C, 0, 32, None) == E
    for napps in (3, 4, 6):
        assert lib.lora_plan_stepn_region(p2._h, napps, A, B, 0, 32, None) == U
    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8))]:
        p = L.Plan(shape, dims).set_source(C)
        for napps in (2, 3, 4, 8):
            assert lib.lora_plan_stepn_region(p._h, napps, A, B, 0, dims[0], None) == U, (shape, napps)
        assert lib.lora_plan_step2(p._h, A, B, None) == U
        df = _lib.GridDiff()
        assert lib.lora_plan_residual(p._h, A, 0, 0, ctypes.byref(df), None) == U


def test_drivers_that_take_no_source_refuse_the_default_one(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    U = _lib.LORA_EUNSUPPORTED
    f = np.zeros(L.padded_shape("box3d1r", (8, 8, 8)))
    a, out = np.zeros_like(f), np.zeros_like(f)
    a16 = np.zeros(f.shape, dtype=np.uint16)
    dims, grid = L.ops._dims_arg((8, 8, 8)), (ctypes.c_int * 2)(1, 2)
    sid = L.ops.shape_id("box3d1r")
    assert L.set_default_source(f) is None
    try:
        assert lib.lora_run_host_multi(sid, _lib.F64, a.ctypes.data, out.ctypes.data, None, 1, dims, 2, 1, None) == U
        assert "source" in lib.lora_last_error().decode()
        assert lib.lora_run_host_blocks(sid, _lib.F64, a.ctypes.data, out.ctypes.data, None, 1, dims, grid, 1, None) == U
        assert lib.lora_run_host_dtype(sid, _lib.BF16, a16.ctypes.data, a16.ctypes.data, None, 1, dims, 1, None) == U
    finally:
        assert L.set_default_source(None) is f
    # the C function returns the previous pointer, like lora_set_default_boundary returns the previous boundary
    assert lib.lora_set_default_source(f.ctypes.data) is None
    assert lib.lora_set_default_source(None) == f.ctypes.data
    with pytest.raises(ValueError):
        L.run_host("box3d1r", a, source=np.zeros((3, 3, 3)))


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_a_step_with_a_source_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8))]:
        p = L.Plan(shape, dims).set_source(A + 131072)
        calls = [lambda: p.step(A, A + 65536), lambda: p.step_region(A, A + 65536, 0, 2)]
        if p.get_option("steps_per_launch") == 2:
            calls.append(lambda: p.stepk(A, A + 65536))
        for call in calls:
            with pytest.raises(L.LoraError) as e:
                call()
            assert e.value.status == _lib.LORA_ENODEVICE, shape
    f = np.zeros(L.padded_shape("star2d1r", (32, 64)))
    with pytest.raises(L.LoraError) as e:
        L.run_host("star2d1r", f, times=1, source=f)
    assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_source_parse_errors_and_refusals(engine_built):
    need = "Invalid argument: --source=const:V or --source=point:V needs a number V.\n"
    for bad in ("--source=", "--source=const", "--source=const:", "--source=point:abc", "--source=const:1x", "--source=line:1"):
        rc, out, err = cli(2, "star2d1r", "64", "64", "4", bad)
        assert rc == 1 and err == need and out == "", bad
    refused = "--source runs on one GPU in fp64"
    for extra in (["--gpus=2"], ["--gpus=1"], ["--grid=1x2"], ["--check"]):
        rc, out, err = cli(2, "star2d1r", "64", "64", "4", "--source=const:1", *extra)
        assert rc == 1 and err.startswith(refused) and out == "", extra
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--source=point:2")
    assert rc == 1 and err.startswith(refused) and out == ""
    rc, out, err = cli(1, "1d1r", "64", "4", "--until=1e-9", "--source=point:2", "--check")
    assert rc == 1 and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_with_a_source_reaches_the_operator(engine_built):
    for args in (["--source=point:1"], ["--source=const:-0.5e-3", "--until=1e-9", "--bc=dirichlet"]):
        rc, out, _ = cli(2, "star2d1r", "64", "128", "2", *args)
        assert out.startswith("INFO: shape = star_2d1r, m = 64, n = 128, times = 2\n")
        assert rc == 1 and "no HIP device" in out
