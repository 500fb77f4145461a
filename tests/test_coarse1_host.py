"""CPU tests of the one-launch coarsest-level CG (include/lorastencil.h): the new symbols and their Python mirrors,
plan option "coarse1" with its thread default, which plans read "cg_small" = 1, the status codes of lora_plan_cg_small in their
documented order on addresses nobody dereferences (no call here is valid with iters > 0, so nothing is launched on a box with
a GPU either), and the CLIs' --coarse1 flag.
"""
import os
import subprocess

import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C = A + (1 << 20), A + (2 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

# every key lora_plan_get_option answered before the options existed
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "leap3", "spans3", "torus", "tapset",
        "variant", "fused_eval", "boundary", "fused_residual", "cg", "mg", "pcg", "source"]

PLANS = [("1d1r", (300,), "f64"), ("star2d1r", (64, 128), "f64"), ("box2d3r", (64, 127), "f64"), ("star3d1r", (16, 16, 32), "f64"),
         ("box3d1r", (16, 16, 32), "bf16")]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature


def test_symbols_and_mirrors(L):
    from lorastencil_amd import _lib

    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    assert "int lora_set_default_coarse1(int on);" in header
    assert ("int lora_plan_cg_small(lora_plan *plan, void *d_x, void *d_r, int iters, double sigma, double tau, double *d_info, "
            "void *stream);") in header
    for name in ("lora_set_default_coarse1", "lora_plan_cg_small"):
        assert getattr(_lib.lib(), name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["lora_plan_cg_small"][1]) == 8
    assert callable(L.set_default_coarse1) and callable(L.Plan.cg_small)


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=[f"{s}-{'x'.join(map(str, d))}-{t}" for s, d, t in PLANS])
def test_option_round_trips_and_moves_nothing_else(L, shape, dims, dtype):
    p = L.Plan(shape, dims, dtype=dtype)
    before = state(p)
    assert p.get_option("coarse1") == 0
    for value, reads in ((1, 1), (0, 0), (7, 1), (-3, 1)):
        p.set_option("coarse1", value)
        assert p.get_option("coarse1") == reads, value
        assert state(p) == before
    p.set_option("coarse1", 0)
    assert state(p) == before == state(L.Plan(shape, dims, dtype=dtype))


def test_thread_default_reaches_new_plans(L):
    assert L.set_default_coarse1(0) == 0
    try:
        assert L.set_default_coarse1(1) == 0
        assert L.set_default_coarse1(5) == 1  # any non-zero value is 1
        for shape, dims, dtype in PLANS:
            assert L.Plan(shape, dims, dtype=dtype).get_option("coarse1") == 1, shape
        p = L.Plan("star2d1r", (64, 64))
        assert L.set_default_coarse1(0) == 1
        assert p.get_option("coarse1") == 1  # a plan keeps what it was created with
        assert L.Plan("star2d1r", (64, 64)).get_option("coarse1") == 0
    finally:
        L.set_default_coarse1(0)


def test_cg_small_is_read_only_and_follows_the_size(L):
    from lorastencil_amd import _lib

    fits = [("star2d1r", (4, 4)), ("box2d3r", (32, 32)), ("star2d1r", (4, 512)), ("box2d3r", (64, 64)), ("star3d1r", (12, 12, 12)),
            ("box3d1r", (4, 4, 4)), ("star2d1r", (1, 2)), ("box3d1r", (16, 16, 16))]
    for shape, dims in fits:
        p = L.Plan(shape, dims)
        assert p.get_option("cg") == 1 and p.get_option("cg_small") == 1, (shape, dims)
        with pytest.raises(L.LoraError) as e:
            p.set_option("cg_small", 0)
        assert e.value.status == _lib.LORA_EINVAL and p.get_option("cg_small") == 1
    too_large = [("star2d1r", (2048, 2048)), ("star2d1r", (64, 66)), ("star3d1r", (16, 16, 18)),  # more than 4096 cells
                 ("star2d1r", (4, 1024)), ("star2d1r", (2, 2048)), ("star2d1r", (1, 4096))]       # 4096 cells, more than 64 KiB of LDS
    for shape, dims in too_large:
        assert L.Plan(shape, dims).get_option("cg_small") == 0, (shape, dims)
    # the plans without the CG kernels: bf16, a source, an odd innermost extent, the matrix-pipe variant; and 1D
    assert L.Plan("box3d1r", (8, 8, 8), dtype="bf16").get_option("cg_small") == 0
    p = L.Plan("star2d1r", (32, 32)).set_source(A)
    assert p.get_option("cg_small") == 0
    assert p.set_source(None).get_option("cg_small") == 1
    assert L.Plan("star2d1r", (32, 31)).get_option("cg_small") == 0
    assert L.Plan("star3d1r", (4, 4, 5)).get_option("cg_small") == 0
    assert L.Plan("box2d3r", (32, 32)).set_variant(_lib.VARIANT_MFMA).get_option("cg_small") == 0
    assert L.Plan("1d1r", (64,)).get_option("cg_small") == 0
    # neither option moves the other, nor the boundary either of them
    q = L.Plan("star2d1r", (32, 32)).set_option("coarse1", 1).set_boundary("dirichlet")
    assert q.get_option("cg_small") == 1 and q.get_option("coarse1") == 1


def test_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    for shape, dims in (("star2d1r", (4, 4)), ("box3d1r", (4, 6, 8))):
        p = L.Plan(shape, dims)
        h = p._h
        call = lib.lora_plan_cg_small
        # -- LORA_EINVAL: a null plan or buffer, equal buffers, a negative count, a pair that is not finite
        assert call(None, A, B, 0, 1.0, 1.0, None, None) == E
        assert call(h, None, B, 0, 1.0, 1.0, None, None) == E
        assert call(h, A, None, 0, 1.0, 1.0, None, None) == E
        assert call(h, A, A, 0, 1.0, 1.0, None, None) == E
        assert call(h, A, B, -1, 1.0, 1.0, None, None) == E
        for bad in (inf, -inf, nan):
            assert call(h, A, B, 0, bad, 1.0, None, None) == E
            assert call(h, A, B, 0, 1.0, bad, None, None) == E
        # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument with a misaligned buffer, on a plan without the kernel
        assert call(h, A + 8, B, -1, 1.0, 1.0, None, None) == E
        p.set_source(C)
        assert call(h, A + 8, B, 4, nan, 1.0, None, None) == E
        # -- LORA_EUNSUPPORTED: a misaligned buffer, before the plan is looked at
        assert call(h, A + 8, B, 4, 1.0, 1.0, None, None) == U and "16-byte" in lib.lora_last_error().decode()
        assert call(h, A, B + 8, 4, 1.0, 1.0, None, None) == U and "16-byte" in lib.lora_last_error().decode()
        # -- LORA_EUNSUPPORTED: a plan whose option "cg_small" reads 0, also with nothing to do
        assert p.get_option("cg_small") == 0
        assert call(h, A, B, 4, 1.0, 1.0, None, None) == U and "cg_small" in lib.lora_last_error().decode()
        assert call(h, A, B, 0, 1.0, 1.0, None, None) == U
        p.set_source(None)
        # -- nothing to do is no error, launches nothing and needs no device
        assert call(h, A, B, 0, 1.0, 1.0, None, None) == 0
        assert call(h, A, B, 0, -1.0, 8.0, C, None) == 0
    big = L.Plan("star2d1r", (2048, 2048))
    assert lib.lora_plan_cg_small(big._h, A, B, 4, 1.0, 1.0, None, None) == U


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_launch_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in (("star2d1r", (4, 4)), ("box3d1r", (4, 6, 8))):
        with pytest.raises(L.LoraError) as e:
            L.Plan(shape, dims).cg_small(A, B, 4)
        assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_coarse1_parse(engine_built):
    for dim, args in ((2, ["star2d1r", "64", "64", "4"]), (3, ["star3d1r", "8", "8", "8", "4"])):
        rc, out, err = cli(dim, *args, "--coarse1")
        assert rc == 1 and out == "" and err.startswith("--coarse1 ") and err.count("\n") == 1, dim
        rc, out, err = cli(dim, *args, "--cg", "--until=1e-9", "--coarse1")
        assert rc == 1 and out == "" and err.startswith("--coarse1 "), dim
    rc, out, err = cli(1, "1d1r", "64", "4", "--coarse1")
    assert rc == 1 and out == "" and err == "Unknown option: --coarse1\n"


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_coarse1_reaches_the_operators(engine_built):
    for extra in (["--mg", "--until=1e-9"], ["--pcg", "--until=1e-9"], ["--implicit=64", "--precond=mg"]):
        rc, out, err = cli(2, "star2d1r", "64", "64", "8", "--normalize", *extra, "--coarse1")
        assert out.startswith("INFO: shape = "), (extra, err)
        assert rc == 1 and "no HIP device" in out, extra
    rc, out, _ = cli(3, "star3d1r", "16", "16", "16", "8", "--normalize", "--mg", "--until=1e-9", "--coarse1")
    assert out.startswith("INFO: shape = ") and rc == 1 and "no HIP device" in out
