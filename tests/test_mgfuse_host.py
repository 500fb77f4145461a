"""CPU tests of the fused defect-and-restrict launch (include/lorastencil.h): the new symbols and their Python
mirrors, plan option "mgfuse" with its thread default, the status codes of lora_plan_mg_defect_restrict in their documented order
on addresses nobody dereferences (no call here gets past the device check on a box without a GPU, and none that would is made on
a box with one), and the CLIs' --mgfuse flag.
"""
import os
import subprocess

import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C = A + (1 << 20), A + (2 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

# every key lora_plan_get_option answered before the option existed
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "leap3", "coarse1", "spans3", "torus",
        "tapset", "variant", "fused_eval", "boundary", "fused_residual", "cg", "mg", "pcg", "cg_small", "source"]

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
    assert "int lora_set_default_mgfuse(int on);" in header
    assert ("int lora_plan_mg_defect_restrict(lora_plan *plan, const void *d_u, const void *d_f, void *d_coarse, double scale, "
            "void *stream);") in header
    for name in ("lora_set_default_mgfuse", "lora_plan_mg_defect_restrict"):
        assert getattr(_lib.lib(), name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["lora_plan_mg_defect_restrict"][1]) == 6
    assert callable(L.set_default_mgfuse) and callable(L.Plan.mg_defect_restrict)


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=[f"{s}-{'x'.join(map(str, d))}-{t}" for s, d, t in PLANS])
def test_option_round_trips_and_moves_nothing_else(L, shape, dims, dtype):
    p = L.Plan(shape, dims, dtype=dtype)
    before = state(p)
    assert p.get_option("mgfuse") == 0
    for value, reads in ((1, 1), (0, 0), (7, 1), (-3, 1)):
        p.set_option("mgfuse", value)
        assert p.get_option("mgfuse") == reads, value
        assert state(p) == before
    p.set_option("mgfuse", 0)
    assert state(p) == before == state(L.Plan(shape, dims, dtype=dtype))


def test_thread_default_reaches_new_plans(L):
    assert L.set_default_mgfuse(0) == 0
    try:
        old = L.Plan("star2d1r", (64, 64))
        assert L.set_default_mgfuse(1) == 0
        assert L.set_default_mgfuse(5) == 1  # any non-zero value is 1
        for shape, dims, dtype in PLANS:
            p = L.Plan(shape, dims, dtype=dtype)
            assert p.get_option("mgfuse") == 1 and p.get_option("coarse1") == 0, shape
        assert old.get_option("mgfuse") == 0  # an existing plan is left alone
        p = L.Plan("star2d1r", (64, 64))
        assert L.set_default_mgfuse(0) == 1
        assert p.get_option("mgfuse") == 1  # a plan keeps what it was created with
        assert L.Plan("star2d1r", (64, 64)).get_option("mgfuse") == 0
        # the two defaults do not move each other
        assert L.set_default_coarse1(1) == 0
        q = L.Plan("star2d1r", (64, 64))
        assert q.get_option("mgfuse") == 0 and q.get_option("coarse1") == 1
    finally:
        L.set_default_mgfuse(0)
        L.set_default_coarse1(0)


def test_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    call = lib.lora_plan_mg_defect_restrict
    # plans whose option "mg" reads 0: 1D, bf16, an odd innermost extent in 2D, extents that do not coarsen
    no_mg = [L.Plan("1d1r", (300,)), L.Plan("box3d1r", (16, 16, 32), dtype="bf16"), L.Plan("box2d3r", (64, 127)),
             L.Plan("star2d1r", (7, 64)), L.Plan("star2d1r", (64, 6)), L.Plan("star3d1r", (16, 6, 32))]
    for p in no_mg:
        assert p.get_option("mg") == 0
    for p in [L.Plan("star2d1r", (64, 64)), L.Plan("box3d1r", (8, 10, 12))] + no_mg:
        h = p._h
        # -- 1. LORA_EINVAL: a null plan, d_u or d_coarse (d_f may be null)
        assert call(None, A, B, C, 1.0, None) == E
        assert call(h, None, B, C, 1.0, None) == E
        assert call(h, A, B, None, 1.0, None) == E
        assert call(h, None, None, None, nan, None) == E
        # -- 2. LORA_EINVAL: a scale that is not finite
        for bad in (inf, -inf, nan):
            assert call(h, A, B, C, bad, None) == E
            assert call(h, A, None, C, bad, None) == E
        # -- 3. LORA_EINVAL: any two buffers equal
        assert call(h, A, B, A, 1.0, None) == E
        assert call(h, A, A, C, 1.0, None) == E
        assert call(h, A, C, C, 1.0, None) == E
        assert call(h, A, None, A, 1.0, None) == E
        # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument with a misaligned buffer
        assert call(h, A + 8, B, C, nan, None) == E
        assert call(h, A + 8, A + 8, C, 1.0, None) == E
        # -- 4. LORA_EUNSUPPORTED: a misaligned buffer, before the plan is looked at
        for bufs in ((A + 8, B, C), (A, B + 8, C), (A, B, C + 8), (A + 8, None, C)):
            assert call(h, *bufs, 1.0, None) == U and "16-byte" in lib.lora_last_error().decode(), bufs
    # -- 5. LORA_EUNSUPPORTED: a plan whose option "mg" reads 0, before a device is asked for
    for p in no_mg:
        assert call(p._h, A, B, C, 1.0, None) == U and "multigrid" in lib.lora_last_error().decode()
        assert call(p._h, A, None, C, 0.37, None) == U
    # a plan that carries a source has no CG kernels, so none of these: f is an argument
    p = L.Plan("star2d1r", (64, 64)).set_source(C)
    assert p.get_option("mg") == 0 and call(p._h, A, None, B, 1.0, None) == U
    assert p.set_source(None).get_option("mg") == 1


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_launch_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in (("star2d1r", (64, 64)), ("box3d1r", (8, 10, 12))):
        for f in (B, None):
            with pytest.raises(L.LoraError) as e:
                L.Plan(shape, dims).mg_defect_restrict(A, f, C, 0.37)
            assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_mgfuse_parse(engine_built):
    """refused exactly as --coarse1 is: the same exit code, nothing on stdout, one line that begins with the flag"""
    for dim, args in ((2, ["star2d1r", "64", "64", "4"]), (3, ["star3d1r", "8", "8", "8", "4"])):
        for extra in ([], ["--cg", "--until=1e-9"]):
            rc, out, err = cli(dim, *args, *extra, "--mgfuse")
            rc1, out1, err1 = cli(dim, *args, *extra, "--coarse1")
            assert (rc, out) == (rc1, out1) == (1, ""), (dim, extra)
            assert err.startswith("--mgfuse ") and err1.startswith("--coarse1 ") and err.count("\n") == err1.count("\n") == 1
    rc, out, err = cli(1, "1d1r", "64", "4", "--mgfuse")
    assert rc == 1 and out == "" and err == "Unknown option: --mgfuse\n"


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_mgfuse_reaches_the_operators(engine_built):
    for extra in (["--mg", "--until=1e-9"], ["--pcg", "--until=1e-9"], ["--implicit=64", "--precond=mg"]):
        for flags in (["--mgfuse"], ["--mgfuse", "--coarse1"]):
            rc, out, err = cli(2, "star2d1r", "64", "64", "8", "--normalize", *extra, *flags)
            assert out.startswith("INFO: shape = "), (extra, err)
            assert rc == 1 and "no HIP device" in out, extra
    rc, out, _ = cli(3, "star3d1r", "16", "16", "16", "8", "--normalize", "--mg", "--until=1e-9", "--mgfuse")
    assert out.startswith("INFO: shape = ") and rc == 1 and "no HIP device" in out
