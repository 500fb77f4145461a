"""CPU tests of plan option "leap3" (3D fp64: two leapfrog steps per launch; include/lorastencil.h): the option and
its thread default, which plans read which leapfrog depth with it, that it moves nothing else a plan resolves to, the status codes
of the two-step entries on a 3D plan in their documented order on addresses nobody dereferences, and the CLI's --leap3 flag.
"""
import os
import subprocess

import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C, D, F = A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (4 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")

# every key lora_plan_get_option answered before the option existed
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "spans3", "torus", "tapset", "variant",
        "fused_eval", "boundary", "fused_residual", "source"]

PLANS = [("1d1r", (300,), "f64"), ("1d2r", (301,), "f64"), ("star2d1r", (64, 128), "f64"), ("box2d3r", (64, 127), "f64"),
         ("star3d1r", (16, 16, 32), "f64"), ("box3d1r", (16, 16, 33), "f64"), ("box3d1r", (16, 16, 32), "bf16")]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature


def test_symbol_and_mirrors(L):
    from lorastencil_amd import _lib

    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    assert "int lora_set_default_leap3(int on);" in header and "leap3" in header
    assert getattr(_lib.lib(), "lora_set_default_leap3") and "lora_set_default_leap3" in _lib.SIGNATURES
    assert callable(L.set_default_leap3)


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=[f"{s}-{'x'.join(map(str, d))}-{t}" for s, d, t in PLANS])
def test_option_round_trips_on_every_plan(L, shape, dims, dtype):
    p = L.Plan(shape, dims, dtype=dtype)
    assert p.get_option("leap3") == 0
    for value, reads in ((1, 1), (0, 0), (7, 1), (-3, 1), (0, 0)):
        p.set_option("leap3", value)
        assert p.get_option("leap3") == reads, value


def test_thread_default_reaches_new_plans(L):
    assert L.set_default_leap3(0) == 0
    try:
        assert L.set_default_leap3(1) == 0
        assert L.set_default_leap3(5) == 1  # any non-zero value is 1
        for shape, dims, dtype in PLANS:
            assert L.Plan(shape, dims, dtype=dtype).get_option("leap3") == 1, shape
        p = L.Plan("star3d1r", (16, 16, 32))
        assert p.leapfrog_depth == 2
        assert L.set_default_leap3(0) == 1
        assert p.get_option("leap3") == 1  # a plan keeps what it was created with
        assert L.Plan("star3d1r", (16, 16, 32)).get_option("leap3") == 0
    finally:
        L.set_default_leap3(0)


def test_depth_table(L):
    from lorastencil_amd import _lib

    on = lambda shape, dims, **kw: L.Plan(shape, dims, **kw).set_option("leap3", 1)  # noqa: E731
    assert on("box3d1r", (16, 16, 32)).leapfrog_depth == 2
    assert on("star3d1r", (16, 16, 32)).leapfrog_depth == 2
    assert on("box3d1r", (16, 16, 33)).leapfrog_depth == 1
    assert on("box3d1r", (16, 16, 32), dtype="bf16").leapfrog_depth == 0
    p = on("star3d1r", (16, 16, 32)).set_source(A)
    assert p.leapfrog_depth == 0
    p.set_source(None)
    assert p.leapfrog_depth == 2
    # without the option a 3D plan keeps depth 1, and the option leaves 1D and 2D plans where they are
    assert L.Plan("box3d1r", (16, 16, 32)).leapfrog_depth == 1
    for shape, dims, depth in [("1d1r", (300,), 1), ("star2d1r", (64, 128), 2), ("star2d1r", (64, 127), 1), ("box2d3r", (64, 128), 2)]:
        assert L.Plan(shape, dims).leapfrog_depth == depth
        assert on(shape, dims).leapfrog_depth == depth, shape
    assert on("box2d3r", (64, 128)).set_variant(_lib.VARIANT_MFMA).leapfrog_depth == 0
    # neither the boundary nor the scratch option moves it
    assert on("star3d1r", (16, 16, 32)).set_boundary("periodic").set_option("scratch", 0).leapfrog_depth == 2
    # switching it off again restores depth 1
    assert on("star3d1r", (16, 16, 32)).set_option("leap3", 0).leapfrog_depth == 1


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=[f"{s}-{'x'.join(map(str, d))}-{t}" for s, d, t in PLANS])
def test_option_moves_nothing_else(L, shape, dims, dtype):
    """kernel name, signature and every other readable option are what they were"""
    p = L.Plan(shape, dims, dtype=dtype)
    before = state(p)
    p.set_option("leap3", 1)
    assert state(p) == before
    for key, value in (("steps_per_launch", 1), ("fused_z_chunk", 8)):
        q, r = L.Plan(shape, dims, dtype=dtype), L.Plan(shape, dims, dtype=dtype).set_option("leap3", 1)
        q.set_option(key, value)
        r.set_option(key, value)
        assert state(q) == state(r), key
    p.set_option("leap3", 0)
    assert state(p) == before and state(p) == state(L.Plan(shape, dims, dtype=dtype))


def test_step2_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    for shape in ("star3d1r", "box3d1r"):
        p = L.Plan(shape, (6, 6, 8))
        h = p._h
        # -- without the option: a 3D plan has no two-step kernel
        assert p.leapfrog_depth == 1
        assert lib.lora_plan_step2_leapfrog(h, A, B, C, D, -1.0, None) == U
        assert "leap3" in lib.lora_last_error().decode()
        assert lib.lora_plan_step2_leapfrog_region(h, A, B, C, D, -1.0, 0, 2, None) == U
        assert lib.lora_plan_step2_leapfrog_src(h, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, None) == U
        assert lib.lora_plan_step2_leapfrog_src_region(h, A, B, None, C, D, 1.0, -1.0, 1.0, -1.0, 0, 2, None) == U
        p.set_option("leap3", 1)
        assert p.leapfrog_depth == 2
        # -- LORA_EINVAL: null pointer, non-finite coefficient, bad range (planes), equal buffers
        bufs = [A, B, C, D]
        for i in range(4):
            args = list(bufs)
            args[i] = None
            assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == E, i
            assert lib.lora_plan_step2_leapfrog_src(h, args[0], args[1], F, args[2], args[3], 1.0, -1.0, 1.0, -1.0, None) == E, i
        for c in (inf, -inf, nan):
            assert lib.lora_plan_step2_leapfrog(h, A, B, C, D, c, None) == E
            for k in range(4):
                co = [1.0, -1.0, 1.0, -1.0]
                co[k] = c
                assert lib.lora_plan_step2_leapfrog_src(h, A, B, F, C, D, *co, None) == E
        for begin, end in ((-1, 4), (0, 7), (5, 4)):
            assert lib.lora_plan_step2_leapfrog_region(h, A, B, C, D, -1.0, begin, end, None) == E
            assert lib.lora_plan_step2_leapfrog_src_region(h, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, begin, end, None) == E
        for i in range(4):
            for j in range(i + 1, 4):
                args = list(bufs)
                args[j] = args[i]
                assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == E, (i, j)
        for i in range(4):
            args = list(bufs)
            assert lib.lora_plan_step2_leapfrog_src(h, args[0], args[1], args[i], args[2], args[3], 1.0, -1.0, 1.0, -1.0, None) == E, i
        # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument with a misaligned buffer
        assert lib.lora_plan_step2_leapfrog(h, A + 8, B, C, D, nan, None) == E
        # -- LORA_EUNSUPPORTED: a misaligned buffer
        for i in range(4):
            args = list(bufs)
            args[i] += 8
            assert lib.lora_plan_step2_leapfrog(h, *args, -1.0, None) == U and "16-byte" in lib.lora_last_error().decode(), i
        assert lib.lora_plan_step2_leapfrog_src(h, A, B, F + 8, C, D, 1.0, -1.0, 1.0, -1.0, None) == U
        # -- LORA_EUNSUPPORTED: the plan lost its kernels
        p.set_source(F)
        assert lib.lora_plan_step2_leapfrog(h, A, B, C, D, -1.0, None) == U
        p.set_source(None)
        # -- nothing to do is no error and needs no device
        assert lib.lora_plan_step2_leapfrog_region(h, A, B, C, D, 0.5, 3, 3, None) == 0
        assert lib.lora_plan_step2_leapfrog_src_region(h, A, B, F, C, D, 1.0, -1.0, 1.0, -1.0, 3, 3, None) == 0
        assert lib.lora_plan_run_leapfrog(h, A, B, -1.0, 0, None) == 0
        assert lib.lora_plan_prepare_leapfrog(h, 0) == 0
    # an odd innermost extent keeps depth 1 with the option on
    odd = L.Plan("box3d1r", (6, 6, 7)).set_option("leap3", 1)
    assert lib.lora_plan_step2_leapfrog(odd._h, A, B, C, D, -1.0, None) == U


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_two_step_launch_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape in ("star3d1r", "box3d1r"):
        for bc in ("reference", "dirichlet", "periodic"):
            p = L.Plan(shape, (6, 6, 8)).set_boundary(bc).set_option("leap3", 1)
            calls = [lambda: p.step2_leapfrog(A, B, C, D), lambda: p.step2_leapfrog_region(A, B, C, D, 0.7, 1, 3),
                     lambda: p.step2_leapfrog_src(A, B, F, C, D, 1.2, -0.2, 1.1, -0.1),
                     lambda: p.step2_leapfrog_src_region(A, B, None, C, D, 1.2, -0.2, 1.1, -0.1, 0, 6),
                     lambda: p.run_leapfrog(A, B, -1.0, 9), lambda: p.run_leapfrog_src(A, B, F, 1.0, -1.0, 9)]
            for i, call in enumerate(calls):
                with pytest.raises(L.LoraError) as e:
                    call()
                assert e.value.status == _lib.LORA_ENODEVICE, (shape, bc, i)
            p.prepare_leapfrog(9)  # allocates nothing here, and says so by staying quiet


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_leap3_parse(engine_built):
    rc, out, err = cli(3, "star3d1r", "8", "8", "8", "4", "--leap3")
    assert rc == 1 and out == "" and err.startswith("--leap3 ") and err.count("\n") == 1
    for dim, args in ((2, ["star2d1r", "64", "64", "4"]), (1, ["1d1r", "64", "4"])):
        rc, out, err = cli(dim, *args, "--leapfrog", "--leap3")
        assert rc == 1 and out == "" and err == "Unknown option: --leap3\n", dim
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--leapfrog", "--leap3")
    assert rc == 1 and err.startswith("--leapfrog runs on one GPU in fp64") and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_leap3_reaches_the_operator(engine_built):
    for extra in (["--leapfrog"], ["--leapfrog=-0.5", "--bc=dirichlet"], ["--chebyshev=0.9"]):
        rc, out, _ = cli(3, "star3d1r", "8", "8", "8", "8", *extra, "--leap3")
        assert out.startswith("INFO: shape = ")
        assert rc == 1 and "no HIP device" in out
