"""CPU tests of plan option "wave3" (3D fp64: two wave steps per launch; include/lorastencil.h): the option and its
thread default, which plans read which wave depth with it, that it moves nothing else a plan resolves to, the status codes of
lora_plan_step2_wave_region on a 3D plan in their documented order on addresses nobody dereferences, the CLI's --wave3 flag, and
the compiler's own resource report of every instantiation of kernels_3d_step2.hip.
"""
import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C, D, K = A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (4 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")
CSRC = os.path.join(ROOT, "lorastencil_amd", "csrc")

# every key lora_plan_get_option answered before the option existed (the list of tests/test_wave_host.py)
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "spans3", "torus", "tapset", "variant",
        "fused_eval", "boundary", "fused_residual", "source", "leap3"]

PLANS = [("1d1r", (300,), "f64"), ("1d2r", (301,), "f64"), ("star2d1r", (64, 128), "f64"), ("box2d3r", (64, 127), "f64"),
         ("star3d1r", (16, 16, 32), "f64"), ("box3d1r", (16, 16, 32), "f64"), ("box3d1r", (16, 16, 31), "f64"),
         ("box3d1r", (16, 16, 32), "bf16")]
PLAN_IDS = [f"{s}-{'x'.join(map(str, d))}-{t}" for s, d, t in PLANS]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature, p.leapfrog_depth


def test_symbol_and_mirrors(L):
    from lorastencil_amd import _lib

    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    assert "int lora_set_default_wave3(int on);" in header and '"wave3"' in header
    assert getattr(_lib.lib(), "lora_set_default_wave3") and "lora_set_default_wave3" in _lib.SIGNATURES
    assert callable(L.set_default_wave3) and L.ops.set_default_wave3 is L.set_default_wave3


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=PLAN_IDS)
def test_option_round_trips_on_every_plan(L, shape, dims, dtype):
    p = L.Plan(shape, dims, dtype=dtype)
    assert p.get_option("wave3") == 0
    for value, reads in ((1, 1), (0, 0), (7, 1), (-3, 1), (0, 0)):
        p.set_option("wave3", value)
        assert p.get_option("wave3") == reads, value


def test_thread_default_reaches_new_plans(L):
    assert L.set_default_wave3(0) == 0
    try:
        assert L.set_default_wave3(1) == 0
        assert L.set_default_wave3(5) == 1  # any non-zero value is 1
        for shape, dims, dtype in PLANS:
            q = L.Plan(shape, dims, dtype=dtype)
            assert q.get_option("wave3") == 1 and q.get_option("leap3") == 0, shape
        p = L.Plan("star3d1r", (16, 16, 32))
        assert p.wave_depth == 2 and p.leapfrog_depth == 1
        assert L.set_default_wave3(0) == 1
        assert p.get_option("wave3") == 1 and p.wave_depth == 2  # a plan keeps what it was created with
        assert L.Plan("star3d1r", (16, 16, 32)).get_option("wave3") == 0
        assert L.Plan("star3d1r", (16, 16, 32)).wave_depth == 1
    finally:
        L.set_default_wave3(0)


def test_depth_table(L):
    from lorastencil_amd import _lib

    on = lambda shape, dims, **kw: L.Plan(shape, dims, **kw).set_option("wave3", 1)  # noqa: E731
    assert on("star3d1r", (16, 16, 32)).wave_depth == 2
    assert on("box3d1r", (16, 16, 32)).wave_depth == 2
    assert on("star3d1r", (16, 16, 31)).wave_depth == 1
    assert on("box3d1r", (16, 16, 31)).wave_depth == 1
    assert on("box3d1r", (16, 16, 32), dtype="bf16").wave_depth == 0
    p = on("star3d1r", (16, 16, 32)).set_source(A)
    assert p.wave_depth == 0
    p.set_source(None)
    assert p.wave_depth == 2
    # without the option a 3D plan keeps depth 1, with leap3 too; the options are independent
    assert L.Plan("box3d1r", (16, 16, 32)).wave_depth == 1
    for shape in ("star3d1r", "box3d1r"):
        q = L.Plan(shape, (16, 16, 32)).set_option("leap3", 1)
        assert (q.get_option("wave3"), q.leapfrog_depth, q.wave_depth) == (0, 2, 1)
        q.set_option("wave3", 1)
        assert (q.get_option("leap3"), q.leapfrog_depth, q.wave_depth) == (1, 2, 2)
        q.set_option("leap3", 0)
        assert (q.get_option("wave3"), q.leapfrog_depth, q.wave_depth) == (1, 1, 2)
    # 1D and 2D plans read what they read without it
    for shape, dims, depth in [("1d1r", (300,), 1), ("1d2r", (301,), 1), ("star2d1r", (64, 128), 2), ("star2d1r", (64, 127), 1),
                               ("box2d3r", (64, 128), 2), ("box2d3r", (64, 127), 1)]:
        assert L.Plan(shape, dims).wave_depth == depth
        assert on(shape, dims).wave_depth == depth, shape
    assert on("box2d3r", (64, 128)).set_variant(_lib.VARIANT_MFMA).wave_depth == 0
    # neither the boundary nor the scratch option moves it
    assert on("star3d1r", (16, 16, 32)).set_boundary("periodic").set_option("scratch", 0).wave_depth == 2
    # switching it off again restores depth 1
    assert on("star3d1r", (16, 16, 32)).set_option("wave3", 0).wave_depth == 1


@pytest.mark.parametrize("shape,dims,dtype", PLANS, ids=PLAN_IDS)
def test_option_moves_nothing_else(L, shape, dims, dtype):
    """kernel name, signature, leapfrog depth and every other readable option are what they were"""
    p = L.Plan(shape, dims, dtype=dtype)
    before = state(p)
    p.set_option("wave3", 1)
    assert state(p) == before
    for key, value in (("steps_per_launch", 1), ("fused_z_chunk", 8), ("leap3", 1)):
        q, r = L.Plan(shape, dims, dtype=dtype), L.Plan(shape, dims, dtype=dtype).set_option("wave3", 1)
        q.set_option(key, value)
        r.set_option(key, value)
        assert state(q) == state(r), key
    p.set_option("wave3", 0)
    assert state(p) == before and state(p) == state(L.Plan(shape, dims, dtype=dtype))


def test_step2_wave_region_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    bufs = [A, B, K, C, D]  # prev, cur, k, out1, out2
    for shape in ("star3d1r", "box3d1r"):
        p = L.Plan(shape, (6, 6, 8))
        h = p._h
        # -- without the option a 3D plan has no two-step wave kernel, with leap3 neither
        for leap3 in (0, 1):
            p.set_option("leap3", leap3)
            assert p.wave_depth == 1
            assert lib.lora_plan_step2_wave_region(h, *bufs, 2.0, -1.0, 0, 2, None) == U
            assert "wave3" in lib.lora_last_error().decode()
            assert lib.lora_plan_step2_wave(h, *bufs, 2.0, -1.0, None) == U
        p.set_option("leap3", 0).set_option("wave3", 1)
        assert p.wave_depth == 2
        # -- LORA_EINVAL: null plan / pointer, non-finite b or c, bad range (planes), equal buffers (d_k among them)
        assert lib.lora_plan_step2_wave_region(None, *bufs, 2.0, -1.0, 0, 2, None) == E
        for i in range(5):
            args = list(bufs)
            args[i] = None
            assert lib.lora_plan_step2_wave_region(h, *args, 2.0, -1.0, 0, 6, None) == E, i
            assert lib.lora_plan_step2_wave(h, *args, 2.0, -1.0, None) == E, i
        for x in (inf, -inf, nan):
            for b, c in ((x, -1.0), (2.0, x)):
                assert lib.lora_plan_step2_wave_region(h, *bufs, b, c, 0, 6, None) == E
        for begin, end in ((-1, 4), (0, 7), (5, 4)):
            assert lib.lora_plan_step2_wave_region(h, *bufs, 2.0, -1.0, begin, end, None) == E
        for i in range(5):
            for j in range(i + 1, 5):
                args = list(bufs)
                args[j] = args[i]
                assert lib.lora_plan_step2_wave_region(h, *args, 2.0, -1.0, 0, 6, None) == E, (i, j)
        # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument with a misaligned buffer
        assert lib.lora_plan_step2_wave_region(h, A + 8, B, K, C, D, nan, -1.0, 0, 6, None) == E
        assert lib.lora_plan_step2_wave_region(h, A + 8, B, K, C, D, 2.0, -1.0, 0, 7, None) == E
        # -- LORA_EUNSUPPORTED: a misaligned buffer
        for i in range(5):
            args = list(bufs)
            args[i] += 8
            assert lib.lora_plan_step2_wave_region(h, *args, 2.0, -1.0, 0, 6, None) == U, i
            assert "16-byte" in lib.lora_last_error().decode(), i
        # -- LORA_EUNSUPPORTED: the plan lost its kernels
        p.set_source(K)
        assert lib.lora_plan_step2_wave_region(h, *bufs, 2.0, -1.0, 0, 6, None) == U
        p.set_source(None)
        # -- nothing to do is no error and needs no device
        assert lib.lora_plan_step2_wave_region(h, *bufs, 0.5, 0.25, 3, 3, None) == 0
        assert lib.lora_plan_run_wave(h, A, B, K, 2.0, -1.0, 0, None) == 0
        assert lib.lora_plan_prepare_wave(h, 0) == 0
        # -- LORA_ENODEVICE from the launch
        if not has_gpu():
            assert lib.lora_plan_step2_wave_region(h, *bufs, 2.0, -1.0, 0, 6, None) == _lib.LORA_ENODEVICE
            assert lib.lora_plan_step2_wave_region(h, *bufs, 0.7, 0.3, 1, 3, None) == _lib.LORA_ENODEVICE
    # an odd innermost extent keeps depth 1 with the option on
    odd = L.Plan("box3d1r", (6, 6, 7)).set_option("wave3", 1)
    assert odd.wave_depth == 1
    assert lib.lora_plan_step2_wave_region(odd._h, *bufs, 2.0, -1.0, 0, 6, None) == U
    assert "two wave steps" in lib.lora_last_error().decode()


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_two_step_launch_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape in ("star3d1r", "box3d1r"):
        for bc in ("reference", "dirichlet", "periodic"):
            p = L.Plan(shape, (6, 6, 8)).set_boundary(bc).set_option("wave3", 1)
            calls = [lambda: p.step2_wave(A, B, K, C, D), lambda: p.step2_wave_region(A, B, K, C, D, 0.7, 0.3, 1, 3),
                     lambda: p.run_wave(A, B, K, 2.0, -1.0, 9), lambda: p.step_wave(A, B, K)]
            for i, call in enumerate(calls):
                with pytest.raises(L.LoraError) as e:
                    call()
                assert e.value.status == _lib.LORA_ENODEVICE, (shape, bc, i)
            p.prepare_wave(9)  # allocates nothing here, and says so by staying quiet


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_wave3_parse(engine_built):
    for extra in ([], ["--leapfrog"], ["--leapfrog", "--leap3"]):
        rc, out, err = cli(3, "star3d1r", "8", "8", "8", "4", *extra, "--wave3")
        assert rc == 1 and out == "" and err.startswith("--wave3 ") and err.count("\n") == 1, extra
    for dim, args in ((2, ["star2d1r", "64", "64", "4"]), (1, ["1d1r", "64", "4"])):
        for extra in ([], ["--wave=0.1,0.2"]):
            rc, out, err = cli(dim, *args, *extra, "--wave3")
            assert rc == 1 and out == "" and err == "Unknown option: --wave3\n", (dim, extra)
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--wave=0.1", "--wave3")
    assert rc == 1 and err.startswith("--wave runs on one GPU in fp64") and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_wave3_reaches_the_operator(engine_built):
    for extra in (["--wave=0.1,0.2"], ["--wave=0.05", "--bc=dirichlet"]):
        rc, out, _ = cli(3, "star3d1r", "8", "8", "8", "8", *extra, "--wave3")
        assert out.startswith("INFO: shape = ")
        assert rc == 1 and "no HIP device" in out


# ---- the compiler's report (read as tests/test_wave_host.py reads it) -----------------------------------------------------------
EPI_LEAP, EPI_LEAP_SCALED, EPI_LEAP_SRC, EPI_WAVE = 1, 2, 3, 4
FIELDS = (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)"))


def resource_report(unit):
    """{(kernel family, template arguments): {scratch, waves, vgprs}} of every kernel of one translation unit"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
                        "-c", unit, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?\d+(stencil\w+_kernel)I((?:Li\d+E)+)E", line)
        if m:
            name = (m.group(1), tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(2))))
            seen[name] = {}
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def test_instantiations_have_no_scratch_and_their_workgroups_per_cu():
    """kernels_3d_step2.hip holds eight kernels: a workgroup is four waves, one per SIMD, so waves per SIMD are workgroups per CU.
    The six leapfrog instantiations: no scratch and three; the two EPI_WAVE ones: no scratch and at least two"""
    got = resource_report("kernels_3d_step2.hip")
    for k, v in sorted(got.items()):
        print(k, v)
    want = [("stencil3d_step2_kernel", (t, e)) for t in (0, 1) for e in (EPI_LEAP, EPI_LEAP_SCALED, EPI_LEAP_SRC, EPI_WAVE)]
    assert sorted(got) == sorted(want)
    for (family, (taps, epi)), r in got.items():
        assert r["scratch"] == 0, (taps, epi, r)
        if epi == EPI_WAVE:
            assert r["waves"] >= 2, (taps, r)
        else:
            assert r["waves"] == 3, (taps, epi, r)
