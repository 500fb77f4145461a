"""CPU tests of the variable-coefficient wave entries' boundary (lora_plan_wave_depth ... lora_run_host_wave; include/lorastencil.h,
DESIGN 3.18): the symbols, the status codes in their documented order on addresses nobody dereferences, which plans have which
wave depth, that no wave call changes what a plan resolves to, the loud failure without a device, the CLI's --wave flag, and the
compiler's own resource report of every EPI_WAVE instantiation against the EPI_LEAP_SRC one of the same family and tap set.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT, has_gpu

A = 4096  # 16-byte aligned addresses nobody dereferences
B, C, D, K = A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (4 << 20)
BIN = os.path.join(ROOT, "lorastencil_amd", "bin")
CSRC = os.path.join(ROOT, "lorastencil_amd", "csrc")

ENTRIES = ["lora_plan_wave_depth", "lora_plan_step_wave", "lora_plan_step_wave_region", "lora_plan_step2_wave",
           "lora_plan_step2_wave_region", "lora_plan_run_wave", "lora_plan_prepare_wave", "lora_run_host_wave"]

# every key lora_plan_get_option answers in the shipped library (the list of tests/test_leapfrog_host.py, and leap3)
KEYS = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "stream", "stream_rows", "wg", "wg_rows", "wg_prio",
        "wg_edge_pct", "stream_depth", "stream3", "lanes3", "stream3_waves", "stream3_async", "stream3_pipe", "stream3_slots",
        "stream_share", "stream_prefetch", "stream_sync", "scratch", "mfma_split", "graph", "lowrank_valu", "separable", "lds_dma",
        "cols_per_lane", "fused_rows", "steps_per_launch", "fused_pipeline", "fused_z_chunk", "spans3", "torus", "tapset", "variant",
        "fused_eval", "boundary", "fused_residual", "source", "leap3"]


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def state(p):
    return {k: p.get_option(k) for k in KEYS}, p.kernel_name, p.kernel_signature, p.leapfrog_depth


def test_symbols_are_exported_and_mirrored(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lorastencil.h")).read()
    for name in ENTRIES:
        assert getattr(lib, name) and name in _lib.SIGNATURES, name
        assert f"int {name}(" in header, name
    assert "int lora_plan_step_wave(lora_plan *plan, const void *d_cur, void *d_prev, const void *d_k, double b, double c, void *stream);" in header
    assert "int lora_plan_run_wave(lora_plan *plan, void *d_prev, void *d_cur, const void *d_k, double b, double c, int times, void *stream);" in header
    for name in ("step_wave", "step_wave_region", "step2_wave", "step2_wave_region", "run_wave", "prepare_wave"):
        assert callable(getattr(L.Plan, name)), name
    assert isinstance(L.Plan.wave_depth, property) and callable(L.run_host_wave) and L.ops.run_host_wave is L.run_host_wave


def test_depth_table(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    assert lib.lora_plan_wave_depth(None) == 0
    table = [("1d1r", (300,), 1), ("1d2r", (301,), 1), ("star2d1r", (64, 128), 2), ("star2d1r", (64, 127), 1), ("star2d3r", (64, 128), 2),
             ("star2d3r", (64, 127), 1), ("box2d1r", (64, 128), 2), ("box2d3r", (64, 128), 2), ("box2d3r", (64, 127), 1),
             ("star3d1r", (16, 16, 32), 1), ("star3d1r", (16, 16, 31), 1), ("box3d1r", (16, 16, 32), 1), ("box3d1r", (16, 16, 31), 1)]
    for shape, dims, depth in table:
        p = L.Plan(shape, dims)
        assert p.wave_depth == depth, (shape, dims)
        p.set_source(A)  # a plan that carries a source has no wave kernel
        assert p.wave_depth == 0, (shape, dims)
        p.set_source(None)
        assert p.wave_depth == depth, (shape, dims)
    box = L.Plan("box2d3r", (64, 128))
    box.set_variant(_lib.VARIANT_MFMA)
    assert box.get_option("variant") == _lib.VARIANT_MFMA and box.wave_depth == 0
    assert L.Plan("box3d1r", (16, 16, 32), dtype="bf16").wave_depth == 0
    # there is no two-step wave launch in 3D: option leap3 moves the leapfrog depth alone
    for shape in ("box3d1r", "star3d1r"):
        p3 = L.Plan(shape, (16, 16, 32)).set_option("leap3", 1)
        assert p3.get_option("leap3") == 1 and p3.leapfrog_depth == 2 and p3.wave_depth == 1
    # neither the boundary nor the scratch option moves it: they choose the run's schedule, not the kernels a plan has
    assert L.Plan("star2d1r", (64, 128)).set_boundary("periodic").set_option("scratch", 0).wave_depth == 2


def test_status_codes_in_order(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    inf, nan = float("inf"), float("nan")
    p = L.Plan("star2d1r", (32, 64))
    h = p._h
    # -- LORA_EINVAL: null plan / pointer (d_k is mandatory), non-finite b or c, bad range, times < 0, equal buffers
    assert lib.lora_plan_step_wave(None, A, B, K, 2.0, -1.0, None) == E
    assert lib.lora_plan_step_wave_region(None, A, B, K, 2.0, -1.0, 0, 1, None) == E
    assert lib.lora_plan_step2_wave(None, A, B, K, C, D, 2.0, -1.0, None) == E
    assert lib.lora_plan_step2_wave_region(None, A, B, K, C, D, 2.0, -1.0, 0, 1, None) == E
    assert lib.lora_plan_run_wave(None, A, B, K, 2.0, -1.0, 1, None) == E
    assert lib.lora_plan_prepare_wave(None, 1) == E
    for cur, prev, k in ((None, B, K), (A, None, K), (A, B, None), (A, A, K), (A, B, A), (A, B, B)):
        assert lib.lora_plan_step_wave(h, cur, prev, k, 2.0, -1.0, None) == E, (cur, prev, k)
        assert lib.lora_plan_step_wave_region(h, cur, prev, k, 2.0, -1.0, 0, 32, None) == E, (cur, prev, k)
        assert lib.lora_plan_run_wave(h, prev, cur, k, 2.0, -1.0, 3, None) == E, (cur, prev, k)
    for x in (inf, -inf, nan):
        for b, c in ((x, -1.0), (2.0, x)):
            assert lib.lora_plan_step_wave(h, A, B, K, b, c, None) == E
            assert lib.lora_plan_step2_wave(h, A, B, K, C, D, b, c, None) == E
            assert lib.lora_plan_run_wave(h, A, B, K, b, c, 3, None) == E
    for begin, end in ((-1, 4), (0, 33), (5, 4)):
        assert lib.lora_plan_step_wave_region(h, A, B, K, 2.0, -1.0, begin, end, None) == E
        assert lib.lora_plan_step2_wave_region(h, A, B, K, C, D, 2.0, -1.0, begin, end, None) == E
    p1 = L.Plan("1d1r", (300,))
    assert p1.region_granularity == 2
    assert lib.lora_plan_step_wave_region(p1._h, A, B, K, 2.0, -1.0, 3, 10, None) == E
    assert lib.lora_plan_run_wave(h, A, B, K, 2.0, -1.0, -1, None) == E
    assert lib.lora_plan_prepare_wave(h, -1) == E
    bufs = [A, B, K, C, D]  # prev, cur, k, out1, out2
    for i in range(5):
        for j in range(i + 1, 5):
            args = list(bufs)
            args[j] = args[i]
            assert lib.lora_plan_step2_wave(h, *args, 2.0, -1.0, None) == E, (i, j)
    for i in range(5):
        args = list(bufs)
        args[i] = None
        assert lib.lora_plan_step2_wave(h, *args, 2.0, -1.0, None) == E, i
    # -- LORA_EINVAL comes before LORA_EUNSUPPORTED: a bad argument on a plan without the kernels, with a misaligned buffer
    bf = L.Plan("box3d1r", (4, 6, 8), dtype="bf16")
    assert lib.lora_plan_step_wave(bf._h, A + 8, A + 8, K, 2.0, -1.0, None) == E
    assert lib.lora_plan_step_wave(bf._h, A, B, K, nan, -1.0, None) == E
    assert lib.lora_plan_run_wave(bf._h, A, B, K, 2.0, -1.0, -1, None) == E
    # -- LORA_EUNSUPPORTED: a misaligned buffer
    for cur, prev, k in ((A + 8, B, K), (A, B + 8, K), (A, B, K + 8)):
        assert lib.lora_plan_step_wave(h, cur, prev, k, 2.0, -1.0, None) == U and "16-byte" in lib.lora_last_error().decode()
        assert lib.lora_plan_run_wave(h, prev, cur, k, 2.0, -1.0, 2, None) == U
    for i in range(5):
        args = list(bufs)
        args[i] += 8
        assert lib.lora_plan_step2_wave(h, *args, 2.0, -1.0, None) == U, i
    # -- LORA_EUNSUPPORTED: the plans without the kernels
    mfma = L.Plan("box2d3r", (32, 64)).set_variant(_lib.VARIANT_MFMA)
    src = L.Plan("star2d1r", (32, 64)).set_source(D)
    for q in (bf, mfma, src):
        n = q.dims[0]
        assert q.wave_depth == 0
        assert lib.lora_plan_step_wave(q._h, A, B, K, 2.0, -1.0, None) == U
        assert lib.lora_plan_step_wave_region(q._h, A, B, K, 2.0, -1.0, 0, n, None) == U
        assert lib.lora_plan_run_wave(q._h, A, B, K, 2.0, -1.0, 4, None) == U
        assert lib.lora_plan_run_wave(q._h, A, B, K, 2.0, -1.0, 0, None) == U
        assert lib.lora_plan_prepare_wave(q._h, 4) == U
        assert lib.lora_plan_step2_wave(q._h, A, B, K, C, D, 2.0, -1.0, None) == U
    # -- the two-step entries on plans of wave depth 1, a 3D plan with leap3 among them
    for shape, dims, leap3 in [("1d1r", (300,), 0), ("star2d1r", (32, 63), 0), ("box3d1r", (4, 6, 8), 0), ("box3d1r", (4, 6, 8), 1)]:
        q = L.Plan(shape, dims)
        if leap3:
            q.set_option("leap3", 1)
        assert q.wave_depth == 1
        assert lib.lora_plan_step2_wave(q._h, A, B, K, C, D, 2.0, -1.0, None) == U, shape
        assert "two wave steps" in lib.lora_last_error().decode()
        assert lib.lora_plan_step2_wave_region(q._h, A, B, K, C, D, 2.0, -1.0, 0, 2, None) == U, shape
    # -- nothing to do is no error and needs no device
    assert lib.lora_plan_run_wave(h, A, B, K, 2.0, -1.0, 0, None) == 0
    assert lib.lora_plan_step_wave_region(h, A, B, K, 2.0, -1.0, 7, 7, None) == 0
    assert lib.lora_plan_step2_wave_region(h, A, B, K, C, D, 0.5, 0.25, 7, 7, None) == 0


def test_host_entry_status_codes(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    E, U = _lib.LORA_EINVAL, _lib.LORA_EUNSUPPORTED
    a = np.zeros(L.padded_shape("star2d1r", (8, 16)))
    out = np.zeros_like(a)
    dims, sid = L.ops._dims_arg((8, 16)), L.ops.shape_id("star2d1r")
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    run = lib.lora_run_host_wave
    assert run(sid, None, dp(a), dp(a), dp(out), None, 2.0, -1.0, 1, 1, dims, 1, None) == E
    assert run(sid, dp(a), None, dp(a), dp(out), None, 2.0, -1.0, 1, 1, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), None, dp(out), None, 2.0, -1.0, 1, 1, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(a), None, None, 2.0, -1.0, 1, 1, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(a), dp(out), None, 2.0, -1.0, 1, 1, None, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(a), dp(out), None, 2.0, -1.0, 1, -1, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(a), dp(out), None, float("nan"), -1.0, 1, 1, dims, 1, None) == E
    assert run(sid, dp(a), dp(a), dp(a), dp(out), None, 2.0, float("inf"), 1, 1, dims, 1, None) == E
    assert L.set_default_source(a) is None
    try:
        assert run(sid, dp(a), dp(a), dp(a), dp(out), None, 2.0, -1.0, 1, 1, dims, 1, None) == U
        assert "source" in lib.lora_last_error().decode()
    finally:
        assert L.set_default_source(None) is a
    with pytest.raises(ValueError):
        L.run_host_wave("star2d1r", a, a, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        L.run_host_wave("star2d1r", a, np.zeros((3, 3)), a)


@pytest.mark.parametrize("shape,dims,leap3", [("1d2r", (300,), 0), ("star2d1r", (64, 128), 0), ("box2d3r", (64, 127), 0),
                                              ("box3d1r", (16, 16, 32), 0), ("box3d1r", (16, 16, 32), 1)],
                         ids=["1d", "2d", "2d-odd", "3d", "3d-leap3"])
def test_wave_calls_leave_the_plan_as_it_was(L, shape, dims, leap3):
    """k, b, c and the buffers are call arguments: every key's value, the kernel name, the signature and the leapfrog depth stay"""
    from lorastencil_amd import _lib

    lib = _lib.lib()
    fresh = lambda: L.Plan(shape, dims).set_option("leap3", leap3) if leap3 else L.Plan(shape, dims)  # noqa: E731
    p = fresh()
    before = state(p)
    n = dims[0]
    if not has_gpu():  # (with a device these would launch on addresses nobody owns; tests/test_gpu_wave.py covers them there)
        lib.lora_plan_step_wave(p._h, A, B, K, 2.0, -1.0, None)
        lib.lora_plan_step_wave_region(p._h, A, B, K, 0.7, 0.3, 0, n, None)
        lib.lora_plan_step2_wave(p._h, A, B, K, C, D, 2.0, -1.0, None)
        lib.lora_plan_step2_wave_region(p._h, A, B, K, C, D, 0.7, 0.3, 0, n, None)
        lib.lora_plan_run_wave(p._h, A, B, K, 1.9, -0.9, 9, None)
    assert lib.lora_plan_step_wave_region(p._h, A, B, K, 0.7, 0.3, 2, 2, None) == 0
    assert lib.lora_plan_run_wave(p._h, A, B, K, 1.9, -0.9, 0, None) == 0
    assert lib.lora_plan_prepare_wave(p._h, 9) == 0
    assert p.wave_depth == (2 if len(dims) == 2 and dims[1] % 2 == 0 else 1)
    assert state(p) == before
    assert state(p) == state(fresh())


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_wave_fails_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    for shape, dims in [("1d1r", (300,)), ("star2d1r", (32, 64)), ("star2d1r", (32, 63)), ("box3d1r", (4, 6, 8)), ("star3d1r", (3, 5, 7))]:
        for bc in ("reference", "periodic"):
            p = L.Plan(shape, dims).set_boundary(bc)
            calls = [lambda: p.step_wave(A, B, K), lambda: p.step_wave_region(A, B, K, 0.7, 0.3, 0, 2), lambda: p.run_wave(A, B, K, 2.0, -1.0, 1),
                     lambda: p.run_wave(A, B, K, 2.0, -1.0, 9)]
            if p.wave_depth == 2:
                calls.append(lambda: p.step2_wave(A, B, K, C, D))
            for i, call in enumerate(calls):
                with pytest.raises(L.LoraError) as e:
                    call()
                assert e.value.status == _lib.LORA_ENODEVICE, (shape, bc, i)
            p.prepare_wave(9)  # allocates nothing here, and says so by staying quiet
    a = np.zeros(L.padded_shape("star2d1r", (32, 64)))
    with pytest.raises(L.LoraError) as e:
        L.run_host_wave("star2d1r", a, a, a, times=1)
    assert e.value.status == _lib.LORA_ENODEVICE


def cli(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_wave_parse_errors_and_refusals(engine_built):
    need = "Invalid argument: --wave=K0[,K1] needs one or two finite numbers.\n"
    for bad in ("--wave=", "--wave=abc", "--wave=1x", "--wave=inf", "--wave=nan", "--wave=-1e999", "--wave=0.1,", "--wave=,0.1",
                "--wave=0.1,nan", "--wave=0.1,0.2,0.3", "--wave=0.1,0.2x"):
        rc, out, err = cli(2, "star2d1r", "64", "64", "4", bad)
        assert rc == 1 and err == need and out == "", bad
    rc, out, err = cli(2, "star2d1r", "64", "64", "4", "--wave")
    assert rc == 1 and err == "Unknown option: --wave\n" and out == ""
    refused = "--wave runs on one GPU in fp64"
    for extra in (["--gpus=2"], ["--gpus=1"], ["--grid=1x2"], ["--check"], ["--until=1e-9"], ["--source=const:1"], ["--leapfrog"],
                  ["--leapfrog=-0.5"], ["--chebyshev=0.5"], ["--cg"], ["--cg", "--until=1e-9"], ["--mg"], ["--mg", "--until=1e-9"], ["--pcg"],
                  ["--implicit=0.5"]):
        for flag in ("--wave=0.1", "--wave=0.1,0.2"):
            for args in ([flag, *extra], [*extra, flag]):
                rc, out, err = cli(2, "star2d1r", "64", "64", "4", *args)
                assert rc == 1 and err.startswith(refused) and err.count("\n") == 1 and out == "", args
    rc, out, err = cli(3, "box3d1r", "8", "8", "8", "4", "--dtype=bf16", "--wave=0.1")
    assert rc == 1 and err.startswith(refused) and out == ""
    rc, out, err = cli(1, "1d1r", "64", "4", "--source=point:2", "--wave=0.25,0.5")
    assert rc == 1 and err.startswith(refused) and out == ""


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_cli_wave_reaches_the_operator(engine_built):
    for dim, args in ((2, ["star2d1r", "64", "128", "7", "--wave=0.1,0.2"]), (1, ["1d1r", "64", "3", "--wave=0.25"]),
                      (3, ["box3d1r", "8", "8", "8", "2", "--wave=0.05,0.1", "--bc=periodic"])):
        rc, out, _ = cli(dim, *args)
        assert out.startswith("INFO: shape = ")
        assert rc == 1 and "no HIP device" in out


# ---- the compiler's report (read as tests/test_step2_resources.py reads it) ---------------------------------------------------------
EPI_LEAP_SRC, EPI_WAVE = 3, 4
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


def test_wave_instantiations_have_no_scratch_and_the_waves_of_the_source_rule():
    """every EPI_WAVE instantiation of kernels_step.hip (five families) and kernels_2d_wave2.hip (three tap sets): no scratch, and
    at least the waves per SIMD of the EPI_LEAP_SRC instantiation of the same family and tap set -- an existing kernel with the same
    operand count, read from the same compiler in this test, so no number is fixed in advance"""
    step = resource_report("kernels_step.hip")
    wave2 = resource_report("kernels_2d_wave2.hip")
    step2 = resource_report("kernels_2d_step2.hip")
    # kernels_2d_wave2.hip holds the wave rule of the three tap sets and nothing else
    assert sorted(wave2) == sorted(("stencil2d_step2_kernel", (t, 6 if t == 1 else 10, EPI_WAVE)) for t in range(3))
    want_step = ([("stencil1d_step_kernel", ()), ("stencil2d_generic_step_kernel", ()), ("stencil3d_generic_step_kernel", ())]
                 + [("stencil2d_step_kernel", (t,)) for t in range(3)] + [("stencil3d_step_kernel", (t,)) for t in range(2)])
    pairs = []
    for family, head in want_step:
        pairs.append((step[family, head + (EPI_WAVE,)], step[family, head + (EPI_LEAP_SRC,)], (family, head)))
    for (family, args), got in wave2.items():
        pairs.append((got, step2[family, args[:-1] + (EPI_LEAP_SRC,)], (family, args[:-1])))
    assert len(pairs) == 11
    for got, base, which in pairs:
        print(which, "wave", got, "leap_src", base)
        assert got["scratch"] == 0, (which, got)
        assert got["waves"] >= base["waves"], (which, got, base)
