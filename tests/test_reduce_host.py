"""CPU tests of the reductions' boundary (include/lorastencil.h: lora_plan_stats, lora_plan_diff, lora_grid_stats_merge,
lora_plan_run_until, lora_run_host_until, the CLIs' --until): the host-only merge against numpy, argument validation, the
loud failure without a device, the ctypes mirror of the structs against a C compiler, the new flags' messages."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT, has_gpu

BIN = os.path.join(ROOT, "lorastencil_amd", "bin")
A, B = 4096, 8192  # 16-byte aligned addresses nobody dereferences: every call below is refused before a launch


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def np_stats(L, x):
    """What lora_plan_stats defines, by numpy, for the cells `x` of a region."""
    x = np.asarray(x, dtype=np.float64).ravel()
    f = x[np.isfinite(x)]
    if f.size == 0:
        return L.GridStats(math.inf, -math.inf, 0.0, 0.0, 0.0, x.size, x.size)
    return L.GridStats(f.min(), f.max(), np.abs(f).max(), f.sum(), (f * f).sum(), x.size, x.size - f.size)


def test_stats_merge_matches_numpy_on_split_arrays(L):
    x = np.random.default_rng(3).integers(-50, 50, 1000).astype(np.float64)  # integer data: sums exact in any order
    x[17], x[400], x[999] = np.nan, np.inf, -np.inf
    for cuts in [(0, 1000), (1, 999), (250, 250), (333, 334), (0, 0)]:  # two of them give an empty part
        parts = [x[:cuts[0]], x[cuts[0]:cuts[1]], x[cuts[1]:]]
        got = L.stats_merge(*[np_stats(L, p) for p in parts])
        assert got == np_stats(L, x), cuts
    # a part without a finite cell changes the counts only
    bad = np.array([np.nan, np.inf, np.nan])
    got = L.stats_merge(np_stats(L, x[:500]), np_stats(L, bad), np_stats(L, x[500:]))
    want = np_stats(L, np.concatenate([x[:500], bad, x[500:]]))
    assert got == want and got.nonfinite == 6
    # nothing merged, and only empty records merged: the empty record
    assert L.stats_merge() == L.EMPTY_STATS == L.stats_merge(L.EMPTY_STATS, np_stats(L, []))
    assert L.stats_merge(np_stats(L, bad)) == L.GridStats(math.inf, -math.inf, 0.0, 0.0, 0.0, 3, 3)


def test_null_pointers_and_bad_ranges_are_einval(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p = L.Plan("star2d1r", (32, 64))
    st, df = _lib.GridStats(), _lib.GridDiff()
    E = _lib.LORA_EINVAL
    assert lib.lora_plan_stats(None, A, 0, 0, ctypes.byref(st), None) == E
    assert lib.lora_plan_stats(p._h, None, 0, 0, ctypes.byref(st), None) == E
    assert lib.lora_plan_stats(p._h, A, 0, 0, None, None) == E
    assert lib.lora_plan_diff(None, A, B, 0, 0, ctypes.byref(df), None) == E
    assert lib.lora_plan_diff(p._h, None, B, 0, 0, ctypes.byref(df), None) == E
    assert lib.lora_plan_diff(p._h, A, None, 0, 0, ctypes.byref(df), None) == E
    assert lib.lora_plan_diff(p._h, A, B, 0, 0, None, None) == E
    for begin, end in [(-1, 4), (0, 33), (5, 4), (33, 33)]:
        assert lib.lora_plan_stats(p._h, A, begin, end, ctypes.byref(st), None) == E, (begin, end)
        assert lib.lora_plan_diff(p._h, A, B, begin, end, ctypes.byref(df), None) == E, (begin, end)
    lib.lora_grid_stats_merge(None, ctypes.byref(st))  # tolerated, nothing to do
    lib.lora_grid_stats_merge(ctypes.byref(st), None)


def test_run_until_validates_its_arguments(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p = L.Plan("star2d1r", (32, 64))
    r = _lib.UntilResult()
    E = _lib.LORA_EINVAL

    def call(u, plan=p._h, b0=A, b1=B, res=r):
        return lib.lora_plan_run_until(plan, b0, b1, ctypes.byref(u) if u is not None else None,
                                       ctypes.byref(res) if res is not None else None, None)

    good = dict(tol=1e-9, rtol=0.0, norm=0, check_every=60, max_times=600)
    for bad in [dict(check_every=3), dict(check_every=1), dict(check_every=0), dict(check_every=-2), dict(check_every=61),
                dict(max_times=-1), dict(norm=2), dict(tol=-1.0), dict(tol=math.nan), dict(rtol=-1e-3)]:
        assert call(_lib.Until(**{**good, **bad})) == E, bad
    u = _lib.Until(**good)
    assert call(u, plan=None) == E and call(u, b0=None) == E and call(u, b1=None) == E and call(u, res=None) == E
    assert call(None) == E and call(u, b0=A, b1=A) == E
    # the group-A form checks the same
    dims = (ctypes.c_int * 3)(32, 64, 0)
    a = np.zeros((40, 72))
    o = np.zeros_like(a)
    info = _lib.RunInfo()
    odd = _lib.Until(**{**good, "check_every": 3})
    assert lib.lora_run_host_until(2, 0, a.ctypes.data, o.ctypes.data, None, dims, ctypes.byref(odd), ctypes.byref(r), 1,
                                   ctypes.byref(info)) == E
    assert lib.lora_run_host_until(2, 0, None, o.ctypes.data, None, dims, ctypes.byref(u), ctypes.byref(r), 1, None) == E
    assert lib.lora_run_host_until(2, 0, a.ctypes.data, o.ctypes.data, None, dims, None, ctypes.byref(r), 1, None) == E


def test_misaligned_buffers_are_unsupported(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    p = L.Plan("star2d1r", (32, 64))
    st, df, r = _lib.GridStats(), _lib.GridDiff(), _lib.UntilResult()
    u = _lib.Until(1e-9, 0.0, 0, 60, 600)
    U = _lib.LORA_EUNSUPPORTED
    assert lib.lora_plan_stats(p._h, A + 8, 0, 0, ctypes.byref(st), None) == U
    assert lib.lora_plan_diff(p._h, A, B + 8, 0, 0, ctypes.byref(df), None) == U
    assert lib.lora_plan_run_until(p._h, A + 8, B, ctypes.byref(u), ctypes.byref(r), None) == U


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_reductions_fail_loudly_without_gpu(L):
    from lorastencil_amd import _lib

    p = L.Plan("star2d1r", (32, 64))
    for call in [lambda: p.stats(A), lambda: p.diff(A, B), lambda: p.run_until(A, B, 1e-9, max_times=600),
                 lambda: L.run_host_until("star2d1r", L.reference_input("star2d1r", (32, 64)), 1e-9, max_times=600)]:
        with pytest.raises(L.LoraError) as e:
            call()
        assert e.value.status == _lib.LORA_ENODEVICE


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a C compiler")
def test_ctypes_structs_match_the_c_layout(L, tmp_path):
    from lorastencil_amd import _lib

    exe = tmp_path / "struct_sizes"
    subprocess.check_call(["g++", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "data", "struct_sizes_main.c"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    mirror = {"lora_grid_stats": _lib.GridStats, "lora_grid_diff": _lib.GridDiff, "lora_until": _lib.Until,
              "lora_until_result": _lib.UntilResult}
    assert len(c) == 13
    for key, value in c.items():
        name, _, fld = key.partition(".")
        got = getattr(mirror[name], fld).offset if fld else ctypes.sizeof(mirror[name])
        assert got == value, key


def run(dim, *args):
    p = subprocess.run([os.path.join(BIN, f"lorastencil_{dim}d"), *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_until_flags_are_validated(engine_built):
    base = ("star2d1r", "16", "24", "600")
    for flag in ["--until=abc", "--until=", "--until=-1e-6", "--until=1e-6x", "--until=nan"]:
        rc, out, err = run(2, *base, flag)
        assert rc == 1 and err == "Invalid argument: --until=TOL needs a non-negative number.\n" and out == "", flag
    for flag in ["--check-every=3", "--check-every=0", "--check-every=-4", "--check-every=x", "--check-every=4x"]:
        rc, out, err = run(2, *base, "--until=1e-6", flag)
        assert rc == 1 and err == "Invalid argument: --check-every=N needs a positive even integer.\n" and out == "", flag
    for other in ["--gpus=2", "--grid=1x2", "--check"]:
        for args in [("--until=1e-6", other), (other, "--until=1e-6")]:
            rc, out, err = run(2, *base, *args)
            assert rc == 1 and out == "", other
            assert err == "--until runs on one GPU against its own residual: not with --gpus, --grid or --check\n", other
    rc, _, err = run(1, "1d1r", "300", "600", "--until=1e-6", "--gpus=2")
    assert rc == 1 and err.startswith("--until runs on one GPU")
    rc, _, err = run(3, "box3d1r", "8", "8", "8", "60", "--dtype=bf16", "--until=zero")
    assert rc == 1 and err.startswith("Invalid argument: --until=TOL")


def test_cli_without_until_still_takes_every_old_flag(engine_built):
    """The old flags parse as before: the run gets as far as its INFO line and then to the device (or to the loud failure
    without one) -- never to "Unknown option"."""
    old2 = ["--no-extra", "--fill=random", "--fill=index", "--fill=ones", "--bc=reference", "--bc=dirichlet", "--normalize",
            "--gpus=1", "--dtype=f64", "--check"]
    rc, out, err = run(2, "star2d1r", "16", "24", "2", *old2)
    assert "Unknown option" not in err and out.startswith("INFO: shape = star_2d1r, m = 16, n = 24, times = 2\n")
    assert "Until:" not in out and rc == (0 if has_gpu() else 1)
    rc, out, err = run(3, "box3d1r", "8", "8", "8", "2", "--dtype=bf16", "--bc=periodic", "--no-extra")
    assert "Unknown option" not in err and out.startswith("INFO: shape = box_3d1r, h = 8, m = 8, n = 8, times = 2\n")
    assert rc == (0 if has_gpu() else 1)
    rc, out, err = run(2, "star2d1r", "16", "24", "2", "--grid=1x1", "--no-extra")
    assert "Unknown option" not in err and out.startswith("INFO:")
    rc, _, err = run(2, "star2d1r", "16", "24", "2", "--until")  # not a flag: the value is part of it
    assert rc == 1 and err == "Unknown option: --until\n"
