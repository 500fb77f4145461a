"""GPU tests of the run-until-steady driver (lora_plan_run_until, lora_run_host_until, the CLIs' --until).

Yardsticks are the engine's own plain runs (lora_plan_run from the same input, code older than the driver) and numpy on
their results: where the driver stops, what it leaves in d_buf0 and the residual it reports are all recomputed from them.
Nothing here hard-codes a step count.
"""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "lorastencil_amd", "bin")


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    return L


def taps_2d():
    w = np.zeros(49)
    w[[24, 23, 25, 17, 31]] = 0.2  # the centre and its four neighbours
    return w


def taps_1d():
    w = np.zeros(9)
    w[[3, 4, 5]] = 1.0 / 3.0
    return w


def normalised(L, shape):
    w = L.effective_weights(shape)
    return w / w.sum()


def make_plan(L, shape, dims, dtype="f64", bc="dirichlet", weights=None):
    p = L.Plan(shape, dims, dtype=dtype).set_boundary(bc)
    if weights is not None:
        p.set_weights(weights)
    return p


def device_pair(a_host, dtype):
    """(d_buf0 = the padded input, d_buf1 = zeros) as a fresh run takes them"""
    import torch

    b0 = torch.from_numpy(a_host).to(torch.bfloat16 if dtype == "bf16" else torch.float64).cuda()
    return b0, torch.zeros_like(b0)


def raw(t):
    """integer view: equality of bits, NaNs included"""
    import torch

    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int64)


def plain_run(plan, a_host, dtype, times):
    """a fresh lora_plan_run(times) from the input: the whole padded result buffer (on the device)"""
    import torch

    b0, b1 = device_pair(a_host, dtype)
    plan.run(b0, b1, times)
    torch.cuda.synchronize()
    return b1 if times % 2 else b0


def residual_of_plain_runs(L, plan, shape, a_host, dtype, T):
    """max |u(T + 1) - u(T)| and the number of non-finite differences, by numpy on two plain runs"""
    u0 = L.interior(shape, plain_run(plan, a_host, dtype, T)).double().cpu().numpy()
    u1 = L.interior(shape, plain_run(plan, a_host, dtype, T + 1)).double().cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        d = u1 - u0
    ok = np.isfinite(d)
    return (float(np.abs(d[ok]).max()) if ok.any() else 0.0), int(d.size - ok.sum())


def check_against_plain_runs(L, plan, shape, a_host, dtype, tol, check_every, max_times):
    """Runs the driver and recomputes everything it reports from plain runs.  Returns the driver's result."""
    import torch

    b0, b1 = device_pair(a_host, dtype)
    r = plan.run_until(b0, b1, tol, check_every=check_every, max_times=max_times)
    torch.cuda.synchronize()
    print(shape, dtype, r)
    T = r.times_done
    assert T % check_every == 0 and T <= max_times and r.checks == T // check_every
    assert torch.equal(raw(b0), raw(plain_run(plan, a_host, dtype, T))), "d_buf0 is not what lora_plan_run(times_done) gives"
    if T == 0:
        return r
    res, bad = residual_of_plain_runs(L, plan, shape, a_host, dtype, T)
    print("plain runs at", T, ":", res, bad)
    assert r.last.nonfinite == bad and r.diverged == (bad > 0)
    assert np.float64(r.residual).tobytes() == np.float64(res).tobytes()
    assert r.converged == (bad == 0 and res <= tol)
    if not (r.converged or r.diverged):
        assert T + check_every > max_times  # it stopped at the cap and nowhere else
    # the check before this one did not stop the run
    if T > check_every:
        before, bad_before = residual_of_plain_runs(L, plan, shape, a_host, dtype, T - check_every)
        print("plain runs at", T - check_every, ":", before, bad_before)
        assert bad_before == 0 and before > tol
        if tol > 0:  # a residual this close to the tolerance would make the stopping step a matter of the last bit
            assert not tol / 1.05 < before < tol * 1.05
    if tol > 0:
        assert not tol / 1.05 < res < tol * 1.05
    return r


def test_converging_2d_dirichlet(L):
    shape, dims = "star2d1r", (16, 24)
    # rand() % 100, halo included; seeded with 4: the un-seeded fill has the residual of sweep 1750 at 1.0025e-9, within 5 % of the
    # tolerance (a numpy replay of this seed: 1.30e-9 after 1800 sweeps, 7.9e-10 after 1850)
    a = L.reference_input(shape, dims, rng=L.GlibcRand(4))
    p = make_plan(L, shape, dims, weights=taps_2d())
    r = check_against_plain_runs(L, p, shape, a, "f64", 1e-9, 50, 6000)
    assert r.converged and not r.diverged and r.residual <= 1e-9 and 0 < r.times_done < 6000
    assert r.last.count == 16 * 24 and r.last.max_abs == r.residual
    # the RMS norm stops no later than the maximum norm, and rtol scales the tolerance with the level
    b0, b1 = device_pair(a, "f64")
    rms = p.run_until(b0, b1, 1e-9, norm="rms", check_every=50, max_times=6000)
    assert rms.converged and rms.times_done <= r.times_done
    assert rms.residual == np.sqrt(rms.last.sum_sq / rms.last.count) <= rms.last.max_abs
    b0, b1 = device_pair(a, "f64")
    rel = p.run_until(b0, b1, 0.0, rtol=1e-9, check_every=50, max_times=6000)
    assert rel.converged and rel.times_done < r.times_done and rel.residual <= 1e-9 * rel.last.a_abs_max


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-9), ("bf16", 0.0)])
def test_converging_3d_dirichlet(L, dtype, tol):
    """bf16 with tol = 0: the iteration reaches an exact fixed point or the cap -- whichever the plain runs show."""
    shape, dims = "box3d1r", (12, 16, 24)
    # (rand() seeded with 2: the un-seeded fill puts the fp64 residual of sweep 500 at 9.56e-10, within 5 % of the tolerance)
    a = L.reference_input(shape, dims, rng=L.GlibcRand(2))
    p = make_plan(L, shape, dims, dtype=dtype, weights=normalised(L, shape))
    r = check_against_plain_runs(L, p, shape, a, dtype, tol, 50, 6000)
    if dtype == "f64":
        assert r.converged and 0 < r.times_done < 6000
    else:
        assert r.converged or r.times_done == 6000


def test_1d_dirichlet(L):
    """n = 300 diffuses too slowly to reach 1e-9 within 6000 sweeps of these taps (the slowest mode decays by 3.6e-5 a sweep):
    whichever the plain runs show, here across the 1D kernels' launch depths (runs of 50 against one run of times_done)."""
    shape, dims = "1d1r", (300,)
    a = L.reference_input(shape, dims)
    p = make_plan(L, shape, dims, weights=taps_1d())
    r = check_against_plain_runs(L, p, shape, a, "f64", 1e-9, 50, 6000)
    assert not r.diverged and r.times_done > 0
    # a tolerance it does reach early: a numpy replay has the residual at 8.07 after 100 sweeps and at 5.23 after 150
    loose = check_against_plain_runs(L, p, shape, a, "f64", 6.5, 50, 6000)
    assert loose.converged and 0 < loose.times_done < r.times_done


def test_periodic_is_the_plain_run(L):
    shape, dims = "star2d1r", (16, 24)
    a = L.reference_input(shape, dims)
    p = make_plan(L, shape, dims, bc="periodic", weights=taps_2d())
    r = check_against_plain_runs(L, p, shape, a, "f64", 1e-9, 50, 6000)
    assert r.converged and not r.diverged


def test_not_converging_under_the_reference_boundary(L):
    """The alternating halo of the reference driver gives a two-cycle: the residual stalls far above the tolerance."""
    shape, dims = "star2d1r", (16, 24)
    a = L.reference_input(shape, dims)
    p = make_plan(L, shape, dims, bc="reference", weights=taps_2d())
    r = check_against_plain_runs(L, p, shape, a, "f64", 1e-9, 50, 620)
    assert (r.converged, r.diverged, r.times_done, r.checks) == (False, False, 600, 12)
    assert r.residual > 1.0
    # a cap below one round: nothing runs, nothing is touched
    b0, b1 = device_pair(a, "f64")
    none = p.run_until(b0, b1, 1e-9, check_every=50, max_times=49)
    assert (none.times_done, none.checks, none.converged, none.diverged) == (0, 0, False, False) and none.residual == np.inf
    assert np.array_equal(b0.cpu().numpy(), a) and not b1.any()


def test_diverging_integer_taps(L):
    """box2d3r with the reference's integer taps overflows fp64 after about 129 sweeps."""
    import torch

    shape, dims = "box2d3r", (24, 24)
    a = L.reference_input(shape, dims)
    p = make_plan(L, shape, dims, bc="reference")
    expect = None
    for T in range(20, 401, 20):  # the first check whose probe level holds a non-finite value in the plain runs
        if not torch.isfinite(L.interior(shape, plain_run(p, a, "f64", T + 1))).all():
            expect = T
            break
    assert expect is not None and expect > 20
    r = check_against_plain_runs(L, p, shape, a, "f64", 1e-9, 20, 400)
    assert r.diverged and not r.converged and r.times_done == expect and r.last.nonfinite > 0


def test_plan_is_reusable_after_run_until(L):
    import torch

    shape, dims = "star2d1r", (16, 24)
    a = L.reference_input(shape, dims)
    p = make_plan(L, shape, dims, weights=taps_2d())
    b0, b1 = device_pair(a, "f64")
    assert p.run_until(b0, b1, 1e-3, check_every=50, max_times=6000).converged
    fresh = make_plan(L, shape, dims, weights=taps_2d())
    for times in (7, 50, 51):
        assert torch.equal(raw(plain_run(p, a, "f64", times)), raw(plain_run(fresh, a, "f64", times))), times
    # and its reductions still answer
    assert p.stats(plain_run(p, a, "f64", 0)).count == 16 * 24


@pytest.fixture()
def dirichlet_normalised_defaults():
    """what the CLIs' --bc=dirichlet --normalize set for plans created afterwards on this thread"""
    from lorastencil_amd import _lib

    lib = _lib.lib()
    bc, norm = lib.lora_set_default_boundary(_lib.BC_DIRICHLET), lib.lora_set_default_normalize(1)
    yield
    lib.lora_set_default_boundary(bc)
    lib.lora_set_default_normalize(norm)


def test_group_a_and_cli_agree_with_the_plan_form(L, dirichlet_normalised_defaults):
    import torch

    shape, dims = "star2d1r", (16, 24)
    a = L.reference_input(shape, dims)
    p = L.Plan(shape, dims)  # takes the defaults: Dirichlet boundary, the operator's taps over their sum
    assert p.get_option("boundary") == 1 and abs(p.weights.sum() - 1.0) < 1e-12
    for check_every in (50, 60):
        b0, b1 = device_pair(a, "f64")
        want = p.run_until(b0, b1, 1e-9, check_every=check_every, max_times=6000)
        torch.cuda.synchronize()
        assert want.converged
        out, got, info = L.run_host_until(shape, a, 1e-9, check_every=check_every, max_times=6000)
        assert got == want and np.array_equal(out, b0.cpu().numpy())
        assert info.sweep_seconds > 0 and info.gstencils > 0
    # the CLI: same input (its random fill is the reference harness's), same taps, check_every = 60 by default
    exe = os.path.join(BIN, "lorastencil_2d")
    run = subprocess.run([exe, shape, "16", "24", "6000", "--bc=dirichlet", "--normalize", "--until=1e-9"], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "INFO: shape = star_2d1r, m = 16, n = 24, times = 6000" and lines[1] == "LoRAStencil(2D star_2d1r): "
    m = re.search(r"^Until: times_done = (\d+), (converged|diverged|reached the cap), residual = (\S+) ", run.stdout, re.M)
    assert m, run.stdout
    assert int(m.group(1)) == want.times_done and m.group(2) == "converged"
    assert abs(float(m.group(3)) - want.residual) <= 1e-5 * want.residual  # (%g prints six digits)
    starts = [x.split(" ")[0] for x in lines]
    assert starts.index("Until:") > starts.index("GStencil/s")  # after the operator's three lines
    # without --until the same invocation prints no such line
    plain = subprocess.run([exe, shape, "16", "24", "60", "--bc=dirichlet", "--normalize"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "Until:" not in plain.stdout
