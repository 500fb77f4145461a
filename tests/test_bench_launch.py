"""bench.py's launch path: `python bench.py --gpus N` must start its own N ranks (the driver's N = 1 form of the command,
with N > 1) and print ONE JSON line from rank 0.  On a box without a GPU only the plumbing can run
(`--plumbing-only`: rendezvous + one reduction, value null -- the engine has no CPU path to measure); the same command
with real sweeps is the GPU test below."""
import json
import os
import subprocess
import sys

import pytest
from conftest import ROOT


def _bench(*args, env=None, timeout=600):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=e,
                       timeout=timeout, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, lines


def test_bench_starts_its_own_ranks():
    r, lines = _bench("--gpus", "2", "--steps", "4", "--warmup", "0", "--plumbing-only")
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["plumbing_only"] is True and d["value"] is None


def test_planned_launches_follow_the_driver_rule():
    sys.path.insert(0, ROOT)
    import bench

    # (K-application launches, two-application launches, single sweeps) of a slab run: SlabDriver.run's rule
    assert bench.planned_launches(1, 100, 8) == (12, 0, 4)   # 1D: 12 eight-step launches + 4 single sweeps
    assert bench.planned_launches(2, 100, 2) == (50, 0, 0)
    assert bench.planned_launches(2, 21, 2) == (10, 0, 1)
    assert bench.planned_launches(2, 20, 4) == (5, 0, 0)      # an odd number of fused launches is fine in a slab run
    assert bench.planned_launches(2, 23, 4) == (5, 1, 1)      # 2D, K = 4: a two-application launch for the tail
    assert bench.planned_launches(2, 23, 6) == (3, 1, 1)      # K = 6: 18 + a four-application tail + one single sweep
    assert bench.planned_launches(2, 21, 6) == (3, 1, 1)      # ... 18 + a two-application tail + one
    assert bench.planned_launches(3, 23, 4) == (5, 1, 1)      # 3D, K = 4: tails of two
    from lorastencil_amd.slab import launch_depths
    assert launch_depths(2, 6, 23) == [6, 6, 6, 4, 1]
    assert launch_depths(2, 6, 23, tails=(2,)) == [6, 6, 6, 2, 2, 1]   # a stepper without four-application launches
    assert launch_depths(2, 6, 9, steps_done=1) == [1, 6, 2]            # a resumed run starts fusing at an even level
    assert launch_depths(2, 6, 9, fused=False) == [1] * 9
    assert bench.planned_launches(3, 7, 2) == (3, 0, 1)
    assert bench.planned_launches(2, 20, 1) == (0, 0, 20)


def test_dumped_outputs_are_the_interior_or_a_fixed_sample(monkeypatch):
    """--dump-outputs: the result grid's interior, whole (float64; bf16 as float32) or, past the size limit, at the same
    seeded interior points every time -- within the 64 MB the option may write."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from lorastencil_amd.ops import halo, padded_shape

    assert bench.DUMP_WHOLE_BYTES <= 64 << 20 and bench.DUMP_SAMPLE_POINTS * 8 <= 64 << 20
    shape, dims = "star2d1r", (6, 10)
    ps = padded_shape(shape, dims)
    g = torch.arange(ps[0] * ps[1], dtype=torch.float64).reshape(ps)
    out = bench.output_arrays(shape, dims, g)
    assert list(out) == ["out"] and out["out"].dtype == np.float64 and np.array_equal(out["out"], g[4:10, 4:14].numpy())
    out = bench.output_arrays(shape, dims, g.to(torch.bfloat16))
    assert out["out"].dtype == np.float32 and np.array_equal(out["out"], g[4:10, 4:14].to(torch.bfloat16).float().numpy())
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 0)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_POINTS", 40)
    for shape, dims in (("star2d1r", (6, 10)), ("box3d1r", (3, 4, 5)), ("1d2r", (50,))):
        ps = padded_shape(shape, dims)
        g = torch.arange(int(np.prod(ps)), dtype=torch.float64).reshape(ps)
        s1, s2 = bench.output_arrays(shape, dims, g), bench.output_arrays(shape, dims, g.clone())
        assert list(s1) == ["out_sample"] and np.array_equal(s1["out_sample"], s2["out_sample"])
        v = s1["out_sample"]
        assert 0 < v.size <= 40 and v.dtype == np.float64 and np.all(np.diff(v) > 0)  # sorted, no repeats
        interior = np.zeros(ps, bool)
        interior[tuple(slice(k, k + d) for k, d in zip(halo(shape), dims))] = True
        assert interior.ravel()[v.astype(np.int64)].all()


@pytest.mark.gpu
def test_bench_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run prints the headline fields only (no roofline, no CPU baseline); --dump-outputs writes what the K timed
    steps computed, the same in two runs, and it is the oracle's result on the same seeded input."""
    import numpy as np
    import torch

    from oracle import oracle as O

    shape, dims, K, W = "star2d1r", (256, 384), 6, 1
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r, lines = _bench("--steps", str(K), "--warmup", str(W), "--size", *map(str, dims), "--dump-outputs", str(d))
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(lines) == 1
        line = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line
        assert "roofline" not in line and "cpu_baseline" not in line
        assert line["steps"] == K and line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        assert sorted(p.name for p in d.iterdir()) == ["out.npy"]
        outs.append(np.load(d / "out.npy"))
    assert outs[0].dtype == np.float64 and outs[0].shape == dims and np.array_equal(outs[0], outs[1])
    # bench.py's input: small integers from a device generator seeded 1234 (rank 0)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    a = torch.randint(0, 100, O.padded_shape(shape, dims), generator=gen, device="cuda").to(torch.float64).cpu().numpy()
    exp = O.interior(shape, O.run(shape, a, K))
    assert np.abs(outs[0] - exp).max() <= 1e-12 * np.abs(exp).max()


@pytest.mark.gpu
def test_bench_two_ranks_over_gloo_on_one_gpu():
    r, lines = _bench("--gpus", "2", "--steps", "4", "--warmup", "0", "--size", "256", "256", "--no-cpu-baseline",
                      "--full", env={"LORA_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["roofline"]["frac"] <= 1.0


@pytest.mark.gpu
def test_bench_line_roofline_is_a_fraction():
    r, lines = _bench("--steps", "8", "--warmup", "2", "--size", "2048", "2048", "--cpu-seconds", "1", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(lines[-1])
    rf = d["roofline"]
    # 8 sweeps = 6 + 2, which the driver runs as 4 + 4: no full-depth launch, two four-application ones
    assert d["n_gpus"] == 1 and 0 < rf["frac"] <= 1.0 and rf["applications_per_launch"] == 4
    assert 0 < rf["hbm"]["frac"] <= 1.0 and rf["bound"] in ("hbm", "fp64_valu") and rf["limiter"] in ("hbm", "valu", "lds")
    # the arithmetic roof is priced on EXECUTED instructions (the kernel's own PMC profile) or not at all: the direct-form
    # flops the low-rank evaluation never performs are reported, labelled, and never become `frac` beyond what the pipe can do
    fp = rf["fp64"]
    assert fp["useful_direct_form_tflops"] > 0 and fp["flops_per_point_direct_form"] == 49
    if fp["executed"] is not None:
        assert 0 < fp["executed"]["frac"] <= 1.0 and fp["executed"]["ops_per_point"] < 49
    if rf["bound"] == "hbm":
        assert rf["frac"] == rf["hbm"]["frac"] and rf["unit"] == "GB/s"
    else:
        assert rf["unit"] == "TFLOP/s" and rf["frac"] <= 1.0
    assert abs(rf["frac_one_sweep_equiv"] - 4 * rf["hbm"]["frac"]) < 1e-3 and rf["launches"] == 2
    assert rf["tail_fused_launches"] == 2 and rf["clock_ramp_note"] is not None
    assert rf["traffic"] is None or rf["traffic_key"].endswith(rf["kernel"])  # never a number of another kernel
    assert d["cpu_baseline"]["cores"] >= 1
