"""Compile-time guard of the kernels on the shared fp64 tile walk (csrc/tile_walk.h): no GPU needed.

One walk per dimension serves the residual, apply_dot and theta kernels (theta3d_kernel alone restates the 3D walk in its own
file), and one spelling is there for the register allocator (tiles and taps by value in 2D).  What the kernels have is asserted
here from the compiler's own report, so a compiler update or an edit that loses it fails a test instead of a benchmark: the
set of instantiations is the one the walk was folded from, none has scratch, and each keeps at least the waves per SIMD it had
before the fold (profiles/tile_walk_fold_resources.txt).  Exact VGPR counts are printed, not asserted.
"""
import os
import re
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorastencil_amd", "csrc")
STAR3, BOX3 = 0, 1
SHIFT, START, START_SRC, DEFECT, DEFECT_SRC = range(5)

# waves per SIMD by kernel and template arguments (tap set first; bool SRC as 0 / 1; theta: MODE last)
WAVES = {("residual1d", (s,)): 8 for s in (0, 1)}
WAVES.update({("residual2d", (t, s)): 3 for t in range(3) for s in (0, 1)})
WAVES.update({("residual3d", (t, s)): 3 if s else 4 for t in (STAR3, BOX3) for s in (0, 1)})
WAVES.update({("residual3d_bf16", (t,)): 4 for t in range(3)})
WAVES[("apply_dot1d", ())] = 8
WAVES.update({("apply_dot2d", (t,)): 3 for t in range(3)})
WAVES.update({("apply_dot3d", (t,)): 3 for t in (STAR3, BOX3)})
WAVES.update({("theta1d", (m,)): 8 for m in range(5)})
WAVES.update({("theta2d", (t, m)): 3 for t in range(3) for m in range(5)})
WAVES.update({("theta3d", (t, m)): 3 for t in (STAR3, BOX3) for m in (SHIFT, START_SRC)})
WAVES.update({("theta3d", (t, m)): 4 for t in (STAR3, BOX3) for m in (DEFECT, DEFECT_SRC)})
WAVES.update({("theta3d", (STAR3, START)): 4, ("theta3d", (BOX3, START)): 3})


def compile_report(name):
    """{(kernel, template arguments): {scratch, waves, vgprs}} of the fold's kernels in one file, from the compiler's remarks"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
                        "-c", name, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, key = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"\d+(residual[123]d(?:_bf16)?|apply_dot[123]d|theta[123]d)_kernel(?:I((?:L[ib]\d+E)+)E)?", m.group(1))
            key = (k.group(1), tuple(int(a) for a in re.findall(r"L[ib](\d+)E", k.group(2) or ""))) if k else None
            if key:
                seen[key] = {}
        for field, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"),
                           ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and key:
                seen[key][field] = int(m.group(1))
    return seen


def test_walk_kernels_keep_their_waves_and_have_no_scratch():
    seen = {}
    for name in ("kernels_residual.hip", "kernels_cg.hip", "kernels_theta.hip"):
        seen.update(compile_report(name))
    count = lambda prefix: sum(k[0] in prefix for k in seen)
    assert (count(("residual1d", "residual2d", "residual3d")), count(("residual3d_bf16",)), count(("apply_dot1d", "apply_dot2d", "apply_dot3d")),
            count(("theta1d", "theta2d", "theta3d"))) == (12, 3, 6, 30)  # fp64 residual: 2 in 1D, 3 x 2 in 2D, 2 x 2 in 3D
    assert sorted(seen) == sorted(WAVES)
    for key, got in sorted(seen.items()):
        print(key, got)
        assert got["scratch"] == 0, (key, got)
        assert got["waves"] >= WAVES[key], (key, got)
