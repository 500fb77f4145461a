"""Compile-time guard of the 2D two-step kernel (kernels_2d_step2.hip): no GPU needed.

The one body serves four rules, and two of its spellings are there for the register allocator (the comment at the level-1
boundary value).  What they buy is asserted here from the compiler's own report, so a compiler update or an edit that loses
it fails a test instead of a benchmark: every instantiation has no scratch, and keeps the waves per SIMD the three separate
kernels had (profiles/step2_fold_resources.txt): 5 for the star's EPI_SOURCE, 4 for the star's other rules, 3 for the
diamond and the box under __launch_bounds__(256, 3).
"""
import os
import re
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorastencil_amd", "csrc")
STAR, EPI_SOURCE = 1, 0


def test_two_step_kernel_keeps_waves_and_has_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
                        "-c", "kernels_2d_step2.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*stencil2d_step2_kernelILi(\d+)ELi(\d+)ELi(\d+)E", line)
        if m:
            name = tuple(int(g) for g in m.groups())
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    assert sorted(seen) == sorted((t, 6 if t == STAR else 10, e) for t in range(3) for e in range(4))
    for (tapset, r1, epi), got in seen.items():
        print(tapset, r1, epi, got)
        want = 3 if tapset != STAR else (5 if epi == EPI_SOURCE else 4)
        assert got["scratch"] == 0, (tapset, r1, epi, got)
        assert got["waves"] >= want, (tapset, r1, epi, got)
