#!/usr/bin/env python3
"""Generates tests/golden/*.npz from the REAL reference host code (run in the build container only).

Inputs are the reference harness's own fills (un-seeded glibc rand(): rand()%10000 in 1D, rand()%100 in 2D/3D,
1d/main.cu:105-109, 2d/main.cu:232-236, 3d/main.cu:164-168) and its own params tables; expected outputs come
from the reference's own ``test_cpu`` (compiled from /root/reference by oracle/build_ref.sh into oracle/_ref),
chained with the reference driver's ping-pong (buffer 1 starts at zero, halos never written: 2d/gpu.cu:531-554).
So step 1 is exactly what the reference's CHECK_ERROR block compares against; steps > 1 extend it with the
driver semantics read from the reference host code.

Each fixture holds data only: `input`, `params`, `dims`, and `out_t<k>` = whole padded buffer [k % 2] after k steps.

`--ref-pins` writes the three fixtures that pin the oracle to test_cpu without oracle/_ref (tests/test_oracle.py):
  ref_random_params.npz   one sweep of test_cpu on gaussian input and taps: `<shape>_input`, `<shape>_params`, `<shape>_out`
  ref_chain.npz           `<shape>_t5`, `<shape>_t6`: the chain on the fixtures' inputs above, buffer [t % 2]
  ref_1d1r_config0.npz    BASELINE configs[0] (1d1r 2^20, 100 steps): `sha256` of the result's bytes (float64, last
                          element excluded: the operator leaves it untouched) and every 4096th element as `sample`
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle as o  # noqa: E402  (fill + params tables, themselves checked against libc / ref)
from oracle import ref  # noqa: E402

CASES = {
    "1d1r": (2048,),
    "1d2r": (2048,),
    "star2d1r": (64, 128),
    "box2d1r": (32, 64),
    "star2d3r": (64, 128),
    "box2d3r": (64, 128),
    "star3d1r": (8, 16, 128),
    "box3d1r": (8, 16, 128),
}
STEPS = (1, 2, 3, 4)
RANDOM_PARAMS_CASES = [("1d1r", (96,)), ("star2d1r", (16, 32)), ("box2d3r", (8, 24)), ("star2d3r", (12, 20)),
                       ("star3d1r", (5, 6, 18)), ("box3d1r", (4, 9, 10))]
CHAIN_STEPS = (5, 6)


def main():
    if not ref.available():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh (needs /root/reference)")
    here = os.path.dirname(os.path.abspath(__file__))
    for shape, dims in CASES.items():
        a = o.reference_input(shape, dims)
        params = o.default_params(shape)
        data = {"input": a, "params": params, "dims": np.array(dims, dtype=np.int64)}
        for t in STEPS:
            data[f"out_t{t}"] = ref.run_chain(a, params, t)
        path = os.path.join(here, f"{shape}.npz")
        np.savez_compressed(path, **data)
        print(f"{shape:10s} dims={dims} -> {os.path.getsize(path)} bytes")


def ref_pins():
    if not ref.available():
        sys.exit("oracle/_ref is missing: run oracle/build_ref.sh (needs the reference's sources)")
    import hashlib

    here = os.path.dirname(os.path.abspath(__file__))
    data = {}
    rng = np.random.default_rng(42)
    for shape, dims in RANDOM_PARAMS_CASES:
        a = rng.standard_normal(o.padded_shape(shape, dims))
        p = rng.standard_normal(o.NTAPS[len(dims)])
        data.update({f"{shape}_input": a, f"{shape}_params": p, f"{shape}_out": ref.test_cpu(a, p)})
    np.savez_compressed(os.path.join(here, "ref_random_params.npz"), **data)
    data = {}
    for shape, dims in CASES.items():
        a = o.reference_input(shape, dims)
        for t in CHAIN_STEPS:
            data[f"{shape}_t{t}"] = ref.run_chain(a, o.default_params(shape), t)
    np.savez_compressed(os.path.join(here, "ref_chain.npz"), **data)
    a = o.reference_input("1d1r", (1 << 20,))
    exp = ref.run_chain(a, o.default_params("1d1r"), 100)
    assert np.isfinite(exp).all()
    body = np.ascontiguousarray(exp[:-1], dtype="<f8")
    np.savez_compressed(os.path.join(here, "ref_1d1r_config0.npz"), sha256=np.array(hashlib.sha256(body.tobytes()).hexdigest()),
                        sample=body[::4096].copy())
    for f in ("ref_random_params.npz", "ref_chain.npz", "ref_1d1r_config0.npz"):
        print(f"{f:24s} {os.path.getsize(os.path.join(here, f))} bytes")


if __name__ == "__main__":
    if "--ref-pins" in sys.argv[1:]:
        ref_pins()
    else:
        main()
