#!/usr/bin/env python3
"""Records tests/golden/plan_resolution.json.gz: what plans resolve to, observed through the C ABI alone.

A plan resolves without a device (the residency queries answer "fits", launches with null buffers answer
LORA_EUNSUPPORTED for a depth the plan does not have and LORA_EINVAL for one it has), so everything here is host work:

  resolution   the cross product of shapes x boundaries x element types x grids x option overrides x tap tables; per
               case the statuses of the calls that set it up, the kernel signature (name included), every readable
               option, region granularity, padded bytes and the return codes of stepn (1..33), step2 and stepk
  validation   every settable key on one plan per (ndim, dtype), a fixed list of values each: status and signature
  sequences    fixed sequences of set calls as status-and-state traces (order dependence)

tests/test_plan_resolution.py imports this module, observes the same cases with the library under test and compares.
Values that repeat (signatures, option tuples, code strings) are stored once per field and referred to by index; the JSON
is kept gzip-compressed, like the .npz fixtures beside it (`zcat tests/golden/plan_resolution.json.gz | python -m json.tool`
shows it).

    python tests/golden/make_plan_resolution.py      # rewrites the fixture from the library that is built
"""
import ctypes
import gzip
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_resolution.json.gz")

SHAPES = ["1d1r", "1d2r", "star2d1r", "box2d1r", "star2d3r", "box2d3r", "star3d1r", "box3d1r"]
NDIM = {"1d1r": 1, "1d2r": 1, "star2d1r": 2, "box2d1r": 2, "star2d3r": 2, "box2d3r": 2, "star3d1r": 3, "box3d1r": 3}
BOUNDARIES = [0, 1, 2]  # reference, Dirichlet, periodic
F64, BF16 = 0, 1
VARIANT_DIRECT, VARIANT_MFMA = 1, 2

# One grid between every two neighbouring size rules of the resolvers.  3D point counts: 2.0e6, 1.0e7, 1.2e7, 1.4e7,
# 2.4e7, 3.0e7, 1.2e8, 3.0e8; z_chunk (lora_plan_create) comes out 4 (8 x 16 x 128), 7 (312^3) and 16 (496^3); odd
# innermost extents on both sides of the 1.0e7 rule of the register-resident kernels; grids smaller than their halo.
DIMS = {
    1: [(3,), (4096,), (1 << 20,)],
    2: [(2, 2), (64, 128), (64, 127), (8192, 8192)],
    3: [(8, 16, 128), (128, 128, 128), (216, 216, 216), (232, 232, 224), (240, 240, 248), (296, 288, 288),
        (312, 312, 312), (496, 496, 496), (672, 672, 672), (4, 4, 5), (208, 216, 215), (216, 216, 215)],
}

# option overrides: (key, value) pairs applied in order; ("variant", v) goes through lora_plan_set_variant
OVERRIDES = ([[]] + [[("steps_per_launch", k)] for k in (1, 2, 3, 4, 6, 8, 16, 32)] +
             [[("stream", 0)], [("wg", 0)], [("wg", 1)], [("stream3", 0)], [("stream3", 1)], [("lanes3", 0)], [("lanes3", 1)],
              [("separable", 0)]] + [[("lowrank_valu", v)] for v in (0, 1, 2, 3, 4)] +
             [[("stream3_pipe", 1)], [("stream3_async", 1)], [("stream3_waves", 4)], [("stream3_waves", 8)],
              [("stream3_async", 1), ("stream3_waves", 4)], [("variant", VARIANT_MFMA)]])

# every key lora_plan_get_option answered at the commit this fixture was recorded from
READABLE = ["rows_per_thread", "panel_width", "z_chunk", "nt_store", "persistent", "graph", "stream", "stream3", "stream3_waves",
            "stream3_slots", "stream3_pipe", "stream3_async", "stream_rows", "stream_depth", "stream_sync", "boundary",
            "fused_eval", "lowrank_valu", "lds_dma", "separable", "cols_per_lane", "fused_rows", "steps_per_launch",
            "fused_z_chunk", "spans3", "torus", "fused_pipeline", "tapset", "variant"]

# settable keys and the values tried: -2, -1, 0, 1, each bound of the accepted range and one value past it
_COMMON = [-2, -1, 0, 1]
SETTABLE = {
    "rows_per_thread": [3, 4, 5, 8, 16, 17], "panel_width": [2, 32, 1 << 20], "z_chunk": [2, 16, 4096], "nt_store": [2],
    "persistent": [2], "stream": [2], "stream_rows": [1 << 20, (1 << 20) + 1], "wg": [2], "wg_rows": [1 << 20, (1 << 20) + 1],
    "wg_prio": [24, 25], "wg_edge_pct": [100, 101], "stream_depth": [2, 6, 7], "stream3": [2], "lanes3": [2],
    "stream3_waves": [4, 8, 9], "stream3_async": [2], "stream3_pipe": [2], "stream3_slots": [2, 3], "stream_share": [2],
    "stream_prefetch": [2], "stream_sync": [2, 3], "scratch": [2], "mfma_split": [2], "graph": [2], "lowrank_valu": [4, 5],
    "separable": [2], "ablate": [63, 64], "lds_dma": [2], "cols_per_lane": [4, 8, 9], "fused_rows": [6, 8, 10, 11],
    "steps_per_launch": list(range(2, 34)), "fused_pipeline": [2], "fused_z_chunk": [4096, 4097], "spans3": [2, 3], "torus": [2],
    "no_such_option": [],
}
VALIDATION_PLANS = [("1d1r", F64, (4096,)), ("star2d1r", F64, (64, 128)), ("box3d1r", F64, (128, 128, 128)),
                    ("box3d1r", BF16, (128, 128, 128))]


def _lcg_table(n, seed):
    """n non-zero integer taps without structure (no low-rank form, not separable)"""
    out, x = [], seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append(float((x >> 16) % 19 + 1) * (1.0 if (x >> 8) & 1 else -1.0))
    return out


def tap_tables(ndim):
    """name -> taps (None: the shape's own table)"""
    if ndim == 2:
        rank1 = [float(a * b) for a in (1, 2, 3, 4, 5, 6, 7) for b in (1, -1, 2, -2, 3, -3, 4)]  # asymmetric, rank 1
        return {"default": None, "random49": _lcg_table(49, 3), "rank1": rank1}
    if ndim == 3:
        sep = [a * b * c for a in (1.0, 2.0, 1.0) for b in (0.5, 1.0, 0.5) for c in (3.0, 5.0, 7.0)]
        return {"default": None, "separable27": sep, "random27": _lcg_table(27, 5)}
    return {"default": None}


def library():
    from lorastencil_amd import _lib

    return _lib.lib()


def _create(lib, shape, dtype, dims):
    plan = ctypes.c_void_p()
    rc = lib.lora_plan_create(ctypes.byref(plan), SHAPES.index(shape), dtype, (ctypes.c_int * 3)(*dims), None)
    return rc, (plan if rc == 0 else None)


def _set_weights(lib, plan, taps):
    return lib.lora_plan_set_weights(plan, (ctypes.c_double * len(taps))(*taps), len(taps))


def _apply(lib, plan, op):
    key, value = op
    if key == "variant":
        return lib.lora_plan_set_variant(plan, value)
    if key == "boundary":
        return lib.lora_plan_set_boundary(plan, value)
    return lib.lora_plan_set_option(plan, key.encode(), value)


def _get(lib, plan, key):
    v = ctypes.c_int()
    rc = lib.lora_plan_get_option(plan, key.encode(), ctypes.byref(v))
    return v.value if rc == 0 else None


def _code(rc):  # 0 -> "0", LORA_EINVAL -> "1", LORA_EUNSUPPORTED -> "2", ...
    return str(-rc)


def observe(lib, plan):
    """everything the fixture records of a plan's resolved state"""
    codes = [lib.lora_plan_stepn_region(plan, k, None, None, 0, 0, None) for k in range(1, 34)]
    codes += [lib.lora_plan_step2(plan, None, None, None), lib.lora_plan_stepk(plan, None, None, None)]
    sig = lib.lora_plan_kernel_signature(plan).decode()
    name = lib.lora_plan_kernel_name(plan).decode()
    assert sig.startswith(name + "["), (name, sig)
    return {"signature": sig, "options": [_get(lib, plan, k) for k in READABLE],
            "granularity": lib.lora_plan_region_granularity(plan), "padded_bytes": lib.lora_plan_padded_bytes(plan),
            "codes": "".join(_code(rc) for rc in codes)}


def resolution_cases():
    for shape in SHAPES:
        nd = NDIM[shape]
        for dtype in ((F64, BF16) if nd == 3 else (F64,)):
            for dims, bc, (taps_name, taps), over in itertools.product(DIMS[nd], BOUNDARIES, tap_tables(nd).items(), OVERRIDES):
                label = "%s/%s/%s/bc%d/%s/%s" % (shape, "bf16" if dtype else "f64", "x".join(map(str, dims)), bc, taps_name,
                                                 ",".join("%s=%d" % kv for kv in over) or "-")
                yield label, (shape, dtype, dims, bc, taps, over)


def observe_resolution(lib, case):
    shape, dtype, dims, bc, taps, over = case
    rc, plan = _create(lib, shape, dtype, dims)
    if plan is None:
        return {"setup": _code(rc)}
    try:
        setup = [rc]
        if taps is not None:
            setup.append(_set_weights(lib, plan, taps))
        setup.append(lib.lora_plan_set_boundary(plan, bc))
        setup += [_apply(lib, plan, op) for op in over]
        return dict(observe(lib, plan), setup="".join(_code(r) for r in setup))
    finally:
        lib.lora_plan_destroy(plan)


def validation_cases():
    for shape, dtype, dims in VALIDATION_PLANS:
        for key, extra in SETTABLE.items():
            for value in sorted(set(_COMMON + extra)):
                yield "%s/%s/%s=%d" % (shape, "bf16" if dtype else "f64", key, value), (shape, dtype, dims, key, value)


def observe_validation(lib, case):
    shape, dtype, dims, key, value = case
    rc, plan = _create(lib, shape, dtype, dims)
    assert plan is not None, case
    try:
        rc = lib.lora_plan_set_option(plan, key.encode(), value)
        return {"status": rc, "signature": lib.lora_plan_kernel_signature(plan).decode()}
    finally:
        lib.lora_plan_destroy(plan)


def _sequences():
    t2, t3 = tap_tables(2), tap_tables(3)
    w = lambda taps: ("weights", taps)
    o = lambda k, v: (k, v)
    return {
        "2d mfma, unfactorable taps, old taps back": ("box2d3r", F64, (64, 128), [o("variant", VARIANT_MFMA), w(t2["random49"]), w("own"), o("variant", VARIANT_MFMA)]),
        "3d bf16 mfma, unfactorable taps, old taps back": ("box3d1r", BF16, (128, 128, 128), [o("variant", VARIANT_MFMA), w(t3["random27"]), w("own"), o("variant", VARIANT_MFMA)]),
        "2d boundary before steps_per_launch": ("star2d1r", F64, (64, 128), [o("boundary", 1), o("steps_per_launch", 6), o("steps_per_launch", 2), o("boundary", 0)]),
        "2d boundary after steps_per_launch": ("star2d1r", F64, (64, 128), [o("steps_per_launch", 6), o("boundary", 1), o("boundary", 2), o("boundary", 0), o("steps_per_launch", 4), o("boundary", 1)]),
        "2d periodic on a grid smaller than its halo": ("star2d1r", F64, (2, 2), [o("boundary", 2), o("steps_per_launch", 4), o("boundary", 1)]),
        "1d periodic on a grid smaller than its halo": ("1d1r", F64, (3,), [o("boundary", 2), o("steps_per_launch", 32), o("boundary", 1), o("steps_per_launch", 3)]),
        "3d star between the kernels": ("star3d1r", F64, (216, 216, 216), [o("lanes3", 0), o("steps_per_launch", 3), o("lanes3", 1), o("steps_per_launch", 0), o("boundary", 1), o("stream3", 0)]),
        "3d box losing and regaining separability": ("box3d1r", F64, (296, 288, 288), [o("separable", 0), o("stream3", 1), o("separable", -1), o("steps_per_launch", 4), w(t3["random27"]), w("own"), o("lanes3", 0)]),
        "2d odd extent: tile kernel, Dirichlet": ("star2d1r", F64, (64, 127), [o("stream", 0), o("steps_per_launch", 2), o("stream", 1), o("steps_per_launch", 2), o("boundary", 1), o("steps_per_launch", 4), o("boundary", 0)]),
        "2d odd extent: Dirichlet first": ("box2d3r", F64, (64, 127), [o("boundary", 1), o("steps_per_launch", 2), o("steps_per_launch", 6), o("boundary", 0)]),
        "2d mfma refuses fusion": ("star2d1r", F64, (64, 128), [o("variant", VARIANT_MFMA), o("steps_per_launch", 2), o("variant", VARIANT_DIRECT), o("steps_per_launch", 2), o("variant", VARIANT_MFMA)]),
        "3d odd extent": ("star3d1r", F64, (216, 216, 215), [o("steps_per_launch", 4), o("steps_per_launch", 2), o("lanes3", 0), o("steps_per_launch", 0), o("boundary", 1)]),
        "3d bf16 depth against variant": ("box3d1r", BF16, (232, 232, 224), [o("steps_per_launch", 4), o("variant", VARIANT_MFMA), o("steps_per_launch", 1), o("steps_per_launch", 0), o("variant", VARIANT_MFMA), o("boundary", 1)]),
        "2d forms of the taps in turn": ("star2d1r", F64, (64, 128), [w(t2["random49"]), w(t2["rank1"]), w("own"), o("lowrank_valu", 4), w(t2["rank1"]), o("lowrank_valu", 0)]),
        "thread defaults": ("box2d3r", F64, (2, 2), [("default_boundary", 2), ("create", (2, 2)), ("create", (64, 128)), ("default_normalize", 1), ("create", (64, 128)), ("default_boundary", 0), ("default_normalize", 0), ("create", (2, 2))]),
    }


SEQUENCES = _sequences()
_STATE_KEYS = ["variant", "steps_per_launch", "fused_eval", "tapset", "boundary"]


def observe_sequence(lib, seq):
    """[status, signature, variant, steps_per_launch, fused_eval, tapset, boundary] after every call of the sequence"""
    shape, dtype, dims, ops = seq
    rc, plan = _create(lib, shape, dtype, dims)
    assert plan is not None, seq
    n = lib.lora_shape_ntaps(SHAPES.index(shape))
    own = (ctypes.c_double * n)()
    assert lib.lora_plan_get_weights(plan, own, n) == 0
    trace = []
    try:
        for op in ops:
            if op[0] == "weights":
                rc = _set_weights(lib, plan, list(own) if op[1] == "own" else op[1])
            elif op[0] == "default_boundary":
                rc = lib.lora_set_default_boundary(op[1])  # (returns the previous value)
            elif op[0] == "default_normalize":
                rc = lib.lora_set_default_normalize(op[1])
            elif op[0] == "create":
                lib.lora_plan_destroy(plan)
                rc, plan = _create(lib, shape, dtype, op[1])
            else:
                rc = _apply(lib, plan, op)
            state = [lib.lora_plan_kernel_signature(plan).decode()] + [_get(lib, plan, k) for k in _STATE_KEYS] if plan else []
            trace.append([rc] + state)
    finally:
        lib.lora_set_default_boundary(0)
        lib.lora_set_default_normalize(0)
        if plan:
            lib.lora_plan_destroy(plan)
    return trace


class Interned:
    """per field: the distinct values in order of first appearance; a record becomes a list of indices"""

    def __init__(self, fields, tables=None):
        self.fields = fields
        self.tables = tables if tables is not None else {f: [] for f in fields}
        self._index = {f: {json.dumps(v): i for i, v in enumerate(self.tables[f])} for f in fields}

    def pack(self, rec):
        row = []
        for f in self.fields:
            if f not in rec:
                row.append(-1)
                continue
            key = json.dumps(rec[f])
            if key not in self._index[f]:
                self._index[f][key] = len(self.tables[f])
                self.tables[f].append(rec[f])
            row.append(self._index[f][key])
        return row

    def unpack(self, row):
        return {f: self.tables[f][i] for f, i in zip(self.fields, row) if i >= 0}


RESOLUTION_FIELDS = ["setup", "signature", "options", "granularity", "padded_bytes", "codes"]


def record(lib):
    it = Interned(RESOLUTION_FIELDS)
    rows = [it.pack(observe_resolution(lib, case)) for _, case in resolution_cases()]
    return {"readable": READABLE, "fields": RESOLUTION_FIELDS, "tables": it.tables, "resolution": rows,
            "validation": {label: observe_validation(lib, case) for label, case in validation_cases()},
            "sequences": {name: observe_sequence(lib, seq) for name, seq in SEQUENCES.items()}}


def load():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def save(data):
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:  # (no timestamp: same bytes)
        f.write((json.dumps(data, separators=(",", ":")) + "\n").encode())


if __name__ == "__main__":
    data = record(library())
    save(data)
    print("%s: %d resolution cases, %d validation entries, %d sequences, %d bytes" % (
        FIXTURE, len(data["resolution"]), len(data["validation"]), len(data["sequences"]), os.path.getsize(FIXTURE)))
