"""What a plan resolves to, pinned through the C ABI alone (no device needed: tests/golden/make_plan_resolution.py).

tests/golden/plan_resolution.json.gz was recorded from the library as it was BEFORE plan resolution moved into
csrc/plan.cpp; the library under test has to reproduce every entry -- kernel, depth, signature, readable options, the
depths its launch entries accept, option validation and the order-dependent traces.  No entry is left out of the
comparison.  The keys that became readable with the option table are checked separately (they are not in the fixture)."""
import glob
import importlib.util
import os
import re

import pytest
from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("make_plan_resolution", os.path.join(GOLDEN, "make_plan_resolution.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

CSRC = os.path.join(ROOT, "lorastencil_amd", "csrc")


@pytest.fixture(scope="module")
def lib(engine_built):
    return G.library()


@pytest.fixture(scope="module")
def golden():
    return G.load()


@pytest.fixture(scope="module")
def recorded(golden):
    """the fixture's resolution records, unpacked, in the order of resolution_cases()"""
    it = G.Interned(golden["fields"], golden["tables"])
    return [it.unpack(row) for row in golden["resolution"]]


def _report(diffs, total):
    return "%d of %d entries differ; the first ones:\n%s" % (len(diffs), total, "\n".join(diffs[:12]))


def test_resolution_matches_the_recorded_library(lib, golden, recorded):
    assert golden["readable"] == G.READABLE and golden["fields"] == G.RESOLUTION_FIELDS
    cases = list(G.resolution_cases())
    assert len(cases) == len(recorded)
    diffs = []
    for (label, case), want in zip(cases, recorded):
        got = G.observe_resolution(lib, case)
        if got != want:
            diffs.append("%s\n   recorded %s\n   now      %s" % (label, want, got))
    assert not diffs, _report(diffs, len(cases))


def test_option_validation_matches_the_recorded_library(lib, golden):
    cases = list(G.validation_cases())
    assert sorted(golden["validation"]) == sorted(label for label, _ in cases)
    diffs = []
    for label, case in cases:
        got, want = G.observe_validation(lib, case), golden["validation"][label]
        if got != want:
            diffs.append("%s: recorded %s, now %s" % (label, want, got))
    assert not diffs, _report(diffs, len(cases))


def test_set_call_sequences_match_the_recorded_library(lib, golden):
    assert sorted(golden["sequences"]) == sorted(G.SEQUENCES)
    for name, seq in G.SEQUENCES.items():
        got, want = G.observe_sequence(lib, seq), golden["sequences"][name]
        assert got == want, name


# ---- the fixture reaches every resolved form -----------------------------------------------------------------------

def _signatures(recorded):
    return {r["signature"] for r in recorded if "signature" in r}


def test_fixture_names_every_kernel(recorded):
    """every name a kernel_name_* function of csrc/ can return is some case's kernel"""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        text = open(path).read()
        for body in re.findall(r"const char \*kernel_name_\w+\(const Plan &\w*\)\s*\{(.*?)\n?\}", text, flags=re.S):
            names.update(re.findall(r'"(stencil\w+)"', body))
    assert len(names) >= 17, names
    seen = {s.split("[")[0] for s in _signatures(recorded)}
    assert names <= seen, names - seen


def test_fixture_reaches_every_fused_eval(recorded, golden):
    col = golden["readable"].index("fused_eval")
    assert {r["options"][col] for r in recorded if "options" in r} >= set(range(8))


def test_fixture_reaches_every_plane_kernel_instantiation(recorded):
    """every (K, waves, pipe) row of the plane-streaming kernel's LORA_S3 list, and the barrier-free form at 8 and 4 waves
    with two and three applications"""
    text = open(os.path.join(CSRC, "kernels_3d_planes.hip")).read()
    rows = {(int(k), int(w), int(p)) for k, w, _, p in re.findall(r"^\s*LORA_S3\((\d+), (\d+), (\d+), (\d+)\)", text, flags=re.M)}
    assert len(rows) == 5, rows
    seen, seen_async = set(), set()
    for s in _signatures(recorded):
        if not s.startswith("stencil3d_planes_kernel["):
            continue
        f = dict(kv.split("=") for kv in s[s.index("[") + 1:-1].split(","))
        if "async" in f:
            seen_async.add((int(f["k"]), int(f["waves"])))
        else:
            assert f["slots"] == "2"
            seen.add((int(f["k"]), int(f["waves"]), int(f["pipe"])))
    assert rows <= seen, rows - seen
    assert seen_async == {(2, 8), (2, 4), (3, 8), (3, 4)}


# ---- keys that lora_plan_set_option took but lora_plan_get_option did not answer before the option table ----------

NEWLY_READABLE = {"wg": [0, 1, -1], "wg_rows": [0, 64, 1 << 20], "wg_prio": [0, 24, 12], "wg_edge_pct": [-1, 0, 100],
                  "stream_share": [1, 0], "stream_prefetch": [1, 0], "scratch": [0, 1, -1], "mfma_split": [0, 1],
                  "lanes3": [0, 1, -1]}
FLAG_KEYS = {"nt_store", "persistent", "stream", "stream3_async", "stream3_pipe", "stream_share", "stream_prefetch", "mfma_split",
             "lds_dma", "fused_pipeline", "torus"}  # any non-zero value sets them to 1


def test_every_settable_key_is_readable(lib, golden):
    """set, then get, round-trips for every settable key (flags read back as 0 / 1); `ablate` stays refused in the shipped
    library; the read-only keys refuse a set"""
    for key in G.SETTABLE:
        assert key in G.READABLE or key in NEWLY_READABLE or key in ("ablate", "no_such_option"), key
    shape, dtype, dims = G.VALIDATION_PLANS[1]
    for key, values in NEWLY_READABLE.items():
        rc, plan = G._create(lib, shape, dtype, dims)
        assert rc == 0
        try:
            for v in values:
                assert lib.lora_plan_set_option(plan, key.encode(), v) == 0, (key, v)
                assert G._get(lib, plan, key) == v, (key, v)
            if key in FLAG_KEYS:
                assert lib.lora_plan_set_option(plan, key.encode(), 7) == 0 and G._get(lib, plan, key) == 1
        finally:
            lib.lora_plan_destroy(plan)
    # every accepted set of the validation list reads back (requested value, or the resolved one where the key says so)
    for label, (shape, dtype, dims, key, value) in G.validation_cases():
        if golden["validation"][label]["status"] != 0:
            continue
        rc, plan = G._create(lib, shape, dtype, dims)
        try:
            assert lib.lora_plan_set_option(plan, key.encode(), value) == 0
            got = G._get(lib, plan, key)
            assert got is not None, label
            if key not in ("steps_per_launch", "fused_rows"):  # these two read the RESOLVED value
                assert got == (int(value != 0) if key in FLAG_KEYS else value), label
        finally:
            lib.lora_plan_destroy(plan)
    rc, plan = G._create(lib, shape, dtype, dims)
    try:
        for key in ("tapset", "variant", "fused_eval", "boundary"):
            assert lib.lora_plan_set_option(plan, key.encode(), 0) == -1
            assert G._get(lib, plan, key) is not None
        assert lib.lora_plan_set_option(plan, b"ablate", 1) == -1 and G._get(lib, plan, "ablate") is None
    finally:
        lib.lora_plan_destroy(plan)
