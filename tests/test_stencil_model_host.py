"""Host tests of tests/stencil_model.py, the exact integer yardstick of tests/test_gpu_tap_orientation.py.  No GPU.

1. The model's orientation -- which neighbour ``w[t]`` multiplies -- is the CPU oracle's, bit for bit, for all eight shapes.  The
   oracle is tied to the reference's own test_cpu by tests/test_oracle.py; if the two disagreed here, the model would be wrong.
2. The fingerprint tables have teeth: on the GPU tests' own data, every signed axis permutation of a table and every
   transposition of two taps of its support changes the model's output, on the whole grid and on a region of two, and the GPU
   tests' comparison rejects the changed output.
   2b. The same for tests/test_gpu_multisweep_taps.py: its K-application model (``levels``: the contract of lora_plan_stepk) and its
   periodic model are the oracle's drivers bit for bit, whole padded buffer; its tables (ranked, mod-7, separable) are asymmetric,
   hold the equal pairs their docstrings state, stay exact at the depth they run at, and every mirrored, transposed or swapped
   table changes level K; the bf16 oracle has the model's orientation on the separable table.
3. Negative control, and the record of why these files exist: the tap tables of the existing chain tests are blind to the
   symmetries and hold the equal pairs pinned below.
"""
import itertools

import numpy as np
import pytest

import stencil_model as SM
import test_gpu_cg
import test_gpu_multisweep_taps as MS
import test_gpu_pcg
import test_gpu_residual
import test_gpu_tap_orientation as T
from conftest import ALL_SHAPES

ANCHOR_DIMS = {1: (37,), 2: (9, 14), 3: (5, 6, 10)}  # small and ragged: no two extents equal


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


@pytest.fixture(scope="module")
def O(engine_built):
    from oracle import oracle

    return oracle


def tables(O, shape):
    """[(form, integer table)] of a shape: "direct" on the support of the shape's own taps, and "sep" for the 27-tap box"""
    support = O.effective_weights(shape) != 0
    out = [("direct", SM.fingerprint_taps(support, "direct"))]
    if shape == "box3d1r":
        out.append(("sep", SM.fingerprint_taps(support, "sep")))
    return out


# ---- 1. the orientation is the oracle's --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_the_model_is_the_oracle_bit_for_bit(O, shape):
    nd = SM.ndim_of(shape)
    dims = ANCHOR_DIMS[nd]
    assert SM.padded_shape(shape, dims) == tuple(O.padded_shape(shape, dims)) and SM.HALO[nd] == tuple(O.halo(shape))
    u, _, _ = SM.data(shape, dims, SM.seed_of("anchor", shape))
    for form, w in tables(O, shape):
        SM.assert_exact(f"{shape} {form}", [SM.magnitude(shape, u, w)])
        out = O.step(shape, np.array(u), w.astype(np.float64))
        want = SM.apply(shape, u, w)
        assert SM.exactly(O.interior(shape, out).copy(), want), f"{shape} {form}: the model and the oracle disagree: the model is wrong"
        halo = out.copy()
        O.interior(shape, halo)[...] = 0.0
        assert not halo.any()
        # and the model would notice the other orientation: the point-reflected table gives another result
        nd_flip = SM.transform(w, tuple(range(nd)), (1,) * nd)
        assert not SM.exactly(O.interior(shape, out).copy(), SM.apply(shape, u, nd_flip))


def test_the_table_layout_is_the_one_of_the_other_models(O):
    """tests/test_gpu_pcg.py's tap_offsets (copied into the model) and its model_sweep, which tests/test_gpu_coarse1.py's CG model
    is built on, point the same way"""
    for nd, shape in ((2, "box2d3r"), (3, "box3d1r")):
        assert SM.tap_offsets(nd) == test_gpu_pcg.tap_offsets(nd)
        for _, w in tables(O, shape):
            x = np.random.default_rng(nd).integers(-50, 50, ANCHOR_DIMS[nd])
            got = test_gpu_pcg.model_sweep(w.astype(np.float64), x.astype(np.float64))
            assert SM.exactly(got, SM.apply_zero_halo(shape, x, w))
    assert SM.tap_offsets(1) == test_gpu_pcg.tap_offsets(1)


# ---- 2. the tables have teeth ---------------------------------------------------------------------------------------------------------
def mutations(w, support):
    """(name, table) for every non-identity signed axis permutation that keeps the table's shape and every transposition of
    two taps of the support"""
    nd = {9: 1, 49: 2, 27: 3}[w.size]
    for perm, flips in SM.signed_permutations(nd):
        tw = SM.transform(w, perm, flips)
        if tw is not None:
            yield f"axes {perm} mirrored {flips}", tw
    for i, j in itertools.combinations(np.flatnonzero(support), 2):
        tw = w.copy()
        tw[i], tw[j] = w[j], w[i]
        yield f"taps {i} and {j} swapped", tw


TEETH = [c for c in T.SWEEPS if c[2] in ((1027,), (33, 130), (34, 18, 130)) and c[1] != "sep0"]  # the smallest multi-tile case per dimension
TWO = {(1027,): (510, 512), (33, 130): (5, 7), (34, 18, 130): (3, 5)}


@pytest.mark.parametrize("shape,form,dims,regions", TEETH, ids=T.ids(TEETH))
def test_every_mirrored_transposed_or_swapped_table_changes_the_output(O, shape, form, dims, regions):
    u, f, _ = T.model_data(shape, dims)
    support = O.effective_weights(shape) != 0
    w = SM.fingerprint_taps(support, "sep" if form == "sep" else "direct")
    base = SM.source(shape, u, w, f, 0, None)
    lo, hi = TWO[dims]
    count = 0
    for name, tw in mutations(w, support):
        assert not np.array_equal(tw, w)
        delta = SM.apply(shape, u, tw - w)  # S is linear in the taps: the changed output is base + delta
        assert delta.any(), f"{shape} {form} {dims}: {name} leaves the whole output unchanged"
        assert delta[lo:hi].any(), f"{shape} {form} {dims}: {name} leaves the region [{lo}, {hi}) unchanged"
        wrong = (base + delta).astype(np.float64)
        assert not SM.exactly(wrong, base) and not SM.exactly(wrong[lo:hi], base[lo:hi]), name
        count += 1
    n = int(support.sum())
    assert count >= n * (n - 1) // 2 + 1
    # the linearity the loop above leans on, checked once through the model itself
    name, tw = next(iter(mutations(w, support)))
    assert np.array_equal(SM.source(shape, u, tw, f, 0, None), base + SM.apply(shape, u, tw - w))
    assert SM.exactly(base.astype(np.float64), base)


@pytest.mark.parametrize("shape,form,dims", T.CG_SMALL, ids=T.ids(T.CG_SMALL))
def test_the_cg_small_start_has_teeth_and_a_positive_curvature(O, shape, form, dims):
    if form == "sep0":
        form = "direct"
    support = O.effective_weights(shape) != 0
    w = SM.fingerprint_taps(support, form)
    x0, r0 = SM.cg_start(shape, dims, w, SM.seed_of("cg_small", shape, form, dims))
    assert x0.shape == r0.shape == tuple(dims) and np.abs(r0).max() == 40
    for sigma, tau in ((1, 1), (T.SIGMA, T.TAU)):
        q = SM.shifted(shape, SM.with_halo(shape, r0, 0), w, sigma, tau, 0, None)
        assert SM.dot_record(r0, q)[0] > 0
    for name, tw in mutations(w, support):
        assert SM.apply_zero_halo(shape, r0, tw - w).any(), f"{shape} {form} {dims}: {name} leaves q = A r0 unchanged"


def test_fingerprint_taps_refuse_blind_tables():
    assert SM.fingerprint_taps(np.ones(49, bool)).sum() == 1225 and SM.fingerprint_taps(np.ones(49, bool)).max() == 49
    sep = SM.fingerprint_taps(np.ones(27, bool), "sep")
    assert sep.max() == 273 and sep.sum() == 1950 and len(set(sep)) == 27
    with pytest.raises(AssertionError):
        SM.fingerprint_taps(np.ones(27, bool)[:13], "sep")
    with pytest.raises(AssertionError):
        SM.assert_exact("too big", [2 ** 53])
    assert SM.assert_exact("fits", [np.array([-5, 3]), 2 ** 53 - 1]) == 2 ** 53 - 1


# ---- 2b. the K-application contract and the tables that stay exact at depth (tests/test_gpu_multisweep_taps.py) -----------------------
# (shape, table, the deepest launch the GPU tests run it at, equal pairs, tap sum)
DEEP = [("1d1r", "ranked", 8, 0, 28), ("1d2r", "ranked", 8, 0, 45), ("star2d1r", "ranked", 6, 0, 325), ("star2d3r", "ranked", 6, 0, 91),
        ("box2d3r", "ranked", 4, 0, 1225), ("box2d3r", "mod7", 6, 147, 196), ("star3d1r", "ranked", 4, 0, 28),
        ("box3d1r", "ranked", 3, 0, 378), ("box3d1r", "sepk", 4, 0, 3072)]
DEEP_IDS = [f"{s}-{t}" for s, t, _, _, _ in DEEP]
SMALL = {1: (2051,), 2: (7, 13), 3: (3, 5, 7)}  # grids of the GPU tests' own cases


def deep_table(L, shape, tname):
    w = MS.table(L, shape, tname)
    return w, L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0 if tname == "ranked" else np.ones(w.size, bool)


@pytest.mark.parametrize("shape,tname,depth,pairs,total", DEEP, ids=DEEP_IDS)
def test_the_deep_tables_are_asymmetric_and_exact(L, shape, tname, depth, pairs, total):
    w, support = deep_table(L, shape, tname)
    assert SM.invariant_symmetries(w) == [] and SM.equal_pairs(w, support) == pairs and int(w.sum()) == total
    assert not w[~support].any() and (w[support] > 0).all()
    top = MS.top_of(w, depth)
    assert top * total ** depth < SM.EXACT and (top == 9 or (top + 1) * total ** depth >= SM.EXACT)
    if tname == "sepk":
        c, b, a = L.separable_3x3x3(w.astype(np.float64))  # the engine's exact rank-1 test takes the table and reads these factors
        assert (c.tolist(), b.tolist(), a.tolist()) == ([88.0, 64.0, 104.0], [1.25, 1.0, 1.75], [0.5, 1.0, 1.5])
        assert L.separable_3x3x3(SM.fingerprint_taps(np.ones(27, bool), "sep").astype(np.float64)) is None  # (it refuses SEP_FACTORS)
    with pytest.raises(AssertionError):
        MS.top_of(w, 40)


@pytest.mark.parametrize("shape,tname,depth,pairs,total", DEEP, ids=DEEP_IDS)
def test_the_k_level_model_is_the_oracle_bit_for_bit(O, L, shape, tname, depth, pairs, total):
    """lora_plan_stepk's contract is "the state the step-by-step driver would leave": the oracle's driver, K sweeps from an even
    level, WHOLE padded buffer (level K with the halo the contract gives it), under the reference and the Dirichlet rule; and
    the rolled periodic model against the oracle's periodic driver."""
    nd = SM.ndim_of(shape)
    dims = ANCHOR_DIMS[nd]
    w, _ = deep_table(L, shape, tname)
    top = MS.top_of(w, depth)
    u = SM.data_small(shape, dims, SM.seed_of("anchor K", shape, tname), top)
    wf = w.astype(np.float64)
    for K in range(1, depth + 1):
        for dirichlet in (False, True):
            SM.assert_exact(f"{shape} {tname} K = {K}", SM.levels_magnitude(shape, u, w, K, dirichlet))
            want = SM.levels(shape, u, w, K, dirichlet)
            assert np.array_equal(SM.interior(shape, want)[1:3], SM.stepn(shape, u, w, K, 1, 3, dirichlet))
            got = O.run_bc(shape, np.array(u), K, "dirichlet", weights=wf) if dirichlet else O.run(shape, np.array(u), K, weights=wf)
            if nd == 1:  # the 1D driver copies back all but the last element of the padded array (oracle/lorastencil_oracle.h): a halo cell
                got, want = got[:-1], want[:-1]
            assert SM.exactly(got, want), f"{shape} {tname} K = {K} dirichlet = {dirichlet}: the model and the oracle disagree"
        SM.assert_exact(f"{shape} {tname} periodic {K}", SM.periodic_magnitude(shape, u, w, K))
        got = O.interior(shape, O.run_bc(shape, np.array(u), K, "periodic", weights=wf)).copy()
        assert SM.exactly(got, SM.periodic(shape, u, w, K)), f"{shape} {tname} K = {K}: the periodic model and the oracle disagree"
    # the long-double model of the depths without an exact table is the same model: equal to the integers where those are exact
    assert np.array_equal(SM.levels_real(shape, u, wf, depth).astype(np.float64), SM.stepn(shape, u, w, depth, 0, None).astype(np.float64))
    assert np.array_equal(SM.levels_real(shape, u, wf, depth, True).astype(np.float64), SM.stepn(shape, u, w, depth, 0, None, True).astype(np.float64))


@pytest.mark.parametrize("shape,tname,depth,pairs,total", DEEP, ids=DEEP_IDS)
def test_every_mirrored_transposed_or_swapped_table_changes_the_k_level_output(L, shape, tname, depth, pairs, total):
    """On the GPU tests' own data (their smallest grid with every extent above one), at the deepest launch the table runs at:
    every signed axis permutation (under both halo rules) and every transposition of two UNEQUAL taps (under the reference
    rule) changes level K, on the whole grid and on a region of two -- and the GPU tests' comparison rejects the changed output."""
    nd = SM.ndim_of(shape)
    dims = SMALL[nd]
    assert any(c[1] == shape and c[3] == dims for c in MS.CASES)
    w, support = deep_table(L, shape, tname)
    top = MS.top_of(w, depth)
    u = MS.data(shape, dims, top)
    lo, hi = (510, 512) if nd == 1 else (1, 3)
    count = 0
    for dirichlet in (False, True):
        base = SM.stepn(shape, u, w, depth, 0, None, dirichlet)
        for name, tw in mutations(w, support):
            if np.array_equal(tw, w):  # a swap of two equal taps (the mod-7 table has 147): not a mutation
                continue
            if dirichlet and name.startswith("taps"):  # (the transpositions under the reference rule only: time)
                continue
            wrong = SM.stepn(shape, u, tw, depth, 0, None, dirichlet)
            assert (wrong != base).any(), f"{shape} {tname} {dims}: {name} leaves level {depth} unchanged"
            assert (wrong[lo:hi] != base[lo:hi]).any(), f"{shape} {tname} {dims}: {name} leaves [{lo}, {hi}) of level {depth} unchanged"
            assert not SM.exactly(wrong.astype(np.float64), base) and not SM.exactly(wrong[lo:hi].astype(np.float64), base[lo:hi]), name
            count += 1
    n = int(support.sum())
    assert count >= n * (n - 1) // 2 - pairs + 2


def bf16_nearest_even(x):
    """float64 values -> bf16 bit patterns, round to nearest even, in numpy (finite values that fp32 holds exactly)"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x)
    bits = f.view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def test_the_bf16_oracle_has_the_models_orientation_on_the_separable_table(O):
    """One sweep of sep_k_taps / 4096 on data 0 .. 3: every product and partial sum is an integer below 2**24 over 4096 --
    exact in fp32 in any order -- so the oracle's bf16 sweep, in both of its summation orders, must be the model's integers over
    4096 rounded once to the nearest even bf16."""
    shape = "box3d1r"
    wi = SM.sep_k_taps()
    w = MS.bf16_taps()
    assert np.array_equal(w * 4096.0, wi.astype(np.float64))
    for dims, _ in MS.GRIDS_BF16:
        u = MS.data(shape, dims, 3)
        assert SM.assert_exact("bf16 anchor", [SM.magnitude(shape, u, wi)]) < 2 ** 24
        bits = O.to_bf16(u)
        assert np.array_equal(O.from_bf16(bits), u)
        want = bf16_nearest_even(SM.apply(shape, u, wi).astype(np.float64) / 4096.0)
        mirrored = bf16_nearest_even(SM.apply(shape, u, SM.transform(wi, (0, 1, 2), (0, 0, 1))).astype(np.float64) / 4096.0)
        assert not np.array_equal(mirrored, want)
        for separable in (True, False):
            got = O.interior(shape, O.run_bf16(shape, bits, 1, weights=w, separable=separable))
            assert np.array_equal(got, want), f"{dims} separable = {separable}: the bf16 oracle and the model disagree"


# ---- 3. negative control: what the existing tables cannot see ---------------------------------------------------------------------
ID1, ID2, ID3 = (0,), (0, 1), (0, 1, 2)
MIRROR_1D = [(ID1, (1,))]
TRANSPOSE_2D = [((1, 0), (0, 0))]
POINT_2D = [(ID2, (1, 1))]
SQUARE = [(p, f) for p in (ID2, (1, 0)) for f in itertools.product((0, 1), repeat=2) if p != ID2 or any(f)]  # the 7 of the square
YZ = [(p, f + (0,)) for p, f in [((0, 1, 2), fl) for fl in itertools.product((0, 1), repeat=2) if any(fl)]
      + [((1, 0, 2), fl) for fl in itertools.product((0, 1), repeat=2)]]  # z mirror, y mirror, z <-> y: 7, x untouched
YZ_AND_X = [(p, f) for p in (ID3, (1, 0, 2)) for f in itertools.product((0, 1), repeat=3) if p != ID3 or any(f)]  # every mirror, z <-> y: 15
POINT_3D = [(ID3, (1, 1, 1))]
# shape: (blind spots of 1 + arange % 3, its equal pairs, blind spots of symmetric_taps, its equal pairs, pairs in all)
BLIND = {
    "1d1r": ([], 5, MIRROR_1D, 5, 21),
    "1d2r": ([], 9, MIRROR_1D, 10, 36),
    "star2d1r": (TRANSPOSE_2D, 97, POINT_2D, 98, 300),
    "star2d3r": (TRANSPOSE_2D, 22, SQUARE, 22, 78),
    "box2d3r": (TRANSPOSE_2D, 376, POINT_2D, 376, 1176),
    "star3d1r": (YZ, 10, YZ_AND_X, 11, 21),
    "box3d1r": (YZ, 108, POINT_3D, 109, 351),
}


@pytest.mark.parametrize("shape", sorted(BLIND))
def test_what_the_existing_tap_tables_cannot_see(L, shape):
    """axes are listed outermost first: (z, y, x) in 3D, (y, x) in 2D; ((1, 0), (0, 0)) is the x <-> y transposition"""
    arange_blind, arange_pairs, sym_blind, sym_pairs, pairs = BLIND[shape]
    support = L.effective_weights(shape)[:L.ops.ntaps(shape)] != 0
    n = int(support.sum())
    assert n * (n - 1) // 2 == pairs
    first = test_gpu_residual.integer_taps(L, shape, "f64", "")
    assert np.array_equal(first, np.where(support, 1.0 + np.arange(support.size) % 3, 0.0))
    second = test_gpu_cg.symmetric_taps(L, shape, "int")
    assert sorted(SM.invariant_symmetries(first)) == sorted(arange_blind) and SM.equal_pairs(first, support) == arange_pairs
    assert sorted(SM.invariant_symmetries(second)) == sorted(sym_blind) and SM.equal_pairs(second, support) == sym_pairs
    # the fingerprint of the same support: nothing left
    mine = SM.fingerprint_taps(support)
    assert SM.invariant_symmetries(mine) == [] and SM.equal_pairs(mine, support) == 0
