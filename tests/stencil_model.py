"""An exact integer model of the stencil, of the single-launch entries built on it and of the launches of K applications -- the
yardstick of tests/test_gpu_tap_orientation.py and tests/test_gpu_multisweep_taps.py, checked on the CPU by
tests/test_stencil_model_host.py.

Why it exists.  The solver-side kernels are tested by a chain: kernel == ``plan.step_region`` plus one numpy operation, bit for
bit.  The chain's tap tables (``1 + arange % 3`` and ``1 + min(t, n - 1 - t) % 3`` on the shape's support) are invariant under
transpositions, mirrors or point reflection of the table and hold many equal pairs, so a kernel whose offset table is transposed
or mirrored passes.  Here every tap of the support is a different positive integer and no signed axis permutation maps the table
to itself (``fingerprint_taps`` asserts both), the data are small integers, and every quantity stays below 2**53
(``assert_exact``), so the engine's fp64 results are exact whatever its summation order and are compared with ``==``.

The model shares no code with the engine and none with oracle/: ``apply`` is a sum of shifted slices of the whole padded array
in int64.  tests/test_stencil_model_host.py anchors its orientation -- which neighbour ``w[t]`` multiplies -- to the CPU oracle.

Not a conftest.py and no fixtures: a plain module the test files import.
"""
import itertools
import zlib

import numpy as np

HALO = {1: (4,), 2: (4, 4), 3: (1, 2, 4)}       # padded layout per dimension: cells of halo on each side
TABLE = {1: (9,), 2: (7, 7), 3: (3, 3, 3)}      # the tap table per dimension, row-major, outermost axis first
EXACT = 2 ** 53


def ndim_of(shape):
    return int(shape[shape.index("d") - 1])


def tap_offsets(ndim):
    """offset of tap t per axis, outermost first (the table of tests/test_gpu_pcg.py)"""
    if ndim == 1:
        return [(t - 4,) for t in range(9)]
    if ndim == 2:
        return [(t // 7 - 3, t % 7 - 3) for t in range(49)]
    return [(t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1) for t in range(27)]


# ---- tap tables and their symmetries ---------------------------------------------------------------------------------------------
def signed_permutations(ndim):
    """every non-identity (perm, flips): transpose the table by perm, then mirror the axes whose flip is 1"""
    ident = tuple(range(ndim))
    return [(perm, flips) for perm in itertools.permutations(range(ndim)) for flips in itertools.product((0, 1), repeat=ndim)
            if perm != ident or any(flips)]


def transform(w, perm, flips):
    """the flat table w under one signed axis permutation, or None if the transposed table has another shape"""
    w = np.asarray(w)
    nd = {9: 1, 49: 2, 27: 3}[w.size]
    t = np.transpose(w.reshape(TABLE[nd]), perm)
    if t.shape != TABLE[nd]:
        return None
    return np.flip(t, [a for a, f in enumerate(flips) if f]).ravel().copy()


def invariant_symmetries(w):
    """the non-identity signed axis permutations that map the table to itself: what a test on these taps cannot see"""
    w = np.asarray(w)
    nd = {9: 1, 49: 2, 27: 3}[w.size]
    return [(perm, flips) for perm, flips in signed_permutations(nd)
            if (tw := transform(w, perm, flips)) is not None and np.array_equal(tw, w)]


def equal_pairs(w, support):
    """how many pairs of taps of the support hold equal values (swapping such a pair is invisible)"""
    vals = np.asarray(w)[np.asarray(support, dtype=bool)]
    _, counts = np.unique(vals, return_counts=True)
    return int((counts * (counts - 1) // 2).sum())


SEP_FACTORS = ((1, 2, 3), (1, 5, 7), (1, 11, 13))  # a (z), b (y), c (x)


def fingerprint_taps(support, form="direct"):
    """positive integer taps on `support` (a boolean table, flat), pairwise distinct, no symmetry of the table left:
    "direct" = 1 + t; "sep" (the full 27-tap box only) = a (x) b (x) c over z, y, x: an outer product whose 27 entries differ,
    the largest 273, their sum 1950"""
    support = np.asarray(support, dtype=bool).ravel()
    if form == "direct":
        w = np.where(support, 1 + np.arange(support.size), 0).astype(np.int64)
    elif form == "sep":
        assert support.size == 27 and support.all(), "the separable form is a table of the whole 27-tap box"
        a, b, c = (np.array(v, dtype=np.int64) for v in SEP_FACTORS)
        w = np.einsum("i,j,k->ijk", a, b, c).ravel()
        assert w.max() == 273 and w.sum() == 1950
    else:
        raise ValueError(form)
    assert (w[support] > 0).all() and not w[~support].any()
    assert equal_pairs(w, support) == 0, "two taps of the support are equal"
    assert invariant_symmetries(w) == [], "a signed axis permutation maps the table to itself"
    return w


# ---- tables that stay exact at depth K (tests/test_gpu_multisweep_taps.py) -------------------------------------------------------
# A launch of K applications grows the data by (tap sum)**K, and `1 + t` on the 49-tap box (sum 1225) passes 2**53 beyond K = 4.
SEP_K = ((1, 2, 3), (5, 4, 7), (11, 8, 13))  # a (z), b (y), c (x): the centre entries are powers of two


def ranked_taps(support):
    """the values 1 .. n on the n cells of `support` (a boolean table, flat) in row-major order: pairwise distinct (0 equal
    pairs), no symmetry of the table left.  Tap sums: 1d1r 6, 1d2r 15, diamond (star2d1r) 325, star2d3r 91, the 3D star 28,
    the 27-tap box 378, the 49-tap box 1225 (there it is `1 + t`)."""
    support = np.asarray(support, dtype=bool).ravel()
    w = np.zeros(support.size, dtype=np.int64)
    w[support] = 1 + np.arange(int(support.sum()))
    assert equal_pairs(w, support) == 0, "two taps of the support are equal"
    assert invariant_symmetries(w) == [], "a signed axis permutation maps the table to itself"
    return w


def mod7_taps():
    """the 49-tap box at K = 6: 1 + (i + 3 j) % 7, i the row and j the column of the table.  Every row and every column holds
    1 .. 7 once: sum 196 (196**6 * 9 < 2**53), no symmetry of the table left, but 147 equal pairs of the 1176 -- a swap of
    two equal taps is invisible here and shows at K = 4 and 2, where the same kernel runs `1 + t`."""
    i, j = np.divmod(np.arange(49), 7)
    w = (1 + (i + 3 * j) % 7).astype(np.int64)
    assert w.sum() == 196 and equal_pairs(w, np.ones(49, bool)) == 147
    assert invariant_symmetries(w) == [], "a signed axis permutation maps the table to itself"
    return w


def sep_k_taps():
    """the 27-tap box as a (x) b (x) c = (1, 2, 3) (x) (5, 4, 7) (x) (11, 8, 13) over z, y, x.  The engine's exact rank-1 test
    reads the factors back through the centre tap, 2 * 4 * 8 = 64: divisions by a power of two, so it accepts this table
    (c = (88, 64, 104), b = (1.25, 1, 1.75), a = (0.5, 1, 1.5)) where it refuses SEP_FACTORS.  27 distinct entries (0 equal
    pairs), sum 6 * 16 * 32 = 3072, no symmetry left; 3072**4 * 9 < 2**53."""
    a, b, c = (np.array(v, dtype=np.int64) for v in SEP_K)
    w = np.einsum("i,j,k->ijk", a, b, c).ravel()
    assert w.sum() == 3072 and equal_pairs(w, np.ones(27, bool)) == 0
    assert invariant_symmetries(w) == [], "a signed axis permutation maps the table to itself"
    return w


# ---- the stencil ---------------------------------------------------------------------------------------------------------------------
def ints(a):
    """an array of integer values as int64 (a float array must hold integers exactly)"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        assert np.isfinite(a).all() and np.array_equal(a, np.rint(a)), "the model takes integer data"
        assert np.abs(a).max(initial=0) < EXACT
    return a.astype(np.int64)


def interior(shape, a):
    h = HALO[ndim_of(shape)]
    return a[tuple(slice(k, n - k) for k, n in zip(h, a.shape))]


def padded_shape(shape, dims):
    return tuple(n + 2 * k for n, k in zip(dims, HALO[ndim_of(shape)]))


def apply(shape, u_padded, w):
    """S(u) on the interior: out[i] = sum_t w[t] u[i + offset(t)], from shifted slices of the whole padded array (the halo takes
    part: the stencil reads it).  int64."""
    nd = ndim_of(shape)
    u, w = ints(u_padded), ints(w).ravel()
    h, offs = HALO[nd], tap_offsets(nd)
    assert u.ndim == nd and w.size == len(offs)
    dims = tuple(n - 2 * k for n, k in zip(u.shape, h))
    out = np.zeros(dims, dtype=np.int64)
    for t, d in enumerate(offs):
        if w[t]:
            assert all(abs(x) <= k for x, k in zip(d, h))
            out += w[t] * u[tuple(slice(k + x, k + x + n) for k, x, n in zip(h, d, dims))]
    return out


def with_halo(shape, inner, halo=0):
    """a padded int64 array with the given interior; `halo` a number or a padded array to take the halo cells from"""
    inner = ints(inner)
    a = ints(halo).copy() if isinstance(halo, np.ndarray) else np.full(padded_shape(shape, inner.shape), int(halo), dtype=np.int64)
    interior(shape, a)[...] = inner
    return a


def apply_zero_halo(shape, inner, w):
    """S of an interior array inside a zero halo (lora_plan_cg_small's operator)"""
    return apply(shape, with_halo(shape, inner, 0), w)


def _f(shape, f):
    """the interior of a padded source (its halo may hold NaN: it is never used), 0 for None"""
    return 0 if f is None else ints(interior(shape, np.asarray(f)))


# ---- the single-launch entries, each on the outermost range [begin, end) ------------------------------------------------------------
def source(shape, u, w, f, begin, end):
    """S(u) + f"""
    return (apply(shape, u, w) + _f(shape, f))[begin:end]


def leapfrog(shape, cur, prev, w, f, a, c, begin, end):
    """a (S(cur) + f) + c prev"""
    return (a * (apply(shape, cur, w) + _f(shape, f)) + c * interior(shape, ints(prev)))[begin:end]


def defect(shape, u, w, f, begin, end):
    """S(u) + f - u"""
    return (apply(shape, u, w) + _f(shape, f) - interior(shape, ints(u)))[begin:end]


def shifted(shape, p, w, sigma, tau, begin, end):
    """sigma p - tau S(p)"""
    return (sigma * interior(shape, ints(p)) - tau * apply(shape, p, w))[begin:end]


def theta_r(shape, u, w, f, tau, begin, end):
    """tau (S(u) + f - u)"""
    return tau * defect(shape, u, w, f, begin, end)


def source2(shape, u, w, f, begin, end):
    """lora_plan_step2_region with a source: level 1 = S(u) + f on the WHOLE interior inside a halo of zeros (the intermediate
    level's halo cells are taken as 0; the source adds to interior cells only), the result S(level 1) + f on [begin, end)"""
    level1 = with_halo(shape, source(shape, u, w, f, 0, None), 0)
    return source(shape, level1, w, f, begin, end)


def levels(shape, u, w, K, dirichlet=False):
    """The contract of lora_plan_stepk / lora_plan_stepn_region (include/lorastencil.h), which generalises source2 without a
    source: level 0 is the source buffer; level k = S(level k - 1) on the WHOLE interior; the halo cells of level k are 0 at
    odd k and the source buffer's at even k (the state the step-by-step driver leaves), under the Dirichlet option the source
    buffer's at every level.  Returns level K as a padded int64 array."""
    src = ints(u)
    level = src
    for k in range(1, K + 1):
        level = with_halo(shape, apply(shape, level, w), src if dirichlet or k % 2 == 0 else 0)
    return level


def stepn(shape, u, w, K, begin, end, dirichlet=False):
    """K applications in one launch: the interior of level K on the outermost range [begin, end)"""
    return interior(shape, levels(shape, u, w, K, dirichlet))[begin:end]


def levels_real(shape, u, w, K, dirichlet=False):
    """`levels` for real data and taps, evaluated in np.longdouble (the depths no integer table keeps exact): the same shifted
    slices, the same halo rule.  Returns the interior of level K."""
    nd = ndim_of(shape)
    LD = np.longdouble
    src, w = np.asarray(u).astype(LD), np.asarray(w).astype(LD).ravel()
    h, offs = HALO[nd], tap_offsets(nd)
    dims = tuple(n - 2 * k for n, k in zip(src.shape, h))
    level = src
    for k in range(1, K + 1):
        out = np.zeros(dims, dtype=LD)
        for t, d in enumerate(offs):
            if w[t]:
                out += w[t] * level[tuple(slice(q + x, q + x + n) for q, x, n in zip(h, d, dims))]
        level = src.copy() if dirichlet or k % 2 == 0 else np.zeros_like(src)
        interior(shape, level)[...] = out
    return interior(shape, level)


def apply_periodic(shape, inner, w):
    """S on a torus: out[i] = sum_t w[t] inner[(i + offset(t)) mod dims], by np.roll of the interior array (no halo takes
    part; shares nothing with `apply`).  Keeps the dtype of `inner` unless it is an integer array (then int64)."""
    nd = ndim_of(shape)
    inner = np.asarray(inner)
    if inner.dtype.kind in "iu":
        inner = inner.astype(np.int64)
    w = np.asarray(w).ravel()
    out = np.zeros_like(inner)
    for t, d in enumerate(tap_offsets(nd)):
        if w[t]:
            out = out + w[t] * np.roll(inner, tuple(-x for x in d), axis=tuple(range(nd)))
    return out


def periodic(shape, u, w, times):
    """`times` sweeps under the periodic boundary: the interior after them (the halo of u is never used)"""
    level = interior(shape, ints(u))
    for _ in range(times):
        level = apply_periodic(shape, level, ints(w))
    return level


def leapfrog2(shape, prev, cur, w, f, a1, c1, a2, c2, begin, end):
    """lora_plan_step2_leapfrog[_src]: out1 = a1 (S(cur) + f) + c1 prev; level 1 is out1 on the WHOLE interior with the values
    `prev` holds outside the interior; out2 = a2 (S(level 1) + f) + c2 cur.  Returns (out1, out2) on [begin, end)."""
    whole = leapfrog(shape, cur, prev, w, f, a1, c1, 0, None)
    level1 = with_halo(shape, whole, ints(prev))
    return whole[begin:end], leapfrog(shape, level1, cur, w, f, a2, c2, begin, end)


# ---- the records -------------------------------------------------------------------------------------------------------------------
def padded_index(shape, dims, begin):
    """padded linear index of every interior cell of the rows from `begin` on"""
    ps = padded_shape(shape, dims)
    return interior(shape, np.arange(int(np.prod(ps)), dtype=np.int64).reshape(ps))[begin:]


def diff_record(shape, dims, a, b, begin):
    """the six fields of lora_grid_diff for d = a - b over a region that starts at row `begin`, as Python numbers:
    (max_abs, sum_sq, a_abs_max, argmax, count, nonfinite)"""
    d = a - b
    where = padded_index(shape, dims, begin)[:d.shape[0]]
    top = int(np.abs(d).max())
    return (top, sum(int(x) * int(x) for x in d.ravel()), int(np.abs(a).max()), int(where[np.abs(d) == top].min()), d.size, 0)


def dot_record(a, b):
    """the four fields of lora_grid_dot as Python ints: (dot, sum_abs, count, nonfinite)"""
    prod = [int(x) * int(y) for x, y in zip(a.ravel(), b.ravel())]
    return (sum(prod), sum(abs(x) for x in prod), a.size, 0)


# ---- data and the conditions of an exact comparison --------------------------------------------------------------------------------
def data(shape, dims, seed):
    """(u, f, u_prev) as float64 padded arrays of integers: u and u_prev in 0..99 over the whole padded array, f in 0..9 on the
    interior with NaN in its halo; read-only"""
    rng = np.random.default_rng(seed)
    ps = padded_shape(shape, dims)
    u = rng.integers(0, 100, ps).astype(np.float64)
    f = np.full(ps, np.nan)
    interior(shape, f)[...] = rng.integers(0, 10, dims)
    u_prev = rng.integers(0, 100, ps).astype(np.float64)
    for a in (u, f, u_prev):
        a.setflags(write=False)
    return u, f, u_prev


def assert_exact(name, values):
    """Every value a test compares with == must be exact in fp64 in ANY summation order: `values` are the model's largest
    intermediates (arrays of the sums of |w| |u|, records' sums of absolute values, ...); each must be below 2**53.  A
    condition of the test, checked before the engine is called.  Returns the largest."""
    top = 0
    for v in values:
        if isinstance(v, np.ndarray):
            assert v.dtype.kind in "iu", f"{name}: the bound of an exact comparison is computed in integers"
            v = int(np.abs(v).max(initial=0))
        top = max(top, abs(int(v)))
    assert top < EXACT, f"{name}: {top} is not below 2**53 = {EXACT}: the comparison would not be exact"
    return top


def magnitude(shape, u, w, f=None):
    """sum_t |w[t]| |u[i + offset(t)]| + |f|: no partial sum of the kernel's accumulation, in any order, exceeds it"""
    return apply(shape, np.abs(ints(u)), np.abs(ints(w))) + np.abs(_f(shape, f))


def source2_magnitude(shape, u, w, f):
    """the bound of `magnitude` for the second level of source2"""
    level1 = with_halo(shape, magnitude(shape, u, w, f), 0)
    return magnitude(shape, level1, w, f)


def levels_magnitude(shape, u, w, K, dirichlet=False):
    """the bound of `magnitude` for every level of `levels`, which generalises source2_magnitude: the K-level model on |w| and
    |u|.  One array per level, 1 .. K: no partial sum of that level's accumulation, in any order, exceeds it."""
    src = np.abs(ints(u))
    level, out = src, []
    for k in range(1, K + 1):
        mag = magnitude(shape, level, w)
        out.append(mag)
        level = with_halo(shape, mag, src if dirichlet or k % 2 == 0 else 0)
    return out


def periodic_magnitude(shape, u, w, times):
    """the same for `periodic`: one array per sweep"""
    level, out = np.abs(interior(shape, ints(u))), []
    for _ in range(times):
        level = apply_periodic(shape, level, np.abs(ints(w)))
        out.append(level)
    return out


def data_small(shape, dims, seed, top):
    """u as a float64 padded array of integers 0 .. top over the WHOLE padded array (non-zero halos: the halo rule of every
    level is exercised); read-only"""
    u = np.random.default_rng(seed).integers(0, top + 1, padded_shape(shape, dims)).astype(np.float64)
    u.setflags(write=False)
    return u


def leapfrog2_magnitude(shape, prev, cur, w, f, a1, c1, a2, c2):
    """the bound of `magnitude` for the second level of leapfrog2: |a2| (sum |w| |level 1| + |f|) + |c2| |cur|"""
    mag1 = abs(a1) * magnitude(shape, cur, w, f) + abs(c1) * np.abs(interior(shape, ints(prev)))
    level1 = with_halo(shape, mag1, np.abs(ints(prev)))
    return abs(a2) * magnitude(shape, level1, w, f) + abs(c2) * np.abs(interior(shape, ints(cur)))


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def cg_start(shape, dims, w, seed):
    """integer (x0, r0) for ONE exact iteration of lora_plan_cg_small with integer taps.  The taps are positive and sum to far
    more than 1, so p.(sigma p - tau S p) is negative for almost every p and the kernel would halt before it updates anything.
    r0 is therefore the eigenvector of the lowest eigenvalue of the symmetric part of S (zero halo), scaled to +-40 and rounded
    to integers: p.S p < 0, so p.A p > 0 for every sigma > 0, tau > 0 -- the test asserts that in the model.  x0 in 0..99."""
    dims = tuple(dims)
    n = int(np.prod(dims))
    eye = np.eye(n, dtype=np.int64).reshape((n,) + dims)
    S = np.stack([apply_zero_halo(shape, e, w).ravel() for e in eye], axis=1).astype(np.float64)
    vals, vecs = np.linalg.eigh((S + S.T) / 2.0)
    v = vecs[:, 0]
    r0 = np.rint(40.0 * v / np.abs(v).max()).astype(np.int64).reshape(dims)
    x0 = np.random.default_rng(seed).integers(0, 100, dims).astype(np.int64)
    assert vals[0] < 0.0 and r0.any()
    return x0, r0


def exactly(got, want):
    """the comparison of the GPU tests: a float64 array from the engine equals the model's integers, value for value"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype.kind in "iu" and np.abs(want).max(initial=0) < EXACT
    return got.shape == want.shape and bool(np.isfinite(got).all()) and np.array_equal(got, want.astype(np.float64))
