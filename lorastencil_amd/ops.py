"""Host-side mirror of the reference's operator interface, on top of the C ABI (include/lorastencil.h).

* ``gpu_1d1r`` ... ``gpu_star_3d1r``: the reference's seven operators (1d_utils.h:45-47, 2d_utils.h:47-51,
  3d_utils.h:44-48) with the same argument order and meaning, on padded numpy host arrays.
* ``Plan``: the device-resident form of the same sweep (caller-owned device buffers and stream) that the
  benchmark and the multi-GPU slab driver use.
* params tables, the low-rank factor precompute and the glibc ``rand()`` fill of the reference harness.

Everything computes in the HIP library; there is no Python/CPU implementation here.
"""
from __future__ import annotations

import ctypes
import threading
from typing import NamedTuple, Sequence

import numpy as np

from . import _lib
from ._lib import LoraError, RunInfo, check  # noqa: F401  (re-exported)

SHAPES = {
    "1d1r": 0,
    "1d2r": 1,
    "star2d1r": 2,
    "box2d1r": 3,
    "star2d3r": 4,
    "box2d3r": 5,
    "star3d1r": 6,
    "box3d1r": 7,
}
SHAPE_NAMES = {v: k for k, v in SHAPES.items()}
_dp = ctypes.POINTER(ctypes.c_double)


def shape_id(shape) -> int:
    if isinstance(shape, str):
        sid = _lib.lib().lora_shape_from_name(shape.encode())
        if sid < 0:
            raise ValueError(f"unknown shape {shape!r}")
        return sid
    return int(shape)


def ndim(shape) -> int:
    return _lib.lib().lora_shape_ndim(shape_id(shape))


def ntaps(shape) -> int:
    return _lib.lib().lora_shape_ntaps(shape_id(shape))


def gstencil_factor(shape) -> int:
    return _lib.lib().lora_shape_gstencil_factor(shape_id(shape))


def halo(shape) -> tuple:
    return {1: (4,), 2: (4, 4), 3: (1, 2, 4)}[ndim(shape)]


def padded_shape(shape, dims: Sequence[int]) -> tuple:
    h = halo(shape)
    if len(dims) != len(h):
        raise ValueError(f"{shape} takes {len(h)} sizes, got {len(dims)}")
    return tuple(int(d) + 2 * k for d, k in zip(dims, h))


def interior(shape, a):
    """Interior view of a padded numpy array or torch tensor."""
    h = halo(shape)
    return a[tuple(slice(k, a.shape[i] - k) for i, k in enumerate(h))]


def _dims_arg(dims: Sequence[int]):
    d = list(int(x) for x in dims) + [0] * (3 - len(dims))
    return (ctypes.c_int * 3)(*d)


def _p(a: np.ndarray):
    if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("expected a C-contiguous float64 array")
    return a.ctypes.data_as(_dp)


# ---- group C: host helpers -------------------------------------------------------------------------
def default_params(shape) -> np.ndarray:
    """The params table the reference harness passes (1d/main.cu:77-78, 2d/main.cu:139-195, 3d/main.cu:112-125)."""
    sid = shape_id(shape)
    p = np.zeros(49)
    n = _lib.lib().lora_default_params(sid, _p(p))
    if n < 0:
        raise LoraError(n, "lora_default_params")
    return p[:n].copy()


def effective_weights(shape, params=None) -> np.ndarray:
    """The taps the operator really applies for ``params`` (see include/lorastencil.h group A)."""
    sid = shape_id(shape)
    w = np.zeros(49)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    n = _lib.lib().lora_effective_weights(sid, pp, _p(w))
    if n < 0:
        raise LoraError(n, "lora_effective_weights")
    return w[:n].copy()


def factorize_7x7(params):
    """Low-rank factor precompute of the box2d operator (2d/gpu.cu:280-350): returns (u[4,7], v[4,7], residual)."""
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.size != 49:
        raise ValueError("params must hold 49 values")
    u = np.zeros((4, 7))
    v = np.zeros((4, 7))
    res = ctypes.c_double(0.0)
    check(_lib.lib().lora_factorize_7x7(_p(params), _p(u), _p(v), ctypes.byref(res)), "lora_factorize_7x7")
    return u, v, res.value


def svd_7x7(weights):
    """Rank-revealing factorisation of any 7x7 tap matrix: returns (u[7,7], v[7,7], sigma[7]) with
    weights = sum_k outer(u[k], v[k]) and sigma descending; truncating after r terms leaves spectral error sigma[r]."""
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if weights.size != 49:
        raise ValueError("weights must hold 49 values")
    u = np.zeros((7, 7))
    v = np.zeros((7, 7))
    sig = np.zeros(7)
    check(_lib.lib().lora_svd_7x7(_p(weights), _p(u), _p(v), _p(sig)), "lora_svd_7x7")
    return u, v, sig


def separable_3x3x3(weights):
    """Exact rank-1 test of 27 taps in fp32 (what bf16 plans evaluate): returns (c, b, a) float32 factors along
    x, y, z when w[dz,dy,dx] == (a[dz] * b[dy]) * c[dx] holds exactly, else None."""
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if weights.size != 27:
        raise ValueError("weights must hold 27 values")
    cba = np.zeros(9, dtype=np.float32)
    rc = _lib.lib().lora_separable_3x3x3(_p(weights), cba.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    if rc < 0:
        check(rc, "lora_separable_3x3x3")
    return (cba[0:3].copy(), cba[3:6].copy(), cba[6:9].copy()) if rc == 1 else None


class GlibcRand:
    """glibc ``rand()`` stream; seed 1 is what the reference's un-seeded harness draws from."""

    def __init__(self, seed: int = 1):
        self._st = _lib.Rng()
        _lib.lib().lora_rng_seed(ctypes.byref(self._st), seed)

    def next(self) -> int:
        return _lib.lib().lora_rng_next(ctypes.byref(self._st))

    def fill(self, count: int, mod: int, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.empty(count, dtype=np.float64)
        _lib.lib().lora_fill_rand(_p(out), count, mod, ctypes.byref(self._st))
        return out


def reference_input(shape, dims, rng: GlibcRand | None = None) -> np.ndarray:
    """Padded input filled like the reference harness (FILL_RANDOM): rand()%10000 in 1D (n+9 draws),
    rand()%100 over the whole padded array in 2D/3D."""
    rng = rng or GlibcRand()
    ps = padded_shape(shape, dims)
    if len(ps) == 1:
        a = rng.fill(ps[0], 10000)
        rng.next()  # 1d/main.cu:107 draws one value more than the array holds
        return a
    return rng.fill(int(np.prod(ps)), 100).reshape(ps)


BOUNDARIES = {"reference": _lib.BC_REFERENCE, "dirichlet": _lib.BC_DIRICHLET, "periodic": _lib.BC_PERIODIC}
DTYPES = {"f64": _lib.F64, "fp64": _lib.F64, "float64": _lib.F64, "bf16": _lib.BF16, "bfloat16": _lib.BF16}


def dtype_id(dtype) -> int:
    if isinstance(dtype, str):
        return DTYPES[dtype]
    return int(dtype)


def to_bf16(a: np.ndarray) -> np.ndarray:
    """float64 array -> bf16 bit patterns (uint16), round-to-nearest-even."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=np.uint16)
    _lib.lib().lora_f64_to_bf16(_p(a), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), a.size)
    return out


def from_bf16(a: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) -> float64 (exact)."""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    out = np.empty(a.shape, dtype=np.float64)
    _lib.lib().lora_bf16_to_f64(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), _p(out), a.size)
    return out


# ---- reductions on the device: what lora_plan_stats / lora_plan_diff / lora_plan_run_until return -----------------
class GridStats(NamedTuple):
    """Statistics of the finite interior cells of a region; ``count`` cells, ``nonfinite`` of them NaN or +-inf."""
    min: float
    max: float
    abs_max: float
    sum: float
    sum_sq: float
    count: int
    nonfinite: int


EMPTY_STATS = GridStats(float("inf"), float("-inf"), 0.0, 0.0, 0.0, 0, 0)


class GridDiff(NamedTuple):
    """Difference d = a - b over a region: ``argmax`` is the lowest PADDED linear index with |d| == max_abs (-1: none)."""
    max_abs: float
    sum_sq: float
    a_abs_max: float
    argmax: int
    count: int
    nonfinite: int


class UntilResult(NamedTuple):
    times_done: int
    checks: int
    converged: bool
    diverged: bool
    residual: float
    last: GridDiff


class GridDot(NamedTuple):
    """Sum of the products a * b over a region (lora_grid_dot): ``dot`` and ``sum_abs`` = sum |a b| over the cells whose product
    is finite, ``nonfinite`` the number of the others."""
    dot: float
    sum_abs: float
    count: int
    nonfinite: int


class CgResult(NamedTuple):
    """What ``run_cg_until`` returns (lora_cg_result): the until-result, the extreme Ritz values of A = I - S from the run's
    coefficients, the spectral radius of S they imply (NaN when no iteration ran), and whether CG broke down."""
    until: UntilResult
    lambda_min: float
    lambda_max: float
    rho_estimate: float
    breakdown: bool


class ThetaResult(NamedTuple):
    """What ``run_theta`` returns (lora_theta_result): the steps finished, whether CG broke down, the steps that used all their
    iterations, the iterations of the finished steps (their sum and their largest, and ``iterations``: one count per step), r.r
    at the start of the last step and at the run's end, and the true residual S(u) + f - u of the last level."""
    steps_done: int
    breakdown: bool
    unconverged_steps: int
    iterations_total: int
    iterations_max: int
    last_rr0: float
    last_rr: float
    steady: GridDiff
    iterations: tuple = ()


class MgResult(NamedTuple):
    """What ``run_mg_until`` returns (lora_mg_result): the until-result counted in CYCLES and the extents of the levels that ran,
    level 0 first."""
    until: UntilResult
    levels: int
    level_dims: tuple


class PcgResult(NamedTuple):
    """What ``run_pcg_until`` returns (lora_pcg_result): the until-result counted in ITERATIONS, the extreme Ritz values of M A
    from the run's coefficients (NaN when no iteration ran), whether PCG broke down, and the depth of the hierarchy."""
    until: UntilResult
    lambda_min: float
    lambda_max: float
    breakdown: bool
    levels: int


NORMS = {"max": _lib.NORM_MAX, "rms": _lib.NORM_RMS}


def _tuple_of(cls, c):
    return cls(*[getattr(c, f) for f in cls._fields])


def _until_result(r) -> UntilResult:
    return UntilResult(r.times_done, r.checks, bool(r.converged), bool(r.diverged), r.residual, _tuple_of(GridDiff, r.last))


def _cg_result(r) -> CgResult:
    return CgResult(_until_result(r.until), r.lambda_min, r.lambda_max, r.rho_estimate, bool(r.breakdown))


def _theta_result(r, iterations=()) -> ThetaResult:
    return ThetaResult(r.steps_done, bool(r.breakdown), r.unconverged_steps, r.iterations_total, r.iterations_max, r.last_rr0, r.last_rr,
                       _tuple_of(GridDiff, r.steady), tuple(int(k) for k in iterations))


def _mg_result(r, nd: int) -> MgResult:
    return MgResult(_until_result(r.until), r.levels, tuple(tuple(r.level_dims[l][a] for a in range(nd)) for l in range(r.levels)))


def _pcg_result(r) -> PcgResult:
    return PcgResult(_until_result(r.until), r.lambda_min, r.lambda_max, bool(r.breakdown), r.levels)


def _mg_arg(pre, post, omega, max_levels, coarse_iters):
    return _lib.Mg(int(pre), int(post), float(omega), int(max_levels), int(coarse_iters))


def _until_arg(tol, rtol, norm, check_every, max_times):
    n = NORMS[norm] if isinstance(norm, str) else int(norm)
    return _lib.Until(float(tol), float(rtol), n, int(check_every), int(max_times))


def stats_merge(*parts: GridStats) -> GridStats:
    """The record of the union of disjoint regions (lora_grid_stats_merge), e.g. of the own rows of N slabs."""
    acc = _lib.GridStats(*EMPTY_STATS)
    for part in parts:
        one = _lib.GridStats(*part)
        _lib.lib().lora_grid_stats_merge(ctypes.byref(acc), ctypes.byref(one))
    return _tuple_of(GridStats, acc)


# ---- group A: the reference's operators on host arrays -------------------------------------------------
_default_source = threading.local()  # keeps the array lora_set_default_source points at alive, per thread like the C side


def set_default_source(source):
    """The source term f (a padded float64 host array of the operator's grid, or None) that the host operators called
    afterwards on this thread sweep with: u <- S(u) + f (lora_set_default_source).  Returns the previous array or None."""
    old = getattr(_default_source, "array", None)
    if source is None:
        _lib.lib().lora_set_default_source(None)
        _default_source.array = None
        return old
    if not (isinstance(source, np.ndarray) and source.dtype == np.float64 and source.flags["C_CONTIGUOUS"]):
        raise ValueError("the source must be a C-contiguous float64 array")
    _lib.lib().lora_set_default_source(source.ctypes.data)
    _default_source.array = source
    return old


def set_default_leap3(on) -> int:
    """Plan option "leap3" (3D fp64: two leapfrog steps per launch) of the plans created afterwards on this thread, the ones of
    run_host_leapfrog and run_host_chebyshev included (lora_set_default_leap3).  Returns the previous value."""
    return _lib.lib().lora_set_default_leap3(1 if on else 0)


def set_default_wave3(on) -> int:
    """Plan option "wave3" (3D fp64: two wave steps per launch) of the plans created afterwards on this thread, the ones of
    run_host_wave included (lora_set_default_wave3).  Returns the previous value."""
    return _lib.lib().lora_set_default_wave3(1 if on else 0)


def set_default_coarse1(on) -> int:
    """Plan option "coarse1" (multigrid cycles run a coarsest level that fits as one launch) of the plans created afterwards on
    this thread, the ones of run_host_mg, run_host_pcg and run_host_theta_mg included (lora_set_default_coarse1).  Returns the
    previous value."""
    return _lib.lib().lora_set_default_coarse1(1 if on else 0)


def set_default_mgfuse(on) -> int:
    """Plan option "mgfuse" (multigrid cycles restrict a level's defect in the launch that computes it) of the plans created
    afterwards on this thread, the ones of run_host_mg, run_host_pcg and run_host_theta_mg included (lora_set_default_mgfuse).
    Returns the previous value."""
    return _lib.lib().lora_set_default_mgfuse(1 if on else 0)


class _with_source:
    """set the thread's default source for one host-operator call, restore the previous one afterwards"""

    def __init__(self, source, padded):
        if source is not None:
            source = np.ascontiguousarray(source, dtype=np.float64)
            if source.shape != tuple(padded):
                raise ValueError(f"the source must be a padded array of the grid's shape {tuple(padded)}")
        self.source = source

    def __enter__(self):
        if self.source is not None:
            self.old = set_default_source(self.source)

    def __exit__(self, *exc):
        if self.source is not None:
            set_default_source(self.old)


def run_host(shape, in_: np.ndarray, params=None, times: int = 1, quiet: bool = True, out: np.ndarray | None = None, source=None):
    """Generic host-buffer operator.  Returns (out, RunInfo).  A uint16 input is taken as bf16 bit patterns.  ``source``: a
    padded float64 array f of the grid's shape: every sweep is u <- S(u) + f on the interior (fp64 grids)."""
    with _with_source(source, in_.shape):
        return _run_host(shape, in_, params, times, quiet, out)


def _run_host(shape, in_, params, times, quiet, out):
    sid = shape_id(shape)
    if in_.dtype == np.uint16:
        in_ = np.ascontiguousarray(in_)
        h = halo(sid)
        dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
        if out is None:
            out = np.zeros_like(in_)
        pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
        info = RunInfo()
        check(_lib.lib().lora_run_host_dtype(sid, _lib.BF16, in_.ctypes.data, out.ctypes.data, pp, int(times),
                                             _dims_arg(dims), int(quiet), ctypes.byref(info)),
              f"lora_run_host_dtype({SHAPE_NAMES.get(sid, sid)}, bf16)")
        return out, info
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("input rank does not match the shape")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    if out is None:
        out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    info = RunInfo()
    check(_lib.lib().lora_run_host(sid, _p(in_), _p(out), pp, int(times), _dims_arg(dims), int(quiet),
                                   ctypes.byref(info)), f"lora_run_host({SHAPE_NAMES.get(sid, sid)})")
    return out, info


def run_host_until(shape, in_: np.ndarray, tol: float, params=None, rtol: float = 0.0, norm="max", check_every: int = 60,
                   max_times: int = 6000, quiet: bool = True, source=None):
    """run_host with the run-until-steady driver (lora_run_host_until).  Returns (out, UntilResult, RunInfo).  ``source`` as in
    run_host."""
    with _with_source(source, in_.shape):
        return _run_host_until(shape, in_, tol, params, rtol, norm, check_every, max_times, quiet)


def _run_host_until(shape, in_, tol, params, rtol, norm, check_every, max_times, quiet):
    sid = shape_id(shape)
    bf16 = in_.dtype == np.uint16
    in_ = np.ascontiguousarray(in_) if bf16 else np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("input rank does not match the shape")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    u, r, info = _until_arg(tol, rtol, norm, check_every, max_times), _lib.UntilResult(), RunInfo()
    check(_lib.lib().lora_run_host_until(sid, _lib.BF16 if bf16 else _lib.F64, in_.ctypes.data, out.ctypes.data, pp, _dims_arg(dims),
                                         ctypes.byref(u), ctypes.byref(r), int(quiet), ctypes.byref(info)),
          f"lora_run_host_until({SHAPE_NAMES.get(sid, sid)})")
    return out, _until_result(r), info


def run_host_leapfrog(shape, cur: np.ndarray, prev: np.ndarray, c: float = -1.0, times: int = 1, params=None, quiet: bool = True):
    """``times`` leapfrog steps u(t+1) = S(u(t)) + c u(t-1) from the padded float64 host arrays ``cur`` (level 0) and ``prev``
    (level -1) (lora_run_host_leapfrog).  Returns (level ``times`` as a padded array, RunInfo)."""
    sid = shape_id(shape)
    cur = np.ascontiguousarray(cur, dtype=np.float64)
    prev = np.ascontiguousarray(prev, dtype=np.float64)
    h = halo(sid)
    if cur.ndim != len(h) or prev.shape != cur.shape:
        raise ValueError("cur and prev must be padded arrays of the shape's rank and of one size")
    dims = [cur.shape[i] - 2 * h[i] for i in range(cur.ndim)]
    out = np.zeros_like(cur)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    info = RunInfo()
    check(_lib.lib().lora_run_host_leapfrog(sid, _p(cur), _p(prev), _p(out), pp, float(c), int(times), _dims_arg(dims), int(quiet),
                                            ctypes.byref(info)), f"lora_run_host_leapfrog({SHAPE_NAMES.get(sid, sid)})")
    return out, info


def run_host_wave(shape, cur: np.ndarray, prev: np.ndarray, kappa: np.ndarray, b: float = 2.0, c: float = -1.0, laplacian: bool = True,
                  times: int = 1, params=None, quiet: bool = True):
    """``times`` variable-coefficient wave steps u(t+1) = kappa S(u(t)) + b u(t) + c u(t-1) from the padded float64 host arrays ``cur``
    (level 0), ``prev`` (level -1) and ``kappa`` (the per-cell coefficient; its halo is never read) (lora_run_host_wave).  With
    ``laplacian`` S is the zero-sum form of the taps, so b = 2, c = -1 is 2 u - u- + kappa L u.  Returns (level ``times`` as a padded
    array, RunInfo)."""
    sid = shape_id(shape)
    cur = np.ascontiguousarray(cur, dtype=np.float64)
    prev = np.ascontiguousarray(prev, dtype=np.float64)
    kappa = np.ascontiguousarray(kappa, dtype=np.float64)
    h = halo(sid)
    if cur.ndim != len(h) or prev.shape != cur.shape or kappa.shape != cur.shape:
        raise ValueError("cur, prev and kappa must be padded arrays of the shape's rank and of one size")
    dims = [cur.shape[i] - 2 * h[i] for i in range(cur.ndim)]
    out = np.zeros_like(cur)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    info = RunInfo()
    check(_lib.lib().lora_run_host_wave(sid, _p(cur), _p(prev), _p(kappa), _p(out), pp, float(b), float(c), int(bool(laplacian)), int(times),
                                        _dims_arg(dims), int(quiet), ctypes.byref(info)), f"lora_run_host_wave({SHAPE_NAMES.get(sid, sid)})")
    return out, info


def chebyshev_coeffs(rho: float, first_step: int = 1, count: int = 1):
    """The Chebyshev schedule for a spectrum inside [-rho, rho] (lora_chebyshev_coeffs; host only): (a, c) as float64 arrays with
    a[i] = w(first_step + i), c[i] = 1 - a[i]; w(1) = 1, w(2) = 1 / (1 - rho^2 / 2), w(k+1) = 1 / (1 - rho^2 w(k) / 4).  For the
    5-point Jacobi taps on an m x n interior with zero halos rho = (cos(pi / (m+1)) + cos(pi / (n+1))) / 2."""
    n = max(int(count), 0)
    a, c = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    check(_lib.lib().lora_chebyshev_coeffs(float(rho), int(first_step), int(count), _p(a), _p(c)), "lora_chebyshev_coeffs")
    return a[:n], c[:n]


def run_host_chebyshev(shape, in_: np.ndarray, rho: float, times: int = 0, source=None, tol=None, rtol: float = 0.0, norm="max",
                       check_every: int = 60, max_times: int = 6000, params=None, quiet: bool = True):
    """The Chebyshev semi-iteration for u = S(u) + f from the padded float64 host array ``in_`` (both starting levels), ``source``
    a padded host array of f or None (lora_run_host_chebyshev).  ``tol`` None: ``times`` steps; else until the true residual is
    <= tol + rtol * max|S(u) + f|, checked every ``check_every`` steps, ``max_times`` at most.  Returns (the newest level as a
    padded array, UntilResult, RunInfo)."""
    sid = shape_id(shape)
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("in_ must be a padded array of the shape's rank")
    src = None
    if source is not None:
        src = np.ascontiguousarray(source, dtype=np.float64)
        if src.shape != in_.shape:
            raise ValueError("source must be a padded array of in_'s size")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    u = None if tol is None else ctypes.byref(_until_arg(tol, rtol, norm, check_every, max_times))
    r, info = _lib.UntilResult(), RunInfo()
    check(_lib.lib().lora_run_host_chebyshev(sid, _p(in_), None if src is None else _p(src), _p(out), pp, float(rho), int(times), u,
                                             ctypes.byref(r), _dims_arg(dims), int(quiet), ctypes.byref(info)),
          f"lora_run_host_chebyshev({SHAPE_NAMES.get(sid, sid)})")
    return out, _until_result(r), info


def cg_spectrum(alpha, beta):
    """(lambda_min, lambda_max) of the Lanczos tridiagonal of a CG run's coefficients (lora_cg_spectrum; host only):
    T[k, k] = 1 / alpha[k] + beta[k-1] / alpha[k-1], T[k, k+1] = sqrt(beta[k]) / alpha[k]; beta[-1] is not read."""
    a = np.ascontiguousarray(np.atleast_1d(alpha), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_1d(beta), dtype=np.float64)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("alpha and beta must be 1D arrays of one length")
    lo, hi = ctypes.c_double(), ctypes.c_double()
    check(_lib.lib().lora_cg_spectrum(_p(a), _p(b), int(a.size), ctypes.byref(lo), ctypes.byref(hi)), "lora_cg_spectrum")
    return lo.value, hi.value


def run_host_cg(shape, in_: np.ndarray, tol: float, source=None, rtol: float = 0.0, norm="max", check_every: int = 20,
                max_times: int = 2000, params=None, quiet: bool = True):
    """Conjugate gradients for u = S(u) + f from the padded float64 host array ``in_`` (the start iterate, its halo the boundary
    values), ``source`` a padded host array of f or None (lora_run_host_cg): until the true residual is <= tol + rtol *
    max|S(u) + f|, checked every ``check_every`` iterations, ``max_times`` at most.  Returns (the iterate as a padded array,
    CgResult, RunInfo)."""
    sid = shape_id(shape)
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("in_ must be a padded array of the shape's rank")
    src = None
    if source is not None:
        src = np.ascontiguousarray(source, dtype=np.float64)
        if src.shape != in_.shape:
            raise ValueError("source must be a padded array of in_'s size")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    u, r, info = _until_arg(tol, rtol, norm, check_every, max_times), _lib.CgResult(), RunInfo()
    check(_lib.lib().lora_run_host_cg(sid, _p(in_), None if src is None else _p(src), _p(out), pp, ctypes.byref(u), ctypes.byref(r),
                                      _dims_arg(dims), int(quiet), ctypes.byref(info)), f"lora_run_host_cg({SHAPE_NAMES.get(sid, sid)})")
    return out, _cg_result(r), info


def mg_coarse_dims(shape, dims: Sequence[int]) -> tuple:
    """The extents of the next coarser multigrid level (lora_mg_coarse_dims; host only): floor(n / 2) per axis, the innermost
    rounded down to even.  Raises LoraError (LORA_EUNSUPPORTED) for a 1D shape and when an extent would fall below 4."""
    sid = shape_id(shape)
    out = (ctypes.c_int * 3)()
    if len(dims) != ndim(sid):
        raise ValueError("wrong number of sizes for the shape")
    check(_lib.lib().lora_mg_coarse_dims(sid, _dims_arg(dims), out), "lora_mg_coarse_dims")
    return tuple(out[: ndim(sid)])


def mg_coarse_taps(shape, w, dims: Sequence[int], cdims: Sequence[int]) -> np.ndarray:
    """The taps of the coarse operator for the grids ``dims`` -> ``cdims`` from the fine taps ``w`` (lora_mg_coarse_taps; host
    only): w q_a along axis a with q_a = ((n_c + 1) / (n + 1))^2, the geometric blend for diagonal taps, the centre tap keeping
    the tap sum."""
    sid = shape_id(shape)
    w = np.ascontiguousarray(w, dtype=np.float64).ravel()
    if w.size != ntaps(sid) or len(dims) != ndim(sid) or len(cdims) != ndim(sid):
        raise ValueError("wrong number of taps or sizes for the shape")
    out = np.zeros_like(w)
    check(_lib.lib().lora_mg_coarse_taps(sid, _p(w), _dims_arg(dims), _dims_arg(cdims), _p(out)), "lora_mg_coarse_taps")
    return out


def run_host_mg(shape, in_: np.ndarray, tol: float, source=None, pre: int = 2, post: int = 2, omega: float = 0.8, max_levels: int = 0,
                coarse_iters: int = 0, rtol: float = 0.0, norm="max", check_every: int = 1, max_times: int = 50, params=None,
                quiet: bool = True):
    """Multigrid V(pre, post) cycles for u = S(u) + f from the padded float64 host array ``in_`` (the start iterate, its halo the
    boundary values), ``source`` a padded host array of f or None (lora_run_host_mg): until the true residual is <= tol + rtol *
    max|S(u) + f|, checked every ``check_every`` cycles, ``max_times`` cycles at most.  Returns (the iterate as a padded array,
    MgResult, RunInfo)."""
    sid = shape_id(shape)
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("in_ must be a padded array of the shape's rank")
    src = None
    if source is not None:
        src = np.ascontiguousarray(source, dtype=np.float64)
        if src.shape != in_.shape:
            raise ValueError("source must be a padded array of in_'s size")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    m, u = _mg_arg(pre, post, omega, max_levels, coarse_iters), _until_arg(tol, rtol, norm, check_every, max_times)
    r, info = _lib.MgResult(), RunInfo()
    check(_lib.lib().lora_run_host_mg(sid, _p(in_), None if src is None else _p(src), _p(out), pp, ctypes.byref(m), ctypes.byref(u),
                                      ctypes.byref(r), _dims_arg(dims), int(quiet), ctypes.byref(info)), f"lora_run_host_mg({SHAPE_NAMES.get(sid, sid)})")
    return out, _mg_result(r, in_.ndim), info


def run_host_theta(shape, in_: np.ndarray, tau: float, steps: int, source=None, theta: float = 1.0, max_iters: int = 50,
                   rtol: float = 1e-8, params=None, quiet: bool = True):
    """``steps`` implicit steps of du/dt = S(u) + f - u with step ``tau`` from the padded float64 host array ``in_`` (level 0,
    its halo the boundary values), ``source`` a padded host array of f or None (lora_run_host_theta).  ``theta``: 1 backward
    Euler, 0.5 Crank-Nicolson.  Returns (the last level as a padded array, ThetaResult without per-step counts, RunInfo)."""
    sid = shape_id(shape)
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("in_ must be a padded array of the shape's rank")
    src = None
    if source is not None:
        src = np.ascontiguousarray(source, dtype=np.float64)
        if src.shape != in_.shape:
            raise ValueError("source must be a padded array of in_'s size")
    dims = [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    r, info = _lib.ThetaResult(), RunInfo()
    check(_lib.lib().lora_run_host_theta(sid, _p(in_), None if src is None else _p(src), _p(out), pp, float(theta), float(tau), int(steps),
                                         int(max_iters), float(rtol), _dims_arg(dims), int(quiet), ctypes.byref(info), ctypes.byref(r)),
          f"lora_run_host_theta({SHAPE_NAMES.get(sid, sid)})")
    return out, _theta_result(r), info


def _host_arrays(shape, in_, source):
    sid = shape_id(shape)
    in_ = np.ascontiguousarray(in_, dtype=np.float64)
    h = halo(sid)
    if in_.ndim != len(h):
        raise ValueError("in_ must be a padded array of the shape's rank")
    src = None
    if source is not None:
        src = np.ascontiguousarray(source, dtype=np.float64)
        if src.shape != in_.shape:
            raise ValueError("source must be a padded array of in_'s size")
    return sid, in_, src, [in_.shape[i] - 2 * h[i] for i in range(in_.ndim)]


def run_host_pcg(shape, in_: np.ndarray, tol: float, source=None, smooth: int = 2, omega: float = 0.8, max_levels: int = 0,
                 coarse_iters: int = 0, rtol: float = 0.0, norm="max", check_every: int = 2, max_times: int = 50, params=None,
                 quiet: bool = True):
    """Conjugate gradients preconditioned by one V(smooth, smooth) cycle for u = S(u) + f from the padded float64 host array
    ``in_`` (lora_run_host_pcg): until the true residual is <= tol + rtol * max|S(u) + f|, checked every ``check_every``
    iterations.  Returns (the iterate as a padded array, PcgResult, RunInfo)."""
    sid, in_, src, dims = _host_arrays(shape, in_, source)
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    m, u = _mg_arg(smooth, smooth, omega, max_levels, coarse_iters), _until_arg(tol, rtol, norm, check_every, max_times)
    r, info = _lib.PcgResult(), RunInfo()
    check(_lib.lib().lora_run_host_pcg(sid, _p(in_), None if src is None else _p(src), _p(out), pp, ctypes.byref(m), ctypes.byref(u),
                                       ctypes.byref(r), _dims_arg(dims), int(quiet), ctypes.byref(info)), f"lora_run_host_pcg({SHAPE_NAMES.get(sid, sid)})")
    return out, _pcg_result(r), info


def run_host_theta_mg(shape, in_: np.ndarray, tau: float, steps: int, source=None, theta: float = 1.0, max_iters: int = 50,
                      rtol: float = 1e-8, smooth: int = 2, omega: float = 0.8, max_levels: int = 0, coarse_iters: int = 0,
                      check_every: int = 2, params=None, quiet: bool = True):
    """``run_host_theta`` with every step's solve preconditioned by one V(smooth, smooth) cycle for the step's operator
    (lora_run_host_theta_mg); the state is read back every ``check_every`` iterations.  Returns (the last level as a padded
    array, ThetaResult without per-step counts, RunInfo)."""
    sid, in_, src, dims = _host_arrays(shape, in_, source)
    out = np.zeros_like(in_)
    pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
    m, r, info = _mg_arg(smooth, smooth, omega, max_levels, coarse_iters), _lib.ThetaResult(), RunInfo()
    check(_lib.lib().lora_run_host_theta_mg(sid, _p(in_), None if src is None else _p(src), _p(out), pp, float(theta), float(tau), int(steps),
                                            int(max_iters), float(rtol), ctypes.byref(m), int(check_every), _dims_arg(dims), int(quiet),
                                            ctypes.byref(info), ctypes.byref(r)), f"lora_run_host_theta_mg({SHAPE_NAMES.get(sid, sid)})")
    return out, _theta_result(r), info


def _operator(cname: str, nd: int):
    def op(in_, out, params, times, *sizes):
        if len(sizes) != nd:
            raise TypeError(f"{cname[5:]} takes {nd} size argument(s)")
        fn = getattr(_lib.lib(), cname)
        check(fn(_p(in_), _p(out), _p(np.ascontiguousarray(params, dtype=np.float64)), int(times),
                 *[int(s) for s in sizes]), cname)

    op.__name__ = cname[5:]
    op.__doc__ = f"Drop-in for the reference's {cname[5:]}(in, out, params, times, sizes...); prints its three lines."
    return op


gpu_1d1r = _operator("lora_gpu_1d1r", 1)
gpu_1d2r = _operator("lora_gpu_1d2r", 1)
gpu_star_2d1r = _operator("lora_gpu_star_2d1r", 2)
gpu_star_2d3r = _operator("lora_gpu_star_2d3r", 2)
gpu_box_2d3r = _operator("lora_gpu_box_2d3r", 2)
gpu_box_3d1r = _operator("lora_gpu_box_3d1r", 3)
gpu_star_3d1r = _operator("lora_gpu_star_3d1r", 3)


# ---- group B: device-resident plans ---------------------------------------------------------------------
def _ptr(x) -> int:
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    return int(x)


def _optr(x):
    """an optional device buffer: None is the null pointer"""
    return None if x is None else _ptr(x)


def _stream(stream) -> int:
    if isinstance(stream, int):
        return stream
    if stream is None:
        try:
            import torch

            if torch.cuda.is_available():
                return int(torch.cuda.current_stream().cuda_stream)
        except ImportError:
            pass
        return 0
    if hasattr(stream, "cuda_stream"):
        return int(stream.cuda_stream)
    return int(stream)


class Plan:
    """One sweep configuration (shape, interior sizes, taps, kernel variant) on device buffers.

    Buffers are padded device arrays (torch CUDA tensors or raw device pointers); ``stream`` is a
    ``torch.cuda.Stream``, a raw ``hipStream_t`` or None (= torch's current stream).
    """

    def __init__(self, shape, dims: Sequence[int], params=None, dtype="f64"):
        self.shape = shape_id(shape)
        self.dtype = dtype_id(dtype)
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != ndim(self.shape):
            raise ValueError("wrong number of sizes for the shape")
        self._h = ctypes.c_void_p()
        pp = None if params is None else _p(np.ascontiguousarray(params, dtype=np.float64))
        check(_lib.lib().lora_plan_create(ctypes.byref(self._h), self.shape, self.dtype, _dims_arg(self.dims), pp),
              "lora_plan_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().lora_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration
    @property
    def padded_shape(self) -> tuple:
        return padded_shape(self.shape, self.dims)

    @property
    def padded_bytes(self) -> int:
        return _lib.lib().lora_plan_padded_bytes(self._h)

    @property
    def kernel_name(self) -> str:
        return _lib.lib().lora_plan_kernel_name(self._h).decode()

    @property
    def kernel_signature(self) -> str:
        """Kernel name + every resolved option that selects the instantiation / launch geometry."""
        return _lib.lib().lora_plan_kernel_signature(self._h).decode()

    @property
    def weights(self) -> np.ndarray:
        w = np.zeros(ntaps(self.shape))
        check(_lib.lib().lora_plan_get_weights(self._h, _p(w), w.size), "lora_plan_get_weights")
        return w

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64).ravel()
        check(_lib.lib().lora_plan_set_weights(self._h, _p(w), w.size), "lora_plan_set_weights")
        return self

    def set_variant(self, variant: int):
        check(_lib.lib().lora_plan_set_variant(self._h, int(variant)), "lora_plan_set_variant")
        return self

    def set_boundary(self, boundary):
        """"reference" (default: halo never written), "dirichlet" (halo fixed) or "periodic" -- applied by run()."""
        b = BOUNDARIES[boundary] if isinstance(boundary, str) else int(boundary)
        check(_lib.lib().lora_plan_set_boundary(self._h, b), "lora_plan_set_boundary")
        return self

    def set_source(self, d_source):
        """The source term f of u <- S(u) + f: a padded device array of this plan (torch CUDA tensor or raw pointer), or None
        to remove it.  The plan borrows the pointer: keep the array alive while it is set (lora_plan_set_source)."""
        check(_lib.lib().lora_plan_set_source(self._h, None if d_source is None else _ptr(d_source)), "lora_plan_set_source")
        self._source = d_source  # keeps a tensor alive as long as the plan points at it
        return self

    def set_option(self, key: str, value: int):
        check(_lib.lib().lora_plan_set_option(self._h, key.encode(), int(value)), f"lora_plan_set_option({key})")
        return self

    def get_option(self, key: str) -> int:
        v = ctypes.c_int(0)
        check(_lib.lib().lora_plan_get_option(self._h, key.encode(), ctypes.byref(v)), f"lora_plan_get_option({key})")
        return v.value

    @property
    def region_granularity(self) -> int:
        return _lib.lib().lora_plan_region_granularity(self._h)

    # -- execution (asynchronous on the stream)
    def step(self, d_in, d_out, stream=None):
        check(_lib.lib().lora_plan_step(self._h, _ptr(d_in), _ptr(d_out), _stream(stream)), "lora_plan_step")

    def step_region(self, d_in, d_out, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step_region(self._h, _ptr(d_in), _ptr(d_out), int(begin), int(end), _stream(stream)),
              "lora_plan_step_region")

    def step2(self, d_in, d_out, stream=None):
        """Two applications in one launch (d_in must be an even time level; see lora_plan_step2)."""
        check(_lib.lib().lora_plan_step2(self._h, _ptr(d_in), _ptr(d_out), _stream(stream)), "lora_plan_step2")

    def step2_region(self, d_in, d_out, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step2_region(self._h, _ptr(d_in), _ptr(d_out), int(begin), int(end),
                                                _stream(stream)), "lora_plan_step2_region")

    def halo(self, d_dst, mode: str, d_src=None, stream=None):
        """Halo cells of a padded device array: "copy" (from d_src), "zero" or "wrap" (periodic, from d_dst itself)."""
        m = {"copy": 0, "zero": 1, "wrap": 2}[mode]
        check(_lib.lib().lora_plan_halo(self._h, _ptr(d_dst), _ptr(d_src) if d_src is not None else None, m,
                                        _stream(stream)), "lora_plan_halo")

    def stepk(self, d_in, d_out, stream=None):
        """The plan's ``steps_per_launch`` applications in one launch (d_in must be an even time level)."""
        check(_lib.lib().lora_plan_stepk(self._h, _ptr(d_in), _ptr(d_out), _stream(stream)), "lora_plan_stepk")

    def stepk_region(self, d_in, d_out, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_stepk_region(self._h, _ptr(d_in), _ptr(d_out), int(begin), int(end),
                                                _stream(stream)), "lora_plan_stepk_region")

    def stepn_region(self, napps: int, d_in, d_out, begin: int, end: int, stream=None):
        """``napps`` applications in one launch: 1, the plan's depth, or a tail depth of its kernel family."""
        check(_lib.lib().lora_plan_stepn_region(self._h, int(napps), _ptr(d_in), _ptr(d_out), int(begin), int(end),
                                                _stream(stream)), "lora_plan_stepn_region")

    def stepn_region2(self, napps: int, d_in, d_out, begin0: int, end0: int, begin1: int, end1: int, stream=None):
        """``napps`` applications over two disjoint ranges: one launch where the kernel family takes two (3D register-resident)."""
        check(_lib.lib().lora_plan_stepn_region2(self._h, int(napps), _ptr(d_in), _ptr(d_out), int(begin0), int(end0), int(begin1),
                                                 int(end1), _stream(stream)), "lora_plan_stepn_region2")

    def run_profiled(self, d_buf0, d_buf1, times: int, stream=None):
        """run() with HIP events around the fused and the single-sweep launches; blocks until the run is done.
        Returns a ``_lib.RunProfile``."""
        prof = _lib.RunProfile()
        check(_lib.lib().lora_plan_run_profiled(self._h, _ptr(d_buf0), _ptr(d_buf1), int(times), _stream(stream),
                                                ctypes.byref(prof)), "lora_plan_run_profiled")
        return prof

    def prepare_run(self, times: int):
        """Allocate now what ``run(..., times)`` would allocate on first need (scratch grid, extended periodic grid)."""
        check(_lib.lib().lora_plan_prepare_run(self._h, int(times)), "lora_plan_prepare_run")
        return self

    def run(self, d_buf0, d_buf1, times: int, stream=None):
        """`times` sweeps ping-ponging from d_buf0; the result is in buffer [times % 2]."""
        check(_lib.lib().lora_plan_run(self._h, _ptr(d_buf0), _ptr(d_buf1), int(times), _stream(stream)),
              "lora_plan_run")

    # -- leapfrog stepping: u(t+1) = S(u(t)) + c u(t-1), the new level stored over the oldest one
    @property
    def leapfrog_depth(self) -> int:
        """0: no leapfrog kernel; 1: single steps; 2: also the two-step launch (lora_plan_leapfrog_depth)."""
        return _lib.lib().lora_plan_leapfrog_depth(self._h)

    def step_leapfrog(self, d_cur, d_prev, c: float = -1.0, stream=None):
        """One step in place: d_prev <- S(d_cur) + c * d_prev on the interior (lora_plan_step_leapfrog)."""
        check(_lib.lib().lora_plan_step_leapfrog(self._h, _ptr(d_cur), _ptr(d_prev), float(c), _stream(stream)), "lora_plan_step_leapfrog")

    def step_leapfrog_region(self, d_cur, d_prev, c: float, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step_leapfrog_region(self._h, _ptr(d_cur), _ptr(d_prev), float(c), int(begin), int(end), _stream(stream)),
              "lora_plan_step_leapfrog_region")

    def step2_leapfrog(self, d_prev, d_cur, d_out1, d_out2, c: float = -1.0, stream=None):
        """Two steps in one launch: d_out1 = S(d_cur) + c d_prev, d_out2 = S(d_out1) + c d_cur (lora_plan_step2_leapfrog)."""
        check(_lib.lib().lora_plan_step2_leapfrog(self._h, _ptr(d_prev), _ptr(d_cur), _ptr(d_out1), _ptr(d_out2), float(c), _stream(stream)),
              "lora_plan_step2_leapfrog")

    def step2_leapfrog_region(self, d_prev, d_cur, d_out1, d_out2, c: float, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step2_leapfrog_region(self._h, _ptr(d_prev), _ptr(d_cur), _ptr(d_out1), _ptr(d_out2), float(c), int(begin),
                                                         int(end), _stream(stream)), "lora_plan_step2_leapfrog_region")

    def run_leapfrog(self, d_prev, d_cur, c: float = -1.0, times: int = 1, stream=None):
        """``times`` steps from d_prev = level -1, d_cur = level 0; level ``times`` ends in d_cur if ``times`` is even, in d_prev if
        odd (lora_plan_run_leapfrog)."""
        check(_lib.lib().lora_plan_run_leapfrog(self._h, _ptr(d_prev), _ptr(d_cur), float(c), int(times), _stream(stream)),
              "lora_plan_run_leapfrog")

    def prepare_leapfrog(self, times: int):
        """Allocate now what ``run_leapfrog(..., times)`` would allocate on first need (its two scratch grids)."""
        check(_lib.lib().lora_plan_prepare_leapfrog(self._h, int(times)), "lora_plan_prepare_leapfrog")
        return self

    # -- variable-coefficient wave steps: u+ = k S(u) + b u + c u-; d_k is a padded device grid, read on interior cells alone
    @property
    def wave_depth(self) -> int:
        """0: no wave kernel; 1: single steps; 2: also the two-step launch: 2D, and 3D plans with option "wave3"
        (lora_plan_wave_depth)."""
        return _lib.lib().lora_plan_wave_depth(self._h)

    def step_wave(self, d_cur, d_prev, d_k, b: float = 2.0, c: float = -1.0, stream=None):
        """One step in place: d_prev <- d_k * S(d_cur) + b * d_cur + c * d_prev on the interior (lora_plan_step_wave)."""
        check(_lib.lib().lora_plan_step_wave(self._h, _ptr(d_cur), _ptr(d_prev), _ptr(d_k), float(b), float(c), _stream(stream)),
              "lora_plan_step_wave")

    def step_wave_region(self, d_cur, d_prev, d_k, b: float, c: float, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step_wave_region(self._h, _ptr(d_cur), _ptr(d_prev), _ptr(d_k), float(b), float(c), int(begin), int(end),
                                                    _stream(stream)), "lora_plan_step_wave_region")

    def step2_wave(self, d_prev, d_cur, d_k, d_out1, d_out2, b: float = 2.0, c: float = -1.0, stream=None):
        """Two steps in one launch: d_out1 = k S(d_cur) + b d_cur + c d_prev, d_out2 = k S(d_out1) + b d_out1 + c d_cur
        (lora_plan_step2_wave; plans of wave depth 2)."""
        check(_lib.lib().lora_plan_step2_wave(self._h, _ptr(d_prev), _ptr(d_cur), _ptr(d_k), _ptr(d_out1), _ptr(d_out2), float(b), float(c),
                                              _stream(stream)), "lora_plan_step2_wave")

    def step2_wave_region(self, d_prev, d_cur, d_k, d_out1, d_out2, b: float, c: float, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step2_wave_region(self._h, _ptr(d_prev), _ptr(d_cur), _ptr(d_k), _ptr(d_out1), _ptr(d_out2), float(b),
                                                     float(c), int(begin), int(end), _stream(stream)), "lora_plan_step2_wave_region")

    def run_wave(self, d_prev, d_cur, d_k, b: float = 2.0, c: float = -1.0, times: int = 1, stream=None):
        """``times`` steps from d_prev = level -1, d_cur = level 0; level ``times`` ends in ``d_cur`` if ``times`` is even, in
        ``d_prev`` if odd (lora_plan_run_wave)."""
        check(_lib.lib().lora_plan_run_wave(self._h, _ptr(d_prev), _ptr(d_cur), _ptr(d_k), float(b), float(c), int(times), _stream(stream)),
              "lora_plan_run_wave")

    def prepare_wave(self, times: int):
        """Allocate now what ``run_wave(..., times)`` would allocate on first need (the two scratch grids)."""
        check(_lib.lib().lora_plan_prepare_wave(self._h, int(times)), "lora_plan_prepare_wave")

    # -- leapfrog steps with a source and a scale: u+ = a (S(u) + f) + c u-; d_f is a padded device grid or None
    def step_leapfrog_src(self, d_cur, d_prev, d_f, a: float = 1.0, c: float = -1.0, stream=None):
        """One step in place: d_prev <- a * (S(d_cur) + d_f) + c * d_prev on the interior (lora_plan_step_leapfrog_src)."""
        check(_lib.lib().lora_plan_step_leapfrog_src(self._h, _ptr(d_cur), _ptr(d_prev), _optr(d_f), float(a), float(c), _stream(stream)),
              "lora_plan_step_leapfrog_src")

    def step_leapfrog_src_region(self, d_cur, d_prev, d_f, a: float, c: float, begin: int, end: int, stream=None):
        check(_lib.lib().lora_plan_step_leapfrog_src_region(self._h, _ptr(d_cur), _ptr(d_prev), _optr(d_f), float(a), float(c), int(begin),
                                                            int(end), _stream(stream)), "lora_plan_step_leapfrog_src_region")

    def step2_leapfrog_src(self, d_prev, d_cur, d_f, d_out1, d_out2, a1: float, c1: float, a2: float, c2: float, stream=None):
        """Two steps in one launch: d_out1 = a1 (S(d_cur) + f) + c1 d_prev, d_out2 = a2 (S(d_out1) + f) + c2 d_cur
        (lora_plan_step2_leapfrog_src)."""
        check(_lib.lib().lora_plan_step2_leapfrog_src(self._h, _ptr(d_prev), _ptr(d_cur), _optr(d_f), _ptr(d_out1), _ptr(d_out2), float(a1),
                                                      float(c1), float(a2), float(c2), _stream(stream)), "lora_plan_step2_leapfrog_src")

    def step2_leapfrog_src_region(self, d_prev, d_cur, d_f, d_out1, d_out2, a1: float, c1: float, a2: float, c2: float, begin: int,
                                  end: int, stream=None):
        check(_lib.lib().lora_plan_step2_leapfrog_src_region(self._h, _ptr(d_prev), _ptr(d_cur), _optr(d_f), _ptr(d_out1), _ptr(d_out2),
                                                             float(a1), float(c1), float(a2), float(c2), int(begin), int(end),
                                                             _stream(stream)), "lora_plan_step2_leapfrog_src_region")

    def run_leapfrog_src(self, d_prev, d_cur, d_f, a, c, times: int = 1, stream=None):
        """``times`` steps; step i uses a[min(i, len - 1)], c[min(i, len - 1)] (scalars: constant coefficients).  The newest level
        ends in ``d_cur`` if ``times`` is even, in ``d_prev`` if odd (lora_plan_run_leapfrog_src)."""
        aa = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
        cc = np.ascontiguousarray(np.atleast_1d(c), dtype=np.float64)
        if aa.ndim != 1 or aa.shape != cc.shape:
            raise ValueError("a and c must be scalars or 1D arrays of one length")
        check(_lib.lib().lora_plan_run_leapfrog_src(self._h, _ptr(d_prev), _ptr(d_cur), _optr(d_f), _p(aa), _p(cc), int(aa.size),
                                                    int(times), _stream(stream)), "lora_plan_run_leapfrog_src")

    def run_chebyshev_until(self, d_prev, d_cur, d_f, rho: float, tol: float, rtol: float = 0.0, norm="max", check_every: int = 60,
                            max_times: int = 6000, stream=None) -> "UntilResult":
        """Chebyshev steps in runs of ``check_every`` until the TRUE residual max|S(u) + f - u| is <= tol + rtol * max|S(u) + f|
        (lora_plan_run_chebyshev_until); ``d_cur`` (level 0 going in; ``d_prev`` any finite values) then holds level
        ``times_done``, bit for bit what ``run_leapfrog_src`` with ``chebyshev_coeffs(rho, 1, times_done)`` gives.  The probe:
        under ``norm="max"`` on a plan whose option "fused_residual" reads 1, one ``residual_src(d_cur, d_f)`` (no third grid);
        under ``norm="rms"`` and on plans without that kernel, a source sweep into a grid the plan owns plus ``diff``."""
        u, r = _until_arg(tol, rtol, norm, check_every, max_times), _lib.UntilResult()
        check(_lib.lib().lora_plan_run_chebyshev_until(self._h, _ptr(d_prev), _ptr(d_cur), _optr(d_f), float(rho), ctypes.byref(u),
                                                       ctypes.byref(r), _stream(stream)), "lora_plan_run_chebyshev_until")
        return _until_result(r)

    # -- conjugate gradients on A = I - S (fp64 plans whose option "cg" reads 1; ``dot`` alone takes every plan)
    def dot(self, d_a, d_b, begin: int = 0, end: int = 0, stream=None) -> GridDot:
        """Sum of a * b over the interior of the outermost range [begin, end) (lora_plan_dot); ``d_a is d_b`` is allowed."""
        out = _lib.GridDot()
        check(_lib.lib().lora_plan_dot(self._h, _ptr(d_a), _ptr(d_b), int(begin), int(end), ctypes.byref(out), _stream(stream)),
              "lora_plan_dot")
        return _tuple_of(GridDot, out)

    def apply_dot(self, d_p, d_q, begin: int = 0, end: int = 0, stream=None) -> GridDot:
        """q = p - S(p) on the interior cells of [begin, end), each cell ``step_region``'s bits subtracted in one more rounding,
        and the dot of p and q from the same launch (lora_plan_apply_dot).  The halo of ``d_q`` is not touched."""
        out = _lib.GridDot()
        check(_lib.lib().lora_plan_apply_dot(self._h, _ptr(d_p), _ptr(d_q), int(begin), int(end), ctypes.byref(out), _stream(stream)),
              "lora_plan_apply_dot")
        return _tuple_of(GridDot, out)

    def cg_update(self, d_x, d_r, d_p, d_q, alpha: float, begin: int = 0, end: int = 0, stream=None) -> GridDot:
        """x = x + alpha p, r = r - alpha q on the interior cells of [begin, end), every operation its own rounding; returns the
        dot of the new r with itself (lora_plan_cg_update)."""
        out = _lib.GridDot()
        check(_lib.lib().lora_plan_cg_update(self._h, _ptr(d_x), _ptr(d_r), _ptr(d_p), _ptr(d_q), float(alpha), int(begin), int(end),
                                             ctypes.byref(out), _stream(stream)), "lora_plan_cg_update")
        return _tuple_of(GridDot, out)

    def cg_direction(self, d_p, d_r, beta: float, begin: int = 0, end: int = 0, stream=None):
        """p = r + beta p on the interior cells of [begin, end) (lora_plan_cg_direction); asynchronous."""
        check(_lib.lib().lora_plan_cg_direction(self._h, _ptr(d_p), _ptr(d_r), float(beta), int(begin), int(end), _stream(stream)),
              "lora_plan_cg_direction")

    # -- implicit time stepping: theta-scheme steps of du/dt = S(u) + f - u, each a CG solve on sigma I - tau S
    def apply_dot_shift(self, d_p, d_q, sigma: float, tau: float, begin: int = 0, end: int = 0, stream=None) -> GridDot:
        """q = sigma p - tau S(p) on the interior cells of [begin, end) in one pass; returns the dot of p and q
        (lora_plan_apply_dot_shift)."""
        out = _lib.GridDot()
        check(_lib.lib().lora_plan_apply_dot_shift(self._h, _ptr(d_p), _ptr(d_q), float(sigma), float(tau), int(begin), int(end),
                                                   ctypes.byref(out), _stream(stream)), "lora_plan_apply_dot_shift")
        return _tuple_of(GridDot, out)

    def theta_start(self, d_u, d_f, tau: float, d_r, d_p, begin: int = 0, end: int = 0, stream=None) -> GridDot:
        """r = p = tau (S(u) + f - u) on the interior cells of [begin, end) in one pass (``d_f`` may be None); returns the dot
        of r with itself (lora_plan_theta_start)."""
        out = _lib.GridDot()
        check(_lib.lib().lora_plan_theta_start(self._h, _ptr(d_u), _optr(d_f), float(tau), _ptr(d_r), _ptr(d_p), int(begin), int(end),
                                               ctypes.byref(out), _stream(stream)), "lora_plan_theta_start")
        return _tuple_of(GridDot, out)

    def prepare_theta(self, steps: int):
        """Allocate now what ``run_theta(..., steps=steps)`` would allocate on first need (three grids, the states, the history)."""
        check(_lib.lib().lora_plan_prepare_theta(self._h, int(steps)), "lora_plan_prepare_theta")
        return self

    def run_theta(self, d_u, d_f, tau: float, steps: int, theta: float = 1.0, max_iters: int = 50, rtol: float = 1e-8,
                  stream=None) -> ThetaResult:
        """``steps`` implicit steps of ``d_u`` in place with step ``tau`` (lora_plan_run_theta): theta = 1 backward Euler, 0.5
        Crank-Nicolson; each step a CG solve to |r| <= rtol |r0| in at most ``max_iters`` iterations, the whole run enqueued
        without a host wait.  ``d_f`` may be None.  Blocks once, at its end."""
        r, its = _lib.ThetaResult(), (ctypes.c_int * max(int(steps), 1))()
        check(_lib.lib().lora_plan_run_theta(self._h, _ptr(d_u), _optr(d_f), float(theta), float(tau), int(steps), int(max_iters),
                                             float(rtol), its, ctypes.byref(r), _stream(stream)), "lora_plan_run_theta")
        return _theta_result(r, its[:max(int(steps), 0)])

    def prepare_cg(self, max_times: int):
        """Allocate now what ``run_cg_until(..., max_times=max_times)`` would allocate on first need (three grids, the state)."""
        check(_lib.lib().lora_plan_prepare_cg(self._h, int(max_times)), "lora_plan_prepare_cg")
        return self

    def run_cg_until(self, d_x, d_f, tol: float, rtol: float = 0.0, norm="max", check_every: int = 20, max_times: int = 2000,
                     stream=None) -> CgResult:
        """Conjugate gradients for u = S(u) + f in rounds of ``check_every`` iterations until the TRUE residual max|S(u) + f - u|
        is <= tol + rtol * max|S(u) + f| (lora_plan_run_cg_until).  ``d_x``: the start iterate with the boundary values in its
        halo, then the solution; ``d_f``: a padded device grid or None.  Needs point-symmetric taps.  ``rho_estimate`` of the
        result is a spectral radius for ``run_chebyshev_until``."""
        u, r = _until_arg(tol, rtol, norm, check_every, max_times), _lib.CgResult()
        check(_lib.lib().lora_plan_run_cg_until(self._h, _ptr(d_x), _optr(d_f), ctypes.byref(u), ctypes.byref(r), _stream(stream)),
              "lora_plan_run_cg_until")
        return _cg_result(r)

    # -- geometric multigrid (plans whose option "mg" reads 1); the coarse grid is a padded array of mg_coarse_dims(shape, dims)
    def mg_restrict(self, d_fine, d_coarse, scale: float = 1.0, stream=None):
        """coarse = scale * prod(rho) * P^T fine on the interior cells of the coarse grid (lora_plan_mg_restrict); asynchronous."""
        check(_lib.lib().lora_plan_mg_restrict(self._h, _ptr(d_fine), _ptr(d_coarse), float(scale), _stream(stream)), "lora_plan_mg_restrict")

    def mg_prolong_add(self, d_coarse, d_fine, stream=None):
        """fine = fine + P coarse on the interior cells of the fine grid, P linear interpolation with a zero coarse halo
        (lora_plan_mg_prolong_add); asynchronous."""
        check(_lib.lib().lora_plan_mg_prolong_add(self._h, _ptr(d_coarse), _ptr(d_fine), _stream(stream)), "lora_plan_mg_prolong_add")

    def prepare_mg(self, pre: int = 2, post: int = 2, omega: float = 0.8, max_levels: int = 0, coarse_iters: int = 0):
        """Allocate now what ``run_mg_until`` with the same cycle would allocate on first need (the level plans and their grids)."""
        m = _mg_arg(pre, post, omega, max_levels, coarse_iters)
        check(_lib.lib().lora_plan_prepare_mg(self._h, ctypes.byref(m)), "lora_plan_prepare_mg")
        return self

    def run_mg_until(self, d_x, d_f, tol: float, pre: int = 2, post: int = 2, omega: float = 0.8, max_levels: int = 0,
                     coarse_iters: int = 0, rtol: float = 0.0, norm="max", check_every: int = 1, max_times: int = 50,
                     stream=None) -> MgResult:
        """Multigrid V(pre, post) cycles for u = S(u) + f, damped Jacobi with ``omega`` as the smoother and CG on the coarsest
        level, in rounds of ``check_every`` cycles until the TRUE residual max|S(u) + f - u| is <= tol + rtol * max|S(u) + f|
        (lora_plan_run_mg_until).  ``d_x``: the start iterate with the boundary values in its halo, then the solution;
        ``d_f``: a padded device grid or None.  Needs point-symmetric taps."""
        m, u, r = _mg_arg(pre, post, omega, max_levels, coarse_iters), _until_arg(tol, rtol, norm, check_every, max_times), _lib.MgResult()
        check(_lib.lib().lora_plan_run_mg_until(self._h, _ptr(d_x), _optr(d_f), ctypes.byref(m), ctypes.byref(u), ctypes.byref(r),
                                                _stream(stream)), "lora_plan_run_mg_until")
        return _mg_result(r, len(self.dims))

    def mg_cycle_cost(self):
        """(launches, bytes) of one cycle of the last ``run_mg_until`` (lora_plan_mg_cycle_cost)."""
        n, b = ctypes.c_int(), ctypes.c_double()
        check(_lib.lib().lora_plan_mg_cycle_cost(self._h, ctypes.byref(n), ctypes.byref(b)), "lora_plan_mg_cycle_cost")
        return n.value, b.value

    # -- multigrid-preconditioned CG, also for the implicit stepper's operator (plans whose option "pcg" reads 1; ``defect``: "cg")
    def defect(self, d_u, d_f, d_out, begin: int = 0, end: int = 0, stream=None):
        """out = (S(u) + f) - u on the interior cells of [begin, end) in one launch, each cell ``step_region``'s bits (``d_f`` may
        be None: out = S(u) - u); no record, asynchronous (lora_plan_defect).  The halo of ``d_out`` is not touched."""
        check(_lib.lib().lora_plan_defect(self._h, _ptr(d_u), _optr(d_f), _ptr(d_out), int(begin), int(end), _stream(stream)),
              "lora_plan_defect")

    def mg_defect_restrict(self, d_u, d_f, d_coarse, scale: float = 1.0, stream=None):
        """The defect S(u) + f - u of this (fine) plan restricted into ``d_coarse`` in ONE launch (lora_plan_mg_defect_restrict):
        bit for bit ``defect`` into a spare grid followed by ``mg_restrict``, without the spare grid; asynchronous.  ``d_f`` may be
        None; only the interior of ``d_coarse`` (layout: ``mg_coarse_dims``) is written."""
        check(_lib.lib().lora_plan_mg_defect_restrict(self._h, _ptr(d_u), _optr(d_f), _ptr(d_coarse), float(scale), _stream(stream)),
              "lora_plan_mg_defect_restrict")

    def cg_small(self, d_x, d_r, iters: int, sigma: float = 1.0, tau: float = 1.0, d_info=None, stream=None):
        """``iters`` conjugate-gradient iterations for (sigma I - tau S) on a grid that fits one workgroup, in ONE launch
        (lora_plan_cg_small; plans whose option "cg_small" reads 1); asynchronous.  ``d_r`` holds the residual of ``d_x`` on entry;
        only the interiors of both are read and written.  ``d_info``: None or four device doubles {rr0, rr, iterations, halt}."""
        check(_lib.lib().lora_plan_cg_small(self._h, _ptr(d_x), _ptr(d_r), int(iters), float(sigma), float(tau), _optr(d_info),
                                            _stream(stream)), "lora_plan_cg_small")

    def mg_precondition(self, d_r, d_z, sigma: float = 1.0, tau: float = 1.0, pre: int = 2, post: int = 2, omega: float = 0.8,
                        max_levels: int = 0, coarse_iters: int = 0, stream=None):
        """z = M r: one V(pre, post) cycle for (sigma I - tau S) z = r from z = 0 (lora_plan_mg_precondition); asynchronous.
        ``d_z`` is zeroed over its whole padded array first; only interior cells of ``d_r`` are read."""
        m = _mg_arg(pre, post, omega, max_levels, coarse_iters)
        check(_lib.lib().lora_plan_mg_precondition(self._h, _ptr(d_r), _ptr(d_z), ctypes.byref(m), float(sigma), float(tau), _stream(stream)),
              "lora_plan_mg_precondition")

    def prepare_pcg(self, max_times: int, smooth: int = 2, omega: float = 0.8, max_levels: int = 0, coarse_iters: int = 0):
        """Allocate now what ``run_pcg_until`` with the same cycle and ``max_times`` would allocate on first need."""
        m = _mg_arg(smooth, smooth, omega, max_levels, coarse_iters)
        check(_lib.lib().lora_plan_prepare_pcg(self._h, ctypes.byref(m), int(max_times)), "lora_plan_prepare_pcg")
        return self

    def run_pcg_until(self, d_x, d_f, tol: float, smooth: int = 2, omega: float = 0.8, max_levels: int = 0, coarse_iters: int = 0,
                      rtol: float = 0.0, norm="max", check_every: int = 2, max_times: int = 50, pre=None, post=None,
                      stream=None) -> PcgResult:
        """Conjugate gradients for u = S(u) + f preconditioned by one V(smooth, smooth) cycle, in rounds of ``check_every``
        iterations until the TRUE residual max|S(u) + f - u| is <= tol + rtol * max|S(u) + f| (lora_plan_run_pcg_until).
        ``pre`` / ``post`` override ``smooth``; the engine refuses pre != post (the preconditioner must be symmetric)."""
        m = _mg_arg(smooth if pre is None else pre, smooth if post is None else post, omega, max_levels, coarse_iters)
        u, r = _until_arg(tol, rtol, norm, check_every, max_times), _lib.PcgResult()
        check(_lib.lib().lora_plan_run_pcg_until(self._h, _ptr(d_x), _optr(d_f), ctypes.byref(m), ctypes.byref(u), ctypes.byref(r),
                                                 _stream(stream)), "lora_plan_run_pcg_until")
        return _pcg_result(r)

    def run_theta_mg(self, d_u, d_f, tau: float, steps: int, theta: float = 1.0, max_iters: int = 50, rtol: float = 1e-8,
                     smooth: int = 2, omega: float = 0.8, max_levels: int = 0, coarse_iters: int = 0, check_every: int = 2,
                     stream=None) -> ThetaResult:
        """``run_theta`` with every step's solve preconditioned by one V(smooth, smooth) cycle for the step's operator
        (lora_plan_run_theta_mg).  The state is read back every ``check_every`` iterations; blocks there and at its end."""
        m = _mg_arg(smooth, smooth, omega, max_levels, coarse_iters)
        r, its = _lib.ThetaResult(), (ctypes.c_int * max(int(steps), 1))()
        check(_lib.lib().lora_plan_run_theta_mg(self._h, _ptr(d_u), _optr(d_f), float(theta), float(tau), int(steps), int(max_iters),
                                                float(rtol), ctypes.byref(m), int(check_every), its, ctypes.byref(r), _stream(stream)),
              "lora_plan_run_theta_mg")
        return _theta_result(r, its[:max(int(steps), 0)])

    # -- reductions on the device (these block until the result is on the host)
    def stats(self, d_buf, begin: int = 0, end: int = 0, stream=None) -> GridStats:
        """Statistics of the interior of ``d_buf`` over the outermost range [begin, end) (0, 0: the whole interior)."""
        out = _lib.GridStats()
        check(_lib.lib().lora_plan_stats(self._h, _ptr(d_buf), int(begin), int(end), ctypes.byref(out), _stream(stream)),
              "lora_plan_stats")
        return _tuple_of(GridStats, out)

    def diff(self, d_a, d_b, begin: int = 0, end: int = 0, stream=None) -> GridDiff:
        """Difference of two grids of this plan, d = a - b in fp64, over the outermost range [begin, end)."""
        out = _lib.GridDiff()
        check(_lib.lib().lora_plan_diff(self._h, _ptr(d_a), _ptr(d_b), int(begin), int(end), ctypes.byref(out), _stream(stream)),
              "lora_plan_diff")
        return _tuple_of(GridDiff, out)

    def residual(self, d_in, begin: int = 0, end: int = 0, stream=None) -> GridDiff:
        """The change of ONE raw sweep of ``d_in``, d = sweep(d_in) - d_in, over the outermost range [begin, end), reduced inside
        the sweep: the grid is read once and nothing is written.  The exact fields equal ``step_region`` into a second buffer
        followed by ``diff``; plans without the kernel (option "fused_residual" == 0) raise LORA_EUNSUPPORTED."""
        out = _lib.GridDiff()
        check(_lib.lib().lora_plan_residual(self._h, _ptr(d_in), int(begin), int(end), ctypes.byref(out), _stream(stream)),
              "lora_plan_residual")
        return _tuple_of(GridDiff, out)

    def residual_src(self, d_in, d_f, begin: int = 0, end: int = 0, stream=None) -> GridDiff:
        """The TRUE residual of u = S(u) + f, d = (sweep(d_in) + d_f) - d_in, over the outermost range [begin, end), reduced inside
        the sweep (lora_plan_residual_src): ``d_in`` and the interior of ``d_f`` are read once and nothing is written.  ``d_f`` is
        an argument, never the plan's source; ``None`` passes NULL, which is exactly ``residual``.  The exact fields equal a
        source sweep into a second buffer followed by ``diff``."""
        out = _lib.GridDiff()
        check(_lib.lib().lora_plan_residual_src(self._h, _ptr(d_in), _optr(d_f), int(begin), int(end), ctypes.byref(out),
                                                _stream(stream)), "lora_plan_residual_src")
        return _tuple_of(GridDiff, out)

    def run_until(self, d_buf0, d_buf1, tol: float, rtol: float = 0.0, norm="max", check_every: int = 60, max_times: int = 6000,
                  stream=None) -> UntilResult:
        """Sweep in runs of ``check_every`` until the residual of one more sweep is <= tol + rtol * max|u| (see
        lora_plan_run_until); ``d_buf0`` then holds level ``times_done``, bit for bit what ``run(times_done)`` gives."""
        u, r = _until_arg(tol, rtol, norm, check_every, max_times), _lib.UntilResult()
        check(_lib.lib().lora_plan_run_until(self._h, _ptr(d_buf0), _ptr(d_buf1), ctypes.byref(u), ctypes.byref(r), _stream(stream)),
              "lora_plan_run_until")
        return _until_result(r)


def device_count() -> int:
    return _lib.lib().lora_device_count()
