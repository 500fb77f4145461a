"""ctypes loader for the HIP engine (lib/liblorastencil_hip.so, C ABI of include/lorastencil.h).

There is no Python or CPU implementation behind this module: if the shared library has not been built
(``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C lorastencil_amd/csrc``) loading fails
loudly, and without a HIP device every compute entry point returns ``LORA_ENODEVICE`` / a HIP error, which
``check()`` raises as ``LoraError``.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The one engine library, in-tree.  (Development tools that A/B two builds assign LIB_PATH before the first lib() call;
# no environment variable can swap the engine under the product.)
LIB_PATH = os.path.join(_HERE, "lib", "liblorastencil_hip.so")

LORA_OK = 0
LORA_EINVAL = -1
LORA_EUNSUPPORTED = -2
LORA_EHIP = -3
LORA_ENOMEM = -4
LORA_ENODEVICE = -5

F64 = 0
BF16 = 1
VARIANT_AUTO, VARIANT_DIRECT, VARIANT_MFMA = 0, 1, 2
BC_REFERENCE, BC_DIRICHLET, BC_PERIODIC = 0, 1, 2

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p


class LoraError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status} ({detail})")


class RunInfo(ctypes.Structure):
    _fields_ = [
        ("sweep_seconds", ctypes.c_double),
        ("total_seconds", ctypes.c_double),
        ("gstencils", ctypes.c_double),
        ("gstencils_refconv", ctypes.c_double),
        ("hbm_gbs", ctypes.c_double),
        ("variant", ctypes.c_int),
        ("steps_per_launch", ctypes.c_int),
    ]


class RunProfile(ctypes.Structure):
    _fields_ = [
        ("fused_launches", ctypes.c_int),
        ("apps_per_fused_launch", ctypes.c_int),
        ("two_launches", ctypes.c_int),
        ("single_launches", ctypes.c_int),
        ("fused_ms", ctypes.c_float),
        ("two_ms", ctypes.c_float),
        ("single_ms", ctypes.c_float),
    ]


class GridStats(ctypes.Structure):
    """lora_grid_stats: statistics of the finite interior cells of a region."""
    _fields_ = [("min", ctypes.c_double), ("max", ctypes.c_double), ("abs_max", ctypes.c_double), ("sum", ctypes.c_double),
                ("sum_sq", ctypes.c_double), ("count", ctypes.c_longlong), ("nonfinite", ctypes.c_longlong)]


class GridDiff(ctypes.Structure):
    """lora_grid_diff: difference of two grids of one plan over a region."""
    _fields_ = [("max_abs", ctypes.c_double), ("sum_sq", ctypes.c_double), ("a_abs_max", ctypes.c_double),
                ("argmax", ctypes.c_longlong), ("count", ctypes.c_longlong), ("nonfinite", ctypes.c_longlong)]


class Until(ctypes.Structure):
    _fields_ = [("tol", ctypes.c_double), ("rtol", ctypes.c_double), ("norm", ctypes.c_int), ("check_every", ctypes.c_int),
                ("max_times", ctypes.c_int)]


class UntilResult(ctypes.Structure):
    _fields_ = [("times_done", ctypes.c_int), ("checks", ctypes.c_int), ("converged", ctypes.c_int), ("diverged", ctypes.c_int),
                ("residual", ctypes.c_double), ("last", GridDiff)]


class GridDot(ctypes.Structure):
    """lora_grid_dot: sum of the finite products of two grids of one plan over a region."""
    _fields_ = [("dot", ctypes.c_double), ("sum_abs", ctypes.c_double), ("count", ctypes.c_longlong), ("nonfinite", ctypes.c_longlong)]


class CgResult(ctypes.Structure):
    _fields_ = [("until", UntilResult), ("lambda_min", ctypes.c_double), ("lambda_max", ctypes.c_double),
                ("rho_estimate", ctypes.c_double), ("breakdown", ctypes.c_int)]


class ThetaResult(ctypes.Structure):
    """lora_theta_result: what a run of the implicit stepper reports."""
    _fields_ = [("steps_done", ctypes.c_int), ("breakdown", ctypes.c_int), ("unconverged_steps", ctypes.c_int),
                ("iterations_total", ctypes.c_longlong), ("iterations_max", ctypes.c_int), ("last_rr0", ctypes.c_double),
                ("last_rr", ctypes.c_double), ("steady", GridDiff)]


class Mg(ctypes.Structure):
    """lora_mg: the shape of a V-cycle."""
    _fields_ = [("pre", ctypes.c_int), ("post", ctypes.c_int), ("omega", ctypes.c_double), ("max_levels", ctypes.c_int),
                ("coarse_iters", ctypes.c_int)]


class MgResult(ctypes.Structure):
    """lora_mg_result: the until-result counted in cycles, and the hierarchy that ran."""
    _fields_ = [("until", UntilResult), ("levels", ctypes.c_int), ("level_dims", (ctypes.c_int * 3) * 16)]


class PcgResult(ctypes.Structure):
    """lora_pcg_result: the until-result counted in iterations, the Ritz values of M A, and the hierarchy's depth."""
    _fields_ = [("until", UntilResult), ("lambda_min", ctypes.c_double), ("lambda_max", ctypes.c_double), ("breakdown", ctypes.c_int),
                ("levels", ctypes.c_int)]


NORM_MAX, NORM_RMS = 0, 1

_comm_begin_t = ctypes.CFUNCTYPE(ctypes.c_int, _vp)
_comm_xfer_t = ctypes.CFUNCTYPE(ctypes.c_int, _vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp)


class SlabComm(ctypes.Structure):
    """lora_slab_comm: the neighbour-exchange callbacks of the C++ slab driver."""
    _fields_ = [("ctx", _vp), ("group_begin", _comm_begin_t), ("send", _comm_xfer_t), ("recv", _comm_xfer_t),
                ("group_end", _comm_begin_t)]


class SlabDesc(ctypes.Structure):
    _fields_ = [("shape", ctypes.c_int), ("dtype", ctypes.c_int), ("global_dims", ctypes.c_int * 3), ("params", _dp),
                ("weights", _dp), ("rank", ctypes.c_int), ("nranks", ctypes.c_int), ("device", ctypes.c_int),
                ("exchange_every", ctypes.c_int), ("boundary", ctypes.c_int), ("flags", ctypes.c_int),
                ("options", ctypes.c_char_p)]


class SlabInfo(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_int), ("end", ctypes.c_int), ("ghost", ctypes.c_int), ("ghost_top", ctypes.c_int),
                ("ghost_bottom", ctypes.c_int), ("apps_per_launch", ctypes.c_int), ("exchange_every", ctypes.c_int),
                ("steps_done", ctypes.c_int), ("local_dims", ctypes.c_int * 3), ("launches", ctypes.c_long),
                ("exchanges", ctypes.c_long), ("local_bytes", ctypes.c_size_t)]


SLAB_NO_OVERLAP, SLAB_NO_DEFER, SLAB_NO_FUSION, SLAB_RING_OF_ONE, SLAB_OVERLAP = 1, 2, 4, 8, 16


class BlockDesc(ctypes.Structure):
    _fields_ = [("shape", ctypes.c_int), ("dtype", ctypes.c_int), ("global_dims", ctypes.c_int * 3), ("grid", ctypes.c_int * 2),
                ("coords", ctypes.c_int * 2), ("params", _dp), ("weights", _dp), ("device", ctypes.c_int),
                ("exchange_every", ctypes.c_int), ("flags", ctypes.c_int), ("options", ctypes.c_char_p)]


class BlockInfo(ctypes.Structure):
    _fields_ = [("own_begin", ctypes.c_int * 2), ("own_end", ctypes.c_int * 2), ("ghost", ctypes.c_int), ("ghost_lo", ctypes.c_int * 2),
                ("ghost_hi", ctypes.c_int * 2), ("apps_per_launch", ctypes.c_int), ("exchange_every", ctypes.c_int),
                ("steps_done", ctypes.c_int), ("local_dims", ctypes.c_int * 3), ("launches", ctypes.c_long),
                ("exchanges", ctypes.c_long), ("local_bytes", ctypes.c_size_t), ("bytes_per_refresh", ctypes.c_size_t)]


class Rng(ctypes.Structure):
    _fields_ = [("r", ctypes.c_int32 * 34), ("pos", ctypes.c_int32)]


# name -> (restype, argtypes): every symbol include/lorastencil.h declares
SIGNATURES = {
    "lora_shape_ntaps": (ctypes.c_int, [ctypes.c_int]),
    "lora_shape_ndim": (ctypes.c_int, [ctypes.c_int]),
    "lora_shape_from_name": (ctypes.c_int, [ctypes.c_char_p]),
    "lora_shape_info_name": (ctypes.c_char_p, [ctypes.c_int]),
    "lora_padded_count": (ctypes.c_size_t, [ctypes.c_int, _ip]),
    "lora_shape_gstencil_factor": (ctypes.c_int, [ctypes.c_int]),
    "lora_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "lora_last_error": (ctypes.c_char_p, []),
    "lora_device_count": (ctypes.c_int, []),
    "lora_gpu_1d1r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_1d2r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_star_2d1r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_star_2d3r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_box_2d3r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_box_3d1r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lora_gpu_star_3d1r": (ctypes.c_int, [_dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lora_run_host": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, ctypes.c_int, _ip, ctypes.c_int,
                                     ctypes.POINTER(RunInfo)]),
    "lora_run_host_dtype": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _dp, ctypes.c_int, _ip, ctypes.c_int,
                                           ctypes.POINTER(RunInfo)]),
    "lora_last_run_info": (ctypes.c_int, [ctypes.POINTER(RunInfo)]),
    "lora_f64_to_bf16": (None, [_dp, ctypes.POINTER(ctypes.c_uint16), ctypes.c_size_t]),
    "lora_bf16_to_f64": (None, [ctypes.POINTER(ctypes.c_uint16), _dp, ctypes.c_size_t]),
    "lora_plan_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, _ip, _dp]),
    "lora_plan_set_weights": (ctypes.c_int, [_vp, _dp, ctypes.c_int]),
    "lora_plan_get_weights": (ctypes.c_int, [_vp, _dp, ctypes.c_int]),
    "lora_plan_set_variant": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_plan_set_boundary": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_set_default_boundary": (ctypes.c_int, [ctypes.c_int]),
    "lora_set_default_normalize": (ctypes.c_int, [ctypes.c_int]),
    "lora_set_default_leap3": (ctypes.c_int, [ctypes.c_int]),
    "lora_set_default_wave3": (ctypes.c_int, [ctypes.c_int]),
    "lora_set_default_coarse1": (ctypes.c_int, [ctypes.c_int]),
    "lora_set_default_mgfuse": (ctypes.c_int, [ctypes.c_int]),
    "lora_plan_set_source": (ctypes.c_int, [_vp, _vp]),
    "lora_set_default_source": (_vp, [_vp]),
    "lora_plan_set_option": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
    "lora_plan_get_option": (ctypes.c_int, [_vp, ctypes.c_char_p, _ip]),
    "lora_plan_kernel_signature": (ctypes.c_char_p, [_vp]),
    "lora_slab_comm_rccl": (ctypes.c_int, [ctypes.POINTER(SlabComm), _vp]),
    "lora_slab_comm_loopback": (ctypes.c_int, [ctypes.POINTER(SlabComm), ctypes.c_int]),
    "lora_slab_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.POINTER(SlabDesc), ctypes.POINTER(SlabComm)]),
    "lora_slab_destroy": (None, [_vp]),
    "lora_slab_info": (ctypes.c_int, [_vp, ctypes.POINTER(SlabInfo)]),
    "lora_slab_load": (ctypes.c_int, [_vp, _vp]),
    "lora_slab_load_device": (ctypes.c_int, [_vp, _vp]),
    "lora_slab_refresh_ghosts": (ctypes.c_int, [_vp]),
    "lora_slab_run": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_slab_sync": (ctypes.c_int, [_vp]),
    "lora_slab_store": (ctypes.c_int, [_vp, _vp]),
    "lora_slab_buffer": (_vp, [_vp, ctypes.c_int]),
    "lora_slab_stream": (_vp, [_vp]),
    "lora_slab_comm_stream": (_vp, [_vp]),
    "lora_slab_plan": (_vp, [_vp]),
    "lora_slab_run_many": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int]),
    "lora_slab_refresh_ghosts_many": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int]),
    "lora_block_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.POINTER(BlockDesc), ctypes.POINTER(SlabComm)]),
    "lora_block_destroy": (None, [_vp]),
    "lora_block_info": (ctypes.c_int, [_vp, ctypes.POINTER(BlockInfo)]),
    "lora_block_load": (ctypes.c_int, [_vp, _vp]),
    "lora_block_run": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_block_run_many": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int]),
    "lora_block_sync": (ctypes.c_int, [_vp]),
    "lora_block_store": (ctypes.c_int, [_vp, _vp]),
    "lora_block_buffer": (_vp, [_vp, ctypes.c_int]),
    "lora_block_stream": (_vp, [_vp]),
    "lora_block_comm_stream": (_vp, [_vp]),
    "lora_block_plan": (_vp, [_vp]),
    "lora_run_host_blocks": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _dp, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int), ctypes.c_int, _vp]),
    "lora_run_host_multi": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _dp, ctypes.c_int, _ip, ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_plan_run_profiled": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.POINTER(RunProfile)]),
    "lora_plan_padded_bytes": (ctypes.c_size_t, [_vp]),
    "lora_plan_kernel_name": (ctypes.c_char_p, [_vp]),
    "lora_plan_step": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "lora_plan_step_region": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_region_granularity": (ctypes.c_int, [_vp]),
    "lora_plan_step2": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "lora_plan_halo": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp]),
    "lora_copy_block_f64": (ctypes.c_int, [_vp, ctypes.c_long, _vp, ctypes.c_long, ctypes.c_long, ctypes.c_long, _vp]),
    "lora_plan_stepk": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "lora_plan_step2_region": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_stepk_region": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_stepn_region": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_prepare_run": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_plan_stepn_region2": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_debug_span_cover": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "lora_debug_cut_cover": (ctypes.c_int, [ctypes.c_int] * 12 + [ctypes.POINTER(ctypes.c_int)] * 4),
    "lora_debug_wg_layout": (ctypes.c_int, [_vp] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)]),
    "lora_plan_run": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp]),
    "lora_plan_stats": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridStats), _vp]),
    "lora_plan_diff": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDiff), _vp]),
    "lora_plan_residual": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDiff), _vp]),
    "lora_plan_residual_src": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDiff), _vp]),
    "lora_debug_residual_cover": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "lora_grid_stats_merge": (None, [ctypes.POINTER(GridStats), ctypes.POINTER(GridStats)]),
    "lora_plan_run_until": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(Until), ctypes.POINTER(UntilResult), _vp]),
    "lora_run_host_until": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _dp, _ip, ctypes.POINTER(Until),
                                           ctypes.POINTER(UntilResult), ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_plan_leapfrog_depth": (ctypes.c_int, [_vp]),
    "lora_plan_step_leapfrog": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    "lora_plan_step_leapfrog_region": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_step2_leapfrog": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, _vp]),
    "lora_plan_step2_leapfrog_region": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_run_leapfrog": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_int, _vp]),
    "lora_plan_prepare_leapfrog": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_plan_step_leapfrog_src": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp]),
    "lora_plan_step_leapfrog_src_region": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                          _vp]),
    "lora_plan_step2_leapfrog_src": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                    ctypes.c_double, _vp]),
    "lora_plan_step2_leapfrog_src_region": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                           ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_run_leapfrog_src": (ctypes.c_int, [_vp, _vp, _vp, _vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_chebyshev_coeffs": (ctypes.c_int, [ctypes.c_double, ctypes.c_int, ctypes.c_int, _dp, _dp]),
    "lora_plan_wave_depth": (ctypes.c_int, [_vp]),
    "lora_plan_step_wave": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp]),
    "lora_plan_step_wave_region": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_step2_wave": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp]),
    "lora_plan_step2_wave_region": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                   _vp]),
    "lora_plan_run_wave": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp]),
    "lora_plan_prepare_wave": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_plan_run_chebyshev_until": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, ctypes.POINTER(Until), ctypes.POINTER(UntilResult),
                                                     _vp]),
    "lora_run_host_chebyshev": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.c_int, ctypes.POINTER(Until),
                                               ctypes.POINTER(UntilResult), _ip, ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_plan_dot": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDot), _vp]),
    "lora_plan_apply_dot": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDot), _vp]),
    "lora_plan_cg_update": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDot), _vp]),
    "lora_plan_cg_direction": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_run_cg_until": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(Until), ctypes.POINTER(CgResult), _vp]),
    "lora_plan_prepare_cg": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_cg_spectrum": (ctypes.c_int, [_dp, _dp, ctypes.c_int, _dp, _dp]),
    "lora_run_host_cg": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.POINTER(Until), ctypes.POINTER(CgResult), _ip, ctypes.c_int,
                                        ctypes.POINTER(RunInfo)]),
    "lora_plan_apply_dot_shift": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(GridDot), _vp]),
    "lora_plan_theta_start": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(GridDot), _vp]),
    "lora_plan_run_theta": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, _ip,
                                           ctypes.POINTER(ThetaResult), _vp]),
    "lora_plan_prepare_theta": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lora_run_host_theta": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_double, _ip, ctypes.c_int, ctypes.POINTER(RunInfo), ctypes.POINTER(ThetaResult)]),
    "lora_mg_coarse_dims": (ctypes.c_int, [ctypes.c_int, _ip, _ip]),
    "lora_mg_coarse_taps": (ctypes.c_int, [ctypes.c_int, _dp, _ip, _ip, _dp]),
    "lora_plan_mg_restrict": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    "lora_plan_mg_prolong_add": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "lora_plan_run_mg_until": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(Mg), ctypes.POINTER(Until), ctypes.POINTER(MgResult), _vp]),
    "lora_plan_prepare_mg": (ctypes.c_int, [_vp, ctypes.POINTER(Mg)]),
    "lora_plan_mg_cycle_cost": (ctypes.c_int, [_vp, _ip, _dp]),
    "lora_run_host_mg": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.POINTER(Mg), ctypes.POINTER(Until), ctypes.POINTER(MgResult),
                                        _ip, ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_plan_defect": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lora_plan_mg_defect_restrict": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_double, _vp]),
    "lora_plan_cg_small": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "lora_plan_mg_precondition": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(Mg), ctypes.c_double, ctypes.c_double, _vp]),
    "lora_plan_run_pcg_until": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(Mg), ctypes.POINTER(Until), ctypes.POINTER(PcgResult), _vp]),
    "lora_plan_prepare_pcg": (ctypes.c_int, [_vp, ctypes.POINTER(Mg), ctypes.c_int]),
    "lora_plan_run_theta_mg": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                              ctypes.POINTER(Mg), ctypes.c_int, _ip, ctypes.POINTER(ThetaResult), _vp]),
    "lora_run_host_pcg": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.POINTER(Mg), ctypes.POINTER(Until), ctypes.POINTER(PcgResult),
                                         _ip, ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_run_host_theta_mg": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_double, ctypes.POINTER(Mg), ctypes.c_int, _ip, ctypes.c_int, ctypes.POINTER(RunInfo),
                                              ctypes.POINTER(ThetaResult)]),
    "lora_run_host_leapfrog": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.c_int, _ip, ctypes.c_int,
                                              ctypes.POINTER(RunInfo)]),
    "lora_run_host_wave": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                          _ip, ctypes.c_int, ctypes.POINTER(RunInfo)]),
    "lora_plan_destroy": (None, [_vp]),
    "lora_default_params": (ctypes.c_int, [ctypes.c_int, _dp]),
    "lora_effective_weights": (ctypes.c_int, [ctypes.c_int, _dp, _dp]),
    "lora_factorize_7x7": (ctypes.c_int, [_dp, _dp, _dp, _dp]),
    "lora_svd_7x7": (ctypes.c_int, [_dp, _dp, _dp, _dp]),
    "lora_separable_3x3x3": (ctypes.c_int, [_dp, ctypes.POINTER(ctypes.c_float)]),
    "lora_rng_seed": (None, [ctypes.POINTER(Rng), ctypes.c_uint]),
    "lora_rng_next": (ctypes.c_int, [ctypes.POINTER(Rng)]),
    "lora_fill_rand": (None, [_dp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Rng)]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """The loaded engine; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP engine first (python -c 'import __graft_entry__ as g; "
                f"g.build()' or make -C lorastencil_amd/csrc).  lorastencil_amd has no CPU fallback."
            )
        # PyTorch-ROCm ships its own libamdhip64; if this library pulled in the system one first and torch loaded
        # its copy afterwards, the process would hold two HIP runtimes and the second sees no device.  Import torch
        # first wherever it is installed, so that both bind to the same runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status: int, where: str) -> None:
    if status != LORA_OK:
        L = lib()
        detail = L.lora_strerror(status).decode()
        last = L.lora_last_error().decode()
        raise LoraError(status, where, f"{detail}; {last}" if last else detail)
