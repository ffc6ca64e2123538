"""ctypes binding of libtopolow_relax.so (include/topolow_relax.h) -- the MI355X native path.

This is the Python twin of the R `.Call` shim: it hands the `.Call` payload of
`optimize_layout_exact_cpp` (reference R/RcppExports.R:4-6) to the HIP library.  There is
NO fallback: if the library is missing or no HIP device is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libtopolow_relax.so")

SCHEDULE_AUTO, SCHEDULE_SLAB, SCHEDULE_GS = 0, 1, 2
PRECISION_AUTO, PRECISION_F32, PRECISION_F64, PRECISION_F64_EXACT = 0, 1, 2, 3

FAR_F32 = 1.0e18   # phantom coordinate of padding points (relax_common.h)

OK = 0
ERR_TOO_FEW_POINTS, ERR_NONFINITE, ERR_BAD_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, \
    ERR_INTERRUPTED = 1, 2, 3, 4, 5, 6, 7


class NativeError(RuntimeError):
    """An error raised by libtopolow_relax (the R shim turns these into R errors)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


INTERRUPT_CB = C.CFUNCTYPE(C.c_int32, C.c_void_p)
PRINT_CB = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)

# The C types of include/topolow_relax.h, as the structs and the prototype table below spell them.
INT, I32, U32, I64, U64, F64 = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_double
dp, ip, i64p, u64p = C.POINTER(F64), C.POINTER(I32), C.POINTER(I64), C.POINTER(U64)
i8p, u8p = C.POINTER(C.c_int8), C.POINTER(C.c_uint8)
vp = C.c_void_p            # a host pointer the binding does not look into: a session, a prepared handle, a stream
vpp = C.POINTER(vp)
devp = C.c_void_p          # a device address: it travels as a Python int, whatever the header's pointee type
ERR = (C.c_char_p, C.c_size_t)   # the trailing `char* errbuf, size_t errlen` of most entries (_call supplies them)


class TopolowOptions(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("schedule", C.c_int32), ("precision", C.c_int32),
                ("slab_stages", C.c_int32), ("device", C.c_int32), ("gs_max_n", C.c_int32),
                ("n_devices", C.c_int32), ("keep_labels", C.c_int32), ("reserved", C.c_int32 * 3),
                ("interrupt_cb", INTERRUPT_CB), ("interrupt_user", C.c_void_p),
                ("print_cb", PRINT_CB), ("print_user", C.c_void_p), ("devices", ip)]


class TopolowRunStats(C.Structure):
    _fields_ = [("schedule_used", C.c_int32), ("precision_used", C.c_int32),
                ("iterations_run", C.c_int32), ("n_checks", C.c_int32),
                ("device_seconds", C.c_double), ("total_seconds", C.c_double),
                ("stage_launches", C.c_int64), ("setup_seconds", C.c_double), ("reserved", C.c_int64 * 3)]


class TopolowShardStats(C.Structure):
    _fields_ = [("blocks", C.c_int32), ("iterations_run", C.c_int32), ("n_checks", C.c_int32),
                ("groups", C.c_int32), ("loop_seconds", C.c_double), ("total_seconds", C.c_double),
                ("stage_kernel_seconds", C.c_double), ("check_kernel_seconds", C.c_double),
                ("stage_launches", C.c_int64), ("exchanges", C.c_int64), ("warmup_iterations", C.c_int32),
                ("symmetric_segments", C.c_int32), ("timed_seconds", C.c_double), ("reserved", C.c_int64 * 2)]


class TopolowProblem(C.Structure):
    _fields_ = [("initial_positions", dp), ("dissimilarity_matrix", dp),
                ("threshold_matrix", ip), ("degrees", ip),
                ("edge_i", ip), ("edge_j", ip),
                ("edge_dist", dp), ("edge_thresh", ip),
                ("n_edges", C.c_int64), ("n", C.c_int32), ("ndim", C.c_int32), ("n_iter", C.c_int32),
                ("convergence_window", C.c_int32), ("convergence_check_freq", C.c_int32),
                ("reserved0", C.c_int32), ("k0", C.c_double), ("cooling_rate", C.c_double),
                ("c_repulsion", C.c_double), ("relative_epsilon", C.c_double), ("seed", C.c_uint64),
                ("holdout_i", ip), ("holdout_j", ip),
                ("holdout_truth", dp), ("n_holdout", C.c_int64)]


class TopolowCellList(C.Structure):
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("n_cells", C.c_int64),
                ("row", ip), ("col", ip),
                ("value", dp), ("code", ip),
                ("pos_of", i64p), ("by_row", i64p),
                ("row_ptr", i64p)]


PRUNE_MAX_ATTEMPTS = 10   # TOPOLOW_PRUNE_MAX_ATTEMPTS


class TopolowLayoutPrepInfo(C.Structure):
    _fields_ = [("n_edges", C.c_int64), ("n_finite_nonzero", C.c_int64), ("n_infinite", C.c_int64),
                ("n_negative", C.c_int64), ("numeric_max", C.c_double), ("reordered", C.c_int32),
                ("order_route", C.c_int32), ("exact_sums", C.c_int32), ("reserved", C.c_int32 * 5)]


class TopolowSpectrumInfo(C.Structure):
    _fields_ = [("median", C.c_double), ("n_numeric", C.c_int64), ("n_filled", C.c_int64), ("trace", C.c_double),
                ("n_positive", C.c_int64), ("n_negative", C.c_int64), ("sum_positive", C.c_double),
                ("sum_negative", C.c_double), ("deviation_score", C.c_double), ("dims_90", C.c_int32),
                ("reserved32", C.c_int32), ("seconds", C.c_double * 4), ("reserved", C.c_int64 * 4)]


FIT_IN, FIT_OUT, FIT_ALL = 0, 1, 2   # TOPOLOW_FIT_*
FIT_MAX_RANKS = 8                     # TOPOLOW_FIT_MAX_RANKS
FIT_RANK_UPPER = 1 << 32              # TOPOLOW_FIT_RANK_UPPER
_FIT_SERIES = {"in": FIT_IN, "out": FIT_OUT, "all": FIT_ALL, FIT_IN: FIT_IN, FIT_OUT: FIT_OUT, FIT_ALL: FIT_ALL}
FIT_AXIS_TRUE, FIT_AXIS_PREDICTED, FIT_AXIS_ERROR, FIT_AXIS_RESIDUAL = 0, 1, 2, 3   # TOPOLOW_FIT_AXIS_*
FIT_AXES = ("true", "predicted", "error", "residual")   # v, r, v - r, r - v
FIT_MAX_BINS = 8192                   # TOPOLOW_FIT_MAX_BINS
FIT_MAX_GRID = 4096                   # TOPOLOW_FIT_MAX_GRID
_FIT_AXIS = {**{name: k for k, name in enumerate(FIT_AXES)}, **{k: k for k in range(4)}}


class TopolowFitSeries(C.Structure):
    _fields_ = [("count", C.c_int64), ("sum_e", C.c_double), ("sum_abs_e", C.c_double), ("min_e", C.c_double),
                ("max_e", C.c_double), ("pct_count", C.c_int64), ("sum_pct", C.c_double), ("sum_abs_pct", C.c_double),
                ("sum_v", C.c_double), ("sum_r", C.c_double), ("css_e", C.c_double), ("css_v", C.c_double),
                ("css_r", C.c_double), ("css_vr", C.c_double)]


class TopolowFitReport(C.Structure):
    _fields_ = [("series", TopolowFitSeries * 3), ("seconds", C.c_double * 3), ("reserved", C.c_int64 * 4)]


class TopolowPruneInfo(C.Structure):
    _fields_ = [("original_size", C.c_int32), ("final_size", C.c_int32), ("iterations", C.c_int32),
                ("min_connections_used", C.c_int32), ("attempts", C.c_int32), ("stop_reason", C.c_int32),
                ("target_reached", C.c_int32), ("last_remove", C.c_int32), ("original_cells", C.c_int64),
                ("final_cells", C.c_int64), ("seconds", C.c_double * 3),
                ("attempt_iterations", C.c_int32 * PRUNE_MAX_ATTEMPTS), ("attempt_stop_reason", C.c_int32 * PRUNE_MAX_ATTEMPTS),
                ("attempt_last_remove", C.c_int32 * PRUNE_MAX_ATTEMPTS), ("attempt_final_size", C.c_int32 * PRUNE_MAX_ATTEMPTS),
                ("attempt_final_cells", C.c_int64 * PRUNE_MAX_ATTEMPTS), ("reserved", C.c_int64 * 4)]


class TopolowResult(C.Structure):
    _fields_ = [("positions_out", dp), ("final_mae", C.c_double),
                ("final_k", C.c_double), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("iterations_run", C.c_int32), ("n_checks", C.c_int32), ("error_code", C.c_int32),
                ("error_iteration", C.c_int32), ("holdout_sum_abs", C.c_double),
                ("holdout_count", C.c_int64)]


# Additive backend options (the reference's function signatures stay untouched; this mirrors
# what an R user would set through options(topolow.*)).
options: Dict[str, Any] = dict(seed=None, schedule="auto", precision="auto", slab_stages=0,
                               device=-1, gs_max_n=0)
_host_rng = np.random.default_rng()

_SCHEDULES = {"auto": SCHEDULE_AUTO, "slab": SCHEDULE_SLAB, "gs": SCHEDULE_GS}
_PRECISIONS = {"auto": PRECISION_AUTO, "f32": PRECISION_F32, "f64": PRECISION_F64, "f64_exact": PRECISION_F64_EXACT}
_PRECISION_NAMES = {v: k for k, v in _PRECISIONS.items() if k != "auto"}


def set_seed(seed: Optional[int]) -> None:
    """The Python spelling of R's `set.seed(seed)`: the random-walk initial positions are then drawn
    from R's own Mersenne-Twister stream (topolow_amd/r_rng.py), i.e. they equal what the reference
    computes after `set.seed(seed)` (R/core.R:412); the native pair/slab order seed is the next draw
    of the same stream, so the whole run is reproducible (the reference's shuffle is not: it is
    seeded from std::random_device, src/optimization.cpp:153-154).  set_seed(None) returns to
    OS entropy."""
    global _host_rng
    options["seed"] = None
    if seed is None:
        _host_rng = np.random.default_rng()
    else:
        from .r_rng import RUnif
        _host_rng = RUnif(int(seed))


def host_rng() -> np.random.Generator:
    return _host_rng


optionsp, run_statsp, shard_statsp = C.POINTER(TopolowOptions), C.POINTER(TopolowRunStats), C.POINTER(TopolowShardStats)
problemp, resultp, cellsp = C.POINTER(TopolowProblem), C.POINTER(TopolowResult), C.POINTER(TopolowCellList)
prep_infop, prune_infop = C.POINTER(TopolowLayoutPrepInfo), C.POINTER(TopolowPruneInfo)
spectrump, fit_reportp = C.POINTER(TopolowSpectrumInfo), C.POINTER(TopolowFitReport)

# Every function include/topolow_relax.h declares, in the header's order: name -> (restype, argtypes).
# tests/test_native_prototypes.py compares each entry with the header, type by type.
PROTOTYPES = {
    # ---- the `.Call` payload: one embedding, a batch of them
    "topolow_default_options": (None, (optionsp,)),
    "topolow_optimize_layout_exact": (INT, (dp, I32, I32, dp, ip, ip, ip, ip, dp, ip, I64, I32, F64, F64, F64, F64, I32, I32,
                                            I32, optionsp, dp, ip, ip, dp, dp, run_statsp, *ERR)),
    "topolow_optimize_layout_exact_batch": (INT, (problemp, resultp, I32, I32, I32, dp, *ERR)),
    # ---- cross-validation from a cell list
    "topolow_cell_list_index": (INT, (I32, I64, ip, ip, i64p, i64p, i64p)),
    "topolow_cv_fold": (INT, (cellsp, i64p, I64, I32, I32, ip, ip, ip, ip, dp, ip, i64p, ip, ip, dp, i64p, dp)),
    "topolow_cv_sweep": (INT, (cellsp, I32, I32, I32, ip, dp, dp, dp, i64p, i64p, dp, i64p, u64p, I32, F64, I32, I32, I32,
                               I32, dp, i64p, ip, ip, ip, dp, *ERR)),
    "topolow_batch_problem_fits": (I32, (I32, I32, I32, I64)),
    "topolow_cv_fold_pairs": (INT, (cellsp, i64p, I64, I32, I32, ip, ip, dp, i64p, ip, ip, i64p, ip, ip, dp, i64p, *ERR)),
    "topolow_cv_sweep_session": (INT, (cellsp, I32, I32, I32, ip, dp, dp, dp, i64p, i64p, dp, i64p, u64p, I32, F64, I32,
                                       I32, I32, I32, I32, dp, i64p, ip, ip, ip, dp, *ERR)),
    # ---- post-processing: distances, metrics, velocity
    "topolow_est_distances": (INT, (dp, I32, I32, dp, I32, *ERR)),
    "topolow_est_distances_rows": (INT, (dp, I32, I32, I32, I32, dp, I32, *ERR)),
    "topolow_post_metrics": (INT, (dp, I32, I32, dp, ip, dp, dp, i64p, I32, *ERR)),
    "topolow_post_metrics_ex": (INT, (dp, I32, I32, dp, ip, dp, dp, i64p, I32, I32, dp, *ERR)),
    "topolow_kernel_velocity": (INT, (dp, dp, I32, I32, F64, F64, u64p, dp, dp, I32, *ERR)),
    "topolow_kernel_velocity_ex": (INT, (dp, dp, I32, I32, F64, F64, u64p, dp, dp, I32, I32, dp, *ERR)),
    "topolow_scale_objective": (INT, (dp, dp, I32, I32, I32, dp, I32, dp, dp, dp, I32, *ERR)),
    "topolow_scale_objective_ex": (INT, (dp, dp, I32, I32, I32, dp, I32, dp, dp, dp, I32, I32, dp, *ERR)),
    "topolow_scale_to_original_distances": (INT, (dp, dp, I32, I32, I32, F64, F64, F64, dp, dp, ip, dp, dp, I32, I32, *ERR)),
    # ---- prepared layout: a matrix that stays on the device
    "topolow_layout_prep_create": (INT, (vpp, dp, i8p, I32, I32, I32, ip, I32, prep_infop, *ERR)),
    "topolow_layout_prep_fetch": (INT, (vp, ip, ip, ip, ip, dp, ip, dp, ip, dp, i8p, *ERR)),
    "topolow_layout_prep_destroy": (None, (vp,)),
    "topolow_layout_prep_phase_seconds": (INT, (vp, dp)),
    "topolow_session_load_prepared": (INT, (vp, vp, *ERR)),
    "topolow_layout_prep_optimize": (INT, (vp, dp, I32, I32, F64, F64, F64, F64, I32, I32, I32, optionsp, dp, ip, ip, dp, dp,
                                           run_statsp, *ERR)),
    "topolow_layout_prep_post_metrics": (INT, (vp, dp, I32, dp, dp, i64p, *ERR)),
    "topolow_layout_prep_order": (INT, (vp, ip, ip)),
    "topolow_layout_prep_resident_seconds": (INT, (vp, dp)),
    "topolow_layout_order_from_sums": (I32, (I32, dp, i64p, dp, i64p, I32, ip)),
    "topolow_layout_prep_fold": (INT, (vp, i64p, I64, I32, I32, ip, ip, dp, i64p, ip, ip, i64p, ip, ip, dp, i64p, ip, *ERR)),
    "topolow_layout_prep_cv_sweep": (INT, (vp, I32, I32, I32, ip, dp, dp, dp, i64p, i64p, dp, i64p, u64p, I32, F64, I32,
                                           I32, I32, I32, dp, i64p, ip, ip, ip, ip, dp, *ERR)),
    "topolow_layout_prep_fold_seconds": (INT, (vp, dp)),
    "topolow_layout_prep_connectivity": (INT, (vp, ip, I32, ip, i64p, ip, *ERR)),
    "topolow_layout_prep_subsample": (INT, (vp, ip, I32, I32, ip, vpp, prep_infop, *ERR)),
    "topolow_layout_prep_graph_stats": (INT, (vp, ip, dp)),
    "topolow_layout_prep_degrees": (INT, (vp, ip, I32, ip, i64p, *ERR)),
    "topolow_layout_prep_prune": (INT, (vp, I32, F64, I32, I32, u8p, prune_infop, *ERR)),
    "topolow_tridiagonal_eigenvalues": (INT, (dp, dp, I32, I32, dp, *ERR)),
    "topolow_symmetric_eigenvalues": (INT, (dp, I32, I32, dp, dp, dp, *ERR)),   # its d_out is the diagonal, host memory
    "topolow_layout_prep_spectrum": (INT, (vp, dp, dp, spectrump, *ERR)),
    "topolow_layout_prep_fit_report": (INT, (vp, dp, I32, i64p, I64, fit_reportp, *ERR)),
    "topolow_layout_prep_fit_order_stats": (INT, (vp, dp, I32, i64p, I64, I32, i64p, I32, dp, i64p, *ERR)),
    "topolow_layout_prep_fit_extent": (INT, (vp, dp, I32, i64p, I64, I32, dp, i64p, *ERR)),
    "topolow_layout_prep_fit_hist2d": (INT, (vp, dp, I32, i64p, I64, I32, I32, dp, I32, I32, dp, I32, i64p, i64p, i64p, *ERR)),
    "topolow_layout_prep_fit_linear_bins": (INT, (vp, dp, I32, i64p, I64, I32, I32, F64, F64, I32, i64p, u64p, i64p, i64p,
                                                  *ERR)),
    # ---- session: a device-resident run
    "topolow_session_create": (INT, (vpp, I32, I32, I32, I32, I32, I32, *ERR)),
    "topolow_session_destroy": (None, (vp,)),
    "topolow_session_set_relabel": (INT, (vp, U64, *ERR)),
    "topolow_session_labels": (INT, (vp, ip)),
    "topolow_session_load_dense": (INT, (vp, dp, ip, ip, *ERR)),
    "topolow_session_load_coo": (INT, (vp, ip, ip, dp, ip, I64, ip, *ERR)),
    "topolow_session_encoded_ptr": (devp, (vp,)),
    "topolow_session_encoded_ld": (I32, (vp,)),
    "topolow_session_commit_encoded": (INT, (vp, ip, *ERR)),
    "topolow_session_set_edges": (INT, (vp, ip, ip, dp, ip, I64, *ERR)),
    "topolow_session_set_positions": (INT, (vp, dp, *ERR)),
    "topolow_session_get_positions": (INT, (vp, dp, *ERR)),
    "topolow_session_begin": (INT, (vp, I32, F64, F64, F64, F64, I32, I32, U64, I32, *ERR)),
    "topolow_session_enqueue": (INT, (vp, I32, ip, *ERR)),
    "topolow_session_wait": (INT, (vp, *ERR)),
    "topolow_session_sync": (INT, (vp, ip, ip, dp, *ERR)),
    "topolow_session_finish": (INT, (vp, dp, ip, ip, dp, dp, *ERR)),
    "topolow_session_check_trace": (INT, (vp, dp, I32, ip)),
    "topolow_session_hold_out": (INT, (vp, ip, ip, I64, ip, *ERR)),
    "topolow_session_restore_held_out": (INT, (vp, ip, *ERR)),
    "topolow_session_score_pairs": (INT, (vp, ip, ip, dp, I64, dp, i64p, *ERR)),
    "topolow_session_set_profiling": (INT, (vp, I32)),
    "topolow_session_profile_fused": (INT, (vp, dp, i64p, *ERR)),
    "topolow_session_profile_symmetric": (INT, (vp, dp, i64p, dp, i64p, *ERR)),
    "topolow_session_profile": (INT, (vp, dp, i64p, dp, i64p, *ERR)),
    "topolow_session_set_stream": (INT, (vp, vp, I32)),
    "topolow_session_stream": (devp, (vp,)),
    "topolow_session_uses_dense_mae": (I32, (vp,)),
    "topolow_session_stage_launches": (I64, (vp,)),
    "topolow_session_checks_in_apply": (I64, (vp,)),
    "topolow_session_bytes_per_iteration": (I64, (vp,)),
    "topolow_session_set_schedule": (INT, (vp, I32)),
    "topolow_tilegs_pair_order": (I64, (I32, U64, I32, ip)),
    "topolow_session_position_rows": (I32, (vp,)),
    "topolow_session_position_dim": (I32, (vp,)),
    "topolow_session_stage": (INT, (vp, devp, devp, I32, I32, I32, F64, *ERR)),
    "topolow_session_check_partial": (INT, (vp, devp, devp, *ERR)),
    "topolow_session_controller_step": (INT, (vp, devp, devp, I32, F64, *ERR)),
    "topolow_session_can_fuse_checks": (I32, (vp,)),
    "topolow_session_stage_fused": (INT, (vp, devp, devp, I32, F64, devp, *ERR)),
    "topolow_symm_segment_rows": (I32, (I32, I32, I32, ip, ip)),
    "topolow_session_symm_segment_eligible": (I32, (vp, I32)),
    "topolow_session_can_fuse_segment_checks": (I32, (vp,)),
    "topolow_session_degree_terms": (devp, (vp,)),
    "topolow_session_has_thresholds": (I32, (vp,)),
    "topolow_session_symm_segment_build": (INT, (vp, I32, I32, devp, I32, I32, I32, *ERR)),
    "topolow_session_symm_moves": (devp, (vp,)),
    "topolow_session_symm_segment_sweep": (INT, (vp, devp, I32, F64, devp, *ERR)),
    "topolow_session_symm_segment_apply": (INT, (vp, devp, devp, I32, *ERR)),
    "topolow_session_first_nonfinite": (INT, (vp, ip)),
    "topolow_session_edge_error": (INT, (vp, devp, dp, i64p, *ERR)),
    # ---- one embedding row-sharded over sessions
    "topolow_shard_rows": (I32, (I32, I32, I32, ip, ip)),
    "topolow_optimize_layout_exact_sharded": (INT, (dp, I32, I32, dp, ip, ip, ip, ip, dp, ip, I64, I32, F64, F64, F64, F64,
                                                    I32, I32, I32, optionsp, dp, ip, ip, dp, dp, shard_statsp, *ERR)),
    "topolow_sessions_run_sharded": (INT, (vpp, I32, dp, I32, F64, F64, F64, F64, I32, I32, U64, I32, INTERRUPT_CB, vp, I32,
                                           dp, ip, ip, dp, dp, shard_statsp, *ERR)),
    # ---- plans and host-side helpers (no device)
    "topolow_slab_plan": (I32, (I32, I32, U64, I32, ip, I32)),
    "topolow_slab_stages_for_k": (I32, (F64, I32)),
    "topolow_symm_stage_bounds": (I32, (I32, I32, ip)),
    "topolow_symm_stage_order": (I32, (U64, I32, I32, ip)),
    "topolow_symm_stage_rows": (I32, (I32, I32, I32, ip)),
    "topolow_symm_plan": (I32, (I32, I32, I32, I32, I32, I32, ip, I32, ip)),
    "topolow_session_symm_grid": (I32, (vp,)),
    "topolow_slab_stages_at": (I32, (I32, F64, I32)),
    "topolow_gs_pair_order": (I64, (I32, U64, I32, ip)),
    "topolow_encode_target": (U32, (F64, I32)),
    "topolow_encoded_index": (I64, (I32, I32, I32)),
    "topolow_decode_target": (F64, (U32, ip)),
    "topolow_controller_script": (INT, (dp, ip, dp, I32, F64, I32, F64, ip, ip, dp, dp, ip)),
    "topolow_relax_version": (C.c_char_p, ()),
}

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C topolow_amd/csrc`. topolow_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib


_PTR = {np.dtype(t): p for t, p in ((np.float64, dp), (np.int32, ip), (np.int64, i64p), (np.uint64, u64p), (np.int8, i8p),
                                    (np.uint8, u8p))}


def _ptr(a):
    """The typed pointer to an array's data, chosen by its dtype; None stays None (a NULL argument)."""
    if a is None:
        return None
    if a.dtype not in _PTR:
        raise TypeError(f"no pointer type for an array of {a.dtype}")
    return a.ctypes.data_as(_PTR[a.dtype])


_dp = _ip = _ptr   # thin names: tests/test_*_capi.py build their double / int32 arguments with them


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f64F(a):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["F", "A"])


def _i32F(a):
    return np.require(np.asarray(a, dtype=np.int32), requirements=["F", "A"])


def _check(rc: int, err=None) -> None:
    if rc != OK:
        message = err.value.decode(errors="replace") if err is not None else ""
        raise NativeError(rc, message or f"libtopolow_relax error {rc}")


def _call(fn, *args, err=None) -> None:
    """Calls an entry that ends in `errbuf, errlen` (ERR in PROTOTYPES) and raises its message as a NativeError.
    `err`: the buffer a Session / PreparedHandle owns; without one the call gets a fresh buffer."""
    if err is None:
        err = C.create_string_buffer(512)
    _check(fn(*args, err, len(err)), err)


def _fields(s) -> Dict[str, Any]:
    """The fields of a ctypes struct as a dict, the reserved ones left out."""
    return {k: getattr(s, k) for k, _ in s._fields_ if not k.startswith("reserved")}


class _RunOut:
    """The five outputs every relaxation entry ends with (positions_out, converged, iterations, final_mae, final_k):
    `.args` go into the call, `.result(info)` reads them back.  positions=False: NULL, nothing is downloaded."""

    def __init__(self, n, dim, positions=True):
        self.out = np.zeros((n, dim), dtype=np.float64, order="F") if positions else None
        self.conv, self.iters, self.fmae, self.fk = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        self.args = (_ptr(self.out), C.byref(self.conv), C.byref(self.iters), C.byref(self.fmae), C.byref(self.fk))

    def result(self, info=None) -> "NativeResult":
        return NativeResult(None if self.out is None else np.ascontiguousarray(self.out), bool(self.conv.value),
                            int(self.iters.value), float(self.fmae.value), float(self.fk.value),
                            {} if info is None else info)


class _SumCount:
    """k (double, int64) output pairs -- a (sum, count), a profile's (ms, launches) pairs: `.refs` go into the call,
    `.values()` reads them back as one flat tuple."""

    def __init__(self, k=1):
        self.cells = [c for _ in range(k) for c in (C.c_double(0.0), C.c_int64(0))]
        self.refs = [C.byref(c) for c in self.cells]

    def values(self):
        return tuple(c.value for c in self.cells)


def make_options(**kw) -> TopolowOptions:
    lib = load()
    o = TopolowOptions()
    lib.topolow_default_options(C.byref(o))
    cfg = dict(options)
    cfg.update({k: v for k, v in kw.items() if v is not None})
    seed = cfg.get("seed")
    if seed is None:
        seed = int(_host_rng.integers(0, 2 ** 63 - 1))
    o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    sch = cfg.get("schedule", "auto")
    o.schedule = _SCHEDULES[sch] if isinstance(sch, str) else int(sch)
    pr = cfg.get("precision", "auto")
    o.precision = _PRECISIONS[pr] if isinstance(pr, str) else int(pr)
    o.slab_stages = int(cfg.get("slab_stages", 0) or 0)
    o.device = int(cfg.get("device", -1))
    o.gs_max_n = int(cfg.get("gs_max_n", 0) or 0)
    o.keep_labels = int(bool(cfg.get("keep_labels", False)))
    cb = cfg.get("interrupt")
    if cb is not None:   # Python callable() -> truthy to stop; keep a reference alive on the struct
        o._cb_keepalive = INTERRUPT_CB(lambda _user: 1 if cb() else 0)
        o.interrupt_cb = o._cb_keepalive
    pr = cfg.get("print")
    if pr is not None:   # Python callable(str): receives the verbose lines instead of stdout
        o._pr_keepalive = PRINT_CB(lambda line, _user: pr(line.decode(errors="replace")))
        o.print_cb = o._pr_keepalive
    devs = cfg.get("devices")
    if devs is not None:   # row-block sharded over these HIP ordinals (repeats allowed)
        o._dev_keepalive = (C.c_int32 * len(devs))(*[int(d) for d in devs])
        o.devices = C.cast(o._dev_keepalive, ip)
        o.n_devices = len(devs)
    return o


@dataclass
class NativeResult:
    positions: np.ndarray
    converged: bool
    iterations: int
    final_mae: float
    final_k: float
    info: Dict[str, Any] = field(default_factory=dict)


def optimize_layout_exact_arrays(initial_positions, dissimilarity_matrix, threshold_matrix,
                                 degrees, edge_i, edge_j, edge_dist, edge_thresh, n_iter, k0,
                                 cooling_rate, c_repulsion, relative_epsilon, convergence_window,
                                 convergence_check_freq, verbose=False, **opt_kw) -> NativeResult:
    """`optimize_layout_exact_cpp(...)` (reference src/optimization.cpp:109-126) on the GPU."""
    lib = load()
    pos0 = _f64F(initial_positions)
    n, dim = pos0.shape
    D = _f64F(dissimilarity_matrix)
    T = _i32F(threshold_matrix)
    deg, ei, ej, ed, et = _i32(degrees), _i32(edge_i), _i32(edge_j), _f64(edge_dist), _i32(edge_thresh)
    out, stats = _RunOut(n, dim), TopolowRunStats()
    opt = make_options(**opt_kw)
    _call(lib.topolow_optimize_layout_exact,
          _ptr(pos0), n, dim, _ptr(D), _ptr(T), _ptr(deg), _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et),
          int(ei.shape[0]), int(n_iter), float(k0), float(cooling_rate), float(c_repulsion),
          float(relative_epsilon), int(convergence_window), int(convergence_check_freq),
          int(bool(verbose)), C.byref(opt), *out.args, C.byref(stats))
    return out.result(_run_info(stats, opt))


def _run_info(stats: TopolowRunStats, opt: TopolowOptions) -> Dict[str, Any]:
    return dict(schedule={SCHEDULE_SLAB: "slab", SCHEDULE_GS: "gs"}.get(stats.schedule_used),
                precision=_PRECISION_NAMES.get(stats.precision_used),
                iterations_run=stats.iterations_run, n_checks=stats.n_checks,
                device_seconds=stats.device_seconds, total_seconds=stats.total_seconds,
                setup_seconds=stats.setup_seconds, stage_launches=stats.stage_launches, seed=int(opt.seed))


def optimize_layout_exact(call) -> NativeResult:
    """Takes a core.LayoutCall."""
    return optimize_layout_exact_arrays(
        call.initial_positions, call.dissimilarity_matrix, call.threshold_matrix, call.degrees,
        call.edge_i, call.edge_j, call.edge_dist, call.edge_thresh, call.n_iter, call.k0,
        call.cooling_rate, call.c_repulsion, call.relative_epsilon, call.convergence_window,
        call.convergence_check_freq, call.verbose)


def optimize_layout_exact_batch(calls, seeds=None, precision="f64", device=-1, holdouts=None):
    """Relaxes a list of calls as ONE grid of the exact-GS kernel (one workgroup per embedding).
    A call is a core.LayoutCall, or any object with the same fields whose `dissimilarity_matrix` is
    None: its edge list then IS the matrix (every unlisted pair unmeasured) and no n x n array is
    built or uploaded.  `holdouts[b]` = (i, j, truth) arrays of held-out pairs to score on the
    returned positions (info["holdout_sum_abs"], info["holdout_count"]).
    Returns (list of NativeResult-or-NativeError, device_seconds)."""
    lib = load()
    count = len(calls)
    probs = (TopolowProblem * count)()
    ress = (TopolowResult * count)()
    keep = []
    outs = []
    for b, c in enumerate(calls):
        pos0 = _f64F(c.initial_positions)
        n, dim = pos0.shape
        deg, ei, ej, ed, et = _i32(c.degrees), _i32(c.edge_i), _i32(c.edge_j), _f64(c.edge_dist), _i32(c.edge_thresh)
        out = np.zeros((n, dim), dtype=np.float64, order="F")
        p = probs[b]
        if c.dissimilarity_matrix is not None:
            D, T = _f64F(c.dissimilarity_matrix), _i32F(c.threshold_matrix)
            p.dissimilarity_matrix, p.threshold_matrix = _ptr(D), _ptr(T)
            keep.append((D, T))
        keep.append((pos0, deg, ei, ej, ed, et))
        outs.append(out)
        p.initial_positions = _ptr(pos0)
        p.degrees, p.edge_i, p.edge_j, p.edge_dist, p.edge_thresh = _ptr(deg), _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et)
        p.n_edges, p.n, p.ndim, p.n_iter = int(ei.shape[0]), n, dim, int(c.n_iter)
        p.convergence_window, p.convergence_check_freq = int(c.convergence_window), int(c.convergence_check_freq)
        p.k0, p.cooling_rate, p.c_repulsion = float(c.k0), float(c.cooling_rate), float(c.c_repulsion)
        p.relative_epsilon = float(c.relative_epsilon)
        p.seed = int(seeds[b] if seeds is not None else _host_rng.integers(0, 2 ** 63 - 1)) & 0xFFFFFFFFFFFFFFFF
        if holdouts is not None and holdouts[b] is not None and len(holdouts[b][0]) > 0:
            hi, hj, ht = _i32(holdouts[b][0]), _i32(holdouts[b][1]), _f64(holdouts[b][2])
            keep.append((hi, hj, ht))
            p.holdout_i, p.holdout_j, p.holdout_truth, p.n_holdout = _ptr(hi), _ptr(hj), _ptr(ht), int(hi.shape[0])
        ress[b].positions_out = _ptr(out)
    secs = C.c_double(0.0)
    _call(lib.topolow_optimize_layout_exact_batch, probs, ress, count, _PRECISIONS[precision], int(device), C.byref(secs))
    results = []
    for b in range(count):
        r = ress[b]
        if r.error_code != OK:
            results.append(NativeError(r.error_code, "Numerical instability at iteration %d. Reduce k0 or "
                                                     "c_repulsion." % r.error_iteration))
        else:
            results.append(NativeResult(np.ascontiguousarray(outs[b]), bool(r.converged), int(r.iterations),
                                        float(r.final_mae), float(r.final_k),
                                        dict(schedule="gs", precision=precision, iterations_run=r.iterations_run,
                                             n_checks=r.n_checks, seed=int(probs[b].seed),
                                             holdout_sum_abs=float(r.holdout_sum_abs),
                                             holdout_count=int(r.holdout_count))))
    return results, float(secs.value)


class CellList:
    """The non-NA cells of a matrix in the form `topolow_cv_fold` reads (include/topolow_relax.h)."""

    def __init__(self, n, rows, cols, values, codes, pos_of):
        self.n = int(n)
        self.rows, self.cols, self.values, self.codes = _i32(rows), _i32(cols), _f64(values), _i32(codes)
        self.pos_of = _i64(pos_of)
        self.by_row = _i64(np.lexsort((self.cols, self.rows)))
        counts = np.bincount(self.rows, minlength=self.n)
        self.row_ptr = _i64(np.concatenate([[0], np.cumsum(counts)]))
        c = self.c = TopolowCellList()
        c.n, c.n_cells = self.n, int(self.rows.shape[0])
        c.row, c.col, c.value, c.code = _ptr(self.rows), _ptr(self.cols), _ptr(self.values), _ptr(self.codes)
        c.pos_of, c.by_row, c.row_ptr = _ptr(self.pos_of), _ptr(self.by_row), _ptr(self.row_ptr)


def cv_fold(cells: CellList, picks, preserve_order: bool, named: bool):
    """One fold's problem from the cell list (host-side helper of the CV evaluator).  Returns
    (order or None, degrees, edge_i, edge_j, edge_dist, edge_thresh, hold_i, hold_j, hold_truth,
    numeric_max)."""
    lib = load()
    picks = _i64(picks)
    n, m = cells.n, int(cells.rows.shape[0])
    order, deg = np.empty(n, np.int32), np.empty(n, np.int32)
    ei, ej, ed, et = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64), np.empty(m, np.int32)
    hi, hj, ht = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    ne, nh, vmax = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
    rc = lib.topolow_cv_fold(C.byref(cells.c), _ptr(picks), int(picks.shape[0]), int(bool(preserve_order)),
                             int(bool(named)), _ptr(order), _ptr(deg), _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et), C.byref(ne),
                             _ptr(hi), _ptr(hj), _ptr(ht), C.byref(nh), C.byref(vmax))
    if rc != OK:
        raise NativeError(rc, "topolow_cv_fold failed")
    e, h = int(ne.value), int(nh.value)
    return (None if order[0] < 0 else order.astype(np.int64), deg, ei[:e].copy(), ej[:e].copy(), ed[:e].copy(),
            et[:e].copy(), hi[:h].copy(), hj[:h].copy(), ht[:h].copy(), float(vmax.value))


def _cv_sweep_call(symbol, cells: CellList, named, preserve_order, ndims, k0s, cooling_rates, c_repulsions, picks, unit_draws,
                   seeds, n_iter, relative_epsilon, convergence_window, convergence_check_freq, precision, device, *extra):
    """The marshalling of cv_sweep, cv_sweep_session and PreparedHandle.cv_sweep (cells None: the callable brings its
    handle): `symbol` is the bound library entry, `extra` what it takes between `device` and the outputs."""
    nf = len(picks)
    nd, k0, cr, cp = _i32(ndims), _f64(k0s), _f64(cooling_rates), _f64(c_repulsions)
    p_off = np.zeros(nf + 1, dtype=np.int64)
    d_off = np.zeros(nf + 1, dtype=np.int64)
    if nf:
        np.cumsum([len(p) for p in picks], out=p_off[1:])
        np.cumsum([u.size for u in unit_draws], out=d_off[1:])
    p_all = _i64(np.concatenate(picks) if nf else np.zeros(0))
    d_all = _f64(np.concatenate([np.ravel(u) for u in unit_draws]) if nf else np.zeros(0))
    sd = _u64(seeds)
    hsum, hcnt = np.zeros(nf, np.float64), np.zeros(nf, np.int64)
    its, conv, ec = np.zeros(nf, np.int32), np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    secs = C.c_double(0.0)
    _call(symbol, C.byref(cells.c) if cells is not None else None, int(bool(named)), int(bool(preserve_order)), nf,
          _ptr(nd), _ptr(k0), _ptr(cr), _ptr(cp), _ptr(p_all), _ptr(p_off), _ptr(d_all), _ptr(d_off), _ptr(sd), int(n_iter),
          float(relative_epsilon), int(convergence_window), int(convergence_check_freq), _PRECISIONS[precision],
          int(device), *extra, _ptr(hsum), _ptr(hcnt), _ptr(its), _ptr(conv), _ptr(ec), C.byref(secs))
    return hsum, hcnt, its, conv, ec, float(secs.value)


def cv_sweep(cells: CellList, named: bool, preserve_order: bool, ndims, k0s, cooling_rates, c_repulsions, picks, unit_draws,
             seeds, n_iter: int, relative_epsilon: float, convergence_window: int = 5, convergence_check_freq: int = 3,
             precision: str = "f64", device: int = -1):
    """All folds of a CV sweep in one library call (topolow_cv_sweep): fold f holds out the cells picks[f] and starts
    from the random walk built from unit_draws[f] ((ndim, n - 1) uniform(0, 1) numbers).  Returns
    (holdout_sum_abs, holdout_count, iterations, converged, error_code) arrays and the device seconds."""
    return _cv_sweep_call(load().topolow_cv_sweep, cells, named, preserve_order, ndims, k0s, cooling_rates, c_repulsions,
                          picks, unit_draws, seeds, n_iter, relative_epsilon, convergence_window, convergence_check_freq,
                          precision, device)


def cv_fold_pairs(cells: CellList, picks, preserve_order: bool, named: bool):
    """One fold as a resident session holds it out (topolow_cv_fold_pairs): everything in the caller's labels, no edge
    list.  Returns (order or None, degrees, numeric_max, n_edges, (pair_i, pair_j), (score_i, score_j, score_truth))."""
    return _fold_pairs_call(load().topolow_cv_fold_pairs, C.byref(cells.c), cells.n, picks, preserve_order, named)


def _fold_pairs_call(fn, source, n, picks, preserve_order, named, *tail, err=None):
    """The marshalling of cv_fold_pairs and PreparedHandle.fold: `source` is the cell list or the handle, `tail` what
    the entry takes between the shared outputs and the error buffer."""
    picks = _i64(picks)
    k = int(picks.shape[0])
    order, deg = np.empty(n, np.int32), np.empty(n, np.int32)
    pi, pj = np.empty(max(k, 1), np.int32), np.empty(max(k, 1), np.int32)
    si, sj, st = np.empty(max(2 * k, 1), np.int32), np.empty(max(2 * k, 1), np.int32), np.empty(max(2 * k, 1), np.float64)
    ne, npair, ns, vmax = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0.0)
    _call(fn, source, _ptr(picks), k, int(bool(preserve_order)), int(bool(named)), _ptr(order), _ptr(deg), C.byref(vmax),
          C.byref(ne), _ptr(pi), _ptr(pj), C.byref(npair), _ptr(si), _ptr(sj), _ptr(st), C.byref(ns), *tail, err=err)
    p, q = int(npair.value), int(ns.value)
    return (None if order[0] < 0 else order.astype(np.int64), deg, float(vmax.value), int(ne.value),
            (pi[:p].copy(), pj[:p].copy()), (si[:q].copy(), sj[:q].copy(), st[:q].copy()))


def batch_problem_fits(n: int, ndim: int, precision: str = "f64", n_edges: int = 0) -> bool:
    """Does a problem fit the one-workgroup kernel of optimize_layout_exact_batch / cv_sweep (its LDS)?  When not, those
    calls raise ERR_UNSUPPORTED and cv_sweep_session is the path."""
    return bool(load().topolow_batch_problem_fits(int(n), int(ndim), _PRECISIONS[precision], int(n_edges)))


def cv_sweep_session(cells: CellList, named: bool, preserve_order: bool, ndims, k0s, cooling_rates, c_repulsions, picks,
                     unit_draws, seeds, n_iter: int, relative_epsilon: float, convergence_window: int = 5,
                     convergence_check_freq: int = 3, precision: str = "auto", device: int = -1, schedule: str = "auto"):
    """`cv_sweep` on device-resident sessions (topolow_cv_sweep_session): one session per ndim holds the full matrix, a
    fold is held out of it, run, scored and put back.  schedule "auto" / "slab": the slab schedule, "gs": tile
    Gauss-Seidel; precision "auto": f32 for slab, f64 for gs.  Same returns as cv_sweep."""
    return _cv_sweep_call(load().topolow_cv_sweep_session, cells, named, preserve_order, ndims, k0s, cooling_rates,
                          c_repulsions, picks, unit_draws, seeds, n_iter, relative_epsilon, convergence_window,
                          convergence_check_freq, precision, device, _SCHEDULES[schedule])


def symm_stage_bounds(n: int, stages: int):
    """Slab boundaries (labels) of the symmetric form of an S-stage iteration, or None (topolow_symm_stage_bounds)."""
    out = np.zeros(stages + 1, dtype=np.int32)
    return out.tolist() if load().topolow_symm_stage_bounds(int(n), int(stages), _ptr(out)) else None


def symm_stage_order(seed: int, it: int, stages: int):
    """Order of the stages of iteration `it` (topolow_symm_stage_order)."""
    out = np.zeros(stages, dtype=np.int32)
    assert load().topolow_symm_stage_order(C.c_uint64(seed), int(it), int(stages), _ptr(out))
    return out.tolist()


def symm_stage_rows(n: int, stages: int, stage: int):
    """Per tile-row R the int32 row (j0, j1, rp0, rp1): the column blocks stage `stage` of a `stages`-stage iteration
    sweeps in R and the tile-rows whose column sums it adds to R's points; None where the problem is too small
    (topolow_symm_stage_rows; host only)."""
    lib = load()
    tr = lib.topolow_symm_stage_rows(int(n), int(stages), int(stage), None)
    if tr < 0:
        return None
    out = np.zeros((tr, 4), dtype=np.int32)
    assert lib.topolow_symm_stage_rows(int(n), int(stages), int(stage), _ptr(out)) == tr
    return out


def symm_plan(n: int, n_waves: int, stages: int = 0, stage: int = 0, segment: int = 0, n_segments: int = 1):
    """The symmetric sweep's plan for a grid of n_waves waves: (units[n_units, 4] = (tile_row, j0, j1, tile0),
    wave_first[n_waves + 1]) of the whole triangle, of one stage of a 2-, 4- or 8-stage iteration, or of one segment of
    the sharded sweep (topolow_symm_plan; host only)."""
    lib = load()
    args = (int(n), int(n_waves), int(stages), int(stage), int(segment), int(n_segments))
    n_units = lib.topolow_symm_plan(*args, None, 0, None)
    if n_units < 0:
        raise ValueError("symm_plan: no such plan for %r" % (args,))
    units = np.zeros((n_units, 4), dtype=np.int32)
    wave_first = np.zeros(int(n_waves) + 1, dtype=np.int32)
    assert lib.topolow_symm_plan(*args, _ptr(units), n_units, _ptr(wave_first)) == n_units
    return units, wave_first


def symm_segment_rows(n: int, segment: int, n_segments: int):
    """Rows (first, end) of the matrix that hold segment `segment` of `n_segments` of the symmetric sweep's tile list;
    None when a problem of n points has too few tiles to cut (topolow_symm_segment_rows; host only)."""
    lib = load()
    a, b = C.c_int32(0), C.c_int32(0)
    if not lib.topolow_symm_segment_rows(int(n), int(segment), int(n_segments), C.byref(a), C.byref(b)):
        return None
    return int(a.value), int(b.value)


def shard_rows(n: int, blocks: int):
    """Row blocks of the row-sharded path: list of (row_begin, row_end), empty trailing blocks dropped."""
    lib = load()
    used = lib.topolow_shard_rows(int(n), int(blocks), -1, None, None)
    out = []
    for b in range(used):
        rb, re_ = C.c_int32(0), C.c_int32(0)
        lib.topolow_shard_rows(int(n), int(blocks), b, C.byref(rb), C.byref(re_))
        out.append((int(rb.value), int(re_.value)))
    return out


def optimize_layout_exact_sharded(initial_positions, degrees, edge_i, edge_j, edge_dist, edge_thresh, n_iter, k0,
                                  cooling_rate, c_repulsion, relative_epsilon=1e-4, convergence_window=5,
                                  convergence_check_freq=3, verbose=False, dissimilarity_matrix=None,
                                  threshold_matrix=None, devices=(0,), **opt_kw) -> NativeResult:
    """The `.Call` payload as ONE embedding row-sharded over `devices` (topolow_optimize_layout_exact_sharded).
    Without the dense matrices the edge list IS the matrix (large problems)."""
    lib = load()
    pos0 = _f64F(initial_positions)
    n, dim = pos0.shape
    D = _f64F(dissimilarity_matrix) if dissimilarity_matrix is not None else None
    T = _i32F(threshold_matrix) if threshold_matrix is not None else None
    deg, ei, ej, ed, et = _i32(degrees), _i32(edge_i), _i32(edge_j), _f64(edge_dist), _i32(edge_thresh)
    out, stats = _RunOut(n, dim), TopolowShardStats()
    opt = make_options(devices=list(devices), **opt_kw)
    _call(lib.topolow_optimize_layout_exact_sharded,
          _ptr(pos0), n, dim, _ptr(D), _ptr(T), _ptr(deg), _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et), int(ei.shape[0]),
          int(n_iter), float(k0), float(cooling_rate), float(c_repulsion), float(relative_epsilon),
          int(convergence_window), int(convergence_check_freq), int(bool(verbose)), C.byref(opt), *out.args,
          C.byref(stats))
    return out.result(dict(
        schedule="slab", blocks=stats.blocks, groups=stats.groups, iterations_run=stats.iterations_run,
        n_checks=stats.n_checks, loop_seconds=stats.loop_seconds, total_seconds=stats.total_seconds,
        stage_kernel_seconds=stats.stage_kernel_seconds, check_kernel_seconds=stats.check_kernel_seconds,
        stage_launches=stats.stage_launches, exchanges=stats.exchanges, seed=int(opt.seed)))


def run_sharded(sessions, initial_positions, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon=1e-4,
                convergence_window=5, convergence_check_freq=3, seed=0, slab_stages=0, interrupt=None,
                profile=False, warmup_iterations=0) -> NativeResult:
    """ONE embedding over the given row-block sessions (topolow_sessions_run_sharded): one process, one
    host thread per block, peer-stored position slices, replicated controller."""
    lib = load()
    pos0 = _f64F(initial_positions)
    n, dim = pos0.shape
    hs = (C.c_void_p * len(sessions))(*[s._h for s in sessions])
    out, stats = _RunOut(n, dim), TopolowShardStats()
    stats.warmup_iterations = int(warmup_iterations)   # measurement aid: timed_seconds starts after these
    cb = INTERRUPT_CB(lambda _u: 1 if interrupt() else 0) if interrupt is not None else INTERRUPT_CB()
    _call(lib.topolow_sessions_run_sharded, hs, len(sessions), _ptr(pos0), int(n_iter), float(k0), float(cooling_rate),
          float(c_repulsion), float(relative_epsilon), int(convergence_window), int(convergence_check_freq),
          int(seed) & 0xFFFFFFFFFFFFFFFF, int(slab_stages), cb, None, int(bool(profile)), *out.args, C.byref(stats))
    return out.result(dict(
        schedule="slab", blocks=stats.blocks, groups=stats.groups, iterations_run=stats.iterations_run,
        n_checks=stats.n_checks, loop_seconds=stats.loop_seconds, stage_kernel_seconds=stats.stage_kernel_seconds,
        check_kernel_seconds=stats.check_kernel_seconds, stage_launches=stats.stage_launches,
        exchanges=stats.exchanges, timed_seconds=stats.timed_seconds, symmetric_segments=stats.symmetric_segments))


def est_distances(positions) -> np.ndarray:
    """as.matrix(dist(positions)) (reference R/core.R:474) on the GPU."""
    lib = load()
    pos = _f64F(positions)
    n, dim = pos.shape
    out = np.empty((n, n), dtype=np.float64)
    _call(lib.topolow_est_distances, _ptr(pos), n, dim, _ptr(out), int(options.get("device", -1)))
    return out


def est_distances_rows(positions, row_begin: int, row_end: int) -> np.ndarray:
    """Rows [row_begin, row_end) of as.matrix(dist(positions)): shape (row_end - row_begin, n)."""
    lib = load()
    pos = _f64F(positions)
    n, dim = pos.shape
    out = np.empty((int(row_end) - int(row_begin), n), dtype=np.float64)
    _call(lib.topolow_est_distances_rows, _ptr(pos), n, dim, int(row_begin), int(row_end), _ptr(out),
          int(options.get("device", -1)))
    return out


POST_STAGINGS = {"default": 0, "pinned": 1, "register": 2, "pageable": 3}


def mae_of(sum_abs: float, count: int) -> float:
    """mae = sum_abs / count; no counting cell is R's mean of nothing, NaN (no warning)."""
    return float(sum_abs) / int(count) if int(count) > 0 else float("nan")


def post_metrics(positions, values, codes=None, want_est: bool = True, staging: str = "default",
                 phases: Optional[list] = None):
    """The reference's post-processing (R/core.R:474-481) in one pass on the GPU: returns
    (est_distances or None, sum_abs, count) with sum_abs = sum |values - est| over the cells whose value is
    finite and whose code (if codes are given) is 0, the diagonal included; mae = mae_of(sum_abs, count).
    est_distances is bit-identical to est_distances(positions).

    `values` (and `codes`) are used where they lie when they are contiguous.  The library reads column-major
    matrices, so a C-contiguous pair is read as its transpose: est_distances is symmetric bit for bit, so the
    count and the set of summed terms are the same and only the order of the additions (the last bits of
    sum_abs) follows the transposed matrix; an n x n transposing copy is spared.  `staging` and `phases`
    (a list that receives the seconds of the upload, kernel and download phases) are for
    tests/study/post_metrics_timing.py."""
    lib = load()
    pos = _f64F(positions)
    n, dim = pos.shape
    vals = np.asarray(values, dtype=np.float64)
    if vals.shape != (n, n):
        raise ValueError("values must be an n x n matrix with one row per position")
    c_order = vals.flags.c_contiguous and not vals.flags.f_contiguous
    need = ["C", "A"] if c_order else ["F", "A"]
    vals = np.require(vals, requirements=need)
    cds = None
    if codes is not None:
        cds = np.require(np.asarray(codes, dtype=np.int32), requirements=need)
        if cds.shape != (n, n):
            raise ValueError("codes must have the shape of values")
    est = np.empty((n, n), dtype=np.float64) if want_est else None
    sc = _SumCount()
    ph = (C.c_double * 3)()
    _call(lib.topolow_post_metrics_ex, _ptr(pos), n, dim, _ptr(vals), _ptr(cds), _ptr(est), *sc.refs,
          int(options.get("device", -1)), POST_STAGINGS[staging], ph if phases is not None else None)
    if phases is not None:
        phases[:] = [ph[0], ph[1], ph[2]]
    return (est, *sc.values())


def kernel_velocity(positions, times, sigma_t: float, sigma_x: float, excluded_bits=None, device: Optional[int] = None,
                    chunk_cols: Optional[int] = None, timing: Optional[list] = None):
    """The reference's compute_kernel_velocity (R/visualization.R:802-843) on the GPU: returns (velocity n x ndim,
    weight_sum n), rows without an eligible past point (or whose weights are all 0) NaN in velocity.
    excluded_bits: None, or an n x ceil(n / 64) uint64 array in the caller's order -- bit (j % 64) of word
    (j // 64) of row i set = point j does not contribute to row i (topolow_amd.velocity.pack_exclusion_bits).
    `chunk_cols` (a multiple of 64; None = the library's width, a function of n) and `timing` (a list that
    receives the seconds of the kernels) reach the _ex entry: for tests and tests/study/velocity_timing.py."""
    lib = load()
    pos = _f64F(positions)
    if pos.ndim != 2:
        raise ValueError("positions must be an n x ndim matrix")
    n, dim = pos.shape
    t = _f64(times)
    if t.shape != (n,):
        raise ValueError("times must hold one value per position")
    bits = None
    if excluded_bits is not None:
        bits = _u64(excluded_bits)
        if bits.shape != (n, (n + 63) // 64):
            raise ValueError("excluded_bits must be an n x ceil(n / 64) array of 64-bit words")
    vel = np.empty((n, dim), dtype=np.float64, order="F")
    w = np.empty(n, dtype=np.float64)
    secs = C.c_double(0.0)
    dev = int(options.get("device", -1)) if device is None else int(device)
    shared = (_ptr(pos), _ptr(t), n, dim, float(sigma_t), float(sigma_x), _ptr(bits), _ptr(vel), _ptr(w), dev)
    if chunk_cols is None and timing is None:
        _call(lib.topolow_kernel_velocity, *shared)
    else:
        _call(lib.topolow_kernel_velocity_ex, *shared, int(chunk_cols or 0), C.byref(secs) if timing is not None else None)
    if timing is not None:
        timing[:] = [secs.value]
    return vel, w


def _map_and_reduced(positions, reduced):
    pos, red = _f64F(positions), _f64F(reduced)
    if pos.ndim != 2 or red.ndim != 2:
        raise ValueError("positions and reduced must be matrices, n x ndim and n x k")
    if red.shape[0] != pos.shape[0]:
        raise ValueError("reduced must hold one row per position")
    return pos, red


def scale_objective(positions, reduced, scales, device: Optional[int] = None, chunk_cols: Optional[int] = None,
                    timing: Optional[list] = None):
    """The objective of the reference's scale_to_original_distances (R/visualization.R:629-632) on the GPU, with no
    n x n matrix: returns (F, G, H) with F[q] = sum_{i != j} |d_ij - scales[q] r_ij| (up to 8 scales in one pass),
    G = sum d_ij and H = sum r_ij, d and r the pairwise distances of positions (n x ndim) and reduced (n x k).
    `chunk_cols` (64, 128, 256 or 512; None = the library's width, a function of n) and `timing` (a list that
    receives the seconds of the kernels) reach the _ex entry: for tests and tests/study/reduce_timing.py."""
    lib = load()
    pos, red = _map_and_reduced(positions, reduced)
    s = _f64(np.atleast_1d(scales))
    if s.ndim != 1:
        raise ValueError("scales must be a vector")
    F = np.empty(s.size, dtype=np.float64)
    G, H, secs = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    dev = int(options.get("device", -1)) if device is None else int(device)
    shared = (_ptr(pos), _ptr(red), pos.shape[0], pos.shape[1], red.shape[1], _ptr(s), s.size, _ptr(F), C.byref(G),
              C.byref(H), dev)
    if chunk_cols is None and timing is None:
        _call(lib.topolow_scale_objective, *shared)
    else:
        _call(lib.topolow_scale_objective_ex, *shared, int(chunk_cols or 0), C.byref(secs) if timing is not None else None)
    if timing is not None:
        timing[:] = [secs.value]
    return F, G.value, H.value


def scale_to_original_distances(positions, reduced, lower: float = 0.01, upper: float = 40.0,
                                tol: float = float(np.finfo(np.float64).eps) ** 0.25, device: Optional[int] = None,
                                trace_len: int = 0):
    """The scale in [lower, upper] that minimises scale_objective, by Brent's fmin inside the library (the reference's
    optimize call, R/visualization.R:635-636): returns (scale, objective, evaluations, trace) with trace the first
    trace_len evaluated (s, F) pairs as a k x 2 array."""
    lib = load()
    pos, red = _map_and_reduced(positions, reduced)
    scale, objective, evals = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    trace_len = int(trace_len)
    ts = np.full(max(trace_len, 0), np.nan)
    tf = np.full(max(trace_len, 0), np.nan)
    dev = int(options.get("device", -1)) if device is None else int(device)
    _call(lib.topolow_scale_to_original_distances, _ptr(pos), _ptr(red), pos.shape[0], pos.shape[1], red.shape[1],
          float(lower), float(upper), float(tol), C.byref(scale), C.byref(objective), C.byref(evals),
          _ptr(ts) if trace_len > 0 else None, _ptr(tf) if trace_len > 0 else None, trace_len, dev)
    kept = min(trace_len, evals.value)
    return scale.value, objective.value, evals.value, np.column_stack([ts[:kept], tf[:kept]])


ORDER_PRESERVED, ORDER_DEVICE_EXACT, ORDER_DEVICE_GAP, ORDER_DECLINED = 0, 1, 2, 3


@dataclass
class PreparedLayout:
    """What topolow_layout_prep_create / _fetch computed.  `info` holds the fields of topolow_layout_prep_info as a
    dict; order is None where the input order is kept.  On info["order_route"] == ORDER_DECLINED without an `order`
    given, nothing but `info` is filled: the caller orders and calls again."""
    info: Dict[str, Any]
    order: Optional[np.ndarray] = None
    degrees: Optional[np.ndarray] = None
    edge_i: Optional[np.ndarray] = None
    edge_j: Optional[np.ndarray] = None
    edge_dist: Optional[np.ndarray] = None
    edge_thresh: Optional[np.ndarray] = None
    dense: Optional[np.ndarray] = None
    tdense: Optional[np.ndarray] = None
    values_reordered: Optional[np.ndarray] = None
    codes_reordered: Optional[np.ndarray] = None
    phase_seconds: Optional[list] = None


def order_from_sums(row_sum, row_cnt, col_sum, col_cnt, exact_sums: int):
    """topolow_layout_order_from_sums: (route, order or None).  Host only."""
    lib = load()
    rs, cs, rc_, cc = _f64(row_sum), _f64(col_sum), _i64(row_cnt), _i64(col_cnt)
    n = rs.shape[0]
    order = np.empty(max(n, 1), dtype=np.int32)
    route = lib.topolow_layout_order_from_sums(n, _ptr(rs), _ptr(rc_), _ptr(cs), _ptr(cc), int(exact_sums), _ptr(order))
    return int(route), (None if order[0] == -1 else order[:n])


class PreparedHandle:
    """A prepared layout that stays on the device (topolow_layout_prep_*): a context manager around create / destroy.
    `values` (f64, NaN = NA) and `codes` (int8 or None) are used where they lie: a C-contiguous matrix goes with
    transposed=1, a Fortran-contiguous one with transposed=0 (`layout` = "C" / "F" forces the reading of a matrix that
    is both).  `order`: the caller's order (an int array, or [-1] for "keep"), for data on which the device declines
    to order.  `.info` holds the fields of topolow_layout_prep_info; on info["order_route"] == ORDER_DECLINED without an
    `order` given the handle holds nothing else (`.declined`): the caller orders and creates again.

        with PreparedHandle(values, codes) as h:
            res = h.optimize(initial_positions, ndim, n_iter, k0, cooling_rate, c_repulsion)
            est, sum_abs, count = h.post_metrics(res.positions)

    The matrix goes up once; .optimize and .post_metrics read what the handle keeps on the device and return the bits
    of optimize_layout_exact_arrays / post_metrics on the arrays .fetch() returns."""

    def __init__(self, values, codes=None, preserve_order: bool = False, order=None, layout: Optional[str] = None,
                 device: Optional[int] = None):
        self._blank()
        vals = np.asarray(values)
        if vals.ndim != 2 or vals.shape[0] != vals.shape[1]:
            raise ValueError("values must be an n x n matrix")
        n = vals.shape[0]
        if layout is None:
            layout = "F" if (vals.flags.f_contiguous and not vals.flags.c_contiguous) else "C"
        need = [layout, "A"]
        vals = np.require(vals, dtype=np.float64, requirements=need)
        cds = None
        if codes is not None:
            cds = np.require(np.asarray(codes), dtype=np.int8, requirements=need)
            if cds.shape != (n, n):
                raise ValueError("codes must have the shape of values")
        oin = None
        if order is not None:
            oin = _i32(order).reshape(-1)
            if oin.shape[0] != n and not (oin.shape[0] >= 1 and oin[0] == -1):
                raise ValueError("order must have n entries")
        self.n, self.layout, self.has_codes = int(n), layout, cds is not None
        info = TopolowLayoutPrepInfo()
        _call(self.lib.topolow_layout_prep_create, C.byref(self._h), _ptr(vals), _ptr(cds), n, 1 if layout == "C" else 0,
              1 if preserve_order else 0, _ptr(oin), int(options.get("device", -1)) if device is None else int(device),
              C.byref(info), err=self._err)
        self.info = _fields(info)

    def _blank(self):
        """A handle before the library has filled it: the constructor and .subsample start from it."""
        self.lib, self._h, self._err, self._order = load(), C.c_void_p(None), C.create_string_buffer(512), None

    @property
    def declined(self) -> bool:
        return int(self.info["n_edges"]) < 0

    @property
    def order(self) -> Optional[np.ndarray]:
        """The order applied (int32, 0-based), or None where the input order is kept.  n values from the handle's host
        side: nothing of size n x n moves."""
        if self.declined or not self.info["reordered"]:
            return None
        if self._order is None:
            o = np.empty(self.n, dtype=np.int32)
            if self.lib.topolow_layout_prep_order(self._h, _ptr(o), None) != OK:
                raise NativeError(ERR_BAD_ARGUMENT, "topolow_layout_prep_order refused the handle")
            self._order = o
        return self._order

    def fetch(self, want_dense: bool = True, want_reordered: bool = True) -> PreparedLayout:
        """topolow_layout_prep_fetch: the arrays of the 16-argument call as a PreparedLayout (see prepare_layout)."""
        out = PreparedLayout(info=dict(self.info))
        if self.declined:
            return out
        n, layout = self.n, self.layout
        E = int(self.info["n_edges"])
        o = np.empty(n, dtype=np.int32)
        out.degrees = np.empty(n, dtype=np.int32)
        out.edge_i, out.edge_j = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
        out.edge_dist, out.edge_thresh = np.empty(E, dtype=np.float64), np.empty(E, dtype=np.int32)
        if want_dense:
            out.dense = np.empty((n, n), dtype=np.float64, order=layout)
            out.tdense = np.empty((n, n), dtype=np.int32, order=layout)
        want_reordered = bool(want_reordered) and bool(self.info["reordered"])
        if want_reordered:
            out.values_reordered = np.empty((n, n), dtype=np.float64, order=layout)
            out.codes_reordered = np.empty((n, n), dtype=np.int8, order=layout)
        _call(self.lib.topolow_layout_prep_fetch, self._h, _ptr(o), _ptr(out.degrees), _ptr(out.edge_i), _ptr(out.edge_j),
              _ptr(out.edge_dist), _ptr(out.edge_thresh), _ptr(out.dense), _ptr(out.tdense), _ptr(out.values_reordered),
              _ptr(out.codes_reordered), err=self._err)
        out.order = None if o[0] == -1 else o
        out.phase_seconds = self.phase_seconds()
        return out

    def optimize(self, initial_positions, ndim: Optional[int] = None, n_iter: int = 1000, k0: float = 1.0,
                 cooling_rate: float = 0.01, c_repulsion: float = 0.01, relative_epsilon: float = 1e-4,
                 convergence_window: int = 5, convergence_check_freq: int = 3, verbose: bool = False,
                 **opt_kw) -> NativeResult:
        """topolow_layout_prep_optimize: optimize_layout_exact_arrays with the matrix, degrees and edges taken from the
        handle.  initial_positions: n x ndim, row q for the q-th point of the ordered matrix."""
        pos0 = _f64F(initial_positions)
        n, dim = pos0.shape
        if n != self.n or (ndim is not None and int(ndim) != dim):
            raise ValueError("initial_positions must be n x ndim")
        out, stats = _RunOut(n, dim), TopolowRunStats()
        opt = make_options(**opt_kw)
        _call(self.lib.topolow_layout_prep_optimize, self._h, _ptr(pos0), dim, int(n_iter), float(k0), float(cooling_rate),
              float(c_repulsion), float(relative_epsilon), int(convergence_window), int(convergence_check_freq),
              int(bool(verbose)), C.byref(opt), *out.args, C.byref(stats), err=self._err)
        return out.result(_run_info(stats, opt))

    def post_metrics(self, positions, want_est: bool = True):
        """topolow_layout_prep_post_metrics: (est_distances or None, sum_abs, count) of the handle's resident matrix,
        as post_metrics() gives them for the reordered matrix in the handle's layout."""
        pos = _f64F(positions)
        n, dim = pos.shape
        if n != self.n:
            raise ValueError("positions must have one row per point")
        est = np.empty((n, n), dtype=np.float64) if want_est else None
        sc = _SumCount()
        _call(self.lib.topolow_layout_prep_post_metrics, self._h, _ptr(pos), dim, _ptr(est), *sc.refs, err=self._err)
        return (est, *sc.values())

    def fold(self, picks, preserve_order: bool, named: bool):
        """One cross-validation fold prepared on the device (topolow_layout_prep_fold): what cv_fold_pairs computes from
        the cell list, from the resident matrix.  Returns (order or None, degrees, numeric_max, n_edges, (pair_i, pair_j),
        (score_i, score_j, score_truth), order_route); the pairs are cv_fold_pairs' as a set (sorted by (j, i)), everything
        else is equal to it.  order_route == ORDER_DECLINED: the order is the caller's to compute (None is returned)."""
        route = C.c_int32(0)
        out = _fold_pairs_call(self.lib.topolow_layout_prep_fold, self._h, self.n, picks, preserve_order, named,
                               C.byref(route), err=self._err)
        return out + (int(route.value),)

    def cv_sweep(self, named: bool, preserve_order: bool, ndims, k0s, cooling_rates, c_repulsions, picks, unit_draws, seeds,
                 n_iter: int, relative_epsilon: float, convergence_window: int = 5, convergence_check_freq: int = 3,
                 precision: str = "auto", schedule: str = "auto"):
        """`cv_sweep_session` with this handle in place of the cell list (topolow_layout_prep_cv_sweep): the folds are
        prepared on the device from the resident matrix.  Returns cv_sweep_session's (holdout_sum_abs, holdout_count,
        iterations, converged, error_code, device seconds) -- the same bits for every fold that ran -- and, as a seventh
        element, order_route per fold.  A fold with order_route == ORDER_DECLINED did not run (error_code
        ERR_UNSUPPORTED): it is the caller's to rerun through cv_sweep_session."""
        nf = len(picks)
        route = np.zeros(nf, np.int32)

        def symbol(cells, named_, preserve_, nf_, nd, k0, cr, cp, p_all, p_off, d_all, d_off, sd, n_iter_, eps, window, freq,
                   prec, device, sched, *outs):
            return self.lib.topolow_layout_prep_cv_sweep(self._h, named_, preserve_, nf_, nd, k0, cr, cp, p_all, p_off, d_all,
                                                         d_off, sd, n_iter_, eps, window, freq, prec, sched, *outs[:5],
                                                         _ptr(route), *outs[5:])
        out = _cv_sweep_call(symbol, None, named, preserve_order, ndims, k0s, cooling_rates, c_repulsions, picks, unit_draws,
                             seeds, n_iter, relative_epsilon, convergence_window, convergence_check_freq, precision, -1,
                             _SCHEDULES[schedule])
        return out + (route,)

    def _subset(self, indices):
        """`indices` as the C entries take a subset: (int32 array or None, m).  None: all n points."""
        if indices is None:
            return None, self.n
        sub = _i32(indices).reshape(-1)
        return sub, int(sub.shape[0])

    def connectivity(self, subset=None):
        """topolow_layout_prep_connectivity: the components of the measurement graph of the resident matrix, or of the
        points `subset` of it (distinct 0-based indices into the matrix as it was given, any order), on the device.
        Returns (n_components, n_cells, labels): n_cells the non-NaN off-diagonal cells of the induced submatrix over
        both triangles, labels[q] the smallest position in `subset` whose point lies in the component of subset[q]."""
        sub, m = self._subset(subset)
        labels = np.empty(m, dtype=np.int32)
        nc, cells = C.c_int32(0), C.c_int64(0)
        _call(self.lib.topolow_layout_prep_connectivity, self._h, _ptr(sub), m, C.byref(nc), C.byref(cells), _ptr(labels),
              err=self._err)
        return int(nc.value), int(cells.value), labels

    def subsample(self, indices, preserve_order: bool = False, order_in=None) -> "PreparedHandle":
        """topolow_layout_prep_subsample: a PreparedHandle for values[indices][:, indices] (and the codes), gathered
        device to device and prepared as a fresh handle is -- everything it reports equals, bit for bit, what
        PreparedHandle(values[np.ix_(indices, indices)], ...) reports.  `preserve_order` and `order_in` (the `order` of
        the constructor) are relative to the child's own points.  The child outlives this handle; close it as any."""
        sub, m = self._subset(indices)
        oin = None
        if order_in is not None:
            oin = _i32(order_in).reshape(-1)
            if oin.shape[0] != m and not (oin.shape[0] >= 1 and oin[0] == -1):
                raise ValueError("order must have one entry per selected point")
        child = PreparedHandle.__new__(PreparedHandle)
        child._blank()
        child.n, child.layout, child.has_codes = m, self.layout, self.has_codes
        info = TopolowLayoutPrepInfo()
        _call(self.lib.topolow_layout_prep_subsample, self._h, _ptr(sub), m, 1 if preserve_order else 0, _ptr(oin),
              C.byref(child._h), C.byref(info), err=child._err)
        child.info = _fields(info)
        return child

    def degrees(self, subset=None):
        """topolow_layout_prep_degrees: (degrees, n_cells) of the resident matrix or of the points `subset` of it (as
        .connectivity takes them): degrees[q] the measured cells (subset[q], subset[c]), c != q, along the matrix ROW
        (int32), n_cells their sum."""
        sub, m = self._subset(subset)
        deg = np.empty(m, dtype=np.int32)
        cells = C.c_int64(0)
        _call(self.lib.topolow_layout_prep_degrees, self._h, _ptr(sub), m, _ptr(deg), C.byref(cells), err=self._err)
        return deg, int(cells.value)

    def prune(self, min_connections=4, target_completeness=None, max_iterations=100, min_points=10):
        """topolow_layout_prep_prune: the rounds of prune.prune_sparse_matrix on the resident matrix, the whole
        `target_completeness` search included.  Returns (kept, info): kept a bool array over the n points, info the
        fields of topolow_prune_info as a dict (the per-attempt arrays as lists of `attempts` entries, `seconds`: bit
        pass, rounds, the rest).  Non-integer thresholds are rounded up, which decides every `count <` test alike."""
        def as_i32(x):
            return int(min(max(math.ceil(x), -(2 ** 31 - 1)), 2 ** 31 - 1))

        kept = np.zeros(self.n, dtype=np.uint8)
        info = TopolowPruneInfo()
        _call(self.lib.topolow_layout_prep_prune, self._h, as_i32(min_connections),
              float("nan") if target_completeness is None else float(target_completeness), as_i32(max_iterations),
              as_i32(min_points), _ptr(kept), C.byref(info), err=self._err)
        out = {}
        for k, _ in TopolowPruneInfo._fields_:
            v = getattr(info, k)
            if k == "reserved":
                continue
            out[k] = list(v)[:info.attempts] if k.startswith("attempt_") else (list(v) if k == "seconds" else v)
        return kept.astype(bool), out

    def spectrum(self, want_eigenvalues: bool = True, want_centered: bool = False):
        """topolow_layout_prep_spectrum: the data assessment of the reference's Euclidify() (R/core.R:983-1007) of the
        resident matrix in its input order.  Returns (info, eigenvalues or None, centered or None): info the fields of
        topolow_spectrum_info as a dict (`seconds`: median, centring, tridiagonalisation, bisection), the eigenvalues
        descending, centered the matrix B = -0.5 J D^2 J in the handle's layout.  Serves a handle that declined its
        ordering; the handle is not altered.  No numeric cell, or an infinite one: NativeError(ERR_BAD_ARGUMENT)."""
        n = self.n
        eig = np.empty(n, dtype=np.float64) if want_eigenvalues else None
        cen = np.empty((n, n), dtype=np.float64, order=self.layout) if want_centered else None
        info = TopolowSpectrumInfo()
        _call(self.lib.topolow_layout_prep_spectrum, self._h, _ptr(eig), _ptr(cen), C.byref(info), err=self._err)
        out = _fields(info)
        out["seconds"] = list(info.seconds)
        return out, eig, cen

    def _fit_inputs(self, positions, picks):
        pos = _f64F(positions)
        if pos.ndim != 2 or pos.shape[0] != self.n:
            raise ValueError("positions must have one row per point")
        pk = _i64(picks if picks is not None else []).reshape(-1)
        return pos, pk, (_ptr(pk) if pk.size else None)

    def fit_report(self, positions, picks=None):
        """topolow_layout_prep_fit_report: the moments of the signed errors value - distance of the handle's resident
        matrix against `positions` (n x ndim, row q for the q-th point of the ordered matrix, as post_metrics), per
        series "in" / "out" / "all".  `picks`: the held-out cells as linear column-major indices r + c * n in the
        caller's numbering (their mirrors are held out too), or None.  +-Inf cells are in no series (a deviation from
        the reference, as post_metrics).  Returns {"in": {...}, "out": {...}, "all": {...}, "seconds": [pass 1, pass 2,
        total]}, each series with the fields of topolow_fit_series."""
        pos, pk, pkp = self._fit_inputs(positions, picks)
        rep = TopolowFitReport()
        _call(self.lib.topolow_layout_prep_fit_report, self._h, _ptr(pos), pos.shape[1], pkp, int(pk.size), C.byref(rep),
              err=self._err)
        out = {name: _fields(rep.series[s]) for name, s in (("in", FIT_IN), ("out", FIT_OUT), ("all", FIT_ALL))}
        out["seconds"] = list(rep.seconds)
        return out

    def fit_order_stats(self, positions, series, ranks, picks=None):
        """topolow_layout_prep_fit_order_stats: (values, m) -- values[k] has the bits of the ranks[k]-th smallest signed
        error of `series` ("in", "out", "all" or FIT_*), m is the series' count; 1 .. FIT_MAX_RANKS ranks, eight passes
        over the resident matrix whatever their number.  An empty series gives NaN values and m = 0; a rank >= m raises
        NativeError(ERR_BAD_ARGUMENT).  Negative ranks: see include/topolow_relax.h."""
        if series not in _FIT_SERIES:
            raise ValueError('series must be "in", "out" or "all"')
        pos, pk, pkp = self._fit_inputs(positions, picks)
        rk = _i64(ranks).reshape(-1)
        vals = np.full(max(int(rk.size), 1), np.nan)
        m = C.c_int64(0)
        _call(self.lib.topolow_layout_prep_fit_order_stats, self._h, _ptr(pos), pos.shape[1], pkp, int(pk.size),
              _FIT_SERIES[series], _ptr(rk), int(rk.size), _ptr(vals), C.byref(m), err=self._err)
        return vals[:rk.size].copy(), int(m.value)

    def _fit_series_axes(self, series, *axes):
        if series not in _FIT_SERIES:
            raise ValueError('series must be "in", "out" or "all"')
        for axis in axes:
            if axis not in _FIT_AXIS:
                raise ValueError('an axis must be "true", "predicted", "error" or "residual"')
        return (_FIT_SERIES[series],) + tuple(_FIT_AXIS[axis] for axis in axes)

    def fit_extent(self, positions, series, picks=None):
        """topolow_layout_prep_fit_extent: ({"true": (min, max), "predicted": ..., "error": ..., "residual": ...}, m) of
        `series` -- the bits of the extremes of v, r, v - r and r - v; NaN when the series is empty (m = 0).  positions,
        picks and the series as fit_report; the diagonal counts."""
        (s,) = self._fit_series_axes(series)
        pos, pk, pkp = self._fit_inputs(positions, picks)
        out, m = np.full(8, np.nan), C.c_int64(0)
        _call(self.lib.topolow_layout_prep_fit_extent, self._h, _ptr(pos), pos.shape[1], pkp, int(pk.size), s, _ptr(out),
              C.byref(m), err=self._err)
        return {name: (float(out[2 * k]), float(out[2 * k + 1])) for k, name in enumerate(FIT_AXES)}, int(m.value)

    def fit_hist2d(self, positions, series, x_axis, x_edges, y_axis, y_edges, picks=None):
        """topolow_layout_prep_fit_hist2d: (counts, outside, m) -- counts[kx, ky] (int64, len(x_edges) - 1 by
        len(y_edges) - 1) the cells of `series` with x_edges[kx] <= x < x_edges[kx + 1] and the same for y, the last
        bin of either axis closed above: np.histogram2d's rule with explicit edges, and its counts.  outside: the cells
        of the series outside either axis; counts.sum() + outside == m.  Axes: "true", "predicted", "error" (v - r),
        "residual" (r - v).  At most FIT_MAX_BINS bins; the edges finite and strictly increasing."""
        s, ax, ay = self._fit_series_axes(series, x_axis, y_axis)
        pos, pk, pkp = self._fit_inputs(positions, picks)
        xe, ye = _f64(x_edges).reshape(-1), _f64(y_edges).reshape(-1)
        nx, ny = int(xe.size) - 1, int(ye.size) - 1
        fits = nx >= 1 and ny >= 1 and nx * ny <= FIT_MAX_BINS      # (otherwise the library refuses, and says why)
        counts = np.zeros((nx, ny) if fits else (1, 1), dtype=np.int64)
        outside, m = C.c_int64(0), C.c_int64(0)
        _call(self.lib.topolow_layout_prep_fit_hist2d, self._h, _ptr(pos), pos.shape[1], pkp, int(pk.size), s, ax, _ptr(xe),
              nx, ay, _ptr(ye), ny, _ptr(counts), C.byref(outside), C.byref(m), err=self._err)
        return counts, int(outside.value), int(m.value)

    def fit_linear_bins(self, positions, series, axis, lo, up, m=512, picks=None):
        """topolow_layout_prep_fit_linear_bins: (count, frac, outside, total) -- density()'s linear binning of `axis`
        over `series` on the m-point grid over [lo, up], in integers: count[ix] the cells with floor((x - lo) / delta)
        = ix, frac[ix] (uint64) the sum of their (uint64)(fx * 2^32); ix in 0 .. m - 2, every other cell in `outside`.
        error_metrics.linear_bin_masses forms the masses."""
        s, ax = self._fit_series_axes(series, axis)
        pos, pk, pkp = self._fit_inputs(positions, picks)
        m = int(m)
        size = min(max(m, 1), FIT_MAX_GRID)
        count, frac = np.zeros(size, dtype=np.int64), np.zeros(size, dtype=np.uint64)
        outside, total = C.c_int64(0), C.c_int64(0)
        _call(self.lib.topolow_layout_prep_fit_linear_bins, self._h, _ptr(pos), pos.shape[1], pkp, int(pk.size), s, ax,
              float(lo), float(up), m, _ptr(count), _ptr(frac), C.byref(outside), C.byref(total), err=self._err)
        return count, frac, int(outside.value), int(total.value)

    def graph_stats(self):
        """(rounds, [seconds of the bit pass, seconds of the rounds]) of the last .connectivity on this handle."""
        rounds, ph = C.c_int32(0), (C.c_double * 2)()
        self.lib.topolow_layout_prep_graph_stats(self._h, C.byref(rounds), ph)
        return int(rounds.value), list(ph)

    def fold_seconds(self) -> list:
        """Seconds of the last .cv_sweep on this handle, summed over its folds: preparation, hold-out, score, restore."""
        return self._seconds(self.lib.topolow_layout_prep_fold_seconds, 4)

    def phase_seconds(self) -> list:
        return self._seconds(self.lib.topolow_layout_prep_phase_seconds, 5)

    def resident_seconds(self) -> list:
        """Seconds of the last Session.load_prepared, .optimize and .post_metrics on this handle."""
        return self._seconds(self.lib.topolow_layout_prep_resident_seconds, 3)

    def _seconds(self, fn, k: int) -> list:
        ph = (C.c_double * k)()
        fn(self._h, ph)
        return list(ph)

    def close(self):
        if self._h:
            self.lib.topolow_layout_prep_destroy(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tridiagonal_eigenvalues(d, e, device: Optional[int] = None) -> np.ndarray:
    """topolow_tridiagonal_eigenvalues: all eigenvalues of the symmetric tridiagonal matrix (diagonal d, off-diagonal
    e), descending, by Sturm bisection on the device."""
    lib = load()
    d, e = _f64(d).reshape(-1), _f64(e).reshape(-1)
    n = int(d.shape[0])
    if e.shape[0] != max(n - 1, 0):
        raise ValueError("e must have n - 1 entries")
    out = np.empty(max(n, 1), dtype=np.float64)
    _call(lib.topolow_tridiagonal_eigenvalues, _ptr(d), _ptr(e) if n >= 2 else None, n,
          int(options.get("device", -1)) if device is None else int(device), _ptr(out))
    return out[:n]


def symmetric_eigenvalues(a, want_tridiagonal: bool = False, want_eigenvalues: bool = True, device: Optional[int] = None):
    """topolow_symmetric_eigenvalues: the eigenvalues (descending) of the symmetric matrix whose lower triangle is
    a's, by Householder tridiagonalisation and bisection on the device.  Returns the eigenvalues, or with
    want_tridiagonal (eigenvalues or None, d, e): the tridiagonal form."""
    lib = load()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("a must be an n x n matrix")
    a = _f64F(a)
    n = int(a.shape[0])
    eig = np.empty(max(n, 1), dtype=np.float64) if want_eigenvalues else None
    d = np.empty(max(n, 1), dtype=np.float64) if want_tridiagonal else None
    e = np.empty(max(n, 1), dtype=np.float64) if want_tridiagonal else None
    _call(lib.topolow_symmetric_eigenvalues, _ptr(a), n, int(options.get("device", -1)) if device is None else int(device),
          _ptr(d), _ptr(e), _ptr(eig))
    eig = eig[:n] if eig is not None else None
    return (eig, d[:n], e[:max(n - 1, 0)]) if want_tridiagonal else eig


def prepare_layout(values, codes=None, preserve_order: bool = False, order=None, want_dense: bool = True,
                   want_reordered: bool = True, layout: Optional[str] = None) -> PreparedLayout:
    """The reference's pre-processing (R/core.R:269-436) on the GPU: see include/topolow_relax.h, "Prepared layout".
    `values` (f64, NaN = NA) and `codes` (int8 or None) are used where they lie: a C-contiguous matrix goes with
    transposed=1, a Fortran-contiguous one with transposed=0 (`layout` = "C" / "F" forces the reading of a matrix that
    is both); no n x n copy is made of a matrix that is contiguous and of the right dtype.  The n x n outputs come
    back in the layout of the input; values_reordered / codes_reordered stay None where the input order is kept (the
    input is then the reordered matrix).  `order`: the caller's order (an int array, or -1 / None-like [-1] for "keep"),
    for data on which the device declines to order.  (PreparedHandle, created, fetched and destroyed.)"""
    with PreparedHandle(values, codes, preserve_order, order, layout) as h:
        return h.fetch(want_dense, want_reordered)


# ---- host-side helpers (no GPU needed) ---------------------------------------------------
def slab_plan(n: int, slab_stages: int, seed: int, it: int) -> np.ndarray:
    lib = load()
    buf = np.zeros((64, 4), dtype=np.int32)
    ns = lib.topolow_slab_plan(int(n), int(slab_stages), int(seed), int(it), _ptr(buf), 64)
    return buf[:ns].copy()


def slab_stage_count(n: int, slab_stages: int) -> int:
    """Stages of an iteration of n points that asks for slab_stages: its slab geometry's count, without the plan."""
    return int(load().topolow_slab_plan(int(n), int(slab_stages), 0, 0, None, 0))


def slab_stages_for_k(k: float, ndim: int = 5) -> int:
    return int(load().topolow_slab_stages_for_k(float(k), int(ndim)))


def slab_stages_at(it: int, k: float, ndim: int = 5) -> int:
    return int(load().topolow_slab_stages_at(int(it), float(k), int(ndim)))


def gs_pair_order(n: int, seed: int, it: int) -> np.ndarray:
    lib = load()
    buf = np.zeros((n * (n - 1) // 2, 2), dtype=np.int32)
    cnt = lib.topolow_gs_pair_order(int(n), int(seed), int(it), _ptr(buf))
    assert cnt == buf.shape[0]
    return buf


def tilegs_pair_order(n: int, seed: int, it: int) -> np.ndarray:
    lib = load()
    buf = np.zeros((n * (n - 1) // 2, 2), dtype=np.int32)
    cnt = lib.topolow_tilegs_pair_order(int(n), int(seed), int(it), _ptr(buf))
    assert cnt == buf.shape[0], (cnt, buf.shape)
    return buf


def encode_target(d: float, code: int) -> int:
    return int(load().topolow_encode_target(float(d), int(code)))


def decode_target(bits: int):
    c = C.c_int32(0)
    v = load().topolow_decode_target(int(bits), C.byref(c))
    return float(v), int(c.value)


def controller_script(mae_seq, iter_seq, k_seq, k0, window, eps):
    lib = load()
    m, it, ks = _f64(mae_seq), _i32(iter_seq), _f64(k_seq)
    n = int(m.shape[0])
    stopped = C.c_int32(-1)
    snaps = np.zeros(n, dtype=np.int32)
    bm, bk, bi = C.c_double(0), C.c_double(0), C.c_int32(0)
    lib.topolow_controller_script(_ptr(m), _ptr(it), _ptr(ks), n, float(k0), int(window), float(eps),
                                  C.byref(stopped), _ptr(snaps), C.byref(bm), C.byref(bk),
                                  C.byref(bi))
    return dict(stopped_at=int(stopped.value), snapshots=snaps.astype(bool),
                best_mae=float(bm.value), best_k=float(bk.value), best_iter=int(bi.value))


class Session:
    """Device-resident slab session (include/topolow_relax.h, `topolow_session_*`)."""

    def __init__(self, n, ndim, row_begin=0, row_end=None, precision="f32", device=-1):
        self.lib = load()
        self.n, self.ndim = int(n), int(ndim)
        self.row_begin = int(row_begin)
        self.row_end = int(n if row_end is None else row_end)
        self.precision = precision
        self._h = C.c_void_p(None)
        self._err = C.create_string_buffer(512)
        _call(self.lib.topolow_session_create, C.byref(self._h), self.n, self.ndim, self.row_begin, self.row_end,
              _PRECISIONS[precision], int(device), err=self._err)

    def close(self):
        if self._h:
            self.lib.topolow_session_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_dense(self, D, T, degrees):
        D, T = _f64F(D), _i32F(T)
        deg = _i32(degrees)
        _call(self.lib.topolow_session_load_dense, self._h, _ptr(D), _ptr(T), _ptr(deg), err=self._err)

    def load_coo(self, ei, ej, ed, et, degrees):
        ei, ej, ed, et, deg = _i32(ei), _i32(ej), _f64(ed), _i32(et), _i32(degrees)
        _call(self.lib.topolow_session_load_coo, self._h, _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et), int(ei.shape[0]),
              _ptr(deg), err=self._err)

    def load_prepared(self, handle: "PreparedHandle"):
        """topolow_session_load_prepared: targets, degrees and the convergence edge list from a PreparedHandle, device
        to device -- what load_dense + set_edges do with the arrays handle.fetch() returns."""
        _call(self.lib.topolow_session_load_prepared, self._h, handle._h if handle is not None else None, err=self._err)

    @property
    def encoded_ptr(self) -> int:
        return int(self.lib.topolow_session_encoded_ptr(self._h) or 0)

    @property
    def encoded_ld(self) -> int:
        return int(self.lib.topolow_session_encoded_ld(self._h))

    def commit_encoded(self, degrees):
        deg = _i32(degrees)
        assert deg.shape[0] == self.n
        _call(self.lib.topolow_session_commit_encoded, self._h, _ptr(deg), err=self._err)

    def set_edges(self, ei, ej, ed, et):
        ei, ej, ed, et = _i32(ei), _i32(ej), _f64(ed), _i32(et)
        _call(self.lib.topolow_session_set_edges, self._h, _ptr(ei), _ptr(ej), _ptr(ed), _ptr(et), int(ei.shape[0]),
              err=self._err)

    def set_positions(self, pos):
        pos = _f64F(pos)
        assert pos.shape == (self.n, self.ndim)
        _call(self.lib.topolow_session_set_positions, self._h, _ptr(pos), err=self._err)

    def get_positions(self):
        out = np.zeros((self.n, self.ndim), dtype=np.float64, order="F")
        _call(self.lib.topolow_session_get_positions, self._h, _ptr(out), err=self._err)
        return np.ascontiguousarray(out)

    def begin(self, n_iter, k0, cooling_rate, c_repulsion, relative_epsilon=1e-4,
              convergence_window=5, convergence_check_freq=3, seed=0, slab_stages=0):
        _call(self.lib.topolow_session_begin, self._h, int(n_iter), float(k0), float(cooling_rate), float(c_repulsion),
              float(relative_epsilon), int(convergence_window), int(convergence_check_freq),
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(slab_stages), err=self._err)

    def enqueue(self, max_iters) -> int:
        enq = C.c_int32(0)
        _call(self.lib.topolow_session_enqueue, self._h, int(max_iters), C.byref(enq), err=self._err)
        return int(enq.value)

    def wait(self):
        """Waits for the launches enqueued so far; a check waiting to ride on the next sweep stays pending."""
        _call(self.lib.topolow_session_wait, self._h, err=self._err)

    def sync(self):
        it, st, mae = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        _call(self.lib.topolow_session_sync, self._h, C.byref(it), C.byref(st), C.byref(mae), err=self._err)
        return int(it.value), bool(st.value), float(mae.value)

    def finish(self, download: bool = True) -> NativeResult:
        """download = False: the positions stay on the device (score_pairs reads them there); `positions` is None."""
        out = _RunOut(self.n, self.ndim, positions=download)
        _call(self.lib.topolow_session_finish, self._h, *out.args, err=self._err)
        return out.result()

    def hold_out(self, pair_i, pair_j, degrees):
        """The listed pairs (caller's labels) become unmeasured for the coming runs, `degrees` the fold's degrees
        (topolow_session_hold_out); outside a run only."""
        pi, pj, deg = _i32(pair_i), _i32(pair_j), _i32(degrees)
        assert pi.shape == pj.shape and deg.shape[0] == self.n
        _call(self.lib.topolow_session_hold_out, self._h, _ptr(pi), _ptr(pj), int(pi.shape[0]), _ptr(deg), err=self._err)

    def restore_held_out(self, degrees):
        """Puts the held-out cells back, with the full matrix's degrees."""
        deg = _i32(degrees)
        assert deg.shape[0] == self.n
        _call(self.lib.topolow_session_restore_held_out, self._h, _ptr(deg), err=self._err)

    def score_pairs(self, pair_i, pair_j, truth):
        """(sum |truth - distance|, count) over the pairs on the positions finish() restores, on the device."""
        pi, pj, t = _i32(pair_i), _i32(pair_j), _f64(truth)
        assert pi.shape == pj.shape == t.shape
        sc = _SumCount()
        _call(self.lib.topolow_session_score_pairs, self._h, _ptr(pi), _ptr(pj), _ptr(t), int(pi.shape[0]), *sc.refs,
              err=self._err)
        return sc.values()

    def run(self, chunk=64):
        while self.enqueue(chunk) > 0:
            pass
        return self.sync()

    def check_trace(self) -> np.ndarray:
        """(iteration, MAE, k) of every convergence check of the current run, shape (checks, 3)."""
        n = C.c_int32(0)
        _check(self.lib.topolow_session_check_trace(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(int(n.value), 1), 3), dtype=np.float64)
        _check(self.lib.topolow_session_check_trace(self._h, _ptr(out), int(n.value), C.byref(n)))
        return out[: int(n.value)]

    def set_relabel(self, seed: int):
        """Store the points in a random order drawn from `seed` (0 = the caller's order); before loading."""
        _call(self.lib.topolow_session_set_relabel, self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), err=self._err)

    def labels(self) -> np.ndarray:
        """session label -> caller's label."""
        out = np.empty(self.n, dtype=np.int32)
        self.lib.topolow_session_labels(self._h, _ptr(out))
        return out

    def set_schedule(self, schedule: str):
        rc = self.lib.topolow_session_set_schedule(self._h, _SCHEDULES[schedule])
        if rc != OK:
            raise NativeError(rc, "schedule not available for this session")

    def set_profiling(self, enable: bool):
        self.lib.topolow_session_set_profiling(self._h, int(bool(enable)))

    def profile(self):
        """(stage_ms, stage_launches, check_ms, checks) since profiling was enabled."""
        return self._profile(self.lib.topolow_session_profile, 2)

    def _profile(self, fn, k: int):
        out = _SumCount(k)
        _call(fn, self._h, *out.refs, err=self._err)
        return out.values()

    def profile_symmetric(self):
        """(plain_ms, plain_iterations, fused_ms, fused_iterations) of the iterations that ran as a symmetric sweep +
        apply since profiling was enabled (not part of profile() / profile_fused())."""
        return self._profile(self.lib.topolow_session_profile_symmetric, 2)

    def profile_fused(self):
        """(ms, launches) of the stage launches that also reduced a check's MAE; ask before profile()."""
        return self._profile(self.lib.topolow_session_profile_fused, 1)

    def set_stream(self, hip_stream, external: bool = True):
        """hip_stream: integer hipStream_t (0/None = the device's default stream)."""
        self.lib.topolow_session_set_stream(self._h, C.c_void_p(hip_stream or None),
                                            int(bool(external)))

    @property
    def stream(self) -> int:
        return int(self.lib.topolow_session_stream(self._h) or 0)

    @property
    def position_rows(self) -> int:
        return int(self.lib.topolow_session_position_rows(self._h))

    @property
    def uses_dense_mae(self) -> bool:
        return bool(self.lib.topolow_session_uses_dense_mae(self._h))

    @property
    def stage_launches(self) -> int:
        return int(self.lib.topolow_session_stage_launches(self._h))

    @property
    def checks_in_apply(self) -> int:
        """Checks of the current run whose controller step rode in a symmetric apply's launch."""
        return int(self.lib.topolow_session_checks_in_apply(self._h))

    @property
    def symm_grid(self) -> int:
        """Workgroups of the symmetric sweep this session has built, 0 if none (topolow_session_symm_grid)."""
        return int(self.lib.topolow_session_symm_grid(self._h))

    @property
    def bytes_per_iteration(self) -> int:
        return int(self.lib.topolow_session_bytes_per_iteration(self._h))

    def stage(self, d_pos_in: int, d_pos_out: int, it: int, stage: int, n_stages: int, k: float):
        _call(self.lib.topolow_session_stage, self._h, C.c_void_p(d_pos_in), C.c_void_p(d_pos_out), int(it), int(stage),
              int(n_stages), float(k), err=self._err)

    def check_partial(self, d_pos: int, d_out2: int):
        """Enqueue this block's share of the convergence MAE on the positions at d_pos: two doubles
        (sum, count) at the device address d_out2."""
        _call(self.lib.topolow_session_check_partial, self._h, C.c_void_p(d_pos), C.c_void_p(d_out2), err=self._err)

    def controller_step(self, d_total2: int, d_pos: int, iter1: int, k_after: float):
        """Enqueue the controller (reference :303-357) on the all-reduced (sum, count) at d_total2."""
        _call(self.lib.topolow_session_controller_step, self._h, C.c_void_p(d_total2), C.c_void_p(d_pos), int(iter1),
              float(k_after), err=self._err)

    @property
    def can_fuse_checks(self) -> bool:
        return bool(self.lib.topolow_session_can_fuse_checks(self._h))

    def stage_fused(self, d_pos_in: int, d_pos_out: int, it: int, k: float, d_out2: int):
        """The single stage of iteration `it`, also reducing this block's share of the MAE of d_pos_in."""
        _call(self.lib.topolow_session_stage_fused, self._h, C.c_void_p(d_pos_in), C.c_void_p(d_pos_out), int(it), float(k),
              C.c_void_p(d_out2), err=self._err)

    # ---- one-stage iterations as the symmetric sweep sharded over the processes (include/topolow_relax.h) ----
    @property
    def degree_terms_ptr(self) -> int:
        """Device float[n]: degree + 1 per point; a row-block session knows its own rows' (the caller completes it)."""
        return int(self.lib.topolow_session_degree_terms(self._h) or 0)

    @property
    def has_thresholds(self) -> bool:
        return bool(self.lib.topolow_session_has_thresholds(self._h))

    def symm_segment_eligible(self, n_segments: int) -> bool:
        return bool(self.lib.topolow_session_symm_segment_eligible(self._h, int(n_segments)))

    @property
    def can_fuse_segment_checks(self) -> bool:
        """Whether symm_segment_sweep may reduce a check (d_out2): fp32, fused checks enabled, the MAE reduced from the
        block (topolow_session_can_fuse_segment_checks); it is refused otherwise."""
        return bool(self.lib.topolow_session_can_fuse_segment_checks(self._h))

    def symm_segment_build(self, segment: int, n_segments: int, d_rows: int, row_first: int, n_rows: int,
                           any_threshold: bool):
        _call(self.lib.topolow_session_symm_segment_build, self._h, int(segment), int(n_segments), C.c_void_p(d_rows),
              int(row_first), int(n_rows), int(bool(any_threshold)), err=self._err)

    @property
    def symm_moves_ptr(self) -> int:
        """Device float[n][ndim]: the segment's share of every point's move after symm_segment_sweep."""
        return int(self.lib.topolow_session_symm_moves(self._h) or 0)

    def symm_segment_sweep(self, d_pos_in: int, it: int, k: float, d_out2: int = 0):
        _call(self.lib.topolow_session_symm_segment_sweep, self._h, C.c_void_p(d_pos_in), int(it), float(k),
              C.c_void_p(d_out2) if d_out2 else None, err=self._err)

    def symm_segment_apply(self, d_pos_in: int, d_pos_out: int, it: int):
        _call(self.lib.topolow_session_symm_segment_apply, self._h, C.c_void_p(d_pos_in), C.c_void_p(d_pos_out), int(it),
              err=self._err)

    def first_nonfinite(self) -> int:
        it = C.c_int32(0)
        _check(self.lib.topolow_session_first_nonfinite(self._h, C.byref(it)), self._err)
        return int(it.value)

    def edge_error(self, d_pos: int):
        sc = _SumCount()
        _call(self.lib.topolow_session_edge_error, self._h, C.c_void_p(d_pos), *sc.refs, err=self._err)
        return sc.values()
