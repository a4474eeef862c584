"""ctypes binding of libuvs_solver.so (the HIP C ABI of include/uvs_solver.h).

Plumbing only: every number is produced by the HIP kernels in csrc/.  Loading
fails loudly when the shared library has not been built, and `Solver(...)`
fails loudly (RuntimeError) when no GPU is present -- there is no CPU path.
"""
import ctypes as C
import os
import time

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UVS_SOLVER_LIB", os.path.join(_HERE, "libuvs_solver.so"))      # the override is for A/B builds of the same library (tuning experiments)
_lib = None

EXPORTS = [
    "uvs_abi_version", "uvs_default_options", "uvs_create", "uvs_destroy", "uvs_last_error", "uvs_status_string",
    "uvs_solve_window", "uvs_batch_upload", "uvs_batch_solve", "uvs_batch_download", "uvs_batch_stream", "uvs_evaluate", "uvs_marginalize", "uvs_marginalize_resident", "uvs_marginalize_batch",
    "uvs_reduced_dim", "uvs_pg_create", "uvs_pg_destroy", "uvs_pg_last_error", "uvs_pg_optimize", "uvs_pg_debug_step",
    "uvs_lc_create", "uvs_lc_destroy", "uvs_lc_last_error", "uvs_lc_verify", "uvs_lc_debug_pair",
    "uvs_vp_create", "uvs_vp_destroy", "uvs_vp_last_error", "uvs_vp_estimate", "uvs_vp_last_device_ms", "uvs_vp_debug_frame",
    "uvs_kf_create", "uvs_kf_destroy", "uvs_kf_last_error", "uvs_kf_extract", "uvs_kf_last_device_ms", "uvs_kf_debug_frame",
    "uvs_ft_create", "uvs_ft_destroy", "uvs_ft_last_error", "uvs_ft_reset", "uvs_ft_track", "uvs_ft_last_device_ms", "uvs_ft_debug_pyramid", "uvs_ft_debug_point",
    "uvs_ft_set_max_candidates", "uvs_ft_set_mask", "uvs_ft_detect", "uvs_ft_last_detect_device_ms", "uvs_ft_debug_detect",
    "uvs_ft_reject", "uvs_ft_last_reject_device_ms", "uvs_ft_debug_reject",
    "uvs_ft_set_equalize", "uvs_ft_equalize", "uvs_ft_last_equalize_device_ms", "uvs_ft_debug_equalize",
    "uvs_lt_create", "uvs_lt_destroy", "uvs_lt_last_error", "uvs_lt_reset", "uvs_lt_track", "uvs_lt_match", "uvs_lt_last_device_ms", "uvs_lt_debug_line",
    "uvs_lt_gauss_tables",
    "uvs_lt_detect", "uvs_lt_detect_track", "uvs_lt_last_detect_device_ms", "uvs_lt_debug_detect",
    "uvs_lt_set_undistort", "uvs_lt_set_remap", "uvs_lt_get_remap", "uvs_lt_undistort", "uvs_lt_last_undistort_device_ms",
    "uvs_ft_set_camera_model", "uvs_kf_set_camera_model", "uvs_ft_lift", "uvs_ft_project", "uvs_lt_set_undistort_model",
    "uvs_pr_check_vocabulary", "uvs_pr_create", "uvs_pr_destroy", "uvs_pr_last_error", "uvs_pr_size", "uvs_pr_clear", "uvs_pr_transform", "uvs_pr_add",
    "uvs_pr_query", "uvs_pr_detect", "uvs_pr_last_device_ms",
    "uvs_tri_create", "uvs_tri_destroy", "uvs_tri_last_error", "uvs_tri_set_init_depth", "uvs_tri_triangulate", "uvs_tri_check_lines", "uvs_tri_shift_depth",
    "uvs_tri_last_device_ms",
    "uvs_imu_create", "uvs_imu_destroy", "uvs_imu_last_error", "uvs_imu_set_noise", "uvs_imu_preintegrate", "uvs_imu_last_device_ms",
    "uvs_rp_create", "uvs_rp_destroy", "uvs_rp_last_error", "uvs_rp_default_params", "uvs_rp_relative_pose", "uvs_rp_last_device_ms",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.uvs_abi_version.restype = C.c_int
        L.uvs_default_options.argtypes = [C.POINTER(abi.Options)]
        L.uvs_create.argtypes = [C.POINTER(abi.Options), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.uvs_create.restype = C.c_int
        L.uvs_destroy.argtypes = [C.c_void_p]
        L.uvs_last_error.argtypes = [C.c_void_p]; L.uvs_last_error.restype = C.c_char_p
        L.uvs_status_string.argtypes = [C.c_int]; L.uvs_status_string.restype = C.c_char_p
        L.uvs_solve_window.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.POINTER(abi.StateC), C.POINTER(abi.Report)]
        L.uvs_solve_window.restype = C.c_int
        L.uvs_batch_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(abi.WindowC))]
        L.uvs_batch_upload.restype = C.c_int
        L.uvs_batch_solve.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.uvs_batch_solve.restype = C.c_int
        L.uvs_batch_download.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.StateC), C.POINTER(abi.Report)]
        L.uvs_batch_download.restype = C.c_int
        L.uvs_batch_stream.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.POINTER(abi.WindowC)), C.POINTER(abi.StateC), C.POINTER(abi.Report), C.POINTER(C.c_double)]
        L.uvs_batch_stream.restype = C.c_int
        L.uvs_evaluate.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_int, C.POINTER(abi.EvalC)]
        L.uvs_evaluate.restype = C.c_int
        L.uvs_marginalize.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_int, C.POINTER(abi.Prior)]
        L.uvs_marginalize.restype = C.c_int
        L.uvs_marginalize_resident.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_int, C.POINTER(abi.Prior)]
        L.uvs_marginalize_resident.restype = C.c_int
        L.uvs_marginalize_resident_begin.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_int]; L.uvs_marginalize_resident_begin.restype = C.c_int
        L.uvs_marginalize_wait.argtypes = [C.c_void_p, C.POINTER(abi.Prior)]; L.uvs_marginalize_wait.restype = C.c_int
        L.uvs_debug_first_iteration.argtypes = [C.c_void_p, C.POINTER(abi.WindowC)] + [abi.c_double_p] * 6
        L.uvs_debug_first_iteration.restype = C.c_int
        L.uvs_debug_step.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.c_int, C.c_int, abi.c_double_p, C.c_int, abi.c_double_p, abi.c_double_p]
        L.uvs_debug_step.restype = C.c_int
        L.uvs_reduced_dim.argtypes = [C.POINTER(abi.Options)]; L.uvs_reduced_dim.restype = C.c_int
        L.uvs_large_begin.argtypes = [C.c_void_p, C.POINTER(abi.WindowC)]; L.uvs_large_begin.restype = C.c_int
        L.uvs_large_set_nranks.argtypes = [C.c_void_p, C.c_int]; L.uvs_large_set_nranks.restype = C.c_int
        for name in ("uvs_large_need_linearize", "uvs_large_linearize", "uvs_large_step", "uvs_large_decide", "uvs_large_done"):
            getattr(L, name).argtypes = [C.c_void_p]; getattr(L, name).restype = C.c_int
        L.uvs_large_reduced.argtypes = [C.c_void_p, C.POINTER(C.c_int)]; L.uvs_large_reduced.restype = C.c_void_p
        L.uvs_large_scalars.argtypes = [C.c_void_p, C.POINTER(C.c_int)]; L.uvs_large_scalars.restype = C.c_void_p
        L.uvs_large_exchange_host.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, C.c_int]; L.uvs_large_exchange_host.restype = C.c_int
        L.uvs_large_local_x2.argtypes = [C.c_void_p]; L.uvs_large_local_x2.restype = C.c_double
        L.uvs_large_set_landmark_x2.argtypes = [C.c_void_p, C.c_double]
        L.uvs_large_set_debug_step.argtypes = [C.c_void_p, C.c_int]; L.uvs_large_set_debug_step.restype = C.c_int
        L.uvs_large_debug_step.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_double_p]; L.uvs_large_debug_step.restype = C.c_int
        L.uvs_large_finish.argtypes = [C.c_void_p, C.POINTER(abi.StateC), C.POINTER(abi.Report)]; L.uvs_large_finish.restype = C.c_int
        L.uvs_large_solve.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.POINTER(abi.StateC), C.POINTER(abi.Report)]; L.uvs_large_solve.restype = C.c_int
        L.uvs_large_comm_unique_id.argtypes = [C.c_char_p]; L.uvs_large_comm_unique_id.restype = C.c_int
        L.uvs_large_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]; L.uvs_large_comm_init.restype = C.c_int
        L.uvs_large_comm_destroy.argtypes = [C.c_void_p]; L.uvs_large_comm_destroy.restype = None
        L.uvs_large_solve_fused.argtypes = [C.c_void_p, C.POINTER(abi.WindowC), C.POINTER(abi.StateC), C.POINTER(abi.Report), C.POINTER(C.c_float)]; L.uvs_large_solve_fused.restype = C.c_int
        L.uvs_pg_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]; L.uvs_pg_create.restype = C.c_int
        L.uvs_pg_destroy.argtypes = [C.c_void_p]; L.uvs_pg_destroy.restype = None
        L.uvs_pg_last_error.argtypes = [C.c_void_p]; L.uvs_pg_last_error.restype = C.c_char_p
        L.uvs_pg_optimize.argtypes = [C.c_void_p, C.POINTER(abi.PgProblem), abi.c_double_p, C.POINTER(abi.PgReport)]; L.uvs_pg_optimize.restype = C.c_int
        L.uvs_pg_debug_step.argtypes = [C.c_void_p, C.POINTER(abi.PgProblem), C.c_double, abi.c_double_p, abi.c_double_p]
        L.uvs_pg_debug_step.restype = C.c_int
        L.uvs_lc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]; L.uvs_lc_create.restype = C.c_int
        L.uvs_lc_destroy.argtypes = [C.c_void_p]; L.uvs_lc_destroy.restype = None
        L.uvs_lc_last_error.argtypes = [C.c_void_p]; L.uvs_lc_last_error.restype = C.c_char_p
        L.uvs_lc_verify.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.LcPair), abi.c_double_p, abi.c_double_p, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_uint8), C.POINTER(abi.LcResult)]
        L.uvs_lc_verify.restype = C.c_int
        L.uvs_lc_debug_pair.argtypes = [C.c_void_p, C.POINTER(abi.LcPair), abi.c_double_p, abi.c_double_p, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint8), C.POINTER(abi.LcResult), abi.c_double_p]
        L.uvs_lc_debug_pair.restype = C.c_int
        L.uvs_vp_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]; L.uvs_vp_create.restype = C.c_int
        L.uvs_vp_destroy.argtypes = [C.c_void_p]; L.uvs_vp_destroy.restype = None
        L.uvs_vp_last_error.argtypes = [C.c_void_p]; L.uvs_vp_last_error.restype = C.c_char_p
        L.uvs_vp_estimate.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.VpFrame), C.POINTER(abi.VpCamera), C.c_double, C.POINTER(C.c_int32),
                                      abi.c_double_p, C.POINTER(abi.VpResult)]
        L.uvs_vp_estimate.restype = C.c_int
        L.uvs_vp_last_device_ms.argtypes = [C.c_void_p]; L.uvs_vp_last_device_ms.restype = C.c_double
        L.uvs_vp_debug_frame.argtypes = [C.c_void_p, C.POINTER(abi.VpFrame), C.POINTER(abi.VpCamera), C.c_double, abi.c_double_p, C.POINTER(C.c_int32),
                                         abi.c_double_p, abi.c_double_p, abi.c_double_p, C.POINTER(C.c_int32), C.POINTER(abi.VpResult)]
        L.uvs_vp_debug_frame.restype = C.c_int
        L.uvs_kf_create.argtypes = [C.c_int] * 6 + [abi.c_i32_p] * 4 + [C.POINTER(C.c_void_p)]; L.uvs_kf_create.restype = C.c_int
        L.uvs_kf_destroy.argtypes = [C.c_void_p]; L.uvs_kf_destroy.restype = None
        L.uvs_kf_last_error.argtypes = [C.c_void_p]; L.uvs_kf_last_error.restype = C.c_char_p
        L.uvs_kf_extract.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.KfFrame), C.POINTER(abi.KfCamera), abi.c_i32_p, abi.c_u8_p, abi.c_double_p,
                                     abi.c_u64_p, abi.c_u64_p, C.POINTER(abi.KfResult)]
        L.uvs_kf_extract.restype = C.c_int
        L.uvs_kf_last_device_ms.argtypes = [C.c_void_p]; L.uvs_kf_last_device_ms.restype = C.c_double
        L.uvs_kf_debug_frame.argtypes = [C.c_void_p, C.POINTER(abi.KfFrame), C.POINTER(abi.KfCamera), abi.c_u8_p, abi.c_u8_p, abi.c_i32_p, abi.c_u8_p,
                                         abi.c_double_p, abi.c_u64_p, abi.c_u64_p, C.POINTER(abi.KfResult)]
        L.uvs_kf_debug_frame.restype = C.c_int
        L.uvs_ft_create.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_void_p)]; L.uvs_ft_create.restype = C.c_int
        L.uvs_ft_destroy.argtypes = [C.c_void_p]; L.uvs_ft_destroy.restype = None
        L.uvs_ft_last_error.argtypes = [C.c_void_p]; L.uvs_ft_last_error.restype = C.c_char_p
        L.uvs_ft_reset.argtypes = [C.c_void_p, C.c_int]; L.uvs_ft_reset.restype = C.c_int
        L.uvs_ft_track.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.FtItem), C.POINTER(abi.KfCamera), abi.c_double_p, abi.c_i32_p, abi.c_i32_p,
                                   abi.c_double_p, abi.c_i32_p]
        L.uvs_ft_track.restype = C.c_int
        L.uvs_ft_last_device_ms.argtypes = [C.c_void_p]; L.uvs_ft_last_device_ms.restype = C.c_double
        L.uvs_ft_debug_pyramid.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_u8_p, C.c_int64]; L.uvs_ft_debug_pyramid.restype = C.c_int
        L.uvs_ft_debug_point.argtypes = [C.c_void_p, C.POINTER(abi.FtItem), C.POINTER(abi.KfCamera), abi.c_double_p, abi.c_double_p, abi.c_i32_p,
                                         abi.c_i32_p, abi.c_double_p]
        L.uvs_ft_debug_point.restype = C.c_int
        L.uvs_ft_set_max_candidates.argtypes = [C.c_void_p, C.c_int]; L.uvs_ft_set_max_candidates.restype = C.c_int
        L.uvs_ft_set_mask.argtypes = [C.c_void_p, C.c_int, abi.c_u8_p, C.c_int, C.c_int]; L.uvs_ft_set_mask.restype = C.c_int
        L.uvs_ft_detect.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.FtDetectItem), C.c_double, C.c_int, C.POINTER(abi.KfCamera), abi.c_i32_p,
                                    abi.c_double_p, abi.c_double_p, C.POINTER(abi.FtDetectResult)]
        L.uvs_ft_detect.restype = C.c_int
        L.uvs_ft_last_detect_device_ms.argtypes = [C.c_void_p]; L.uvs_ft_last_detect_device_ms.restype = C.c_double
        L.uvs_ft_debug_detect.argtypes = [C.c_void_p, C.POINTER(abi.FtDetectItem), C.c_double, C.c_int, C.POINTER(abi.KfCamera), abi.c_double_p, abi.c_u8_p,
                                          abi.c_i32_p, abi.c_double_p, abi.c_i32_p, abi.c_double_p, abi.c_double_p, C.POINTER(abi.FtDetectResult)]
        L.uvs_ft_debug_detect.restype = C.c_int
        L.uvs_ft_reject.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.FtRejectItem), C.c_double, C.c_double, abi.c_u8_p, C.POINTER(abi.FtRejectResult)]
        L.uvs_ft_reject.restype = C.c_int
        L.uvs_ft_last_reject_device_ms.argtypes = [C.c_void_p]; L.uvs_ft_last_reject_device_ms.restype = C.c_double
        L.uvs_ft_debug_reject.argtypes = [C.c_void_p, C.POINTER(abi.FtRejectItem), C.c_double, C.c_double, abi.c_i32_p, abi.c_double_p, abi.c_i32_p,
                                          abi.c_u8_p, C.POINTER(abi.FtRejectResult)]
        L.uvs_ft_debug_reject.restype = C.c_int
        L.uvs_ft_set_equalize.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int]; L.uvs_ft_set_equalize.restype = C.c_int
        L.uvs_ft_equalize.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.FtImage), C.c_double, C.c_int, C.c_int, abi.c_u8_p]; L.uvs_ft_equalize.restype = C.c_int
        L.uvs_ft_last_equalize_device_ms.argtypes = [C.c_void_p]; L.uvs_ft_last_equalize_device_ms.restype = C.c_double
        L.uvs_ft_debug_equalize.argtypes = [C.c_void_p, C.POINTER(abi.FtImage), C.c_double, C.c_int, C.c_int, abi.c_i32_p, abi.c_u8_p, abi.c_u8_p, abi.c_i32_p]
        L.uvs_ft_debug_equalize.restype = C.c_int
        L.uvs_lt_create.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_void_p)]; L.uvs_lt_create.restype = C.c_int
        L.uvs_lt_destroy.argtypes = [C.c_void_p]; L.uvs_lt_destroy.restype = None
        L.uvs_lt_last_error.argtypes = [C.c_void_p]; L.uvs_lt_last_error.restype = C.c_char_p
        L.uvs_lt_reset.argtypes = [C.c_void_p, C.c_int]; L.uvs_lt_reset.restype = C.c_int
        L.uvs_lt_track.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.LtItem), abi.c_u8_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p, C.POINTER(abi.LtResult)]
        L.uvs_lt_track.restype = C.c_int
        L.uvs_lt_match.argtypes = [C.c_void_p, C.c_int, abi.c_u8_p, abi.c_i32_p, C.c_int, abi.c_u8_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p]
        L.uvs_lt_match.restype = C.c_int
        L.uvs_lt_last_device_ms.argtypes = [C.c_void_p]; L.uvs_lt_last_device_ms.restype = C.c_double
        L.uvs_lt_debug_line.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, abi.c_double_p, abi.c_i32_p, C.POINTER(C.c_int64), abi.c_double_p, abi.c_u8_p]
        L.uvs_lt_debug_line.restype = C.c_int
        L.uvs_lt_gauss_tables.argtypes = [abi.c_double_p, abi.c_double_p]; L.uvs_lt_gauss_tables.restype = None
        det_args = [C.c_void_p, C.c_int, C.POINTER(abi.LtDetItem), C.POINTER(abi.LtDetParams), abi.c_double_p, abi.c_double_p, abi.c_i32_p, C.POINTER(abi.LtDetResult)]
        L.uvs_lt_detect.argtypes = det_args; L.uvs_lt_detect.restype = C.c_int
        L.uvs_lt_detect_track.argtypes = det_args + [abi.c_u8_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p, C.POINTER(abi.LtResult)]
        L.uvs_lt_detect_track.restype = C.c_int
        L.uvs_lt_last_detect_device_ms.argtypes = [C.c_void_p]; L.uvs_lt_last_detect_device_ms.restype = C.c_double
        L.uvs_lt_debug_detect.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.POINTER(abi.LtDetParams), abi.c_u8_p, C.POINTER(C.c_uint32), abi.c_u8_p,
                                          abi.c_u8_p, abi.c_i32_p, abi.c_i32_p, abi.c_u8_p]
        L.uvs_lt_debug_detect.restype = C.c_int
        L.uvs_lt_set_undistort.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.KfCamera), C.c_int, C.c_int, C.c_int, C.c_int]; L.uvs_lt_set_undistort.restype = C.c_int
        L.uvs_lt_set_remap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, abi.c_i32_p]; L.uvs_lt_set_remap.restype = C.c_int
        L.uvs_lt_get_remap.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p]; L.uvs_lt_get_remap.restype = C.c_int
        L.uvs_lt_undistort.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.LtDetItem), abi.c_u8_p]; L.uvs_lt_undistort.restype = C.c_int
        L.uvs_lt_last_undistort_device_ms.argtypes = [C.c_void_p]; L.uvs_lt_last_undistort_device_ms.restype = C.c_double
        cam_p = C.POINTER(abi.CameraModel)
        L.uvs_ft_set_camera_model.argtypes = [C.c_void_p, cam_p]; L.uvs_ft_set_camera_model.restype = C.c_int
        L.uvs_kf_set_camera_model.argtypes = [C.c_void_p, cam_p]; L.uvs_kf_set_camera_model.restype = C.c_int
        L.uvs_ft_lift.argtypes = [C.c_void_p, cam_p, C.c_int, abi.c_double_p, abi.c_double_p, abi.c_double_p]; L.uvs_ft_lift.restype = C.c_int
        L.uvs_ft_project.argtypes = [C.c_void_p, cam_p, C.c_int, abi.c_double_p, abi.c_double_p]; L.uvs_ft_project.restype = C.c_int
        L.uvs_lt_set_undistort_model.argtypes = [C.c_void_p, C.c_int, cam_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_double] * 4
        L.uvs_lt_set_undistort_model.restype = C.c_int
        voc_args = [C.c_int] * 5 + [abi.c_i32_p, abi.c_i32_p, abi.c_double_p, abi.c_u64_p, C.c_int, abi.c_i32_p, abi.c_i32_p]
        L.uvs_pr_check_vocabulary.argtypes = voc_args + [C.c_char_p, C.c_int]; L.uvs_pr_check_vocabulary.restype = C.c_int
        L.uvs_pr_create.argtypes = [C.c_int] + voc_args + [C.c_int, C.c_int, C.POINTER(C.c_void_p)]; L.uvs_pr_create.restype = C.c_int
        L.uvs_pr_destroy.argtypes = [C.c_void_p]; L.uvs_pr_destroy.restype = None
        L.uvs_pr_last_error.argtypes = [C.c_void_p]; L.uvs_pr_last_error.restype = C.c_char_p
        L.uvs_pr_size.argtypes = [C.c_void_p]; L.uvs_pr_size.restype = C.c_int
        L.uvs_pr_clear.argtypes = [C.c_void_p]; L.uvs_pr_clear.restype = C.c_int
        L.uvs_pr_transform.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_u64_p, abi.c_i32_p, abi.c_double_p, abi.c_i32_p, abi.c_i32_p, abi.c_double_p]
        L.uvs_pr_transform.restype = C.c_int
        L.uvs_pr_add.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_u64_p, abi.c_i32_p]; L.uvs_pr_add.restype = C.c_int
        L.uvs_pr_query.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_u64_p, C.c_int, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p, abi.c_double_p]
        L.uvs_pr_query.restype = C.c_int
        L.uvs_pr_detect.argtypes = [C.c_void_p, C.c_int, abi.c_u64_p, C.c_int, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p, abi.c_double_p]
        L.uvs_pr_detect.restype = C.c_int
        L.uvs_pr_last_device_ms.argtypes = [C.c_void_p, C.c_int]; L.uvs_pr_last_device_ms.restype = C.c_double
        L.uvs_tri_create.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_void_p)]; L.uvs_tri_create.restype = C.c_int
        L.uvs_tri_destroy.argtypes = [C.c_void_p]; L.uvs_tri_destroy.restype = None
        L.uvs_tri_last_error.argtypes = [C.c_void_p]; L.uvs_tri_last_error.restype = C.c_char_p
        L.uvs_tri_set_init_depth.argtypes = [C.c_void_p, C.c_double]; L.uvs_tri_set_init_depth.restype = C.c_int
        L.uvs_tri_triangulate.argtypes = [C.c_void_p, C.POINTER(abi.TriBatch), C.c_double, abi.c_double_p, abi.c_i32_p, abi.c_double_p, abi.c_i32_p]
        L.uvs_tri_triangulate.restype = C.c_int
        L.uvs_tri_check_lines.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_double_p, C.c_int, abi.c_i32_p, abi.c_i32_p, abi.c_double_p, abi.c_double_p,
                                          abi.c_double_p, abi.c_i32_p]
        L.uvs_tri_check_lines.restype = C.c_int
        L.uvs_tri_shift_depth.argtypes = [C.c_void_p, C.c_int] + [abi.c_double_p] * 7 + [abi.c_i32_p]; L.uvs_tri_shift_depth.restype = C.c_int
        L.uvs_tri_last_device_ms.argtypes = [C.c_void_p]; L.uvs_tri_last_device_ms.restype = C.c_double
        L.uvs_imu_create.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_void_p)]; L.uvs_imu_create.restype = C.c_int
        L.uvs_imu_destroy.argtypes = [C.c_void_p]; L.uvs_imu_destroy.restype = None
        L.uvs_imu_last_error.argtypes = [C.c_void_p]; L.uvs_imu_last_error.restype = C.c_char_p
        L.uvs_imu_set_noise.argtypes = [C.c_void_p] + [C.c_double] * 4; L.uvs_imu_set_noise.restype = C.c_int
        L.uvs_imu_preintegrate.argtypes = [C.c_void_p, C.POINTER(abi.ImuBatch), C.c_void_p, abi.c_double_p, abi.c_double_p, abi.c_double_p]
        L.uvs_imu_preintegrate.restype = C.c_int
        L.uvs_imu_last_device_ms.argtypes = [C.c_void_p]; L.uvs_imu_last_device_ms.restype = C.c_double
        L.uvs_rp_create.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_void_p)]; L.uvs_rp_create.restype = C.c_int
        L.uvs_rp_destroy.argtypes = [C.c_void_p]; L.uvs_rp_destroy.restype = None
        L.uvs_rp_last_error.argtypes = [C.c_void_p]; L.uvs_rp_last_error.restype = C.c_char_p
        L.uvs_rp_default_params.argtypes = [C.POINTER(abi.RpParams)]; L.uvs_rp_default_params.restype = None
        L.uvs_rp_relative_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.RpItem), C.POINTER(abi.RpParams), abi.c_u8_p, C.c_void_p, C.c_int, C.c_void_p]
        L.uvs_rp_relative_pose.restype = C.c_int
        L.uvs_rp_last_device_ms.argtypes = [C.c_void_p, C.c_int]; L.uvs_rp_last_device_ms.restype = C.c_double
        _lib = L
    return _lib


def _camera_arg(camera):
    """The `camera` argument of the calls that lift: a pointer to a uvs_kf_camera, or NULL for None (a handle that holds a camera model)."""
    return None if camera is None else C.pointer(abi.kf_camera(camera))


def _model_arg(model):
    return None if model is None else C.pointer(abi.camera_model(model))


class _DevPtr:
    """Exposes a raw device pointer through __cuda_array_interface__ so that torch can wrap it without a copy."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 3, "strides": None}


def _device_tensor(ptr, n, device=None):
    import torch
    return torch.as_tensor(_DevPtr(ptr, n), device=device or "cuda")


class _Handle:
    """Owns one native handle of the unit whose C calls start with `_UNIT`: <_UNIT>_create, _destroy and _last_error."""

    _UNIT = None

    def _create(self, *args):
        """<_UNIT>_create(*args, &handle), or a RuntimeError."""
        self._h = C.c_void_p()
        rc = getattr(lib(), self._UNIT + "_create")(*args, C.byref(self._h))
        if rc != abi.UVS_OK:
            raise RuntimeError(f"{self._UNIT}_create failed: {lib().uvs_status_string(rc).decode()} (rc={rc}); the HIP path is the only path")

    def close(self):
        if self._h:
            getattr(lib(), self._UNIT + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return getattr(lib(), self._UNIT + "_last_error")(self._h).decode()

    def _error(self, what, rc):
        return RuntimeError(f"{what}: {lib().uvs_status_string(rc).decode()} / {self.last_error()}")


class Solver(_Handle):
    """Owns one `uvs_solver` handle (device buffers + stream) on one GPU."""

    _UNIT = "uvs"

    def __init__(self, opts=None, device=0, max_batch=1024, max_points=1000, max_point_obs=16000, max_lines=1000, max_line_obs=16000):
        self.opts = opts or abi.default_options()
        self._create(C.byref(self.opts), device, max_batch, max_points, max_point_obs, max_lines, max_line_obs)
        self._keep = None
        self._windows = None

    def _check(self, rc, allow=(abi.UVS_OK,)):
        if rc not in allow:
            raise RuntimeError(f"uvs error {rc}: {lib().uvs_status_string(rc).decode()} / {self.last_error()}")
        return rc

    # ---- single window (host buffers in / out, PCIe inclusive) -------------
    def solve(self, w: abi.Window):
        wc, keep = w.to_c()
        st = abi.State(len(w.inv_depth), len(w.line_orth)); sc = st.alloc_c()
        rep = abi.Report()
        t0 = time.perf_counter()
        rc = lib().uvs_solve_window(self._h, C.byref(wc), C.byref(sc), C.byref(rep))
        self.last_solve_ms = (time.perf_counter() - t0) * 1e3      # the C-ABI call alone: pack + H2D + kernel + D2H (what a C++ caller pays)
        self._check(rc, allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
        return st.from_c(sc), rep

    # ---- batch of independent windows, device resident --------------------
    def upload(self, windows):
        cs = [w.to_c() for w in windows]
        arr = (C.POINTER(abi.WindowC) * len(cs))(*[C.pointer(c[0]) for c in cs])
        t0 = time.perf_counter()
        self._check(lib().uvs_batch_upload(self._h, len(cs), arr))
        self.last_upload_ms = (time.perf_counter() - t0) * 1e3      # the C-ABI call alone: host packing + H2D (the ctypes conversion above is python overhead)
        self._windows = list(windows)

    def solve_resident(self):
        """Runs the solve kernel on the uploaded batch; returns the HIP-event time of the launch in ms."""
        ms = C.c_float(0.0)
        self._check(lib().uvs_batch_solve(self._h, C.byref(ms)))
        return float(ms.value)

    def download(self, n=None):
        ws = self._windows
        n = n or len(ws)
        states = [abi.State(len(w.inv_depth), len(w.line_orth)) for w in ws[:n]]
        sarr = (abi.StateC * n)()
        for i, st in enumerate(states):
            sarr[i].inv_depth = abi._dp(st.inv_depth); sarr[i].line_orth = abi._dp(st.line_orth)
        reps = (abi.Report * n)()
        t0 = time.perf_counter()
        rc = lib().uvs_batch_download(self._h, n, sarr, reps)
        self.last_download_ms = (time.perf_counter() - t0) * 1e3      # the C-ABI call alone
        self._check(rc, allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
        for i, st in enumerate(states):
            st.from_c(sarr[i])
        return states, list(reps)

    def stream(self, windows, per_batch, want_states=True):
        """len(windows) / per_batch batches end to end (uvs_batch_stream): host packing, upload, solve and download of consecutive batches
        overlap.  Returns (states, reports, wall_ms of the C-ABI call)."""
        n = len(windows)
        assert n % per_batch == 0
        cs = [w.to_c() for w in windows]
        arr = (C.POINTER(abi.WindowC) * n)(*[C.pointer(c[0]) for c in cs])
        states = [abi.State(len(w.inv_depth), len(w.line_orth)) for w in windows] if want_states else []
        sarr = (abi.StateC * n)() if want_states else None
        for i, st in enumerate(states):
            sarr[i].inv_depth = abi._dp(st.inv_depth); sarr[i].line_orth = abi._dp(st.line_orth)
        reps = (abi.Report * n)()
        ms = C.c_double(0.0)
        self._check(lib().uvs_batch_stream(self._h, n // per_batch, per_batch, arr, sarr, reps, C.byref(ms)), allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
        for i, st in enumerate(states):
            st.from_c(sarr[i])
        return states, list(reps), float(ms.value)

    # ---- one large window over the whole GPU / several GPUs (BASELINE configs[3]) ----
    def large_solve(self, w: abi.Window, dist=None, device=None):
        """Landmark-sharded solve of ONE window.  With `dist` (an initialised torch.distributed module) `w` must hold only this
        rank's landmarks (synth.shard_landmarks); the pose-block partials and 5 scalars are all-reduced over RCCL in place."""
        wc, keep = w.to_c()
        st = abi.State(len(w.inv_depth), len(w.line_orth)); sc = st.alloc_c()
        rep = abi.Report()
        L = lib()
        if dist is None:
            self._check(L.uvs_large_set_nranks(self._h, 1))
            self._check(L.uvs_large_solve(self._h, C.byref(wc), C.byref(sc), C.byref(rep)), allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
            return st.from_c(sc), rep
        import torch
        gpu_aware = dist.get_backend() == "nccl"          # RCCL reduces the solver's device buffers in place; otherwise stage through the host
        self._check(L.uvs_large_set_nranks(self._h, dist.get_world_size()))
        rc = L.uvs_large_begin(self._h, C.byref(wc))
        # a rank whose shard holds no relocalization block is accepted by uvs_large_begin while another rank's is refused: every rank learns the worst
        # code, so that all of them raise together instead of waiting in a collective for a peer that has left (on the backend's device: RCCL has no CPU tensors)
        worst = torch.tensor([rc], dtype=torch.int64, device=device if gpu_aware else "cpu")
        dist.all_reduce(worst, op=dist.ReduceOp.MAX)
        self._check(rc)
        if int(worst.item()) != abi.UVS_OK:
            raise RuntimeError(f"uvs error {int(worst.item())}: {lib().uvs_status_string(int(worst.item())).decode()} / refused on another rank of the sharded solve")
        x2 = torch.tensor([L.uvs_large_local_x2(self._h)], dtype=torch.float64, device=device if gpu_aware else "cpu")
        dist.all_reduce(x2)
        L.uvs_large_set_landmark_x2(self._h, float(x2.item()))
        n = C.c_int(0)
        p_red = L.uvs_large_reduced(self._h, C.byref(n)); n_red = n.value
        p_sc = L.uvs_large_scalars(self._h, C.byref(n)); n_sc = n.value
        if gpu_aware:
            red = _device_tensor(p_red, n_red, device); scal = _device_tensor(p_sc, n_sc, device)

        def exchange(which):
            """SUM all-reduce of vector `which`; entry LG_ACC + 1 (= n - 7) of the reduced vector is a MAX."""
            if gpu_aware:
                t = red if which == 0 else scal
                mx = t[-7:-6].clone() if which == 0 else None
                dist.all_reduce(t)
                if which == 0:
                    dist.all_reduce(mx, op=dist.ReduceOp.MAX); t[-7:-6] = mx
                torch.cuda.synchronize()
            else:
                buf = np.zeros(n_red if which == 0 else n_sc)
                self._check(L.uvs_large_exchange_host(self._h, which, abi._dp(buf), 0))
                t = torch.from_numpy(buf)
                mx = t[-7:-6].clone() if which == 0 else None
                dist.all_reduce(t)
                if which == 0:
                    dist.all_reduce(mx, op=dist.ReduceOp.MAX); t[-7:-6] = mx
                self._check(L.uvs_large_exchange_host(self._h, which, abi._dp(buf), 1))

        while not L.uvs_large_done(self._h):
            if L.uvs_large_need_linearize(self._h):
                self._check(L.uvs_large_linearize(self._h))
                exchange(0)                                # the pose-block partials (46.7 KB)
            self._check(L.uvs_large_step(self._h))
            exchange(1)
            self._check(L.uvs_large_decide(self._h))
        self._check(L.uvs_large_finish(self._h, C.byref(sc), C.byref(rep)), allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
        return st.from_c(sc), rep

    def large_comm_init(self, dist=None):
        """The handle's own RCCL communicator for large_solve_fused(): rank 0 draws the id, torch.distributed (any backend) carries its
        128 bytes to the other ranks, every rank joins.  Without `dist` (or with one rank) nothing is exchanged and no RCCL is needed."""
        L = lib()
        if dist == "self":          # one-rank communicator through RCCL (tests: the dlopen'ed API, in-place all-reduce on the handle's stream)
            buf = C.create_string_buffer(128)
            self._check(L.uvs_large_comm_unique_id(buf)); self._check(L.uvs_large_comm_init(self._h, 1, 0, buf.raw)); return
        if dist is None or dist.get_world_size() == 1:
            self._check(L.uvs_large_comm_init(self._h, 1, 0, None)); return
        rank, world = dist.get_rank(), dist.get_world_size()
        buf = C.create_string_buffer(128)
        if rank == 0:
            self._check(L.uvs_large_comm_unique_id(buf))
        box = [buf.raw]
        dist.broadcast_object_list(box, src=0)
        self._check(L.uvs_large_comm_init(self._h, world, rank, box[0]))

    def large_solve_fused(self, w: abi.Window):
        """One landmark shard of ONE large window through the fused loop (include/uvs_solver.h: uvs_large_solve_fused): the whole LM loop
        is enqueued on the handle's stream, the pose-block partials and the step scalars are all-reduced in place by the handle's RCCL
        communicator (large_comm_init), accept / reject runs on the device.  Returns (state, report, loop_ms)."""
        wc, keep = w.to_c()
        st = abi.State(len(w.inv_depth), len(w.line_orth)); sc = st.alloc_c()
        rep = abi.Report(); ms = C.c_float(0.0)
        t0 = time.perf_counter()
        rc = lib().uvs_large_solve_fused(self._h, C.byref(wc), C.byref(sc), C.byref(rep), C.byref(ms))
        self.last_solve_ms = (time.perf_counter() - t0) * 1e3      # the C-ABI call alone: pack + H2D + LM loop + D2H
        self._check(rc, allow=(abi.UVS_OK, abi.UVS_ERR_NUMERIC))
        return st.from_c(sc), rep, float(ms.value)

    # ---- diagnostics -------------------------------------------------------
    def evaluate(self, w: abi.Window, robust=True):
        wc, keep = w.to_c()
        ev = abi.Eval(w); ec = ev.alloc_c()
        self._check(lib().uvs_evaluate(self._h, C.byref(wc), int(robust), C.byref(ec)))
        ev.cost = ec.cost
        return ev

    def marginalize(self, w: abi.Window, flag=0, resident=False):
        """resident=True: the factors of `w` are those of the last single-window upload / solve of this handle; only its state is sent."""
        wc, keep = w.to_c()
        p = abi.Prior()
        fn = lib().uvs_marginalize_resident if resident else lib().uvs_marginalize
        self._check(fn(self._h, C.byref(wc), flag, C.byref(p)))
        return p

    def marginalize_batch(self, windows, flags, check=True):
        """uvs_marginalize_batch: the marginalization of independent windows with the cubic work of all of them in two launches; returns (priors, per-window status codes).
        check=False: a failing window does not raise -- its status code says so, the other windows' priors are valid."""
        n = len(windows)
        keeps = [w.to_c() for w in windows]
        arr = (C.POINTER(abi.WindowC) * n)(*[C.pointer(k[0]) for k in keeps])
        fl = (C.c_int * n)(*[int(f) for f in flags])
        pri = (abi.Prior * n)()
        st = (C.c_int * n)()
        L = lib()
        L.uvs_marginalize_batch.restype = C.c_int
        rc = L.uvs_marginalize_batch(self._h, n, arr, fl, pri, st)
        if check: self._check(rc)
        return [pri[i] for i in range(n)], list(st)

    def marginalize_begin(self, w: abi.Window, flag=0):
        """uvs_marginalize_resident_begin: the marginalization of the resident window on a worker thread of the handle; marginalize_wait() delivers the prior.
        The C structures of `w` are kept alive on this object until then (the ABI's contract for the caller's arrays)."""
        wc, keep = w.to_c()
        self._marg_keep = (wc, keep, w)
        self._check(lib().uvs_marginalize_resident_begin(self._h, C.byref(wc), flag))

    def marginalize_wait(self):
        p = abi.Prior()
        rc = lib().uvs_marginalize_wait(self._h, C.byref(p))
        self._marg_keep = None
        self._check(rc)
        return p

    def debug_step(self, w: abi.Window, radii, form=0):
        """uvs_debug_step: the damped step of the first linearization of `w` at radii[0], then at each later radius the way `form` handles a
        rejected step.  -> (step [n_radii, n_step] in the layout of include/uvs_solver.h, scal [n_radii, UVS_DEBUG_SCAL_LEN])."""
        wc, keep = w.to_c()
        o = self.opts
        n_step = 165 + 6 * bool(o.estimate_extrinsic) + bool(o.estimate_td) + 6 * (len(w.relo_lm) > 0) + len(w.inv_depth) + 4 * len(w.line_orth)
        r = np.ascontiguousarray(radii, dtype=np.float64)
        step = np.zeros((len(r), n_step)); scal = np.zeros((len(r), 40))
        self._check(lib().uvs_debug_step(self._h, C.byref(wc), int(form), len(r), abi._dp(r), n_step, abi._dp(step), abi._dp(scal)))
        return step, scal

    @staticmethod
    def debug_step_sharded(solvers, shards, radii):
        """Diagnostic: the step of uvs_debug_step form 1 for a window sharded over `solvers` (one handle per shard of synth.shard_landmarks, all in this
        process), through the step-wise calls with the two exchange vectors summed on the host as large_solve(dist=...) sums them (entry n - 7 of the
        reduced vector is a MAX).  -> per shard (step [n_radii, n_step of the shard], scal [n_radii, UVS_DEBUG_SCAL_LEN])."""
        L = lib()
        G = len(solvers)
        r = np.ascontiguousarray(radii, dtype=np.float64)
        keep = [w.to_c() for w in shards]
        out = []
        for s, w in zip(solvers, shards):
            o = s.opts
            n_step = 165 + 6 * bool(o.estimate_extrinsic) + bool(o.estimate_td) + 6 * (len(w.relo_lm) > 0) + len(w.inv_depth) + 4 * len(w.line_orth)
            out.append((np.zeros((len(r), n_step)), np.zeros((len(r), 40))))
        rcs = []
        for s, (wc, _) in zip(solvers, keep):
            s._check(L.uvs_large_set_nranks(s._h, G)); s._check(L.uvs_large_set_debug_step(s._h, 1))
            rcs.append(L.uvs_large_begin(s._h, C.byref(wc)))
        try:
            for s, rc in zip(solvers, rcs): s._check(rc)      # (a refusal on one rank is every rank's: nothing has been exchanged yet)

            def exchange(which, n):
                bufs = [np.zeros(n) for _ in solvers]
                for s, b in zip(solvers, bufs): s._check(L.uvs_large_exchange_host(s._h, which, abi._dp(b), 0))
                tot = bufs[0].copy()
                for b in bufs[1:]: tot = tot + b
                if which == 0: tot[n - 7] = max(b[n - 7] for b in bufs)
                for s in solvers: s._check(L.uvs_large_exchange_host(s._h, which, abi._dp(tot), 1))

            n = C.c_int(0)
            L.uvs_large_reduced(solvers[0]._h, C.byref(n)); n_red = n.value
            L.uvs_large_scalars(solvers[0]._h, C.byref(n)); n_sc = n.value
            for k in range(len(r)):
                for s in solvers:
                    assert L.uvs_large_need_linearize(s._h)
                    s._check(L.uvs_large_linearize(s._h))
                exchange(0, n_red)
                for s in solvers: s._check(L.uvs_large_step(s._h))
                exchange(1, n_sc)
                for s, (step, scal) in zip(solvers, out):
                    s._check(L.uvs_large_debug_step(s._h, float(r[k + 1]) if k + 1 < len(r) else 0.0, step.shape[1], abi._dp(step[k]), abi._dp(scal[k])))
        finally:
            for s in solvers:
                L.uvs_large_set_debug_step(s._h, 0); L.uvs_large_set_nranks(s._h, 1)
        return out

    def debug_first_iteration(self, w: abi.Window):
        wc, keep = w.to_c()
        S = np.zeros((176, 176)); g = np.zeros(176); hd = np.zeros(176); dd = np.zeros(176); step = np.zeros(176); scal = np.zeros(40)
        self._check(lib().uvs_debug_first_iteration(self._h, C.byref(wc), *[abi._dp(a) for a in (S, g, hd, dd, step, scal)]))
        return dict(S=S, g=g, hd=hd, dd=dd, step=step, cost=scal[0], gmax=scal[1], chol_ok=scal[2], mcc=scal[3], step2=scal[4],
                    line_ahead=int(scal[5]), linearizations=int(scal[6]),      # over the whole solve: line chunks whose pass A ran under the previous gather walk, full linearizations
                    cycles=dict(zip(['setup', 'obs', 'lmprep', 'gather', 'assemble', 'chol', 'trsv', 'backsub', 'cost', 'misc', 'chol_diag', 'chol_panel', 'chol_trail', 'asm_imu', 'asm_zero', 'asm_add'], scal[8:24])), sub_timers=dict(cost_phase=dict(zip(['stage_dx', 'prior_residual', 'observations', 'imu'], scal[24:28])), chol_busy_per_wave=scal[28:32].copy()))


class PoseGraphSolver(_Handle):
    """Owns one `uvs_pose_graph` handle: the 4-DoF pose-graph optimizer of loop closure (PoseGraph::optimize4DoF) on one GPU.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_pg"

    def __init__(self, device=0, max_keyframes=16384, max_loops=256):
        self._create(device, max_keyframes, max_loops)

    def optimize_raw(self, t, q, sequence, constant, loops):
        """-> (return code, yaw_t [n, 4], report) without raising: for the tests of the argument checks."""
        p, keep = abi.pg_problem(t, q, sequence, constant, loops)
        out = np.zeros((max(p.n, 1), 4))
        rep = abi.PgReport()
        t0 = time.perf_counter()
        rc = lib().uvs_pg_optimize(self._h, C.byref(p), abi._dp(out), C.byref(rep))
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: upload, every LM iteration, download
        return rc, out[:p.n], rep

    def optimize(self, t, q, sequence, constant, loops):
        """t [n,3], q [n,4] (x,y,z,w) initial poses, sequence [n], constant [n], loops = [(cur, old, rel_t[3], rel_yaw deg)] in local indices.
        -> (yaw_t [n, 4] = (yaw deg, tx, ty, tz), abi.PgReport)."""
        rc, out, rep = self.optimize_raw(t, q, sequence, constant, loops)
        if rc not in (abi.UVS_OK, abi.UVS_ERR_NUMERIC):
            raise self._error("uvs_pg_optimize", rc)
        return out, rep

    def debug_step_raw(self, t, q, sequence, constant, loops, radius):
        """-> (return code, delta [4 n_free], scal [UVS_PG_DEBUG_SCAL_LEN]) without raising."""
        p, keep = abi.pg_problem(t, q, sequence, constant, loops)
        delta = np.zeros(max(4 * int(np.count_nonzero(keep["constant"] == 0)), 1)); scal = np.zeros(abi.PG_DEBUG_SCAL_LEN)
        rc = lib().uvs_pg_debug_step(self._h, C.byref(p), float(radius), abi._dp(delta), abi._dp(scal))
        return rc, delta[:4 * int(scal[3])], scal

    def debug_step(self, t, q, sequence, constant, loops, radius):
        """Diagnostic: one damped solve of the first LM iteration at `radius` through the product's kernels (uvs_pg_debug_step).
        -> (delta [4 n_free] = the unscaled step in free-keyframe order, dict(factor_fail, capacitance_fail, n_loop_columns, n_free))."""
        rc, delta, scal = self.debug_step_raw(t, q, sequence, constant, loops, radius)
        if rc != abi.UVS_OK:
            raise self._error("uvs_pg_debug_step", rc)
        return delta, dict(factor_fail=int(scal[0]), capacitance_fail=int(scal[1]), n_loop_columns=int(scal[2]), n_free=int(scal[3]))


class LoopVerifier(_Handle):
    """Owns one `uvs_loop_verifier` handle: loop verification of loop closure (KeyFrame::findConnection: BRIEF matching + PnP-RANSAC) on
    one GPU, a batch of candidate pairs per call.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_lc"

    def __init__(self, device=0, max_pairs=64, max_query=1024, max_old=4096):
        self._create(device, max_pairs, max_query, max_old)

    def verify_raw(self, pairs, tic, qic, n_pairs=None, null=()):
        """-> (return code, [result dict], [match_old per pair], [inlier per pair]) without raising: for the tests of the argument checks.
        n_pairs overrides the count passed; `null` names arguments passed as NULL ("pairs", "tic", "qic", "match_old", "inlier", "results")."""
        arr, keep = abi.lc_pairs(pairs)
        nq = [int(arr[b].n_query) for b in range(len(pairs))]
        tq = max(sum(nq), 1)
        tic = np.ascontiguousarray(tic, dtype=np.float64); qic = np.ascontiguousarray(qic, dtype=np.float64)
        mo = np.zeros(tq, np.int32); inl = np.zeros(tq, np.uint8)
        res = (abi.LcResult * max(len(pairs), 1))()
        args = dict(pairs=C.cast(arr, C.POINTER(abi.LcPair)), tic=abi._dp(tic), qic=abi._dp(qic), match_old=mo.ctypes.data_as(C.POINTER(C.c_int32)),
                    inlier=inl.ctypes.data_as(C.POINTER(C.c_uint8)), results=C.cast(res, C.POINTER(abi.LcResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_lc_verify(self._h, len(pairs) if n_pairs is None else int(n_pairs), args["pairs"], args["tic"], args["qic"],
                                 args["match_old"], args["inlier"], args["results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernel, download
        off = np.r_[0, np.cumsum(nq)].astype(int)
        return (rc, [res[b].as_dict() for b in range(len(pairs))], [mo[off[b]:off[b + 1]].copy() for b in range(len(pairs))],
                [inl[off[b]:off[b + 1]].copy() for b in range(len(pairs))])

    def verify(self, pairs, tic, qic):
        """pairs: list of dicts (p3d [nq,3] in the current keyframe's VIO frame, qdesc [nq,4] uint64, vio_t [3], vio_q [4] (x,y,z,w) of its
        origin_vio pose, uv [no,2] normalized keypoints and odesc [no,4] uint64 of the old keyframe, seed); tic [3], qic [4] (x,y,z,w) the
        extrinsic.  -> (results: list of dicts with the uvs_lc_result fields, match_old: list of int32 [nq], inlier: list of uint8 [nq])."""
        rc, res, mo, inl = self.verify_raw(pairs, tic, qic)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lc_verify", rc)
        return res, mo, inl

    def debug_pair(self, pair, tic, qic):
        """Diagnostic (tests only): one pair through the trace instantiation of the kernel.  -> (result dict, match_old [nq], inlier [nq],
        trace: abi.lc_trace of the raw doubles), the first three bit for bit what verify gives."""
        arr, keep = abi.lc_pairs([pair])
        nq = int(arr[0].n_query)
        tic = np.ascontiguousarray(tic, dtype=np.float64); qic = np.ascontiguousarray(qic, dtype=np.float64)
        mo = np.zeros(max(nq, 1), np.int32); inl = np.zeros(max(nq, 1), np.uint8)
        res = (abi.LcResult * 1)()
        raw = np.zeros(abi.LC_TRACE_LEN, np.float64)
        rc = lib().uvs_lc_debug_pair(self._h, C.cast(arr, C.POINTER(abi.LcPair)), abi._dp(tic), abi._dp(qic), mo.ctypes.data_as(C.POINTER(C.c_int32)),
                                     inl.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(res, C.POINTER(abi.LcResult)), abi._dp(raw))
        if rc != abi.UVS_OK:
            raise self._error("uvs_lc_debug_pair", rc)
        return res[0].as_dict(), mo[:nq].copy(), inl[:nq].copy(), abi.lc_trace(raw)


class VanishingPointEstimator(_Handle):
    """Owns one `uvs_vp_estimator` handle: the vanishing points of the line front end (getVPHypVia2Lines, getSphereGrids, getBestVpsHyp,
    lines2Vps of the reference's line_feature_tracker.cpp) on one GPU, a batch of frames per call.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_vp"
    ONE_DEGREE = 1.0 / 180.0 * 3.1415926535897932384626433832795       # thAngle of the reference

    def __init__(self, device=0, max_frames=64, max_lines=1024):
        self._create(device, max_frames, max_lines)

    def estimate_raw(self, frames, camera, th_angle=None, n_frames=None, null=()):
        """-> (return code, [result dict], [tag per frame], [line_vp per frame]) without raising: for the tests of the argument checks.
        n_frames overrides the count passed; `null` names arguments passed as NULL ("frames", "camera", "tag", "line_vp", "results")."""
        arr, keep = abi.vp_frames(frames)
        nl = [int(arr[b].n_lines) for b in range(len(frames))]
        tl = max(sum(nl), 1)
        cam = abi.vp_camera(camera)
        tag = np.zeros(tl, np.int32); lvp = np.zeros((tl, 3))
        res = (abi.VpResult * max(len(frames), 1))()
        args = dict(frames=C.cast(arr, C.POINTER(abi.VpFrame)), camera=C.byref(cam), tag=tag.ctypes.data_as(C.POINTER(C.c_int32)), line_vp=abi._dp(lvp),
                    results=C.cast(res, C.POINTER(abi.VpResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_vp_estimate(self._h, len(frames) if n_frames is None else int(n_frames), args["frames"], args["camera"],
                                   self.ONE_DEGREE if th_angle is None else float(th_angle), args["tag"], args["line_vp"], args["results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernels, download
        self.last_device_ms = float(lib().uvs_vp_last_device_ms(self._h))      # HIP events around upload, kernels, download
        off = np.r_[0, np.cumsum(nl)].astype(int)
        return (rc, [res[b].as_dict() for b in range(len(frames))], [tag[off[b]:off[b + 1]].copy() for b in range(len(frames))],
                [lvp[off[b]:off[b + 1]].copy() for b in range(len(frames))])

    def estimate(self, frames, camera, th_angle=None):
        """frames: list of dicts (segs [n, 4]: x1, y1, x2, y2 in pixels of the undistorted image; seed); camera = (fx, fy, cx, cy); th_angle in
        radians (default: the reference's 1 degree).  -> (results: list of dicts with the uvs_vp_result fields, tag: list of int32 [n] with
        0..2 or 3 for "none", line_vp: list of [n, 3] with vps[tag] / vps[tag].z or zero)."""
        rc, res, tag, lvp = self.estimate_raw(frames, camera, th_angle)
        if rc != abi.UVS_OK:
            raise self._error("uvs_vp_estimate", rc)
        return res, tag, lvp

    def debug_frame(self, frame, camera, th_angle=None):
        """ONE frame with the intermediate results (tests only) -> dict: the uvs_vp_result fields, hyp [37800, 3, 3], cells [37800, 3],
        scores [37800], raw / smooth [90, 360], pair_cell [n (n - 1) / 2]."""
        arr, keep = abi.vp_frames([frame])
        n = int(arr[0].n_lines)
        cam = abi.vp_camera(camera)
        hyp = np.zeros((abi.VP_N_HYPOTHESES, 3, 3)); cells = np.zeros((abi.VP_N_HYPOTHESES, 3), np.int32); scores = np.zeros(abi.VP_N_HYPOTHESES)
        raw = np.zeros((abi.VP_GRID_LA, abi.VP_GRID_LO)); smooth = np.zeros((abi.VP_GRID_LA, abi.VP_GRID_LO))
        pc = np.zeros(max(n * (n - 1) // 2, 1), np.int32)
        res = abi.VpResult()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = lib().uvs_vp_debug_frame(self._h, C.cast(arr, C.POINTER(abi.VpFrame)), C.byref(cam), self.ONE_DEGREE if th_angle is None else float(th_angle),
                                      abi._dp(hyp), ip(cells), abi._dp(scores), abi._dp(raw), abi._dp(smooth), ip(pc), C.byref(res))
        if rc != abi.UVS_OK:
            raise self._error("uvs_vp_debug_frame", rc)
        out = res.as_dict()
        out.update(hyp=hyp, cells=cells, scores=scores, raw=raw, smooth=smooth, pair_cell=pc[:n * (n - 1) // 2])
        return out


class KeyframeExtractor(_Handle):
    """Owns one `uvs_kf_extractor` handle: the features of a pose-graph keyframe (computeWindowBRIEFPoint / computeBRIEFPoint of the reference's
    keyframe.cpp: FAST corners, BRIEF descriptors, normalized keypoints) on one GPU, a batch of images per call.

    `pattern` is the BRIEF pattern as int32 [4, 256] (x1, y1, x2, y2), e.g. abi.load_brief_pattern("brief_pattern.yml").
    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_kf"

    def __init__(self, pattern, device=0, max_frames=16, max_width=752, max_height=480, max_keypoints=4096, max_window=1024):
        pat = np.ascontiguousarray(pattern, dtype=np.int32)
        if pat.shape != (4, abi.KF_PATTERN_BITS):
            raise ValueError(f"pattern must be [4, {abi.KF_PATTERN_BITS}] (x1, y1, x2, y2)")
        self.max_keypoints = int(max_keypoints)
        self._create(device, max_frames, max_width, max_height, max_keypoints, max_window, *[pat[k].ctypes.data_as(abi.c_i32_p) for k in range(4)])

    def _outputs(self, n_frames, n_window):
        K = max(n_frames, 1) * self.max_keypoints
        return dict(xy=np.zeros((K, 2), np.int32), score=np.zeros(K, np.uint8), norm=np.zeros((K, 2)), desc=np.zeros((K, 4), np.uint64),
                    wdesc=np.zeros((max(n_window, 1), 4), np.uint64))

    def _split(self, o, res, nw):
        """The strided keypoint arrays and the packed window descriptors as one dict per frame."""
        off = np.r_[0, np.cumsum(nw)].astype(int)
        out = []
        for b, r in enumerate(res):
            d = r.as_dict()
            s = slice(b * self.max_keypoints, b * self.max_keypoints + d["n_returned"])
            d.update(xy=o["xy"][s].copy(), score=o["score"][s].copy(), norm=o["norm"][s].copy(), desc=o["desc"][s].copy(),
                     window_desc=o["wdesc"][off[b]:off[b + 1]].copy())
            out.append(d)
        return out

    def extract_raw(self, frames, camera, n_frames=None, null=()):
        """-> (return code, [dict per frame]) without raising: for the tests of the argument checks.  n_frames overrides the count passed;
        `null` names arguments passed as NULL ("frames", "camera", "xy", "score", "norm", "desc", "wdesc", "results")."""
        arr, keep = abi.kf_frames(frames)
        nw = [int(arr[b].n_window) for b in range(len(frames))]
        cam = _camera_arg(camera)
        o = self._outputs(len(frames), sum(nw))
        res = (abi.KfResult * max(len(frames), 1))()
        args = dict(frames=C.cast(arr, C.POINTER(abi.KfFrame)), camera=cam, xy=o["xy"].ctypes.data_as(abi.c_i32_p),
                    score=o["score"].ctypes.data_as(abi.c_u8_p), norm=abi._dp(o["norm"]), desc=o["desc"].ctypes.data_as(abi.c_u64_p),
                    wdesc=o["wdesc"].ctypes.data_as(abi.c_u64_p), results=C.cast(res, C.POINTER(abi.KfResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_kf_extract(self._h, len(frames) if n_frames is None else int(n_frames), args["frames"], args["camera"], args["xy"],
                                  args["score"], args["norm"], args["desc"], args["wdesc"], args["results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: repacking, upload, kernels, download
        self.last_device_ms = float(lib().uvs_kf_last_device_ms(self._h))      # HIP events around upload, kernels, download
        return rc, (self._split(o, [res[b] for b in range(len(frames))], nw) if rc == abi.UVS_OK else [])

    def extract(self, frames, camera):
        """frames: list of dicts (image [H, W] uint8; window_uv [n, 2] float32 pixels, optional); camera = (fx, fy, cx, cy[, k1, k2, p1, p2]).
        -> one dict per frame: status, n_keypoints, n_returned, n_corners_before_nms, xy [n, 2] int32 in row-major order, score [n] uint8,
        norm [n, 2] float64, desc [n, 4] uint64, window_desc [n_window, 4] uint64.  norm / desc are what uvs_lc_verify takes as uv / odesc
        of an old keyframe, window_desc as qdesc of the current one."""
        rc, out = self.extract_raw(frames, camera)
        if rc != abi.UVS_OK:
            raise self._error("uvs_kf_extract", rc)
        return out

    def set_camera_model_raw(self, model):
        return lib().uvs_kf_set_camera_model(self._h, _model_arg(model))

    def set_camera_model(self, model):
        """model: an abi.CameraModel, a dict of abi.load_camera_calibration or None.  While one is set, extract() and debug_frame() lift the
        keypoints through it and their `camera` may be None."""
        rc = self.set_camera_model_raw(model)
        if rc != abi.UVS_OK:
            raise self._error("uvs_kf_set_camera_model", rc)

    def debug_frame(self, frame, camera):
        """ONE frame with the whole blurred image and the whole score map (tests only) -> the frame's dict of extract() plus blur, score_map."""
        arr, keep = abi.kf_frames([frame])
        H, W, nw = int(arr[0].height), int(arr[0].width), int(arr[0].n_window)
        cam = _camera_arg(camera)
        o = self._outputs(1, nw)
        blur = np.zeros((H, W), np.uint8); smap = np.zeros((H, W), np.uint8)
        res = abi.KfResult()
        rc = lib().uvs_kf_debug_frame(self._h, C.cast(arr, C.POINTER(abi.KfFrame)), cam, blur.ctypes.data_as(abi.c_u8_p),
                                      smap.ctypes.data_as(abi.c_u8_p), o["xy"].ctypes.data_as(abi.c_i32_p), o["score"].ctypes.data_as(abi.c_u8_p),
                                      abi._dp(o["norm"]), o["desc"].ctypes.data_as(abi.c_u64_p), o["wdesc"].ctypes.data_as(abi.c_u64_p), C.byref(res))
        if rc != abi.UVS_OK:
            raise self._error("uvs_kf_debug_frame", rc)
        out = self._split(o, [res], [nw])[0]
        out.update(blur=blur, score_map=smap)
        return out


class FeatureTracker(_Handle):
    """Owns one `uvs_ft_tracker` handle: the tracking step of the reference's point front end (FeatureTracker::readImage: pyramidal Lucas-Kanade
    with a 21 x 21 window, inBorder, liftProjective of the tracked points) on one GPU.  Each of the `max_streams` slots keeps the pyramid of its
    last image on the device; a call takes one new image per slot and the points to follow into it.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_ft"

    def __init__(self, device=0, max_streams=1, max_width=752, max_height=480, levels=4, max_points=1024):
        self.levels = int(levels)
        self.max_candidates = abi.FT_DEFAULT_CANDIDATES
        self._pyramid_capacity = 2 * int(max_width) * int(max_height)      # level 0 plus the levels above it, which add less than a third
        self._create(device, max_streams, max_width, max_height, levels, max_points)

    def track_raw(self, items, camera, n_items=None, null=()):
        """-> (return code, [dict per item]) without raising: for the tests of the argument checks.  n_items overrides the count passed; `null`
        names arguments passed as NULL ("items", "camera", "next_xy", "status", "iterations", "next_norm", "results")."""
        arr, keep = abi.ft_items(items)
        npt = [int(arr[b].n_points) for b in range(len(items))]
        cam = _camera_arg(camera)
        N = max(sum(npt), 1)
        o = dict(next_xy=np.zeros((N, 2)), status=np.zeros(N, np.int32), iterations=np.zeros(N, np.int32), next_norm=np.zeros((N, 2)),
                 results=np.zeros(max(len(items), 1), np.int32))
        args = dict(items=C.cast(arr, C.POINTER(abi.FtItem)), camera=cam, next_xy=abi._dp(o["next_xy"]),
                    status=o["status"].ctypes.data_as(abi.c_i32_p), iterations=o["iterations"].ctypes.data_as(abi.c_i32_p),
                    next_norm=abi._dp(o["next_norm"]), results=o["results"].ctypes.data_as(abi.c_i32_p))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_ft_track(self._h, len(items) if n_items is None else int(n_items), args["items"], args["camera"], args["next_xy"],
                                args["status"], args["iterations"], args["next_norm"], args["results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: repacking, upload, kernels, download
        self.last_device_ms = float(lib().uvs_ft_last_device_ms(self._h))      # HIP events around upload, kernels, download
        if rc != abi.UVS_OK:
            return rc, []
        off = np.r_[0, np.cumsum(npt)].astype(int)
        out = []
        for b in range(len(items)):
            s = slice(off[b], off[b + 1])
            out.append(dict(next_xy=o["next_xy"][s].copy(), status=o["status"][s].copy(), iterations=o["iterations"][s].copy(),
                            next_norm=o["next_norm"][s].copy(), n_tracked=int(o["results"][b])))
        return rc, out

    def track(self, items, camera):
        """items: list of dicts (stream; image [H, W] uint8, the slot's new image; points [n, 2] float64 pixels in the slot's previous image,
        optional); camera = (fx, fy, cx, cy[, k1, k2, p1, p2]).  -> one dict per item: next_xy [n, 2] float64, status [n] int32 (index of
        abi.FT_STATUS), iterations [n] int32, next_norm [n, 2] float64 (zero where the point is not TRACKED), n_tracked."""
        rc, out = self.track_raw(items, camera)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_track", rc)
        return out

    def reset(self, stream):
        rc = lib().uvs_ft_reset(self._h, int(stream))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_reset", rc)

    # ---- camera models: the handle's model (uvs_ft_set_camera_model) and loose points through a model (uvs_ft_lift, uvs_ft_project)
    def set_camera_model_raw(self, model):
        return lib().uvs_ft_set_camera_model(self._h, _model_arg(model))

    def set_camera_model(self, model):
        """model: an abi.CameraModel, a dict of abi.load_camera_calibration or None.  While one is set, track(), detect() and their debug forms
        lift through it and their `camera` may be None; reset() keeps it."""
        rc = self.set_camera_model_raw(model)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_set_camera_model", rc)

    def lift_raw(self, model, xy, n=None, null=()):
        """-> (return code, ray [n, 3], norm [n, 2]) without raising; `null` names arguments passed as NULL ("model", "xy", "ray", "norm")."""
        p = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        N = max(len(p), 1)
        ray = np.zeros((N, 3)); norm = np.zeros((N, 2))
        args = dict(model=_model_arg(model), xy=abi._dp(p), ray=abi._dp(ray), norm=abi._dp(norm))
        for k in null:
            args[k] = None
        rc = lib().uvs_ft_lift(self._h, args["model"], len(p) if n is None else int(n), args["xy"], args["ray"], args["norm"])
        return rc, ray[:len(p)], norm[:len(p)]

    def lift(self, model, xy):
        """xy [n, 2] float64 pixels -> (ray [n, 3], norm [n, 2]) through the model, on the device."""
        rc, ray, norm = self.lift_raw(model, xy)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_lift", rc)
        return ray, norm

    def project_raw(self, model, ray, n=None, null=()):
        """-> (return code, xy [n, 2]) without raising; `null` names arguments passed as NULL ("model", "ray", "xy")."""
        r = np.ascontiguousarray(ray, np.float64).reshape(-1, 3)
        xy = np.zeros((max(len(r), 1), 2))
        args = dict(model=_model_arg(model), ray=abi._dp(r), xy=abi._dp(xy))
        for k in null:
            args[k] = None
        rc = lib().uvs_ft_project(self._h, args["model"], len(r) if n is None else int(n), args["ray"], args["xy"])
        return rc, xy[:len(r)]

    def project(self, model, ray):
        """ray [n, 3] float64 -> xy [n, 2] pixels through the model (spaceToPlane), on the device."""
        rc, xy = self.project_raw(model, ray)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_project", rc)
        return xy

    def debug_pyramid(self, stream):
        """The stored pyramid of a slot (tests only) -> [level 0, level 1, ..] uint8 arrays."""
        sizes = np.zeros((abi.FT_MAX_LEVELS, 2), np.int32)
        cap = self._pyramid_capacity
        px = np.zeros(cap, np.uint8)
        rc = lib().uvs_ft_debug_pyramid(self._h, int(stream), sizes.ctypes.data_as(abi.c_i32_p), px.ctypes.data_as(abi.c_u8_p), cap)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_debug_pyramid", rc)
        out, o = [], 0
        for l in range(self.levels):
            w, h = int(sizes[l, 0]), int(sizes[l, 1])
            out.append(px[o:o + w * h].reshape(h, w).copy()); o += w * h
        return out

    def debug_point(self, item, camera):
        """ONE item with ONE point (tests only) -> the item's dict of track() plus trace [4, 320] float64 (include/uvs_solver.h lists its
        entries)."""
        arr, keep = abi.ft_items([item])
        cam = _camera_arg(camera)
        trace = np.zeros((abi.FT_MAX_LEVELS, abi.FT_TRACE_LEVEL)); xy = np.zeros((1, 2)); nm = np.zeros((1, 2))
        st = np.zeros(1, np.int32); it = np.zeros(1, np.int32)
        rc = lib().uvs_ft_debug_point(self._h, C.cast(arr, C.POINTER(abi.FtItem)), cam, abi._dp(trace), abi._dp(xy),
                                      st.ctypes.data_as(abi.c_i32_p), it.ctypes.data_as(abi.c_i32_p), abi._dp(nm))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_debug_point", rc)
        return dict(next_xy=xy, status=st, iterations=it, next_norm=nm, n_tracked=int(st[0] == 0), trace=trace)

    # ---- new points: Shi-Tomasi corners of the image a slot holds (uvs_ft_detect)
    def set_max_candidates(self, max_candidates):
        rc = lib().uvs_ft_set_max_candidates(self._h, int(max_candidates))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_set_max_candidates", rc)
        self.max_candidates = int(max_candidates)

    def set_mask(self, stream, mask):
        """mask [H, W] uint8 of the size of the slot's image (detection is allowed where it is non-zero), or None to clear it."""
        if mask is None:
            rc = lib().uvs_ft_set_mask(self._h, int(stream), None, 0, 0)
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            rc = lib().uvs_ft_set_mask(self._h, int(stream), m.ctypes.data_as(abi.c_u8_p), m.shape[1], m.shape[0])
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_set_mask", rc)

    @staticmethod
    def _detect_split(o, res, max_new):
        off = np.r_[0, np.cumsum(max_new)].astype(int)
        out = []
        for b, r in enumerate(res):
            s = slice(off[b], off[b] + int(r.n_new))
            out.append(dict(xy=o["xy"][s].copy(), score=o["score"][s].copy(), norm=o["norm"][s].copy(), status=int(r.status), n_new=int(r.n_new),
                            n_candidates=int(r.n_candidates), max_score=float(r.max_score), threshold=float(r.threshold)))
        return out

    def detect_raw(self, items, camera, quality_level=0.01, min_distance=30, n_items=None, null=()):
        """-> (return code, [dict per item]) without raising: for the tests of the argument checks.  n_items overrides the count passed; `null`
        names arguments passed as NULL ("items", "camera", "new_xy", "new_score", "new_norm", "results")."""
        arr, keep = abi.ft_detect_items(items)
        max_new = [max(int(arr[b].max_new), 0) for b in range(len(items))]
        cam = _camera_arg(camera)
        N = max(sum(max_new), 1)
        o = dict(xy=np.zeros((N, 2), np.int32), score=np.zeros(N), norm=np.zeros((N, 2)))
        res = (abi.FtDetectResult * max(len(items), 1))()
        args = dict(items=C.cast(arr, C.POINTER(abi.FtDetectItem)), camera=cam, new_xy=o["xy"].ctypes.data_as(abi.c_i32_p),
                    new_score=abi._dp(o["score"]), new_norm=abi._dp(o["norm"]), results=C.cast(res, C.POINTER(abi.FtDetectResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_ft_detect(self._h, len(items) if n_items is None else int(n_items), args["items"], float(quality_level), int(min_distance),
                                 args["camera"], args["new_xy"], args["new_score"], args["new_norm"], args["results"])
        self.last_detect_ms = (time.perf_counter() - t0) * 1e3      # the whole C-ABI call
        if rc != abi.UVS_OK:
            return rc, []
        return rc, self._detect_split(o, [res[b] for b in range(len(items))], max_new)

    def detect(self, items, camera, quality_level=0.01, min_distance=30):
        """items: list of dicts (stream: a slot that holds an image; occupied [n, 2] float64 pixels, optional: no new point within min_distance
        of one; max_new); camera as in track().  -> one dict per item: xy [n_new, 2] int32, score [n_new] float64, norm [n_new, 2] float64
        (liftProjective of xy), in the order the points were taken (best first), status (abi.FT_DETECT_*), n_new, n_candidates, max_score,
        threshold."""
        rc, out = self.detect_raw(items, camera, quality_level, min_distance)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_detect", rc)
        return out

    def last_detect_device_ms(self):
        """HIP events around upload, kernels and download of the last detect()."""
        return float(lib().uvs_ft_last_detect_device_ms(self._h))

    def debug_detect(self, item, camera, shape, quality_level=0.01, min_distance=30):
        """ONE item (tests only); shape = (H, W) of the slot's image -> the item's dict of detect() plus score_map [H, W] float64, allowed [H, W]
        uint8, cand_index and cand_score: the ranked candidates (min(n_candidates, max_candidates) of them)."""
        arr, keep = abi.ft_detect_items([item])
        cam = _camera_arg(camera)
        H, W = int(shape[0]), int(shape[1])
        M = max(int(arr[0].max_new), 1)
        o = dict(xy=np.zeros((M, 2), np.int32), score=np.zeros(M), norm=np.zeros((M, 2)))
        smap = np.zeros((H, W)); allowed = np.zeros((H, W), np.uint8)
        ci = np.zeros(self.max_candidates, np.int32); cs = np.zeros(self.max_candidates)
        res = abi.FtDetectResult()
        rc = lib().uvs_ft_debug_detect(self._h, C.cast(arr, C.POINTER(abi.FtDetectItem)), float(quality_level), int(min_distance), cam,
                                       abi._dp(smap), allowed.ctypes.data_as(abi.c_u8_p), ci.ctypes.data_as(abi.c_i32_p), abi._dp(cs),
                                       o["xy"].ctypes.data_as(abi.c_i32_p), abi._dp(o["score"]), abi._dp(o["norm"]), C.byref(res))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_debug_detect", rc)
        out = self._detect_split(o, [res], [M])[0]
        n = min(out["n_candidates"], self.max_candidates)
        out.update(score_map=smap, allowed=allowed, cand_index=ci[:n].copy(), cand_score=cs[:n].copy())
        return out

    # ---- outlier rejection: fundamental-matrix RANSAC over the tracks of a frame (uvs_ft_reject)
    @staticmethod
    def _reject_dict(r, keep):
        return dict(status=int(r.status), n_inliers=int(r.n_inliers), hypothesis=int(r.hypothesis), root=int(r.root), iterations=int(r.iterations),
                    F=np.array(r.F[:], np.float64), keep=keep.copy())

    def reject_raw(self, items, threshold, confidence=0.99, n_items=None, null=()):
        """-> (return code, [dict per item]) without raising: for the tests of the argument checks.  n_items overrides the count passed; `null`
        names arguments passed as NULL ("items", "keep", "results")."""
        arr, keepalive = abi.ft_reject_items(items)
        npt = [max(int(arr[b].n_points), 0) for b in range(len(items))]
        keep = np.zeros(max(sum(npt), 1), np.uint8)
        res = (abi.FtRejectResult * max(len(items), 1))()
        args = dict(items=C.cast(arr, C.POINTER(abi.FtRejectItem)), keep=keep.ctypes.data_as(abi.c_u8_p), results=C.cast(res, C.POINTER(abi.FtRejectResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_ft_reject(self._h, len(items) if n_items is None else int(n_items), args["items"], float(threshold), float(confidence),
                                 args["keep"], args["results"])
        self.last_reject_ms = (time.perf_counter() - t0) * 1e3      # the whole C-ABI call
        if rc != abi.UVS_OK:
            return rc, []
        off = np.r_[0, np.cumsum(npt)].astype(int)
        return rc, [self._reject_dict(res[b], keep[off[b]:off[b + 1]]) for b in range(len(items))]

    def reject(self, items, threshold, confidence=0.99):
        """items: list of dicts (prev [n, 2], next [n, 2] float64 NORMALIZED points of the tracks; seed); threshold in normalized units
        (F_THRESHOLD / FOCAL_LENGTH).  -> one dict per item: keep [n] uint8 (1 = keep the track), status (abi.FT_REJECT_*), n_inliers,
        hypothesis, root, iterations, F [9] float64."""
        rc, out = self.reject_raw(items, threshold, confidence)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_reject", rc)
        return out

    def last_reject_device_ms(self):
        """HIP events around upload, kernel and download of the last reject()."""
        return float(lib().uvs_ft_last_reject_device_ms(self._h))

    def debug_reject(self, item, threshold, confidence=0.99):
        """ONE item (tests only), every round evaluated -> the item's dict of reject() plus samples [1000, 7] int32, models [1000, 3, 9] float64 and
        counts [1000, 3] int32 of every hypothesis."""
        arr, keepalive = abi.ft_reject_items([item])
        n = max(int(arr[0].n_points), 0)
        keep = np.zeros(max(n, 1), np.uint8)
        smp = np.zeros((abi.FT_REJECT_HYPOTHESES, 7), np.int32); mod = np.zeros((abi.FT_REJECT_HYPOTHESES, 3, 9))
        cnt = np.zeros((abi.FT_REJECT_HYPOTHESES, 3), np.int32)
        res = abi.FtRejectResult()
        rc = lib().uvs_ft_debug_reject(self._h, C.cast(arr, C.POINTER(abi.FtRejectItem)), float(threshold), float(confidence),
                                       smp.ctypes.data_as(abi.c_i32_p), abi._dp(mod), cnt.ctypes.data_as(abi.c_i32_p), keep.ctypes.data_as(abi.c_u8_p),
                                       C.byref(res))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_debug_reject", rc)
        out = self._reject_dict(res, keep[:n])
        out.update(samples=smp, models=mod, counts=cnt)
        return out

    # ---- equalization: CLAHE of a slot's raw images (uvs_ft_set_equalize) and of loose images (uvs_ft_equalize)
    def set_equalize_raw(self, stream, clip_limit=3.0, tiles_x=8, tiles_y=8):
        return lib().uvs_ft_set_equalize(self._h, int(stream), float(clip_limit), int(tiles_x), int(tiles_y))

    def set_equalize(self, stream, clip_limit=3.0, tiles_x=8, tiles_y=None):
        """Switches the equalization of a slot on: track() then takes the slot's images raw.  tiles_x = 0 switches it off; reset() does too."""
        rc = self.set_equalize_raw(stream, clip_limit, tiles_x, tiles_x if tiles_y is None else tiles_y)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_set_equalize", rc)

    def equalize_raw(self, images, clip_limit=3.0, tiles_x=8, tiles_y=8, n_images=None, null=()):
        """-> (return code, [equalized image]) without raising: for the tests of the argument checks.  n_images overrides the count passed; `null`
        names arguments passed as NULL ("images", "out")."""
        arr, keep = abi.ft_images(images)
        out = np.zeros(max(sum(im.size for im in keep), 1), np.uint8)
        args = dict(images=C.cast(arr, C.POINTER(abi.FtImage)), out=out.ctypes.data_as(abi.c_u8_p))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_ft_equalize(self._h, len(images) if n_images is None else int(n_images), args["images"], float(clip_limit), int(tiles_x),
                                   int(tiles_y), args["out"])
        self.last_equalize_ms = (time.perf_counter() - t0) * 1e3
        if rc != abi.UVS_OK:
            return rc, []
        res, o = [], 0
        for im in keep:
            res.append(out[o:o + im.size].reshape(im.shape).copy()); o += im.size
        return rc, res

    def equalize(self, images, clip_limit=3.0, tiles_x=8, tiles_y=None):
        """images: list of [H, W] uint8 (at most max_streams) -> the equalized images.  Stateless: no slot is touched."""
        rc, out = self.equalize_raw(images, clip_limit, tiles_x, tiles_x if tiles_y is None else tiles_y)
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_equalize", rc)
        return out

    def last_equalize_device_ms(self):
        return float(lib().uvs_ft_last_equalize_device_ms(self._h))

    def debug_equalize(self, image, clip_limit=3.0, tiles_x=8, tiles_y=None):
        """ONE image (tests only) -> dict(out [H, W] uint8, bins [tiles_y, tiles_x, 256] int32, luts [tiles_y, tiles_x, 256] uint8, info int32
        (Wp, Hp, N, clip))."""
        tiles_y = tiles_x if tiles_y is None else tiles_y
        arr, keep = abi.ft_images([image])
        n = max(int(tiles_x) * int(tiles_y), 1)
        bins = np.zeros((n, 256), np.int32); luts = np.zeros((n, 256), np.uint8); out = np.zeros(keep[0].shape, np.uint8); info = np.zeros(4, np.int32)
        rc = lib().uvs_ft_debug_equalize(self._h, C.cast(arr, C.POINTER(abi.FtImage)), float(clip_limit), int(tiles_x), int(tiles_y),
                                         bins.ctypes.data_as(abi.c_i32_p), luts.ctypes.data_as(abi.c_u8_p), out.ctypes.data_as(abi.c_u8_p),
                                         info.ctypes.data_as(abi.c_i32_p))
        if rc != abi.UVS_OK:
            raise self._error("uvs_ft_debug_equalize", rc)
        return dict(out=out, bins=bins.reshape(tiles_y, tiles_x, 256), luts=luts.reshape(tiles_y, tiles_x, 256), info=info)


class LineTracker(_Handle):
    """Owns one `uvs_lt_tracker` handle: the line tracking of the line front end (lineBiDes->compute and lineMatching of the reference's
    line_feature_tracker.cpp) on one GPU.  The caller supplies a frame's segments with the image they were detected in; each slot keeps its
    previous lines' descriptors and gate points on the device, and a call describes a batch of new frames, one per slot, and says which
    previous line each new line continues.  detect() finds the segments of an image on the device (line-support regions, the project's own
    rule), detect_track() does both steps with one upload of the image.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path (gauss_tables needs none)."""

    _UNIT = "uvs_lt"

    def __init__(self, device=0, max_streams=1, max_width=752, max_height=480, max_lines=256, max_length=abi.LT_MAX_LENGTH):
        self._create(device, max_streams, max_width, max_height, max_lines, max_length)
        self.max_lines = int(max_lines)

    @staticmethod
    def gauss_tables():
        """-> (G [63], Lc [21]): the coefficient tables a handle uploads (host only)."""
        G = np.zeros(abi.LT_ROWS); Lc = np.zeros(21)
        lib().uvs_lt_gauss_tables(abi._dp(G), abi._dp(Lc))
        return G, Lc

    def track_raw(self, items, n_items=None, null=()):
        """-> (return code, [dict per item]) without raising: for the tests of the argument checks.  n_items overrides the count passed;
        `null` names arguments passed as NULL ("items", "desc", "line_status", "prev_index", "distance", "results")."""
        arr, keep = abi.lt_items(items)
        nl = [len(k) for k in keep[1::2]]
        tl = max(sum(nl), 1)
        desc = np.zeros((tl, abi.LT_DESC_BYTES), np.uint8); status = np.zeros(tl, np.int32); prev = np.full(tl, -1, np.int32); dist = np.full(tl, -1, np.int32)
        res = (abi.LtResult * max(len(items), 1))()
        args = dict(items=C.cast(arr, C.POINTER(abi.LtItem)), desc=desc.ctypes.data_as(abi.c_u8_p), line_status=abi._ip(status),
                    prev_index=abi._ip(prev), distance=abi._ip(dist), results=C.cast(res, C.POINTER(abi.LtResult)))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_lt_track(self._h, len(items) if n_items is None else int(n_items), args["items"], args["desc"], args["line_status"],
                                args["prev_index"], args["distance"], args["results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernels, download
        self.last_device_ms = float(lib().uvs_lt_last_device_ms(self._h))      # HIP events around upload, kernels, download
        off = np.r_[0, np.cumsum(nl)].astype(int)
        return rc, [dict(desc=desc[off[b]:off[b + 1]].copy(), status=status[off[b]:off[b + 1]].copy(), prev_index=prev[off[b]:off[b + 1]].copy(),
                         distance=dist[off[b]:off[b + 1]].copy(), n_described=int(res[b].n_described), n_matched=int(res[b].n_matched))
                    for b in range(len(items))]

    def track(self, items):
        """items: list of dicts (stream, image [H, W] uint8, segs [n, 4]: sx, sy, ex, ey in pixels of that image) -> list of dicts: desc
        [n, 32] uint8, status [n] (abi.LT_STATUS), prev_index [n] (the slot's previous line this one continues, or -1), distance [n] (the
        Hamming distance of that match, or -1), n_described, n_matched."""
        rc, out = self.track_raw(items)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_track", rc)
        return out

    def reset(self, stream):
        rc = lib().uvs_lt_reset(self._h, int(stream))
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_reset", rc)

    def match_raw(self, prev_desc, prev_ends, cur_desc, cur_ends, n_prev=None, n_cur=None):
        """-> (return code, match_of_prev, distance, prev_of_cur) without raising."""
        pd = np.ascontiguousarray(prev_desc, np.uint8).reshape(-1, abi.LT_DESC_BYTES); pe = np.ascontiguousarray(prev_ends, np.int32).reshape(-1, 4)
        cd = np.ascontiguousarray(cur_desc, np.uint8).reshape(-1, abi.LT_DESC_BYTES); ce = np.ascontiguousarray(cur_ends, np.int32).reshape(-1, 4)
        mop = np.full(max(len(pd), 1), -1, np.int32); dist = np.full(max(len(pd), 1), -1, np.int32); poc = np.full(max(len(cd), 1), -1, np.int32)
        u8 = lambda a: a.ctypes.data_as(abi.c_u8_p) if len(a) else None
        i32 = lambda a: abi._ip(a) if len(a) else None
        rc = lib().uvs_lt_match(self._h, len(pd) if n_prev is None else int(n_prev), u8(pd), i32(pe), len(cd) if n_cur is None else int(n_cur),
                                u8(cd), i32(ce), abi._ip(mop), abi._ip(dist), abi._ip(poc))
        return rc, mop[:len(pd)], dist[:len(pd)], poc[:len(cd)]

    def match(self, prev_desc, prev_ends, cur_desc, cur_ends):
        """Stateless: descriptors [., 32] uint8 and gate points [., 4] int32 -> (match_of_prev, distance, prev_of_cur); every line counts as OK."""
        rc, mop, dist, poc = self.match_raw(prev_desc, prev_ends, cur_desc, cur_ends)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_match", rc)
        return mop, dist, poc

    def debug_line_raw(self, image, segment, null=()):
        im = np.ascontiguousarray(image, np.uint8); seg = np.ascontiguousarray(segment, np.float64).reshape(4)
        geom = np.zeros(8, np.int32); S = np.zeros((abi.LT_ROWS, 4), np.int64); df = np.zeros(abi.LT_DESC_FLOATS); desc = np.zeros(abi.LT_DESC_BYTES, np.uint8)
        args = dict(image=im.ctypes.data_as(abi.c_u8_p), segment=abi._dp(seg), geom=abi._ip(geom), row_sums=S.ctypes.data_as(C.POINTER(C.c_int64)),
                    desc_float=abi._dp(df), desc=desc.ctypes.data_as(abi.c_u8_p))
        for k in null:
            args[k] = None
        rc = lib().uvs_lt_debug_line(self._h, args["image"], im.shape[1], im.shape[0], args["segment"], args["geom"], args["row_sums"],
                                     args["desc_float"], args["desc"])
        return rc, dict(geom=geom, row_sums=S, desc_float=df, desc=desc)

    def debug_line(self, image, segment):
        """ONE segment with the intermediate results (tests only) -> dict: geom [8], row_sums [63, 4] int64, desc_float [72], desc [32]."""
        rc, out = self.debug_line_raw(image, segment)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_debug_line", rc)
        return out

    # ---- segment detection (uvs_lt_detect, uvs_lt_detect_track)
    @staticmethod
    def _det_params(grad_threshold=40, min_pixels=10, min_length=12.0):
        return abi.LtDetParams(int(grad_threshold), int(min_pixels), float(min_length))

    def _det_call(self, track, items, params, n_items=None, null=()):
        arr, keep = abi.lt_det_items(items)
        n = max(len(items), 1); ml = self.max_lines
        seg = np.zeros((n * ml, 4)); w2 = np.zeros(n * ml); info = np.zeros((n * ml, 4), np.int32)
        dres = (abi.LtDetResult * n)()
        desc = np.zeros((n * ml, abi.LT_DESC_BYTES), np.uint8); status = np.zeros(n * ml, np.int32); prev = np.full(n * ml, -1, np.int32)
        dist = np.full(n * ml, -1, np.int32); res = (abi.LtResult * n)()
        pr = self._det_params(**params)
        args = dict(items=C.cast(arr, C.POINTER(abi.LtDetItem)), params=C.pointer(pr), seg=abi._dp(seg), width2=abi._dp(w2), info=abi._ip(info),
                    det_results=C.cast(dres, C.POINTER(abi.LtDetResult)), desc=desc.ctypes.data_as(abi.c_u8_p), line_status=abi._ip(status),
                    prev_index=abi._ip(prev), distance=abi._ip(dist), results=C.cast(res, C.POINTER(abi.LtResult)))
        for k in null:
            args[k] = None
        order = ["items", "params", "seg", "width2", "info", "det_results"] + (["desc", "line_status", "prev_index", "distance", "results"] if track else [])
        fn = lib().uvs_lt_detect_track if track else lib().uvs_lt_detect
        t0 = time.perf_counter()
        rc = fn(self._h, len(items) if n_items is None else int(n_items), *[args[k] for k in order])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernels, download
        self.last_detect_device_ms = float(lib().uvs_lt_last_detect_device_ms(self._h))      # HIP events around upload, kernels, download
        out = []
        off = 0
        for b in range(len(items)):
            k = int(dres[b].n_returned); r = slice(b * ml, b * ml + k)
            d = dict(seg=seg[r].copy(), width2=w2[r].copy(), info=info[r].copy(), n_found=int(dres[b].n_found), n_returned=k,
                     n_support=int(dres[b].n_support), n_regions=[int(dres[b].n_regions[0]), int(dres[b].n_regions[1])], det_status=int(dres[b].status),
                     tail_is_zero=not seg[b * ml + k:(b + 1) * ml].any() and not info[b * ml + k:(b + 1) * ml].any())
            if track:
                t = slice(off, off + k); off += k
                d.update(desc=desc[t].copy(), status=status[t].copy(), prev_index=prev[t].copy(), distance=dist[t].copy(),
                         n_described=int(res[b].n_described), n_matched=int(res[b].n_matched))
            out.append(d)
        return rc, out

    def detect_raw(self, items, n_items=None, null=(), **params):
        """-> (return code, [dict per item]) without raising: for the tests of the argument checks.  `null` names arguments passed as NULL
        ("items", "params", "seg", "width2", "info", "det_results")."""
        return self._det_call(False, items, params, n_items, null)

    def detect(self, items, **params):
        """items: list of dicts (image [H, W] uint8); params: grad_threshold, min_pixels, min_length -> list of dicts: seg [k, 4] (start x, y,
        end x, y, ranked by length), width2 [k], info [k, 4] (name, partition, n, s), n_found, n_returned = k, n_support, n_regions [2],
        det_status (abi.LT_DET_*).  Stateless."""
        rc, out = self.detect_raw(items, **params)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_detect", rc)
        return out

    def detect_track_raw(self, items, n_items=None, null=(), **params):
        """As detect_raw for uvs_lt_detect_track; `null` may also name "desc", "line_status", "prev_index", "distance", "results"."""
        return self._det_call(True, items, params, n_items, null)

    def detect_track(self, items, **params):
        """items: list of dicts (stream, image) -> detect()'s dicts with track()'s entries for the returned segments beside them (desc, status,
        prev_index, distance, n_described, n_matched).  The image is uploaded once."""
        rc, out = self.detect_track_raw(items, **params)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_detect_track", rc)
        return out

    def debug_detect_raw(self, image, null=(), **params):
        im = np.ascontiguousarray(image, np.uint8)
        H, W = im.shape
        o = dict(blur=np.zeros((H, W), np.uint8), grad=np.zeros((H, W), np.uint32), sector_a=np.zeros((H, W), np.uint8), sector_b=np.zeros((H, W), np.uint8),
                 name_a=np.zeros((H, W), np.int32), name_b=np.zeros((H, W), np.int32), vote=np.zeros((H, W), np.uint8))
        pr = self._det_params(**params)
        args = dict(image=im.ctypes.data_as(abi.c_u8_p), params=C.pointer(pr), blur=o["blur"].ctypes.data_as(abi.c_u8_p),
                    grad=o["grad"].ctypes.data_as(C.POINTER(C.c_uint32)), sector_a=o["sector_a"].ctypes.data_as(abi.c_u8_p),
                    sector_b=o["sector_b"].ctypes.data_as(abi.c_u8_p), name_a=abi._ip(o["name_a"]), name_b=abi._ip(o["name_b"]),
                    vote=o["vote"].ctypes.data_as(abi.c_u8_p))
        for k in null:
            args[k] = None
        rc = lib().uvs_lt_debug_detect(self._h, args["image"], W, H, args["params"], args["blur"], args["grad"], args["sector_a"], args["sector_b"],
                                       args["name_a"], args["name_b"], args["vote"])
        return rc, o

    def debug_detect(self, image, **params):
        """ONE image with the per-pixel stages (tests only) -> dict of [H, W] arrays: blur, grad (gx | gy << 16), sector_a, sector_b (255 = no
        support), name_a, name_b (-1 = none), vote (0 = A, 1 = B, 255 = no support)."""
        rc, o = self.debug_detect_raw(image, **params)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_debug_detect", rc)
        return o

    # ---- undistortion: a slot's map (uvs_lt_set_undistort, uvs_lt_set_remap, uvs_lt_get_remap) and loose raw images through it (uvs_lt_undistort)
    def set_undistort_raw(self, stream, camera, width, height, col_margin=0, row_margin=0):
        cam = None if camera is None else C.byref(abi.kf_camera(camera))
        return lib().uvs_lt_set_undistort(self._h, int(stream), cam, int(width), int(height), int(col_margin), int(row_margin))

    def set_undistort(self, stream, camera, width, height, col_margin=0, row_margin=0):
        """Builds the slot's map on the device from camera = (fx, fy, cx, cy, k1, k2, p1, p2) of the raw image width x height, cropped by the
        margins: detect_track() then takes the slot's images raw.  camera = None switches it off; reset() keeps it."""
        rc = self.set_undistort_raw(stream, camera, width, height, col_margin, row_margin)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_set_undistort", rc)

    def set_undistort_model_raw(self, stream, model, width, height, out_camera, col_margin=0, row_margin=0):
        fx, fy, cx, cy = (float(v) for v in out_camera)
        return lib().uvs_lt_set_undistort_model(self._h, int(stream), _model_arg(model), int(width), int(height), int(col_margin), int(row_margin),
                                                fx, fy, cx, cy)

    def set_undistort_model(self, stream, model, width, height, out_camera, col_margin=0, row_margin=0):
        """The slot's map for any camera model (abi.CameraModel or a dict of abi.load_camera_calibration) of the raw image width x height:
        output pixel (u, v) of the pinhole out_camera = (fx, fy, cx, cy) reads the raw image where the model projects its ray.  model = None
        switches the slot's map off."""
        rc = self.set_undistort_model_raw(stream, model, width, height, out_camera, col_margin, row_margin)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_set_undistort_model", rc)

    def set_remap_raw(self, stream, src_width, src_height, map_xy, out_width=None, out_height=None, null=False):
        m = np.ascontiguousarray(map_xy, np.int32)
        oh, ow = m.shape[:2]
        return lib().uvs_lt_set_remap(self._h, int(stream), int(src_width), int(src_height), ow if out_width is None else int(out_width),
                                      oh if out_height is None else int(out_height), None if null else abi._ip(m))

    def set_remap(self, stream, src_width, src_height, map_xy):
        """The caller's own map [Ho, Wo, 2] int32 (X, Y in 1/32 px of the raw image src_width x src_height) as the slot's map."""
        rc = self.set_remap_raw(stream, src_width, src_height, map_xy)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_set_remap", rc)

    def get_remap_raw(self, stream, sizes_only=False, null=()):
        """-> (return code, map [Ho, Wo, 2] int32 or, with sizes_only, (Wo, Ho)) without raising."""
        ow = C.c_int32(0); oh = C.c_int32(0)
        args = dict(out_width=C.byref(ow), out_height=C.byref(oh))
        for k in null:
            args[k] = None
        rc = lib().uvs_lt_get_remap(self._h, int(stream), args["out_width"], args["out_height"], None)
        if rc != abi.UVS_OK or sizes_only:
            return rc, (int(ow.value), int(oh.value))
        m = np.zeros((oh.value, ow.value, 2), np.int32)
        rc = lib().uvs_lt_get_remap(self._h, int(stream), args["out_width"], args["out_height"], abi._ip(m))
        return rc, m

    def get_remap(self, stream):
        """-> the slot's map [Ho, Wo, 2] int32."""
        rc, m = self.get_remap_raw(stream)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_get_remap", rc)
        return m

    def undistort_raw(self, images, n_images=None, null=()):
        """-> (return code, [undistorted image]) without raising: for the tests of the argument checks.  images: dicts (stream, image [H, W]
        uint8, the raw image).  n_images overrides the count passed; `null` names arguments passed as NULL ("images", "out")."""
        arr, keep = abi.lt_det_items(images)
        shapes = []
        for d in images:          # the sizes of the outputs are the slots'; a slot without a map has none, and the call says so
            rc, wh = self.get_remap_raw(d.get("stream", 0), sizes_only=True)
            shapes.append((wh[1], wh[0]) if rc == abi.UVS_OK else (0, 0))
        out = np.zeros(max(sum(h * w for h, w in shapes), 1), np.uint8)
        args = dict(images=C.cast(arr, C.POINTER(abi.LtDetItem)), out=out.ctypes.data_as(abi.c_u8_p))
        for k in null:
            args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_lt_undistort(self._h, len(images) if n_images is None else int(n_images), args["images"], args["out"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernel, download
        self.last_undistort_device_ms = float(lib().uvs_lt_last_undistort_device_ms(self._h))
        if rc != abi.UVS_OK:
            return rc, []
        res, o = [], 0
        for h, w in shapes:
            res.append(out[o:o + h * w].reshape(h, w).copy()); o += h * w
        return rc, res

    def undistort(self, images):
        """images: list of dicts (stream, image [H, W] uint8: a raw image of the size of the slot's map) -> the undistorted, cropped images.
        Two images may name one slot; no line state is touched."""
        rc, out = self.undistort_raw(images)
        if rc != abi.UVS_OK:
            raise self._error("uvs_lt_undistort", rc)
        return out


def check_vocabulary(voc):
    """uvs_pr_check_vocabulary on an abi.load_vocabulary dict -> (return code, message).  Host only: needs no GPU."""
    args, keep = abi.pr_vocabulary_args(voc)
    msg = C.create_string_buffer(256)
    rc = lib().uvs_pr_check_vocabulary(*args, msg, len(msg))
    return rc, msg.value.decode()


class PlaceRecognizer(_Handle):
    """Owns one `uvs_place_recognizer` handle: place recognition of loop closure (PoseGraph::detectLoop of the reference: DBoW2's vocabulary
    tree, tf-idf bag-of-words vectors and the L1 query of their database) on one GPU.

    `voc` is a vocabulary as abi.load_vocabulary gives it (the reference's brief_k10L6.bin).  Descriptors are uint64 [n, 4] arrays as
    KeyframeExtractor returns them.  Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_pr"

    def __init__(self, voc, device=0, max_features=4096, initial_entries=1024):
        rc, msg = check_vocabulary(voc)
        if rc != abi.UVS_OK:
            raise ValueError(f"uvs_pr_check_vocabulary: {lib().uvs_status_string(rc).decode()} / {msg}")
        args, keep = abi.pr_vocabulary_args(voc)
        self.max_features = int(max_features)
        self._create(device, *args, max_features, initial_entries)
        self.last_device_ms = dict(total=0.0, transform=0.0, query=0.0)

    def _check(self, what, rc):
        if rc != abi.UVS_OK:
            raise self._error(what, rc)
        L = lib()
        self.last_device_ms = dict(total=float(L.uvs_pr_last_device_ms(self._h, 0)), transform=float(L.uvs_pr_last_device_ms(self._h, 1)),
                                   query=float(L.uvs_pr_last_device_ms(self._h, 2)))

    def size(self):
        return int(lib().uvs_pr_size(self._h))

    def clear(self):
        self._check("uvs_pr_clear", lib().uvs_pr_clear(self._h))

    def transform_raw(self, frames, n_frames=None):
        """-> (return code, [dict(words, weights, bow_words, bow_values) per frame]) without raising."""
        nf, desc = abi.pr_frames(frames)
        n, tot = len(frames), max(int(nf.sum()), 1)
        words = np.zeros(tot, np.int32); weights = np.zeros(tot); bow_n = np.zeros(max(n, 1), np.int32)
        bw = np.zeros(max(n, 1) * self.max_features, np.int32); bv = np.zeros(max(n, 1) * self.max_features)
        rc = lib().uvs_pr_transform(self._h, n if n_frames is None else int(n_frames), nf.ctypes.data_as(abi.c_i32_p), desc.ctypes.data_as(abi.c_u64_p),
                                    words.ctypes.data_as(abi.c_i32_p), abi._dp(weights), bow_n.ctypes.data_as(abi.c_i32_p), bw.ctypes.data_as(abi.c_i32_p), abi._dp(bv))
        off = np.r_[0, np.cumsum(nf)].astype(int)
        out = []
        for f in range(n):
            s = slice(f * self.max_features, f * self.max_features + int(bow_n[f]))
            out.append(dict(words=words[off[f]:off[f + 1]].copy(), weights=weights[off[f]:off[f + 1]].copy(), bow_words=bw[s].copy(), bow_values=bv[s].copy()))
        return rc, out

    def transform(self, frames):
        """frames: list of uint64 [n_f, 4] descriptor arrays -> list of dicts: words int32 [n_f] and weights [n_f] (the leaf of every
        descriptor, stop words included), bow_words int32 [m] ascending and bow_values [m] (the normalized tf-idf vector).  Changes no state."""
        rc, out = self.transform_raw(frames)
        self._check("uvs_pr_transform", rc)
        return out

    def add(self, frames):
        """Appends the frames' vectors in order -> their entry ids int32 [n]."""
        nf, desc = abi.pr_frames(frames)
        ids = np.zeros(max(len(frames), 1), np.int32)
        rc = lib().uvs_pr_add(self._h, len(frames), nf.ctypes.data_as(abi.c_i32_p), desc.ctypes.data_as(abi.c_u64_p), ids.ctypes.data_as(abi.c_i32_p))
        self._check("uvs_pr_add", rc)
        return ids[:len(frames)].copy()

    def query(self, frames, max_results=4, max_id=-1):
        """The frames against the database as it is -> list of (ids int32 [m], scores [m]) in descending score, a tie to the lower id.
        max_results 0: all; max_id: one int or one per frame (entry e is eligible iff e < max_id or max_id == -1 or e is the last entry)."""
        nf, desc = abi.pr_frames(frames)
        n = len(frames)
        mid = np.ascontiguousarray(np.broadcast_to(np.asarray(max_id, np.int32), (n,)))
        stride = max(int(max_results) if max_results > 0 else self.size(), 1)
        nres = np.zeros(max(n, 1), np.int32); ids = np.zeros(max(n, 1) * stride, np.int32); sc = np.zeros(max(n, 1) * stride)
        rc = lib().uvs_pr_query(self._h, n, nf.ctypes.data_as(abi.c_i32_p), desc.ctypes.data_as(abi.c_u64_p), int(max_results), mid.ctypes.data_as(abi.c_i32_p),
                                nres.ctypes.data_as(abi.c_i32_p), ids.ctypes.data_as(abi.c_i32_p), abi._dp(sc))
        self._check("uvs_pr_query", rc)
        st = int(max_results) if max_results > 0 else self.size()
        return [(ids[f * st:f * st + int(nres[f])].copy(), sc[f * st:f * st + int(nres[f])].copy()) for f in range(n)]

    def detect(self, desc, frame_index):
        """detectLoop for one keyframe: query(4, frame_index - 50), then add, then the score gates -> (loop index or -1, ids, scores)."""
        nf, d = abi.pr_frames([desc])
        loop = C.c_int32(-1); nres = C.c_int32(0)
        ids = np.zeros(abi.PR_DETECT_RESULTS, np.int32); sc = np.zeros(abi.PR_DETECT_RESULTS)
        t0 = time.perf_counter()
        rc = lib().uvs_pr_detect(self._h, int(nf[0]), d.ctypes.data_as(abi.c_u64_p), int(frame_index), C.byref(loop), C.byref(nres),
                                 ids.ctypes.data_as(abi.c_i32_p), abi._dp(sc))
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call
        self._check("uvs_pr_detect", rc)
        return int(loop.value), ids[:nres.value].copy(), sc[:nres.value].copy()


class Triangulator(_Handle):
    """Owns one `uvs_tri` handle: the state a solve starts from -- FeatureManager::triangulate, triangulateLine, the validity rule of setLineOrtho
    and the re-anchoring of removeBackShiftDepth -- for whole batches of landmarks on one GPU, one lane per landmark.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_tri"
    INIT_DEPTH = 5.0

    def __init__(self, device=0, max_windows=256, max_points=40000, max_point_obs=None, max_lines=10000, init_depth=None):
        self._create(device, max_windows, max_points, max_points * abi.NUM_FRAMES if max_point_obs is None else max_point_obs, max_lines)
        self.init_depth = self.INIT_DEPTH if init_depth is None else float(init_depth)
        self.set_init_depth(self.init_depth)

    def set_init_depth_raw(self, init_depth):
        return lib().uvs_tri_set_init_depth(self._h, float(init_depth))

    def set_init_depth(self, init_depth):
        """The depth uvs_tri_shift_depth falls back to, and the default of triangulate()."""
        rc = self.set_init_depth_raw(init_depth)
        if rc != abi.UVS_OK:
            raise self._error("uvs_tri_set_init_depth", rc)
        self.init_depth = float(init_depth)

    def _timed(self, fn, *args):
        t0 = time.perf_counter()
        rc = fn(self._h, *args)
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: packing, upload, kernels, download
        self.last_device_ms = float(lib().uvs_tri_last_device_ms(self._h))      # HIP events around the kernels alone
        return rc

    def triangulate_raw(self, batch, init_depth=None, null=(), n_windows=None):
        """-> (return code, depth, pt_flag, orth, ln_flag) without raising: for the tests of the argument checks.  `null` names batch fields or
        outputs ("depth", "pt_flag", "orth", "ln_flag") passed as NULL, or "batch"; n_windows overrides the count passed."""
        b, keep = abi.tri_batch(batch, null)
        if n_windows is not None:
            b.n_windows = int(n_windows)
        depth = np.zeros(max(b.n_points, 1)); pf = np.full(max(b.n_points, 1), -1, np.int32)
        orth = np.zeros((max(b.n_lines, 1), 4)); lf = np.full(max(b.n_lines, 1), -1, np.int32)
        out = dict(depth=abi._dp(depth), pt_flag=pf.ctypes.data_as(abi.c_i32_p), orth=abi._dp(orth), ln_flag=lf.ctypes.data_as(abi.c_i32_p))
        for k in null:
            if k in out:
                out[k] = None
        rc = self._timed(lib().uvs_tri_triangulate, None if "batch" in null else C.byref(b), self.init_depth if init_depth is None else float(init_depth),
                         out["depth"], out["pt_flag"], out["orth"], out["ln_flag"])
        return rc, depth[:b.n_points], pf[:b.n_points], orth[:b.n_lines], lf[:b.n_lines]

    def triangulate(self, batch, init_depth=None):
        """batch: a dict with the fields of uvs_tri_batch as arrays (abi.tri_batch) -> (depth [n_points], pt_flag, orth [n_lines, 4], ln_flag).
        pt_flag 0 kept / 1 below 0.1 / 2 not finite (1, 2: init_depth returned); ln_flag 0 ok / 2 degenerate (four zeros returned)."""
        rc, depth, pf, orth, lf = self.triangulate_raw(batch, init_depth)
        if rc != abi.UVS_OK:
            raise self._error("uvs_tri_triangulate", rc)
        return depth, pf, orth, lf

    def check_lines_raw(self, pose, ex_pose, ln_window, ln_start, ln_sp0, ln_ep0, orth_old):
        f64 = lambda a, *shape: np.ascontiguousarray(a, np.float64).reshape(*shape)
        pose, ex = f64(pose, -1, abi.NUM_FRAMES, 7), f64(ex_pose, -1, 7)
        win, start = np.ascontiguousarray(ln_window, np.int32), np.ascontiguousarray(ln_start, np.int32)
        sp, ep, old = f64(ln_sp0, -1, 3), f64(ln_ep0, -1, 3), f64(orth_old, -1, 4)
        n = len(win)
        flag = np.full(max(n, 1), -1, np.int32)
        ip = lambda a: a.ctypes.data_as(abi.c_i32_p)
        rc = self._timed(lib().uvs_tri_check_lines, len(pose), abi._dp(pose), abi._dp(ex), n, ip(win), ip(start), abi._dp(sp), abi._dp(ep), abi._dp(old), ip(flag))
        return rc, flag[:n]

    def check_lines(self, pose, ex_pose, ln_window, ln_start, ln_sp0, ln_ep0, orth_old):
        """The decision of setLineOrtho with the OLD parameters -> flag [n_lines]: 1 valid, 2 an end point behind the start camera."""
        rc, flag = self.check_lines_raw(pose, ex_pose, ln_window, ln_start, ln_sp0, ln_ep0, orth_old)
        if rc != abi.UVS_OK:
            raise self._error("uvs_tri_check_lines", rc)
        return flag

    def shift_depth_raw(self, uv0, depth, marg_R, marg_P, new_R, new_P):
        f64 = lambda a, *shape: np.ascontiguousarray(a, np.float64).reshape(*shape)
        uv0, depth = f64(uv0, -1, 3), f64(depth, -1)
        mR, mP, nR, nP = f64(marg_R, 3, 3), f64(marg_P, 3), f64(new_R, 3, 3), f64(new_P, 3)
        n = len(depth)
        out = np.zeros(max(n, 1)); flag = np.full(max(n, 1), -1, np.int32)
        rc = self._timed(lib().uvs_tri_shift_depth, n, abi._dp(uv0), abi._dp(depth), abi._dp(mR), abi._dp(mP), abi._dp(nR), abi._dp(nP), abi._dp(out),
                         flag.ctypes.data_as(abi.c_i32_p))
        return rc, out[:n], flag[:n]

    def shift_depth(self, uv0, depth, marg_R, marg_P, new_R, new_P):
        """The re-anchoring of removeBackShiftDepth -> (depth_out [n], flag [n]: 0, or 1 where init_depth was put)."""
        rc, out, flag = self.shift_depth_raw(uv0, depth, marg_R, marg_P, new_R, new_P)
        if rc != abi.UVS_OK:
            raise self._error("uvs_tri_shift_depth", rc)
        return out, flag

    @staticmethod
    def tracks_of(windows):
        """The batch dict of a list of abi.Window: a point's track is the anchor's pts_i, then each pts_j, of its observations in order (they must
        lie in consecutive frames from pt_fi on); a line's two views are the first and the last of its observations."""
        b = dict(pose=np.stack([w.pose for w in windows]), ex_pose=np.stack([w.ex_pose for w in windows]))
        pw, ps, pn, po, lw, lfi, lfj, ends = [], [], [], [], [], [], [], [[], [], [], []]
        for wi, w in enumerate(windows):
            order = np.argsort(w.pt_lm, kind="stable")
            lm = np.asarray(w.pt_lm)[order]
            first = np.flatnonzero(np.r_[True, lm[1:] != lm[:-1]]); count = np.diff(np.r_[first, len(lm)])
            if len(first) != len(w.inv_depth) or (len(lm) and not np.array_equal(lm[first], np.arange(len(first)))):
                raise ValueError("triangulate_windows: every point needs at least one observation")
            k_in_track = np.arange(len(lm)) - np.repeat(first, count)
            if np.any(np.asarray(w.pt_fj)[order] != np.asarray(w.pt_fi)[order] + 1 + k_in_track):
                raise ValueError("triangulate_windows: a point's observations must lie in consecutive frames after its start frame")
            pw += [wi] * len(first); ps += list(np.asarray(w.pt_fi)[order][first]); pn += list(count + 1)
            for f, c in zip(first, count):
                po.append(np.asarray(w.pt_pi)[order[f]][None]); po.append(np.asarray(w.pt_pj)[order[f:f + c]])
            order = np.argsort(w.ln_lm, kind="stable")
            lm = np.asarray(w.ln_lm)[order]
            first = np.flatnonzero(np.r_[True, lm[1:] != lm[:-1]]); last = np.r_[first[1:], len(lm)] - 1
            if len(first) != len(w.line_orth) or (len(lm) and not np.array_equal(lm[first], np.arange(len(first)))):
                raise ValueError("triangulate_windows: every line needs at least one observation")
            a, z = order[first], order[last]
            lw += [wi] * len(first); lfi += list(np.asarray(w.ln_fj)[a]); lfj += list(np.asarray(w.ln_fj)[z])
            for dst, src in zip(ends, (w.ln_sp[a], w.ln_ep[a], w.ln_sp[z], w.ln_ep[z])):
                dst.append(np.asarray(src).reshape(-1, 3))
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros((0, 3))
        b.update(pt_window=np.array(pw, np.int32), pt_start=np.array(ps, np.int32), pt_obs_begin=np.r_[0, np.cumsum(pn)].astype(np.int32), pt_obs=cat(po),
                 ln_window=np.array(lw, np.int32), ln_fi=np.array(lfi, np.int32), ln_fj=np.array(lfj, np.int32),
                 ln_sp_i=cat(ends[0]), ln_ep_i=cat(ends[1]), ln_sp_j=cat(ends[2]), ln_ep_j=cat(ends[3]))
        return b

    def triangulate_windows(self, windows, init_depth=None):
        """Every landmark of every window in one call -> (inv_depth: list of [n_points] arrays, line_orth: list of [n_lines, 4] arrays, pt_flag,
        ln_flag), ready to be put into the windows that go to the batch or the large-window entry points."""
        b = self.tracks_of(windows)
        depth, pf, orth, lf = self.triangulate(b, init_depth)
        pcut = np.cumsum([len(w.inv_depth) for w in windows])[:-1]; lcut = np.cumsum([len(w.line_orth) for w in windows])[:-1]
        return np.split(1.0 / depth, pcut), np.split(orth, lcut), np.split(pf, pcut), np.split(lf, lcut)


class ImuPreintegrator(_Handle):
    """Owns one `uvs_imu` handle: IntegrationBase's pre-integration (and, on request, processIMU's dead reckoning) for whole batches of
    intervals on one GPU, one wavefront per interval.  Re-propagation is the same call with other biases.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_imu"
    FILL = -7.0        # what preintegrate_raw puts into its outputs before the call: a refused call must leave it there

    def __init__(self, device=0, max_intervals=2560, max_samples=2560 * 64):
        self._create(device, int(max_intervals), int(max_samples))
        self.last_ms = self.last_device_ms = 0.0

    def set_noise_raw(self, acc_n, gyr_n, acc_w, gyr_w):
        return lib().uvs_imu_set_noise(self._h, float(acc_n), float(gyr_n), float(acc_w), float(gyr_w))

    def set_noise(self, acc_n, gyr_n, acc_w, gyr_w):
        """The noise densities behind `covariance` (a new handle: synth.ACC_N, GYR_N, ACC_W, GYR_W)."""
        rc = self.set_noise_raw(acc_n, gyr_n, acc_w, gyr_w)
        if rc != abi.UVS_OK:
            raise self._error("uvs_imu_set_noise", rc)

    def preintegrate_raw(self, batch, null=(), n_intervals=None):
        """-> (return code, blocks, pred_p, pred_R, pred_v) without raising: for the tests of the argument checks.  `null` names batch fields or
        outputs ("blocks", "pred_p", "pred_R", "pred_v") passed as NULL, or "batch"; n_intervals overrides the count passed.  The outputs are
        filled with FILL before the call (every byte of `blocks` with 0xA5)."""
        b, keep = abi.imu_batch(batch, null)
        if n_intervals is not None:
            b.n_intervals = int(n_intervals)
        n = max(len(keep["sample_begin"]) - 1, 0)
        blocks = np.frombuffer(bytearray(b"\xa5" * (max(n, 1) * abi.IMU_BLOCK_DTYPE.itemsize)), abi.IMU_BLOCK_DTYPE)
        pp = np.full((max(n, 1), 3), self.FILL); pR = np.full((max(n, 1), 3, 3), self.FILL); pv = np.full((max(n, 1), 3), self.FILL)
        out = dict(blocks=C.c_void_p(blocks.ctypes.data), pred_p=abi._dp(pp), pred_R=abi._dp(pR), pred_v=abi._dp(pv))
        for k in null:
            if k in out:
                out[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_imu_preintegrate(self._h, None if "batch" in null else C.byref(b), out["blocks"], out["pred_p"], out["pred_R"], out["pred_v"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: checks, packing, upload, kernel, download
        self.last_device_ms = float(lib().uvs_imu_last_device_ms(self._h))      # HIP events around the kernel alone
        return rc, blocks[:n], pp[:n], pR[:n], pv[:n]

    def preintegrate(self, batch):
        """batch: a dict with the fields of uvs_imu_batch as arrays (abi.imu_batch, abi.imu_batch_of) -> blocks, a structured array of
        abi.IMU_BLOCK_DTYPE [n_intervals]; with the dead-reckoning state in the batch -> (blocks, pred_p [n, 3], pred_R [n, 3, 3], pred_v [n, 3])."""
        rc, blocks, pp, pR, pv = self.preintegrate_raw(batch)
        if rc != abi.UVS_OK:
            raise self._error("uvs_imu_preintegrate", rc)
        return (blocks, pp, pR, pv) if batch.get("state_p") is not None else blocks

    @staticmethod
    def block_dict(rec):
        """One record of the structured blocks as the dict abi.Window.imu carries."""
        return dict(sum_dt=float(rec["sum_dt"]), delta_p=rec["delta_p"].copy(), delta_q=rec["delta_q"].copy(), delta_v=rec["delta_v"].copy(),
                    linearized_ba=rec["linearized_ba"].copy(), linearized_bg=rec["linearized_bg"].copy(), jacobian=rec["jacobian"].copy(),
                    covariance=rec["covariance"].copy(), frame_i=int(rec["frame_i"]), skip=int(rec["skip"]))

    def preintegrate_windows(self, samples_per_window, ba, bg):
        """samples_per_window: per window the list synth._simulate_frames(..., samples=) fills -- entry 0 holds the one message the first interval
        starts from, entry f + 1 the (dt, acc, gyr) messages of the interval frame f -> f + 1; ba, bg: per window [3], or [n_frames - 1, 3] per
        interval.  One call for every interval of every window -> per window the `imu` list of abi.Window (frame_i = 0, 1, ...)."""
        intervals = []
        for wi, frames in enumerate(samples_per_window):
            start = frames[0][-1]
            wba = np.broadcast_to(np.asarray(ba[wi], np.float64), (len(frames) - 1, 3)); wbg = np.broadcast_to(np.asarray(bg[wi], np.float64), (len(frames) - 1, 3))
            for f, msgs in enumerate(frames[1:]):
                intervals.append(dict(acc_0=start[1], gyr_0=start[2], ba=wba[f], bg=wbg[f], frame_i=f, dt=[m[0] for m in msgs],
                                      acc=np.array([m[1] for m in msgs]).reshape(-1, 3), gyr=np.array([m[2] for m in msgs]).reshape(-1, 3)))
                if msgs:
                    start = msgs[-1]
        blocks = self.preintegrate(abi.imu_batch_of(intervals))
        out, at = [], 0
        for frames in samples_per_window:
            out.append([self.block_dict(blocks[at + f]) for f in range(len(frames) - 1)]); at += len(frames) - 1
        return out


class RelativePose(_Handle):
    """Owns one `uvs_rp` handle: Estimator::relativePose -- the gates, the fundamental-matrix RANSAC of uvs_ft_reject and recoverPose -- for
    batches of frame pairs (frame_l, WINDOW_SIZE) on one GPU.  The ten pairs of a window are ten items of one launch; a window's answer is its
    first item with ok.

    Fails loudly (RuntimeError) without a GPU -- there is no CPU path."""

    _UNIT = "uvs_rp"
    FILL = 0xA5        # what solve_raw puts into every byte of its outputs before the call: a refused call must leave it there

    def __init__(self, device=0, max_items=2560, max_points=1024, **params):
        self._create(device, int(max_items), int(max_points))
        self.params = abi.rp_params(**params)
        self.last_ms = 0.0
        self.last_device_ms = (0.0, 0.0, 0.0)

    def solve_raw(self, items, n_windows=None, null=(), n_items=None, params=None):
        """-> (return code, item results [n] of abi.RP_ITEM_RESULT_DTYPE, list of final masks, window results [n_windows] of
        abi.RP_WINDOW_RESULT_DTYPE) without raising: for the tests of the argument checks.  `null` names "items", "params", "mask",
        "item_results", "window_results", or "left" / "right" (the point arrays of every item); n_items / n_windows override the counts."""
        arr, keep = abi.rp_items_of(items, null)
        nw = (max([int(it.get("window", 0)) for it in items], default=0) + 1) if n_windows is None else int(n_windows)
        counts = [len(keep[2 * k]) for k in range(len(items))]
        mask = np.full(max(sum(counts), 1), self.FILL, np.uint8)
        res = np.frombuffer(bytearray(bytes([self.FILL]) * (max(len(items), 1) * abi.RP_ITEM_RESULT_DTYPE.itemsize)), abi.RP_ITEM_RESULT_DTYPE)
        win = np.frombuffer(bytearray(bytes([self.FILL]) * (max(nw, 1) * abi.RP_WINDOW_RESULT_DTYPE.itemsize)), abi.RP_WINDOW_RESULT_DTYPE)
        p = self.params if params is None else params
        args = dict(items=arr, params=C.byref(p), mask=mask.ctypes.data_as(abi.c_u8_p), item_results=C.c_void_p(res.ctypes.data),
                    window_results=C.c_void_p(win.ctypes.data))
        for k in null:
            if k in args:
                args[k] = None
        t0 = time.perf_counter()
        rc = lib().uvs_rp_relative_pose(self._h, len(items) if n_items is None else int(n_items), args["items"], args["params"], args["mask"],
                                        args["item_results"], nw, args["window_results"])
        self.last_ms = (time.perf_counter() - t0) * 1e3       # the whole C-ABI call: checks, packing, upload, kernels, download
        self.last_device_ms = tuple(float(lib().uvs_rp_last_device_ms(self._h, k)) for k in range(3))      # gate, RANSAC, recover
        cut = np.cumsum(counts)[:-1] if counts else []
        return rc, res[:len(items)], np.split(mask[:sum(counts)], cut), win[:max(nw, 0)]

    def solve(self, items, n_windows=None):
        """items: dicts with window, frame_l, seed, left [n, 2], right [n, 2] (abi.rp_items_of) -> (item results, a structured array of
        abi.RP_ITEM_RESULT_DTYPE; the final recoverPose mask of every item; window results of abi.RP_WINDOW_RESULT_DTYPE)."""
        rc, res, masks, win = self.solve_raw(items, n_windows)
        if rc != abi.UVS_OK:
            raise self._error("uvs_rp_relative_pose", rc)
        return res, masks, win

    @staticmethod
    def corresponding(tracks, frame_l, frame_r=abi.WINDOW_SIZE):
        """FeatureManager::getCorresponding: of the tracks (start_frame, points [n_frames, 2 or 3]), in feature order, those with
        start_frame <= frame_l and start_frame + n_frames - 1 >= frame_r -> (left [n, 2], right [n, 2])."""
        l, r = [], []
        for start, pts in tracks:
            pts = np.asarray(pts, np.float64)
            if start <= frame_l and start + len(pts) - 1 >= frame_r:
                l.append(pts[frame_l - start, :2]); r.append(pts[frame_r - start, :2])
        return np.array(l, np.float64).reshape(-1, 2), np.array(r, np.float64).reshape(-1, 2)

    @classmethod
    def window_items(cls, windows, seeds=None):
        """The WINDOW_SIZE items of every window: windows[w] is the window's track list; the seed of item (w, l) is seeds[w][l], or
        w * WINDOW_SIZE + l."""
        items = []
        for w, tracks in enumerate(windows):
            for l in range(abi.WINDOW_SIZE):
                left, right = cls.corresponding(tracks, l)
                items.append(dict(window=w, frame_l=l, seed=(w * abi.WINDOW_SIZE + l) if seeds is None else seeds[w][l], left=left, right=right))
        return items

    def relative_pose_windows(self, windows, seeds=None):
        """windows: per window the tracks as (start_frame, per-frame points) in feature order.  One call for the ten pairs of every window
        -> (l [n_windows] (-1: no pair passed), Rotation [n_windows, 3, 3], Translation [n_windows, 3], the per-item results, the masks)."""
        res, masks, win = self.solve(self.window_items(windows, seeds), n_windows=len(windows))
        return win["l"].copy(), win["Rotation"].copy(), win["Translation"].copy(), res, masks
