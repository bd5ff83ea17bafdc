"""ctypes binding of libpcp's C ABI (include/pcp_abi.h).

This is plumbing for tests, the benchmark and Python callers: every compute call goes to
the HIP library.  There is no CPU fallback: if libpcp.so is missing or no GPU is present,
the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "_lib" / "libpcp.so"

PCP_OK = 0
PCP_E_INVALID = -1
PCP_E_HIP = -2
PCP_E_CAPACITY = -3
PCP_E_STATE = -4
PCP_E_NOMEM = -5

MAX_STEPS = 4096   # PCP_MAX_STEPS of include/pcp_abi.h: the longest step table a query marches

# pcp_debug_math's ops (PCP_MATH_* of include/pcp_abi.h)
MATH_SCORE_SIN_PART, MATH_ACOS_RAW, MATH_ATAN2_RAW, MATH_ATAN2_CR = 1, 2, 3, 4
MATH_ATAN2F, MATH_SINF, MATH_COSF, MATH_DIVF, MATH_SQRTF = 10, 11, 12, 13, 14
(MATH_F64_DIV, MATH_F64_SQRT, MATH_F64_TO_F32, MATH_F64_FMA, MATH_F64_NEXTAFTER,
 MATH_F64_NEARBYINT) = 20, 21, 22, 23, 24, 25
MATH_NORMAL = 30

PCP_MEM_DEVICE_IN = 1
PCP_MEM_DEVICE_OUT = 2

F_RANGE_Z, F_FOV_Z, F_VIS_Z, F_RANGE_M, F_FOV_M, F_VIS_M = 1, 2, 4, 8, 16, 32

KERNELS = ["raycast_fan", "score_cells", "zx120_cells", "pose_sum", "cell_flags",
           "candidates", "index_build", "crop", "voxel", "transform", "filter_merge", "excavate",
           "excav_setup", "voxel_redo", "place_sensors"]


class PcpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pcp error {code}: {msg}")
        self.code = code


class CloudView(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n", C.c_uint64), ("point_step", C.c_uint32),
                ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32)]


class Rigid(C.Structure):
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4)]


class VlParams(C.Structure):
    _fields_ = [("grid_resolution", C.c_double), ("sensor_height", C.c_double),
                ("search_radius", C.c_double), ("max_distance", C.c_double),
                ("num_candidates", C.c_int32), ("vertical_layers", C.c_int32)]


class VlReport(C.Structure):
    _fields_ = [("best_idx", C.c_int64), ("best_score", C.c_double),
                ("zx120_total_score", C.c_double),
                ("zx120_range_ok", C.c_int32), ("zx120_fov_ok", C.c_int32),
                ("zx120_visible_ok", C.c_int32), ("total_cells", C.c_int32),
                ("zx120_green", C.c_int32), ("zx120_red", C.c_int32),
                ("zx120_blue", C.c_int32), ("zx120_yellow", C.c_int32),
                ("green", C.c_int32), ("red", C.c_int32), ("blue", C.c_int32),
                ("yellow", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class FanParams(C.Structure):
    _fields_ = [("n_az", C.c_int32), ("n_el", C.c_int32), ("el_min", C.c_double),
                ("el_max", C.c_double), ("max_distance", C.c_double)]


ABI_VERSION = 2   # PCP_ABI_VERSION of include/pcp_abi.h

PLACE_MAX = 16     # PCP_PLACE_MAX: sensors one pcp_place_sensors call places at most
OWNER_ZX120 = -1   # PCP_OWNER_ZX120 / PCP_OWNER_NONE: cell owners that are no placement round
OWNER_NONE = -2


class PlaceParams(C.Structure):
    """pcp_place_params."""
    _fields_ = [("k_max", C.c_int32), ("reserved", C.c_int32), ("min_separation", C.c_double)]


PAIR_MAX_POSES = 2048   # PCP_PAIR_MAX_POSES: poses one pcp_place_pair call searches at most


class PairParams(C.Structure):
    """pcp_pair_params."""
    _fields_ = [("n_fixed", C.c_int32), ("reserved", C.c_int32), ("min_separation", C.c_double),
                ("fixed", C.c_int64 * PLACE_MAX)]


TRIPLE_MAX_POSES = 512         # PCP_TRIPLE_MAX_POSES: poses one pcp_place_triple call searches
TRIPLE_TABLE_MAX_POSES = 128   # PCP_TRIPLE_TABLE_MAX_POSES: the dense [n][n][n] table's limit

REFINE_MAX_MOVES = 64   # PCP_REFINE_MAX_MOVES: moves one pcp_place_refine call records at most


class RefineParams(C.Structure):
    """pcp_refine_params."""
    _fields_ = [("k", C.c_int32), ("n_locked", C.c_int32), ("max_moves", C.c_int32),
                ("reserved", C.c_int32), ("min_separation", C.c_double),
                ("start", C.c_int64 * PLACE_MAX)]


AIM_MAX = 64           # PCP_AIM_MAX: aims one pcp_place_aimed call searches per pose
AIM_MAX_ROWS = 65536   # PCP_AIM_MAX_ROWS: (pose, aim) rows one call searches at most


class AimParams(C.Structure):
    """pcp_aim_params."""
    _fields_ = [("k_max", C.c_int32), ("n_aims", C.c_int32), ("n_fixed", C.c_int32),
                ("reserved", C.c_int32), ("h_fov", C.c_double), ("v_fov", C.c_double),
                ("min_separation", C.c_double), ("fixed_pose", C.c_int64 * PLACE_MAX),
                ("fixed_aim", C.c_int32 * PLACE_MAX)]


SCAN_MAX_POSES = 64   # PCP_SCAN_MAX_POSES: poses one pcp_simulate_scan call casts (mask bits)


COVER_MAX_POSES = 1024   # PCP_COVER_MAX_POSES: poses one pcp_place_coverage call searches


class CoverParams(C.Structure):
    """pcp_cover_params."""
    _fields_ = [("k_max", C.c_int32), ("n_fixed", C.c_int32), ("reserved", C.c_int32 * 2),
                ("min_separation", C.c_double), ("fixed", C.c_int64 * PLACE_MAX)]


COVER_AIM_MAX = 64   # PCP_COVER_AIM_MAX: aims one pcp_place_coverage_aimed call searches per pose


class CoverAimParams(C.Structure):
    """pcp_cover_aim_params."""
    _fields_ = [("k_max", C.c_int32), ("n_aims", C.c_int32), ("n_fixed", C.c_int32),
                ("w_az", C.c_int32), ("w_el", C.c_int32), ("reserved", C.c_int32 * 3),
                ("min_separation", C.c_double), ("fixed_pose", C.c_int64 * PLACE_MAX),
                ("fixed_aim", C.c_int32 * PLACE_MAX)]


class ScanReturn(C.Structure):
    """pcp_scan_return: one blocked ray's hit (24 bytes)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("range", C.c_float),
                ("ray", C.c_uint32), ("point", C.c_uint32)]


# the same record as a NumPy structured dtype (Context.simulate_scan's `returns`)
SCAN_RETURN_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32),
                              ("range", np.float32), ("ray", np.uint32), ("point", np.uint32)])


class IndexInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("cell", C.c_double), ("nx", C.c_int32),
                ("ny", C.c_int32), ("nz", C.c_int32), ("fine_pivot", C.c_int32),
                ("bmin", C.c_double * 3),
                ("bmax", C.c_double * 3), ("scan_layout", C.c_int32), ("fine_tile", C.c_int32)]


class FineGeo(C.Structure):
    """pcp_fine_geo: the fine-window copy's geometry (pcp_debug_fine_copy)."""
    _fields_ = ([(k, C.c_int32) for k in ("built", "tile", "skip", "packed", "nx", "ny", "nz", "F",
                                          "reach", "fnx", "fny", "rz", "tsteps")] +
                [(k, C.c_uint64) for k in ("n_points", "n_records", "n_entries", "start_off",
                                           "frec_bytes", "wpts_bytes", "pts_bytes")] +
                [(k, C.c_double) for k in ("ox", "oy", "oz", "c", "inv_c", "r_q", "cf", "inv_cf",
                                           "R2", "zq", "clear_zt0", "clear_c")])


class FinePivotGeo(C.Structure):
    """pcp_fine_pivot_geo: the pivot table's geometry (pcp_debug_fine_pivot)."""
    _fields_ = ([(k, C.c_int32) for k in ("built", "enabled", "fnx", "fny", "tx", "ty")] +
                [(k, C.c_uint64) for k in ("n_slots", "bytes")] +
                [(k, C.c_double) for k in ("ox", "oy", "cf")])


class RuntimeInfo(C.Structure):
    _fields_ = [("hip_runtime_version", C.c_int32), ("rccl_version", C.c_int32),
                ("hip_path", C.c_char * 512), ("rccl_path", C.c_char * 512)]


# (name, restype, argtypes) for every entry point of include/pcp_abi.h
_P = C.c_void_p
_SIGS = [
    ("pcp_abi_version", C.c_int, []),
    ("pcp_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("pcp_alloc_stats", C.c_int, [_P, _P, _P]),
    ("pcp_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("pcp_destroy", None, [_P]),
    ("pcp_last_error", C.c_char_p, [_P]),
    ("pcp_synchronize", C.c_int, [_P]),
    ("pcp_dev_alloc", C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    ("pcp_dev_free", C.c_int, [_P, _P]),
    ("pcp_memcpy_h2d", C.c_int, [_P, _P, _P, C.c_uint64]),
    ("pcp_memcpy_d2h", C.c_int, [_P, _P, _P, C.c_uint64]),
    ("pcp_host_alloc", C.c_int, [_P, C.c_uint64, _P]),
    ("pcp_host_free", C.c_int, [_P, _P]),
    ("pcp_host_register", C.c_int, [_P, _P, C.c_uint64]),
    ("pcp_host_unregister", C.c_int, [_P, _P]),
    ("pcp_profile_enable", C.c_int, [_P, C.c_int]),
    ("pcp_profile_reset", C.c_int, [_P]),
    ("pcp_profile_get", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("pcp_kernel_name", C.c_char_p, [C.c_int]),
    ("pcp_crop_box", C.c_int, [_P, C.POINTER(CloudView), _P, _P, _P, C.c_uint64,
                               C.POINTER(C.c_uint64)]),
    ("pcp_voxel_grid", C.c_int, [_P, C.POINTER(CloudView), C.c_float, _P, _P, _P, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("pcp_crop_voxel", C.c_int, [_P, C.POINTER(CloudView), _P, C.c_float, _P, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("pcp_transform_concat", C.c_int, [_P, C.c_int, C.POINTER(CloudView), C.POINTER(Rigid), _P,
                                       _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("pcp_filter_merge", C.c_int, [_P, C.c_int, C.POINTER(CloudView), _P, C.c_float,
                                   C.POINTER(Rigid), _P, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                   _P, C.c_uint32]),
    ("pcp_filter_merge_nodes", C.c_int, [_P, C.c_int, C.POINTER(CloudView), _P, C.c_float,
                                         C.POINTER(Rigid), _P, _P, C.c_uint64,
                                         C.POINTER(C.c_uint64), _P, _P, _P]),
    ("pcp_set_terrain", C.c_int, [_P, C.POINTER(CloudView)]),
    ("pcp_set_aux_cloud", C.c_int, [_P, C.POINTER(CloudView)]),
    ("pcp_set_cells", C.c_int, [_P, _P, _P, C.c_uint64]),
    ("pcp_set_excavation_area", C.c_int, [_P, _P, C.c_double, C.c_int32, _P, _P]),
    ("pcp_set_excavation_area_async", C.c_int, [_P, _P, C.c_double, C.c_int32, _P, _P]),
    ("pcp_cells_count", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("pcp_get_cells", C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    ("pcp_get_area_normals", C.c_int, [_P, _P, C.c_uint64, _P]),
    ("pcp_excavate", C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, _P]),
    ("pcp_excavate_bounds", C.c_int, [_P, C.c_uint64, _P, _P]),
    ("pcp_filter_merge_landed", C.c_int, [_P, C.c_int, _P, _P]),
    ("pcp_excavate_area_async", C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P,
                                          _P, C.c_double, C.c_int32, _P, _P]),
    ("pcp_excavate_landed", C.c_int, [_P, _P, _P]),
    ("pcp_drivable_area", C.c_int, [_P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                                    _P, _P, C.c_uint64, _P, _P]),
    ("pcp_generate_candidates", C.c_int, [_P, _P, C.POINTER(VlParams), _P, _P, C.c_uint64,
                                          C.POINTER(C.c_uint64)]),
    ("pcp_score_poses", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams), _P, _P, _P,
                                  C.POINTER(VlReport)]),
    ("pcp_generate_and_score", C.c_int, [_P, _P, C.POINTER(VlParams), _P, _P, C.c_uint64,
                                         C.POINTER(C.c_uint64), _P, _P, _P, C.POINTER(VlReport)]),
    ("pcp_raycast_fan", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P, _P, _P,
                                  C.POINTER(C.c_int64)]),
    ("pcp_raycast_fan_stats", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P]),
    ("pcp_raycast_fan_stamps", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P]),
    ("pcp_raycast_fan_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), C.c_int,
                                        C.POINTER(C.c_double)]),
    ("pcp_raycast_fan_keys", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), C.c_uint64,
                                       C.c_uint64, _P, _P, _P]),
    ("pcp_comm_unique_id", C.c_int, [_P]),
    ("pcp_comm_init_rank", C.c_int, [_P, C.c_int, _P, C.c_int]),
    ("pcp_comm_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("pcp_get_runtime_info", C.c_int, [C.POINTER(RuntimeInfo)]),
    ("pcp_raycast_fan_allreduce", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), C.c_uint64,
                                            C.c_uint64, _P, _P, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_double)]),
    ("pcp_score_poses_allreduce", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                            C.c_uint64, C.c_uint64, _P, _P, _P,
                                            C.POINTER(VlReport), C.POINTER(C.c_double)]),
    ("pcp_score_poses_stats", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams), _P]),
    ("pcp_score_matrix", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams), _P, _P]),
    ("pcp_place_sensors", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                    C.POINTER(PlaceParams), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("pcp_place_pair", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                 C.POINTER(PairParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                 _P, _P, _P]),
    ("pcp_place_pair_burst", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                       C.POINTER(PairParams), C.c_int, C.POINTER(C.c_double)]),
    ("pcp_place_triple", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                   C.POINTER(PairParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _P, _P, _P, _P, _P, _P, _P]),
    ("pcp_place_triple_burst", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                         C.POINTER(PairParams), C.c_int, C.POINTER(C.c_double)]),
    ("pcp_place_refine", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                   C.POINTER(RefineParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _P, _P, _P, _P, _P]),
    ("pcp_place_refine_burst", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                         C.POINTER(RefineParams), C.c_int,
                                         C.POINTER(C.c_double)]),
    ("pcp_place_aimed", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                  C.POINTER(AimParams), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _P]),
    ("pcp_place_aimed_burst", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams),
                                        C.POINTER(AimParams), _P, C.c_int,
                                        C.POINTER(C.c_double)]),
    ("pcp_simulate_scan", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P, C.c_uint64,
                                    C.POINTER(C.c_uint64), _P, _P, _P, _P, _P, C.c_uint64,
                                    C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint64)]),
    ("pcp_simulate_scan_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), C.c_int,
                                          _P]),
    ("pcp_raycast_fan_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P, _P, _P, _P,
                                          C.POINTER(C.c_int64)]),
    ("pcp_raycast_fan_mounted_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                C.c_int, C.POINTER(C.c_double)]),
    ("pcp_simulate_scan_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P, _P,
                                            C.c_uint64, C.POINTER(C.c_uint64), _P, _P, _P, _P, _P,
                                            C.c_uint64, C.POINTER(C.c_uint64), _P,
                                            C.POINTER(C.c_uint64)]),
    ("pcp_simulate_scan_mounted_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                  C.c_int, _P]),
    ("pcp_place_coverage", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                     C.POINTER(CoverParams), _P, C.c_uint64, _P, _P, _P, _P, _P,
                                     _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                             C.POINTER(CoverParams), _P, C.c_uint64, _P, _P, _P,
                                             _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                           C.POINTER(CoverParams), _P, C.c_uint64, C.c_int, _P]),
    ("pcp_place_coverage_mounted_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                   C.POINTER(CoverParams), _P, C.c_uint64,
                                                   C.c_int, _P]),
    ("pcp_place_coverage_pair", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                          C.POINTER(PairParams), _P, C.c_uint64, _P,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_uint64), _P, _P, _P, _P, _P, _P,
                                          C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_pair_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                  C.POINTER(PairParams), _P, C.c_uint64, _P,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_uint64), _P, _P, _P, _P, _P, _P,
                                                  C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_pair_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                C.POINTER(PairParams), _P, C.c_uint64, C.c_int,
                                                _P]),
    ("pcp_place_coverage_pair_mounted_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                        _P, C.POINTER(PairParams), _P,
                                                        C.c_uint64, C.c_int, _P]),
    ("pcp_place_coverage_refine", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                            C.POINTER(RefineParams), _P, C.c_uint64, _P,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P, _P,
                                            _P, _P, _P, _P, _P, _P, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_refine_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                    C.POINTER(RefineParams), _P, C.c_uint64, _P,
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                    _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64,
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_refine_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                  C.POINTER(RefineParams), _P, C.c_uint64,
                                                  C.c_int, _P]),
    ("pcp_place_coverage_refine_mounted_burst", C.c_int, [_P, _P, C.c_uint64,
                                                          C.POINTER(FanParams), _P,
                                                          C.POINTER(RefineParams), _P,
                                                          C.c_uint64, C.c_int, _P]),
    ("pcp_place_coverage_aimed", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                           C.POINTER(CoverAimParams), _P, _P, C.c_uint64, _P, _P,
                                           _P, _P, _P, _P, _P, _P, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_aimed_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P,
                                                   C.POINTER(CoverAimParams), _P, _P, C.c_uint64,
                                                   _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64,
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_aimed_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                 C.POINTER(CoverAimParams), _P, _P, C.c_uint64,
                                                 C.c_int, _P]),
    ("pcp_place_coverage_aimed_mounted_burst", C.c_int, [_P, _P, C.c_uint64,
                                                         C.POINTER(FanParams), _P,
                                                         C.POINTER(CoverAimParams), _P, _P,
                                                         C.c_uint64, C.c_int, _P]),
    ("pcp_place_coverage_weighted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                              C.POINTER(CoverParams), _P, C.c_uint64, _P, _P, _P,
                                              _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_weighted_mounted", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                      _P, C.POINTER(CoverParams), _P, C.c_uint64,
                                                      _P, _P, _P, _P, _P, _P, _P, C.c_uint64,
                                                      C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_uint64),
                                                      C.POINTER(C.c_int32)]),
    ("pcp_place_coverage_weighted_burst", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams),
                                                    C.POINTER(CoverParams), _P, C.c_uint64,
                                                    C.c_int, _P]),
    ("pcp_place_coverage_weighted_mounted_burst", C.c_int, [_P, _P, C.c_uint64,
                                                            C.POINTER(FanParams), _P,
                                                            C.POINTER(CoverParams), _P,
                                                            C.c_uint64, C.c_int, _P]),
    ("pcp_debug_exclusive_scan", C.c_int, [_P, _P, C.c_uint64, _P]),
    ("pcp_debug_math", C.c_int, [_P, C.c_int, _P, _P, C.c_uint64, _P, _P]),
    ("pcp_debug_fine_copy", C.c_int, [_P, C.POINTER(FineGeo), _P, C.c_uint64, _P, C.c_uint64, _P,
                                      C.c_uint64]),
    ("pcp_debug_fine_pivot", C.c_int, [_P, C.POINTER(FinePivotGeo), _P, C.c_uint64]),
    ("pcp_debug_fine_band", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), _P,
                                      C.c_uint64]),
    ("pcp_score_poses_burst", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams), C.c_int,
                                        C.POINTER(C.c_double)]),
    ("pcp_stream_create", C.c_int, [_P, C.POINTER(_P)]),
    ("pcp_stream_destroy", C.c_int, [_P, _P]),
    ("pcp_step_table", C.c_int, [C.c_double, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("pcp_terrain_info", C.c_int, [_P, C.POINTER(IndexInfo)]),
    ("pcp_multi_create", C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    ("pcp_multi_destroy", None, [_P]),
    ("pcp_multi_last_error", C.c_char_p, [_P]),
    ("pcp_multi_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("pcp_multi_ctx", _P, [_P, C.c_int]),
    ("pcp_multi_set_terrain", C.c_int, [_P, C.POINTER(CloudView)]),
    ("pcp_multi_set_aux_cloud", C.c_int, [_P, C.POINTER(CloudView)]),
    ("pcp_multi_set_cells", C.c_int, [_P, _P, _P, C.c_uint64]),
    ("pcp_multi_raycast_fan", C.c_int, [_P, _P, C.c_uint64, C.POINTER(FanParams), _P, _P,
                                        C.POINTER(C.c_int64)]),
    ("pcp_multi_score_poses", C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(VlParams), _P, _P,
                                        _P, C.POINTER(VlReport)]),
]
ABI_SYMBOLS = [s[0] for s in _SIGS]

_lib = None


def load_library(path: str | os.PathLike | None = None) -> C.CDLL:
    """Load libpcp.so (raises OSError when it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # PCP_LIB: another build of the same library (A/B timing of kernel variants)
    p = Path(path) if path else Path(os.environ.get("PCP_LIB", LIB_PATH))
    if not p.exists():
        raise OSError(f"libpcp.so not found at {p}: run __graft_entry__.build() "
                      f"(make -C pointcloud_processor_amd/csrc)")
    # RTLD_GLOBAL, and before torch: a PyTorch wheel ships its own libamdhip64.so.7 /
    # librccl.so.1, and whichever copy is loaded first serves every later NEEDED entry of that
    # SONAME.  Loaded first, libpcp runs on the runtime its RUNPATH names (/opt/rocm/lib);
    # runtime_info() reports which one it got.
    lib = C.CDLL(str(p), mode=C.RTLD_GLOBAL)
    for name, res, args in _SIGS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pcp_abi_version() != ABI_VERSION:   # struct layouts of this binding
        raise OSError(f"{p}: ABI version {lib.pcp_abi_version()}, binding expects {ABI_VERSION}: "
                      "rebuild (make -C pointcloud_processor_amd/csrc)")
    if path is None:
        _lib = lib
    return lib


def runtime_info() -> dict:
    """pcp_get_runtime_info: the HIP runtime and RCCL this process's libpcp runs on (versions
    and the files they were loaded from).  No device call."""
    ri = RuntimeInfo()
    rc = load_library().pcp_get_runtime_info(C.byref(ri))
    if rc != PCP_OK:
        raise PcpError(rc, "pcp_get_runtime_info failed")
    hv, rv = ri.hip_runtime_version, ri.rccl_version
    return {"hip_runtime_version": hv,
            "hip_runtime": f"{hv // 10**7}.{hv // 10**5 % 100}.{hv % 10**5}",
            "hip_path": os.path.realpath(ri.hip_path.decode()) if ri.hip_path else None,
            "rccl_version": rv,
            "rccl": f"{rv // 10**4}.{rv // 100 % 100}.{rv % 100}",
            "rccl_path": os.path.realpath(ri.rccl_path.decode()) if ri.rccl_path else None}


def alloc_stats() -> dict:
    """pcp_alloc_stats: the process's device / pinned (re)allocations and their bytes so far
    (every growth of a grow-only buffer counts one)."""
    d, p, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = load_library().pcp_alloc_stats(C.byref(d), C.byref(p), C.byref(b))
    if rc != PCP_OK:
        raise PcpError(rc, "pcp_alloc_stats failed")
    return {"device": d.value, "pinned": p.value, "bytes": b.value}


def device_count() -> int:
    """Visible gfx950 devices (pcp_device_count)."""
    n = C.c_int(0)
    rc = load_library().pcp_device_count(C.byref(n))
    return n.value if rc == PCP_OK else 0


def comm_unique_id() -> bytes:
    """pcp_comm_unique_id: rank 0's 128-byte RCCL id, to be shared with the other ranks out
    of band (bench.py: torch.distributed over gloo) before their comm_init_rank."""
    buf = (C.c_uint8 * 128)()
    rc = load_library().pcp_comm_unique_id(buf)
    if rc != PCP_OK:
        raise PcpError(rc, "pcp_comm_unique_id failed (ncclGetUniqueId)")
    return bytes(buf)


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _poses5(x) -> np.ndarray:
    """poses5 as the ABI reads it: C-contiguous float64 [P, 5]."""
    return np.ascontiguousarray(x, np.float64).reshape(-1, 5)


def _zx5(x) -> np.ndarray:
    """zx120_pose5 as the ABI reads it: C-contiguous float64."""
    return np.ascontiguousarray(x, np.float64)


def cloud_view(arr: np.ndarray, point_step: int | None = None, offs=(0, 4, 8)) -> CloudView:
    """CloudView over a C-contiguous array whose rows are point records.

    float32 (N, k>=3) arrays are read as k*4-byte records with x, y, z first; structured or
    uint8 (N, point_step) arrays must pass point_step and offsets explicitly."""
    if not arr.flags.c_contiguous:
        raise ValueError("cloud array must be C-contiguous")
    n = arr.shape[0] if arr.ndim >= 1 else 0
    if point_step is None:
        if arr.dtype != np.float32 or arr.ndim != 2 or arr.shape[1] < 3:
            raise ValueError("pass point_step for non (N,k) float32 clouds")
        point_step = arr.shape[1] * 4
    return CloudView(arr.ctypes.data if n else None, n, point_step, *offs)


class ExcavationParams(C.Structure):
    """pcp_excavation_params (excavated_surface_generator.cpp:29-51 defaults)."""
    _fields_ = [("depth", C.c_double), ("slope_angle_deg", C.c_double),
                ("offset_x", C.c_double), ("offset_y", C.c_double),
                ("point_density", C.c_double), ("terrain_search_radius", C.c_double),
                ("l_shape_enabled", C.c_int32), ("arm1_length", C.c_double),
                ("arm1_width", C.c_double), ("arm2_length", C.c_double),
                ("arm2_width", C.c_double), ("width", C.c_double), ("length", C.c_double)]


def excavation_params(**kw) -> ExcavationParams:
    p = ExcavationParams(1.0, 75.0, 4.0, 1.0, 0.05, 0.5, 1, 2.0, 1.2, 2.0, 1.2, 1.2, 1.8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class DrivableParams(C.Structure):
    """pcp_drivable_params (calc_drivable_area.cpp:20-26 defaults)."""
    _fields_ = [("grid_resolution", C.c_double), ("map_width", C.c_double),
                ("map_height", C.c_double), ("max_gradient", C.c_double),
                ("min_points_per_cell", C.c_int32), ("start_clear_radius", C.c_double)]


def drivable_params(**kw) -> DrivableParams:
    p = DrivableParams(1.0, 100.0, 100.0, 0.3, 10, 3.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Context:
    """One libpcp context: one HIP device + stream + resident buffers (not thread-safe)."""

    def __init__(self, device: int = 0, lib_path=None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.pcp_create(device, C.byref(h))
        if rc != PCP_OK:
            raise PcpError(rc, f"pcp_create(device={device}) failed (is a gfx950 GPU visible?)")
        self.h = h
        self.device = device
        self._keep = []

    # -- plumbing ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.pcp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != PCP_OK:
            msg = self.lib.pcp_last_error(self.h)
            raise PcpError(rc, f"{what}: {msg.decode() if msg else ''}")

    def synchronize(self):
        self._check(self.lib.pcp_synchronize(self.h), "pcp_synchronize")

    def profile(self, enable: bool = True):
        self._check(self.lib.pcp_profile_enable(self.h, int(enable)), "pcp_profile_enable")

    def profile_reset(self):
        self._check(self.lib.pcp_profile_reset(self.h), "pcp_profile_reset")

    def profile_get(self, kernel: str | int):
        kid = KERNELS.index(kernel) if isinstance(kernel, str) else kernel
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.lib.pcp_profile_get(self.h, kid, C.byref(ms), C.byref(n)),
                    "pcp_profile_get")
        return ms.value, n.value

    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self.lib.pcp_dev_alloc(self.h, nbytes, C.byref(p)), "pcp_dev_alloc")
        return p.value

    def dev_free(self, p: int):
        self._check(self.lib.pcp_dev_free(self.h, p), "pcp_dev_free")

    def h2d(self, dst: int, src: np.ndarray):
        self._check(self.lib.pcp_memcpy_h2d(self.h, dst, _ptr(src), src.nbytes), "h2d")

    def d2h(self, dst: np.ndarray, src: int):
        self._check(self.lib.pcp_memcpy_d2h(self.h, _ptr(dst), src, dst.nbytes), "d2h")

    # -- pointcloud_filter ------------------------------------------------------------------------
    def crop_box(self, cloud: np.ndarray, box, point_step=None, offs=(0, 4, 8)):
        """cropFrontArea: returns (kept_idx uint32, xyz float32 (m,4))."""
        v = cloud_view(cloud, point_step, offs)
        n = v.n
        kept = np.empty(max(n, 1), np.uint32)
        xyz = np.empty((max(n, 1), 4), np.float32)
        box = np.ascontiguousarray(box, np.float64)
        m = C.c_uint64()
        self._check(self.lib.pcp_crop_box(self.h, C.byref(v), _ptr(box), _ptr(kept), _ptr(xyz),
                                          n, C.byref(m)), "pcp_crop_box")
        return kept[: m.value].copy(), xyz[: m.value].copy()

    def voxel_grid(self, cloud: np.ndarray, leaf: float, point_step=None, offs=(0, 4, 8)):
        """pcl::VoxelGrid: returns (xyz (k,4), voxel_idx, voxel_count, passthrough)."""
        v = cloud_view(cloud, point_step, offs)
        n = max(v.n, 1)
        out = np.empty((n, 4), np.float32)
        idx = np.empty(n, np.uint32)
        cnt = np.empty(n, np.uint32)
        k = C.c_uint64()
        pt = C.c_int32()
        self._check(self.lib.pcp_voxel_grid(self.h, C.byref(v), C.c_float(leaf), _ptr(out),
                                            _ptr(idx), _ptr(cnt), n, C.byref(k), C.byref(pt)),
                    "pcp_voxel_grid")
        k = k.value
        return out[:k].copy(), idx[:k].copy(), cnt[:k].copy(), bool(pt.value)

    def crop_voxel(self, cloud: np.ndarray, box, leaf: float, point_step=None, offs=(0, 4, 8)):
        """processCloudSimple: crop then voxel -> (xyz (k,4), n_cropped)."""
        v = cloud_view(cloud, point_step, offs)
        n = max(v.n, 1)
        out = np.empty((n, 4), np.float32)
        box = np.ascontiguousarray(box, np.float64)
        k, nc = C.c_uint64(), C.c_uint64()
        self._check(self.lib.pcp_crop_voxel(self.h, C.byref(v), _ptr(box), C.c_float(leaf),
                                            _ptr(out), n, C.byref(k), C.byref(nc)),
                    "pcp_crop_voxel")
        return out[: k.value].copy(), nc.value

    # -- pointcloud_merger ------------------------------------------------------------------------
    @staticmethod
    def _rigids(tfs):
        arr = (Rigid * max(len(tfs), 1))()
        for i, (t, q) in enumerate(tfs):
            arr[i].t[:] = [float(x) for x in t]
            arr[i].q[:] = [float(x) for x in q]
        return arr

    def transform_concat(self, clouds, tfs, rgbs):
        """processPointClouds/processRobotCloud: -> (N, 8) float32 PointXYZRGB memory image."""
        k = len(clouds)
        views = (CloudView * max(k, 1))(*[cloud_view(c) for c in clouds])
        total = sum(c.shape[0] for c in clouds)
        out = np.empty((max(total, 1), 8), np.float32)
        rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
        n = C.c_uint64()
        self._check(self.lib.pcp_transform_concat(self.h, k, views, self._rigids(tfs), _ptr(rgb),
                                                  _ptr(out), total, C.byref(n)),
                    "pcp_transform_concat")
        return out[: n.value].copy()

    def filter_merge(self, clouds, boxes, leaf, tfs, rgbs, out=None):
        """Host-buffer filter_merge.  ``out`` (optional, float32 [>= total, 8], e.g. a
        host_register-ed array for pinned D2H) receives the merged cloud; a view of it is
        returned in that case, a fresh copy otherwise."""
        k = len(clouds)
        views = (CloudView * max(k, 1))(*[cloud_view(c) for c in clouds])
        total = sum(c.shape[0] for c in clouds)
        own = out is None
        if own:
            out = np.empty((max(total, 1), 8), np.float32)
        elif (out.dtype != np.float32 or out.ndim != 2 or out.shape[1] != 8
              or out.shape[0] < total or not out.flags.c_contiguous):
            raise ValueError("filter_merge: out must be C-contiguous float32 [>= total, 8]")
        rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
        bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1))
        n = C.c_uint64()
        per = np.zeros(max(k, 1), np.uint64)
        self._check(self.lib.pcp_filter_merge(self.h, k, views, _ptr(bx), C.c_float(leaf),
                                              self._rigids(tfs), _ptr(rgb), _ptr(out), total,
                                              C.byref(n), _ptr(per), 0), "pcp_filter_merge")
        res = out[: n.value].copy() if own else out[: n.value]
        return res, per[:k].copy()

    def filter_merge_nodes(self, clouds, boxes, leaf, tfs, rgbs):
        """pcp_filter_merge_nodes: the filter node (every cloud) and the merger node in one call
        -> (merged float32 [n, 8], [each cloud's centroids float32 [n_i, 4]], n_cropped)."""
        k = len(clouds)
        views = (CloudView * max(k, 1))(*[cloud_view(c) for c in clouds])
        total = sum(c.shape[0] for c in clouds)
        out = np.empty((max(total, 1), 8), np.float32)
        filt = [np.empty((max(c.shape[0], 1), 4), np.float32) for c in clouds]
        fptr = (C.c_void_p * max(k, 1))(*[f.ctypes.data for f in filt])
        rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
        bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1))
        n = C.c_uint64()
        per = np.zeros(max(k, 1), np.uint64)
        crop = np.zeros(max(k, 1), np.uint64)
        self._check(self.lib.pcp_filter_merge_nodes(self.h, k, views, _ptr(bx), C.c_float(leaf),
                                                    self._rigids(tfs), _ptr(rgb), _ptr(out),
                                                    total, C.byref(n), _ptr(per), fptr,
                                                    _ptr(crop)), "pcp_filter_merge_nodes")
        return (out[: n.value].copy(), [f[: int(p)].copy() for f, p in zip(filt, per[:k])],
                crop[:k].copy())

    def filter_merge_device(self, views, boxes, leaf, tfs, rgbs, out_dev: int, cap: int):
        """Device-resident pipeline (benchmark): views hold device pointers."""
        k = len(views)
        varr = (CloudView * max(k, 1))(*views)
        rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
        bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1))
        n = C.c_uint64()
        per = np.zeros(max(k, 1), np.uint64)
        self._keep = [rgb, bx]
        self._check(self.lib.pcp_filter_merge(self.h, k, varr, _ptr(bx), C.c_float(leaf),
                                              self._rigids(tfs), _ptr(rgb), out_dev, cap,
                                              C.byref(n), _ptr(per),
                                              PCP_MEM_DEVICE_IN | PCP_MEM_DEVICE_OUT),
                    "pcp_filter_merge")
        return n.value, per[:k].copy()

    def filter_merge_device_prepared(self, views, boxes, leaf, tfs, rgbs, out_dev: int,
                                     cap: int):
        """filter_merge_device with its ctypes arguments built once: returns a call that runs
        one frame and returns (n_out, per_cloud) -- the steady-state frame of a node whose
        clouds land in the same device buffers every time (the library replays its graph)."""
        k = len(views)
        varr = (CloudView * max(k, 1))(*views)
        rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
        bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1))
        rig = self._rigids(tfs)
        n = C.c_uint64()
        per = np.zeros(max(k, 1), np.uint64)
        keep = (varr, rgb, bx, rig, n, per)
        fn, h, lf, nref = self.lib.pcp_filter_merge, self.h, C.c_float(leaf), C.byref(n)
        bxp, rgbp, perp = bx.ctypes.data, rgb.ctypes.data, per.ctypes.data
        flags = PCP_MEM_DEVICE_IN | PCP_MEM_DEVICE_OUT

        def run():
            rc = fn(h, k, varr, bxp, lf, rig, rgbp, out_dev, cap, nref, perp, flags)
            if rc != PCP_OK:
                self._check(rc, "pcp_filter_merge")
            return n.value, per[:k]

        run.keep = keep
        return run

    # -- virtual_lidar ------------------------------------------------------------------------
    def set_terrain(self, cloud: np.ndarray, point_step=None, offs=(0, 4, 8)):
        v = cloud_view(cloud, point_step, offs)
        self._check(self.lib.pcp_set_terrain(self.h, C.byref(v)), "pcp_set_terrain")

    def set_aux_cloud(self, cloud: np.ndarray, point_step=None, offs=(0, 4, 8)):
        v = cloud_view(cloud, point_step, offs)
        self._check(self.lib.pcp_set_aux_cloud(self.h, C.byref(v)), "pcp_set_aux_cloud")

    def set_cells(self, xyz: np.ndarray, normals: np.ndarray):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert xyz.shape == nrm.shape
        self._check(self.lib.pcp_set_cells(self.h, _ptr(xyz), _ptr(nrm), xyz.shape[0]),
                    "pcp_set_cells")
        self.n_cells = xyz.shape[0]

    def set_excavation_area(self, area: np.ndarray, grid_resolution: float = 0.1,
                            vertical_layers: int = 10, point_step=None, offs=(0, 4, 8)):
        """excavationAreaCallback: GPU normals + 3-D cell grid; the cells become the scoring
        cells.  Returns (grid_bbox (6,), n_cells)."""
        v = cloud_view(area, point_step, offs)
        bbox = np.zeros(6, np.float64)
        n = C.c_uint64()
        self._check(self.lib.pcp_set_excavation_area(self.h, C.byref(v), float(grid_resolution),
                                                      int(vertical_layers), _ptr(bbox),
                                                      C.byref(n)), "pcp_set_excavation_area")
        self.n_cells = n.value
        return bbox, n.value

    def set_excavation_area_async(self, area: np.ndarray, grid_resolution: float = 0.1,
                                  vertical_layers: int = 10, point_step=None, offs=(0, 4, 8)):
        """pcp_set_excavation_area_async: the same setup enqueued, not waited for.  Returns
        (grid_bbox (6,), cells_cap): the count is settled by the next call that needs it
        (cells_count(), generate_and_score with a cells_cap-sized flag array, ...)."""
        v = cloud_view(area, point_step, offs)
        bbox = np.zeros(6, np.float64)
        n = C.c_uint64()
        self._check(self.lib.pcp_set_excavation_area_async(
            self.h, C.byref(v), float(grid_resolution), int(vertical_layers), _ptr(bbox),
            C.byref(n)), "pcp_set_excavation_area_async")
        return bbox, n.value   # (the host bytes are copied or staged before the return)

    def cells_count(self) -> int:
        n = C.c_uint64()
        self._check(self.lib.pcp_cells_count(self.h, C.byref(n)), "pcp_cells_count")
        self.n_cells = n.value
        return n.value

    def get_cells(self):
        n = C.c_uint64()
        rc = self.lib.pcp_get_cells(self.h, None, None, 0, C.byref(n))
        if rc not in (PCP_OK, PCP_E_CAPACITY):
            self._check(rc, "pcp_get_cells")
        xyz = np.empty((n.value, 3), np.float64)
        nrm = np.empty((n.value, 3), np.float32)
        self._check(self.lib.pcp_get_cells(self.h, _ptr(xyz), _ptr(nrm), n.value, C.byref(n)),
                    "pcp_get_cells")
        return xyz, nrm

    def get_area_normals(self):
        n = C.c_uint64()
        rc = self.lib.pcp_get_area_normals(self.h, None, 0, C.byref(n))
        if rc not in (PCP_OK, PCP_E_CAPACITY):
            self._check(rc, "pcp_get_area_normals")
        out = np.empty((n.value, 3), np.float32)
        self._check(self.lib.pcp_get_area_normals(self.h, _ptr(out), n.value, C.byref(n)),
                    "pcp_get_area_normals")
        return out

    def excavate(self, cloud: np.ndarray, zx120_tf, params: ExcavationParams | None = None,
                 point_step=None, offs=(0, 4, 8)):
        """matchedCloudCallback: -> (excavated_terrain (N, 8) f32 PointXYZRGB records,
        excavation_area (M, 8) f32, pose (cx, cy, cz, yaw))."""
        v = cloud_view(cloud, point_step, offs)
        p = params or excavation_params()
        tf = Rigid((C.c_double * 3)(*zx120_tf[0]), (C.c_double * 4)(*zx120_tf[1]))
        nt, na = C.c_uint64(), C.c_uint64()
        pose = np.zeros(4, np.float64)
        self._check(self.lib.pcp_excavate_bounds(C.byref(p), v.n, C.byref(nt), C.byref(na)),
                    "pcp_excavate_bounds")
        terr = np.empty((max(nt.value, 1), 8), np.float32)
        area = np.empty((max(na.value, 1), 8), np.float32)
        self._check(self.lib.pcp_excavate(self.h, C.byref(v), C.byref(p), C.byref(tf),
                                          _ptr(terr), terr.shape[0], C.byref(nt), _ptr(area),
                                          area.shape[0], C.byref(na), _ptr(pose)),
                    "pcp_excavate")
        return terr[:nt.value], area[:na.value], pose

    def excavate_area_async(self, cloud: np.ndarray, zx120_tf, params: ExcavationParams | None = None,
                            grid_resolution: float = 0.1, vertical_layers: int = 10,
                            point_step=None, offs=(0, 4, 8), landed: bool = False,
                            zero_copy: bool = False):
        """pcp_excavate_area_async: excavate(), then set_excavation_area_async() over its area
        (when not empty) and set_terrain() over its terrain, fed from the carve's landed
        records.  -> (terrain, area, pose, grid_bbox (6,), cells_cap).  landed=True: null
        outputs, terrain / area read from the landing (pcp_excavate_landed) and returned as
        copies; zero_copy=True (explicit opt-in) returns read-only views of the landing instead,
        valid only until the context's next excavate call or close() (the landing may be
        reallocated or freed then: a view held past that reads freed memory)."""
        v = cloud_view(cloud, point_step, offs)
        p = params or excavation_params()
        tf = Rigid((C.c_double * 3)(*zx120_tf[0]), (C.c_double * 4)(*zx120_tf[1]))
        nt, na, cap = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pose = np.zeros(4, np.float64)
        bbox = np.zeros(6, np.float64)
        if landed:
            self._check(self.lib.pcp_excavate_area_async(
                self.h, C.byref(v), C.byref(p), C.byref(tf), None, 0, C.byref(nt), None, 0,
                C.byref(na), _ptr(pose), float(grid_resolution), int(vertical_layers), _ptr(bbox),
                C.byref(cap)), "pcp_excavate_area_async")
            tp, ap = C.c_void_p(), C.c_void_p()
            self._check(self.lib.pcp_excavate_landed(self.h, C.byref(tp), C.byref(ap)),
                        "pcp_excavate_landed")

            def view(ptr, n):
                if n == 0:
                    return np.empty((0, 8), np.float32)
                a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n, 8))
                if not zero_copy:
                    return a.copy()
                a.flags.writeable = False
                return a
            return view(tp, nt.value), view(ap, na.value), pose, bbox, cap.value
        self._check(self.lib.pcp_excavate_bounds(C.byref(p), v.n, C.byref(nt), C.byref(na)),
                    "pcp_excavate_bounds")
        terr = np.empty((max(nt.value, 1), 8), np.float32)
        area = np.empty((max(na.value, 1), 8), np.float32)
        self._check(self.lib.pcp_excavate_area_async(
            self.h, C.byref(v), C.byref(p), C.byref(tf), _ptr(terr), terr.shape[0], C.byref(nt),
            _ptr(area), area.shape[0], C.byref(na), _ptr(pose), float(grid_resolution),
            int(vertical_layers), _ptr(bbox), C.byref(cap)), "pcp_excavate_area_async")
        return terr[:nt.value], area[:na.value], pose, bbox, cap.value

    def drivable_area(self, cloud: np.ndarray, cloud_to_map, robot_xy, start_xy,
                      params: DrivableParams | None = None, point_step=None, offs=(0, 4, 8)):
        """calc_drivable_area robotCloudCallback -> (grid (h, w) int8, origin (2,))."""
        v = cloud_view(cloud, point_step, offs)
        p = params or drivable_params()
        tf = Rigid((C.c_double * 3)(*cloud_to_map[0]), (C.c_double * 4)(*cloud_to_map[1]))
        gw, gh = int(p.map_width / p.grid_resolution), int(p.map_height / p.grid_resolution)
        grid = np.zeros((max(gh, 1), max(gw, 1)), np.int8)
        dims = np.zeros(2, np.int32)
        origin = np.zeros(2, np.float64)
        self._check(self.lib.pcp_drivable_area(self.h, C.byref(v), C.byref(tf), float(robot_xy[0]),
                                               float(robot_xy[1]), float(start_xy[0]),
                                               float(start_xy[1]), C.byref(p), _ptr(grid),
                                               grid.size, _ptr(dims), _ptr(origin)),
                    "pcp_drivable_area")
        return grid[:dims[1], :dims[0]], origin

    def host_register(self, arr: np.ndarray):
        """Pin a (contiguous) numpy array in place; unregister before it is freed."""
        self._check(self.lib.pcp_host_register(self.h, _ptr(arr), arr.nbytes), "pcp_host_register")

    def host_unregister(self, arr: np.ndarray):
        self._check(self.lib.pcp_host_unregister(self.h, _ptr(arr)), "pcp_host_unregister")

    def terrain_info(self) -> dict:
        info = IndexInfo()
        self._check(self.lib.pcp_terrain_info(self.h, C.byref(info)), "pcp_terrain_info")
        return {"n_points": info.n_points, "cell": info.cell,
                "dims": (info.nx, info.ny, info.nz),
                "bmin": tuple(info.bmin), "bmax": tuple(info.bmax),
                "scan_layout": ("cells", "blocks", "fine")[info.scan_layout],
                "fine_tile": int(info.fine_tile), "fine_pivot": int(info.fine_pivot)}

    def generate_candidates(self, grid_bbox, params: VlParams, zx120_pose5, cap=None):
        bb = np.ascontiguousarray(grid_bbox, np.float64)
        zx = _zx5(zx120_pose5)
        gs = int(np.ceil(np.sqrt(float(params.num_candidates))))
        cap = cap or max(gs * gs, 1)
        out = np.empty((cap, 5), np.float64)
        n = C.c_uint64()
        self._check(self.lib.pcp_generate_candidates(self.h, _ptr(bb), C.byref(params), _ptr(zx),
                                                     _ptr(out), cap, C.byref(n)),
                    "pcp_generate_candidates")
        return out[: n.value].copy()

    def score_poses(self, poses5: np.ndarray, zx120_pose5, params: VlParams,
                    cell_flags: np.ndarray):
        """runOptimization scoring; cell_flags (uint8, n_cells) is updated in place."""
        poses = _poses5(poses5)
        P = poses.shape[0]
        zx = _zx5(zx120_pose5)
        assert cell_flags.dtype == np.uint8 and cell_flags.flags.c_contiguous
        tot = np.empty(max(P, 1), np.float64)
        cov = np.empty(max(P, 1), np.int32)
        rep = VlReport()
        self._check(self.lib.pcp_score_poses(self.h, _ptr(poses), P, _ptr(zx), C.byref(params),
                                             _ptr(cell_flags), _ptr(tot), _ptr(cov),
                                             C.byref(rep)), "pcp_score_poses")
        return tot[:P].copy(), cov[:P].copy(), rep

    def generate_and_score(self, grid_bbox, params: VlParams, zx120_pose5,
                           cell_flags: np.ndarray):
        """runOptimization's device part in one call (pcp_generate_and_score): returns
        (poses [n, 5], totals, covered, report); cell_flags updated in place."""
        bb = np.ascontiguousarray(grid_bbox, np.float64)
        zx = _zx5(zx120_pose5)
        assert cell_flags.dtype == np.uint8 and cell_flags.flags.c_contiguous
        gs = int(np.ceil(np.sqrt(float(params.num_candidates))))
        cap = max(gs * gs, 1)
        poses = np.empty((cap, 5), np.float64)
        tot = np.empty(cap, np.float64)
        cov = np.empty(cap, np.int32)
        n = C.c_uint64()
        rep = VlReport()
        self._check(self.lib.pcp_generate_and_score(self.h, _ptr(bb), C.byref(params), _ptr(zx),
                                                    _ptr(poses), cap, C.byref(n),
                                                    _ptr(cell_flags), _ptr(tot), _ptr(cov),
                                                    C.byref(rep)), "pcp_generate_and_score")
        P = n.value
        return poses[:P].copy(), tot[:P].copy(), cov[:P].copy(), rep

    def score_poses_into(self, poses5: np.ndarray, zx120_pose5: np.ndarray, params: VlParams,
                         cell_flags: np.ndarray, tot: np.ndarray, cov: np.ndarray,
                         rep: "VlReport"):
        """score_poses into caller-owned arrays (steady-state query, no allocation): poses5
        C-contiguous float64 [P, 5], zx120_pose5 float64 [5], tot float64 [>=P], cov int32
        [>=P]; cell_flags updated in place."""
        P = poses5.shape[0]
        if (poses5.dtype != np.float64 or not poses5.flags.c_contiguous or poses5.ndim != 2
                or zx120_pose5.dtype != np.float64 or not zx120_pose5.flags.c_contiguous
                or cell_flags.dtype != np.uint8 or not cell_flags.flags.c_contiguous
                or tot.dtype != np.float64 or cov.dtype != np.int32
                or tot.shape[0] < P or cov.shape[0] < P):
            raise ValueError("score_poses_into: bad array types or sizes")
        self._check(self.lib.pcp_score_poses(self.h, poses5.ctypes.data, P,
                                             zx120_pose5.ctypes.data, C.byref(params),
                                             cell_flags.ctypes.data, tot.ctypes.data,
                                             cov.ctypes.data, C.byref(rep)), "pcp_score_poses")

    def raycast_fan_into(self, poses5: np.ndarray, fan: FanParams, blocked: np.ndarray,
                         units: np.ndarray) -> int:
        """raycast_fan into caller-owned arrays (no allocation per call: the benchmark's and a
        node's steady-state query); poses5 C-contiguous float64 [P, 5], blocked uint32 [P],
        units uint64 [P].  Returns the best (fewest blocked, lowest) pose index."""
        P = poses5.shape[0]
        if (poses5.dtype != np.float64 or not poses5.flags.c_contiguous or poses5.ndim != 2
                or poses5.shape[1] != 5 or blocked.dtype != np.uint32 or units.dtype != np.uint64
                or blocked.shape[0] < P or units.shape[0] < P):
            raise ValueError("raycast_fan_into: poses float64 [P,5], blocked u32 [>=P], units u64 [>=P]")
        best = C.c_int64()
        self._check(self.lib.pcp_raycast_fan(self.h, poses5.ctypes.data, P, C.byref(fan),
                                             blocked.ctypes.data, units.ctypes.data, None,
                                             C.byref(best)), "pcp_raycast_fan")
        return best.value

    def raycast_fan_keys(self, poses5: np.ndarray, fan: FanParams, lo: int, p_total: int,
                         keys_dev_ptr: int, units_dev_ptr: int | None = None,
                         wait_stream: int | None = None):
        """pcp_raycast_fan_keys: this rank's poses [lo, lo + P) of p_total as int64 keys
        (blocked << 32) | pose in the DEVICE buffer at keys_dev_ptr (p_total entries, INT64_MAX
        in other ranks' slots), e.g. a torch int64 tensor's data_ptr(); wait_stream: a
        hipStream_t of libpcp's OWN HIP runtime made to wait for the keys, or None (the call
        returns once they are written) -- never a torch stream handle (the wheel's runtime)."""
        P = poses5.shape[0]
        if (poses5.dtype != np.float64 or not poses5.flags.c_contiguous or poses5.ndim != 2
                or poses5.shape[1] != 5):
            raise ValueError("raycast_fan_keys: poses float64 [P, 5]")
        self._check(self.lib.pcp_raycast_fan_keys(self.h, poses5.ctypes.data, P, C.byref(fan),
                                                  lo, p_total, keys_dev_ptr, units_dev_ptr,
                                                  wait_stream), "pcp_raycast_fan_keys")

    def stream_create(self) -> int:
        """A second HIP stream of libpcp's own runtime on this context's device (a wait_stream
        for raycast_fan_keys); release with stream_destroy."""
        h = C.c_void_p()
        self._check(self.lib.pcp_stream_create(self.h, C.byref(h)), "pcp_stream_create")
        return h.value

    def stream_destroy(self, stream: int):
        self._check(self.lib.pcp_stream_destroy(self.h, stream), "pcp_stream_destroy")

    def comm_init_rank(self, nranks: int, uid: bytes, rank: int):
        """pcp_comm_init_rank: this context's own RCCL communicator (one process per GPU)."""
        if len(uid) != 128:
            raise ValueError("comm_init_rank: the id is 128 bytes (comm_unique_id)")
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.pcp_comm_init_rank(self.h, nranks, buf, rank), "pcp_comm_init_rank")

    def comm_info(self):
        n, r = C.c_int(), C.c_int()
        self._check(self.lib.pcp_comm_info(self.h, C.byref(n), C.byref(r)), "pcp_comm_info")
        return n.value, r.value

    def raycast_fan_allreduce(self, poses5: np.ndarray, fan: FanParams, lo: int, p_total: int,
                              blocked_all: np.ndarray | None = None,
                              units: np.ndarray | None = None, timed: bool = False):
        """pcp_raycast_fan_allreduce: this rank's poses [lo, lo + P) of p_total, the keys
        reduced by libpcp's own RCCL communicator (comm_init_rank).  blocked_all (uint32
        [p_total]) / units (uint64 [P]) are filled when given.  -> (best index, collective ms
        or None)."""
        P = poses5.shape[0]
        if (poses5.dtype != np.float64 or not poses5.flags.c_contiguous or poses5.ndim != 2
                or poses5.shape[1] != 5):
            raise ValueError("raycast_fan_allreduce: poses float64 [P, 5]")
        if blocked_all is not None and (blocked_all.dtype != np.uint32 or
                                        blocked_all.shape[0] < p_total):
            raise ValueError("raycast_fan_allreduce: blocked_all uint32 [>= p_total]")
        if units is not None and (units.dtype != np.uint64 or units.shape[0] < P):
            raise ValueError("raycast_fan_allreduce: units uint64 [>= P]")
        best = C.c_int64()
        ms = C.c_double()
        self._check(self.lib.pcp_raycast_fan_allreduce(
            self.h, poses5.ctypes.data if P else None, P, C.byref(fan), lo, p_total,
            _ptr(blocked_all), _ptr(units), C.byref(best), C.byref(ms) if timed else None),
            "pcp_raycast_fan_allreduce")
        return best.value, (ms.value if timed else None)

    def debug_exclusive_scan(self, a: np.ndarray) -> np.ndarray:
        """pcp_debug_exclusive_scan: the device exclusive scan of uint32 `a` -> (n + 1,)."""
        a = np.ascontiguousarray(a, np.uint32)
        out = np.zeros(a.size + 1, np.uint32)
        self._check(self.lib.pcp_debug_exclusive_scan(self.h, _ptr(a), a.size, _ptr(out)),
                    "pcp_debug_exclusive_scan")
        return out

    def debug_math(self, op: int, a: np.ndarray, b: np.ndarray | None = None):
        """pcp_debug_math: op (MATH_*) element-wise on the device through the production device
        functions.  float64 ops take float64 arrays, the float libm ops and MATH_NORMAL (a: (n, 9)
        covariances, b: (n, 3) query points -> (n, 3)) float32; MATH_F64_FMA takes b (n, 2).
        Returns out, or (out, phase int32) for MATH_SCORE_SIN_PART."""
        f32 = op in (MATH_ATAN2F, MATH_SINF, MATH_COSF, MATH_DIVF, MATH_SQRTF, MATH_NORMAL)
        dt = np.float32 if f32 else np.float64
        a = np.ascontiguousarray(a, dt)
        n = a.shape[0]
        if b is not None:
            b = np.ascontiguousarray(b, dt)
            if b.shape[0] != n:
                raise ValueError("debug_math: a and b differ in length")
        if op == MATH_NORMAL and (a.shape != (n, 9) or b is None or b.shape != (n, 3)):
            raise ValueError("debug_math: MATH_NORMAL takes a (n, 9) and b (n, 3)")
        if op == MATH_F64_FMA and (b is None or b.shape != (n, 2)):
            raise ValueError("debug_math: MATH_F64_FMA takes b (n, 2)")
        out = np.zeros((n, 3) if op == MATH_NORMAL else n,
                       np.float32 if f32 or op == MATH_F64_TO_F32 else np.float64)
        aux = np.zeros(n, np.int32) if op == MATH_SCORE_SIN_PART else None
        self._check(self.lib.pcp_debug_math(self.h, op, _ptr(a), _ptr(b), n, _ptr(out), _ptr(aux)),
                    "pcp_debug_math")
        return (out, aux) if aux is not None else out

    def debug_fine_copy(self):
        """pcp_debug_fine_copy: the terrain's fine-window copy as built -> (geo dict, frec uint8,
        wpts uint8, pts float32 (n, 4)), raw device bytes; the arrays are None and geo["built"]
        is 0 when the copy is not built."""
        geo = FineGeo()
        self._check(self.lib.pcp_debug_fine_copy(self.h, C.byref(geo), None, 0, None, 0, None, 0),
                    "pcp_debug_fine_copy")
        d = {k: getattr(geo, k) for k, _ in geo._fields_}
        if not geo.built:
            return d, None, None, None
        frec = np.zeros(geo.frec_bytes, np.uint8)
        wpts = np.zeros(geo.wpts_bytes, np.uint8)
        pts = np.zeros((geo.n_points, 4), np.float32)
        self._check(self.lib.pcp_debug_fine_copy(self.h, C.byref(geo), _ptr(frec), frec.nbytes,
                                                 _ptr(wpts), wpts.nbytes, _ptr(pts), pts.nbytes),
                    "pcp_debug_fine_copy")
        return d, frec, wpts, pts

    def debug_fine_pivot(self):
        """pcp_debug_fine_pivot: the fine copy's pivot table as built -> (geo dict, float32
        (n_slots, 3) records in tile order); (geo, None) with geo["built"] 0 when there is none."""
        geo = FinePivotGeo()
        self._check(self.lib.pcp_debug_fine_pivot(self.h, C.byref(geo), None, 0),
                    "pcp_debug_fine_pivot")
        d = {k: getattr(geo, k) for k, _ in geo._fields_}
        if not geo.built:
            return d, None
        piv = np.zeros((geo.n_slots, 3), np.float32)
        self._check(self.lib.pcp_debug_fine_pivot(self.h, C.byref(geo), _ptr(piv), piv.nbytes),
                    "pcp_debug_fine_pivot")
        return d, piv

    def debug_fine_band(self):
        """pcp_debug_fine_band: the tight twin of the split records' thresholds as built ->
        (enabled, uint16 array, one word lo | hi << 8 per record slot in the threshold array's
        layout); (enabled, None) when there is no twin."""
        nbytes, enabled = C.c_uint64(), C.c_int32()
        self._check(self.lib.pcp_debug_fine_band(self.h, C.byref(nbytes), C.byref(enabled), None, 0),
                    "pcp_debug_fine_band")
        if not nbytes.value:
            return int(enabled.value), None
        band = np.zeros(nbytes.value // 2, np.uint16)
        self._check(self.lib.pcp_debug_fine_band(self.h, C.byref(nbytes), C.byref(enabled),
                                                 _ptr(band), band.nbytes), "pcp_debug_fine_band")
        return int(enabled.value), band

    def score_matrix(self, poses5, zx120_pose5, params: VlParams):
        """pcp_score_matrix -> (score_mobile [P, C], score_zx120 [C]): evaluateCellScore per
        (pose, cell) as k_score_cells computes it (the per-cell parity bar)."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        C_ = self.cells_count()
        P = poses.shape[0]
        sm = np.zeros((max(P, 1), max(C_, 1)), np.float64)
        sz = np.zeros(max(C_, 1), np.float64)
        self._check(self.lib.pcp_score_matrix(self.h, _ptr(poses), P, _ptr(zx), C.byref(params),
                                              _ptr(sm), _ptr(sz)), "pcp_score_matrix")
        return sm[:P, :C_].copy(), sz[:C_].copy()

    def _cell_buffers(self, want_cells: bool):
        """(n_cells, cell_score, cell_owner) for a placement call: its buffers when wanted."""
        if not want_cells:
            return 0, None, None
        n = self.cells_count()
        return n, np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.int32)

    @staticmethod
    def _cells_out(out: dict, cells) -> dict:
        """out with the call's cell_score / cell_owner [n_cells], where _cell_buffers made them."""
        n, cs, co = cells
        if cs is not None:
            out["cell_score"] = cs[:n].copy()
            out["cell_owner"] = co[:n].copy()
        return out

    def _place_burst(self, symbol: str, poses5, zx120_pose5, params: VlParams, call_params,
                     reps: int, *extra) -> float:
        """A placement call's timing entry point -> its ms per repetition; extra: what the call
        takes between its parameters and reps."""
        poses, zx = _poses5(poses5), _zx5(zx120_pose5)
        ms = C.c_double(0.0)
        self._check(getattr(self.lib, symbol)(self.h, _ptr(poses), poses.shape[0], _ptr(zx),
                                              C.byref(params), C.byref(call_params), *extra,
                                              int(reps), C.byref(ms)), symbol)
        return ms.value

    def place_sensors(self, poses5, zx120_pose5, params: VlParams, k_max: int,
                      min_separation: float = 0.0, want_round_totals: bool = False,
                      want_cells: bool = False, reserved: int = 0) -> dict:
        """pcp_place_sensors: up to k_max of the poses placed greedily (a cell's combined score
        is the max over zx120 and the placed sensors; each round takes the pose with the highest
        ordered total while it adds anything).  -> dict: n_selected, selected / total_after /
        covered_after [n_selected], zx120_total, zx120_covered, and on request round_totals
        [n_selected, P] (-inf at poses out of the search), cell_score / cell_owner [n_cells]."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        P = poses.shape[0]
        pp = PlaceParams(int(k_max), int(reserved), float(min_separation))
        kk = max(min(int(k_max), PLACE_MAX), 1)
        sel = np.full(kk, -1, np.int64)
        tot = np.zeros(kk, np.float64)
        cov = np.zeros(kk, np.int32)
        rt = np.zeros((kk, max(P, 1)), np.float64) if want_round_totals else None
        cells = _, cs, co = self._cell_buffers(want_cells)
        zt, zc, ns = C.c_double(), C.c_int32(), C.c_int32()
        self._check(self.lib.pcp_place_sensors(self.h, _ptr(poses) if P else None, P, _ptr(zx),
                                               C.byref(params), C.byref(pp), _ptr(sel), _ptr(tot),
                                               _ptr(cov), _ptr(rt), _ptr(cs), _ptr(co),
                                               C.byref(zt), C.byref(zc), C.byref(ns)),
                    "pcp_place_sensors")
        n = ns.value
        out = {"n_selected": n, "selected": sel[:n].copy(), "total_after": tot[:n].copy(),
               "covered_after": cov[:n].copy(), "zx120_total": zt.value,
               "zx120_covered": zc.value}
        if want_round_totals:
            out["round_totals"] = rt[:n, :P].copy()
        return self._cells_out(out, cells)

    @staticmethod
    def _pair_params(fixed, min_separation, reserved, n_fixed=None) -> PairParams:
        fixed = [int(f) for f in fixed]
        pp = PairParams(len(fixed) if n_fixed is None else int(n_fixed), int(reserved),
                        float(min_separation))
        for i, f in enumerate(fixed[:PLACE_MAX]):
            pp.fixed[i] = f
        return pp

    def place_pair(self, poses5, zx120_pose5, params: VlParams, fixed=(),
                   min_separation: float = 0.0, want_pair_totals: bool = False,
                   want_single_totals: bool = False, want_cells: bool = False,
                   reserved: int = 0) -> dict:
        """pcp_place_pair: the exact best pair of the poses beside zx120 and the `fixed` poses
        (every admissible pair a < b evaluated; the first maximum in row-major order), with the
        best single pose and the base for comparison.  -> dict: n_selected (2: the pair beats the
        single, 1: only the single adds, 0), best_pair (2,), pair_total, pair_covered,
        best_single, single_total, single_covered, base_total, base_covered, and on request
        pair_totals [P, P] (-inf off the admissible upper triangle), single_totals [P],
        cell_score / cell_owner [n_cells] of the answer."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        P = poses.shape[0]
        pp = self._pair_params(fixed, min_separation, reserved)
        bp = np.full(2, -1, np.int64)
        pt, st, bt = C.c_double(), C.c_double(), C.c_double()
        pc, sc, bc, ns = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        bs = C.c_int64(-1)
        dense = P <= PAIR_MAX_POSES   # (a refused call writes nothing: no table for it)
        tab = np.zeros((max(P, 1), max(P, 1)), np.float64) if want_pair_totals and dense else None
        sg = np.zeros(max(P, 1), np.float64) if want_single_totals else None
        cells = _, cs, co = self._cell_buffers(want_cells)
        self._check(self.lib.pcp_place_pair(
            self.h, _ptr(poses) if P else None, P, _ptr(zx), C.byref(params), C.byref(pp),
            _ptr(bp), C.byref(pt), C.byref(pc), C.byref(bs), C.byref(st), C.byref(sc),
            C.byref(bt), C.byref(bc), _ptr(tab), _ptr(sg), _ptr(cs), _ptr(co), C.byref(ns)),
            "pcp_place_pair")
        out = {"n_selected": ns.value, "best_pair": bp, "pair_total": pt.value,
               "pair_covered": pc.value, "best_single": bs.value, "single_total": st.value,
               "single_covered": sc.value, "base_total": bt.value, "base_covered": bc.value}
        if want_pair_totals:
            out["pair_totals"] = tab[:P, :P].copy()
        if want_single_totals:
            out["single_totals"] = sg[:P].copy()
        return self._cells_out(out, cells)

    def place_pair_burst(self, poses5, zx120_pose5, params: VlParams, fixed=(),
                         min_separation: float = 0.0, reps: int = 20) -> float:
        """pcp_place_pair_burst -> ms per repetition of the pair phase (preparation, pair tiles,
        selection; the scoring once before the interval)."""
        return self._place_burst("pcp_place_pair_burst", poses5, zx120_pose5, params,
                                 self._pair_params(fixed, min_separation, 0), reps)

    @staticmethod
    def _aim_params(k_max, n_aims, h_fov, v_fov, fixed, min_separation, reserved,
                    n_fixed=None) -> AimParams:
        fixed = [(int(p), int(a)) for p, a in fixed]
        ap = AimParams(int(k_max), int(n_aims), len(fixed) if n_fixed is None else int(n_fixed),
                       int(reserved), float(h_fov), float(v_fov), float(min_separation))
        for i, (p, a) in enumerate(fixed[:PLACE_MAX]):
            ap.fixed_pose[i] = p
            ap.fixed_aim[i] = a
        return ap

    def place_aimed(self, poses5, zx120_pose5, params: VlParams, aims, h_fov: float,
                    v_fov: float, k_max: int, fixed=(), min_separation: float = 0.0,
                    want_round_totals: bool = False, want_cells: bool = False,
                    reserved: int = 0) -> dict:
        """pcp_place_aimed: up to k_max sensors with a field of view of h_fov x v_fov (full
        angles, radians) placed greedily, every pose searched with every aim of `aims` [A, 2] (yaw
        offset, pitch) beside zx120 and the `fixed` (pose, aim) pairs.  -> dict: n_selected,
        selected / selected_aim / total_after / covered_after [n_selected], base_total,
        base_covered, and on request round_totals [n_selected, P, A] (-inf at poses out of the
        search), cell_score / cell_owner [n_cells]."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        aims = np.ascontiguousarray(aims, np.float64).reshape(-1, 2)
        P, A = poses.shape[0], aims.shape[0]
        ap = self._aim_params(k_max, A, h_fov, v_fov, fixed, min_separation, reserved)
        kk = max(min(int(k_max), PLACE_MAX), 1)
        sel = np.full(kk, -1, np.int64)
        sa = np.full(kk, -1, np.int32)
        tot = np.zeros(kk, np.float64)
        cov = np.zeros(kk, np.int32)
        fits = P <= PAIR_MAX_POSES and P * A <= AIM_MAX_ROWS   # (a refused call writes nothing)
        rt = np.zeros((kk, max(P, 1), max(A, 1)), np.float64) \
            if want_round_totals and fits else None
        cells = _, cs, co = self._cell_buffers(want_cells)
        bt, bc, ns = C.c_double(), C.c_int32(), C.c_int32()
        self._check(self.lib.pcp_place_aimed(
            self.h, _ptr(poses) if P else None, P, _ptr(zx), C.byref(params), C.byref(ap),
            _ptr(aims) if A else None, _ptr(sel), _ptr(sa), _ptr(tot), _ptr(cov), _ptr(rt),
            _ptr(cs), _ptr(co), C.byref(bt), C.byref(bc), C.byref(ns)), "pcp_place_aimed")
        n = ns.value
        out = {"n_selected": n, "selected": sel[:n].copy(), "selected_aim": sa[:n].copy(),
               "total_after": tot[:n].copy(), "covered_after": cov[:n].copy(),
               "base_total": bt.value, "base_covered": bc.value}
        if want_round_totals:
            out["round_totals"] = rt[:n, :P, :A].copy()
        return self._cells_out(out, cells)

    def place_aimed_burst(self, poses5, zx120_pose5, params: VlParams, aims, h_fov: float,
                          v_fov: float, fixed=(), min_separation: float = 0.0,
                          reps: int = 20) -> float:
        """pcp_place_aimed_burst -> ms per round of the aimed placement (round 0's launch: every
        (pose, aim) row's total and the last block's selection; the scoring, the tables and the
        base once before the interval)."""
        aims = np.ascontiguousarray(aims, np.float64).reshape(-1, 2)
        ap = self._aim_params(1, aims.shape[0], h_fov, v_fov, fixed, min_separation, 0)
        return self._place_burst("pcp_place_aimed_burst", poses5, zx120_pose5, params, ap, reps,
                                 _ptr(aims))

    def place_triple(self, poses5, zx120_pose5, params: VlParams, fixed=(),
                     min_separation: float = 0.0, want_first: bool = False,
                     want_triple_totals: bool = False, want_cells: bool = False,
                     reserved: int = 0) -> dict:
        """pcp_place_triple: the exact best triple of the poses beside zx120 and the `fixed` poses
        (every admissible triple a < b < c evaluated; the lexicographically first maximum), with
        the best pair, the best single pose and the base for comparison.  -> dict: n_selected (3:
        the triple beats the pair, the single and the base; 2, 1, 0 as place_pair), best_triple
        (3,), triple_total, triple_covered, best_pair (2,), pair_total, pair_covered, best_single,
        single_total, single_covered, base_total, base_covered, and on request first_totals [P] /
        first_partners [P, 2] (the best (b, c) of every first sensor a), triple_totals [P, P, P]
        (-inf off the admissible a < b < c; P <= TRIPLE_TABLE_MAX_POSES), cell_score /
        cell_owner [n_cells] of the answer."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        P = poses.shape[0]
        pp = self._pair_params(fixed, min_separation, reserved)
        bt3, bp = np.full(3, -1, np.int64), np.full(2, -1, np.int64)
        tt, pt, st, bt = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        tc, pc, sc, bc, ns = (C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32())
        bs = C.c_int64(-1)
        n1 = max(P, 1) if P <= TRIPLE_MAX_POSES else 1   # (a refused call writes nothing)
        ft = np.zeros(n1, np.float64) if want_first else None
        fp = np.zeros((n1, 2), np.int64) if want_first else None
        # (past the table's limit the call is refused: one entry stands for the argument)
        nt = max(P, 1) if P <= TRIPLE_TABLE_MAX_POSES else 1
        tab = np.zeros((nt, nt, nt), np.float64) if want_triple_totals else None
        cells = _, cs, co = self._cell_buffers(want_cells)
        self._check(self.lib.pcp_place_triple(
            self.h, _ptr(poses) if P else None, P, _ptr(zx), C.byref(params), C.byref(pp),
            _ptr(bt3), C.byref(tt), C.byref(tc), _ptr(bp), C.byref(pt), C.byref(pc),
            C.byref(bs), C.byref(st), C.byref(sc), C.byref(bt), C.byref(bc), _ptr(ft), _ptr(fp),
            _ptr(tab), _ptr(cs), _ptr(co), C.byref(ns)), "pcp_place_triple")
        out = {"n_selected": ns.value, "best_triple": bt3, "triple_total": tt.value,
               "triple_covered": tc.value, "best_pair": bp, "pair_total": pt.value,
               "pair_covered": pc.value, "best_single": bs.value, "single_total": st.value,
               "single_covered": sc.value, "base_total": bt.value, "base_covered": bc.value}
        if want_first:
            out["first_totals"] = ft[:P].copy()
            out["first_partners"] = fp[:P].copy()
        if want_triple_totals:
            out["triple_totals"] = tab[:P, :P, :P].copy()
        return self._cells_out(out, cells)

    def place_triple_burst(self, poses5, zx120_pose5, params: VlParams, fixed=(),
                           min_separation: float = 0.0, reps: int = 20) -> float:
        """pcp_place_triple_burst -> ms per repetition of the triple phase (the pair phase it
        builds on, the triple tiles, the rows' maxima and the selection; the scoring once before
        the interval)."""
        return self._place_burst("pcp_place_triple_burst", poses5, zx120_pose5, params,
                                 self._pair_params(fixed, min_separation, 0), reps)

    @staticmethod
    def _refine_params(start, n_locked, max_moves, min_separation, reserved,
                       k=None) -> RefineParams:
        start = [int(f) for f in start]
        rp = RefineParams(len(start) if k is None else int(k), int(n_locked), int(max_moves),
                          int(reserved), float(min_separation))
        for i, f in enumerate(start[:PLACE_MAX]):
            rp.start[i] = f
        return rp

    def place_refine(self, poses5, zx120_pose5, params: VlParams, start, n_locked: int = 0,
                     max_moves: int = REFINE_MAX_MOVES, min_separation: float = 0.0,
                     want_swap_totals: bool = False, want_cells: bool = False,
                     reserved: int = 0) -> dict:
        """pcp_place_refine: the set `start` of poses improved by single-sensor exchanges (every
        unlocked sensor tried at every other pose with the rest held; the best exchange taken
        while it raises the total).  -> dict: selected [k], total, covered, start_total,
        start_covered, n_moves, converged (1: no single move raises the total; 0: max_moves ran
        out first), move_slot / move_from / move_to / move_total / move_covered [n_moves], and on
        request swap_totals [n_moves + 1, k, P] (-inf at inadmissible moves), cell_score /
        cell_owner [n_cells] of the refined set."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        P = poses.shape[0]
        rp = self._refine_params(start, n_locked, max_moves, min_separation, reserved)
        k = max(min(rp.k, PLACE_MAX), 1)
        mm = max(min(int(max_moves), REFINE_MAX_MOVES), 0)
        sel = np.full(k, -1, np.int64)
        tot, st = C.c_double(), C.c_double()
        cov, sc, nm, cv = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        m_slot = np.zeros(max(mm, 1), np.int32)
        m_from = np.zeros(max(mm, 1), np.int64)
        m_to = np.zeros(max(mm, 1), np.int64)
        m_tot = np.zeros(max(mm, 1), np.float64)
        m_cov = np.zeros(max(mm, 1), np.int32)
        dense = P <= PAIR_MAX_POSES   # (a refused call writes nothing: no table for it)
        tab = (np.zeros((mm + 1, k, max(P, 1)), np.float64)
               if want_swap_totals and dense else None)
        cells = _, cs, co = self._cell_buffers(want_cells)
        self._check(self.lib.pcp_place_refine(
            self.h, _ptr(poses), P, _ptr(zx), C.byref(params), C.byref(rp), _ptr(sel),
            C.byref(tot), C.byref(cov), C.byref(st), C.byref(sc), _ptr(m_slot), _ptr(m_from),
            _ptr(m_to), _ptr(m_tot), _ptr(m_cov), _ptr(tab), _ptr(cs), _ptr(co), C.byref(nm),
            C.byref(cv)), "pcp_place_refine")
        n = nm.value
        out = {"selected": sel, "total": tot.value, "covered": cov.value,
               "start_total": st.value, "start_covered": sc.value, "n_moves": n,
               "converged": cv.value, "move_slot": m_slot[:n].copy(),
               "move_from": m_from[:n].copy(), "move_to": m_to[:n].copy(),
               "move_total": m_tot[:n].copy(), "move_covered": m_cov[:n].copy()}
        if want_swap_totals:
            # (without cells nothing is evaluated: no table)
            out["swap_totals"] = tab[:n + 1 if self.cells_count() else 0, :, :P].copy()
        return self._cells_out(out, cells)

    def place_refine_burst(self, poses5, zx120_pose5, params: VlParams, start, n_locked: int = 0,
                           min_separation: float = 0.0, reps: int = 20) -> float:
        """pcp_place_refine_burst -> ms per evaluation of the start set (preparation and
        evaluation launches; the scoring and the setup once before the interval)."""
        return self._place_burst("pcp_place_refine_burst", poses5, zx120_pose5, params,
                                 self._refine_params(start, n_locked, 0, min_separation, 0), reps)

    def simulate_scan(self, poses5, fan: FanParams, want_dense: bool = False,
                      want_mask: bool = True, returns_cap: int | None = None,
                      mask_cap: int | None = None, _mounted=None) -> dict:
        """pcp_simulate_scan: the fan of up to SCAN_MAX_POSES poses with every blocked ray
        resolved to the terrain point it hit.  -> dict: returns (SCAN_RETURN_DTYPE, the poses'
        segments in ray order), offsets [P + 1], n_points, hit_point / range / first_hit
        [P, n_el, n_az] (want_dense, else None), point_mask uint64 [n_points] / seen_points [P] /
        n_seen_any (want_mask, else None).  returns_cap None: n * n_az * n_el; mask_cap None: the
        terrain cloud's size.  A short capacity raises PcpError(PCP_E_CAPACITY) whose `partial`
        attribute holds the same dict (counts, offsets and dense outputs valid)."""
        # (_mounted: simulate_scan_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_simulate_scan_mounted" if _mounted else "pcp_simulate_scan"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        P = poses.shape[0]
        rays = int(fan.n_az) * int(fan.n_el)
        cap = P * rays if returns_cap is None else int(returns_cap)
        ret = np.zeros(max(cap, 1), SCAN_RETURN_DTYPE)
        offsets = np.zeros(P + 1, np.uint64)
        shape = (P, fan.n_el, fan.n_az)
        hp = np.empty(shape, np.int32) if want_dense else None
        rg = np.empty(shape, np.float32) if want_dense else None
        fh = np.empty(shape, np.int16) if want_dense else None
        mcap = 0
        if want_mask:
            mcap = self.scan_points() if mask_cap is None else int(mask_cap)
        mask = np.zeros(max(mcap, 1), np.uint64) if want_mask else None
        seen = np.zeros(max(P, 1), np.uint32) if want_mask else None
        nret, npts, nany = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = fn(
            self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, _ptr(ret), cap,
            C.byref(nret),
            _ptr(offsets), _ptr(hp), _ptr(rg), _ptr(fh), _ptr(mask), mcap, C.byref(npts),
            _ptr(seen), C.byref(nany) if want_mask else None)
        if rc not in (PCP_OK, PCP_E_CAPACITY):
            self._check(rc, what)
        N = npts.value
        # (views of the call's own arrays: no second copy of a scan's tens of megabytes)
        out = {"returns": ret[:min(nret.value, cap)], "n_returns": nret.value,
               "offsets": offsets, "n_points": N, "hit_point": hp, "range": rg, "first_hit": fh,
               "point_mask": mask[:min(N, mcap)] if want_mask else None,
               "seen_points": seen[:P] if want_mask else None,
               "n_seen_any": nany.value if want_mask else None}
        if rc == PCP_E_CAPACITY:
            try:
                self._check(rc, what)
            except PcpError as e:
                e.partial = out
                raise
        return out

    @staticmethod
    def _el_table(fan: FanParams, el_table):
        if el_table is None:
            return None
        t = np.ascontiguousarray(el_table, np.float64).reshape(-1)
        if t.shape[0] != int(fan.n_el):
            raise ValueError(f"el_table: {t.shape[0]} entries for n_el = {int(fan.n_el)}")
        return t

    def simulate_scan_mounted(self, poses6, fan: FanParams, el_table=None,
                              want_dense: bool = False, want_mask: bool = True,
                              returns_cap: int | None = None,
                              mask_cap: int | None = None) -> dict:
        """pcp_simulate_scan_mounted: simulate_scan from tilted mounts -- poses6 rows x, y, z,
        roll, pitch, yaw (pitch negative looks down) -- with an optional beam table el_table
        [n_el] in radians.  -> simulate_scan's dict."""
        return self.simulate_scan(poses6, fan, want_dense, want_mask, returns_cap, mask_cap,
                                  _mounted=(self._el_table(fan, el_table),))

    def raycast_fan_mounted(self, poses6, fan: FanParams, el_table=None, want_first_hit=False):
        """pcp_raycast_fan_mounted -> raycast_fan's (blocked, units, first_hit, best_idx) for
        poses6 rows x, y, z, roll, pitch, yaw and an optional beam table [n_el] (radians)."""
        poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
        tab = self._el_table(fan, el_table)
        P = poses.shape[0]
        blocked = np.zeros(max(P, 1), np.uint32)
        units = np.zeros(max(P, 1), np.uint64)
        fh = np.empty((P, fan.n_el, fan.n_az), np.int16) if want_first_hit else None
        best = C.c_int64()
        self._check(self.lib.pcp_raycast_fan_mounted(self.h, _ptr(poses), P, C.byref(fan),
                                                     _ptr(tab), _ptr(blocked), _ptr(units),
                                                     _ptr(fh), C.byref(best)),
                    "pcp_raycast_fan_mounted")
        return blocked[:P].copy(), units[:P].copy(), fh, best.value

    def raycast_fan_mounted_burst(self, poses6, fan: FanParams, el_table=None,
                                  reps: int = 20) -> float:
        """pcp_raycast_fan_mounted_burst -> the mounted launch's ms per launch."""
        poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
        ms = C.c_double()
        self._check(self.lib.pcp_raycast_fan_mounted_burst(
            self.h, _ptr(poses), poses.shape[0], C.byref(fan),
            _ptr(self._el_table(fan, el_table)), reps, C.byref(ms)),
            "pcp_raycast_fan_mounted_burst")
        return ms.value

    def simulate_scan_mounted_burst(self, poses6, fan: FanParams, el_table=None, reps: int = 20):
        """pcp_simulate_scan_mounted_burst -> (fan ms per launch, resolve ms per repetition)."""
        poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
        ms = np.zeros(2, np.float64)
        self._check(self.lib.pcp_simulate_scan_mounted_burst(
            self.h, _ptr(poses), poses.shape[0], C.byref(fan),
            _ptr(self._el_table(fan, el_table)), reps, _ptr(ms)),
            "pcp_simulate_scan_mounted_burst")
        return float(ms[0]), float(ms[1])

    def scan_points(self) -> int:
        """N of pcp_simulate_scan: the input point count of the cloud the terrain index was built
        from (an n == 0 query: nothing is launched)."""
        fan = FanParams(1, 1, -0.1, 0.1, 1.0)
        nret, npts = C.c_uint64(), C.c_uint64()
        off = np.zeros(1, np.uint64)
        self._check(self.lib.pcp_simulate_scan(self.h, None, 0, C.byref(fan), None, 0,
                                               C.byref(nret), _ptr(off), None, None, None, None,
                                               0, C.byref(npts), None, None),
                    "pcp_simulate_scan")
        return npts.value

    def simulate_scan_burst(self, poses5, fan: FanParams, reps: int = 20):
        """pcp_simulate_scan_burst -> (fan kernel ms per launch, resolve phase ms per repetition)."""
        poses = _poses5(poses5)
        ms = np.zeros(2, np.float64)
        self._check(self.lib.pcp_simulate_scan_burst(self.h, _ptr(poses), poses.shape[0],
                                                     C.byref(fan), reps, _ptr(ms)),
                    "pcp_simulate_scan_burst")
        return float(ms[0]), float(ms[1])

    @staticmethod
    def _cover_params(k_max, min_separation, fixed, reserved, n_fixed=None) -> CoverParams:
        fixed = [int(f) for f in fixed]
        cp = CoverParams(int(k_max), len(fixed) if n_fixed is None else int(n_fixed),
                         (C.c_int32 * 2)(int(reserved), 0), float(min_separation))
        for i, f in enumerate(fixed[:PLACE_MAX]):
            cp.fixed[i] = f
        return cp

    @staticmethod
    def _roi(roi):
        if roi is None:
            return None, 0
        r = np.ascontiguousarray(np.asarray(roi).reshape(-1) != 0, np.uint8)
        return r, r.shape[0]

    def place_coverage(self, poses5, fan: FanParams, k_max: int, min_separation: float = 0.0,
                       fixed=(), roi=None, want_round_gains: bool = False,
                       want_owner: bool = False, reserved: int = 0, owner_cap: int | None = None,
                       _mounted=None) -> dict:
        """pcp_place_coverage: greedy maximum coverage over simulated scans -- each round places
        the pose whose scan reaches the most terrain points of the region of interest `roi` (None:
        every point; else [N], non-zero counts) that no placed or fixed sensor reaches yet.
        -> dict: selected, gain, covered_after [n_selected], n_selected, n_points, roi_points,
        base_covered, seen_points [P], round_gains int64 [n_selected, P] (want_round_gains, else
        None; -1: not alive), point_owner int32 [n_points] (want_owner, else None; OWNER_NONE:
        nobody reaches the point, or it lies outside the region)."""
        # (_mounted: place_coverage_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_mounted" if _mounted else "pcp_place_coverage"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        P = poses.shape[0]
        K = max(int(k_max), 1)
        cp = self._cover_params(k_max, min_separation, fixed, reserved)
        r8, rn = self._roi(roi)
        sel = np.zeros(min(K, PLACE_MAX), np.int64)
        gain = np.zeros(min(K, PLACE_MAX), np.uint64)
        cov = np.zeros(min(K, PLACE_MAX), np.uint64)
        rg = np.zeros((min(K, PLACE_MAX), max(P, 1)), np.int64) if want_round_gains else None
        seen = np.zeros(max(P, 1), np.uint32)
        ocap = 0
        if want_owner:
            ocap = self.scan_points() if owner_cap is None else int(owner_cap)
        own = np.zeros(max(ocap, 1), np.int32) if want_owner else None
        npts, rpts, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ns = C.c_int32()
        self._check(fn(self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, C.byref(cp),
                       _ptr(r8), rn, _ptr(sel), _ptr(gain), _ptr(cov), _ptr(rg), _ptr(seen),
                       _ptr(own), ocap, C.byref(npts), C.byref(rpts), C.byref(base),
                       C.byref(ns)), what)
        k = ns.value
        return {"selected": sel[:k].copy(), "gain": gain[:k].copy(),
                "covered_after": cov[:k].copy(), "n_selected": k, "n_points": npts.value,
                "roi_points": rpts.value, "base_covered": base.value, "seen_points": seen[:P],
                "round_gains": rg[:k, :P] if want_round_gains else None,
                "point_owner": own[:npts.value] if want_owner else None}

    def place_coverage_mounted(self, poses6, fan: FanParams, el_table=None, k_max: int = 1,
                               min_separation: float = 0.0, fixed=(), roi=None,
                               want_round_gains: bool = False, want_owner: bool = False,
                               reserved: int = 0) -> dict:
        """pcp_place_coverage_mounted: place_coverage over tilted mounts -- poses6 rows x, y, z,
        roll, pitch, yaw -- with an optional beam table el_table [n_el] in radians."""
        return self.place_coverage(poses6, fan, k_max, min_separation, fixed, roi,
                                   want_round_gains, want_owner, reserved,
                                   _mounted=(self._el_table(fan, el_table),))

    def place_coverage_burst(self, poses5, fan: FanParams, k_max: int = 1,
                             min_separation: float = 0.0, fixed=(), roi=None, reps: int = 20,
                             _mounted=None):
        """pcp_place_coverage_burst -> (fan kernel ms per launch, bitset phase ms per repetition,
        round 0's gain launch ms per repetition)."""
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_mounted_burst" if _mounted else "pcp_place_coverage_burst"
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        cp = self._cover_params(k_max, min_separation, fixed, 0)
        r8, rn = self._roi(roi)
        ms = np.zeros(3, np.float64)
        self._check(getattr(self.lib, what)(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                            *lead, C.byref(cp), _ptr(r8), rn, reps, _ptr(ms)),
                    what)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def place_coverage_mounted_burst(self, poses6, fan: FanParams, el_table=None, k_max: int = 1,
                                     min_separation: float = 0.0, fixed=(), roi=None,
                                     reps: int = 20):
        """pcp_place_coverage_mounted_burst -> place_coverage_burst's triple."""
        return self.place_coverage_burst(poses6, fan, k_max, min_separation, fixed, roi, reps,
                                         _mounted=(self._el_table(fan, el_table),))

    @staticmethod
    def _weight(weight):
        """The weights as the ABI reads them: uint8 [N], each 0 .. 255 exactly (None stays null)."""
        if weight is None:
            return None, 0
        w = np.asarray(weight).reshape(-1)
        w8 = np.ascontiguousarray(w, np.uint8)
        if w.dtype != np.uint8 and not np.array_equal(w8, w):   # (bytes are passed as they are)
            raise ValueError("weights must be integers 0 .. 255")
        # (an empty array still has an address: the call tells no weights from null weights)
        return (w8 if w8.size else np.zeros(1, np.uint8)), w8.shape[0]

    def place_coverage_weighted(self, poses5, fan: FanParams, weight, k_max: int,
                                min_separation: float = 0.0, fixed=(),
                                want_round_gains: bool = False, want_owner: bool = False,
                                reserved: int = 0, owner_cap: int | None = None,
                                _mounted=None) -> dict:
        """pcp_place_coverage_weighted: place_coverage with a weight 0 .. 255 per terrain point
        (`weight` [N], required; 0: outside the region) -- each round places the pose whose scan
        reaches the most weight nobody reaches yet.
        -> place_coverage's dict with gain, covered_after, base_covered and round_gains in weight,
        plus gain_points uint64 [n_selected] (the points each round gained), roi_weight (the
        region's weight; roi_points stays its point count) and base_points."""
        # (_mounted: place_coverage_weighted_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_weighted_mounted" if _mounted else "pcp_place_coverage_weighted"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        P = poses.shape[0]
        K = min(max(int(k_max), 1), PLACE_MAX)
        cp = self._cover_params(k_max, min_separation, fixed, reserved)
        w8, wn = self._weight(weight)
        sel = np.zeros(K, np.int64)
        gain, cov, gpts = np.zeros(K, np.uint64), np.zeros(K, np.uint64), np.zeros(K, np.uint64)
        rg = np.zeros((K, max(P, 1)), np.int64) if want_round_gains else None
        seen = np.zeros(max(P, 1), np.uint32)
        ocap = 0
        if want_owner:
            ocap = self.scan_points() if owner_cap is None else int(owner_cap)
        own = np.zeros(max(ocap, 1), np.int32) if want_owner else None
        npts, rpts, rw = C.c_uint64(), C.c_uint64(), C.c_uint64()
        base, bpts = C.c_uint64(), C.c_uint64()
        ns = C.c_int32()
        self._check(fn(self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, C.byref(cp),
                       _ptr(w8), wn, _ptr(sel), _ptr(gain), _ptr(cov), _ptr(gpts), _ptr(rg),
                       _ptr(seen), _ptr(own), ocap, C.byref(npts), C.byref(rpts), C.byref(rw),
                       C.byref(base), C.byref(bpts), C.byref(ns)), what)
        k = ns.value
        return {"selected": sel[:k].copy(), "gain": gain[:k].copy(),
                "covered_after": cov[:k].copy(), "gain_points": gpts[:k].copy(), "n_selected": k,
                "n_points": npts.value, "roi_points": rpts.value, "roi_weight": rw.value,
                "base_covered": base.value, "base_points": bpts.value, "seen_points": seen[:P],
                "round_gains": rg[:k, :P] if want_round_gains else None,
                "point_owner": own[:npts.value] if want_owner else None}

    def place_coverage_weighted_mounted(self, poses6, fan: FanParams, weight, el_table=None,
                                        k_max: int = 1, min_separation: float = 0.0, fixed=(),
                                        want_round_gains: bool = False, want_owner: bool = False,
                                        reserved: int = 0) -> dict:
        """pcp_place_coverage_weighted_mounted: place_coverage_weighted over tilted mounts --
        poses6 rows x, y, z, roll, pitch, yaw -- with an optional beam table el_table [n_el]."""
        return self.place_coverage_weighted(poses6, fan, weight, k_max, min_separation, fixed,
                                            want_round_gains, want_owner, reserved,
                                            _mounted=(self._el_table(fan, el_table),))

    def place_coverage_weighted_burst(self, poses5, fan: FanParams, weight, k_max: int = 1,
                                      min_separation: float = 0.0, fixed=(), reps: int = 20,
                                      _mounted=None):
        """pcp_place_coverage_weighted_burst -> (fan kernel ms per launch, the build with the
        weight planes ms per repetition, round 0's gain launch ms per repetition)."""
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = ("pcp_place_coverage_weighted_mounted_burst" if _mounted
                else "pcp_place_coverage_weighted_burst")
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        cp = self._cover_params(k_max, min_separation, fixed, 0)
        w8, wn = self._weight(weight)
        ms = np.zeros(3, np.float64)
        self._check(getattr(self.lib, what)(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                            *lead, C.byref(cp), _ptr(w8), wn, reps, _ptr(ms)),
                    what)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def place_coverage_weighted_mounted_burst(self, poses6, fan: FanParams, weight,
                                              el_table=None, k_max: int = 1,
                                              min_separation: float = 0.0, fixed=(),
                                              reps: int = 20):
        """pcp_place_coverage_weighted_mounted_burst -> place_coverage_weighted_burst's triple."""
        return self.place_coverage_weighted_burst(poses6, fan, weight, k_max, min_separation,
                                                  fixed, reps,
                                                  _mounted=(self._el_table(fan, el_table),))

    @staticmethod
    def _cover_aim_params(k_max, n_aims, w_az, w_el, min_separation, fixed,
                          reserved) -> CoverAimParams:
        fixed = [(int(p), int(a)) for p, a in fixed]
        ap = CoverAimParams(int(k_max), int(n_aims), len(fixed), int(w_az), int(w_el),
                            (C.c_int32 * 3)(int(reserved), 0, 0), float(min_separation))
        for i, (p, a) in enumerate(fixed[:PLACE_MAX]):
            ap.fixed_pose[i] = p
            ap.fixed_aim[i] = a
        return ap

    def place_coverage_aimed(self, poses5, fan: FanParams, w_az: int, w_el: int, aims,
                             k_max: int, min_separation: float = 0.0, fixed=(), roi=None,
                             want_round_gains: bool = False, want_owner: bool = False,
                             want_aim_points: bool = False, reserved: int = 0,
                             owner_cap: int | None = None, n_aims: int | None = None,
                             _mounted=None) -> dict:
        """pcp_place_coverage_aimed: greedy coverage placement of sensors with a limited field of
        view -- every pose searched with every aim of `aims` [A, 2] (az0, el0), a window of w_az
        columns (wrapping) by w_el rings of the pose's own fan (cover_aims() makes them from
        angles); each round places the (pose, aim) whose window reaches the most terrain points of
        `roi` nobody reaches yet.  fixed: (pose, aim) pairs already placed.
        -> dict: selected, selected_aim, gain, covered_after [n_selected], n_selected, n_points,
        roi_points, base_covered, seen_points [P], round_gains int64 [n_selected, P, A]
        (want_round_gains, else None; -1: not alive), aim_points uint32 [P, A] (want_aim_points,
        else None), point_owner int32 [n_points] (want_owner, else None)."""
        # (_mounted: place_coverage_aimed_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_aimed_mounted" if _mounted else "pcp_place_coverage_aimed"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        aims = np.ascontiguousarray(aims, np.int32).reshape(-1, 2)
        A = aims.shape[0] if n_aims is None else int(n_aims)
        P = poses.shape[0]
        K = min(max(int(k_max), 1), PLACE_MAX)
        ap = self._cover_aim_params(k_max, A, w_az, w_el, min_separation, fixed, reserved)
        r8, rn = self._roi(roi)
        sel = np.zeros(K, np.int64)
        sel_aim = np.zeros(K, np.int32)
        gain = np.zeros(K, np.uint64)
        cov = np.zeros(K, np.uint64)
        # (a refused call writes nothing: the tables' shapes need not fit it)
        At = min(max(A, 1), COVER_AIM_MAX)
        Pt = max(min(P, AIM_MAX_ROWS // At), 1)
        rg = np.zeros((K, Pt, At), np.int64) if want_round_gains else None
        apts = np.zeros((Pt, At), np.uint32) if want_aim_points else None
        seen = np.zeros(max(P, 1), np.uint32)
        ocap = 0
        if want_owner:
            ocap = self.scan_points() if owner_cap is None else int(owner_cap)
        own = np.zeros(max(ocap, 1), np.int32) if want_owner else None
        npts, rpts, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ns = C.c_int32()
        self._check(fn(self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, C.byref(ap),
                       _ptr(aims), _ptr(r8), rn, _ptr(sel), _ptr(sel_aim), _ptr(gain),
                       _ptr(cov), _ptr(rg), _ptr(seen), _ptr(apts), _ptr(own), ocap,
                       C.byref(npts), C.byref(rpts), C.byref(base), C.byref(ns)), what)
        k = ns.value
        return {"selected": sel[:k].copy(), "selected_aim": sel_aim[:k].copy(),
                "gain": gain[:k].copy(), "covered_after": cov[:k].copy(), "n_selected": k,
                "n_points": npts.value, "roi_points": rpts.value, "base_covered": base.value,
                "seen_points": seen[:P],
                "round_gains": rg[:k, :P] if want_round_gains else None,
                "aim_points": apts[:P] if want_aim_points else None,
                "point_owner": own[:npts.value] if want_owner else None}

    def place_coverage_aimed_mounted(self, poses6, fan: FanParams, w_az: int, w_el: int, aims,
                                     el_table=None, k_max: int = 1, min_separation: float = 0.0,
                                     fixed=(), roi=None, want_round_gains: bool = False,
                                     want_owner: bool = False, want_aim_points: bool = False,
                                     reserved: int = 0) -> dict:
        """pcp_place_coverage_aimed_mounted: place_coverage_aimed over tilted mounts -- poses6 rows
        x, y, z, roll, pitch, yaw -- with an optional beam table el_table [n_el] in radians; an
        aim turns the head about its own spin axis."""
        return self.place_coverage_aimed(poses6, fan, w_az, w_el, aims, k_max, min_separation,
                                         fixed, roi, want_round_gains, want_owner,
                                         want_aim_points, reserved,
                                         _mounted=(self._el_table(fan, el_table),))

    def place_coverage_aimed_burst(self, poses5, fan: FanParams, w_az: int, w_el: int, aims,
                                   k_max: int = 1, min_separation: float = 0.0, fixed=(),
                                   roi=None, reps: int = 20, _mounted=None):
        """pcp_place_coverage_aimed_burst -> (fan kernel ms per launch, the whole build with the
        aim masks ms per repetition, round 0's launch ms per repetition)."""
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = ("pcp_place_coverage_aimed_mounted_burst" if _mounted
                else "pcp_place_coverage_aimed_burst")
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        aims = np.ascontiguousarray(aims, np.int32).reshape(-1, 2)
        ap = self._cover_aim_params(k_max, aims.shape[0], w_az, w_el, min_separation, fixed, 0)
        r8, rn = self._roi(roi)
        ms = np.zeros(3, np.float64)
        self._check(getattr(self.lib, what)(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                            *lead, C.byref(ap), _ptr(aims), _ptr(r8), rn, reps,
                                            _ptr(ms)), what)
        return float(ms[0]), float(ms[1]), float(ms[2])

    def place_coverage_aimed_mounted_burst(self, poses6, fan: FanParams, w_az: int, w_el: int,
                                           aims, el_table=None, k_max: int = 1,
                                           min_separation: float = 0.0, fixed=(), roi=None,
                                           reps: int = 20):
        """pcp_place_coverage_aimed_mounted_burst -> place_coverage_aimed_burst's triple."""
        return self.place_coverage_aimed_burst(poses6, fan, w_az, w_el, aims, k_max,
                                               min_separation, fixed, roi, reps,
                                               _mounted=(self._el_table(fan, el_table),))

    def place_coverage_pair(self, poses5, fan: FanParams, min_separation: float = 0.0, fixed=(),
                            roi=None, want_pair_gains: bool = False, want_owner: bool = False,
                            reserved: int = 0, owner_cap: int | None = None,
                            _mounted=None) -> dict:
        """pcp_place_coverage_pair: the exact best pair of the poses by the terrain points of the
        region `roi` their scans reach beside the `fixed` poses (every admissible pair a < b
        evaluated; the first maximum in row-major order), with the best single pose for comparison.
        -> dict: n_selected (2: the pair beats the single, 1: only the single adds, 0), best_pair
        (2,), pair_gain, best_single, single_gain, single_gains / partner / partner_gain int64 [P]
        (-1: not admissible / no pair in the row), n_points, roi_points, base_covered, seen_points
        [P], pair_gains int64 [P, P] (want_pair_gains, else None; -1 off the admissible upper
        triangle), point_owner int32 [n_points] of the answer (want_owner, else None)."""
        # (_mounted: place_coverage_pair_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_pair_mounted" if _mounted else "pcp_place_coverage_pair"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        P = poses.shape[0]
        pp = self._pair_params(fixed, min_separation, reserved)
        r8, rn = self._roi(roi)
        bp = np.full(2, -1, np.int64)
        pg, sgn = C.c_uint64(), C.c_uint64()
        bs = C.c_int64(-1)
        sg = np.full(max(P, 1), -1, np.int64)
        partner = np.full(max(P, 1), -1, np.int64)
        pgain = np.full(max(P, 1), -1, np.int64)
        dense = want_pair_gains and P <= COVER_MAX_POSES   # (a refused call writes nothing)
        tab = np.full((max(P, 1), max(P, 1)), -1, np.int64) if dense else None
        seen = np.zeros(max(P, 1), np.uint32)
        ocap = 0
        if want_owner:
            ocap = self.scan_points() if owner_cap is None else int(owner_cap)
        own = np.zeros(max(ocap, 1), np.int32) if want_owner else None
        npts, rpts, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ns = C.c_int32()
        self._check(fn(self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, C.byref(pp),
                       _ptr(r8), rn, _ptr(bp), C.byref(pg), C.byref(bs), C.byref(sgn), _ptr(sg),
                       _ptr(tab), _ptr(partner), _ptr(pgain), _ptr(seen), _ptr(own), ocap,
                       C.byref(npts), C.byref(rpts), C.byref(base), C.byref(ns)), what)
        return {"n_selected": ns.value, "best_pair": bp, "pair_gain": pg.value,
                "best_single": bs.value, "single_gain": sgn.value, "single_gains": sg[:P],
                "partner": partner[:P], "partner_gain": pgain[:P], "n_points": npts.value,
                "roi_points": rpts.value, "base_covered": base.value, "seen_points": seen[:P],
                "pair_gains": tab[:P, :P] if want_pair_gains and dense else None,
                "point_owner": own[:npts.value] if want_owner else None}

    def place_coverage_pair_mounted(self, poses6, fan: FanParams, el_table=None,
                                    min_separation: float = 0.0, fixed=(), roi=None,
                                    want_pair_gains: bool = False, want_owner: bool = False,
                                    reserved: int = 0) -> dict:
        """pcp_place_coverage_pair_mounted: place_coverage_pair over tilted mounts -- poses6 rows
        x, y, z, roll, pitch, yaw -- with an optional beam table el_table [n_el] in radians."""
        return self.place_coverage_pair(poses6, fan, min_separation, fixed, roi, want_pair_gains,
                                        want_owner, reserved,
                                        _mounted=(self._el_table(fan, el_table),))

    def place_coverage_pair_burst(self, poses5, fan: FanParams, min_separation: float = 0.0,
                                  fixed=(), roi=None, reps: int = 20, _mounted=None):
        """pcp_place_coverage_pair_burst -> (mask pass with the singles, pair tiles with the
        selection), ms per repetition each."""
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = ("pcp_place_coverage_pair_mounted_burst" if _mounted
                else "pcp_place_coverage_pair_burst")
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        pp = self._pair_params(fixed, min_separation, 0)
        r8, rn = self._roi(roi)
        ms = np.zeros(2, np.float64)
        self._check(getattr(self.lib, what)(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                            *lead, C.byref(pp), _ptr(r8), rn, reps, _ptr(ms)),
                    what)
        return float(ms[0]), float(ms[1])

    def place_coverage_pair_mounted_burst(self, poses6, fan: FanParams, el_table=None,
                                          min_separation: float = 0.0, fixed=(), roi=None,
                                          reps: int = 20):
        """pcp_place_coverage_pair_mounted_burst -> place_coverage_pair_burst's pair."""
        return self.place_coverage_pair_burst(poses6, fan, min_separation, fixed, roi, reps,
                                              _mounted=(self._el_table(fan, el_table),))

    def place_coverage_refine(self, poses5, fan: FanParams, start, n_locked: int = 0,
                              max_moves: int = 16, min_separation: float = 0.0, roi=None,
                              want_swap_covered: bool = False, want_owner: bool = False,
                              reserved: int = 0, owner_cap: int | None = None,
                              _mounted=None) -> dict:
        """pcp_place_coverage_refine: the set `start` of poses improved by single-sensor exchanges
        over the coverage objective (every unlocked slot tried at every other pose with the rest
        held; the best exchange taken while it raises the count of terrain points of the region
        `roi` the set's scans reach).  max_moves + 1 evaluations are enqueued up front and those
        behind the stop return at once: an empty pair of launches still costs queue time, so a
        large max_moves is paid for after an early convergence too.
        -> dict: selected [k], covered, start_covered, n_moves, converged (1: no single move
        raises the count; 0: max_moves ran out first), move_slot / move_from / move_to /
        move_covered [n_moves], slot_unique [k] (the points only that slot of the final set
        reaches), seen_points [P], n_points, roi_points, and on request swap_covered int64
        [n_moves + 1, k, P] (-1 at inadmissible moves), point_owner int32 [n_points] (the lowest
        slot that reaches the point; OWNER_NONE: nobody does, or it lies outside the region)."""
        # (_mounted: place_coverage_refine_mounted's (el_table,), the same call on poses6 rows)
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = "pcp_place_coverage_refine_mounted" if _mounted else "pcp_place_coverage_refine"
        fn = getattr(self.lib, what)
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        P = poses.shape[0]
        rp = self._refine_params(start, n_locked, max_moves, min_separation, reserved)
        r8, rn = self._roi(roi)
        k = max(min(rp.k, PLACE_MAX), 1)
        mm = max(min(int(max_moves), REFINE_MAX_MOVES), 0)
        sel = np.full(k, -1, np.int64)
        cov, sc = C.c_uint64(), C.c_uint64()
        m_slot = np.zeros(max(mm, 1), np.int32)
        m_from = np.zeros(max(mm, 1), np.int64)
        m_to = np.zeros(max(mm, 1), np.int64)
        m_cov = np.zeros(max(mm, 1), np.uint64)
        dense = want_swap_covered and P <= COVER_MAX_POSES   # (a refused call writes nothing)
        tab = np.full((mm + 1, k, max(P, 1)), -1, np.int64) if dense else None
        uniq = np.zeros(k, np.uint64)
        seen = np.zeros(max(P, 1), np.uint32)
        ocap = 0
        if want_owner:
            ocap = self.scan_points() if owner_cap is None else int(owner_cap)
        own = np.zeros(max(ocap, 1), np.int32) if want_owner else None
        npts, rpts = C.c_uint64(), C.c_uint64()
        nm, cv = C.c_int32(), C.c_int32()
        self._check(fn(self.h, _ptr(poses) if P else None, P, C.byref(fan), *lead, C.byref(rp),
                       _ptr(r8), rn, _ptr(sel), C.byref(cov), C.byref(sc), _ptr(m_slot),
                       _ptr(m_from), _ptr(m_to), _ptr(m_cov), _ptr(tab), _ptr(uniq), _ptr(seen),
                       _ptr(own), ocap, C.byref(npts), C.byref(rpts), C.byref(nm), C.byref(cv)),
                    what)
        n = nm.value
        evals = n + 1 if npts.value else 0   # (without terrain nothing is evaluated: no table)
        return {"selected": sel, "covered": cov.value, "start_covered": sc.value, "n_moves": n,
                "converged": cv.value, "move_slot": m_slot[:n].copy(),
                "move_from": m_from[:n].copy(), "move_to": m_to[:n].copy(),
                "move_covered": m_cov[:n].copy(), "slot_unique": uniq, "seen_points": seen[:P],
                "n_points": npts.value, "roi_points": rpts.value,
                "swap_covered": tab[:evals, :, :P].copy() if dense else None,
                "point_owner": own[:npts.value] if want_owner else None}

    def place_coverage_refine_mounted(self, poses6, fan: FanParams, start, el_table=None,
                                      n_locked: int = 0, max_moves: int = 16,
                                      min_separation: float = 0.0, roi=None,
                                      want_swap_covered: bool = False, want_owner: bool = False,
                                      reserved: int = 0) -> dict:
        """pcp_place_coverage_refine_mounted: place_coverage_refine over tilted mounts -- poses6
        rows x, y, z, roll, pitch, yaw -- with an optional beam table el_table [n_el] in radians."""
        return self.place_coverage_refine(poses6, fan, start, n_locked, max_moves, min_separation,
                                          roi, want_swap_covered, want_owner, reserved,
                                          _mounted=(self._el_table(fan, el_table),))

    def place_coverage_refine_burst(self, poses5, fan: FanParams, start, n_locked: int = 0,
                                    min_separation: float = 0.0, roi=None, reps: int = 20,
                                    _mounted=None):
        """pcp_place_coverage_refine_burst -> (the start set's preparation pass, its evaluation
        launch with the selection), ms per repetition each."""
        poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 6 if _mounted else 5)
        what = ("pcp_place_coverage_refine_mounted_burst" if _mounted
                else "pcp_place_coverage_refine_burst")
        lead = (_ptr(_mounted[0]),) if _mounted else ()
        rp = self._refine_params(start, n_locked, 0, min_separation, 0)
        r8, rn = self._roi(roi)
        ms = np.zeros(2, np.float64)
        self._check(getattr(self.lib, what)(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                            *lead, C.byref(rp), _ptr(r8), rn, reps, _ptr(ms)),
                    what)
        return float(ms[0]), float(ms[1])

    def place_coverage_refine_mounted_burst(self, poses6, fan: FanParams, start, el_table=None,
                                            n_locked: int = 0, min_separation: float = 0.0,
                                            roi=None, reps: int = 20):
        """pcp_place_coverage_refine_mounted_burst -> place_coverage_refine_burst's pair."""
        return self.place_coverage_refine_burst(poses6, fan, start, n_locked, min_separation, roi,
                                                reps, _mounted=(self._el_table(fan, el_table),))

    def score_poses_stats(self, poses5, zx120_pose5, params: VlParams) -> dict:
        """pcp_score_poses_stats: the gather lane-loads of the query's visibility rays
        (diagnostic twin of k_score_cells; the caller's flags are not touched)."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        st = np.zeros(4, np.uint64)
        self._check(self.lib.pcp_score_poses_stats(self.h, _ptr(poses), poses.shape[0], _ptr(zx),
                                                   C.byref(params), _ptr(st)),
                    "pcp_score_poses_stats")
        return {"probes": int(st[0]), "walk_starts": int(st[1]), "point_tests": int(st[2]),
                "directory_loads": int(st[3])}

    def score_poses_burst(self, poses5, zx120_pose5, params: VlParams, reps: int = 20) -> float:
        """pcp_score_poses_burst: the query's production k_score_cells launch `reps` times
        back-to-back between two events -> ms per launch."""
        poses = _poses5(poses5)
        zx = _zx5(zx120_pose5)
        ms = C.c_double()
        self._check(self.lib.pcp_score_poses_burst(self.h, _ptr(poses), poses.shape[0], _ptr(zx),
                                                   C.byref(params), reps, C.byref(ms)),
                    "pcp_score_poses_burst")
        return ms.value

    def score_poses_allreduce(self, poses5: np.ndarray, zx120_pose5: np.ndarray,
                              params: VlParams, lo: int, p_total: int, cell_flags: np.ndarray,
                              tot_all: np.ndarray | None, cov_all: np.ndarray | None,
                              rep: "VlReport", timed: bool = False):
        """pcp_score_poses_allreduce: runOptimization's scoring of this rank's poses [lo, lo + P)
        of p_total, ONE ncclAllReduce(MAX) over libpcp's own communicator (comm_init_rank), the
        stale flags, argmax (rep.best_idx, global) and colour statistics on every rank.
        tot_all float64 / cov_all int32 ([>= p_total], or None) receive every pose's total and
        covered count; cell_flags updated in place.  -> collective ms (timed) or None."""
        P = poses5.shape[0]
        if (poses5.dtype != np.float64 or not poses5.flags.c_contiguous or poses5.ndim != 2
                or zx120_pose5.dtype != np.float64 or not zx120_pose5.flags.c_contiguous
                or cell_flags.dtype != np.uint8 or not cell_flags.flags.c_contiguous
                or (tot_all is not None and (tot_all.dtype != np.float64
                                             or tot_all.shape[0] < p_total))
                or (cov_all is not None and (cov_all.dtype != np.int32
                                             or cov_all.shape[0] < p_total))):
            raise ValueError("score_poses_allreduce: bad array types or sizes")
        ms = C.c_double()
        self._check(self.lib.pcp_score_poses_allreduce(
            self.h, poses5.ctypes.data if P else None, P, zx120_pose5.ctypes.data,
            C.byref(params), lo, p_total, cell_flags.ctypes.data, _ptr(tot_all), _ptr(cov_all),
            C.byref(rep), C.byref(ms) if timed else None), "pcp_score_poses_allreduce")
        return ms.value if timed else None

    def raycast_fan(self, poses5: np.ndarray, fan: FanParams, want_first_hit=False):
        poses = _poses5(poses5)
        P = poses.shape[0]
        blocked = np.zeros(max(P, 1), np.uint32)
        units = np.zeros(max(P, 1), np.uint64)
        fh = np.empty((P, fan.n_el, fan.n_az), np.int16) if want_first_hit else None
        best = C.c_int64()
        self._check(self.lib.pcp_raycast_fan(self.h, _ptr(poses), P, C.byref(fan), _ptr(blocked),
                                             _ptr(units), _ptr(fh), C.byref(best)),
                    "pcp_raycast_fan")
        return blocked[:P].copy(), units[:P].copy(), fh, best.value


class Multi:
    """pcp_multi: one process, n GPUs -- the pose search sharded over
    contexts with ONE RCCL collective per query.  devices: one device id per rank, all
    distinct (RCCL) or all the same (a rehearsal of n ranks on one GPU: no RCCL, the keys
    combine on the device); a mixed list is refused."""

    def __init__(self, devices, lib_path=None):
        self.lib = load_library(lib_path)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.lib.pcp_multi_create(len(devices), devs, C.byref(h))
        if rc != PCP_OK:
            raise PcpError(rc, f"pcp_multi_create(devices={list(devices)}) failed")
        self.h = h
        n, rccl = C.c_int(), C.c_int()
        self.lib.pcp_multi_info(self.h, C.byref(n), C.byref(rccl))
        self.n, self.uses_rccl = n.value, bool(rccl.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pcp_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != PCP_OK:
            msg = self.lib.pcp_multi_last_error(self.h)
            raise PcpError(rc, f"{what}: {msg.decode() if msg else ''}")

    def set_terrain(self, cloud: np.ndarray, point_step=None, offs=(0, 4, 8)):
        v = cloud_view(cloud, point_step, offs)
        self._check(self.lib.pcp_multi_set_terrain(self.h, C.byref(v)), "pcp_multi_set_terrain")

    def set_aux_cloud(self, cloud: np.ndarray, point_step=None, offs=(0, 4, 8)):
        v = cloud_view(cloud, point_step, offs)
        self._check(self.lib.pcp_multi_set_aux_cloud(self.h, C.byref(v)),
                    "pcp_multi_set_aux_cloud")

    def set_cells(self, xyz: np.ndarray, normals: np.ndarray):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert xyz.shape == nrm.shape
        self._check(self.lib.pcp_multi_set_cells(self.h, _ptr(xyz), _ptr(nrm), xyz.shape[0]),
                    "pcp_multi_set_cells")

    def raycast_fan(self, poses5: np.ndarray, fan: FanParams):
        poses = _poses5(poses5)
        P = poses.shape[0]
        blocked = np.zeros(max(P, 1), np.uint32)
        units = np.zeros(max(P, 1), np.uint64)
        best = C.c_int64()
        self._check(self.lib.pcp_multi_raycast_fan(self.h, _ptr(poses), P, C.byref(fan),
                                                   _ptr(blocked), _ptr(units), C.byref(best)),
                    "pcp_multi_raycast_fan")
        return blocked[:P].copy(), units[:P].copy(), best.value

    def score_poses(self, poses5: np.ndarray, zx120_pose5, params: VlParams,
                    cell_flags: np.ndarray):
        poses = _poses5(poses5)
        P = poses.shape[0]
        zx = _zx5(zx120_pose5)
        assert cell_flags.dtype == np.uint8 and cell_flags.flags.c_contiguous
        tot = np.empty(max(P, 1), np.float64)
        cov = np.empty(max(P, 1), np.int32)
        rep = VlReport()
        self._check(self.lib.pcp_multi_score_poses(self.h, _ptr(poses), P, _ptr(zx),
                                                   C.byref(params), _ptr(cell_flags), _ptr(tot),
                                                   _ptr(cov), C.byref(rep)),
                    "pcp_multi_score_poses")
        return tot[:P].copy(), cov[:P].copy(), rep


def _fan_stats(self, poses5, fan):
    """pcp_raycast_fan_stats: the fan launch's gather lane-loads by kind.  Over the split fine
    records: samples_visited = probes (2-byte threshold loads); scanned_stencils = walk starts
    actually loaded (a candidate settled by its window's pivot loads none, DESIGN.md §5 Skip 6);
    point_tests = every exact point test, the pivot tests included; their sum is the launch's
    gather count.  directory_loads is 0 over a fine copy."""
    poses = _poses5(poses5)
    st = np.zeros(4, np.uint64)
    self._check(self.lib.pcp_raycast_fan_stats(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                               _ptr(st)), "pcp_raycast_fan_stats")
    return {"samples_visited": int(st[0]), "scanned_stencils": int(st[1]),
            "point_tests": int(st[2]), "directory_loads": int(st[3])}


Context.raycast_fan_stats = _fan_stats


def _fan_stamps(self, poses5, fan):
    """Per-wave shader-clock stamps (diagnostic build): (P, waves, 4) uint64."""
    poses = _poses5(poses5)
    waves = (fan.n_az * fan.n_el + 63) // 64
    st = np.zeros((poses.shape[0], waves, 4), np.uint64)
    self._check(self.lib.pcp_raycast_fan_stamps(self.h, _ptr(poses), poses.shape[0],
                                                C.byref(fan), _ptr(st)),
                "pcp_raycast_fan_stamps")
    return st


Context.raycast_fan_stamps = _fan_stamps


def _fan_burst(self, poses5, fan, reps=20):
    """Average launch time (ms) of the production fan kernel over `reps` back-to-back launches."""
    poses = _poses5(poses5)
    ms = C.c_double()
    self._check(self.lib.pcp_raycast_fan_burst(self.h, _ptr(poses), poses.shape[0], C.byref(fan),
                                               reps, C.byref(ms)), "pcp_raycast_fan_burst")
    return ms.value


Context.raycast_fan_burst = _fan_burst


def step_table(end: float) -> np.ndarray:
    lib = load_library()
    n = C.c_uint64()
    lib.pcp_step_table(end, None, 0, C.byref(n))
    out = np.empty(max(n.value, 1), np.float64)
    lib.pcp_step_table(end, _ptr(out), n.value, C.byref(n))
    return out[: n.value]


def default_vl_params(**kw) -> VlParams:
    """virtual_lidar.cpp:66-71 defaults."""
    p = VlParams(0.1, 1.1, 3.0, 15.0, 100, 10)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def fan_params(n_az=1024, n_el=256, el_min_deg=-85.0, el_max_deg=85.0, max_distance=15.0):
    return FanParams(n_az, n_el, el_min_deg * np.pi / 180.0, el_max_deg * np.pi / 180.0,
                     max_distance)


def cover_aims(fan: FanParams, h_fov: float, v_fov: float, yaws, pitches):
    """Angles -> pcp_place_coverage_aimed's (w_az, w_el, aims int32 [len(yaws) * len(pitches), 2]),
    yaw-major.  Column i of a fan looks along azimuth i * da, da = 2 pi / n_az, from the pose's
    heading; ring j along elevation el_min + (j + 0.5) * de, de = (el_max - el_min) / n_el.
    The rounding rule, nearest(x) = floor(x + 0.5):
      w_az = nearest(h_fov / da) held to 1 .. n_az, w_el = nearest(v_fov / de) held to 1 .. n_el
      (a window is at least one column by one ring, however narrow the angles);
      az0 = nearest(yaw / da - (w_az - 1) / 2) mod n_az: the window's middle on the column
      nearest the yaw (azimuth wraps);
      el0 = nearest((pitch - el_min) / de - 0.5 - (w_el - 1) / 2) held to 0 .. n_el - w_el: the
      window's middle on the ring nearest the pitch, pushed back inside the fan (rings do not
      wrap)."""
    n_az, n_el = int(fan.n_az), int(fan.n_el)
    da = 2.0 * np.pi / n_az
    de = (fan.el_max - fan.el_min) / n_el

    def nearest(x):
        return int(np.floor(x + 0.5))

    w_az = min(max(nearest(h_fov / da), 1), n_az)
    w_el = min(max(nearest(v_fov / de), 1), n_el)
    aims = []
    for yaw in np.asarray(yaws, np.float64).reshape(-1):
        az0 = nearest(yaw / da - (w_az - 1) / 2.0) % n_az
        for pitch in np.asarray(pitches, np.float64).reshape(-1):
            el0 = nearest((pitch - fan.el_min) / de - 0.5 - (w_el - 1) / 2.0)
            aims.append((az0, min(max(el0, 0), n_el - w_el)))
    return w_az, w_el, np.array(aims, np.int32).reshape(-1, 2)
