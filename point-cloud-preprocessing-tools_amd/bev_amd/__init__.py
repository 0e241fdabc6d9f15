"""ctypes binding of the C ABI in include/bev_mi355x.h (libbev_mi355x.so).

Python is plumbing here (tests, bench.py, smoke): the product is the HIP
library.  There is no Python or CPU implementation of the hot path in this
package; if the library is missing or no GPU is usable, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent
REPO_DIR = PKG_DIR.parent
# BEV_AMD_LIB: developer override (e.g. the `make clk` build with in-kernel phase clocks); never a fallback
LIB_PATH = Path(os.environ["BEV_AMD_LIB"]) if os.environ.get("BEV_AMD_LIB") else PKG_DIR / "csrc" / "libbev_mi355x.so"
SYNTH_PATH = PKG_DIR / "synth" / "libbev_synth.so"

# pcl::PointXYZIRCT in memory (reference BatchMultiBevGen.h:43-54), 32 bytes
POINT_DTYPE = np.dtype(
    {
        "names": ["x", "y", "z", "_pad0", "intensity", "row", "col", "t", "label", "_pad1"],
        "formats": ["<f4", "<f4", "<f4", "<f4", "<f4", "<u2", "<u2", "<u4", "<i2", "<u2"],
        "offsets": [0, 4, 8, 12, 16, 20, 22, 24, 28, 30],
        "itemsize": 32,
    }
)

GROUND_GRID_CELLS = 75 * 50


class BevParams(C.Structure):
    _fields_ = [
        ("n_scan", C.c_int32),
        ("horizon_scan", C.c_int32),
        ("ground_upper_scan", C.c_int32),
        ("height_res", C.c_float),
        ("interval", C.c_float),
        ("max_range", C.c_int32),
        ("n_layers", C.c_int32),
        ("lidar_to_ground", C.c_float),
    ]

    @property
    def slots(self) -> int:
        return self.n_scan * self.horizon_scan

    @property
    def mat_size(self) -> int:
        return int(np.float32(self.max_range * 2) / np.float32(self.interval))


class KernelStat(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("launches", C.c_uint64),
        ("total_ms", C.c_double),
        ("frames", C.c_uint64),
    ]


class BevError(RuntimeError):
    pass


_lib = None
LAYOUT_UNKNOWN, LAYOUT_STRUCTURED, LAYOUT_FIRING_ORDER = 0, 3, 4  # bev_set_layout_hint
PROJECT_MULRAN, PROJECT_OXFORD, PROJECT_KITTI = 0, 1, 2  # BEV_PROJECT_*
PROJECT_KITTI_GROUP = 16  # BEV_PROJECT_KITTI_GROUP: frames per launch group of the batched KITTI projection
KITTI_SLOTS = 64 * 2083
FLOAT_BEV_MAX_POSES = 64  # BEV_FLOAT_BEV_MAX_POSES: poses per frame of float_bev_device / float_bev_batch
POSED_BEV_MAX_POSES = 64  # BEV_POSED_BEV_MAX_POSES: poses per frame of posed_bev_device / posed_bev_batch
SUBMAP_MAX_ENTRIES = 1 << 20  # BEV_SUBMAP_MAX_ENTRIES: (frame, pose) entries of one submap_bev_device / submap_bev_batch call
SUBMAP_COARSE_MAX_TARGET = 1 << 22  # BEV_SUBMAP_COARSE_MAX_TARGET: rows of one map, entries times stride (submap_coarse_registration_device)
SUBMAP_SEARCH_GRID_MAX = 1024  # BEV_SUBMAP_SEARCH_GRID_MAX: the largest cap of cells per axis of set_submap_search_grid
PAIR_SEARCH_GRID_MAX = 1024  # BEV_PAIR_SEARCH_GRID_MAX: the largest cap of cells per axis of set_pair_search_grid
SUBMAP_REG_MAX_TARGET = 1 << 22  # BEV_SUBMAP_REG_MAX_TARGET: records of one map's entries' frames together (submap_registration_*)

# every symbol include/bev_mi355x.h declares
ABI_SYMBOLS = [
    "bev_params_for_sensor", "bev_num_slots", "bev_multi_bytes", "bev_single_bytes",
    "bev_create", "bev_destroy", "bev_strerror", "bev_last_error",
    "bev_process_batch", "bev_process_device_resident", "bev_synchronize",
    "bev_order_cloud", "bev_mark_ground", "bev_multi_bev", "bev_single_bev",
    "bev_float_bev", "bev_float_bev_size", "bev_transform_cloud", "bev_yaw_translate_matrix", "bev_project_xyzi", "bev_project_out_points", "bev_host_alloc", "bev_host_free",
    "bev_set_lanes", "bev_set_layout_hint", "bev_profile_enable", "bev_profile_reset", "bev_profile_get",
    "bev_debug_get_cell_avg", "bev_debug_get_frame_info", "bev_debug_get_code_overflow", "bev_debug_angle_predicate", "bev_debug_exact_eval", "bev_abi_version",
    "bev_top_part_flatten", "bev_voxel_grid_xyz", "bev_normals_2d", "bev_registration_front_device_resident",
    "bev_regfront_max_out",
    "bev_icp_coarse_defaults", "bev_icp_point_to_plane", "bev_coarse_registration_device_resident",
    "bev_voxel_grid_irct", "bev_icp_fine_defaults", "bev_icp_whole_defaults", "bev_icp_point_to_point",
    "bev_fine_registration_device_resident",
    "bev_project_device_resident", "bev_project_batch_out_points", "bev_process_batch_xyzi",
    "bev_float_bev_device_resident", "bev_float_bev_batch",
    "bev_posed_bev_device_resident", "bev_posed_bev_batch",
    "bev_submap_bev_device_resident", "bev_submap_bev_batch",
    "bev_submap_float_bev_device_resident", "bev_submap_float_bev_batch",
    "bev_submap_registration_device_resident", "bev_submap_registration_batch",
    "bev_submap_voxel_registration_device_resident", "bev_submap_voxel_registration_batch",
    "bev_submap_voxel_cloud_device_resident",
    "bev_submap_coarse_registration_device_resident",
    "bev_submap_coarse_voxel_registration_device_resident", "bev_submap_pn_cloud_device_resident",
    "bev_submap_top_part_cloud_device_resident", "bev_submap_top_part_coarse_registration_device_resident",
    "bev_submap_top_part_max_out",
    "bev_set_submap_search_grid", "bev_debug_get_submap_grid",
    "bev_set_pair_search_grid", "bev_debug_get_pair_grid",
    "bev_place_defaults", "bev_place_descriptor_bytes", "bev_place_desc_handle_bytes",
    "bev_place_descriptor_device_resident", "bev_place_match_device_resident", "bev_place_retrieval_batch",
    "bev_verify_defaults", "bev_verify_clouds", "bev_verify_registration_device_resident",
    "bev_submap_verify_registration_device_resident", "bev_verify_registration_batch",
    "bev_align_defaults", "bev_align_grid_bytes", "bev_align_grid_device_resident", "bev_align_hits_device_resident",
    "bev_align_batch",
]

# bev_debug_exact_eval (include/bev_mi355x.h, BEV_EVAL_* in id order): name -> (input kinds f / u / d, output kind, params)
EXACT_EVAL = {
    "fd_atanf": ("f", "f", 0), "fd_atan2f": ("ff", "f", 0), "kitti_azimuth": ("ff", "f", 0), "kitti_col": ("f", "i", 0),
    "kitti_crossing": ("ff", "i", 0), "project_mulran": ("uff", "u", 0), "project_oxford": ("fff", "u", 0),
    "fd_sin": ("d", "d", 0), "fd_cos": ("d", "d", 0), "cvtt_f32": ("f", "i", 0), "cvtt_f64": ("d", "i", 0),
    "floor_half_to_int": ("f", "i", 0), "ground_cell": ("ff", "i", 0), "round_half_up_bin": ("f", "i", 0),
    "height_times4": ("f", "i", 0), "bin_in_range": ("fu", "u", 0), "bin_of_shifted": ("fu", "u", 0),
    "bev_bin": ("fff", "i", 0), "count_advance": ("fu", "f", 0), "exact_reciprocal": ("f", "f", 0),
    "angle_is_ground_nodiv": ("fff", "i", 0), "angle_is_ground": ("fff", "i", 0), "transform_xyz": ("fff", "f3", 12),
    "degrees_of": ("f", "f", 0), "wrap_azimuth": ("f", "f", 0), "to_u16": ("f", "i", 0), "bev_code": ("fff", "u", 5),
    "kitti_col_xy": ("ff", "i", 0),
}
EXACT_EVAL_NAMES = list(EXACT_EVAL)
EXACT_EVAL_MAX_N = 1 << 24  # BEV_EVAL_MAX_N
_EVAL_IN = {"f": np.float32, "u": np.uint32, "d": np.float64}
_EVAL_OUT = {"f": np.float32, "i": np.int32, "u": np.uint32, "d": np.float64, "f3": np.float32}

# registration front end (include/bev_mi355x.h): pcl::PointXYZ, pcl::Normal, pcl::PointNormal as float rows
XYZ_FLOATS, NORMAL_FLOATS, POINT_NORMAL_FLOATS = 4, 8, 12

# coarse ICP (include/bev_mi355x.h): bev_icp_result_t, bev_match_t and the convergence states
ICP_RESULT_DTYPE = np.dtype([("T", "<f4", (16,)), ("fitness", "<f8"), ("converged", "<i4"), ("iterations", "<i4"),
                             ("state", "<i4"), ("_pad", "<i4")])
MATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("match_idx", "<i4"), ("angle_guess", "<f4")])
ICP_NOT_CONVERGED, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES = range(6)


class IcpParams(C.Structure):
    """bev_icp_params_t"""
    _fields_ = [("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("max_iterations", C.c_int32), ("_pad", C.c_int32)]


def icp_params(max_correspondence_distance=10.0, max_iterations=10, transformation_epsilon=0.0,
               euclidean_fitness_epsilon=-1.7976931348623157e308) -> IcpParams:
    """The coarse defaults of the registration tools (bev_icp_coarse_defaults), any of them overridden."""
    return IcpParams(max_correspondence_distance, transformation_epsilon, euclidean_fitness_epsilon, max_iterations, 0)


# place retrieval (include/bev_mi355x.h): bev_place_hit_t, whose first twelve bytes are a MATCH_DTYPE record
PLACE_HIT_DTYPE = np.dtype([("query_idx", "<i4"), ("match_idx", "<i4"), ("angle_guess", "<f4"), ("shift", "<i4"),
                            ("distance", "<f8")])
PLACE_MAX_TOP_K = 64  # BEV_PLACE_MAX_TOP_K


class PlaceParams(C.Structure):
    """bev_place_params_t"""
    _fields_ = [("n_rings", C.c_int32), ("n_sectors", C.c_int32), ("max_range", C.c_float), ("skip_label0", C.c_int32)]


def place_params(n_rings=20, n_sectors=60, max_range=80.0, skip_label0=True) -> PlaceParams:
    """The defaults of place retrieval (bev_place_defaults), any of them overridden."""
    return PlaceParams(n_rings, n_sectors, max_range, 1 if skip_label0 else 0)


# verification of registered matches (include/bev_mi355x.h): bev_verify_result_t
VERIFY_MAX_THRESHOLDS = 8  # BEV_VERIFY_MAX_THRESHOLDS
VERIFY_RESULT_DTYPE = np.dtype([("n_query", "<u4"), ("n_target", "<u4"), ("query_within", "<u4", (8,)),
                                ("target_within", "<u4", (8,))])


class VerifyParams(C.Structure):
    """bev_verify_params_t"""
    _fields_ = [("leaf", C.c_float), ("n_thresholds", C.c_int32), ("threshold", C.c_float * 8)]


def verify_params(thresholds=(0.1, 0.2, 0.5, 1.0), leaf=0.2) -> VerifyParams:
    """The defaults of the verification calls (bev_verify_defaults), either of them overridden.  More than 8 thresholds: the
    first 8 go into the record and n_thresholds says how many were given, which the calls refuse."""
    t = [float(v) for v in thresholds]
    return VerifyParams(leaf, len(t), (C.c_float * 8)(*t[:8]))


# translation guess of retrieved pairs (include/bev_mi355x.h): bev_align_detail_t
ALIGN_DETAIL_DTYPE = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("k", "<i4"), ("flip", "<i4"), ("score", "<u4"), ("eq", "<u4"),
                               ("ec", "<u4"), ("off_x", "<f4"), ("off_y", "<f4")])


class AlignParams(C.Structure):
    """bev_align_params_t"""
    _fields_ = [("grid", C.c_int32), ("cell", C.c_float), ("max_shift", C.c_int32), ("yaw_steps", C.c_int32),
                ("yaw_step", C.c_float), ("skip_label0", C.c_int32)]


def align_params(grid=128, cell=0.5, max_shift=16, yaw_steps=1, yaw_step=2.0, skip_label0=True) -> AlignParams:
    """The defaults of the translation guess (bev_align_defaults), any of them overridden."""
    return AlignParams(grid, cell, max_shift, yaw_steps, yaw_step, 1 if skip_label0 else 0)


def load_lib() -> C.CDLL:
    """Load libbev_mi355x.so; raise if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two
    # HIP runtimes in one process cannot both open the GPU.  Importing torch FIRST
    # makes the dynamic linker resolve our NEEDED libamdhip64.so.7 to the copy torch
    # already loaded (same SONAME), so the process has exactly one runtime.
    import sys
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not LIB_PATH.exists():
        raise BevError(
            f"{LIB_PATH} is missing: build it with __graft_entry__.build() or "
            f"`make -C {PKG_DIR}`. There is no CPU/Python fallback for the hot path."
        )
    lib = C.CDLL(str(LIB_PATH))
    vp, i32, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    lib.bev_params_for_sensor.argtypes = [C.c_char_p, C.POINTER(BevParams)]
    lib.bev_num_slots.argtypes = [C.POINTER(BevParams)]
    lib.bev_num_slots.restype = sz
    lib.bev_multi_bytes.argtypes = [C.POINTER(BevParams)]
    lib.bev_multi_bytes.restype = sz
    lib.bev_single_bytes.argtypes = [C.POINTER(BevParams)]
    lib.bev_single_bytes.restype = sz
    lib.bev_create.argtypes = [C.POINTER(vp), i32, C.POINTER(BevParams), i32, sz]
    lib.bev_destroy.argtypes = [vp]
    lib.bev_destroy.restype = None
    lib.bev_strerror.argtypes = [i32]
    lib.bev_strerror.restype = C.c_char_p
    lib.bev_last_error.argtypes = [vp]
    lib.bev_last_error.restype = C.c_char_p
    lib.bev_process_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp),
                                      C.POINTER(vp), C.POINTER(vp)]
    lib.bev_process_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), vp, vp, vp, vp]
    lib.bev_synchronize.argtypes = [vp]
    lib.bev_order_cloud.argtypes = [vp, vp, u32, vp]
    lib.bev_mark_ground.argtypes = [vp, vp, vp]
    lib.bev_multi_bev.argtypes = [vp, vp, u32, vp]
    lib.bev_single_bev.argtypes = [vp, vp, u32, vp]
    lib.bev_float_bev.argtypes = [vp, vp, u32, C.c_float, i32, vp]
    lib.bev_float_bev_size.argtypes = [C.c_float]
    lib.bev_float_bev_size.restype = sz
    lib.bev_project_xyzi.argtypes = [vp, i32, vp, u32, vp]
    lib.bev_transform_cloud.argtypes = [vp, vp, u32, vp, vp]
    lib.bev_yaw_translate_matrix.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, vp]
    lib.bev_yaw_translate_matrix.restype = None
    lib.bev_host_alloc.argtypes = [C.POINTER(vp), sz]
    lib.bev_host_free.argtypes = [vp]
    lib.bev_project_out_points.argtypes = [i32, u32]
    lib.bev_project_out_points.restype = C.c_size_t
    lib.bev_set_lanes.argtypes = [vp, i32]
    try:  # (an older build of the library, selected with BEV_AMD_LIB for a same-box A/B: scripts/ab_libs.sh)
        lib.bev_set_layout_hint.argtypes = [vp, i32]
    except AttributeError:
        pass
    lib.bev_profile_enable.argtypes = [vp, i32]
    lib.bev_profile_reset.argtypes = [vp]
    lib.bev_profile_get.argtypes = [vp, C.POINTER(KernelStat), i32]
    lib.bev_debug_get_cell_avg.argtypes = [vp, i32, i32, vp]
    lib.bev_debug_get_frame_info.argtypes = [vp, i32, i32, vp]
    if hasattr(lib, "bev_debug_get_code_overflow"):  # (absent from older builds selected through BEV_AMD_LIB for A/B runs)
        lib.bev_debug_get_code_overflow.argtypes = [vp, i32, i32, vp]
    lib.bev_debug_angle_predicate.argtypes = [vp, vp, vp, vp, vp, sz]
    if hasattr(lib, "bev_debug_exact_eval"):  # (absent from older builds selected through BEV_AMD_LIB)
        lib.bev_debug_exact_eval.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp]
    lib.bev_abi_version.restype = i32
    if hasattr(lib, "bev_registration_front_device_resident"):  # (absent from older builds selected through BEV_AMD_LIB)
        lib.bev_top_part_flatten.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
        lib.bev_voxel_grid_xyz.argtypes = [vp, vp, u32, C.c_float, vp, C.POINTER(u32)]
        lib.bev_normals_2d.argtypes = [vp, vp, u32, i32, C.c_float, vp, vp]
        lib.bev_registration_front_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, C.c_float,
                                                               vp, vp, sz, vp]
        lib.bev_regfront_max_out.argtypes = [sz]
        lib.bev_regfront_max_out.restype = sz
    if hasattr(lib, "bev_coarse_registration_device_resident"):
        lib.bev_icp_coarse_defaults.argtypes = []
        lib.bev_icp_coarse_defaults.restype = IcpParams
        lib.bev_icp_point_to_plane.argtypes = [vp, vp, u32, vp, u32, vp, C.POINTER(IcpParams), vp]
        lib.bev_coarse_registration_device_resident.argtypes = [vp, i32, vp, sz, vp, i32, vp, C.POINTER(IcpParams), vp, vp]
    if hasattr(lib, "bev_fine_registration_device_resident"):
        lib.bev_voxel_grid_irct.argtypes = [vp, vp, u32, C.c_float, vp, C.POINTER(u32)]
        lib.bev_icp_fine_defaults.argtypes = lib.bev_icp_whole_defaults.argtypes = []
        lib.bev_icp_fine_defaults.restype = lib.bev_icp_whole_defaults.restype = IcpParams
        lib.bev_icp_point_to_point.argtypes = [vp, vp, u32, vp, u32, vp, C.POINTER(IcpParams), vp]
        lib.bev_fine_registration_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, i32, vp, vp,
                                                              vp, C.POINTER(IcpParams), vp]
    if hasattr(lib, "bev_project_device_resident"):
        lib.bev_project_device_resident.argtypes = [vp, i32, i32, vp, C.POINTER(C.c_uint64), vp]
        lib.bev_project_batch_out_points.argtypes = [i32, i32, C.POINTER(C.c_uint64)]
        lib.bev_project_batch_out_points.restype = sz
        lib.bev_process_batch_xyzi.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(vp),
                                               C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, "bev_float_bev_device_resident"):
        lib.bev_float_bev_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, i32, i32, vp, vp]
        lib.bev_float_bev_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.c_float, i32, i32, vp, C.POINTER(vp)]
    if hasattr(lib, "bev_posed_bev_device_resident"):
        lib.bev_posed_bev_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, vp, vp, vp]
        lib.bev_posed_bev_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), i32, vp, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, "bev_submap_bev_device_resident"):
        lib.bev_submap_bev_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, C.POINTER(C.c_uint64), vp, vp, vp, vp]
        lib.bev_submap_bev_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), i32, C.POINTER(C.c_uint64), vp, vp,
                                             C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, "bev_submap_float_bev_device_resident"):
        lib.bev_submap_float_bev_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, i32, i32,
                                                             C.POINTER(C.c_uint64), vp, vp, vp]
        lib.bev_submap_float_bev_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.c_float, i32, i32,
                                                   C.POINTER(C.c_uint64), vp, vp, C.POINTER(vp)]
    if hasattr(lib, "bev_submap_registration_device_resident"):
        lib.bev_submap_registration_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, i32,
                                                                C.POINTER(C.c_uint64), vp, vp, i32, vp, vp, vp,
                                                                C.POINTER(IcpParams), vp]
        lib.bev_submap_registration_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.c_float, i32,
                                                      C.POINTER(C.c_uint64), vp, vp, i32, vp, C.POINTER(IcpParams), vp]
    if hasattr(lib, "bev_submap_voxel_registration_device_resident"):
        lib.bev_submap_voxel_registration_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, C.c_float,
                                                                      i32, C.POINTER(C.c_uint64), vp, vp, i32, vp, vp, vp,
                                                                      C.POINTER(IcpParams), vp]
        lib.bev_submap_voxel_registration_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.c_float, C.c_float, i32,
                                                            C.POINTER(C.c_uint64), vp, vp, i32, vp, C.POINTER(IcpParams), vp]
        lib.bev_submap_voxel_cloud_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, C.c_float, i32,
                                                               C.POINTER(C.c_uint64), vp, vp, C.c_uint64, vp, vp]
    if hasattr(lib, "bev_submap_coarse_registration_device_resident"):
        lib.bev_submap_coarse_registration_device_resident.argtypes = [vp, i32, vp, sz, vp, i32, C.POINTER(C.c_uint64), vp, vp,
                                                                       i32, vp, C.POINTER(IcpParams), vp, vp]
    if hasattr(lib, "bev_submap_coarse_voxel_registration_device_resident"):
        lib.bev_submap_coarse_voxel_registration_device_resident.argtypes = [vp, i32, vp, sz, vp, C.c_float, C.c_float, vp, i32,
                                                                             C.POINTER(C.c_uint64), vp, vp, i32, vp,
                                                                             C.POINTER(IcpParams), vp, vp]
        lib.bev_submap_pn_cloud_device_resident.argtypes = [vp, i32, vp, sz, vp, C.c_float, C.c_float, vp, i32,
                                                            C.POINTER(C.c_uint64), vp, vp, C.c_uint64, vp, vp]
    if hasattr(lib, "bev_submap_top_part_cloud_device_resident"):
        lib.bev_submap_top_part_cloud_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), C.c_float, C.c_float, vp,
                                                                  i32, C.POINTER(C.c_uint64), vp, vp, C.c_uint64, vp, vp]
        lib.bev_submap_top_part_coarse_registration_device_resident.argtypes = [
            vp, i32, vp, C.POINTER(C.c_uint64), vp, sz, vp, C.c_float, C.c_float, vp, i32, C.POINTER(C.c_uint64), vp, vp, i32, vp,
            C.POINTER(IcpParams), vp, vp]
        lib.bev_submap_top_part_max_out.argtypes = [sz]
        lib.bev_submap_top_part_max_out.restype = sz
    if hasattr(lib, "bev_set_submap_search_grid"):
        lib.bev_set_submap_search_grid.argtypes = [vp, i32, i32]
        lib.bev_debug_get_submap_grid.argtypes = [vp, i32, i32, i32, vp]
    if hasattr(lib, "bev_set_pair_search_grid"):
        lib.bev_set_pair_search_grid.argtypes = [vp, i32, i32]
        lib.bev_debug_get_pair_grid.argtypes = [vp, i32, i32, i32, vp]
    if hasattr(lib, "bev_place_match_device_resident"):
        lib.bev_place_defaults.argtypes = []
        lib.bev_place_defaults.restype = PlaceParams
        lib.bev_place_descriptor_bytes.argtypes = lib.bev_place_desc_handle_bytes.argtypes = [C.POINTER(PlaceParams)]
        lib.bev_place_descriptor_bytes.restype = lib.bev_place_desc_handle_bytes.restype = sz
        lib.bev_place_descriptor_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, vp, vp, vp,
                                                             C.POINTER(PlaceParams), vp, vp]
        lib.bev_place_match_device_resident.argtypes = [vp, C.POINTER(PlaceParams), i32, vp, i32, vp, vp, i32, vp]
        lib.bev_place_retrieval_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), i32, vp, vp, vp,
                                                  C.POINTER(PlaceParams), vp, i32, vp]
    if hasattr(lib, "bev_verify_registration_device_resident"):
        lib.bev_verify_defaults.argtypes = []
        lib.bev_verify_defaults.restype = VerifyParams
        lib.bev_verify_clouds.argtypes = [vp, vp, u32, vp, u32, vp, C.POINTER(VerifyParams), vp]
        lib.bev_verify_registration_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, vp, vp,
                                                                C.POINTER(VerifyParams), vp]
        lib.bev_submap_verify_registration_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32,
                                                                       C.POINTER(C.c_uint64), vp, vp, C.c_float, i32, vp, vp,
                                                                       C.POINTER(VerifyParams), vp]
        lib.bev_verify_registration_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), i32, vp, vp,
                                                      C.POINTER(VerifyParams), vp]
    if hasattr(lib, "bev_align_hits_device_resident"):
        lib.bev_align_defaults.argtypes = []
        lib.bev_align_defaults.restype = AlignParams
        lib.bev_align_grid_bytes.argtypes = [C.POINTER(AlignParams)]
        lib.bev_align_grid_bytes.restype = sz
        lib.bev_align_grid_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, vp, vp, vp,
                                                       C.POINTER(AlignParams), vp, vp]
        lib.bev_align_hits_device_resident.argtypes = [vp, i32, vp, C.POINTER(C.c_uint64), i32, vp, vp, i32, vp,
                                                       C.POINTER(AlignParams), vp, vp, vp]
        lib.bev_align_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), i32, vp, vp, vp, i32, vp,
                                        C.POINTER(AlignParams), vp, vp, vp]
    _lib = lib
    return lib


def params_for_sensor(sensor: str) -> BevParams:
    p = BevParams()
    rc = load_lib().bev_params_for_sensor(sensor.encode(), C.byref(p))
    if rc != 0:
        raise BevError(f"unknown sensor type {sensor!r}")
    return p


def _ptr(a: np.ndarray | None) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(None)


def _offsets(offsets, n_frames):
    """the n_frames + 1 offsets of packed frames as the C ABI takes them: (contiguous uint64 array, its pointer)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert offsets.shape[0] == n_frames + 1
    return offsets, offsets.ctypes.data_as(C.POINTER(C.c_uint64))


def _host_clouds(clouds, dtype=POINT_DTYPE, per=1):
    """host clouds as the batched calls take them: (the contiguous clouds, to be kept alive; their void* array, None for an
    empty cloud; their uint32 counts of items of `per` elements)"""
    clouds = [np.ascontiguousarray(f, dtype=dtype).reshape(-1) for f in clouds]
    n = max(len(clouds), 1)
    return (clouds, (C.c_void_p * n)(*[f.ctypes.data if f.size >= per else None for f in clouds]),
            (C.c_uint32 * n)(*[f.size // per for f in clouds]))


def _rows(out):
    """the void* array of an output's rows (one per frame or map); None when the output is not wanted"""
    return (C.c_void_p * max(len(out), 1))(*[row.ctypes.data for row in out]) if out is not None else None


class BevContext:
    """One context per GPU (bev_create / bev_destroy)."""

    def __init__(self, params: BevParams, device: int = 0, max_batch: int = 8, max_points: int | None = None):
        self.lib = load_lib()
        self.params = params
        self.S = params.slots
        self.M = params.mat_size
        self.L = params.n_layers
        self.max_batch = max_batch
        self.max_points = int(max_points if max_points is not None else self.S + 8192)
        self._h = C.c_void_p(None)
        rc = self.lib.bev_create(C.byref(self._h), device, C.byref(params), max_batch, self.max_points)
        if rc != 0:
            raise BevError(f"bev_create failed: {self.lib.bev_strerror(rc).decode()} (status {rc})")

    def close(self):
        if self._h:
            self.lib.bev_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.bev_strerror(rc).decode()
            detail = self.lib.bev_last_error(self._h).decode() if self._h else ""
            raise BevError(f"{what} failed: {msg} (status {rc}) {detail}")

    # ---- whole hot path, host buffers ---------------------------------
    def _batch_outputs(self, n, want_multi, want_single, want_ground_mat):
        """the four outputs of process_batch / process_batch_xyzi for n frames, None for those that are not wanted"""
        ordered = np.empty((n, self.S), dtype=POINT_DTYPE)
        multi = np.empty((n, self.L, self.M, self.M), dtype=np.uint8) if want_multi else None
        single = np.empty((n, self.M, self.M), dtype=np.uint8) if want_single else None
        gm = np.empty((n, self.params.n_scan, self.params.horizon_scan), dtype=np.int8) if want_ground_mat else None
        return ordered, multi, single, gm

    def process_batch(self, frames, want_multi=True, want_single=True, want_ground_mat=False):
        frames, pts, npts = _host_clouds(frames)
        out = self._batch_outputs(len(frames), want_multi, want_single, want_ground_mat)
        rc = self.lib.bev_process_batch(self._h, len(frames), pts, npts, *[_rows(o) for o in out])
        self._check(rc, "bev_process_batch")
        return out

    def process_batch_xyzi(self, kind: int, frames, want_multi=True, want_single=True, want_ground_mat=False):
        """process_batch on raw returns (bev_process_batch_xyzi): frames[f] is what project_xyzi(kind, .) takes; the
        outputs are those of process_batch on the projected clouds."""
        frames, raw, nret = _host_clouds(frames, np.float32, 4)
        out = self._batch_outputs(len(frames), want_multi, want_single, want_ground_mat)
        rc = self.lib.bev_process_batch_xyzi(self._h, kind, len(frames), raw, nret, *[_rows(o) for o in out])
        self._check(rc, "bev_process_batch_xyzi")
        return out

    # ---- whole hot path, device pointers --------------------------------
    def process_device(self, n_frames, d_pts, offsets, d_ordered, d_multi, d_single, d_ground_mat=None):
        offsets, offs = _offsets(offsets, n_frames)
        rc = self.lib.bev_process_device_resident(
            self._h, n_frames, C.c_void_p(d_pts), offs,
            C.c_void_p(d_ordered), C.c_void_p(d_multi), C.c_void_p(d_single), C.c_void_p(d_ground_mat))
        self._check(rc, "bev_process_device_resident")

    def project_device(self, kind, n_frames, d_xyzi, offsets, d_out):
        """bev_project_device_resident on device pointers: frame f = returns [offsets[f], offsets[f + 1]) of d_xyzi; kinds
        0 / 1 write records at the same offsets of d_out, KITTI frame f's structured cloud at f * KITTI_SLOTS.
        Asynchronous: a process_device behind it reads finished records; synchronize() before the host reads d_out."""
        offsets, offs = _offsets(offsets, n_frames)
        rc = self.lib.bev_project_device_resident(self._h, kind, n_frames, C.c_void_p(d_xyzi), offs, C.c_void_p(d_out))
        self._check(rc, "bev_project_device_resident")

    def synchronize(self):
        self._check(self.lib.bev_synchronize(self._h), "bev_synchronize")

    # ---- per-function entry points ---------------------------------------
    def order_cloud(self, pts):
        pts = np.ascontiguousarray(pts, dtype=POINT_DTYPE)
        out = np.empty(self.S, dtype=POINT_DTYPE)
        self._check(self.lib.bev_order_cloud(self._h, _ptr(pts) if len(pts) else None, len(pts), _ptr(out)),
                    "bev_order_cloud")
        return out

    def mark_ground(self, ordered, want_ground_mat=True):
        cloud = np.array(ordered, dtype=POINT_DTYPE, copy=True)
        assert cloud.shape == (self.S,)
        gm = np.empty((self.params.n_scan, self.params.horizon_scan), dtype=np.int8) if want_ground_mat else None
        self._check(self.lib.bev_mark_ground(self._h, _ptr(cloud), _ptr(gm)), "bev_mark_ground")
        return cloud, gm

    def multi_bev(self, cloud):
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        out = np.empty((self.L, self.M, self.M), dtype=np.uint8)
        self._check(self.lib.bev_multi_bev(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), _ptr(out)),
                    "bev_multi_bev")
        return out

    def single_bev(self, cloud):
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        out = np.empty((self.M, self.M), dtype=np.uint8)
        self._check(self.lib.bev_single_bev(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), _ptr(out)),
                    "bev_single_bev")
        return out

    def float_bev(self, cloud, interval=1.0, skip_label0=True):
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        M = int(self.lib.bev_float_bev_size(interval))
        out = np.empty((M, M), dtype=np.float32)
        self._check(self.lib.bev_float_bev(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), interval,
                                           1 if skip_label0 else 0, _ptr(out)), "bev_float_bev")
        return out

    def _poses(self, poses, n_frames):
        """(n_frames, n_poses, 12) float32 or None -> (n_poses, array or None)"""
        if poses is None:
            return 0, None
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(n_frames, -1, 12)
        return poses.shape[1], (poses if poses.shape[1] else None)

    def float_bev_device(self, n_frames, d_clouds, offsets, d_out, interval=1.0, skip_label0=True, poses=None):
        """bev_float_bev_device_resident on device pointers: frame f = records [offsets[f], offsets[f + 1]) of d_clouds;
        poses: None, or (n_frames, n_poses, 12) host floats (row-major 3 x 4, yaw_translate_matrix); d_out receives
        n_frames * max(1, n_poses) grids of M * M floats.  Asynchronous: synchronize() before the host reads d_out."""
        offsets, offs = _offsets(offsets, n_frames)
        n_poses, poses = self._poses(poses, n_frames)
        rc = self.lib.bev_float_bev_device_resident(self._h, n_frames, C.c_void_p(d_clouds), offs, interval,
                                                    1 if skip_label0 else 0, n_poses, _ptr(poses), C.c_void_p(d_out))
        self._check(rc, "bev_float_bev_device_resident")

    def float_bev_batch(self, clouds, interval=1.0, skip_label0=True, poses=None):
        """bev_float_bev_batch on host clouds; returns (n_frames, max(1, n_poses), M, M) float32."""
        clouds, pts, npts = _host_clouds(clouds)
        n = len(clouds)
        n_poses, poses = self._poses(poses, n)
        M = int(self.lib.bev_float_bev_size(interval))
        out = np.empty((n, max(1, n_poses), M, M), dtype=np.float32)
        rc = self.lib.bev_float_bev_batch(self._h, n, pts, npts, interval, 1 if skip_label0 else 0, n_poses, _ptr(poses),
                                          _rows(out))
        self._check(rc, "bev_float_bev_batch")
        return out

    def posed_bev_device(self, n_frames, d_clouds, offsets, d_multi, d_single, poses=None):
        """bev_posed_bev_device_resident on device pointers: frame f = records [offsets[f], offsets[f + 1]) of d_clouds;
        poses: None, or (n_frames, n_poses, 12) host floats; d_multi / d_single (0 or None: not wanted) receive
        n_frames * max(1, n_poses) images of L * M * M / M * M bytes.  Asynchronous: synchronize() before the host reads them."""
        offsets, offs = _offsets(offsets, n_frames)
        n_poses, poses = self._poses(poses, n_frames)
        rc = self.lib.bev_posed_bev_device_resident(self._h, n_frames, C.c_void_p(d_clouds), offs, n_poses, _ptr(poses),
                                                    C.c_void_p(d_multi or None), C.c_void_p(d_single or None))
        self._check(rc, "bev_posed_bev_device_resident")

    def posed_bev_batch(self, clouds, poses=None, want_multi=True, want_single=True):
        """bev_posed_bev_batch on host clouds; returns (multi, single): (n_frames, max(1, n_poses), L, M, M) and
        (n_frames, max(1, n_poses), M, M) uint8, None for the one that is not wanted."""
        clouds, pts, npts = _host_clouds(clouds)
        n = len(clouds)
        n_poses, poses = self._poses(poses, n)
        K = max(1, n_poses)
        multi = np.empty((n, K, self.L, self.M, self.M), dtype=np.uint8) if want_multi else None
        single = np.empty((n, K, self.M, self.M), dtype=np.uint8) if want_single else None
        rc = self.lib.bev_posed_bev_batch(self._h, n, pts, npts, n_poses, _ptr(poses), _rows(multi), _rows(single))
        self._check(rc, "bev_posed_bev_batch")
        return multi, single

    @staticmethod
    def _submap_entries(map_offsets, entry_frame, entry_pose):
        """the three host arrays of a submap call, contiguous: (n_maps, offsets, frames or None, matrices or None)"""
        map_offsets = np.ascontiguousarray(map_offsets, dtype=np.uint64)
        entry_frame = np.ascontiguousarray(entry_frame, dtype=np.int32).reshape(-1)
        entry_pose = np.ascontiguousarray(entry_pose, dtype=np.float32).reshape(-1, 12)
        assert map_offsets.ndim == 1 and len(map_offsets) >= 1 and len(entry_frame) == len(entry_pose)
        assert len(entry_frame) >= int(map_offsets.max())
        return len(map_offsets) - 1, map_offsets, (entry_frame if len(entry_frame) else None), (entry_pose if len(entry_pose) else None)

    def submap_bev_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, d_multi, d_single):
        """bev_submap_bev_device_resident on device pointers: frame f = records [offsets[f], offsets[f + 1]) of d_clouds; map g
        = entries [map_offsets[g], map_offsets[g + 1]), entry e = frame entry_frame[e] under the row-major 3 x 4 matrix
        entry_pose[e] (12 floats); d_multi / d_single (0 or None: not wanted) receive one image of L * M * M / M * M bytes
        per map: the rasters of all its entries' moved clouds together.  Asynchronous: synchronize() before the host reads
        them."""
        offsets, offs = _offsets(offsets, n_frames)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        rc = self.lib.bev_submap_bev_device_resident(self._h, n_frames, C.c_void_p(d_clouds), offs, n_maps,
                                                     map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame),
                                                     _ptr(entry_pose), C.c_void_p(d_multi or None), C.c_void_p(d_single or None))
        self._check(rc, "bev_submap_bev_device_resident")

    def submap_bev_batch(self, clouds, map_offsets, entry_frame, entry_pose, want_multi=True, want_single=True):
        """bev_submap_bev_batch on host clouds; maps as for submap_bev_device; returns (multi, single): (n_maps, L, M, M) and
        (n_maps, M, M) uint8, None for the one that is not wanted."""
        clouds, pts, npts = _host_clouds(clouds)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        multi = np.empty((n_maps, self.L, self.M, self.M), dtype=np.uint8) if want_multi else None
        single = np.empty((n_maps, self.M, self.M), dtype=np.uint8) if want_single else None
        rc = self.lib.bev_submap_bev_batch(self._h, len(clouds), pts, npts, n_maps,
                                           map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame),
                                           _ptr(entry_pose), _rows(multi), _rows(single))
        self._check(rc, "bev_submap_bev_batch")
        return multi, single

    def submap_float_bev_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, d_out, interval=1.0,
                                skip_label0=True):
        """bev_submap_float_bev_device_resident on device pointers: frames, maps and entries as for submap_bev_device; d_out
        receives one grid of M * M floats per map: the float BEV of all its entries' moved clouds together.  Asynchronous:
        synchronize() before the host reads d_out."""
        offsets, offs = _offsets(offsets, n_frames)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        rc = self.lib.bev_submap_float_bev_device_resident(self._h, n_frames, C.c_void_p(d_clouds), offs, interval,
                                                           1 if skip_label0 else 0, n_maps,
                                                           map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame),
                                                           _ptr(entry_pose), C.c_void_p(d_out or None))
        self._check(rc, "bev_submap_float_bev_device_resident")

    def submap_float_bev_batch(self, clouds, map_offsets, entry_frame, entry_pose, interval=1.0, skip_label0=True):
        """bev_submap_float_bev_batch on host clouds; maps as for submap_bev_device; returns (n_maps, M, M) float32."""
        clouds, pts, npts = _host_clouds(clouds)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        M = int(self.lib.bev_float_bev_size(interval))
        out = np.empty((n_maps, M, M), dtype=np.float32)
        rc = self.lib.bev_submap_float_bev_batch(self._h, len(clouds), pts, npts, interval, 1 if skip_label0 else 0, n_maps,
                                                 map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame),
                                                 _ptr(entry_pose), _rows(out))
        self._check(rc, "bev_submap_float_bev_batch")
        return out

    def place_descriptor_device(self, n_frames, d_clouds, offsets, d_desc, d_units, params: PlaceParams | None = None,
                                map_offsets=None, entry_frame=None, entry_pose=None):
        """bev_place_descriptor_device_resident on device pointers: frames as for float_bev_device; without map_offsets one
        descriptor per frame from its raw coordinates, else one per map (maps and entries as for submap_bev_device).  d_desc
        (0 or None: not wanted) receives place_descriptor_bytes(params) per descriptor, d_units (0 or None: not wanted) one
        record of place_desc_handle_bytes(params), 64-byte aligned.  Asynchronous: synchronize() before the host reads them."""
        offsets, offs = _offsets(offsets, n_frames)
        prm = params if params is not None else place_params()
        n_maps, mo, ef, ep = 0, None, None, None
        if map_offsets is not None:
            n_maps, mo, ef, ep = self._submap_entries(map_offsets, entry_frame, entry_pose)
        rc = self.lib.bev_place_descriptor_device_resident(self._h, n_frames, C.c_void_p(d_clouds), offs, n_maps, _ptr(mo), _ptr(ef),
                                                           _ptr(ep), C.byref(prm), C.c_void_p(d_desc or None),
                                                           C.c_void_p(d_units or None))
        self._check(rc, "bev_place_descriptor_device_resident")

    def place_match_device(self, n_queries, d_units_q, n_db, d_units_db, d_hits, top_k=1, limit=None,
                           params: PlaceParams | None = None):
        """bev_place_match_device_resident on device pointers: the best top_k candidates of every query among candidates
        0 .. limit[q] - 1 (None: all n_db) of the database; d_hits receives n_queries * top_k PLACE_HIT_DTYPE records, a query's
        in rank order.  Asynchronous: synchronize() before the host reads d_hits."""
        prm = params if params is not None else place_params()
        lim = np.ascontiguousarray(limit, dtype=np.int32) if limit is not None else None
        assert lim is None or lim.shape == (n_queries,)
        rc = self.lib.bev_place_match_device_resident(self._h, C.byref(prm), n_queries, C.c_void_p(d_units_q or None), n_db,
                                                      C.c_void_p(d_units_db or None), _ptr(lim), top_k, C.c_void_p(d_hits or None))
        self._check(rc, "bev_place_match_device_resident")

    def place_retrieval_batch(self, clouds, top_k=1, limit=None, params: PlaceParams | None = None, map_offsets=None,
                              entry_frame=None, entry_pose=None):
        """bev_place_retrieval_batch on host clouds: every frame a query, the database the maps (maps and entries as for
        submap_bev_device) or, without map_offsets, the frames themselves; returns (n_frames, top_k) PLACE_HIT_DTYPE records."""
        clouds, pts, npts = _host_clouds(clouds)
        prm = params if params is not None else place_params()
        n_maps, mo, ef, ep = 0, None, None, None
        if map_offsets is not None:
            n_maps, mo, ef, ep = self._submap_entries(map_offsets, entry_frame, entry_pose)
        lim = np.ascontiguousarray(limit, dtype=np.int32) if limit is not None else None
        assert lim is None or lim.shape == (len(clouds),)
        hits = np.zeros((len(clouds), top_k), dtype=PLACE_HIT_DTYPE)
        rc = self.lib.bev_place_retrieval_batch(self._h, len(clouds), pts, npts, n_maps, _ptr(mo), _ptr(ef), _ptr(ep),
                                                C.byref(prm), _ptr(lim), top_k, _ptr(hits))
        self._check(rc, "bev_place_retrieval_batch")
        return hits

    def transform_cloud(self, cloud, m):
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        m = np.ascontiguousarray(m, dtype=np.float32).reshape(12)
        out = np.empty_like(cloud)
        self._check(self.lib.bev_transform_cloud(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), _ptr(m),
                                                 _ptr(out) if len(cloud) else None), "bev_transform_cloud")
        return out

    def project_xyzi(self, kind: int, xyzi):
        """kind 0: MulRan/Ouster (n, 4) interleaved; kind 1: Oxford (4, n) planes; kind 2: KITTI (n, 4)
        interleaved, returns the structured 64 * 2083 cloud."""
        xyzi = np.ascontiguousarray(xyzi, dtype=np.float32)
        n = xyzi.size // 4
        n_out = int(self.lib.bev_project_out_points(kind, n))
        out = np.empty(n_out, dtype=POINT_DTYPE)
        self._check(self.lib.bev_project_xyzi(self._h, kind, _ptr(xyzi) if n else None, n, _ptr(out) if n_out else None),
                    "bev_project_xyzi")
        return out

    # ---- registration front end (DESIGN.md "Registration front end") ------------------------------------------
    def top_part_flatten(self, cloud):
        """extractTopAndFlatten: (m, 4) float32 PointXYZ rows (x, y, 0, 0)."""
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        out = np.zeros((regfront_max_out(len(cloud)), XYZ_FLOATS), dtype=np.float32)
        m = C.c_uint32(0)
        self._check(self.lib.bev_top_part_flatten(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), _ptr(out),
                                                  C.byref(m)), "bev_top_part_flatten")
        return out[: m.value].copy()

    def voxel_grid(self, xyz, leaf=0.2):
        """pcl::VoxelGrid<PointXYZ> with one leaf size: xyz is (n, 4) or (n, 3) float32; returns (v, 4) centroids."""
        xyz = _xyz4(xyz)
        out = np.zeros((max(len(xyz), 1), XYZ_FLOATS), dtype=np.float32)
        m = C.c_uint32(0)
        self._check(self.lib.bev_voxel_grid_xyz(self._h, _ptr(xyz) if len(xyz) else None, len(xyz), leaf, _ptr(out),
                                                C.byref(m)), "bev_voxel_grid_xyz")
        return out[: m.value].copy()

    def normals_2d(self, xyz, radius=2.0, viewpoint=(0.0, 0.0, 0.0), k_search=0):
        """Normal2dEstimation::compute(PointCloud<Normal>), radius mode: (n, 8) float32 pcl::Normal rows."""
        xyz = _xyz4(xyz)
        out = np.zeros((len(xyz), NORMAL_FLOATS), dtype=np.float32)
        vp = np.asarray(viewpoint, dtype=np.float32).reshape(3)
        self._check(self.lib.bev_normals_2d(self._h, _ptr(xyz) if len(xyz) else None, len(xyz), k_search, radius,
                                            _ptr(vp), _ptr(out) if len(xyz) else None), "bev_normals_2d")
        return out

    def registration_front_device(self, n_frames, d_clouds, offsets, d_out, out_stride, d_counts, leaf=0.2, radius=2.0,
                                  viewpoint=(0.0, 0.0, 0.0)):
        """The chain on device pointers (bev_registration_front_device_resident); offsets None: d_clouds is the d_ordered
        layout (n_frames * S points).  Asynchronous: synchronize() before reading d_out / d_counts."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        vp = np.asarray(viewpoint, dtype=np.float32).reshape(3)
        self._check(self.lib.bev_registration_front_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds), offs, leaf, radius, _ptr(vp), C.c_void_p(d_out), out_stride,
            C.c_void_p(d_counts)), "bev_registration_front_device_resident")

    def registration_front(self, clouds, leaf=0.2, radius=2.0, viewpoint=(0.0, 0.0, 0.0)):
        """The chain on host clouds (uploaded through torch): a list of (k, 12) float32 pcl::PointNormal arrays."""
        import torch

        clouds = [np.ascontiguousarray(c_, dtype=POINT_DTYPE) for c_ in clouds]
        n = len(clouds)
        if n == 0:
            return []
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(c_) for c_ in clouds])
        stride = regfront_max_out(max(len(c_) for c_ in clouds))
        dev = torch.device("cuda", torch.cuda.current_device())
        packed = np.concatenate(clouds) if offs[-1] else np.zeros(1, dtype=POINT_DTYPE)
        d_in = torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(dev)
        d_out = torch.zeros(n * stride * POINT_NORMAL_FLOATS, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        self.registration_front_device(n, d_in.data_ptr(), offs, d_out.data_ptr(), stride, d_cnt.data_ptr(), leaf, radius,
                                       viewpoint)
        self.synchronize()
        out = d_out.cpu().numpy().reshape(n, stride, POINT_NORMAL_FLOATS)
        cnt = d_cnt.cpu().numpy().astype(np.int64)
        return [out[f, : cnt[f]].copy() for f in range(n)]

    # ---- coarse point-to-plane ICP ---------------------------------------------------------------
    def icp_point_to_plane(self, src, tgt, guess=None, params: IcpParams | None = None):
        """One problem: src / tgt are (n, 12) float32 pcl::PointNormal rows, guess a 4 x 4 (None: identity).  Returns one
        ICP_RESULT_DTYPE record."""
        src = _pn12(src)
        tgt = _pn12(tgt)
        g = None if guess is None else np.ascontiguousarray(np.asarray(guess, dtype=np.float32).reshape(16))
        prm = params if params is not None else icp_params()
        out = np.zeros(1, dtype=ICP_RESULT_DTYPE)
        self._check(self.lib.bev_icp_point_to_plane(self._h, _ptr(src) if len(src) else None, len(src),
                                                    _ptr(tgt) if len(tgt) else None, len(tgt),
                                                    _ptr(g) if g is not None else None, C.byref(prm), _ptr(out)),
                    "bev_icp_point_to_plane")
        return out[0]

    def coarse_registration_device(self, n_frames, d_pn, stride, d_counts, matches, d_results, d_best,
                                   params: IcpParams | None = None):
        """bev_coarse_registration_device_resident on device pointers; matches: MATCH_DTYPE records (host).
        Asynchronous: synchronize() before reading d_results (2 ICP_RESULT_DTYPE per match) and d_best (int32)."""
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_params()
        self._check(self.lib.bev_coarse_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_pn), stride, C.c_void_p(d_counts), len(m), _ptr(m) if len(m) else None,
            C.byref(prm), C.c_void_p(d_results), C.c_void_p(d_best)), "bev_coarse_registration_device_resident")

    def coarse_registration(self, pn_clouds, matches, params: IcpParams | None = None):
        """The tool's coarse loop on host clouds (uploaded through torch): pn_clouds is a list of (k, 12) float32
        PointNormal arrays, matches MATCH_DTYPE records or (query_idx, match_idx, angle_guess) tuples.  Returns
        (results (n_matches, 2) ICP_RESULT_DTYPE, best (n_matches,) int32)."""
        import torch

        m = np.array([tuple(r) for r in matches], dtype=MATCH_DTYPE) if not isinstance(matches, np.ndarray) else \
            np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        n = len(m)
        res = np.zeros((n, 2), dtype=ICP_RESULT_DTYPE)
        best = np.zeros(n, dtype=np.int32)
        if n == 0:
            return res, best
        clouds = [_pn12(c_) for c_ in pn_clouds]
        F = len(clouds)
        stride = max([len(c_) for c_ in clouds] + [1])
        packed = np.zeros((F, stride, POINT_NORMAL_FLOATS), dtype=np.float32)
        for f, c_ in enumerate(clouds):
            packed[f, : len(c_)] = c_
        dev = torch.device("cuda", torch.cuda.current_device())
        d_pn = torch.from_numpy(packed.reshape(-1)).to(dev)
        d_cnt = torch.from_numpy(np.array([len(c_) for c_ in clouds], dtype=np.int32)).to(dev)
        d_res = torch.zeros(n * 2 * ICP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_best = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        self.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_res.data_ptr(),
                                        d_best.data_ptr(), params)
        self.synchronize()
        res[:] = d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(n, 2)
        best[:] = d_best.cpu().numpy()
        return res, best

    # ---- fine stage: VoxelGrid<PointXYZIRCT> and point-to-point ICP ---------------------------------
    def voxel_grid_irct(self, cloud, leaf=0.2):
        """pcl::VoxelGrid<PointXYZIRCT> with one leaf size: POINT_DTYPE records in, POINT_DTYPE voxels out."""
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        out = np.zeros(max(len(cloud), 1), dtype=POINT_DTYPE)
        m = C.c_uint32(0)
        self._check(self.lib.bev_voxel_grid_irct(self._h, _ptr(cloud) if len(cloud) else None, len(cloud), leaf,
                                                 _ptr(out), C.byref(m)), "bev_voxel_grid_irct")
        return out[: m.value].copy()

    def icp_point_to_point(self, src, tgt, guess=None, params: IcpParams | None = None):
        """One problem: src / tgt are POINT_DTYPE records (or (n, 3) / (n, 4) float rows: x, y, z), guess a 4 x 4 (None:
        identity), params None: the fine defaults.  Returns one ICP_RESULT_DTYPE record."""
        src, tgt = as_points(src), as_points(tgt)
        g = None if guess is None else np.ascontiguousarray(np.asarray(guess, dtype=np.float32).reshape(16))
        prm = params if params is not None else icp_fine_defaults()
        out = np.zeros(1, dtype=ICP_RESULT_DTYPE)
        self._check(self.lib.bev_icp_point_to_point(self._h, _ptr(src) if len(src) else None, len(src),
                                                    _ptr(tgt) if len(tgt) else None, len(tgt),
                                                    _ptr(g) if g is not None else None, C.byref(prm), _ptr(out)),
                    "bev_icp_point_to_point")
        return out[0]

    def fine_registration_device(self, n_frames, d_clouds, offsets, matches, d_results, d_coarse=None, d_best=None,
                                 leaf=0.2, params: IcpParams | None = None):
        """bev_fine_registration_device_resident on device pointers; offsets None: d_clouds is the d_ordered layout
        (n_frames * S records); d_coarse / d_best: the coarse entry's outputs (top-part tool) or None (whole tool).
        Asynchronous: synchronize() before reading d_results (one ICP_RESULT_DTYPE per match)."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_fine_defaults()
        self._check(self.lib.bev_fine_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds), offs, leaf, len(m), _ptr(m) if len(m) else None,
            C.c_void_p(d_coarse) if d_coarse else None, C.c_void_p(d_best) if d_best else None, C.byref(prm),
            C.c_void_p(d_results)), "bev_fine_registration_device_resident")

    def fine_registration(self, clouds, matches, coarse=None, best=None, leaf=0.2, params: IcpParams | None = None):
        """The fine stage on host clouds (uploaded through torch): clouds is a list of POINT_DTYPE arrays, matches
        MATCH_DTYPE records or (query_idx, match_idx, angle_guess) tuples; coarse / best: the coarse results
        ((n, 2) ICP_RESULT_DTYPE, (n,) int32) whose better transform is the guess, or None (the yaw guess).  Returns
        (n_matches,) ICP_RESULT_DTYPE."""
        import torch

        m = np.array([tuple(r) for r in matches], dtype=MATCH_DTYPE) if not isinstance(matches, np.ndarray) else \
            np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        n = len(m)
        res = np.zeros(n, dtype=ICP_RESULT_DTYPE)
        if n == 0:
            return res
        clouds = [np.ascontiguousarray(c_, dtype=POINT_DTYPE) for c_ in clouds]
        offs = np.zeros(len(clouds) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(c_) for c_ in clouds])
        dev = torch.device("cuda", torch.cuda.current_device())
        packed = np.concatenate(clouds) if offs[-1] else np.zeros(1, dtype=POINT_DTYPE)
        d_in = torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(dev)
        d_res = torch.zeros(n * ICP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_coarse = d_best = None
        if coarse is not None:
            cr = np.ascontiguousarray(coarse, dtype=ICP_RESULT_DTYPE).reshape(-1)
            d_coarse = torch.from_numpy(cr.view(np.uint8).copy()).to(dev)
            d_best = torch.from_numpy(np.ascontiguousarray(best, dtype=np.int32).copy()).to(dev)
        torch.cuda.synchronize()
        self.fine_registration_device(len(clouds), d_in.data_ptr(), offs, m, d_res.data_ptr(),
                                      d_coarse.data_ptr() if d_coarse is not None else None,
                                      d_best.data_ptr() if d_best is not None else None, leaf, params)
        self.synchronize()
        res[:] = d_res.cpu().numpy().view(ICP_RESULT_DTYPE)
        return res

    # ---- scan-to-map fine ICP: frames against submaps ---------------------------------------------
    def submap_registration_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, matches,
                                   d_results, d_coarse=None, d_best=None, leaf=0.2, params: IcpParams | None = None):
        """bev_submap_registration_device_resident on device pointers: frames as for fine_registration_device (offsets None:
        the d_ordered layout), maps and entries as for submap_bev_device; matches: MATCH_DTYPE records (host) whose match_idx
        names a MAP: the query frame's voxel cloud is registered against the map's entries' moved voxel clouds, concatenated
        in the order given.  Asynchronous: synchronize() before reading d_results (one ICP_RESULT_DTYPE per match)."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_fine_defaults()
        self._check(self.lib.bev_submap_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, leaf, n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), len(m),
            _ptr(m) if len(m) else None, C.c_void_p(d_coarse) if d_coarse else None, C.c_void_p(d_best) if d_best else None,
            C.byref(prm), C.c_void_p(d_results or None)), "bev_submap_registration_device_resident")

    def submap_registration_batch(self, clouds, map_offsets, entry_frame, entry_pose, matches, leaf=0.2,
                                  params: IcpParams | None = None):
        """bev_submap_registration_batch on host clouds (yaw guesses); maps as for submap_bev_device, matches MATCH_DTYPE
        records or (query_idx, map index, angle_guess) tuples.  Returns (n_matches,) ICP_RESULT_DTYPE."""
        clouds, pts, npts = _host_clouds(clouds)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.array([tuple(r) for r in matches], dtype=MATCH_DTYPE) if not isinstance(matches, np.ndarray) else \
            np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_fine_defaults()
        res = np.zeros(len(m), dtype=ICP_RESULT_DTYPE)
        self._check(self.lib.bev_submap_registration_batch(
            self._h, len(clouds), pts, npts, leaf, n_maps, map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            _ptr(entry_frame), _ptr(entry_pose), len(m), _ptr(m) if len(m) else None, C.byref(prm),
            _ptr(res) if len(m) else None), "bev_submap_registration_batch")
        return res

    # ---- the same against maps thinned by a voxel grid over their union --------------------------------
    def submap_voxel_registration_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, matches,
                                         d_results, map_leaf, d_coarse=None, d_best=None, leaf=0.2,
                                         params: IcpParams | None = None):
        """bev_submap_voxel_registration_device_resident: submap_registration_device with every map's concatenation thinned
        by a voxel grid of map_leaf over the union (map_leaf 0: no second grid, submap_registration_device's bytes)."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_fine_defaults()
        self._check(self.lib.bev_submap_voxel_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, leaf, map_leaf, n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), len(m),
            _ptr(m) if len(m) else None, C.c_void_p(d_coarse) if d_coarse else None, C.c_void_p(d_best) if d_best else None,
            C.byref(prm), C.c_void_p(d_results or None)), "bev_submap_voxel_registration_device_resident")

    def submap_voxel_registration_batch(self, clouds, map_offsets, entry_frame, entry_pose, matches, map_leaf, leaf=0.2,
                                        params: IcpParams | None = None):
        """bev_submap_voxel_registration_batch on host clouds (yaw guesses): submap_registration_batch with map_leaf.
        Returns (n_matches,) ICP_RESULT_DTYPE."""
        clouds, pts, npts = _host_clouds(clouds)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.array([tuple(r) for r in matches], dtype=MATCH_DTYPE) if not isinstance(matches, np.ndarray) else \
            np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_fine_defaults()
        res = np.zeros(len(m), dtype=ICP_RESULT_DTYPE)
        self._check(self.lib.bev_submap_voxel_registration_batch(
            self._h, len(clouds), pts, npts, leaf, map_leaf, n_maps, map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            _ptr(entry_frame), _ptr(entry_pose), len(m), _ptr(m) if len(m) else None, C.byref(prm),
            _ptr(res) if len(m) else None), "bev_submap_voxel_registration_batch")
        return res

    def submap_voxel_cloud_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, map_leaf,
                                  out_stride, d_out, d_counts, leaf=0.2):
        """bev_submap_voxel_cloud_device_resident: every map's target (map_leaf 0: the concatenation) as x, y, z, 0 float
        rows at d_out + 16 * g * out_stride bytes, its row count at d_counts[g] (uint32).  Asynchronous."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        self._check(self.lib.bev_submap_voxel_cloud_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, leaf, map_leaf, n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), int(out_stride),
            C.c_void_p(d_out or None), C.c_void_p(d_counts or None)), "bev_submap_voxel_cloud_device_resident")

    # ---- scan-to-map coarse ICP: PointNormal frames against submaps ---------------------------------
    def submap_coarse_registration_device(self, n_frames, d_pn, stride, d_counts, map_offsets, entry_frame, entry_pose,
                                          matches, d_results, d_best, params: IcpParams | None = None):
        """bev_submap_coarse_registration_device_resident on device pointers: frames as for coarse_registration_device
        (PointNormal rows, stride, counts), maps and entries as for submap_bev_device; matches: MATCH_DTYPE records (host)
        whose match_idx names a MAP: the query frame is registered point-to-plane, from both yaw guesses, against the map's
        entries' moved rows, concatenated in the order given.  Asynchronous: synchronize() before reading d_results (2
        ICP_RESULT_DTYPE per match) and d_best (int32); both go as they are into the fine calls' d_coarse / d_best."""
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_params()
        self._check(self.lib.bev_submap_coarse_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_pn or None), stride, C.c_void_p(d_counts or None), n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), len(m),
            _ptr(m) if len(m) else None, C.byref(prm), C.c_void_p(d_results or None), C.c_void_p(d_best or None)),
            "bev_submap_coarse_registration_device_resident")

    # ---- the same against maps thinned over their union, normals recomputed ----------------------------
    def submap_coarse_voxel_registration_device(self, n_frames, d_pn, stride, d_counts, map_offsets, entry_frame, entry_pose,
                                                matches, d_results, d_best, pn_leaf, radius=2.0, viewpoint=None,
                                                params: IcpParams | None = None):
        """bev_submap_coarse_voxel_registration_device_resident: submap_coarse_registration_device with every map's
        concatenation thinned by a voxel grid of pn_leaf over the union and its 2-D normals recomputed there (radius,
        viewpoint: three floats, None: the origin).  pn_leaf 0: no grid, submap_coarse_registration_device's bytes."""
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_params()
        vp = np.ascontiguousarray(viewpoint, dtype=np.float32).reshape(3) if viewpoint is not None else None
        self._check(self.lib.bev_submap_coarse_voxel_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_pn or None), stride, C.c_void_p(d_counts or None), pn_leaf, radius, _ptr(vp), n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), len(m),
            _ptr(m) if len(m) else None, C.byref(prm), C.c_void_p(d_results or None), C.c_void_p(d_best or None)),
            "bev_submap_coarse_voxel_registration_device_resident")

    def submap_pn_cloud_device(self, n_frames, d_pn, stride, d_counts, map_offsets, entry_frame, entry_pose, pn_leaf,
                               out_stride, d_out, d_counts_out, radius=2.0, viewpoint=None):
        """bev_submap_pn_cloud_device_resident: every map's target (pn_leaf 0: the concatenation) as PointNormal rows of 12
        floats at d_out + 48 * g * out_stride bytes, its row count at d_counts_out[g] (uint32).  Asynchronous."""
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        vp = np.ascontiguousarray(viewpoint, dtype=np.float32).reshape(3) if viewpoint is not None else None
        self._check(self.lib.bev_submap_pn_cloud_device_resident(
            self._h, n_frames, C.c_void_p(d_pn or None), stride, C.c_void_p(d_counts or None), pn_leaf, radius, _ptr(vp), n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), int(out_stride),
            C.c_void_p(d_out or None), C.c_void_p(d_counts_out or None)), "bev_submap_pn_cloud_device_resident")

    # ---- the same against the thinned top part over the union of a map's moved FULL clouds -------------
    def submap_top_part_cloud_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, pn_leaf,
                                     out_stride, d_out, d_counts_out, radius=2.0, viewpoint=None):
        """bev_submap_top_part_cloud_device_resident: full labelled clouds as for submap_voxel_registration_device (offsets
        None: d_ordered); every map's target, the top part over the union of its entries' moved clouds thinned by pn_leaf with
        its 2-D normals (pn_leaf 0: the top part's rows x y 0 and zeros), as PointNormal rows of 12 floats at
        d_out + 48 * g * out_stride bytes (out_stride >= submap_top_part_max_out of the largest union), its row count at
        d_counts_out[g] (uint32).  Asynchronous."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        vp = np.ascontiguousarray(viewpoint, dtype=np.float32).reshape(3) if viewpoint is not None else None
        self._check(self.lib.bev_submap_top_part_cloud_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, pn_leaf, radius, _ptr(vp), n_maps,
            map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame), _ptr(entry_pose), int(out_stride),
            C.c_void_p(d_out or None), C.c_void_p(d_counts_out or None)), "bev_submap_top_part_cloud_device_resident")

    def submap_top_part_coarse_registration_device(self, n_frames, d_clouds, offsets, d_pn, stride, d_counts, map_offsets,
                                                   entry_frame, entry_pose, matches, d_results, d_best, pn_leaf, radius=2.0,
                                                   viewpoint=None, params: IcpParams | None = None):
        """bev_submap_top_part_coarse_registration_device_resident: the queries are the front end's rows (d_pn, stride,
        d_counts) of the same n_frames frames; match m's query is registered point-to-plane, from both yaw guesses, against
        submap_top_part_cloud_device's target of map match_idx (pn_leaf > 0).  Outputs as submap_coarse_registration_device's."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else icp_params()
        vp = np.ascontiguousarray(viewpoint, dtype=np.float32).reshape(3) if viewpoint is not None else None
        self._check(self.lib.bev_submap_top_part_coarse_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, C.c_void_p(d_pn or None), stride, C.c_void_p(d_counts or None),
            pn_leaf, radius, _ptr(vp), n_maps, map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(entry_frame),
            _ptr(entry_pose), len(m), _ptr(m) if len(m) else None, C.byref(prm), C.c_void_p(d_results or None),
            C.c_void_p(d_best or None)), "bev_submap_top_part_coarse_registration_device_resident")

    # ---- verification of registered matches: two-way inlier counts --------------------------------------
    def verify_clouds(self, src, tgt, T, params: VerifyParams | None = None):
        """One problem: src / tgt are POINT_DTYPE records (or (n, 3) / (n, 4) float rows: x, y, z), T a 4 x 4 whose rows
        0 ... 2 move src; params None: the defaults (the leaf is not read: no voxel grid).  Returns one VERIFY_RESULT_DTYPE
        record."""
        src, tgt = as_points(src), as_points(tgt)
        t16 = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(16))
        prm = params if params is not None else verify_params()
        out = np.zeros(1, dtype=VERIFY_RESULT_DTYPE)
        self._check(self.lib.bev_verify_clouds(self._h, _ptr(src) if len(src) else None, len(src),
                                               _ptr(tgt) if len(tgt) else None, len(tgt), _ptr(t16), C.byref(prm), _ptr(out)),
                    "bev_verify_clouds")
        return out[0]

    def verify_registration_device(self, n_frames, d_clouds, offsets, matches, d_results, d_verify,
                                   params: VerifyParams | None = None):
        """bev_verify_registration_device_resident on device pointers: frames as for fine_registration_device, d_results its
        output (only T is read).  Asynchronous: synchronize() before reading d_verify (one VERIFY_RESULT_DTYPE per match)."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else verify_params()
        self._check(self.lib.bev_verify_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, len(m), _ptr(m) if len(m) else None,
            C.c_void_p(d_results or None), C.byref(prm), C.c_void_p(d_verify or None)),
            "bev_verify_registration_device_resident")

    def submap_verify_registration_device(self, n_frames, d_clouds, offsets, map_offsets, entry_frame, entry_pose, matches,
                                          d_results, d_verify, map_leaf=0.0, params: VerifyParams | None = None):
        """bev_submap_verify_registration_device_resident: the same against maps; maps, entries and map_leaf as for
        submap_voxel_registration_device, whose d_results go in as they are."""
        offsets, offs = _offsets(offsets, n_frames) if offsets is not None else (None, None)
        n_maps, map_offsets, entry_frame, entry_pose = self._submap_entries(map_offsets, entry_frame, entry_pose)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        prm = params if params is not None else verify_params()
        self._check(self.lib.bev_submap_verify_registration_device_resident(
            self._h, n_frames, C.c_void_p(d_clouds or None), offs, n_maps, map_offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            _ptr(entry_frame), _ptr(entry_pose), map_leaf, len(m), _ptr(m) if len(m) else None, C.c_void_p(d_results or None),
            C.byref(prm), C.c_void_p(d_verify or None)), "bev_submap_verify_registration_device_resident")

    def verify_registration_batch(self, clouds, matches, results, params: VerifyParams | None = None):
        """bev_verify_registration_batch on host clouds: matches MATCH_DTYPE records or (query_idx, match_idx, angle_guess)
        tuples, results their ICP_RESULT_DTYPE records (only T is read).  Returns (n_matches,) VERIFY_RESULT_DTYPE."""
        clouds, pts, npts = _host_clouds(clouds)
        m = np.array([tuple(r) for r in matches], dtype=MATCH_DTYPE) if not isinstance(matches, np.ndarray) else \
            np.ascontiguousarray(matches, dtype=MATCH_DTYPE)
        res = np.ascontiguousarray(results, dtype=ICP_RESULT_DTYPE).reshape(-1)
        assert len(res) == len(m)
        prm = params if params is not None else verify_params()
        out = np.zeros(len(m), dtype=VERIFY_RESULT_DTYPE)
        self._check(self.lib.bev_verify_registration_batch(
            self._h, len(clouds), pts, npts, len(m), _ptr(m) if len(m) else None, _ptr(res) if len(m) else None,
            C.byref(prm), _ptr(out) if len(m) else None), "bev_verify_registration_batch")
        return out

    # ---- a translation guess for retrieved pairs: height-grid offset search -----------------------------
    def align_grid_device(self, n_frames, d_clouds, offsets, d_grids, d_energy, params: AlignParams | None = None,
                          map_offsets=None, entry_frame=None, entry_pose=None):
        """bev_align_grid_device_resident on device pointers: frames as for float_bev_device; without map_offsets one grid per
        frame from its raw coordinates, else one per map (maps and entries as for submap_bev_device).  d_grids receives
        align_grid_bytes(params) per grid, d_energy one uint32 per grid.  Asynchronous: synchronize() before the host reads."""
        offsets, offs = _offsets(offsets, n_frames)
        prm = params if params is not None else align_params()
        n_maps, mo, ef, ep = 0, None, None, None
        if map_offsets is not None:
            n_maps, mo, ef, ep = self._submap_entries(map_offsets, entry_frame, entry_pose)
        rc = self.lib.bev_align_grid_device_resident(self._h, n_frames, C.c_void_p(d_clouds or None), offs, n_maps, _ptr(mo),
                                                     _ptr(ef), _ptr(ep), C.byref(prm), C.c_void_p(d_grids or None),
                                                     C.c_void_p(d_energy or None))
        self._check(rc, "bev_align_grid_device_resident")

    def align_hits_device(self, n_frames, d_clouds, offsets, n_db, d_grids, d_energy, hits, d_results, d_best, d_detail=None,
                          params: AlignParams | None = None):
        """bev_align_hits_device_resident on device pointers: the queries' packed frames, the n_db candidate grids of
        align_grid_device under the same params, hits MATCH_DTYPE records (PLACE_HIT_DTYPE records are cut to their first twelve
        bytes).  d_results receives 2 * n_hits ICP_RESULT_DTYPE, d_best n_hits int32, d_detail (0 or None: not wanted)
        2 * n_hits ALIGN_DETAIL_DTYPE.  Asynchronous: d_results / d_best go into the fine calls as d_coarse / d_best."""
        offsets, offs = _offsets(offsets, n_frames)
        m = _matches(hits)
        prm = params if params is not None else align_params()
        rc = self.lib.bev_align_hits_device_resident(self._h, n_frames, C.c_void_p(d_clouds or None), offs, n_db,
                                                     C.c_void_p(d_grids or None), C.c_void_p(d_energy or None), len(m),
                                                     _ptr(m) if len(m) else None, C.byref(prm), C.c_void_p(d_results or None),
                                                     C.c_void_p(d_best or None), C.c_void_p(d_detail or None))
        self._check(rc, "bev_align_hits_device_resident")

    def align_batch(self, clouds, hits, params: AlignParams | None = None, map_offsets=None, entry_frame=None, entry_pose=None,
                    want_detail=True):
        """bev_align_batch on host clouds: the frames are the queries, the candidates the maps or, without map_offsets, the
        frames themselves.  Returns (results (n, 2) ICP_RESULT_DTYPE, best (n,) int32, detail (n, 2) ALIGN_DETAIL_DTYPE or
        None)."""
        clouds, pts, npts = _host_clouds(clouds)
        m = _matches(hits)
        prm = params if params is not None else align_params()
        n_maps, mo, ef, ep = 0, None, None, None
        if map_offsets is not None:
            n_maps, mo, ef, ep = self._submap_entries(map_offsets, entry_frame, entry_pose)
        n = len(m)
        res, best = np.zeros((n, 2), dtype=ICP_RESULT_DTYPE), np.zeros(n, dtype=np.int32)
        det = np.zeros((n, 2), dtype=ALIGN_DETAIL_DTYPE) if want_detail else None
        rc = self.lib.bev_align_batch(self._h, len(clouds), pts, npts, n_maps, _ptr(mo), _ptr(ef), _ptr(ep), n,
                                      _ptr(m) if n else None, C.byref(prm), _ptr(res) if n else None,
                                      _ptr(best) if n else None, _ptr(det) if n and want_detail else None)
        self._check(rc, "bev_align_batch")
        return res, best, det

    def set_layout_hint(self, layout: int):
        """LAYOUT_UNKNOWN (the library looks), LAYOUT_STRUCTURED, LAYOUT_FIRING_ORDER: include/bev_mi355x.h"""
        self._check(self.lib.bev_set_layout_hint(self._h, layout), "bev_set_layout_hint")

    def set_submap_search_grid(self, fine: int, coarse: int):
        """The cap of cells per axis of the maps' search grids in the fine and the coarse scan-to-map calls made from now on:
        0 the grids of always (128 and 64 at most), 1 .. SUBMAP_SEARCH_GRID_MAX grids sized to the map (bev_set_submap_search_grid;
        DESIGN.md §6s).  Results do not depend on it."""
        self._check(self.lib.bev_set_submap_search_grid(self._h, int(fine), int(coarse)), "bev_set_submap_search_grid")

    def debug_submap_grid(self, coarse: int, first: int, n: int) -> np.ndarray:
        """Test hook (synchronises): (n, 4) uint32 rows {nx, ny, searchable points, largest count of one cell} of maps first ..
        first + n - 1 of the last launch group of the last fine (coarse = 0) or coarse (1) scan-to-map call."""
        out = np.zeros((n, 4), dtype=np.uint32)
        self._check(self.lib.bev_debug_get_submap_grid(self._h, int(coarse), int(first), int(n), _ptr(out)),
                    "bev_debug_get_submap_grid")
        return out

    def set_pair_search_grid(self, fine: int, coarse: int):
        """The cap of cells per axis of the targets' search grids in the fine and the coarse PAIR calls made from now on
        (icp_point_to_point, fine_registration*; icp_point_to_plane, coarse_registration*): 0 the grids of always (128 and 64 at
        most), 1 .. PAIR_SEARCH_GRID_MAX grids sized to the cloud (bev_set_pair_search_grid).  Results do not
        depend on it; the scan-to-map calls do not read it."""
        self._check(self.lib.bev_set_pair_search_grid(self._h, int(fine), int(coarse)), "bev_set_pair_search_grid")

    def debug_pair_grid(self, coarse: int, first: int, n: int) -> np.ndarray:
        """Test hook (synchronises): (n, 4) uint32 rows {nx, ny, searchable points, largest count of one cell} of the grids of
        the targets of matches first .. first + n - 1 of the last fine (coarse = 0) or coarse (1) pair call."""
        out = np.zeros((max(n, 0), 4), dtype=np.uint32)
        self._check(self.lib.bev_debug_get_pair_grid(self._h, int(coarse), int(first), int(n), _ptr(out)),
                    "bev_debug_get_pair_grid")
        return out

    # ---- measurement / test hooks ------------------------------------------
    def set_lanes(self, n: int) -> int:
        r = self.lib.bev_set_lanes(self._h, n)
        if r < 0:
            self._check(r, "bev_set_lanes")
        return r

    def profile_enable(self, on=True):
        self._check(self.lib.bev_profile_enable(self._h, 1 if on else 0), "bev_profile_enable")

    def profile_reset(self):
        self._check(self.lib.bev_profile_reset(self._h), "bev_profile_reset")

    def profile_get(self):
        arr = (KernelStat * 16)()
        n = self.lib.bev_profile_get(self._h, arr, 16)
        if n < 0:
            self._check(n, "bev_profile_get")
        return [
            {"name": arr[i].name.decode(), "launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms),
             "frames": int(arr[i].frames)}
            for i in range(min(n, 16))
        ]

    def cell_avg(self, first_frame=0, n_frames=1):
        out = np.empty((n_frames, GROUND_GRID_CELLS), dtype=np.float32)
        self._check(self.lib.bev_debug_get_cell_avg(self._h, first_frame, n_frames, _ptr(out)),
                    "bev_debug_get_cell_avg")
        return out

    def frame_info(self, first_frame=0, n_frames=1):
        """(n, 4) uint32: T, mode (0 general, 1 sorted prefix read in place, 2 read in place then redone, 3 structured cloud
        read in place, 4 firing order read in place), consumed, failed of the frames of the last sub-batch."""
        out = np.empty((n_frames, 4), dtype=np.uint32)
        self._check(self.lib.bev_debug_get_frame_info(self._h, first_frame, n_frames, _ptr(out)), "bev_debug_get_frame_info")
        return out

    def code_overflow(self, first_frame=0, n_frames=1):
        """(n,) uint32: per frame of the last sub-batch, the number of (writer, raster band) code lists that overflowed;
        those bands were rastered from the ordered cloud instead"""
        if not hasattr(self.lib, "bev_debug_get_code_overflow"):
            raise BevError("this build of libbev_mi355x.so (selected through BEV_AMD_LIB?) has no bev_debug_get_code_overflow")
        out = np.empty(n_frames, dtype=np.uint32)
        self._check(self.lib.bev_debug_get_code_overflow(self._h, first_frame, n_frames, _ptr(out)), "bev_debug_get_code_overflow")
        return out

    def angle_predicate(self, dx, dy, dz):
        dx = np.ascontiguousarray(dx, dtype=np.float32)
        dy = np.ascontiguousarray(dy, dtype=np.float32)
        dz = np.ascontiguousarray(dz, dtype=np.float32)
        out = np.empty(dx.shape[0], dtype=np.uint8)
        self._check(self.lib.bev_debug_angle_predicate(self._h, _ptr(dx), _ptr(dy), _ptr(dz), _ptr(out), dx.shape[0]),
                    "bev_debug_angle_predicate")
        return out

    def exact_eval(self, fn, *inputs, params=None):
        """bev_debug_exact_eval: function `fn` (a name of EXACT_EVAL, or its id) of the shared host/device arithmetic on
        the device, element by element.  inputs: the arrays of EXACT_EVAL[fn] in order; returns int32, uint32, float32,
        float64 or (n, 3) float32 as the function does."""
        name = fn if isinstance(fn, str) else EXACT_EVAL_NAMES[fn]
        kinds, out_kind, n_params = EXACT_EVAL[name]
        if len(inputs) != len(kinds):
            raise BevError(f"exact_eval({name}) takes {len(kinds)} arrays")
        arrs = [np.ascontiguousarray(a, dtype=_EVAL_IN[k]) for a, k in zip(inputs, kinds)]
        n = arrs[0].shape[0]
        if any(a.shape != (n,) for a in arrs):
            raise BevError("exact_eval: the arrays differ in length")
        prm = None if not n_params else np.ascontiguousarray(params, dtype=np.float32).reshape(n_params)
        out = np.zeros((n, 3) if out_kind == "f3" else n, dtype=_EVAL_OUT[out_kind])
        ptrs = [_ptr(a) for a in arrs] + [None] * (4 - len(arrs))
        self._check(self.lib.bev_debug_exact_eval(self._h, EXACT_EVAL_NAMES.index(name), n, *ptrs,
                                                  _ptr(prm) if prm is not None else None, _ptr(out)), "bev_debug_exact_eval")
        return out


def project_batch_out_points(kind: int, n_frames: int, offsets) -> int:
    """Records the d_out of project_device must hold (host only); 0 for an unknown kind or decreasing offsets."""
    offsets, offs = _offsets(offsets, n_frames)
    return int(load_lib().bev_project_batch_out_points(kind, n_frames, offs))


def _matches(hits) -> np.ndarray:
    """MATCH_DTYPE records of match records, hit records (their first twelve bytes) or (query_idx, match_idx, angle_guess)
    tuples"""
    if isinstance(hits, np.ndarray) and hits.dtype.names:
        m = np.zeros(hits.size, dtype=MATCH_DTYPE)
        for f in MATCH_DTYPE.names:
            m[f] = hits.reshape(-1)[f]
        return m
    return np.array([tuple(r) for r in hits], dtype=MATCH_DTYPE)


def align_grid_bytes(params: AlignParams | None = None) -> int:
    """bev_align_grid_bytes: grid * grid; 0 for parameters outside the admitted values."""
    return int(load_lib().bev_align_grid_bytes(C.byref(params) if params is not None else None))


def place_descriptor_bytes(params: PlaceParams | None = None) -> int:
    """bev_place_descriptor_bytes: n_rings * n_sectors; 0 for parameters outside the admitted values."""
    return int(load_lib().bev_place_descriptor_bytes(C.byref(params) if params is not None else None))


def place_desc_handle_bytes(params: PlaceParams | None = None) -> int:
    """bev_place_desc_handle_bytes: the opaque per-descriptor record of place_descriptor_device / place_match_device."""
    return int(load_lib().bev_place_desc_handle_bytes(C.byref(params) if params is not None else None))


def regfront_max_out(n: int) -> int:
    """Records the registration front end can emit for a cloud of n points (host only)."""
    return int(load_lib().bev_regfront_max_out(n))


def submap_top_part_max_out(union_records: int) -> int:
    """Rows the top part over a union of that many records can have (host only): submap_top_part_cloud_device's out_stride."""
    return int(load_lib().bev_submap_top_part_max_out(union_records))


def _pn12(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, POINT_NORMAL_FLOATS))


def icp_coarse_defaults() -> IcpParams:
    """bev_icp_coarse_defaults(): D = 10, 10 iterations, transformation_epsilon 0, euclidean_fitness_epsilon -DBL_MAX."""
    return load_lib().bev_icp_coarse_defaults()


def icp_fine_defaults() -> IcpParams:
    """bev_icp_fine_defaults(): the top-part tool's fine ICP — D = 1, transformation_epsilon 1e-6,
    euclidean_fitness_epsilon 0.01, 100 iterations."""
    return load_lib().bev_icp_fine_defaults()


def icp_whole_defaults() -> IcpParams:
    """bev_icp_whole_defaults(): the whole tool's ICP — D = 4, 1e-6, 0.001, 200 iterations."""
    return load_lib().bev_icp_whole_defaults()


def as_points(a) -> np.ndarray:
    """POINT_DTYPE records as they are, or (n, 3) / (n, 4) float rows as records with x, y, z set (every other field 0)."""
    if isinstance(a, np.ndarray) and a.dtype == POINT_DTYPE:
        return np.ascontiguousarray(a)
    f = np.asarray(a, dtype=np.float32).reshape(len(a), -1) if len(a) else np.zeros((0, 3), np.float32)
    out = np.zeros(len(f), dtype=POINT_DTYPE)
    out["x"], out["y"], out["z"] = f[:, 0], f[:, 1], f[:, 2]
    return out


def _xyz4(xyz) -> np.ndarray:
    a = np.asarray(xyz, dtype=np.float32)
    if a.ndim == 2 and a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1)
    return np.ascontiguousarray(a.reshape(-1, XYZ_FLOATS))


def yaw_translate_matrix(tx: float, ty: float, tz: float, yaw_deg: float) -> np.ndarray:
    """[R | t] of cloud_manip (CloudManip.cpp:119-128) as 12 floats, row-major; host arithmetic only."""
    m = np.empty(12, dtype=np.float32)
    load_lib().bev_yaw_translate_matrix(tx, ty, tz, yaw_deg, _ptr(m))
    return m


def host_alloc(shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (bev_host_alloc); the memory is never returned to the system —
    meant for long-lived I/O buffers of a driver script."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    rc = load_lib().bev_host_alloc(C.byref(p), n)
    if rc != 0 or not p.value:
        raise BevError(f"bev_host_alloc({n}) failed: status {rc}")
    buf = (C.c_char * n).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def algorithmic_bytes_per_frame(params: BevParams, n_points: float) -> float:
    """32*P + 32*S + n_layers*M*M + M*M."""
    M = params.mat_size
    return 32.0 * n_points + 32.0 * params.slots + params.n_layers * M * M + M * M
