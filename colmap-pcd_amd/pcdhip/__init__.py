"""pcdhip -- ctypes binding of libpcdhip.so (include/pcdhip.h).

Plumbing only: every computation happens in the HIP library.  There is no
CPU fallback; on a box without a gfx950 device `Cloud(...)`/`BA(...)` raise
PcdError(PCD_ERR_NO_DEVICE).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)            # colmap-pcd_amd/
LIB_PATH = os.environ.get("PCDHIP_LIB", os.path.join(_ROOT, "libpcdhip.so"))   # override: tuning variants only

PCD_OK, PCD_ERR_INVALID, PCD_ERR_NO_DEVICE, PCD_ERR_HIP, PCD_ERR_OOM, PCD_ERR_UNSUPPORTED = range(6)
NN_AUTO, NN_BRUTEFORCE, NN_FALLBACK_ONLY, NN_GRID = 0, 1, 2, 3
GATE_MAPPER_LOCAL, GATE_MAPPER_GLOBAL, GATE_CONTROLLER = 0, 1, 2
GATE_BOUNDED_SEARCH = 0x100   # OR-ed into a gate mode: search bounded by the gate (pcdhip.h)
LIDAR_NONE, LIDAR_ICP, LIDAR_ICP_GROUND = 0, 1, 2
LIDAR_PROJ = 3
LOSS_TRIVIAL, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2
LAYOUT_XYZ_NRM, LAYOUT_AOS32 = 0, 1
NORMALS_ORIENT_NONE, NORMALS_ORIENT_VIEWPOINT = 0, 1
KEY_NONE = 0x7FFFFFFFFFFFFFFF

CAMERA_MODELS = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE",
                 "FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]


class PcdError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"pcdhip status {status}: {msg}")
        self.status = status


class CloudOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("layout", C.c_int32), ("raw_lidar_frame", C.c_int32),
                ("cell_size", C.c_float), ("index_base", C.c_uint32), ("index_stride", C.c_uint32),
                ("reserved", C.c_int32 * 8)]


class CloudInfo(C.Structure):
    _fields_ = [("cell_size", C.c_float), ("origin", C.c_float * 3), ("dims", C.c_int32 * 3),
                ("block_dims", C.c_int32 * 3), ("num_indexed", C.c_uint64), ("occupied_cells", C.c_uint64),
                ("build_ms", C.c_double), ("bbox_lo", C.c_float * 3), ("bbox_hi", C.c_float * 3)]


class AssocOut(C.Structure):
    _fields_ = [("lidar_xyz", C.c_void_p), ("abcd", C.c_void_p), ("type", C.c_void_p), ("dist", C.c_void_p),
                ("angle", C.c_void_p), ("dist2plane", C.c_void_p), ("nn_idx", C.c_void_p),
                ("nn_sqdist", C.c_void_p)]


class AssocHit(C.Structure):
    _fields_ = [("lidar_xyz", C.c_double * 3), ("abcd", C.c_double * 4), ("dist", C.c_double), ("angle", C.c_double),
                ("query", C.c_uint32), ("type", C.c_uint8), ("pad", C.c_uint8 * 3)]


HIT_DTYPE = np.dtype([("lidar_xyz", np.float64, 3), ("abcd", np.float64, 4), ("dist", np.float64), ("angle", np.float64),
                      ("query", np.uint32), ("type", np.uint8), ("pad", np.uint8, 3)])
assert HIT_DTYPE.itemsize == 80 and C.sizeof(AssocHit) == 80


class BADesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("num_cameras", C.c_int32), ("cam_model", C.c_void_p),
                ("cam_param_offset", C.c_void_p), ("cam_params", C.c_void_p), ("cam_params_len", C.c_uint64),
                ("num_images", C.c_int32), ("poses", C.c_void_p), ("image_camera", C.c_void_p),
                ("image_const_pose", C.c_void_p), ("image_const_tvec", C.c_void_p),
                ("num_points", C.c_int32), ("points", C.c_void_p), ("point_const", C.c_void_p),
                ("num_obs", C.c_uint64), ("obs_image", C.c_void_p), ("obs_point", C.c_void_p),
                ("obs_xy", C.c_void_p),
                ("num_lidar", C.c_uint64), ("lidar_point", C.c_void_p), ("lidar_abcd", C.c_void_p),
                ("lidar_weight", C.c_void_p),
                ("loss_type", C.c_int32), ("loss_scale", C.c_double), ("camera_refine", C.c_void_p),
                ("reserved", C.c_int32 * 8)]


CAM_JAC_STRIDE = 12


class BAOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cost", "residuals", "jac_q", "jac_t", "jac_X", "jac_lidar",
                                           "H_img", "g_img", "H_pt", "g_pt", "W", "jac_cam",
                                           "H_cam", "g_cam", "E_cam", "W_cam")]


class BABlocks(C.Structure):
    """pcd_ba_blocks: pointers into the handle's pinned buffers"""
    _fields_ = [(n, C.c_void_p) for n in ("residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "jac_cam", "pose_row")] + \
               [("num_pose_rows", C.c_uint64), ("bytes_d2h", C.c_uint64)]


class BABlocksCompact(C.Structure):
    """pcd_ba_blocks_compact: pointers into the handle's pinned buffers"""
    _fields_ = [(n, C.c_void_p) for n in ("residuals", "records", "lidar_residuals", "jac_lidar", "jac_cam")] + \
               [("cam_stride", C.c_int32), ("bytes_d2h", C.c_uint64)]


DAMP_MARQUARDT, DAMP_LEVENBERG = 0, 1
_DAMPING = {"marquardt": DAMP_MARQUARDT, "levenberg": DAMP_LEVENBERG}


class BASchurOpts(C.Structure):
    _fields_ = [("mu", C.c_double), ("damping", C.c_int32), ("reserved", C.c_int32 * 7)]


class BASchurOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cost", "S_diag", "S_off", "rhs", "S", "num_skipped")]


class BASchurCamOut(C.Structure):
    """pcd_ba_schur_cam_out"""
    _fields_ = [(n, C.c_void_p) for n in ("cost", "S_diag", "S_off", "rhs", "B", "S_cam", "rhs_cam", "S", "num_skipped")]


MAX_CAMERA_SLOTS = 8


class BASchurInfo(C.Structure):
    _fields_ = [("build_ms", C.c_double), ("num_entries", C.c_uint64), ("scratch_bytes", C.c_uint64)]


class BASchurBuildInfo(C.Structure):
    _fields_ = [("build_ms", C.c_double), ("num_slots", C.c_int32), ("num_syncs", C.c_int32), ("num_pairs", C.c_uint64),
                ("num_entries", C.c_uint64)]


_SCHUR_LISTS = ("slot_image", "obs_pos", "blk_start", "ent_a", "ent_b", "pair_ij", "row_start", "row_blk", "row_col")


class BASchurLists(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _SCHUR_LISTS]


PRECOND_IDENTITY, PRECOND_SCHUR_JACOBI = 0, 1
_PRECOND = {"identity": PRECOND_IDENTITY, "schur_jacobi": PRECOND_SCHUR_JACOBI}
PCG_MAX_ITERATIONS, PCG_Q_TOLERANCE, PCG_R_TOLERANCE, PCG_BREAKDOWN, PCG_ZERO_RHS = range(5)
SOLVE_MAX_ITERATIONS, SOLVE_FUNCTION_TOLERANCE, SOLVE_GRADIENT_TOLERANCE, SOLVE_MIN_RADIUS = range(4)


class BAPcgOpts(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("min_iterations", C.c_int32), ("preconditioner", C.c_int32),
                ("q_tolerance", C.c_double), ("r_tolerance", C.c_double), ("reserved", C.c_int32 * 8)]


class BAPcgInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("termination", C.c_int32), ("precond_fallbacks", C.c_uint32),
                ("rhs_norm", C.c_double), ("residual_norm", C.c_double), ("q", C.c_double),
                ("step_dot_residual", C.c_double)]


PCG_INFO_DTYPE = np.dtype([("iterations", np.int32), ("termination", np.int32), ("precond_fallbacks", np.uint32),
                           ("pad", np.uint32), ("rhs_norm", np.float64), ("residual_norm", np.float64),
                           ("q", np.float64), ("step_dot_residual", np.float64)])
assert PCG_INFO_DTYPE.itemsize == C.sizeof(BAPcgInfo) == 48


LINEAR_PCG, LINEAR_CHOLESKY, LINEAR_PCG_CAM = 0, 1, 2
_LINEAR = {"pcg": LINEAR_PCG, "cholesky": LINEAR_CHOLESKY, "pcg_cam": LINEAR_PCG_CAM}
CHOL_OK, CHOL_NOT_POSITIVE_DEFINITE = 0, 1


class BACholInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("failed_column", C.c_int32), ("n", C.c_int32), ("n_padded", C.c_int32),
                ("panels", C.c_int32), ("min_pivot", C.c_double), ("max_pivot", C.c_double)]


CHOL_INFO_DTYPE = np.dtype([("status", np.int32), ("failed_column", np.int32), ("n", np.int32), ("n_padded", np.int32),
                            ("panels", np.int32), ("pad", np.int32), ("min_pivot", np.float64),
                            ("max_pivot", np.float64)])
assert CHOL_INFO_DTYPE.itemsize == C.sizeof(BACholInfo) == 40


class BASolveOpts(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("damping", C.c_int32), ("initial_radius", C.c_double),
                ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("linear", BAPcgOpts),
                ("linear_solver", C.c_int32), ("refine_intrinsics", C.c_int32), ("reserved", C.c_int32 * 6)]


assert C.sizeof(BASolveOpts) == 152   # linear_solver and refine_intrinsics came out of reserved: the size did not change


class BASolveIteration(C.Structure):
    _fields_ = [("cost", C.c_double), ("candidate_cost", C.c_double), ("model_decrease", C.c_double),
                ("relative_decrease", C.c_double), ("radius", C.c_double), ("gradient_max_norm", C.c_double),
                ("accepted", C.c_int32), ("linear_iterations", C.c_int32), ("linear_termination", C.c_int32),
                ("num_skipped", C.c_uint64)]


class BASolveSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("num_iterations", C.c_int32),
                ("num_accepted", C.c_int32), ("termination", C.c_int32), ("total_ms", C.c_double),
                ("linear_solver_ms", C.c_double)]


class BAAssocOpts(C.Structure):
    """pcd_ba_assoc_opts (pcdhip.h)."""
    _fields_ = [("gate_mode", C.c_int32), ("d_max_range", C.c_void_p), ("max_range_count", C.c_uint64),
                ("d_select", C.c_void_p), ("icp_weight", C.c_double), ("icp_ground_weight", C.c_double),
                ("reserved", C.c_int32 * 8)]


class BAAssocInfo(C.Structure):
    _fields_ = [("num_queries", C.c_uint64), ("num_terms", C.c_uint64), ("num_icp", C.c_uint64),
                ("num_icp_ground", C.c_uint64), ("assoc_ms", C.c_double), ("rebuild_ms", C.c_double)]


class BAProjOpts(C.Structure):
    """pcd_ba_proj_opts (pcdhip.h)."""
    _fields_ = [("cam_width", C.c_void_p), ("cam_height", C.c_void_p), ("d_image_select", C.c_void_p),
                ("d_point_mode", C.c_void_p), ("gate_mode", C.c_int32), ("d_max_range", C.c_void_p),
                ("max_range_count", C.c_uint64), ("proj_weight", C.c_double), ("icp_weight", C.c_double),
                ("icp_ground_weight", C.c_double), ("reserved", C.c_int32 * 8)]


class BAProjInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("num_images", "num_features", "num_found", "num_terms", "num_proj", "num_icp",
                                           "num_icp_ground", "pairs")] + \
               [(n, C.c_double) for n in ("proj_ms", "assoc_ms", "rebuild_ms")]


class BAFilterOpts(C.Structure):
    """pcd_ba_filter_opts (pcdhip.h)."""
    _fields_ = [("max_reproj_error", C.c_double), ("min_tri_angle_deg", C.c_double), ("reserved", C.c_int32 * 8)]


class BAFilterOut(C.Structure):
    """pcd_ba_filter_out (pcdhip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("obs_erase", "obs_negative_depth", "point_delete", "point_error", "summary")]


class BARemoveInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("num_obs", "num_obs_removed", "num_lidar", "num_lidar_removed",
                                           "num_points_emptied")] + [("rebuild_ms", C.c_double)]


class BAAddInfo(C.Structure):
    """pcd_ba_add_info (pcdhip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("num_obs", "num_obs_added", "num_points", "num_points_added",
                                           "num_pose_rows")] + [("rebuild_ms", C.c_double)]


class BAWindowOpts(C.Structure):
    """pcd_ba_window_opts (pcdhip.h)."""
    _fields_ = [("center_image", C.c_int32), ("radius", C.c_double), ("d_image_set", C.c_void_p),
                ("d_extra_const_pose", C.c_void_p), ("reserved", C.c_int32 * 8)]


class BAWindowInfo(C.Structure):
    """pcd_ba_window_info (pcdhip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("num_images_in", "num_points_active", "num_obs", "num_lidar",
                                           "num_pose_rows")] + [("build_ms", C.c_double)]


class BALocalBundleOpts(C.Structure):
    """pcd_ba_local_bundle_opts (pcdhip.h)."""
    _fields_ = [("image", C.c_int32), ("num_images", C.c_int32), ("min_tri_angle_deg", C.c_double),
                ("reserved", C.c_int32 * 8)]


class BALocalWindowOpts(C.Structure):
    """pcd_ba_local_window_opts (pcdhip.h)."""
    _fields_ = [("d_image_set", C.c_void_p), ("d_point_variable", C.c_void_p), ("image", C.c_int32),
                ("max_track_length", C.c_uint32), ("d_extra_const_pose", C.c_void_p), ("reserved", C.c_int32 * 8)]


class BALocalWindowInfo(C.Structure):
    """pcd_ba_local_window_info (pcdhip.h)."""
    _fields_ = [(n, C.c_uint64) for n in ("num_images_in", "num_points_variable", "num_points_fixed", "num_obs",
                                           "num_lidar", "num_pose_rows")] + [("build_ms", C.c_double)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class NormalsOptions(C.Structure):
    """pcd_normals_options (pcdhip.h)."""
    _fields_ = [("radius", C.c_float), ("min_neighbors", C.c_int32), ("orient", C.c_int32),
                ("viewpoint", C.c_float * 3), ("only_missing", C.c_int32), ("reserved", C.c_int32 * 8)]


class NormalsInfo(C.Structure):
    _fields_ = [("num_estimated", C.c_uint64), ("num_too_few", C.c_uint64), ("num_degenerate", C.c_uint64),
                ("num_kept", C.c_uint64), ("pair_tests", C.c_uint64), ("max_neighbors", C.c_uint32),
                ("mean_neighbors", C.c_double), ("ms", C.c_double)]


class VoxelOptions(C.Structure):
    """pcd_voxel_options (pcdhip.h)."""
    _fields_ = [("leaf", C.c_float * 3), ("min_points", C.c_int32), ("cell_size", C.c_float),
                ("reserved", C.c_int32 * 8)]


class VoxelInfo(C.Structure):
    _fields_ = [("num_input", C.c_uint64), ("num_voxels", C.c_uint64), ("num_output", C.c_uint64),
                ("num_dropped_rows", C.c_uint64), ("min_b", C.c_int32 * 3), ("dims", C.c_int32 * 3),
                ("max_points_per_voxel", C.c_uint32), ("ms", C.c_double), ("build_ms", C.c_double)]


class NNStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("queries", "brick_groups", "staged_points", "fallback_queries",
                                           "fallback_points", "pair_evals")]


# every symbol include/pcdhip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "pcd_last_error", "pcd_version", "pcd_device_count",
    "pcd_cloud_options_default", "pcd_cloud_create", "pcd_cloud_destroy", "pcd_cloud_size",
    "pcd_cloud_get_info", "pcd_cloud_download",
    "pcd_nn_query", "pcd_nn_query_algo", "pcd_nn_query_device", "pcd_nn_refine_device",
    "pcd_associate", "pcd_associate_device", "pcd_assoc_staging", "pcd_associate_staged", "pcd_nn_winner_payload_device",
    "pcd_associate_from_payload_device", "pcd_search_range_schedule",
    "pcd_camera_num_params", "pcd_camera_param_groups", "pcd_ba_create", "pcd_ba_destroy", "pcd_ba_set_parameters", "pcd_ba_set_camera_parameters",
    "pcd_ba_evaluate", "pcd_ba_evaluate_device", "pcd_ba_device_parameters",
    "pcd_profile_enable", "pcd_profile_only", "pcd_profile_reset", "pcd_profile_get", "pcd_nn_last_stats",
    "pcd_sift_match", "pcd_sift_match_device", "pcd_sift_match_batch", "pcd_sift_match_batch_device",
    "pcd_filter_lidar_outlier_device", "pcd_ba_observation_errors", "pcd_ba_observation_errors_device",
    "pcd_proj_default_options", "pcd_proj_create", "pcd_proj_destroy", "pcd_proj_num_submaps",
    "pcd_proj_last_pairs", "pcd_proj_scale_coeffs", "pcd_proj_set_new_images",
    "pcd_sift_matcher_create", "pcd_sift_matcher_destroy", "pcd_sift_matcher_set_max_sift",
    "pcd_sift_matcher_set_descriptors", "pcd_sift_matcher_match",
    "pcd_sift_match_guided", "pcd_sift_match_guided_device", "pcd_sift_match_guided_batch",
    "pcd_sift_match_guided_batch_device", "pcd_sift_matcher_set_locations", "pcd_sift_matcher_match_guided",
    "pcd_ba_evaluate_blocks", "pcd_ba_evaluate_blocks_compact", "pcd_ba_filter_tracks", "pcd_ba_filter_tracks_device",
    "pcd_cloud_create_sharded", "pcd_cloud_shards_destroy", "pcd_cloud_shards_count", "pcd_cloud_shards_size",
    "pcd_cloud_shards_get", "pcd_nn_query_sharded", "pcd_associate_sharded",
    "pcd_ba_set_parameters_device", "pcd_ba_schur_structure", "pcd_ba_schur_device", "pcd_ba_schur",
    "pcd_ba_schur_back_substitute_device", "pcd_ba_plus_device", "pcd_ba_schur_stats",
    "pcd_ba_pcg_opts_default", "pcd_ba_schur_solve_pcg_device", "pcd_ba_schur_solve_pcg", "pcd_ba_get_parameters",
    "pcd_ba_solve_opts_default", "pcd_ba_solve",
    "pcd_ba_schur_solve_cholesky_device", "pcd_ba_schur_solve_cholesky",
    "pcd_ba_camera_slots", "pcd_ba_schur_cam_device", "pcd_ba_schur_cam", "pcd_ba_schur_cam_solve_cholesky_device",
    "pcd_ba_schur_cam_back_substitute_device", "pcd_ba_plus_cam_device", "pcd_ba_get_camera_parameters",
    "pcd_ba_schur_cam_solve_pcg_device", "pcd_ba_schur_cam_solve_pcg",
    "pcd_normals_options_default", "pcd_cloud_estimate_normals_device", "pcd_cloud_estimate_normals",
    "pcd_voxel_options_default", "pcd_cloud_voxel_downsample", "pcd_cloud_voxel_downsample_device",
    "pcd_ba_set_lidar_device", "pcd_ba_get_lidar", "pcd_ba_lidar_device", "pcd_ba_assoc_opts_default",
    "pcd_ba_associate_lidar_device",
    "pcd_proj_set_new_images_device", "pcd_ba_proj_opts_default", "pcd_ba_project_lidar_device",
    "pcd_ba_filter_opts_default", "pcd_ba_filter_points_device", "pcd_ba_filter_points",
    "pcd_ba_remove_observations_device", "pcd_ba_add_observations_device", "pcd_ba_add_observations",
    "pcd_ba_schur_build_device", "pcd_ba_schur_structure_lists",
    "pcd_ba_window_opts_default", "pcd_ba_window_create_device", "pcd_ba_window_commit_device",
    "pcd_ba_local_bundle_opts_default", "pcd_ba_local_bundle_device", "pcd_ba_local_bundle",
    "pcd_ba_local_window_opts_default", "pcd_ba_local_window_create_device",
]


class ProjOptions(C.Structure):
    """lidar/pcd_projection.h:31-47 (numeric members)."""
    _fields_ = [("depth_image_scale", C.c_double), ("max_proj_scale", C.c_int32), ("min_proj_scale", C.c_int32),
                ("min_proj_dist", C.c_double), ("submap_length", C.c_float), ("submap_width", C.c_float),
                ("submap_height", C.c_float), ("choose_meter", C.c_float), ("min_lidar_proj_dist", C.c_double)]


class ProjImage(C.Structure):
    _fields_ = [("qvec", C.c_double * 4), ("tvec", C.c_double * 3), ("params", C.c_double * 8),
                ("width", C.c_uint64), ("height", C.c_uint64), ("feat_begin", C.c_uint64), ("feat_end", C.c_uint64)]

_LIB = None


def build():
    """Compile libpcdhip.so in-tree with hipcc for gfx950 (works without a GPU)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", _ROOT, "libpcdhip.so"])


def lib():
    """Load the HIP library.  Fails loudly if it is missing: there is no other backend."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise PcdError(PCD_ERR_NO_DEVICE, f"{LIB_PATH} not built; run __graft_entry__.build() or make -C colmap-pcd_amd")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 / libhsa-runtime64.
    # If libpcdhip pulled in /opt/rocm's copy first, torch would later mix the two and find no GPU, so
    # when torch is installed let it load its runtime first; libpcdhip then binds to the same soname.
    if os.environ.get("PCDHIP_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    L.pcd_last_error.restype = C.c_char_p
    L.pcd_cloud_size.restype = C.c_uint64
    L.pcd_cloud_size.argtypes = [C.c_void_p]
    L.pcd_cloud_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CloudOptions), C.POINTER(C.c_void_p)]
    L.pcd_cloud_destroy.argtypes = [C.c_void_p]
    L.pcd_cloud_destroy.restype = None
    L.pcd_cloud_get_info.argtypes = [C.c_void_p, C.POINTER(CloudInfo)]
    L.pcd_cloud_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcd_nn_query_algo.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcd_nn_query.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcd_nn_query_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.pcd_associate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                C.POINTER(AssocOut)]
    L.pcd_associate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                       C.c_void_p, C.POINTER(AssocOut), C.c_void_p]
    L.pcd_nn_winner_payload_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pcd_associate_from_payload_device.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.POINTER(AssocOut),
                                                    C.c_void_p]
    L.pcd_search_range_schedule.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.pcd_profile_get.argtypes = [C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]
    L.pcd_nn_last_stats.argtypes = [C.c_void_p, C.POINTER(NNStats)]
    if hasattr(L, "pcd_nn_last_wave_records"):   # (a library of an older tree, loaded through PCDHIP_LIB for A/B runs)
        L.pcd_nn_last_wave_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64)]
    if hasattr(L, "pcd_nn_last_fb_wave_records"):
        L.pcd_nn_last_fb_wave_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]
    L.pcd_normals_options_default.argtypes = [C.POINTER(NormalsOptions)]
    L.pcd_normals_options_default.restype = None
    L.pcd_cloud_estimate_normals_device.argtypes = [C.c_void_p, C.POINTER(NormalsOptions), C.c_void_p, C.c_void_p,
                                                    C.c_void_p]
    L.pcd_cloud_estimate_normals.argtypes = [C.c_void_p, C.POINTER(NormalsOptions), C.c_void_p, C.c_void_p,
                                             C.POINTER(NormalsInfo)]
    L.pcd_voxel_options_default.argtypes = [C.POINTER(VoxelOptions)]
    L.pcd_voxel_options_default.restype = None
    L.pcd_cloud_voxel_downsample.argtypes = [C.c_void_p, C.POINTER(VoxelOptions), C.c_void_p, C.POINTER(C.c_void_p),
                                             C.POINTER(VoxelInfo)]
    L.pcd_cloud_voxel_downsample_device.argtypes = [C.c_void_p, C.POINTER(VoxelOptions), C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_void_p), C.POINTER(VoxelInfo)]
    if hasattr(L, "pcd_ba_create"):
        L.pcd_ba_create.argtypes = [C.POINTER(BADesc), C.POINTER(C.c_void_p)]
        L.pcd_ba_destroy.argtypes = [C.c_void_p]
        L.pcd_ba_destroy.restype = None
        L.pcd_ba_set_parameters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.pcd_ba_evaluate.argtypes = [C.c_void_p, C.POINTER(BAOut)]
        L.pcd_ba_evaluate_device.argtypes = [C.c_void_p, C.POINTER(BAOut), C.c_void_p]
        L.pcd_ba_device_parameters.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.pcd_ba_set_camera_parameters.argtypes = [C.c_void_p, C.c_void_p]
        L.pcd_ba_evaluate_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(BABlocks)]
        L.pcd_ba_evaluate_blocks_compact.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(BABlocksCompact)]
    if hasattr(L, "pcd_ba_schur_device"):
        L.pcd_ba_set_parameters_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pcd_ba_schur_structure.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                             C.c_void_p, C.c_void_p]
        L.pcd_ba_schur_device.argtypes = [C.c_void_p, C.POINTER(BASchurOpts), C.POINTER(BASchurOut), C.c_void_p]
        L.pcd_ba_schur.argtypes = [C.c_void_p, C.POINTER(BASchurOpts), C.POINTER(BASchurOut)]
        L.pcd_ba_schur_back_substitute_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pcd_ba_plus_device.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.pcd_ba_schur_stats.argtypes = [C.c_void_p, C.POINTER(BASchurInfo)]
    if hasattr(L, "pcd_ba_solve"):
        L.pcd_ba_pcg_opts_default.argtypes = [C.POINTER(BAPcgOpts)]
        L.pcd_ba_pcg_opts_default.restype = None
        L.pcd_ba_schur_solve_pcg_device.argtypes = [C.c_void_p, C.POINTER(BAPcgOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        L.pcd_ba_schur_solve_pcg.argtypes = [C.c_void_p, C.POINTER(BAPcgOpts), C.c_void_p, C.POINTER(BAPcgInfo)]
        L.pcd_ba_get_parameters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.pcd_ba_solve_opts_default.argtypes = [C.POINTER(BASolveOpts)]
        L.pcd_ba_solve_opts_default.restype = None
        L.pcd_ba_solve.argtypes = [C.c_void_p, C.POINTER(BASolveOpts), C.POINTER(BASolveSummary), C.c_void_p]
    if hasattr(L, "pcd_ba_schur_build_device"):
        L.pcd_ba_schur_build_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BASchurBuildInfo)]
        L.pcd_ba_schur_structure_lists.argtypes = [C.c_void_p, C.POINTER(BASchurLists)]
    if hasattr(L, "pcd_ba_schur_solve_cholesky_device"):
        L.pcd_ba_schur_solve_cholesky_device.argtypes = [C.c_void_p] * 6
        L.pcd_ba_schur_solve_cholesky.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(BACholInfo)]
    if hasattr(L, "pcd_ba_schur_cam_device"):
        L.pcd_ba_camera_slots.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
        L.pcd_ba_schur_cam_device.argtypes = [C.c_void_p, C.POINTER(BASchurOpts), C.POINTER(BASchurCamOut), C.c_void_p]
        L.pcd_ba_schur_cam.argtypes = [C.c_void_p, C.POINTER(BASchurOpts), C.POINTER(BASchurCamOut)]
        L.pcd_ba_schur_cam_solve_cholesky_device.argtypes = [C.c_void_p] * 4
        L.pcd_ba_schur_cam_back_substitute_device.argtypes = [C.c_void_p] * 5
        L.pcd_ba_plus_cam_device.argtypes = [C.c_void_p] * 7
        L.pcd_ba_get_camera_parameters.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "pcd_ba_schur_cam_solve_pcg_device"):
        L.pcd_ba_schur_cam_solve_pcg_device.argtypes = [C.c_void_p, C.POINTER(BAPcgOpts), C.c_void_p, C.c_void_p,
                                                        C.c_void_p]
        L.pcd_ba_schur_cam_solve_pcg.argtypes = [C.c_void_p, C.POINTER(BAPcgOpts), C.c_void_p, C.POINTER(BAPcgInfo)]
    if hasattr(L, "pcd_ba_set_lidar_device"):
        L.pcd_ba_set_lidar_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.pcd_ba_get_lidar.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)] + [C.c_void_p] * 5
        L.pcd_ba_lidar_device.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_void_p)] * 5
        L.pcd_ba_assoc_opts_default.argtypes = [C.POINTER(BAAssocOpts)]
        L.pcd_ba_assoc_opts_default.restype = None
        L.pcd_ba_proj_opts_default.argtypes = [C.POINTER(BAProjOpts)]
        L.pcd_ba_proj_opts_default.restype = None
        L.pcd_ba_project_lidar_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BAProjOpts), C.c_void_p,
                                                  C.POINTER(BAProjInfo)]
        L.pcd_ba_associate_lidar_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BAAssocOpts), C.c_void_p,
                                                    C.POINTER(BAAssocInfo)]
    if hasattr(L, "pcd_ba_remove_observations_device"):
        L.pcd_ba_filter_opts_default.argtypes = [C.POINTER(BAFilterOpts)]
        L.pcd_ba_filter_opts_default.restype = None
        L.pcd_ba_filter_points.argtypes = [C.c_void_p, C.POINTER(BAFilterOpts), C.POINTER(BAFilterOut)]
        L.pcd_ba_filter_points_device.argtypes = [C.c_void_p, C.POINTER(BAFilterOpts), C.POINTER(BAFilterOut), C.c_void_p]
        L.pcd_ba_remove_observations_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.POINTER(BARemoveInfo)]
    if hasattr(L, "pcd_ba_add_observations_device"):
        L.pcd_ba_add_observations_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_uint64, C.c_void_p, C.POINTER(BAAddInfo)]
        L.pcd_ba_add_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint64, C.POINTER(BAAddInfo)]
    if hasattr(L, "pcd_ba_window_create_device"):
        L.pcd_ba_window_opts_default.argtypes = [C.POINTER(BAWindowOpts)]
        L.pcd_ba_window_opts_default.restype = None
        L.pcd_ba_window_create_device.argtypes = [C.c_void_p, C.POINTER(BAWindowOpts), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(BAWindowInfo)]
        L.pcd_ba_window_commit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "pcd_ba_local_bundle_device"):
        L.pcd_ba_local_bundle_opts_default.argtypes = [C.POINTER(BALocalBundleOpts)]
        L.pcd_ba_local_bundle_opts_default.restype = None
        L.pcd_ba_local_bundle_device.argtypes = [C.c_void_p, C.POINTER(BALocalBundleOpts)] + [C.c_void_p] * 6
        L.pcd_ba_local_bundle.argtypes = [C.c_void_p, C.POINTER(BALocalBundleOpts)] + [C.c_void_p] * 4
        L.pcd_ba_local_window_opts_default.argtypes = [C.POINTER(BALocalWindowOpts)]
        L.pcd_ba_local_window_opts_default.restype = None
        L.pcd_ba_local_window_create_device.argtypes = [C.c_void_p, C.POINTER(BALocalWindowOpts), C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(BALocalWindowInfo)]
    _LIB = L
    return L


def _check(st):
    if st != PCD_OK:
        raise PcdError(st, lib().pcd_last_error().decode(errors="replace"))


def device_count():
    return lib().pcd_device_count()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr(x):
    """numpy array -> host pointer; int -> raw (device) pointer; torch tensor -> data_ptr()."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


def normals_options(radius=0.15, min_neighbors=3, orient=None, viewpoint=(0, 0, 0), only_missing=False):
    o = NormalsOptions()
    lib().pcd_normals_options_default(C.byref(o))
    o.radius, o.min_neighbors, o.only_missing = radius, min_neighbors, int(bool(only_missing))
    if orient is not None:
        o.orient = orient
    o.viewpoint[:] = [float(v) for v in viewpoint]
    return o


def voxel_options(leaf=0.05, min_points=0, cell_size=0.0):
    """pcd_voxel_options; leaf: one edge for all three axes, or three"""
    o = VoxelOptions()
    lib().pcd_voxel_options_default(C.byref(o))
    l3 = np.broadcast_to(np.asarray(leaf, np.float32), (3,))
    o.leaf[:] = [float(v) for v in l3]
    o.min_points, o.cell_size = int(min_points), float(cell_size)
    return o


def _voxel_info(i):
    d = {k: getattr(i, k) for k, _ in VoxelInfo._fields_}
    d["min_b"], d["dims"] = list(i.min_b), list(i.dims)
    return d


class Cloud:
    """Device-resident LiDAR cloud index (reference: lidar::PointCloudProcess + lidar::Kdtree)."""

    def __init__(self, xyz, nrm=None, device=0, raw_lidar_frame=True, cell_size=0.0, layout=LAYOUT_XYZ_NRM,
                 index_base=0, index_stride=1):
        xyz = np.ascontiguousarray(xyz, np.float32)
        n = xyz.shape[0] if xyz.ndim > 1 else 0
        if layout == LAYOUT_XYZ_NRM:
            xyz = xyz.reshape(-1, 3)
            nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
            assert nrm.shape[0] == xyz.shape[0]
            n = xyz.shape[0]
        else:
            xyz = xyz.reshape(-1, 8)
            n = xyz.shape[0]
        o = CloudOptions()
        lib().pcd_cloud_options_default(C.byref(o))
        o.device, o.layout, o.raw_lidar_frame, o.cell_size = device, layout, int(raw_lidar_frame), cell_size
        o.index_base, o.index_stride = index_base, index_stride
        h = C.c_void_p()
        self._h = None
        _check(lib().pcd_cloud_create(_vp(xyz), _vp(nrm), n, C.byref(o), C.byref(h)))
        self._h = h
        self.device = device

    @classmethod
    def _from_handle(cls, handle, device=0):
        """a Cloud that OWNS an existing pcd_cloud* (what pcd_cloud_voxel_downsample returns)"""
        c = cls.__new__(cls)
        c._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        c.device = device
        return c

    def close(self):
        if self._h:
            lib().pcd_cloud_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def __len__(self):
        return int(lib().pcd_cloud_size(self._h))

    def info(self):
        i = CloudInfo()
        _check(lib().pcd_cloud_get_info(self._h, C.byref(i)))
        return dict(cell_size=i.cell_size, origin=list(i.origin), dims=list(i.dims), block_dims=list(i.block_dims),
                    num_indexed=i.num_indexed, occupied_cells=i.occupied_cells, build_ms=i.build_ms,
                    bbox_lo=list(i.bbox_lo), bbox_hi=list(i.bbox_hi))

    def download(self):
        n = len(self)
        xyz = np.empty((n, 3), np.float32)
        nrm = np.empty((n, 3), np.float32)
        _check(lib().pcd_cloud_download(self._h, _vp(xyz), _vp(nrm)))
        return xyz, nrm

    def estimate_normals(self, radius=0.15, min_neighbors=3, orient=NORMALS_ORIENT_VIEWPOINT, viewpoint=(0, 0, 0),
                         only_missing=False):
        """Radius-PCA normals for every row, stored in the handle (pcd_cloud_estimate_normals): returns the
        neighbour count (uint32) and curvature (float64) per row and the info counters as a dict."""
        n = len(self)
        count = np.empty(n, np.uint32)
        curv = np.empty(n, np.float64)
        info = NormalsInfo()
        o = normals_options(radius, min_neighbors, orient, viewpoint, only_missing)
        _check(lib().pcd_cloud_estimate_normals(self._h, C.byref(o), _vp(count), _vp(curv), C.byref(info)))
        return {"count": count, "curvature": curv, "info": {k: getattr(info, k) for k, _ in NormalsInfo._fields_}}

    def estimate_normals_device(self, d_count=None, d_curvature=None, radius=0.15, min_neighbors=3,
                                orient=NORMALS_ORIENT_VIEWPOINT, viewpoint=(0, 0, 0), only_missing=False, stream=0):
        """the same with device outputs (torch tensors or raw pointers; either may be None), asynchronous on `stream`"""
        o = normals_options(radius, min_neighbors, orient, viewpoint, only_missing)
        _check(lib().pcd_cloud_estimate_normals_device(self._h, C.byref(o), _ptr(d_count), _ptr(d_curvature),
                                                       C.c_void_p(stream)))

    def voxel_downsample(self, leaf, min_points=0, cell_size=0.0, want_map=False):
        """Voxel-grid downsampling into a NEW handle (pcd_cloud_voxel_downsample): returns (Cloud, info dict), with
        want_map also row_voxel (uint32 per row of this cloud: its output row, 0xFFFFFFFF for none).  leaf: one edge or
        three; cell_size is the new handle's.  This cloud is not modified."""
        o = voxel_options(leaf, min_points, cell_size)
        row_voxel = np.empty(len(self), np.uint32) if want_map else None
        h, info = C.c_void_p(), VoxelInfo()
        _check(lib().pcd_cloud_voxel_downsample(self._h, C.byref(o), _vp(row_voxel), C.byref(h), C.byref(info)))
        out = Cloud._from_handle(h, self.device)
        return (out, _voxel_info(info), row_voxel) if want_map else (out, _voxel_info(info))

    def voxel_downsample_device(self, d_row_voxel, leaf, min_points=0, cell_size=0.0, stream=0):
        """the same with the map written to device memory (a torch int32 tensor of len(self) or a raw pointer; may be
        None), on `stream` -- which is synchronised: the row count sizes the new handle.  Returns (Cloud, info)."""
        o = voxel_options(leaf, min_points, cell_size)
        h, info = C.c_void_p(), VoxelInfo()
        _check(lib().pcd_cloud_voxel_downsample_device(self._h, C.byref(o), _ptr(d_row_voxel), C.c_void_p(stream),
                                                       C.byref(h), C.byref(info)))
        return Cloud._from_handle(h, self.device), _voxel_info(info)

    def nn(self, q, algo=NN_AUTO):
        """Kdtree::GetClosestPoint for a batch: returns (idx uint32, sqdist float32, found uint8)."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
        Q = q.shape[0]
        idx = np.empty(Q, np.uint32)
        sq = np.empty(Q, np.float32)
        found = np.empty(Q, np.uint8)
        _check(lib().pcd_nn_query_algo(self._h, _vp(q), Q, algo, _vp(idx), _vp(sq), _vp(found)))
        return idx, sq, found

    def nn_device(self, d_q, Q, d_keys, algo=NN_AUTO, stream=0):
        _check(lib().pcd_nn_query_device(self._h, _ptr(d_q), Q, algo, _ptr(d_keys), C.c_void_p(stream)))

    def nn_refine_device(self, d_q, Q, d_keys, d_skip=None, stream=0):
        """second phase of a sharded search: keys in/out (pcd_nn_refine_device)"""
        L = lib()
        L.pcd_nn_refine_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.pcd_nn_refine_device(self._h, _ptr(d_q), Q, _ptr(d_skip), _ptr(d_keys), C.c_void_p(stream)))

    def associate(self, q, max_range=None, gate_mode=GATE_MAPPER_LOCAL):
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
        Q = q.shape[0]
        out = dict(lidar_xyz=np.empty((Q, 3)), abcd=np.empty((Q, 4)), type=np.empty(Q, np.uint8),
                   dist=np.empty(Q), angle=np.empty(Q), dist2plane=np.empty(Q),
                   nn_idx=np.empty(Q, np.uint32), nn_sqdist=np.empty(Q, np.float32))
        ao = AssocOut(*[_vp(out[k]) for k in ("lidar_xyz", "abcd", "type", "dist", "angle", "dist2plane",
                                               "nn_idx", "nn_sqdist")])
        mr, mrc = None, 0
        if (gate_mode & 0xFF) != GATE_CONTROLLER:
            mr = np.ascontiguousarray(np.atleast_1d(np.asarray(max_range, np.float64)))
            mrc = mr.shape[0]
        _check(lib().pcd_associate(self._h, _vp(q), Q, _vp(mr), mrc, gate_mode, C.byref(ao)))
        return out

    def staging(self, Q):
        """pinned input buffers of the staged host path: (q_xyz [Q][3], max_range [Q]) numpy views"""
        L = lib()
        L.pcd_assoc_staging.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        a, b = C.c_void_p(), C.c_void_p()
        _check(L.pcd_assoc_staging(self._h, Q, C.byref(a), C.byref(b)))
        q = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_double)), shape=(max(Q, 1), 3))[:Q]
        mr = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_double)), shape=(max(Q, 1),))[:Q]
        return q, mr

    def associate_staged(self, Q, mr_count, gate_mode=GATE_MAPPER_LOCAL):
        """runs on the buffers of staging(); returns the accepted associations as a structured numpy view (80-byte
        records, ascending query) of the handle's pinned result buffer -- valid until the next call"""
        L = lib()
        L.pcd_associate_staged.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_uint64)]
        h, n = C.c_void_p(), C.c_uint64(0)
        _check(L.pcd_associate_staged(self._h, Q, mr_count, gate_mode, C.byref(h), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, HIT_DTYPE)
        buf = (C.c_char * (80 * n.value)).from_address(h.value)
        return np.frombuffer(buf, dtype=HIT_DTYPE, count=n.value)

    def associate_device(self, d_q, Q, d_max_range, mr_count, gate_mode, d_out, d_keys_in=None, stream=0):
        ao = AssocOut(*[_ptr(d_out.get(k)) for k in ("lidar_xyz", "abcd", "type", "dist", "angle", "dist2plane",
                                                      "nn_idx", "nn_sqdist")])
        _check(lib().pcd_associate_device(self._h, _ptr(d_q), Q, _ptr(d_max_range), mr_count, gate_mode,
                                          _ptr(d_keys_in), C.byref(ao), C.c_void_p(stream)))

    def winner_payload_device(self, d_keys, Q, d_payload, stream=0):
        _check(lib().pcd_nn_winner_payload_device(self._h, _ptr(d_keys), Q, _ptr(d_payload), C.c_void_p(stream)))

    def last_stats(self):
        s = NNStats()
        _check(lib().pcd_nn_last_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in NNStats._fields_}

    def last_wave_records(self):
        """(records, nitems) of the last grid-path call: nitems = its work items; records = uint64 [waves, 3] of
        {start, end, items} per wavefront of the brick kernel (wall-clock ticks), kept only by a statistics pass with
        set_nn_tuning(collect_stats=5), else empty"""
        L = lib()
        nw, ni = C.c_uint64(0), C.c_uint64(0)
        _check(L.pcd_nn_last_wave_records(self._h, None, 0, C.byref(nw), C.byref(ni)))
        rec = np.zeros((nw.value, 3), np.uint64)
        if nw.value:
            _check(L.pcd_nn_last_wave_records(self._h, _vp(rec), nw.value, C.byref(nw), C.byref(ni)))
        return rec, int(ni.value)

    def last_fb_wave_records(self):
        """(records, waves per workgroup) of the last call that ran the fallback walk: records = uint64 [waves, 3] of
        {start, end, walk steps} per wavefront of k_nn_fallback (wall-clock ticks), in the order workgroup * waves per
        workgroup + wave; kept only by a pass with set_nn_tuning(collect_stats=16), else empty"""
        L = lib()
        nw, wpb = C.c_uint64(0), C.c_uint64(0)
        _check(L.pcd_nn_last_fb_wave_records(self._h, None, 0, C.byref(nw), C.byref(wpb)))
        rec = np.zeros((nw.value, 3), np.uint64)
        if nw.value:
            _check(L.pcd_nn_last_fb_wave_records(self._h, _vp(rec), nw.value, C.byref(nw), C.byref(wpb)))
        return rec, int(wpb.value)


def associate_from_payload_device(device, d_q, Q, d_max_range, mr_count, gate_mode, d_keys, d_payload, d_out,
                                  stream=0):
    ao = AssocOut(*[_ptr(d_out.get(k)) for k in ("lidar_xyz", "abcd", "type", "dist", "angle", "dist2plane",
                                                  "nn_idx", "nn_sqdist")])
    _check(lib().pcd_associate_from_payload_device(device, _ptr(d_q), Q, _ptr(d_max_range), mr_count, gate_mode,
                                                   _ptr(d_keys), _ptr(d_payload), C.byref(ao), C.c_void_p(stream)))


class ShardReduce(C.Structure):
    """pcd_shard_reduce: the exchange steps of the sharded search (NULL members: the library's own peer-copy reduction)"""
    MINFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_uint64)
    SUMFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_uint64)
    _fields_ = [("min_u64", MINFN), ("sum_i32", SUMFN), ("user", C.c_void_p)]


class _BorrowedCloud(Cloud):
    """a Cloud over a handle somebody else owns: close() forgets the handle instead of destroying it"""

    def __init__(self, handle, owner):
        self._h = C.c_void_p(handle)
        self._owner = owner          # keeps the owner alive
        self.device = 0

    def close(self):
        self._h = None


class ShardedCloud:
    """One cloud over several devices of this process (pcd_cloud_create_sharded): what a multi-GPU C++ host builds in
    LoadPointcloud.  devices may repeat (tests put every shard on device 0)."""

    def __init__(self, xyz, nrm, devices, raw_lidar_frame=True, cell_size=0.0, layout=LAYOUT_XYZ_NRM):
        L = lib()
        xyz = np.ascontiguousarray(xyz, np.float32)
        if layout == LAYOUT_AOS32:
            xyz, nrm = xyz.reshape(-1, 8), None        # one array of 8-float rows, nrm ignored
        else:
            nrm = np.ascontiguousarray(nrm, np.float32)
        o = CloudOptions()
        L.pcd_cloud_options_default(C.byref(o))
        o.layout = layout
        o.raw_lidar_frame = int(raw_lidar_frame)
        o.cell_size = cell_size
        dv = (C.c_int * len(devices))(*devices)
        L.pcd_cloud_create_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CloudOptions), C.POINTER(C.c_int),
                                               C.c_int, C.POINTER(C.c_void_p)]
        L.pcd_cloud_shards_destroy.argtypes = [C.c_void_p]
        L.pcd_cloud_shards_destroy.restype = None
        L.pcd_cloud_shards_size.argtypes = [C.c_void_p]
        L.pcd_cloud_shards_size.restype = C.c_uint64
        L.pcd_cloud_shards_count.argtypes = [C.c_void_p]
        L.pcd_cloud_shards_get.argtypes = [C.c_void_p, C.c_int]
        L.pcd_cloud_shards_get.restype = C.c_void_p
        self._h = C.c_void_p()
        n = xyz.shape[0]
        _check(L.pcd_cloud_create_sharded(_vp(xyz) if n else None, _vp(nrm) if n and nrm is not None else None, n,
                                          C.byref(o), dv, len(devices), C.byref(self._h)))

    def __len__(self):
        return int(lib().pcd_cloud_shards_size(self._h))

    def count(self):
        """number of shards (pcd_cloud_shards_count)"""
        return int(lib().pcd_cloud_shards_count(self._h))

    def shard(self, i):
        """shard i as a Cloud (pcd_cloud_shards_get).  Borrowed: it answers with the ORIGINAL row indices of the whole
        cloud, lives as long as this object and is not destroyed by its own close()."""
        h = lib().pcd_cloud_shards_get(self._h, int(i))
        if not h:
            raise IndexError(f"shard {i} of {self.count()}")
        return _BorrowedCloud(h, self)

    def close(self):
        if self._h:
            lib().pcd_cloud_shards_destroy(self._h)
            self._h = None

    def nn(self, q, reduce=None):
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
        Q = q.shape[0]
        idx = np.empty(Q, np.uint32); sq = np.empty(Q, np.float32); found = np.empty(Q, np.uint8)
        L = lib()
        L.pcd_nn_query_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.pcd_nn_query_sharded(self._h, _vp(q) if Q else None, Q, C.byref(reduce) if reduce is not None else None,
                                      _vp(idx), _vp(sq), _vp(found)))
        return idx, sq, found

    def associate(self, q, max_range, gate_mode=0, reduce=None):
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
        Q = q.shape[0]
        mr = np.ascontiguousarray(np.atleast_1d(max_range), np.float64)
        out = dict(lidar_xyz=np.zeros((Q, 3)), abcd=np.zeros((Q, 4)), type=np.zeros(Q, np.uint8), dist=np.zeros(Q),
                   angle=np.zeros(Q), dist2plane=np.zeros(Q), nn_idx=np.zeros(Q, np.uint32), nn_sqdist=np.zeros(Q, np.float32))
        ao = AssocOut(*[_vp(out[k]) for k in ("lidar_xyz", "abcd", "type", "dist", "angle", "dist2plane", "nn_idx", "nn_sqdist")])
        L = lib()
        L.pcd_associate_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                            C.POINTER(AssocOut)]
        _check(L.pcd_associate_sharded(self._h, _vp(q), Q, _vp(mr), mr.shape[0], gate_mode,
                                       C.byref(reduce) if reduce is not None else None, C.byref(ao)))
        return out


def _sift_pair(d1, d2, max_ratio, max_distance, cross_check, device, guide=None):
    """pcd_sift_match, or with guide = (loc1, loc2, H, F, h_max_residual, f_max_residual) pcd_sift_match_guided"""
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 128)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 128)
    n1, n2 = d1.shape[0], d2.shape[0]
    m = np.zeros((max(n1, 1), 2), np.uint32)
    cnt = C.c_int32(0)
    vp = lambda a: _vp(a) if a is not None and a.shape[0] else None
    tail = (C.c_float(max_ratio), C.c_float(max_distance), int(cross_check), _vp(m), C.byref(cnt))
    if guide is None:
        _check(lib().pcd_sift_match(device, vp(d1), n1, vp(d2), n2, *tail))
    else:
        loc1, loc2, H, F, th, tf = guide
        l1 = np.ascontiguousarray(loc1, np.float32).reshape(n1, 2)
        l2 = np.ascontiguousarray(loc2, np.float32).reshape(n2, 2)
        _check(lib().pcd_sift_match_guided(device, vp(d1), vp(l1), n1, vp(d2), vp(l2), n2, vp(_mat3(H)), vp(_mat3(F)),
                                           C.c_float(th), C.c_float(tf), *tail))
    return m[:cnt.value].copy()


def sift_match(d1, d2, max_ratio=0.8, max_distance=0.7, cross_check=True, device=0):
    """MatchSiftFeaturesCPUBruteForce semantics on the GPU: returns matches [M][2] uint32"""
    return _sift_pair(d1, d2, max_ratio, max_distance, cross_check, device)


def sift_match_device(d_d1, n1, d_d2, n2, d_m12, d_m21, d_matches, d_count, max_ratio=0.8, max_distance=0.7,
                      cross_check=True, device=0, stream=0):
    L = lib()
    L.pcd_sift_match_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(L.pcd_sift_match_device(device, _ptr(d_d1), n1, _ptr(d_d2), n2, max_ratio, max_distance, int(cross_check),
                                   _ptr(d_m12), _ptr(d_m21), _ptr(d_matches), _ptr(d_count), C.c_void_p(stream)))


SIFT_GUIDE_NONE, SIFT_GUIDE_H, SIFT_GUIDE_F, SIFT_GUIDE_HF = 0, 1, 2, 3


class SiftGuide(C.Structure):
    """pcd_sift_guide: mode (SIFT_GUIDE_*) and the row-major 3x3 H / F of one pair"""
    _fields_ = [("mode", C.c_int32), ("H", C.c_float * 9), ("F", C.c_float * 9)]


def _mat3(m):
    return None if m is None else np.ascontiguousarray(m, np.float32).reshape(9)


def _sift_arena(arrays, dtype=np.uint8, width=128):
    """list of [n_i][width] arrays -> (arena [sum n_i][width], first_row [len + 1] uint64)"""
    ds = [np.ascontiguousarray(d, dtype).reshape(-1, width) for d in arrays]
    first = np.zeros(len(ds) + 1, np.uint64)
    first[1:] = np.cumsum([d.shape[0] for d in ds])
    arena = np.concatenate(ds, axis=0) if ds and first[-1] else np.zeros((0, width), dtype)
    return np.ascontiguousarray(arena), first


def _sift_batch(descriptors, pairs, max_ratio, max_distance, cross_check, device, guide=None):
    """pcd_sift_match_batch, or with guide = (locations, guides, h_max_residual, f_max_residual)
    pcd_sift_match_guided_batch"""
    arena, first = _sift_arena(descriptors)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    P = pairs.shape[0]
    off = np.zeros(P + 1, np.uint64)
    n1 = (first[1:] - first[:-1])[pairs[:, 0]] if P else np.zeros(0, np.uint64)
    cap = int(n1.sum())   # worst case: one match per descriptor of every pair's first image
    m = np.zeros((max(cap, 1), 2), np.uint32)
    vp = lambda a: _vp(a) if a.shape[0] else None
    head = (device, vp(arena))
    mid = (_vp(first), len(descriptors), vp(pairs), P)
    tail = (C.c_float(max_ratio), C.c_float(max_distance), int(cross_check), _vp(m), C.c_uint64(cap),
            _vp(off))
    if guide is None:
        _check(lib().pcd_sift_match_batch(*head, *mid, *tail))
    else:
        locations, guides, th, tf = guide
        loc_arena, lfirst = _sift_arena(locations, np.float32, 2)
        assert np.array_equal(lfirst, first)
        g = (SiftGuide * max(P, 1))()
        for p, (H, F) in enumerate(guides):
            g[p].mode = (SIFT_GUIDE_H if H is not None else 0) | (SIFT_GUIDE_F if F is not None else 0)
            if H is not None:
                g[p].H[:] = [float(v) for v in _mat3(H)]
            if F is not None:
                g[p].F[:] = [float(v) for v in _mat3(F)]
        _check(lib().pcd_sift_match_guided_batch(*head, vp(loc_arena), *mid, C.cast(g, C.c_void_p), C.c_float(th),
                                                 C.c_float(tf), *tail))
    return [m[int(off[p]):int(off[p + 1])].copy() for p in range(P)]


def sift_match_batch(descriptors, pairs, max_ratio=0.8, max_distance=0.7, cross_check=True, device=0):
    """SiftFeatureMatcher::Match(image_pairs) (feature/matching.cc:798): `descriptors` = one [n_i][128] uint8 array
    per image, `pairs` = [P][2] image indices.  Returns a list of P match arrays [M_p][2] uint32, each equal to
    sift_match(descriptors[a], descriptors[b])."""
    return _sift_batch(descriptors, pairs, max_ratio, max_distance, cross_check, device)


def sift_match_guided(d1, loc1, d2, loc2, H=None, F=None, h_max_residual=16.0, f_max_residual=16.0, max_ratio=0.8,
                      max_distance=0.7, cross_check=True, device=0):
    """MatchGuidedSiftFeaturesCPU semantics (feature/sift.cc:1092-1162) on the GPU: loc1 / loc2 [n][2] float32, H / F
    row-major 3x3 or None; returns matches [M][2] uint32 (with neither matrix: exactly sift_match)"""
    return _sift_pair(d1, d2, max_ratio, max_distance, cross_check, device,
                      (loc1, loc2, H, F, h_max_residual, f_max_residual))


def sift_match_guided_batch(descriptors, locations, pairs, guides, h_max_residual=16.0, f_max_residual=16.0,
                            max_ratio=0.8, max_distance=0.7, cross_check=True, device=0):
    """GuidedSiftGPUFeatureMatcher's per-pair loop (feature/matching.cc:523-575) in one call: `locations` = one [n_i][2]
    float32 array per image, `guides` = one (H or None, F or None) per pair.  Returns a list of P match arrays, each
    equal to sift_match_guided(...) of that pair."""
    return _sift_batch(descriptors, pairs, max_ratio, max_distance, cross_check, device,
                       (locations, guides, h_max_residual, f_max_residual))


def exhaustive_blocks(n_images, block_size=50):
    """The image-pair lists of ExhaustiveFeatureMatcher::Run (feature/matching.cc:902-960), one per block pair, in the
    reference's order: blocks of `block_size` consecutive images, pair (i1, i2) taken when
    (i1 > i2 and i1 % B <= i2 % B) or (i1 < i2 and i1 % B < i2 % B) -- every unordered pair exactly once.  Each list
    is what the reference hands to SiftFeatureMatcher::Match(image_pairs) = sift_match_batch[_device]."""
    B = int(block_size)
    for s1 in range(0, n_images, B):
        e1 = min(n_images, s1 + B)
        for s2 in range(0, n_images, B):
            e2 = min(n_images, s2 + B)
            i1, i2 = np.meshgrid(np.arange(s1, e1), np.arange(s2, e2), indexing="ij")
            b1, b2 = i1 % B, i2 % B
            keep = ((i1 > i2) & (b1 <= b2)) | ((i1 < i2) & (b1 < b2))
            yield np.stack([i1[keep], i2[keep]], axis=1).astype(np.uint32)


def sift_match_batch_device(d_arena, first_row, pairs, d_matches, match_offset, d_counts, max_ratio=0.8,
                            max_distance=0.7, cross_check=True, device=0, stream=0):
    """device form: first_row / pairs / match_offset are numpy (host) arrays, the rest torch device tensors"""
    first_row = np.ascontiguousarray(first_row, np.uint64)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    match_offset = np.ascontiguousarray(match_offset, np.uint64)
    L = lib()
    L.pcd_sift_match_batch_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                              C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(L.pcd_sift_match_batch_device(device, _ptr(d_arena), _vp(first_row), first_row.shape[0] - 1, _vp(pairs),
                                         pairs.shape[0], max_ratio, max_distance, int(cross_check), _ptr(d_matches),
                                         _vp(match_offset), _ptr(d_counts), C.c_void_p(stream)))


def filter_lidar_outlier_device(d_points, d_lidar_xyz, d_type, n, max_proj, max_icp, d_erase, device=0, stream=0):
    L = lib()
    L.pcd_filter_lidar_outlier_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    _check(L.pcd_filter_lidar_outlier_device(device, _ptr(d_points), _ptr(d_lidar_xyz), _ptr(d_type), n, max_proj,
                                             max_icp, _ptr(d_erase), C.c_void_p(stream)))


class Projector:
    """Depth-projection association over a Cloud (reference: lidar::PcdProj, lidar/pcd_projection.h:48-185)."""

    def __init__(self, cloud, options=None, **kw):
        L = lib()
        L.pcd_proj_create.argtypes = [C.c_void_p, C.POINTER(ProjOptions), C.POINTER(C.c_void_p)]
        L.pcd_proj_destroy.argtypes = [C.c_void_p]
        L.pcd_proj_destroy.restype = None
        L.pcd_proj_num_submaps.argtypes = [C.c_void_p]
        L.pcd_proj_num_submaps.restype = C.c_uint64
        L.pcd_proj_last_pairs.argtypes = [C.c_void_p]
        L.pcd_proj_last_pairs.restype = C.c_uint64
        L.pcd_proj_scale_coeffs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.pcd_proj_set_new_images.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ProjImage), C.c_uint64] + \
            [C.c_void_p] * 6
        L.pcd_proj_set_new_images_device.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ProjImage), C.c_uint64] + \
            [C.c_void_p] * 7
        if options is None:
            options = ProjOptions()
            L.pcd_proj_default_options(C.byref(options))
        for k, v in kw.items():
            setattr(options, k, v)
        self.options = options
        self._cloud = cloud          # keep the cloud alive
        self._h = None
        h = C.c_void_p()
        _check(L.pcd_proj_create(cloud._h, C.byref(options), C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().pcd_proj_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_submaps(self):
        return int(lib().pcd_proj_num_submaps(self._h))

    @property
    def last_pairs(self):
        return int(lib().pcd_proj_last_pairs(self._h))

    def scale_coeffs(self, set_to=None):
        c4 = np.zeros(4, np.float64) if set_to is None else np.ascontiguousarray(set_to, np.float64)
        latched = C.c_int(0)
        _check(lib().pcd_proj_scale_coeffs(self._h, 0 if set_to is None else 1, _vp(c4), C.byref(latched)))
        return c4, bool(latched.value)

    @staticmethod
    def _images(images):
        arr = (ProjImage * max(len(images), 1))()
        for k, im in enumerate(images):
            arr[k] = ProjImage((C.c_double * 4)(*im["qvec"]), (C.c_double * 3)(*im["tvec"]),
                               (C.c_double * 8)(*im["params"]), im["width"], im["height"], im["feat_begin"],
                               im["feat_end"])
        return arr

    def set_new_images_device(self, images, d_feat_xy, want=("found", "lidar_index", "dist", "lidar6", "cam_xyz"),
                              stream=None):
        """pcd_proj_set_new_images_device: d_feat_xy is a torch device tensor [n_feat][2] float64 on the cloud's device;
        the outputs named in `want` are allocated there and returned as a dict of torch tensors (the others are not
        computed).  All work is on `stream` (a raw handle; None: torch's current stream), which is synchronised once."""
        import torch
        d_feat_xy = d_feat_xy.contiguous()
        assert d_feat_xy.dtype == torch.float64 and d_feat_xy.is_cuda
        nf = int(d_feat_xy.numel()) // 2
        if stream is None:
            stream = torch.cuda.current_stream(d_feat_xy.device).cuda_stream
        shapes = dict(found=((nf,), torch.uint8), lidar_index=((nf,), torch.int32), dist=((nf,), torch.float32),
                      lidar6=((nf, 6), torch.float64), cam_xyz=((nf, 3), torch.float64))
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=d_feat_xy.device) for k in want}
        ptr = [_ptr(out.get(k)) for k in ("found", "lidar_index", "dist", "lidar6", "cam_xyz")]
        _check(lib().pcd_proj_set_new_images_device(self._h, len(images), self._images(images), nf, _ptr(d_feat_xy), *ptr,
                                                    C.c_void_p(stream)))
        return out

    def set_new_images(self, images, feat_xy):
        """images: list of dict(qvec, tvec, params[8], width, height, feat_begin, feat_end).
        Returns found, lidar_index, dist, lidar6, cam_xyz."""
        feat_xy = np.ascontiguousarray(feat_xy, np.float64).reshape(-1, 2)
        nf = feat_xy.shape[0]
        arr = self._images(images)
        found = np.zeros(nf, np.uint8)
        index = np.zeros(nf, np.uint32)
        dist = np.zeros(nf, np.float32)
        l6 = np.zeros((nf, 6), np.float64)
        cam = np.zeros((nf, 3), np.float64)
        _check(lib().pcd_proj_set_new_images(self._h, len(images), arr, nf, _vp(feat_xy), _vp(found), _vp(index),
                                             _vp(dist), _vp(l6), _vp(cam)))
        return found, index, dist, l6, cam


def camera_param_groups(model_id):
    """0 focal length / 1 principal point / 2 extra parameter, per parameter of the model"""
    k = lib().pcd_camera_num_params(int(model_id))
    g = np.zeros(max(k, 1), np.uint8)
    L = lib()
    L.pcd_camera_param_groups.argtypes = [C.c_int, C.c_void_p]
    _check(L.pcd_camera_param_groups(int(model_id), _vp(g)))
    return g[:k]


def camera_refine_mask(cam_model, refine_focal_length, refine_principal_point, refine_extra_params,
                       constant_cameras=()):
    """BundleAdjuster::ParameterizeCameras (optim/bundle_adjustment.cc:1047-1100) as a flat mask over cam_params"""
    sel = [bool(refine_focal_length), bool(refine_principal_point), bool(refine_extra_params)]
    out = []
    for c, m in enumerate(cam_model):
        g = camera_param_groups(m)
        out.extend([0] * len(g) if c in constant_cameras else [int(sel[x]) for x in g])
    return np.array(out, np.uint8)


def search_range_schedule(opt_num, kd_max=1.5, kd_min=0.2, drop=0.1):
    opt_num = np.ascontiguousarray(opt_num, np.int32)
    out = np.empty(opt_num.shape[0], np.float64)
    _check(lib().pcd_search_range_schedule(_vp(opt_num), opt_num.shape[0], kd_max, kd_min, drop, _vp(out)))
    return out


def set_nn_tuning(brick_cells=0, halo_cells=-1, collect_stats=0):
    """statistics switch of the grid path; the brick geometry is fixed at 2 / 2 (0 / -1 = leave it), others are refused"""
    _check(lib().pcd_nn_set_tuning(int(brick_cells), int(halo_cells), int(collect_stats)))


def set_nn_search(kernel=0):
    """first stage of the grid path: 0 = clipped brick kernel (default), 1 = the same with the clip off (stages the whole
    region: the A/B reference)"""
    _check(lib().pcd_nn_set_search(int(kernel)))


def set_nn_schedule(schedule=0):
    """how the brick kernel's work items are spread over its wavefronts: 0 = static rounds, then chunks handed out from a
    cursor per block class (default), 1 = the static strided schedule alone (the A/B reference; results identical)"""
    _check(lib().pcd_nn_set_schedule(int(schedule)))


def nn_schedule_params():
    """(static share of a wavefront's rounds in percent, items per chunk) of schedule 0: compile-time constants"""
    a, b = C.c_int(0), C.c_int(0)
    _check(lib().pcd_nn_schedule_params(C.byref(a), C.byref(b)))
    return a.value, b.value


def set_sift_tuning(nchunk=0, batch_partials=0):
    """tests / fuzzing: column chunks per stripe walk and partial results per sub-batch, counted in int4 elements
    (16-byte units); 0 = the library's choice"""
    L = lib()
    L.pcd_sift_set_tuning.argtypes = [C.c_int, C.c_uint64]
    _check(L.pcd_sift_set_tuning(int(nchunk), int(batch_partials)))


def set_nn_bookkeeping(radix_sort=0):
    _check(lib().pcd_nn_set_bookkeeping(int(radix_sort)))


def profile_enable(on=True):
    lib().pcd_profile_enable(int(on))


def profile_only(scope=None):
    """time just one scope (None: all of them)"""
    L = lib()
    L.pcd_profile_only.argtypes = [C.c_char_p]
    L.pcd_profile_only(scope.encode() if scope else None)


def profile_reset():
    lib().pcd_profile_reset()


def profile_get():
    arr = (KernelTime * 64)()
    n = C.c_int(0)
    lib().pcd_profile_get(arr, 64, C.byref(n))
    return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n.value, 64))}


class BA:
    """Flat BA problem on the device (reference: what BundleAdjuster::SetUp*ByLidar builds for Ceres)."""

    def __init__(self, cam_model, cam_params_list, poses, image_camera, points, obs_image, obs_point, obs_xy,
                 lidar_point=None, lidar_abcd=None, lidar_weight=None, image_const_pose=None,
                 image_const_tvec=None, point_const=None, loss_type=LOSS_TRIVIAL, loss_scale=1.0, device=0,
                 camera_refine=None):
        self.cam_model = np.ascontiguousarray(cam_model, np.int32)
        offs, flat = [], []
        for cp in cam_params_list:
            offs.append(len(flat))
            flat.extend(list(cp))
        self.cam_param_off = np.ascontiguousarray(offs, np.int32)
        self.cam_params = np.ascontiguousarray(flat, np.float64)
        self.poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        self.image_camera = np.ascontiguousarray(image_camera, np.int32)
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self.obs_image = np.ascontiguousarray(obs_image, np.int32)
        self.obs_point = np.ascontiguousarray(obs_point, np.int32)
        self.obs_xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
        nl = 0 if lidar_point is None else len(lidar_point)
        self.lidar_point = np.ascontiguousarray(lidar_point if nl else [], np.int32)
        self.lidar_abcd = np.ascontiguousarray(lidar_abcd if nl else [], np.float64).reshape(-1, 4)
        self.lidar_weight = np.ascontiguousarray(lidar_weight if nl else [], np.float64)
        self.I, self.P, self.O, self.L = self.poses.shape[0], self.points.shape[0], len(self.obs_image), nl
        self.image_const_pose = None if image_const_pose is None else np.ascontiguousarray(image_const_pose, np.uint8)
        self.image_const_tvec = None if image_const_tvec is None else np.ascontiguousarray(image_const_tvec, np.uint8)
        self.point_const = None if point_const is None else np.ascontiguousarray(point_const, np.uint8)
        d = BADesc()
        d.device = device
        d.num_cameras = len(self.cam_model); d.cam_model = _vp(self.cam_model)
        d.cam_param_offset = _vp(self.cam_param_off); d.cam_params = _vp(self.cam_params)
        d.cam_params_len = len(self.cam_params)
        d.num_images = self.I; d.poses = _vp(self.poses); d.image_camera = _vp(self.image_camera)
        d.image_const_pose = _vp(self.image_const_pose); d.image_const_tvec = _vp(self.image_const_tvec)
        d.num_points = self.P; d.points = _vp(self.points); d.point_const = _vp(self.point_const)
        d.num_obs = self.O; d.obs_image = _vp(self.obs_image); d.obs_point = _vp(self.obs_point)
        d.obs_xy = _vp(self.obs_xy)
        d.num_lidar = nl; d.lidar_point = _vp(self.lidar_point); d.lidar_abcd = _vp(self.lidar_abcd)
        d.lidar_weight = _vp(self.lidar_weight)
        d.loss_type, d.loss_scale = int(loss_type), float(loss_scale)
        self.camera_refine = None if camera_refine is None else np.ascontiguousarray(camera_refine, np.uint8)
        if self.camera_refine is not None:
            assert self.camera_refine.shape[0] == len(self.cam_params)
            d.camera_refine = _vp(self.camera_refine)
        self.C = len(self.cam_model)
        self.device = device
        h = C.c_void_p()
        self._h = None
        _check(lib().pcd_ba_create(C.byref(d), C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().pcd_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def set_parameters(self, poses=None, points=None):
        p = None if poses is None else np.ascontiguousarray(poses, np.float64)
        x = None if points is None else np.ascontiguousarray(points, np.float64)
        _check(lib().pcd_ba_set_parameters(self._h, _vp(p), _vp(x)))

    def set_camera_parameters(self, cam_params):
        """refined intrinsics between iterations: a list of per-camera vectors (as cam_params_list) or the packed
        array, same layout as at creation"""
        flat = np.asarray(cam_params, np.float64) if np.ndim(cam_params[0]) == 0 else np.concatenate(
            [np.asarray(c, np.float64) for c in cam_params])
        flat = np.ascontiguousarray(flat, np.float64)
        assert flat.shape == self.cam_params.shape
        _check(lib().pcd_ba_set_camera_parameters(self._h, _vp(flat)))
        self.cam_params = flat

    def evaluate_blocks(self, want_jacobians=True, want_jac_cam=False):
        """the Ceres route (pcd_ba_evaluate_blocks): raw blocks of every residual block through the handle's pinned
        buffers, copied out before returning.  jac_q / jac_t hold one row per variable-pose observation, pose_row [O]
        uint32 is observation o's row (0xFFFFFFFF: constant pose).  Arrays that were not asked for are None (the C
        pointer is NULL); an array that was asked for and has no rows is empty."""
        bl = BABlocks()
        _check(lib().pcd_ba_evaluate_blocks(self._h, int(bool(want_jacobians)), int(bool(want_jac_cam)), C.byref(bl)))
        V = int(bl.num_pose_rows)

        def take(name, shape, wanted, dtype=np.float64):
            ptr = getattr(bl, name)
            n = int(np.prod(shape))
            if not wanted:
                if ptr:
                    raise PcdError(PCD_ERR_INVALID, f"pcd_ba_evaluate_blocks: {name} not requested but not NULL")
                return None
            if n == 0:
                return np.zeros(shape, dtype)
            if not ptr:
                raise PcdError(PCD_ERR_INVALID, f"pcd_ba_evaluate_blocks: {name} is NULL")
            return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype).reshape(shape).copy()
        wj = bool(want_jacobians)
        out = dict(residuals=take("residuals", (2 * self.O + self.L,), True),
                   jac_q=take("jac_q", (V, 2, 4), wj), jac_t=take("jac_t", (V, 2, 3), wj),
                   jac_X=take("jac_X", (self.O, 2, 3), wj), jac_lidar=take("jac_lidar", (self.L, 3), wj),
                   jac_cam=take("jac_cam", (self.O, 2, CAM_JAC_STRIDE), wj and bool(want_jac_cam)),
                   pose_row=take("pose_row", (self.O,), True, np.uint32),
                   num_pose_rows=V, bytes_d2h=int(bl.bytes_d2h))
        return out

    def evaluate_blocks_compact(self, want_jacobians=True, want_jac_cam=False):
        """the compact Ceres route (pcd_ba_evaluate_blocks_compact), copied out before returning: with Jacobians
        records [O][8] = {r0, r1, M row-major 2x3} (M = dr/dP: jac_t = M, jac_X = M D(q), jac_q = M dPdq(q, X); not zero
        for constant-pose observations), lidar_residuals [L], jac_lidar [L][3], jac_cam [O][2][cam_stride]; without them
        residuals [2 O] and lidar_residuals.  Arrays that were not asked for are None (the C pointer is NULL); an array
        that was asked for and has no rows is empty."""
        bl = BABlocksCompact()
        _check(lib().pcd_ba_evaluate_blocks_compact(self._h, int(bool(want_jacobians)), int(bool(want_jac_cam)),
                                                    C.byref(bl)))
        cs = int(bl.cam_stride)

        def take(name, shape, wanted):
            ptr = getattr(bl, name)
            n = int(np.prod(shape))
            if not wanted:
                if ptr:
                    raise PcdError(PCD_ERR_INVALID, f"pcd_ba_evaluate_blocks_compact: {name} not requested but not NULL")
                return None
            if n == 0:
                return np.zeros(shape)
            if not ptr:
                raise PcdError(PCD_ERR_INVALID, f"pcd_ba_evaluate_blocks_compact: {name} is NULL")
            return np.frombuffer((C.c_char * (n * 8)).from_address(ptr), np.float64).reshape(shape).copy()
        wj = bool(want_jacobians)
        return dict(residuals=take("residuals", (2 * self.O,), not wj), records=take("records", (self.O, 8), wj),
                    lidar_residuals=take("lidar_residuals", (self.L,), True),
                    jac_lidar=take("jac_lidar", (self.L, 3), wj),
                    jac_cam=take("jac_cam", (self.O, 2, cs), wj and bool(want_jac_cam)),
                    cam_stride=cs, bytes_d2h=int(bl.bytes_d2h))

    def evaluate(self, want=("cost", "residuals", "jac_q", "jac_t", "jac_X", "jac_lidar", "H_img", "g_img", "H_pt",
                             "g_pt")):
        shapes = dict(cost=(1,), residuals=(2 * self.O + self.L,), jac_q=(self.O, 2, 4), jac_t=(self.O, 2, 3),
                      jac_X=(self.O, 2, 3), jac_lidar=(self.L, 3), H_img=(self.I, 6, 6), g_img=(self.I, 6),
                      H_pt=(self.P, 3, 3), g_pt=(self.P, 3), W=(self.O, 6, 3), jac_cam=(self.O, 2, CAM_JAC_STRIDE),
                      H_cam=(self.C, CAM_JAC_STRIDE, CAM_JAC_STRIDE), g_cam=(self.C, CAM_JAC_STRIDE),
                      E_cam=(self.I, CAM_JAC_STRIDE, 6), W_cam=(self.O, CAM_JAC_STRIDE, 3))
        out = {k: np.zeros(shapes[k]) for k in want}
        bo = BAOut(*[_vp(out.get(n)) for n, _ in BAOut._fields_])
        _check(lib().pcd_ba_evaluate(self._h, C.byref(bo)))
        return out

    def evaluate_device(self, d_out, stream=0):
        bo = BAOut(*[_ptr(d_out.get(n)) for n, _ in BAOut._fields_])
        _check(lib().pcd_ba_evaluate_device(self._h, C.byref(bo), C.c_void_p(stream)))

    def observation_errors(self):
        """(squared reprojection error, camera-frame depth) per observation: inputs of the post-BA filters"""
        sq = np.empty(self.O)
        depth = np.empty(self.O)
        L = lib()
        L.pcd_ba_observation_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.pcd_ba_observation_errors(self._h, _vp(sq), _vp(depth)))
        return sq, depth

    def filter_tracks(self, max_reproj_error):
        """post-BA filters reduced per track on the device (pcd_ba_filter_tracks): dict of obs_erase [O],
        obs_negative_depth [O], point_delete [P], point_error [P] (-1: no error), num_filtered, mean_reproj_error,
        num_points_with_error, num_negative_depth"""
        class FO(C.Structure):
            _fields_ = [(n, C.c_void_p) for n in ("obs_erase", "obs_negative_depth", "point_delete", "point_error", "summary")]
        out = dict(obs_erase=np.zeros(self.O, np.uint8), obs_negative_depth=np.zeros(self.O, np.uint8),
                   point_delete=np.zeros(self.P, np.uint8), point_error=np.zeros(self.P), summary=np.zeros(4))
        fo = FO(*[_vp(out[k]) for k in ("obs_erase", "obs_negative_depth", "point_delete", "point_error", "summary")])
        L = lib()
        L.pcd_ba_filter_tracks.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        _check(L.pcd_ba_filter_tracks(self._h, float(max_reproj_error), C.byref(fo)))
        sm = out.pop("summary")
        out.update(num_filtered=int(sm[0]), mean_reproj_error=float(sm[1]), num_points_with_error=int(sm[2]),
                   num_negative_depth=int(sm[3]))
        return out

    @staticmethod
    def _filter_opts(max_reproj_error, min_tri_angle):
        o = BAFilterOpts()
        lib().pcd_ba_filter_opts_default(C.byref(o))
        o.max_reproj_error, o.min_tri_angle_deg = float(max_reproj_error), float(min_tri_angle)
        return o

    def filter_points(self, max_reproj_error=8.0, min_tri_angle=1.5):
        """Reconstruction::FilterPoints3D on the device (pcd_ba_filter_points): filter_tracks, then the
        triangulation-angle filter (degrees; <= 0: the first filter alone) on what it left.  The same dict as
        filter_tracks; num_filtered counts elements for the first filter and one per point for the second."""
        out = dict(obs_erase=np.zeros(self.O, np.uint8), obs_negative_depth=np.zeros(self.O, np.uint8),
                   point_delete=np.zeros(self.P, np.uint8), point_error=np.zeros(self.P), summary=np.zeros(4))
        fo = BAFilterOut(*[_vp(out[k]) for k, _ in BAFilterOut._fields_])
        o = self._filter_opts(max_reproj_error, min_tri_angle)
        _check(lib().pcd_ba_filter_points(self._h, C.byref(o), C.byref(fo)))
        sm = out.pop("summary")
        out.update(num_filtered=int(sm[0]), mean_reproj_error=float(sm[1]), num_points_with_error=int(sm[2]),
                   num_negative_depth=int(sm[3]))
        return out

    def filter_points_device(self, max_reproj_error=8.0, min_tri_angle=1.5, out=None):
        """pcd_ba_filter_points_device on the current torch stream: dict of torch device tensors obs_erase [O] uint8,
        obs_negative_depth [O] uint8, point_delete [P] uint8, point_error [P], summary [4] float64 (made here, or the
        tensors of `out` reused; a key of `out` set to None is not computed).  Nothing is synchronised."""
        torch, dev, stream = self._torch()
        if out is None:
            out = dict(obs_erase=torch.empty(self.O, dtype=torch.uint8, device=dev),
                       obs_negative_depth=torch.empty(self.O, dtype=torch.uint8, device=dev),
                       point_delete=torch.empty(self.P, dtype=torch.uint8, device=dev),
                       point_error=torch.empty(self.P, dtype=torch.float64, device=dev),
                       summary=torch.empty(4, dtype=torch.float64, device=dev))
        fo = BAFilterOut(*[_ptr(out.get(k)) for k, _ in BAFilterOut._fields_])
        o = self._filter_opts(max_reproj_error, min_tri_angle)
        _check(lib().pcd_ba_filter_points_device(self._h, C.byref(o), C.byref(fo), C.c_void_p(stream)))
        return out

    def remove_observations(self, obs_erase=None, point_delete=None, want_map=False):
        """pcd_ba_remove_observations_device: drop the observations with obs_erase != 0 and, for every point with
        point_delete != 0, all its observations and LiDAR terms ([O] / [P] uint8, torch device tensors or numpy; None:
        none).  Afterwards the handle equals one created from the compacted arrays; point ids stay, a deleted point's
        coordinates are meaningless.  Synchronises the current stream once.  Returns the info dict (num_obs,
        num_obs_removed, num_lidar, num_lidar_removed, num_points_emptied, rebuild_ms), with want_map also "obs_map": an
        [O before] int32 device tensor, the new index of every old observation, -1 for a dropped one (the C ABI's
        0xFFFFFFFF)."""
        torch, dev, stream = self._torch()
        e, p = self._stage(obs_erase, np.uint8), self._stage(point_delete, np.uint8)
        if e is not None and int(e.numel()) != self.O:
            raise ValueError("remove_observations: obs_erase must have one entry per observation")
        if p is not None and int(p.numel()) != self.P:
            raise ValueError("remove_observations: point_delete must have one entry per point")
        if e is not None and self.O == 0:
            e = None    # an empty tensor has a null data pointer anyway: no observation to erase
        m = None
        if want_map:
            m = torch.arange(self.O, dtype=torch.int32, device=dev)   # the identity: what a call without flags leaves
        info = BARemoveInfo()
        _check(lib().pcd_ba_remove_observations_device(self._h, _ptr(e), _ptr(p), _ptr(m), C.c_void_p(stream),
                                                       C.byref(info)))
        out = {k: getattr(info, k) for k, _ in BARemoveInfo._fields_}
        if e is not None or p is not None:
            self.O, self.L = int(info.num_obs), int(info.num_lidar)
            self.obs_image = self.obs_point = self.obs_xy = None      # stale: the handle has the current rows
            self.lidar_point = self.lidar_abcd = self.lidar_weight = None
            self.__dict__.pop("_schur_dims", None)                    # the co-visibility structure is built anew
        if want_map:
            out["obs_map"] = m
        return out

    def add_observations(self, obs_image, obs_point, obs_xy, new_points=None):
        """pcd_ba_add_observations_device: append new_points ([Pn][3] or None; they get the ids P .. P + Pn - 1) and the
        rows obs_image / obs_point [A] int32, obs_xy [A][2] (numpy or torch device tensors; obs_point may name old and
        new points).  Afterwards the handle equals one created from the concatenated arrays: old observation indices
        stay, the new rows are O .. O + A - 1 in the order given, new points are variable and carry no LiDAR term.
        Arrays with one entry per point that the caller passes later (max_range, select, point_delete, set_parameters)
        must have the new length.  Rows out of range raise PcdError(PCD_ERR_INVALID) and leave the handle untouched.
        Synchronises the current stream once.  Returns the info dict (num_obs, num_obs_added, num_points,
        num_points_added, num_pose_rows, rebuild_ms)."""
        _, _, stream = self._torch()
        oi, op, xy = self._stage(obs_image, np.int32), self._stage(obs_point, np.int32), self._stage(obs_xy, np.float64)
        x = self._stage(new_points, np.float64)
        A = 0 if oi is None else int(oi.numel())
        if (0 if op is None else int(op.numel())) != A or (0 if xy is None else int(xy.numel())) != 2 * A:
            raise ValueError("add_observations: obs_image, obs_point [A] and obs_xy [A][2] must agree")
        Pn = 0 if x is None else int(x.numel())
        if Pn % 3:
            raise ValueError("add_observations: new_points must be [Pn][3]")
        Pn //= 3
        info = BAAddInfo()
        # an empty tensor has a null data pointer: a count of 0 goes with NULL
        _check(lib().pcd_ba_add_observations_device(self._h, _ptr(x) if Pn else None, Pn, _ptr(oi) if A else None,
                                                    _ptr(op) if A else None, _ptr(xy) if A else None, A,
                                                    C.c_void_p(stream), C.byref(info)))
        if A or Pn:
            self.O, self.P = int(info.num_obs), int(info.num_points)
            self.obs_image = self.obs_point = self.obs_xy = None      # stale: the handle has the current rows
            self.points = self.point_const = None
            self.__dict__.pop("_schur_dims", None)                    # the co-visibility structure is built anew
        return {k: getattr(info, k) for k, _ in BAAddInfo._fields_}

    def _window_object(self, h, info, t_in, extra):
        """the BA of a window handle `h` derived from this one: this object's description with the window's counts and
        the host mirror of its pose mask"""
        w = BA.__new__(BA)
        w.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_h", "_schur_dims")})
        w._h = h
        w.O, w.L = int(info.num_obs), int(info.num_lidar)
        w.obs_image = w.obs_point = w.obs_xy = None                # the handle has the rows and the terms
        w.lidar_point = w.lidar_abcd = w.lidar_weight = None
        # the host mirror of the window's pose mask (BA._cam_dims counts the pose slots from it): src's | !in | extra,
        # from O(I) bytes read back behind the call's own synchronisation
        cpose = t_in.cpu().numpy() == 0
        if self.image_const_pose is not None:
            cpose |= self.image_const_pose != 0
        if extra is not None:
            cpose |= extra.cpu().numpy() != 0
        w.image_const_pose = cpose.astype(np.uint8)
        w.__dict__.pop("_ncs", None)
        w.poses = w.points = None                                  # BA.get_parameters() has the current ones
        return w

    def sphere_window(self, center_image=None, radius=40.0, image_set=None, extra_const_pose=None, want=()):
        """pcd_ba_window_create_device: the sphere sub-problem of one global round (AdjustGlobalBundleByLidar) as a NEW
        handle derived on the device; this handle is only read.  The images within `radius` of center_image's projection
        centre are "in" (or those flagged in image_set [I], with center_image None); every other image gets a constant
        pose, as do those flagged in extra_const_pose [I]; the points seen from an "in" image keep all their observations
        and LiDAR terms, the others keep none.  I, P and C are unchanged: indices mean the same in both handles.
        Synchronises the current stream once.  Returns (BA, info): info holds num_images_in, num_points_active, num_obs,
        num_lidar, num_pose_rows, build_ms and, for the names in `want`, the device tensors image_in [I] uint8,
        point_active [P] uint8 and obs_map [O] int32 (row in the window, -1: not in it).  BA.commit_window carries the
        window's parameters back; close the window when done."""
        torch, dev, stream = self._torch()
        o = BAWindowOpts()
        lib().pcd_ba_window_opts_default(C.byref(o))
        o.center_image = -1 if center_image is None else int(center_image)
        o.radius = float(radius)
        iset, extra = self._stage(image_set, np.uint8), self._stage(extra_const_pose, np.uint8)
        for name, t in (("image_set", iset), ("extra_const_pose", extra)):
            if t is not None and int(t.numel()) != self.I:
                raise ValueError(f"sphere_window: {name} must have one entry per image")
        o.d_image_set = None if iset is None else iset.data_ptr()
        o.d_extra_const_pose = None if extra is None else extra.data_ptr()
        bad = set(want) - {"image_in", "point_active", "obs_map"}
        if bad:
            raise ValueError(f"sphere_window: unknown output {sorted(bad)}")
        t_in = torch.empty(self.I, dtype=torch.uint8, device=dev)   # always: the window's host mask mirror needs it
        t_act = torch.empty(self.P, dtype=torch.uint8, device=dev) if "point_active" in want else None
        t_map = torch.empty(self.O, dtype=torch.int32, device=dev) if "obs_map" in want and self.O else None
        h, info = C.c_void_p(), BAWindowInfo()
        _check(lib().pcd_ba_window_create_device(self._h, C.byref(o), _ptr(t_in), _ptr(t_act), _ptr(t_map),
                                                 C.c_void_p(stream), C.byref(h), C.byref(info)))
        w = self._window_object(h, info, t_in, extra)
        out = {k: getattr(info, k) for k, _ in BAWindowInfo._fields_}
        if "image_in" in want:
            out["image_in"] = t_in
        if "point_active" in want:
            out["point_active"] = t_act
        if "obs_map" in want:
            out["obs_map"] = t_map if t_map is not None else torch.empty(0, dtype=torch.int32, device=dev)
        return w, out

    def local_bundle(self, image, num_images=6, min_tri_angle=6.0, want=(), read_back=True):
        """pcd_ba_local_bundle_device: IncrementalMapper::FindLocalBundle for `image` on this handle -- the at most
        num_images - 1 most connected images with a sufficient triangulation angle (pcdhip.h states the selection).  The
        library call does not synchronise; this method then reads the bundle back, which waits for the current stream --
        unless read_back is False: then nothing waits, the first value returned is None and info["num"] is a device
        tensor [1] (the image_set is all BA.local_window needs).  Returns (bundle, info): bundle is the int32 numpy array
        of the selected images in selection order; info holds num, the device tensor image_set [I] uint8 (1 for `image`
        and the bundle) and, for the names in `want`, shared [I] int32, tri_angle [I] float64 (-1: not computed) and
        bundle [num_images - 1] int32 as the device holds it (-1 behind the last)."""
        torch, dev, stream = self._torch()
        bad = set(want) - {"shared", "tri_angle", "bundle"}
        if bad:
            raise ValueError(f"local_bundle: unknown output {sorted(bad)}")
        o = BALocalBundleOpts()
        lib().pcd_ba_local_bundle_opts_default(C.byref(o))
        o.image, o.num_images, o.min_tri_angle_deg = int(image), int(num_images), float(min_tri_angle)
        cap = max(int(num_images) - 1, 1)
        t_bundle = torch.empty(cap, dtype=torch.int32, device=dev)
        t_num = torch.empty(1, dtype=torch.int32, device=dev)
        t_set = torch.empty(self.I, dtype=torch.uint8, device=dev)
        t_shared = torch.empty(self.I, dtype=torch.int32, device=dev) if "shared" in want else None
        t_tri = torch.empty(self.I, dtype=torch.float64, device=dev) if "tri_angle" in want else None
        _check(lib().pcd_ba_local_bundle_device(self._h, C.byref(o), _ptr(t_bundle), _ptr(t_num), _ptr(t_set),
                                                _ptr(t_shared), _ptr(t_tri), C.c_void_p(stream)))
        num = int(t_num.item()) if read_back else t_num
        out = dict(image_set=t_set, num=num)
        for name, t in (("shared", t_shared), ("tri_angle", t_tri), ("bundle", t_bundle)):
            if name in want:
                out[name] = t
        return (t_bundle[:num].cpu().numpy() if read_back else None), out

    def local_window(self, image_set, point_variable=None, image=None, max_track_length=1000, extra_const_pose=None,
                     want=()):
        """pcd_ba_local_window_create_device: the sub-problem of one local round (AdjustLocalBundle) as a NEW handle
        derived on the device; this handle is only read.  image_set [I] flags `image` and its bundle (BA.local_bundle's
        image_set); the variable points are point_variable [P], or, with `image`, those `image` observes with a track of
        at most max_track_length rows.  A row stays if its image is in the set or its point is variable; a point that
        keeps only part of its track becomes constant; a LiDAR term stays if its point is variable; every image outside
        the set gets a constant pose, as do those flagged in extra_const_pose [I].  Synchronises the current stream once.
        Returns (BA, info): info holds num_images_in, num_points_variable, num_points_fixed, num_obs, num_lidar,
        num_pose_rows, build_ms and, for the names in `want`, the device tensors point_variable [P] uint8 and obs_map
        [O] int32 (row in the window, -1: not in it).  BA.commit_window carries the window's parameters back; close
        the window when done."""
        torch, dev, stream = self._torch()
        o = BALocalWindowOpts()
        lib().pcd_ba_local_window_opts_default(C.byref(o))
        iset, extra = self._stage(image_set, np.uint8), self._stage(extra_const_pose, np.uint8)
        var = self._stage(point_variable, np.uint8)
        for name, t, n in (("image_set", iset, self.I), ("extra_const_pose", extra, self.I), ("point_variable", var, self.P)):
            if t is not None and int(t.numel()) != n:
                raise ValueError(f"local_window: {name} has the wrong length")
        o.d_image_set = None if iset is None else iset.data_ptr()
        o.d_extra_const_pose = None if extra is None else extra.data_ptr()
        o.d_point_variable = None if var is None else var.data_ptr()
        o.image = -1 if image is None else int(image)
        o.max_track_length = int(max_track_length)
        bad = set(want) - {"point_variable", "obs_map"}
        if bad:
            raise ValueError(f"local_window: unknown output {sorted(bad)}")
        t_var = torch.empty(self.P, dtype=torch.uint8, device=dev) if "point_variable" in want else None
        t_map = torch.empty(self.O, dtype=torch.int32, device=dev) if "obs_map" in want and self.O else None
        h, info = C.c_void_p(), BALocalWindowInfo()
        _check(lib().pcd_ba_local_window_create_device(self._h, C.byref(o), _ptr(t_var), _ptr(t_map), C.c_void_p(stream),
                                                       C.byref(h), C.byref(info)))
        w = self._window_object(h, info, iset, extra)
        w.point_const = None                                       # the handle has the window's point mask
        out = {k: getattr(info, k) for k, _ in BALocalWindowInfo._fields_}
        if "point_variable" in want:
            out["point_variable"] = t_var
        if "obs_map" in want:
            out["obs_map"] = t_map if t_map is not None else torch.empty(0, dtype=torch.int32, device=dev)
        return w, out

    def commit_window(self, win):
        """pcd_ba_window_commit_device: the window's poses and points (and, when it refines intrinsics, its camera
        parameters) over this handle's, device to device on the current stream.  Exact: the window's constant poses and
        inactive points never moved.  The Schur state of this handle's last call is dropped, its structure stays."""
        _, _, stream = self._torch()
        _check(lib().pcd_ba_window_commit_device(win._h, self._h, C.c_void_p(stream)))
        if win.camera_refine is not None and np.any(win.camera_refine):
            self.cam_params = self.get_camera_parameters()

    def device_parameters(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().pcd_ba_device_parameters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- point elimination on the device (pcd_ba_schur*) ----
    def _torch(self):
        import torch
        dev = torch.device("cuda", self.device)
        return torch, dev, torch.cuda.current_stream(dev).cuda_stream

    def _schur_counts(self):
        """(num_slots, num_pairs) of the co-visibility structure, cached until an edit drops the structure"""
        if not hasattr(self, "_schur_dims"):
            st = self.schur_structure()
            self._schur_dims = (st["num_slots"], st["pairs"].shape[0])
        return self._schur_dims

    def schur_structure(self):
        """co-visibility structure: dict(image_slot [I] int32 (-1 = constant pose), num_slots, pairs [num_pairs][2]
        int32 slot pairs i < j sharing an eliminated point, ascending)"""
        L = lib()
        ns, npair = C.c_int32(0), C.c_uint64(0)
        _check(L.pcd_ba_schur_structure(self._h, None, C.byref(ns), C.byref(npair), None, None))
        slot = np.zeros(self.I, np.int32)
        pi = np.zeros(max(npair.value, 1), np.int32)
        pj = np.zeros(max(npair.value, 1), np.int32)
        _check(L.pcd_ba_schur_structure(self._h, _vp(slot), C.byref(ns), C.byref(npair), _vp(pi), _vp(pj)))
        n = npair.value
        return dict(image_slot=slot, num_slots=ns.value, pairs=np.stack([pi[:n], pj[:n]], axis=1))

    def schur_build(self, stream=None):
        """pcd_ba_schur_build_device: builds the co-visibility structure now, on the device, if the handle has none (a
        fresh handle, or one whose observations remove_observations changed).  stream: a torch stream (None: the current
        one).  Returns dict(build_ms (0: already built), num_slots, num_syncs, num_pairs, num_entries)."""
        cur = self._torch()[2]
        info = BASchurBuildInfo()
        _check(lib().pcd_ba_schur_build_device(self._h, C.c_void_p(cur if stream is None else stream.cuda_stream),
                                               C.byref(info)))
        self._schur_dims = (int(info.num_slots), int(info.num_pairs))
        return {k: getattr(info, k) for k, _ in BASchurBuildInfo._fields_}

    def schur_lists(self):
        """pcd_ba_schur_structure_lists: every list of the co-visibility structure as numpy arrays (slot_image int32, the
        rest uint32; the layout is the header's), with the counts num_slots, num_pairs, num_entries"""
        info = BASchurBuildInfo()
        _check(lib().pcd_ba_schur_build_device(self._h, None, C.byref(info)))
        ns, npair, nent = int(info.num_slots), int(info.num_pairs), int(info.num_entries)
        size = dict(slot_image=ns, obs_pos=self.O, blk_start=ns + npair + 1, ent_a=nent, ent_b=nent, pair_ij=2 * npair,
                    row_start=ns + 1, row_blk=ns + 2 * npair, row_col=ns + 2 * npair)
        out = {k: np.zeros(size[k], np.int32 if k == "slot_image" else np.uint32) for k in _SCHUR_LISTS}
        o = BASchurLists(*[_vp(out[k]) if size[k] else None for k in _SCHUR_LISTS])
        _check(lib().pcd_ba_schur_structure_lists(self._h, C.byref(o)))
        out.update(num_slots=ns, num_pairs=npair, num_entries=nent)
        return out

    def schur_stats(self):
        i = BASchurInfo()
        _check(lib().pcd_ba_schur_stats(self._h, C.byref(i)))
        return dict(build_ms=i.build_ms, num_entries=int(i.num_entries), scratch_bytes=int(i.scratch_bytes))

    def schur(self, mu, damping="marquardt", dense=False, want=("cost", "S_diag", "S_off", "rhs", "num_skipped")):
        """normal equations at the current parameters, points eliminated on the device: dict of torch device
        tensors cost [1], S_diag [ns][6][6], S_off [num_pairs][6][6], rhs [ns][6], num_skipped [1] (int64) and, with
        dense=True, S [6 ns][6 ns]"""
        torch, dev, stream = self._torch()
        ns, npair = self._schur_counts()
        f64 = dict(dtype=torch.float64, device=dev)
        shapes = dict(cost=(1,), S_diag=(ns, 6, 6), S_off=(npair, 6, 6), rhs=(ns, 6), S=(6 * ns, 6 * ns))
        out = {k: torch.empty(shapes[k], **f64) for k in want if k in shapes}
        if "num_skipped" in want:
            out["num_skipped"] = torch.zeros(1, dtype=torch.int64, device=dev)
        if dense:
            out["S"] = torch.empty(shapes["S"], **f64)
        o = BASchurOut(*[_ptr(out.get(n)) for n, _ in BASchurOut._fields_])
        opts = BASchurOpts(float(mu), _DAMPING[damping])
        _check(lib().pcd_ba_schur_device(self._h, C.byref(opts), C.byref(o), C.c_void_p(stream)))
        return out

    def back_substitute(self, dpose, dpoint=None, model_decrease=True):
        """point steps of the last schur() call for the pose step dpose [ns][6] (torch, device): returns
        (dpoint [P][3], model decrease [1] or None)"""
        torch, dev, stream = self._torch()
        dpose = dpose.to(device=dev, dtype=torch.float64).contiguous()
        if dpoint is None:
            dpoint = torch.empty((self.P, 3), dtype=torch.float64, device=dev)
        md = torch.empty(1, dtype=torch.float64, device=dev) if model_decrease else None
        _check(lib().pcd_ba_schur_back_substitute_device(self._h, _ptr(dpose), _ptr(dpoint), _ptr(md), C.c_void_p(stream)))
        return dpoint, md

    def plus(self, dpose, dpoint, poses_out=None, points_out=None):
        """candidate parameters (quaternion manifold Plus, t + dt, X + dX; constants copied) from the handle's current
        ones: returns (poses [I][7], points [P][3]) torch device tensors"""
        torch, dev, stream = self._torch()
        dpose = dpose.to(device=dev, dtype=torch.float64).contiguous()
        dpoint = dpoint.to(device=dev, dtype=torch.float64).contiguous()
        if poses_out is None:
            poses_out = torch.empty((self.I, 7), dtype=torch.float64, device=dev)
        if points_out is None:
            points_out = torch.empty((self.P, 3), dtype=torch.float64, device=dev)
        _check(lib().pcd_ba_plus_device(self._h, _ptr(dpose), _ptr(dpoint), _ptr(poses_out), _ptr(points_out),
                                        C.c_void_p(stream)))
        return poses_out, points_out

    def schur_solve_pcg(self, dpose=None, **opts):
        """block-sparse PCG on the reduced system of the last schur() call (whose S_diag / S_off / rhs must have stayed
        in the handle: want without them).  opts: pcg_opts() arguments.  Returns (dpose [ns][6] torch device tensor,
        info dict: iterations, termination, precond_fallbacks, rhs_norm, residual_norm, q, step_dot_residual)"""
        torch, dev, stream = self._torch()
        ns = self._schur_counts()[0]
        if dpose is None:
            dpose = torch.empty((ns, 6), dtype=torch.float64, device=dev)
        d_info = torch.zeros(C.sizeof(BAPcgInfo), dtype=torch.uint8, device=dev)
        o = pcg_opts(**opts)
        _check(lib().pcd_ba_schur_solve_pcg_device(self._h, C.byref(o), _ptr(dpose), _ptr(d_info), C.c_void_p(stream)))
        return dpose, _device_info(d_info, PCG_INFO_DTYPE)

    def schur_solve_pcg_host(self, **opts):
        """pcd_ba_schur_solve_pcg: the same solve with host outputs (numpy dpose [ns][6], info dict)"""
        ns = self.schur_structure()["num_slots"]
        dpose = np.zeros((ns, 6))
        info = BAPcgInfo()
        o = pcg_opts(**opts)
        _check(lib().pcd_ba_schur_solve_pcg(self._h, C.byref(o), _vp(dpose), C.byref(info)))
        return dpose, _pcg_info(info)

    def schur_solve_cholesky(self, S=None, rhs=None, dpose=None):
        """direct solve of the reduced system (blocked fp64 Cholesky on the device).  Without arguments: the handle's own
        blocks of the last schur() call (whose S_diag / S_off / rhs must have stayed in the handle).  With S [6 ns][6 ns]
        and rhs (torch device tensors, fp64): that system; only the lower triangle of S is read and S is not modified.
        Returns (dpose [ns][6] torch device tensor -- zeros when the factorisation failed --, info dict: status,
        failed_column, n, n_padded, panels, min_pivot, max_pivot)"""
        torch, dev, stream = self._torch()
        ns = self._schur_counts()[0]
        if S is not None:
            S = S.to(device=dev, dtype=torch.float64).contiguous()
            if tuple(S.shape) != (6 * ns, 6 * ns):
                raise ValueError(f"S must be [{6 * ns}][{6 * ns}], got {tuple(S.shape)}")
        if rhs is not None:
            rhs = rhs.to(device=dev, dtype=torch.float64).contiguous()
            if rhs.numel() != 6 * ns:
                raise ValueError(f"rhs must have {6 * ns} entries, got {rhs.numel()}")
        if dpose is None:
            dpose = torch.empty((ns, 6), dtype=torch.float64, device=dev)
        d_info = torch.zeros(C.sizeof(BACholInfo), dtype=torch.uint8, device=dev)
        # an empty tensor (ns = 0) has a null data pointer, which would read as "not given": lend it one element
        one = torch.zeros(1, dtype=torch.float64, device=dev)
        ps = None if S is None else _ptr(S if S.numel() else one)
        pr = None if rhs is None else _ptr(rhs if rhs.numel() else one)
        _check(lib().pcd_ba_schur_solve_cholesky_device(self._h, ps, pr, _ptr(dpose), _ptr(d_info), C.c_void_p(stream)))
        return dpose, _device_info(d_info, CHOL_INFO_DTYPE)

    def schur_solve_cholesky_host(self, S=None, rhs=None):
        """pcd_ba_schur_solve_cholesky, the host form of the C ABI that C and C++ callers use: the same solve with host
        arrays (numpy S, rhs or neither; numpy dpose, info dict).  Here for the tests of that entry point; Python
        callers want schur_solve_cholesky, which keeps everything on the device."""
        ns = self.schur_structure()["num_slots"]
        dpose = np.zeros((ns, 6))
        info = BACholInfo()
        S = None if S is None else np.ascontiguousarray(S, np.float64)
        rhs = None if rhs is None else np.ascontiguousarray(rhs, np.float64)
        _check(lib().pcd_ba_schur_solve_cholesky(self._h, None if S is None else _vp(S), None if rhs is None else _vp(rhs),
                                                 _vp(dpose), C.byref(info)))
        return dpose, {n: getattr(info, n) for n, _ in BACholInfo._fields_}

    # ---- refined intrinsics: camera rows in the reduced system (pcd_ba_schur_cam*) ----
    def camera_slots(self):
        """dict(camera_slot [C] int32 (-1: no refined parameter), num_slots, active [num_slots][12] uint8): the camera
        unknowns of the reduced system, n = 6 ns + 12 num_slots"""
        ncs = C.c_int32(0)
        _check(lib().pcd_ba_camera_slots(self._h, None, C.byref(ncs), None))
        slot = np.zeros(self.C, np.int32)
        active = np.zeros((ncs.value, CAM_JAC_STRIDE), np.uint8)
        _check(lib().pcd_ba_camera_slots(self._h, _vp(slot), C.byref(ncs), _vp(active) if active.size else None))
        return dict(camera_slot=slot, num_slots=ncs.value, active=active)

    def _cam_dims(self):
        """(ns, ncs).  The pose slots are the variable-pose images: counted here, since the structure queries of the
        plain route are refused on a handle with refined intrinsics"""
        if not hasattr(self, "_ncs"):
            self._ncs = self.camera_slots()["num_slots"]
        ns = self.I if self.image_const_pose is None else int(np.count_nonzero(self.image_const_pose == 0))
        return ns, self._ncs

    def schur_cam(self, mu, damping="marquardt", dense=False,
                  want=("cost", "S_diag", "rhs", "B", "S_cam", "rhs_cam", "num_skipped"), num_pairs=None):
        """schur() with the camera rows: dict of torch device tensors cost [1], S_diag [ns][6][6], rhs [ns][6],
        B [ns][ncs][12][6], S_cam [ncs][ncs][12][12], rhs_cam [ncs][12], num_skipped [1] and, with dense=True,
        S [n][n], n = 6 ns + 12 ncs (both triangles).  S_off [num_pairs][6][6] needs the pair count: it is that of the
        same problem without camera_refine (schur_structure() there).  As in schur(), S_diag / S_off / rhs named in want
        leave the handle for caller memory: schur_cam_solve_cholesky reads the handle's own, so keep them out of want
        before it."""
        torch, dev, stream = self._torch()
        ns, ncs = self._cam_dims()
        n = 6 * ns + CAM_JAC_STRIDE * ncs
        f64 = dict(dtype=torch.float64, device=dev)
        shapes = dict(cost=(1,), S_diag=(ns, 6, 6), rhs=(ns, 6), B=(ns, ncs, CAM_JAC_STRIDE, 6),
                      S_cam=(ncs, ncs, CAM_JAC_STRIDE, CAM_JAC_STRIDE), rhs_cam=(ncs, CAM_JAC_STRIDE), S=(n, n))
        if "S_off" in want:
            if num_pairs is None:
                raise ValueError("S_off needs num_pairs")
            shapes["S_off"] = (int(num_pairs), 6, 6)
        out = {k: torch.zeros(shapes[k], **f64) for k in want if k in shapes and k != "S"}
        if "num_skipped" in want:
            out["num_skipped"] = torch.zeros(1, dtype=torch.int64, device=dev)
        if dense:
            out["S"] = torch.zeros(shapes["S"], **f64)
        # an empty tensor has a null data pointer, which reads as "not asked for": nothing would be written anyway
        o = BASchurCamOut(*[_ptr(out[k]) if k in out and out[k].numel() else None for k, _ in BASchurCamOut._fields_])
        opts = BASchurOpts(float(mu), _DAMPING[damping])
        _check(lib().pcd_ba_schur_cam_device(self._h, C.byref(opts), C.byref(o), C.c_void_p(stream)))
        return out

    def schur_cam_solve_cholesky(self, delta=None):
        """direct solve of the bordered system of the last schur_cam() call from the handle's own blocks: (delta [n] torch
        device tensor = dpose [ns][6] then dcam [ncs][12], zeros when the factorisation failed; info dict as
        schur_solve_cholesky)"""
        torch, dev, stream = self._torch()
        ns, ncs = self._cam_dims()
        n = 6 * ns + CAM_JAC_STRIDE * ncs
        if delta is None:
            delta = torch.empty(n, dtype=torch.float64, device=dev)
        d_info = torch.zeros(C.sizeof(BACholInfo), dtype=torch.uint8, device=dev)
        pad = torch.zeros(1, dtype=torch.float64, device=dev)   # n = 0: an empty tensor's pointer is null
        _check(lib().pcd_ba_schur_cam_solve_cholesky_device(self._h, _ptr(delta if n else pad), _ptr(d_info),
                                                            C.c_void_p(stream)))
        return delta, _device_info(d_info, CHOL_INFO_DTYPE)

    def schur_cam_solve_pcg(self, delta=None, **opts):
        """bordered PCG on the system of the last schur_cam() call from the handle's own blocks (keep S_diag / S_off / rhs
        out of want before it).  opts: pcg_opts() arguments.  Returns (delta [n] torch device tensor = dpose [ns][6] then
        dcam [ncs][12], info dict as schur_solve_pcg).  Without camera slots it is schur_solve_pcg."""
        torch, dev, stream = self._torch()
        ns, ncs = self._cam_dims()
        n = 6 * ns + CAM_JAC_STRIDE * ncs
        if delta is None:
            delta = torch.empty(n, dtype=torch.float64, device=dev)
        d_info = torch.zeros(C.sizeof(BAPcgInfo), dtype=torch.uint8, device=dev)
        pad = torch.zeros(1, dtype=torch.float64, device=dev)   # n = 0: an empty tensor's pointer is null
        o = pcg_opts(**opts)
        _check(lib().pcd_ba_schur_cam_solve_pcg_device(self._h, C.byref(o), _ptr(delta if n else pad), _ptr(d_info),
                                                       C.c_void_p(stream)))
        return delta, _device_info(d_info, PCG_INFO_DTYPE)

    def schur_cam_solve_pcg_host(self, **opts):
        """pcd_ba_schur_cam_solve_pcg: the same solve with host outputs (numpy delta [n], info dict)"""
        ns, ncs = self._cam_dims()
        delta = np.zeros(max(1, 6 * ns + CAM_JAC_STRIDE * ncs))
        info = BAPcgInfo()
        o = pcg_opts(**opts)
        _check(lib().pcd_ba_schur_cam_solve_pcg(self._h, C.byref(o), _vp(delta), C.byref(info)))
        return delta[:6 * ns + CAM_JAC_STRIDE * ncs], _pcg_info(info)

    def back_substitute_cam(self, delta, dpoint=None, model_decrease=True):
        """point steps of the last schur_cam() call for delta [n] (dpose then dcam; torch, device): returns
        (dpoint [P][3], model decrease [1] or None)"""
        torch, dev, stream = self._torch()
        delta = delta.to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
        pad = torch.zeros(1, dtype=torch.float64, device=dev)
        if dpoint is None:
            dpoint = torch.empty((self.P, 3), dtype=torch.float64, device=dev)
        md = torch.empty(1, dtype=torch.float64, device=dev) if model_decrease else None
        _check(lib().pcd_ba_schur_cam_back_substitute_device(self._h, _ptr(delta if delta.numel() else pad), _ptr(dpoint),
                                                             _ptr(md), C.c_void_p(stream)))
        return dpoint, md

    def plus_cam(self, delta, dpoint):
        """candidate parameters from the handle's current ones: plus() on poses and points, p + dcam on the active camera
        parameters (everything constant copied bit for bit).  Returns (poses [I][7], points [P][3], cam_params
        [cam_params_len]) torch device tensors"""
        torch, dev, stream = self._torch()
        delta = delta.to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
        dpoint = dpoint.to(device=dev, dtype=torch.float64).contiguous()
        pad = torch.zeros(1, dtype=torch.float64, device=dev)
        poses = torch.empty((self.I, 7), dtype=torch.float64, device=dev)
        points = torch.empty((self.P, 3), dtype=torch.float64, device=dev)
        cams = torch.empty(len(self.cam_params), dtype=torch.float64, device=dev)
        _check(lib().pcd_ba_plus_cam_device(self._h, _ptr(delta if delta.numel() else pad), _ptr(dpoint), _ptr(poses),
                                            _ptr(points), _ptr(cams), C.c_void_p(stream)))
        return poses, points, cams

    def get_camera_parameters(self):
        """the handle's current camera parameters, device -> host: packed numpy [cam_params_len]"""
        out = np.empty(len(self.cam_params))
        _check(lib().pcd_ba_get_camera_parameters(self._h, _vp(out)))
        return out

    def get_parameters(self):
        """the handle's current parameters, device -> host: (poses [I][7], points [P][3]) numpy"""
        poses, points = np.empty((self.I, 7)), np.empty((self.P, 3))
        _check(lib().pcd_ba_get_parameters(self._h, _vp(poses), _vp(points)))
        return poses, points

    def set_parameters_device(self, poses=None, points=None):
        """device -> device parameter update from torch tensors (None keeps the old values)"""
        _, _, stream = self._torch()
        _check(lib().pcd_ba_set_parameters_device(self._h, _ptr(poses), _ptr(points), C.c_void_p(stream)))

    def cost_device(self, out=None):
        """cost at the current parameters (the residual-only pass) into a torch device tensor [1]"""
        torch, dev, stream = self._torch()
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=dev)
        self.evaluate_device({"cost": out}, stream=stream)
        return out

    # ---- LiDAR terms rebuilt on the device (pcd_ba_set_lidar_device / pcd_ba_associate_lidar_device) ----
    def _stage(self, x, dtype):
        """numpy (or anything array-like) -> contiguous torch device tensor on the handle's device; torch tensors are
        converted in place of a copy when they already fit; None stays None"""
        if x is None:
            return None
        torch, dev, _ = self._torch()
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype))
        return x.to(device=dev, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()

    def _terms_changed(self, n):
        self.L = int(n)
        self.lidar_point = self.lidar_abcd = self.lidar_weight = None   # stale: BA.get_lidar() has the current terms

    def set_lidar_device(self, type, abcd, weight, point=None, lidar_xyz=None):
        """pcd_ba_set_lidar_device: replace ALL LiDAR terms by those of the rows (type [Q] uint8, abcd [Q][4], point [Q]
        int32 or None: row q is point q, lidar_xyz [Q][3] or None; numpy or torch).  A row becomes a term iff its type is
        not 0 and its abcd holds no NaN; its weight is weight[type] (a sequence of 4: -, Icp, IcpGround, Proj).  Host
        arrays are staged to the device through torch.  Synchronises the current stream once.  Returns the number of
        terms; afterwards the handle equals one created with that term list."""
        _, _, stream = self._torch()
        t, a = self._stage(type, np.uint8), self._stage(abcd, np.float64)
        p, x = self._stage(point, np.int32), self._stage(lidar_xyz, np.float64)
        Q = int(t.numel())
        if int(a.numel()) != 4 * Q or (p is not None and int(p.numel()) != Q) or (x is not None and int(x.numel()) != 3 * Q):
            raise ValueError("set_lidar_device: type [Q], abcd [Q][4], point [Q], lidar_xyz [Q][3] disagree on Q")
        w = np.ascontiguousarray(weight, np.float64)
        if w.shape != (4,):
            raise ValueError("set_lidar_device: weight must have 4 entries (by type: -, Icp, IcpGround, Proj)")
        n = C.c_uint64(0)
        if p is not None and Q == 0:
            # an empty tensor has a null data pointer, which would read as "no point array": lend it one element
            p = self._stage(np.zeros(1, np.int32), np.int32)
        _check(lib().pcd_ba_set_lidar_device(self._h, Q, _ptr(p), _ptr(t), _ptr(a), _ptr(x), _vp(w), C.c_void_p(stream),
                                             C.byref(n)))
        self._terms_changed(n.value)
        return int(n.value)

    def get_lidar(self):
        """pcd_ba_get_lidar: host copies of the current terms, dict of point [L] int32, abcd [L][4], weight [L], type [L]
        uint8, lidar_xyz [L][3] (type and lidar_xyz are zero for terms that came from the constructor)"""
        n = C.c_uint64(0)
        _check(lib().pcd_ba_get_lidar(self._h, C.byref(n), None, None, None, None, None))
        L = int(n.value)
        out = dict(point=np.zeros(L, np.int32), abcd=np.zeros((L, 4)), weight=np.zeros(L), type=np.zeros(L, np.uint8),
                   lidar_xyz=np.zeros((L, 3)))
        _check(lib().pcd_ba_get_lidar(self._h, C.byref(n), _vp(out["point"]), _vp(out["abcd"]), _vp(out["weight"]),
                                      _vp(out["type"]), _vp(out["lidar_xyz"])))
        return out

    def lidar_device(self):
        """pcd_ba_lidar_device: (L, dict of raw device pointers point / abcd / weight / type / lidar_xyz), valid until the
        terms change"""
        n = C.c_uint64(0)
        ptrs = [C.c_void_p() for _ in range(5)]
        _check(lib().pcd_ba_lidar_device(self._h, C.byref(n), *[C.byref(p) for p in ptrs]))
        return int(n.value), dict(zip(("point", "abcd", "weight", "type", "lidar_xyz"), [p.value for p in ptrs]))

    def associate_lidar(self, cloud, max_range=None, gate_mode=GATE_MAPPER_GLOBAL, select=None, icp_weight=100.0,
                        icp_ground_weight=1000.0):
        """pcd_ba_associate_lidar_device: associate the handle's CURRENT points against `cloud` and install the accepted
        associations as the handle's LiDAR terms (one per point at most, ascending point).  max_range: one value or one
        per point (ignored for GATE_CONTROLLER); select: [P] mask of the points that are queries (None: all), applied
        after a full association.  Returns the info dict (num_queries, num_terms, num_icp, num_icp_ground, assoc_ms,
        rebuild_ms)."""
        _, _, stream = self._torch()
        o = BAAssocOpts()
        lib().pcd_ba_assoc_opts_default(C.byref(o))
        o.gate_mode = int(gate_mode)
        mr = None
        if (int(gate_mode) & 0xFF) != GATE_CONTROLLER:
            mr = self._stage(np.atleast_1d(np.asarray(max_range, np.float64)) if not hasattr(max_range, "data_ptr")
                             else max_range, np.float64)
            o.d_max_range, o.max_range_count = mr.data_ptr(), int(mr.numel())
        sel = self._stage(select, np.uint8)
        if sel is not None:
            if int(sel.numel()) != self.P:
                raise ValueError("associate_lidar: select must have one entry per point")
            o.d_select = sel.data_ptr()
        o.icp_weight, o.icp_ground_weight = float(icp_weight), float(icp_ground_weight)
        info = BAAssocInfo()
        _check(lib().pcd_ba_associate_lidar_device(self._h, cloud._h, C.byref(o), C.c_void_p(stream), C.byref(info)))
        self._terms_changed(info.num_terms)
        return {k: getattr(info, k) for k, _ in BAAssocInfo._fields_}

    def project_lidar(self, projector, cam_size, image_select=None, point_mode=None, max_range=None,
                      gate_mode=GATE_MAPPER_LOCAL, proj_weight=1.0, icp_weight=100.0, icp_ground_weight=1000.0):
        """pcd_ba_project_lidar_device: project the handle's images at their CURRENT poses with `projector`, pick per
        point among the candidates of its track (MatchVariablePoint2LidarPoint), associate the points of mode 2 against
        the projector's cloud, and install the terms (one per point at most, ascending point).  cam_size: one
        (width, height) or one per camera; image_select: [I] mask (None: all); point_mode: [P] of 0 no term / 1 Proj / 2
        nearest neighbour (None: every point Proj, no association); max_range / gate_mode: for mode-2 points, as
        associate_lidar.  Returns the info dict (num_images, num_features, num_found, num_terms, num_proj, num_icp,
        num_icp_ground, pairs, proj_ms, assoc_ms, rebuild_ms)."""
        _, _, stream = self._torch()
        o = BAProjOpts()
        lib().pcd_ba_proj_opts_default(C.byref(o))
        wh = None
        if cam_size is not None:
            wh = np.ascontiguousarray(cam_size, np.uint64).reshape(-1, 2)
            if wh.shape[0] == 1 and self.C > 1:
                wh = np.repeat(wh, self.C, axis=0)
            if wh.shape[0] != self.C:
                raise ValueError("project_lidar: cam_size must be one (width, height) or one per camera")
            w, h = np.ascontiguousarray(wh[:, 0]), np.ascontiguousarray(wh[:, 1])
            o.cam_width, o.cam_height = w.ctypes.data, h.ctypes.data
        o.gate_mode = int(gate_mode)
        sel = self._stage(image_select, np.uint8)
        if sel is not None:
            if int(sel.numel()) != self.I:
                raise ValueError("project_lidar: image_select must have one entry per image")
            o.d_image_select = sel.data_ptr()
        pm = self._stage(point_mode, np.uint8)
        mr = None
        if pm is not None:
            if int(pm.numel()) != self.P:
                raise ValueError("project_lidar: point_mode must have one entry per point")
            o.d_point_mode = pm.data_ptr()
            if (int(gate_mode) & 0xFF) != GATE_CONTROLLER and max_range is not None:
                mr = self._stage(np.atleast_1d(np.asarray(max_range, np.float64)) if not hasattr(max_range, "data_ptr")
                                 else max_range, np.float64)
                o.d_max_range, o.max_range_count = mr.data_ptr(), int(mr.numel())
        o.proj_weight, o.icp_weight, o.icp_ground_weight = float(proj_weight), float(icp_weight), float(icp_ground_weight)
        info = BAProjInfo()
        _check(lib().pcd_ba_project_lidar_device(self._h, projector._h, C.byref(o), C.c_void_p(stream), C.byref(info)))
        self._terms_changed(info.num_terms)
        return {k: getattr(info, k) for k, _ in BAProjInfo._fields_}


def pcg_opts(max_iterations=None, min_iterations=None, preconditioner=None, q_tolerance=None, r_tolerance=None):
    """pcd_ba_pcg_opts at the library's defaults (100, 0, schur_jacobi, 0.1, -1) with the given fields replaced"""
    o = BAPcgOpts()
    lib().pcd_ba_pcg_opts_default(C.byref(o))
    if max_iterations is not None:
        o.max_iterations = int(max_iterations)
    if min_iterations is not None:
        o.min_iterations = int(min_iterations)
    if preconditioner is not None:
        o.preconditioner = _PRECOND[preconditioner] if isinstance(preconditioner, str) else int(preconditioner)
    if q_tolerance is not None:
        o.q_tolerance = float(q_tolerance)
    if r_tolerance is not None:
        o.r_tolerance = float(r_tolerance)
    return o


def _device_info(d_info, dtype):
    """a device info record (uint8 tensor; PCG_INFO_DTYPE or CHOL_INFO_DTYPE) as a dict of Python numbers"""
    i = d_info.cpu().numpy().view(dtype)[0]
    return {k: (float(i[k]) if dtype[k] == np.float64 else int(i[k])) for k in dtype.names if k != "pad"}


def _pcg_info(i):
    return dict(iterations=int(i.iterations), termination=int(i.termination),
                precond_fallbacks=int(i.precond_fallbacks), rhs_norm=float(i.rhs_norm),
                residual_norm=float(i.residual_norm), q=float(i.q), step_dot_residual=float(i.step_dot_residual))


def ba_solve(ba, max_num_iterations=None, damping=None, initial_radius=None, max_radius=None, min_radius=None,
             min_relative_decrease=None, function_tolerance=None, gradient_tolerance=None, linear=None,
             linear_solver="pcg", refine_intrinsics=False):
    """pcd_ba_solve: the LM loop in the library (Schur, PCG, back-substitution, cost pass; no torch).  Options left
    None keep pcd_ba_solve_opts_default; linear is a dict of pcg_opts() arguments.  linear_solver="cholesky" takes the
    exact step of the library's blocked Cholesky instead of the PCG's inexact one (linear_iterations is then 0 and
    linear_termination a CHOL_* status).  Returns (summary dict, list of one dict per iteration); the handle holds
    the accepted parameters (BA.get_parameters()).  refine_intrinsics=True solves for the refined camera parameters
    too (camera rows in the reduced system; linear_solver="cholesky" or "pcg_cam", the bordered PCG) and leaves the
    accepted ones in the handle (BA.get_camera_parameters()); without it a handle with camera_refine is refused."""
    L = lib()
    o = BASolveOpts()
    L.pcd_ba_solve_opts_default(C.byref(o))
    if max_num_iterations is not None:
        o.max_num_iterations = int(max_num_iterations)
    if damping is not None:
        o.damping = _DAMPING[damping]
    for name, v in (("initial_radius", initial_radius), ("max_radius", max_radius), ("min_radius", min_radius),
                    ("min_relative_decrease", min_relative_decrease), ("function_tolerance", function_tolerance),
                    ("gradient_tolerance", gradient_tolerance)):
        if v is not None:
            setattr(o, name, float(v))
    o.linear_solver = _LINEAR[linear_solver] if isinstance(linear_solver, str) else int(linear_solver)
    o.refine_intrinsics = int(bool(refine_intrinsics))
    if linear is not None:
        o.linear = linear if isinstance(linear, BAPcgOpts) else pcg_opts(**linear)
    its = (BASolveIteration * max(o.max_num_iterations, 1))()
    sm = BASolveSummary()
    _check(L.pcd_ba_solve(ba._h, C.byref(o), C.byref(sm), C.cast(its, C.c_void_p)))
    summary = {n: getattr(sm, n) for n, _ in BASolveSummary._fields_}
    hist = []
    for k in range(sm.num_iterations):
        r = {n: getattr(its[k], n) for n, _ in BASolveIteration._fields_}
        r["accepted"] = bool(r["accepted"])
        r["rho"] = r["relative_decrease"]
        hist.append(r)
    return summary, hist


def register_refine(ba, cloud, rounds, kd_max=1.5, kd_min=0.2, drop=0.1, gate_mode=GATE_MAPPER_GLOBAL, select=None,
                    projector=None, cam_size=None, point_mode=None, image_select=None, proj_weight=1.0, **solve_opts):
    """The association / solve half of IncrementalMapper::AdjustGlobalBundleByLidar (sfm/incremental_mapper.cc:1413-1478)
    on whatever the handle holds, without the sphere selection of :1347-1408 (global_round is the whole function),
    GlobalOptNum advancing once per round: in round r every selected point searches within search_range_schedule(r)
    (kd_max, kd_min, drop), BA.associate_lidar installs the accepted associations, ba_solve(**solve_opts) refines.
    Nothing goes through the host and nothing that depends on the observations alone is rebuilt; no device work of its
    own.  Returns one (association info, solve summary, iterations) per round.
    With a `projector` (over `cloud`; cam_size as BA.project_lidar) a round is the mapper's LOCAL one: "project +
    associate + solve" through BA.project_lidar -- the points of point_mode 1 take a depth-projection term from the images
    of image_select, those of mode 2 the nearest-neighbour association within the round's range (point_mode None: every
    point Proj); `select` is not used then (mode 0 is "not a query")."""
    out = []
    for r in range(int(rounds)):
        rng = float(search_range_schedule(np.array([r], np.int32), kd_max, kd_min, drop)[0])
        if projector is not None:
            info = ba.project_lidar(projector, cam_size, image_select=image_select, point_mode=point_mode, max_range=rng,
                                    gate_mode=gate_mode, proj_weight=proj_weight)
        else:
            info = ba.associate_lidar(cloud, max_range=rng, gate_mode=gate_mode, select=select)
        info["max_range"] = rng
        summary, its = ba_solve(ba, **solve_opts)
        out.append((info, summary, its))
    return out


def global_round(ba, cloud, center_image, radius, opt_num, kd_max=1.5, kd_min=0.2, drop=0.1, extra_const_pose=None,
                 **solve_opts):
    """One call of IncrementalMapper::AdjustGlobalBundleByLidar (sfm/incremental_mapper.cc:1297-1493) on the device:
    BA.sphere_window(center_image, radius, extra_const_pose) derives the sphere sub-problem, the window's active points
    search `cloud` within search_range_schedule(opt_num) per point (:1423-1427) and BA.associate_lidar installs the
    accepted associations on the window, ba_solve(**solve_opts) refines it, BA.commit_window carries the parameters back
    into `ba`, and opt_num [P] (int32 numpy or torch device tensor, updated in place: GlobalOptNum, :1483-1487) advances
    for the active points.  `ba` keeps its rows, terms and co-visibility structure.  Returns (window info, association
    info, solve summary, iterations)."""
    torch, dev, _ = ba._torch()
    win, winfo = ba.sphere_window(center_image, radius, extra_const_pose=extra_const_pose, want=("point_active",))
    try:
        active = winfo.pop("point_active")
        host_num = opt_num.cpu().numpy() if isinstance(opt_num, torch.Tensor) else np.asarray(opt_num)
        rng = search_range_schedule(np.ascontiguousarray(host_num, np.int32), kd_max, kd_min, drop)
        ainfo = win.associate_lidar(cloud, max_range=rng, gate_mode=GATE_MAPPER_GLOBAL, select=active)
        summary, its = ba_solve(win, **solve_opts)
        ba.commit_window(win)
    finally:
        win.close()
    if isinstance(opt_num, torch.Tensor):
        opt_num += active.to(opt_num.dtype)
    else:
        opt_num += active.cpu().numpy().astype(opt_num.dtype)
    return winfo, ainfo, summary, its


def local_round(ba, cloud, image, projector=None, cam_size=None, num_images=6, min_tri_angle=6.0, point_variable=None,
                max_track_length=1000, extra_const_pose=None, opt_num=None, kd_max=1.5, kd_min=0.2, drop=0.1,
                image_select=None, point_mode=None, proj_weight=1.0, **solve_opts):
    """One call of IncrementalMapper::AdjustLocalBundle (sfm/incremental_mapper.cc:1004-1213) on the device:
    BA.local_bundle(image, num_images, min_tri_angle) picks the bundle, BA.local_window derives the sub-problem (the
    variable points: point_variable [P], or those `image` observes with at most max_track_length rows), the window takes
    its LiDAR terms -- with a `projector` (over `cloud`; cam_size, image_select, point_mode, proj_weight as
    BA.project_lidar, the range of mode-2 points from opt_num) through BA.project_lidar, else the variable points search
    `cloud` within search_range_schedule(opt_num) per point (:1159-1164; opt_num None: zeros) through BA.associate_lidar --
    ba_solve(**solve_opts) refines it and BA.commit_window carries the parameters back into `ba`.  `ba` keeps its rows,
    terms and co-visibility structure; the camera-constness rule (:1064-1080) stays with the caller.  Returns (bundle,
    window info, term info, solve summary, iterations)."""
    torch, dev, _ = ba._torch()
    bundle, binfo = ba.local_bundle(image, num_images, min_tri_angle)
    win, winfo = ba.local_window(binfo["image_set"], point_variable=point_variable,
                                 image=None if point_variable is not None else image,
                                 max_track_length=max_track_length, extra_const_pose=extra_const_pose,
                                 want=("point_variable",))
    try:
        variable = winfo.pop("point_variable")
        if opt_num is None:
            host_num = np.zeros(ba.P, np.int32)
        else:
            host_num = opt_num.cpu().numpy() if isinstance(opt_num, torch.Tensor) else np.asarray(opt_num)
        rng = search_range_schedule(np.ascontiguousarray(host_num, np.int32), kd_max, kd_min, drop)
        if projector is not None:
            tinfo = win.project_lidar(projector, cam_size, image_select=image_select, point_mode=point_mode, max_range=rng,
                                      gate_mode=GATE_MAPPER_LOCAL, proj_weight=proj_weight)
        else:
            tinfo = win.associate_lidar(cloud, max_range=rng, gate_mode=GATE_MAPPER_LOCAL, select=variable)
        summary, its = ba_solve(win, **solve_opts)
        ba.commit_window(win)
    finally:
        win.close()
    return bundle, winfo, tinfo, summary, its


def refine_filter(ba, max_refinements=5, max_change=0.0005, max_reproj_error=8.0, min_tri_angle=1.5, complete=None,
                  **solve_opts):
    """The loop of IncrementalMapperController's IterativeGlobalRefinement (controllers/incremental_mapper.cc:150-199) on
    one handle: ba_solve(**solve_opts), BA.filter_points_device, BA.remove_observations with the filter's flags, until a
    round changes less than max_change of the observations it started with (changed = num_filtered / observations before
    the round's removal; a handle without observations counts as unchanged) or max_refinements rounds have run.  No
    observation payload crosses PCIe; per round the host reads the filter's 4-double summary and the removal's counts.
    CompleteAndMergeTracks and retriangulation add observations: finding them is the host's business.  complete, if
    given, is called as complete(ba, round) between the solve and the filter (the place of CompleteAndMergeTracks at
    :178) and returns None or a dict(obs_image, obs_point, obs_xy, new_points) that goes in through
    BA.add_observations; the rows it adds count in `changed` with the filtered ones, as in the reference's
    num_changed_observations, and the round's tuple gains the add info as a fourth entry.  Without complete the
    function behaves as before: `changed` counts the filtered observations alone.  Returns one (solve summary, filter
    summary, remove info) per round; the filter summary is a dict of num_filtered, mean_reproj_error,
    num_points_with_error, num_negative_depth, changed."""
    out = []
    for r in range(int(max_refinements)):
        num_obs = ba.O
        summary, _its = ba_solve(ba, **solve_opts)
        added = None
        if complete is not None:
            rows = complete(ba, r)
            if rows is not None:
                added = ba.add_observations(rows["obs_image"], rows["obs_point"], rows["obs_xy"], rows.get("new_points"))
        f = ba.filter_points_device(max_reproj_error, min_tri_angle)
        info = ba.remove_observations(f["obs_erase"], f["point_delete"])
        sm = f["summary"].cpu().numpy()
        num_changed = float(sm[0]) + (added["num_obs_added"] if added else 0)
        changed = num_changed / num_obs if num_obs else 0.0
        fl = dict(num_filtered=int(sm[0]), mean_reproj_error=float(sm[1]), num_points_with_error=int(sm[2]),
                  num_negative_depth=int(sm[3]), changed=changed)
        out.append((summary, fl, info) if complete is None else (summary, fl, info, added))
        if changed < max_change:
            break
    return out


def ba_solve_lm(ba, max_iterations=10, initial_radius=1e4, damping="marquardt", min_relative_decrease=1e-3,
                max_radius=1e16, linear_solver="cholesky", pcg=None):
    """Device-resident Levenberg-Marquardt on a BA handle.  Each iteration: ba.schur (points eliminated on the
    device), torch.linalg.cholesky of the dense reduced camera system (a failed factorisation counts as a rejected
    step), back-substitution and plus into candidate buffers, the cost pass at the candidate, then Ceres' trust-region
    rule: accept if rho = (cost - candidate cost) / model decrease > min_relative_decrease; on success
    radius /= max(1/3, 1 - (2 rho - 1)^3) and the decrease factor resets to 2, on failure radius /= decrease factor
    and the factor doubles.  mu = 1 / radius.

    There is no Jacobi scaling of the columns (Ceres scales them by default), so the iterates are not Ceres' own
    iterate for iterate; the step, model and radius rules are.  On return the handle holds the accepted parameters.
    Returns a list with one dict per iteration: cost (before the step), candidate_cost, rho, accepted, radius (after
    the update), num_skipped.

    linear_solver="pcg" replaces the dense factorisation with BA.schur_solve_pcg on the block-sparse system (the dense
    S is not asked for); pcg is a dict of pcg_opts() arguments.  A BREAKDOWN counts as a rejected step.  Each record
    then also has linear_iterations and linear_termination.

    linear_solver="cholesky_hip" keeps the dense route and hands S and rhs to BA.schur_solve_cholesky (the library's
    blocked Cholesky) in place of torch's factorisation; linear_termination is then a CHOL_* status."""
    import torch
    if linear_solver not in ("cholesky", "pcg", "cholesky_hip"):
        raise ValueError(f"linear_solver {linear_solver!r}: 'cholesky', 'cholesky_hip' or 'pcg'")
    use_pcg = linear_solver == "pcg"
    use_hip = linear_solver == "cholesky_hip"
    dev = torch.device("cuda", ba.device)
    ns = ba.schur_structure()["num_slots"]
    zero_pose = torch.zeros((ns, 6), dtype=torch.float64, device=dev)
    zero_pt = torch.zeros((ba.P, 3), dtype=torch.float64, device=dev)
    acc_poses, acc_points = ba.plus(zero_pose, zero_pt)   # copy of the current parameters
    cand_poses, cand_points = torch.empty_like(acc_poses), torch.empty_like(acc_points)
    radius, decrease_factor = float(initial_radius), 2.0
    history = []
    for _ in range(int(max_iterations)):
        if use_pcg:
            out = ba.schur(1.0 / radius, damping=damping, want=("cost", "num_skipped"))
        else:
            out = ba.schur(1.0 / radius, damping=damping, dense=True, want=("cost", "rhs", "num_skipped"))
        cost = float(out["cost"].item())
        rec = dict(cost=cost, candidate_cost=float("nan"), rho=float("nan"), accepted=False,
                   num_skipped=int(out["num_skipped"].item()))
        factored = True
        if use_pcg:
            dpose_pcg, info = ba.schur_solve_pcg(**(pcg or {}))
            rec.update(linear_iterations=info["iterations"], linear_termination=info["termination"])
            factored = info["termination"] != PCG_BREAKDOWN
        elif use_hip:
            dpose_pcg, info = ba.schur_solve_cholesky(out["S"], out["rhs"])
            rec.update(linear_iterations=0, linear_termination=info["status"])
            factored = info["status"] == CHOL_OK
        elif ns:
            Lc, info = torch.linalg.cholesky_ex(out["S"])
            factored = int(info.item()) == 0
        if factored:   # ns = 0 (every pose constant): no reduced system, only the points move
            if use_pcg or use_hip:
                dpose = dpose_pcg
            else:
                dpose = torch.cholesky_solve(out["rhs"].reshape(-1, 1), Lc).reshape(-1, 6) if ns else zero_pose
            dpoint, md = ba.back_substitute(dpose)
            ba.plus(dpose, dpoint, cand_poses, cand_points)
            ba.set_parameters_device(cand_poses, cand_points)
            new_cost = float(ba.cost_device().item())
            model = float(md.item())
            rho = (cost - new_cost) / model if model > 0 else float("-inf")
            rec.update(candidate_cost=new_cost, rho=rho, accepted=bool(rho > min_relative_decrease))
        if rec["accepted"]:
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rec["rho"] - 1.0) ** 3))
            decrease_factor = 2.0
            acc_poses, cand_poses = cand_poses, acc_poses
            acc_points, cand_points = cand_points, acc_points
        else:
            ba.set_parameters_device(acc_poses, acc_points)
            radius /= decrease_factor
            decrease_factor *= 2.0
        rec["radius"] = radius
        history.append(rec)
    torch.cuda.synchronize(dev)
    return history
