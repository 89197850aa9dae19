"""The C ABI as ctypes sees it: the structures of ``include/flimo_c.h`` / ``flimo_dev.h`` / ``flimo_localizer_c.h`` and ONE row
per exported function.  ``_lib.load_hip()`` and ``api.load_host()`` declare their library from the rows (``declare``); the lists of
symbols the tests compare with the headers are read off them.

A new entry that both a ``flimo_ctx`` and a ``flimo_loc`` offer is one row of ``PAIRED`` -- the two symbols and the arguments after
the handle -- and one method of ``_lib._SharedEntries``; ``HipCtx`` and ``Localizer`` then both have it.  ``PAIRED_NDT`` and
``PAIRED_GICP`` hold the rows of the NDT and the GICP entries in the same form, ``PAIRED_SC`` those of Scan Context,
``PAIRED_SEG`` those of the map segments."""
from __future__ import annotations

import ctypes as C
import numpy as np

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

CHAIN_MAX_PASSES = 12


class MapCfg(C.Structure):
    _fields_ = [("min_extent", C.c_float), ("bucket_size", C.c_int), ("downsample", C.c_int),
                ("cell_size", C.c_float)]


class MatchCfg(C.Structure):
    _fields_ = [("NUM_MATCH_POINTS", C.c_int), ("MAX_NUM_MATCHES", C.c_int), ("MAX_NUM_PC2MATCH", C.c_int),
                ("MAX_DIST_PLANE", C.c_double), ("PLANE_THRESHOLD", C.c_double), ("estimate_extrinsics", C.c_int)]


class Frame(C.Structure):
    _fields_ = [("p", C.c_float * 3), ("q", C.c_float * 4), ("v", C.c_float * 3), ("g", C.c_float * 3),
                ("w", C.c_float * 3), ("a", C.c_float * 3), ("bg", C.c_float * 3), ("ba", C.c_float * 3),
                ("time", C.c_double)]


class FilterCfg(C.Structure):
    """flimo_filter_cfg (include/flimo_c.h)."""
    _fields_ = [("crop_active", C.c_int), ("crop_min", C.c_float * 3), ("crop_max", C.c_float * 3), ("dist_active", C.c_int),
                ("min_dist", C.c_float), ("rate_active", C.c_int), ("rate_value", C.c_int), ("time_kind", C.c_int),
                ("end_of_sweep", C.c_int), ("sweep_ref_time", C.c_double), ("fov_active", C.c_int), ("fov_angle", C.c_float)]


class CarveCfg(C.Structure):
    """flimo_carve_cfg (include/flimo_c.h)."""
    _fields_ = [("res", C.c_int), ("win", C.c_int), ("margin", C.c_float), ("rel_margin", C.c_float), ("max_depth", C.c_float)]


class _Stats(C.Structure):
    """The statistics an entry returns: counters and, in float64, moments."""

    def as_dict(self):
        return {name: (float if kind in (C.c_double, C.c_float) else int)(getattr(self, name)) for name, kind in self._fields_}


class OutlierCfg(C.Structure):
    """flimo_outlier_cfg (include/flimo_c.h)."""
    _fields_ = [("k", C.c_int), ("max_dist", C.c_float), ("min_pts", C.c_int), ("std_mul", C.c_float)]


class OutlierStats(_Stats):
    """flimo_outlier_stats (include/flimo_c.h)."""
    _fields_ = [("n", C.c_uint64), ("n_stat", C.c_uint64), ("mu", C.c_double), ("sigma", C.c_double), ("threshold", C.c_double),
                ("few", C.c_uint64), ("far", C.c_uint64), ("outliers", C.c_uint64)]


class FpfhCfg(C.Structure):
    """flimo_fpfh_cfg (include/flimo_c.h)."""
    _fields_ = [("k", C.c_int), ("max_dist", C.c_float), ("normal_k", C.c_int), ("normal_max_dist", C.c_float), ("normal_min_pts", C.c_int),
                ("has_viewpoint", C.c_int), ("viewpoint", C.c_float * 3)]


class KeypointCfg(C.Structure):
    """flimo_keypoint_cfg (include/flimo_c.h)."""
    _fields_ = [("k", C.c_int), ("max_dist", C.c_float), ("min_pts", C.c_int), ("gamma21", C.c_float), ("gamma32", C.c_float),
                ("nms_k", C.c_int), ("nms_max_dist", C.c_float)]


class ClusterCfg(C.Structure):
    """flimo_cluster_cfg (include/flimo_c.h)."""
    _fields_ = [("tol", C.c_float), ("min_size", C.c_int), ("max_size", C.c_int)]


class ClusterStats(_Stats):
    """flimo_cluster_stats (include/flimo_c.h)."""
    _fields_ = [("n", C.c_uint64), ("clusters", C.c_uint64), ("largest", C.c_uint64), ("sel_clusters", C.c_uint64),
                ("sel_points", C.c_uint64)]


class CorrCfg(C.Structure):
    """flimo_corr_cfg (include/flimo_c.h)."""
    _fields_ = [("edge_sim", C.c_float), ("min_edge", C.c_float), ("max_dist", C.c_float)]


class PlaneCfg(C.Structure):
    """flimo_plane_cfg (include/flimo_c.h)."""
    _fields_ = [("dist", C.c_float), ("min_edge", C.c_float), ("min_sin", C.c_float), ("axis", C.c_float * 3), ("min_cos", C.c_float)]


class PlaneSel(C.Structure):
    """flimo_plane_sel (include/flimo_c.h)."""
    _fields_ = [("normal", C.c_float * 3), ("anchor", C.c_float * 3), ("dist", C.c_float), ("side", C.c_int)]


class VoxelCfg(C.Structure):
    """flimo_voxel_cfg (include/flimo_c.h)."""
    _fields_ = [("leaf", C.c_float), ("keep", C.c_int), ("max_pts", C.c_int)]


class VoxelStats(_Stats):
    """flimo_voxel_stats (include/flimo_c.h)."""
    _fields_ = [("n", C.c_uint64), ("voxels", C.c_uint64), ("largest", C.c_uint64), ("outside", C.c_uint64), ("sel_points", C.c_uint64)]


class RegionCfg(C.Structure):
    """flimo_region_cfg (include/flimo_c.h)."""
    _fields_ = [("tol", C.c_float), ("normal_k", C.c_int), ("normal_max_dist", C.c_float), ("normal_min_pts", C.c_int), ("min_cos", C.c_float),
                ("max_curv", C.c_float), ("border", C.c_int), ("min_size", C.c_int), ("max_size", C.c_int)]


class RegionStats(_Stats):
    """flimo_region_stats (include/flimo_c.h)."""
    _fields_ = [("n", C.c_uint64), ("smooth", C.c_uint64), ("regions", C.c_uint64), ("largest", C.c_uint64), ("sel_regions", C.c_uint64),
                ("unassigned", C.c_uint64), ("sel_points", C.c_uint64)]


class NdtCfg(C.Structure):
    """flimo_ndt_cfg (include/flimo_c.h)."""
    _fields_ = [("leaf", C.c_float), ("min_pts", C.c_int), ("eig_ratio", C.c_double)]


class NdtInfo(_Stats):
    """flimo_ndt_model_info (include/flimo_c.h)."""
    _fields_ = [("cells", C.c_uint64), ("map_size_at_build", C.c_uint64), ("eig_ratio", C.c_double), ("leaf", C.c_float),
                ("min_pts", C.c_int), ("stale", C.c_int)]


class GicpCfg(C.Structure):
    """flimo_gicp_cfg (include/flimo_c.h)."""
    _fields_ = [("k", C.c_int), ("max_dist", C.c_float), ("min_pts", C.c_int), ("rule", C.c_int), ("eps", C.c_double)]


class GicpInfo(_Stats):
    """flimo_gicp_model_info (include/flimo_c.h)."""
    _fields_ = [("points", C.c_uint64), ("n_cov", C.c_uint64), ("eps", C.c_double), ("k", C.c_int), ("max_dist", C.c_float),
                ("min_pts", C.c_int), ("rule", C.c_int), ("stale", C.c_int)]


class ScCfg(C.Structure):
    """flimo_sc_cfg (include/flimo_c.h)."""
    _fields_ = [("rings", C.c_int), ("sectors", C.c_int), ("min_range", C.c_float), ("max_range", C.c_float), ("z_offset", C.c_float)]


class ScMatchCfg(C.Structure):
    """flimo_sc_match_cfg (include/flimo_c.h)."""
    _fields_ = [("k", C.c_int), ("min_cols", C.c_int), ("max_dist", C.c_float)]


class CorrGraphCfg(C.Structure):
    """flimo_corr_graph_cfg (include/flimo_c.h)."""
    _fields_ = [("tol", C.c_float), ("min_edge", C.c_float), ("edge_sim", C.c_float)]


class ChainPass(C.Structure):
    _fields_ = [("M", C.c_int), ("stragglers", C.c_int), ("ties", C.c_int), ("HTH", C.c_double * 144), ("HTh", C.c_double * 12),
                ("dx", C.c_double * 23), ("x_after", C.c_double * 26)]


class ChainIO(C.Structure):
    """flimo_chain_io (include/flimo_c.h): arguments and results of flimo_update_chain."""
    _fields_ = [("x26", C.c_double * 26), ("P", C.c_double * 529), ("limits", C.c_double * 23), ("R", C.c_double), ("D", C.c_double),
                ("max_iter", C.c_int), ("want_log", C.c_int),
                ("status", C.c_int), ("reason", C.c_int), ("passes", C.c_int), ("it_next", C.c_int), ("t", C.c_int),
                ("x26_out", C.c_double * 26), ("meas_valid", C.c_int), ("meas_M", C.c_int), ("meas_HTH", C.c_double * 144),
                ("meas_HTh", C.c_double * 12), ("log", ChainPass * CHAIN_MAX_PASSES)]


class LocCfg(C.Structure):
    _fields_ = [
        ("NUM_MATCH_POINTS", C.c_int), ("MAX_NUM_MATCHES", C.c_int), ("MAX_NUM_PC2MATCH", C.c_int),
        ("bucket_size", C.c_int),
        ("MAX_DIST_PLANE", C.c_double), ("PLANE_THRESHOLD", C.c_double),
        ("min_extent", C.c_float), ("downsampling", C.c_int),
        ("MAX_NUM_ITERS", C.c_int), ("estimate_extrinsics", C.c_int),
        ("LIMITS", C.c_double * 23),
        ("cov_gyro", C.c_double), ("cov_acc", C.c_double), ("cov_bias_gyro", C.c_double), ("cov_bias_acc", C.c_double),
        ("time_offset", C.c_int), ("end_of_sweep", C.c_int), ("num_threads", C.c_int),
        ("imu2baselink_t", C.c_float * 3), ("imu2baselink_R", C.c_float * 9),
        ("lidar2baselink_t", C.c_float * 3), ("lidar2baselink_R", C.c_float * 9),
        ("accel_bias", C.c_float * 3), ("gyro_bias", C.c_float * 3), ("imu_sm", C.c_float * 9),
        ("voxel_active", C.c_int), ("leaf_size", C.c_float),
        ("crop_active", C.c_int), ("cropBoxMin", C.c_float * 3), ("cropBoxMax", C.c_float * 3),
        ("dist_active", C.c_int), ("min_dist", C.c_double),
        ("rate_active", C.c_int), ("rate_value", C.c_int),
        ("fov_active", C.c_int), ("fov_angle", C.c_float),
        ("sensor_type", C.c_int),
        ("gravity_align", C.c_int), ("calibrate_accel", C.c_int), ("calibrate_gyro", C.c_int),
        ("imu_calib_time", C.c_double),
        ("gpu_device", C.c_int), ("gpu_cell_size", C.c_float), ("debug", C.c_int),
    ]


# ---- the functions ----
P = C.POINTER
vp, sz, i, f, d, u64, ull = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double, C.c_uint64, C.c_ulonglong
uintpp = np.ctypeslib.ndpointer(np.uintp, flags="C_CONTIGUOUS")

# What a flimo_ctx and a flimo_loc both offer: (symbol of libflimo_hip.so, symbol of libfast_limo.so, the arguments after the
# handle); every one returns the code.  Arrays go in as addresses (``.ctypes.data``, None for an optional one left out).
PAIRED = (
    ("flimo_map_seen_through", "flimo_loc_map_seen_through", [vp, vp, P(CarveCfg), vp, sz, P(sz)]),
    ("flimo_map_carve", "flimo_loc_map_carve", [vp, vp, P(CarveCfg), vp, vp, P(sz)]),
    ("flimo_map_outliers", "flimo_loc_map_outliers", [sz, sz, P(OutlierCfg), vp, vp, vp, P(OutlierStats)]),
    ("flimo_map_remove_outliers", "flimo_loc_map_remove_outliers", [sz, sz, P(OutlierCfg), P(sz), P(OutlierStats)]),
    ("flimo_map_fpfh", "flimo_loc_map_fpfh", [sz, sz, P(FpfhCfg), vp, vp, vp]),
    ("flimo_map_keypoints", "flimo_loc_map_keypoints", [sz, sz, P(KeypointCfg), vp, vp, vp, P(sz)]),
    ("flimo_map_clusters", "flimo_loc_map_clusters", [sz, sz, P(ClusterCfg), vp, vp, vp, P(ClusterStats)]),
    ("flimo_map_remove_clusters", "flimo_loc_map_remove_clusters", [sz, sz, P(ClusterCfg), P(sz), P(ClusterStats)]),
    ("flimo_map_planes", "flimo_loc_map_planes", [vp, sz, P(PlaneCfg), vp, vp, vp, vp]),
    ("flimo_map_plane_mask", "flimo_loc_map_plane_mask", [sz, sz, P(PlaneSel), vp, P(sz)]),
    ("flimo_map_remove_plane", "flimo_loc_map_remove_plane", [sz, sz, P(PlaneSel), P(sz)]),
    ("flimo_map_voxels", "flimo_loc_map_voxels", [P(VoxelCfg), sz, P(sz), vp, vp, vp, vp, vp, vp, P(VoxelStats)]),
    ("flimo_map_voxel_mask", "flimo_loc_map_voxel_mask", [sz, sz, P(VoxelCfg), vp, vp, P(VoxelStats)]),
    ("flimo_map_thin", "flimo_loc_map_thin", [sz, sz, P(VoxelCfg), P(sz), P(VoxelStats)]),
    ("flimo_map_regions", "flimo_loc_map_regions", [sz, sz, P(RegionCfg), vp, vp, vp, P(RegionStats)]),
    ("flimo_map_region_list", "flimo_loc_map_region_list", [P(RegionCfg), sz, P(sz), vp, vp, vp, vp, vp, P(RegionStats)]),
    ("flimo_map_remove_regions", "flimo_loc_map_remove_regions", [sz, sz, P(RegionCfg), P(sz), P(RegionStats)]),
    ("flimo_radius_search", "flimo_loc_map_radius_search", [vp, sz, f, C.c_uint, vp, vp, vp, vp, sz, P(u64)]),
    ("flimo_knn_k", "flimo_loc_map_knn", [vp, sz, i, f, vp, vp, vp, vp]),
    ("flimo_map_normals", "flimo_loc_map_normals", [vp, sz, i, f, i, vp, vp, vp, vp, vp, vp]),
    ("flimo_map_normals_range", "flimo_loc_map_normals_range", [sz, sz, i, f, i, vp, vp, vp, vp, vp, vp]),
    ("flimo_scan_fitness", "flimo_loc_scan_fitness", [vp, sz, f, vp, vp, vp, vp]),
    ("flimo_scan_linearize", "flimo_loc_scan_linearize", [vp, sz, i, f, i, f, vp, vp, vp, vp, vp, vp]),
    ("flimo_corr_poses", "flimo_loc_corr_poses", [vp, vp, sz, vp, sz, P(CorrCfg), vp, vp, vp, vp, vp]),
    ("flimo_corr_graph", "flimo_loc_corr_graph", [vp, vp, sz, P(CorrGraphCfg), vp, vp, vp, vp]),
    ("flimo_desc_ref_set", "flimo_loc_desc_ref_set", [vp, sz, i]),
    ("flimo_desc_match", "flimo_loc_desc_match", [vp, sz, i, i, vp, vp, vp]),
)
# The resident NDT models and the passes against them: paired rows like the ones above, in a table of their own.
PAIRED_NDT = (
    ("flimo_ndt_build", "flimo_loc_ndt_build", [i, P(NdtCfg), P(sz)]),
    ("flimo_ndt_cells", "flimo_loc_ndt_cells", [i, sz, P(sz), vp, vp, vp, vp, vp, vp]),
    ("flimo_ndt_info", "flimo_loc_ndt_info", [i, P(NdtInfo)]),
    ("flimo_ndt_clear", "flimo_loc_ndt_clear", [i]),
    ("flimo_scan_ndt", "flimo_loc_scan_ndt", [i, vp, sz, i, d, vp, vp, vp, vp, vp, vp, vp]),
)
# The resident GICP model, the scan's covariances and the pass against both.
PAIRED_GICP = (
    ("flimo_gicp_build", "flimo_loc_gicp_build", [P(GicpCfg), P(sz)]),
    ("flimo_gicp_model", "flimo_loc_gicp_model", [sz, sz, vp]),
    ("flimo_gicp_info", "flimo_loc_gicp_info", [P(GicpInfo)]),
    ("flimo_gicp_clear", "flimo_loc_gicp_clear", []),
    ("flimo_scan_cov_set", "flimo_loc_scan_cov_set", [vp, sz]),
    ("flimo_scan_gicp", "flimo_loc_scan_gicp", [vp, sz, f, vp, vp, vp, vp, vp, vp]),
)
# Scan Context: the descriptor of the resident scan, the resident database and the match.
PAIRED_SC = (
    ("flimo_scan_context", "flimo_loc_scan_context", [P(ScCfg), vp, vp, vp]),
    ("flimo_sc_db_add", "flimo_loc_sc_db_add", [vp, sz, i, i, P(sz)]),
    ("flimo_sc_db_add_scan", "flimo_loc_sc_db_add_scan", [P(ScCfg), vp, P(sz)]),
    ("flimo_sc_db_get", "flimo_loc_sc_db_get", [sz, sz, vp]),
    ("flimo_sc_db_clear", "flimo_loc_sc_db_clear", []),
    ("flimo_sc_match", "flimo_loc_sc_match", [vp, sz, i, i, sz, sz, P(ScMatchCfg), vp, vp, vp, vp, vp]),
)
# Map segments: the table, the move of the map by segment, forgetting by age.
PAIRED_SEG = (
    ("flimo_map_segment_mark", "flimo_loc_map_segment_mark", [P(sz)]),
    ("flimo_map_segments", "flimo_loc_map_segments", [vp, sz, P(sz), P(i)]),
    ("flimo_map_segments_reset", "flimo_loc_map_segments_reset", []),
    ("flimo_map_corrected", "flimo_loc_map_corrected", [vp, sz, sz, sz, vp, P(sz)]),
    ("flimo_map_correct", "flimo_loc_map_correct", [vp, sz, P(sz)]),
    ("flimo_map_transform", "flimo_loc_map_transform", [vp, P(sz)]),
    ("flimo_map_remove_range", "flimo_loc_map_remove_range", [sz, sz, P(sz)]),
)
PAIRED_ALL = PAIRED + PAIRED_NDT + PAIRED_GICP + PAIRED_SC + PAIRED_SEG
LOC_OF = {hip: loc for hip, loc, _ in PAIRED_ALL}

# Everything else: (result, symbol, every argument -- the handle, where there is one, included).
HIP_ONLY = (
    (i, "flimo_ctx_create", [i, P(vp)]),
    (None, "flimo_ctx_destroy", [vp]),
    (C.c_char_p, "flimo_last_error", [vp]),
    (C.c_char_p, "flimo_version", []),
    # map
    (i, "flimo_map_config", [vp, P(MapCfg)]),
    (i, "flimo_map_add", [vp, f32p, sz, sz, d]),
    (i, "flimo_map_clear", [vp]),
    (i, "flimo_map_crop_box", [vp, vp, vp, P(sz)]),
    (i, "flimo_map_crop_stats", [vp, P(u64)]),
    (i, "flimo_map_carve_stats", [vp, P(u64)]),
    (sz, "flimo_map_size", [vp]),
    (d, "flimo_map_last_time", [vp]),
    (i, "flimo_map_points", [vp, vp, sz, P(sz)]),
    (i, "flimo_map_add_scan", [vp, f64p, d]),
    (i, "flimo_knn", [vp, f32p, sz, i, i32p, f32p, i32p]),
    (i, "flimo_radius_candidates", [vp, f32p, sz, f, vp]),
    (i, "flimo_knn_k_candidates", [vp, vp, sz, i, f, vp]),
    # chunks and plans of the map and scan entries
    (i, "flimo_set_outlier_chunk", [vp, sz]),
    (i, "flimo_set_fpfh_chunk", [vp, sz]),
    (i, "flimo_set_keypoints_chunk", [vp, sz]),
    (i, "flimo_set_cluster_chunk", [vp, sz]),
    (i, "flimo_set_plane_chunk", [vp, sz]),
    (i, "flimo_set_voxel_plan", [vp, i]),
    (i, "flimo_set_region_chunk", [vp, sz]),
    (i, "flimo_set_normals_chunk", [vp, sz]),
    (i, "flimo_set_fitness_chunk", [vp, sz]),
    (i, "flimo_set_linearize_chunk", [vp, sz]),
    (i, "flimo_set_ndt_chunk", [vp, sz]),
    (i, "flimo_set_gicp_chunk", [vp, sz]),
    (i, "flimo_set_corr_chunk", [vp, sz]),
    (i, "flimo_set_desc_chunk", [vp, sz, sz]),
    (sz, "flimo_desc_ref_size", [vp]),
    (i, "flimo_desc_ref_dim", [vp]),
    (f, "flimo_desc_last_ms", [vp]),
    (i, "flimo_set_sc_chunk", [vp, sz, sz]),
    (sz, "flimo_sc_db_size", [vp]),
    (i, "flimo_sc_db_shape", [vp, P(i), P(i)]),
    (f, "flimo_sc_last_ms", [vp]),
    (i, "flimo_set_segment_plan", [vp, sz, i]),
    # the functions the kernels call, on the host
    (i, "flimo_plane_solve_host", [vp, P(PlaneCfg), vp, vp]),
    (i, "flimo_voxel_key_host", [vp, f, vp, P(u64)]),
    (i, "flimo_region_joined_host", [vp, vp, vp, vp, P(RegionCfg), P(i), P(i), P(i)]),
    (i, "flimo_corr_pose_host", [vp, vp, P(CorrCfg), vp, vp]),
    (i, "flimo_corr_compatible_host", [vp, vp, vp, vp, P(CorrGraphCfg)]),
    (i, "flimo_desc_dist_host", [vp, vp, i, vp]),
    (i, "flimo_sc_bin_host", [vp, P(ScCfg), vp, P(i), P(i), P(f)]),
    (i, "flimo_sc_dist_host", [vp, vp, i, i, i, P(f), P(i), vp]),
    (i, "flimo_ndt_term_host", [vp, vp, vp, vp, vp, vp, d, vp]),
    (i, "flimo_gicp_eigen_host", [vp, vp]),
    (i, "flimo_gicp_regularize_host", [vp, i, d, vp]),
    (i, "flimo_gicp_term_host", [vp, vp, vp, vp, vp, vp, vp]),
    (i, "flimo_seg_move_host", [vp, vp, vp]),
    (None, "flimo_plane_fit5_host", [f32p, f32p]),
    (i, "flimo_plane_eval5_host", [f32p, f32p, f]),
    (i, "flimo_calculate_H_host", [f64p, f32p, f32p, f32p, sz, i, f64p, f64p]),
    (i, "flimo_insert_rule_replay", [f, i, f32p, vp, sz, vp, P(sz)]),
    # scan
    (i, "flimo_scan_set", [vp, f32p, sz, sz]),
    (sz, "flimo_scan_size", [vp]),
    (sz, "flimo_scan_cov_size", [vp]),
    (i, "flimo_scan_get", [vp, vp, sz, P(sz)]),
    (i, "flimo_scan_voxel_filter", [vp, f, P(sz)]),
    (i, "flimo_raw_scan_set", [vp, f32p, sz, sz, f64p]),
    (i, "flimo_raw_scan_filter_set", [vp, vp, sz, P(FilterCfg), P(sz), P(d), P(i)]),
    (i, "flimo_raw_scan_filter_order_set", [vp, vp, sz, P(FilterCfg), i, P(sz), P(d), P(i), P(i)]),
    (i, "flimo_raw_scan_order", [vp, vp, sz, P(sz)]),
    (i, "flimo_upload_stage", [vp, sz, P(vp)]),
    (i, "flimo_scan_adopt", [vp, vp]),
    (i, "flimo_deskew_resident", [vp, vp, sz, f32p, f64p]),
    (i, "flimo_deskew_resident_offset", [vp, vp, sz, f32p, f64p, d]),
    (i, "flimo_deskew", [vp, f32p, sz, sz, f64p, vp, sz, f32p, f64p]),
    (i, "flimo_scan_to_world", [vp, f64p, vp, sz]),
    (i, "flimo_scan_clouds", [vp, f64p, P(vp), P(vp), P(sz)]),
    (i, "flimo_scan_debug_clouds", [vp, f64p, P(vp), P(vp), P(sz)]),
    # measurement pass and update
    (i, "flimo_match_reduce", [vp, f64p, P(MatchCfg), f64p, f64p, P(i)]),
    (i, "flimo_match_reduce_overlap", [vp, f64p, P(MatchCfg), f64p, f64p, P(i), vp, vp]),      # (.., void (*while_in_flight)(void*), void* arg)
    (i, "flimo_match_fetch", [vp, vp, sz, P(sz)]),
    (i, "flimo_match_fetch_H", [vp, vp, vp, sz, P(sz)]),
    (i, "flimo_update_chain", [vp, P(MatchCfg), P(ChainIO)]),
    (i, "flimo_chain_stats", [vp, f64p, i]),
    (i, "flimo_set_update_mode", [vp, i]),
    (i, "flimo_update_mode", [vp, P(i), P(d)]),
    (i, "flimo_set_pass_pipeline", [vp, i]),
    (i, "flimo_pass_pipeline_end", [vp]),
    (i, "flimo_pass_pipeline_last", [vp]),
    (i, "flimo_pass_pipeline_stats", [vp, P(ull)]),
    (i, "flimo_device_large_bar", [i, P(i)]),
    # instrumentation
    (i, "flimo_set_timing", [vp, i]),
    (i, "flimo_set_timing_stride", [vp, i]),
    (i, "flimo_set_timing_deferred", [vp, i]),
    (i, "flimo_set_wait_timeout_ms", [vp, i]),
    (i, "flimo_set_debug_records", [vp, i]),
    (i, "flimo_set_path_switches", [vp, i, i]),
    (ull, "flimo_pass_count", [vp]),
    (ull, "flimo_fused_pass_count", [vp]),
    (i, "flimo_tie_stats", [vp, P(ull)]),
    (i, "flimo_fine_stats", [vp, P(ull)]),
    (i, "flimo_map_index_bytes", [vp, P(u64)]),
    (i, "flimo_map_index_layout", [vp, i, P(d)]),
    (i, "flimo_map_grid_selfcheck", [vp, P(u64), P(u64)]),
    (i, "flimo_last_kernel_ms", [vp, P(f), P(f), P(f)]),
    (d, "flimo_last_candidates_per_query", [vp]),
    (i, "flimo_last_widen_count", [vp]),
    (i, "flimo_last_stragglers", [vp]),
    (i, "flimo_stragglers_by_pass", [vp, P(i)]),
    (i, "flimo_timing_totals", [vp, P(d), P(d), P(d), P(C.c_longlong), P(C.c_longlong), i]),
    (i, "flimo_timing_split", [vp, f64p, i]),
    # the filter's device algebra on its own
    (i, "flimo_ieskf_op_shape", [i, P(i), P(i)]),
    (i, "flimo_ieskf_eval", [vp, i, f64p, sz, f64p]),
    (i, "flimo_ieskf_eval_host", [i, f64p, sz, f64p, vp]),
    (i, "flimo_ieskf_run_fixed", [vp, f64p, f64p, f64p, d, d, i, i, f64p, f64p, vp, f64p, f64p, P(i)]),
)

HOST_ONLY = (
    (i, "flimo_loc_create", [P(LocCfg), P(vp)]),
    (None, "flimo_loc_destroy", [vp]),
    (vp, "flimo_loc_ctx", [vp]),
    (None, "flimo_loc_sync", [vp]),
    (None, "flimo_loc_set_async_insert", [vp, i]),
    (None, "flimo_loc_set_lazy_time_order", [vp, i]),
    (None, "flimo_loc_set_gpu_filters", [vp, i]),
    (None, "flimo_loc_set_exact_tied_order", [vp, i]),
    (None, "flimo_loc_set_local_map", [vp, f32p, f]),
    (i, "flimo_local_map_rule", [f64p, f32p, f, f64p, P(i), f32p, f32p]),
    (None, "flimo_loc_set_map_carving", [vp, i, P(CarveCfg)]),
    (i, "flimo_carve_rule", [i, P(i)]),
    (None, "flimo_carve_sensor", [f64p, f32p]),
    (sz, "flimo_loc_last_carve_removed", [vp]),
    (i, "flimo_loc_last_sweep_tied", [vp]),
    (None, "flimo_loc_set_propagation_wait", [vp, d]),
    (d, "flimo_loc_last_insert_seconds", [vp]),
    (i, "flimo_loc_update_imu", [vp, d, f32p, f32p]),
    (i, "flimo_loc_update_imu_n", [vp, sz, f64p, f32p, f32p]),
    (i, "flimo_loc_replay", [vp, sz, P(vp), uintpp, f64p, f64p, sz, f64p, f32p, f32p, i32p, f64p]),
    (i, "flimo_loc_update_pointcloud", [vp, f32p, sz, d]),
    (i, "flimo_loc_update_pointcloud_points", [vp, vp, sz, d]),
    (i, "flimo_loc_map_add", [vp, f32p, sz, d]),
    (sz, "flimo_loc_map_size", [vp]),
    (None, "flimo_loc_get_x", [vp, f64p]),
    (None, "flimo_loc_set_x", [vp, f64p]),
    (None, "flimo_loc_get_P", [vp, f64p]),
    (None, "flimo_loc_set_P", [vp, f64p]),
    (None, "flimo_loc_set_flags", [vp, i, i, i]),
    (i, "flimo_loc_num_passes", [vp]),
    (None, "flimo_loc_get_pass", [vp, i, P(i), f64p, f64p, f64p, f64p]),
    (sz, "flimo_loc_get_pc2match", [vp, vp, sz]),
    (sz, "flimo_loc_get_final_scan", [vp, vp, sz]),
    (sz, "flimo_loc_get_debug_cloud", [vp, i, vp, sz]),
    (None, "flimo_loc_get_stage_times", [vp, f64p]),
    (None, "flimo_loc_get_pose_cov", [vp, f64p]),
    (None, "flimo_loc_host_profile", [vp, f64p, i]),
    (i, "flimo_loc_register_resident", [vp, f64p, f64p]),
    # the host mirror's pieces on their own
    (None, "flimo_host_state_update", [f32p, d, d]),
    (i, "flimo_host_time_order", [vp, i, sz, i, i, vp]),
    (i, "flimo_host_plane", [f32p, f32p, i, i, d, d, f32p, f32p, P(f)]),
    (i, "flimo_eskf_update_fixed", [f64p, f64p, f64p, f64p, i, i, f64p, d, d, P(i)]),
    (i, "flimo_eskf_predict", [f64p, f64p, d, f64p, f64p, f64p]),
    (i, "flimo_ieskf_gj12_host", [i, f64p, sz, f64p]),
    (i, "flimo_ieskf_run_fixed_host", [f64p, f64p, f64p, d, d, i, i, f64p, f64p, P(i), f64p, f64p, P(i)]),
    (None, "flimo_host_eigen_solver6", [f64p, f64p, f64p, f64p]),
)

HIP_SYMBOLS = [hip for hip, _, _ in PAIRED_ALL] + [name for _, name, _ in HIP_ONLY]
HOST_SYMBOLS = [loc for _, loc, _ in PAIRED_ALL] + [name for _, name, _ in HOST_ONLY]


def declare(lib, side):
    """Give every function of ``lib`` its result and argument types; ``side`` 0: libflimo_hip.so, 1: libfast_limo.so."""
    for row in PAIRED_ALL:
        fn = getattr(lib, row[side])
        fn.restype, fn.argtypes = C.c_int, [vp] + row[2]
    for restype, name, args in (HIP_ONLY, HOST_ONLY)[side]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, args
