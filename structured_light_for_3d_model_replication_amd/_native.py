"""ctypes binding of ``libslgpu.so`` (C ABI in ``include/slgpu.h``).

The library is built in-tree (``build.build_native``) and must be present: there is no CPU
fallback in the product path.  ``torch`` is imported first so that the library's
``libamdhip64.so.7`` dependency resolves to the HIP runtime torch already loaded (one HIP
runtime per process; a second one would not understand torch's streams or pointers).
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

LIB_NAME = "libslgpu.so"
PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)
# A/B builds of the same ABI (tools/build_ab.sh -> ab_libs/, build_ab/; tools/kbench.py, ab.py):
# only libraries inside those in-tree build directories may replace the product library
AB_DIRS = (os.path.join(REPO_DIR, "ab_libs"), os.path.join(REPO_DIR, "build_ab"))
AB_LIB = None
if os.environ.get("SLG_LIB"):
    _p = os.path.realpath(os.environ["SLG_LIB"])
    if not any(os.path.commonpath([_p, os.path.realpath(d)]) == os.path.realpath(d) for d in AB_DIRS):
        raise ImportError(f"SLG_LIB={_p}: A/B libraries must live in {' or '.join(AB_DIRS)}")
    LIB_PATH = AB_LIB = _p

ABI_VERSION = 2          # SLG_ABI_VERSION in include/slgpu.h
SLG_OK = 0
SLG_ERR_INVALID = 1
SLG_ERR_HIP = 2
SLG_ERR_UNSUPPORTED = 3
SLG_ERR_NOT_ENOUGH = 4
SLG_ERR_INDEX = 5

THRESH_OTSU, THRESH_MANUAL, THRESH_PERCENTILE = 0, 1, 2
VARIANT_PROCESSING, VARIANT_SLSYSTEM = 0, 1
RAYS_TABLE, RAYS_PINHOLE = 0, 1
GRAY_PNG, GRAY_BMP = 0, 1

c_i32, c_i64, c_dbl, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p


class Capture(ctypes.Structure):
    _fields_ = [("frames", c_vp), ("frame_stride", c_i64), ("n_frames", c_i32),
                ("height", c_i32), ("width", c_i32), ("reserved", c_i32), ("texture", c_vp)]


class DecodeParams(ctypes.Structure):
    _fields_ = [("proj_cols", c_i32), ("proj_rows", c_i32), ("n_sets_col", c_i32),
                ("n_sets_row", c_i32), ("variant", c_i32), ("thresh_mode", c_i32),
                ("shadow_val", c_dbl), ("contrast_val", c_dbl)]


class Calib(ctypes.Structure):
    _fields_ = [("rays", c_vp), ("ray_mode", c_i32), ("reserved", c_i32),
                ("fx", c_dbl), ("fy", c_dbl), ("cx", c_dbl), ("cy", c_dbl),
                ("oc", c_dbl * 3), ("col_planes", c_vp), ("n_col_planes", c_i32),
                ("reserved2", c_i32), ("row_planes", c_vp), ("n_row_planes", c_i32),
                ("reserved3", c_i32), ("col_planes_num", c_vp), ("row_planes_num", c_vp)]


class TriParams(ctypes.Structure):
    _fields_ = [("row_mode", c_i32), ("xyz_f64", c_i32), ("epipolar_tol", c_dbl)]


class Maps(ctypes.Structure):
    _fields_ = [("col", c_vp), ("row", c_vp), ("mask", c_vp), ("texture", c_vp),
                ("height", c_i32), ("width", c_i32)]


class Cloud(ctypes.Structure):
    _fields_ = [("xyz", c_vp), ("bgr", c_vp), ("count", c_vp), ("capacity", c_i64)]


class PngFrame(ctypes.Structure):
    _fields_ = [("z", c_vp), ("zlen", c_i64), ("raw", c_vp), ("out", c_vp), ("out_pitch", c_i64),
                ("width", c_i32), ("height", c_i32), ("channels", c_i32), ("reserved", c_i32)]


PNG_E_STREAM, PNG_E_SIZE, PNG_E_ADLER, PNG_E_FILTER, PNG_E_UNSUPPORTED = 1, 2, 3, 4, 5


EXPORTS = {
    "slg_version": (c_i32, []),
    "slg_build_id": (ctypes.c_char_p, []),
    "slg_kernel_table": (c_i32, [ctypes.c_char_p, c_i64]),
    "slg_last_kernel": (c_i32, [ctypes.c_char_p, c_i64]),
    "slg_last_error": (ctypes.c_char_p, []),
    "slg_workspace_bytes": (c_i64, [c_i64]),
    "slg_workspace_init": (c_i32, [c_vp, c_i64, c_vp]),
    "slg_workspace_set_arena": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_vp]),
    "slg_decode_stats": (c_i32, [ctypes.POINTER(Capture), ctypes.POINTER(DecodeParams), c_vp, c_vp]),
    "slg_decode_histograms": (c_i32, [ctypes.POINTER(Capture), ctypes.POINTER(DecodeParams), c_vp, c_vp, c_vp]),
    "slg_thresholds_from_histograms": (c_i32, [c_vp, c_i64, ctypes.POINTER(DecodeParams), c_vp, c_i64, c_vp]),
    "slg_decode": (c_i32, [ctypes.POINTER(Capture), ctypes.POINTER(DecodeParams), c_vp,
                           c_vp, c_vp, c_vp, c_vp]),
    "slg_triangulate": (c_i32, [ctypes.POINTER(Maps), ctypes.POINTER(Calib),
                                ctypes.POINTER(TriParams), c_vp, ctypes.POINTER(Cloud), c_vp]),
    "slg_reconstruct": (c_i32, [ctypes.POINTER(Capture), ctypes.POINTER(DecodeParams),
                                ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp,
                                ctypes.POINTER(Cloud), c_vp]),
    "slg_decode_triangulate": (c_i32, [ctypes.POINTER(Capture), ctypes.POINTER(DecodeParams),
                                       ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp,
                                       ctypes.POINTER(Cloud), c_vp]),
    "slg_reconstruct_batch": (c_i32, [ctypes.POINTER(Capture), c_i32, ctypes.POINTER(DecodeParams),
                                      ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp, c_i64,
                                      ctypes.POINTER(Cloud), ctypes.POINTER(c_vp), c_vp]),
    "slg_decode_stats_batch": (c_i32, [ctypes.POINTER(Capture), c_i32, ctypes.POINTER(DecodeParams),
                                       c_vp, c_i64, c_vp]),
    "slg_decode_triangulate_batch": (c_i32, [ctypes.POINTER(Capture), c_i32, ctypes.POINTER(DecodeParams),
                                             ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp,
                                             c_i64, ctypes.POINTER(Cloud), ctypes.POINTER(c_vp), c_vp]),
    "slg_decode_triangulate_batch_next": (c_i32, [ctypes.POINTER(Capture), c_i32, ctypes.POINTER(DecodeParams),
                                                  ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp,
                                                  c_i64, ctypes.POINTER(Cloud), ctypes.POINTER(Capture), c_i32,
                                                  ctypes.POINTER(c_vp), c_vp]),
    "slg_decode_triangulate_batch_carry": (c_i32, [ctypes.POINTER(Capture), c_i32, ctypes.POINTER(DecodeParams),
                                                   ctypes.POINTER(Calib), ctypes.POINTER(TriParams), c_vp,
                                                   c_i64, ctypes.POINTER(Cloud), ctypes.POINTER(Capture), c_i32,
                                                   c_vp, c_i32, ctypes.POINTER(c_vp), c_vp]),
    "slg_decode_stats_partials_batch": (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(DecodeParams), c_vp, c_i64,
                                                c_vp]),
    "slg_ply_write": (c_i64, [ctypes.c_char_p, c_vp, c_vp, c_i64, c_i32]),
    "slg_ply_format_bound": (c_i64, [c_i64]),
    "slg_ply_format_ws_bytes": (c_i64, [c_i64]),
    "slg_ply_format": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_png_gray8_size": (c_i32, [ctypes.c_char_p, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "slg_png_gray8_decode": (c_i32, [ctypes.c_char_p, c_vp, c_i64, c_i32, c_i32]),
    "slg_png_zstream": (c_i32, [ctypes.c_char_p, c_vp, c_i64, ctypes.POINTER(c_i32)]),
    "slg_png_info": (c_i32, [ctypes.c_char_p, ctypes.POINTER(c_i32)]),
    "slg_png_read": (c_i32, [ctypes.c_char_p, c_vp, c_i64, c_vp, c_i64, ctypes.POINTER(c_i32)]),
    "slg_png_raw_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "slg_png_decode_device": (c_i32, [c_vp, c_i32, c_vp, c_vp]),
    "slg_stream_create_reserving": (c_i32, [c_i32, c_vp]),
    "slg_stream_destroy": (c_i32, [c_vp]),
    "slg_rays_match_pinhole": (c_i32, [c_vp, c_i32, c_i32, c_dbl, c_dbl, c_dbl, c_dbl, c_vp, c_vp]),
    "slg_rgb_to_gray": (c_i32, [c_vp, c_i32, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp, c_i32, c_vp]),
    "slg_gray_texture": (c_i32, [c_vp, c_i64, c_vp, c_vp]),
    "slg_gather_unique_id": (c_i32, [c_vp]),
    "slg_gather_init": (c_i32, [ctypes.POINTER(c_vp), c_i32, c_i32, c_vp]),
    "slg_gather_counts": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp]),
    "slg_gatherv": (c_i32, [c_vp, c_vp, c_i64, c_vp, ctypes.POINTER(c_i64), c_i32, c_vp]),
    "slg_gather_destroy": (c_i32, [c_vp]),
    "slg_gatherv_plan": (c_i32, [c_i32, c_i32, c_i32, c_i64, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64),
                                 ctypes.POINTER(c_i32)]),
    "slg_filter_ws_bytes": (c_i64, [c_i64, c_i32]),
    "slg_radius_outlier": (c_i32, [c_vp, c_i64, c_dbl, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_statistical_outlier": (c_i32, [c_vp, c_i64, c_i32, c_dbl, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_cloud_select": (c_i32, [c_vp, c_vp, c_i64, c_vp, ctypes.POINTER(Cloud), c_vp, c_vp, c_vp]),
    "slg_dbscan": (c_i32, [c_vp, c_i64, c_dbl, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_voxel_downsample": (c_i32, [c_vp, c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "slg_estimate_normals": (c_i32, [c_vp, c_i64, c_dbl, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_orient_normals": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i32, c_vp]),
    "slg_cloud_centroid": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "slg_icp_ws_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "slg_icp_point_to_plane": (c_i32, [c_vp, c_i64, c_vp, c_vp, c_i64, c_dbl, ctypes.POINTER(c_dbl), c_dbl, c_dbl,
                                       c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_cloud_transform": (c_i32, [c_vp, c_vp, c_i64, ctypes.POINTER(c_dbl), c_vp, c_vp, c_vp]),
    "slg_fpfh_ws_bytes": (c_i64, [c_i64, c_i32]),
    "slg_fpfh": (c_i32, [c_vp, c_vp, c_i64, c_dbl, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_feature_match_ws_bytes": (c_i64, [c_i64, c_i64]),
    "slg_feature_match": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "slg_ransac_ws_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "slg_ransac_prepare": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_ransac_batch": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_dbl, c_dbl, c_dbl, c_i64, c_i64,
                                 c_i32, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "slg_plane_ws_bytes": (c_i64, [c_i64, c_i32]),
    "slg_plane_batch": (c_i32, [c_vp, c_i64, c_dbl, c_i32, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp]),
    "slg_plane_finish": (c_i32, [c_vp, c_i64, ctypes.POINTER(c_dbl), c_dbl, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "slg_orient_ws_bytes": (c_i64, [c_i64, c_i32]),
    "slg_knn_lists": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_emst": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_orient_tangent": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "slg_mesh_ws_bytes": (c_i64, [c_i32, c_i32, c_i64, c_i64]),
    "slg_mesh_set_header": (c_i32, [c_vp, c_i32, ctypes.POINTER(c_dbl), c_dbl, c_dbl, c_vp]),
    "slg_mesh_grid": (c_i32, [c_vp, c_i64, c_i32, c_dbl, c_vp, c_i64, c_vp]),
    "slg_mesh_splat": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_mesh_divergence": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "slg_mesh_solve": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp]),
    "slg_mesh_sample": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_mesh_iso": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_mesh_count": (c_i32, [c_vp, c_i32, c_vp, c_i64, c_vp]),
    "slg_mesh_emit": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp]),
    "slg_mesh_quantile": (c_i32, [c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp]),
    "slg_mesh_remove": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "slg_mesh_triangle_normals": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "slg_mesh_stl_pack": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "slg_mesh_post_ws_bytes": (c_i64, [c_i32, c_i64, c_i64]),
    "slg_mesh_adjacency_count": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_i64, c_vp]),
    "slg_mesh_adjacency_emit": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "slg_mesh_smooth_pass": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_dbl, c_vp]),
    "slg_mesh_holes_count": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "slg_mesh_holes_emit": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_mesh_decimate_ws_bytes": (c_i64, [c_i64, c_i64]),
    "slg_mesh_decimate_init": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_mesh_decimate_round": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp]),
    "slg_mesh_decimate_emit": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
}
# The surface mesher's table (include/slgpu_surface.h, csrc/cloud_surface.hip): the same library,
# bound by the same lib().  A table of its own until a change that may edit the tests pinned to
# EXPORTS folds the two together.
SURFACE_EXPORTS = {
    "slg_surface_ws_bytes": (c_i64, [c_i32, c_i64, c_i64, c_i64]),
    "slg_surface_begin": (c_i32, [c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp]),
    "slg_surface_count": (c_i32, [c_vp, c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp, c_vp]),
    "slg_surface_emit": (c_i32, [c_vp, c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp]),
    "slg_surface_round": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_i64, c_vp]),
    "slg_surface_commit": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
}
# The banded mesher's table (include/slgpu_band.h, csrc/cloud_band.hip), by the same precedent
# (DESIGN.md §21).
BAND_EXPORTS = {
    "slg_band_ws_bytes": (c_i64, [c_i32, c_i32, c_i64, c_i64]),
    "slg_band_level": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    "slg_band_blocks": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "slg_band_nodes": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_band_splat": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_band_divergence": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "slg_band_prolong": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "slg_band_smooth": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "slg_band_iso": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_band_count": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "slg_band_emit": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64,
                              c_vp]),
}
# The mesh audit's table (include/slgpu_audit.h, csrc/cloud_audit.hip), by the same precedent
# (DESIGN.md §22).
AUDIT_EXPORTS = {
    "slg_audit_ws_bytes": (c_i64, [c_i32, c_i64, c_i64]),
    "slg_audit_edges": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_audit_components_count": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_audit_components_emit": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "slg_audit_fans": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "slg_audit_measure": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "slg_audit_keep": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "slg_audit_select": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
}
# The self-intersection test's table (include/slgpu_intersect.h, csrc/cloud_intersect.hip), by the same
# precedent.
INTERSECT_EXPORTS = {
    "slg_isect_ws_bytes": (c_i64, [c_i32, c_i64, c_i64, c_i64]),
    "slg_isect_boxes": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_dbl, c_vp, c_i64, c_vp]),
    "slg_isect_entries": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp]),
    "slg_isect_candidates_count": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    "slg_isect_candidates_emit": (c_i32, [c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp]),
    "slg_isect_test": (c_i32, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp]),
    "slg_isect_list": (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp]),
}
ISECT_WS_BOXES, ISECT_WS_ENTRIES, ISECT_WS_PAIRS, ISECT_WS_LIST = range(4)       # SLG_ISECT_WS_*
ISECT_SPAN_CAP, ISECT_MAX_CELLS, ISECT_TILE = 64, 1024, 64                       # SLG_ISECT_*
ISECT_BOUND_HEX = "0x1.c000000000007p-51"                                         # SLG_ISECT_BOUND: (7 + 56 E) E, E = 2^-53
ISECT_INTERSECTING, ISECT_UNCERTAIN = 1, 2                                        # the bits of a verdict and of a class byte
# SLG_ISECT_STAT_*: indices into the header's stats, in the names of mesh.self_intersections' dict
ISECT_STATS = ("adjacent_pairs", "tested_pairs", "intersecting_pairs", "uncertain_pairs", "intersecting_triangles",
               "uncertain_triangles")
AUDIT_WS_AUDIT, AUDIT_WS_MEASURE, AUDIT_WS_SELECT = range(3)                      # SLG_AUDIT_WS_*
AUDIT_CHUNK = 2048                                                                # SLG_AUDIT_CHUNK
# SLG_AUDIT_STAT_*: indices into the audit header's stats, in the names of mesh.audit's dict
AUDIT_STATS = ("edges", "boundary_edges", "manifold_edges", "nonmanifold_edges", "inconsistent_edges",
               "degenerate_triangles", "duplicate_triangles", "nonmanifold_vertices")
# SLG_AUDIT_VERTEX_* and SLG_AUDIT_TRIANGLE_*: the bits of vertex_class and triangle_class
(AUDIT_VERTEX_REFERENCED, AUDIT_VERTEX_BOUNDARY, AUDIT_VERTEX_NONMANIFOLD_EDGE, AUDIT_VERTEX_INCONSISTENT,
 AUDIT_VERTEX_NONMANIFOLD) = 1, 2, 4, 8, 16
AUDIT_TRIANGLE_DEGENERATE, AUDIT_TRIANGLE_DUPLICATE = 1, 2
BAND_MIN_DEPTH, BAND_MAX_DEPTH, BAND_MAX_BASE_DEPTH, BAND_BLOCK = 3, 12, 10, 8     # SLG_BAND_*
BAND_WS_BLOCKS, BAND_WS_SPLAT, BAND_WS_ISO, BAND_WS_EXTRACT = range(4)            # SLG_BAND_WS_*
# SLG_BAND_STAT_*: indices into a level header's stats
BAND_STATS = ("seeded_blocks", "active_blocks", "node_blocks", "band_nodes", "interior_nodes")
SURFACE_WS_GRID, SURFACE_WS_PASS = 0, 1          # SLG_SURFACE_WS_*
SURFACE_MAX_NEIGHBOURS, SURFACE_MAX_RADII = 512, 8   # SLG_SURFACE_MAX_NEIGHBOURS, SLG_SURFACE_MAX_RADII
FILTER_BAD_NEIGHBOURS = 8                        # SLG_FILTER_BAD_NEIGHBOURS (slgpu_surface.h)
MESH_HDR_BYTES, MESH_MAX_DEPTH = 256, 10        # SLG_MESH_HDR_BYTES; kMaxDepth of csrc/cloud_mesh.hip
# SLG_MESH_WS_*: the stages of slg_mesh_ws_bytes
(MESH_WS_GRID, MESH_WS_SPLAT, MESH_WS_SOLVE, MESH_WS_ISO, MESH_WS_EXTRACT, MESH_WS_QUANTILE, MESH_WS_REMOVE,
 MESH_WS_ALL) = range(8)
MESH_WS_ADJACENCY, MESH_WS_HOLES = 8, 9          # the stages of slg_mesh_post_ws_bytes (csrc/cloud_meshpost.hip)
MESH_SMOOTH_LAPLACIAN, MESH_SMOOTH_STEP = 0, 1   # SLG_MESH_SMOOTH_*
MESH_HOLES_MAX_SIZE = 64                         # SLG_MESH_HOLES_MAX_SIZE
# SLG_MESH_HOLES_STAT_*: indices into the header's stats after slg_mesh_holes_count
(MESH_HOLES_STAT_EDGES, MESH_HOLES_STAT_LOOPS, MESH_HOLES_STAT_CLOSABLE_EDGES, MESH_HOLES_STAT_LONG_EDGES,
 MESH_HOLES_STAT_BLOCKED_EDGES) = range(5)
MESH_DECIMATE_SWEEPS = 4                         # SLG_MESH_DECIMATE_SWEEPS
# SLG_MESH_DECIMATE_STAT_*: the last round's counts in the header's stats (csrc/cloud_decimate.hip)
MESH_DECIMATE_STATS = ("boundary", "nonmanifold", "link", "valence", "flip", "nan", "valid", "selected")
ORIENT_MAX_K, ORIENT_STATS_LEN = 128, 128        # SLG_ORIENT_MAX_K, SLG_ORIENT_STATS_LEN
# SLG_ORIENT_STAT_*: indices into the stats of slg_emst / slg_orient_tangent
(ORIENT_STAT_EMST_ROUNDS, ORIENT_STAT_TREE_ROUNDS, ORIENT_STAT_LIST_FAR, ORIENT_STAT_WALKED, ORIENT_STAT_FAR,
 ORIENT_STAT_SAT_OUT) = range(6)
ORIENT_STAT_ROUND_WALKED, ORIENT_STAT_ROUND_FAR, ORIENT_STAT_ROUND_SAT_OUT = 16, 48, 80
PLANE_MAX_BATCH, PLANE_RECORD_STRIDE, PLANE_SUMS_LEN, PLANE_MAX_RANSAC_N = 4096, 16, 16, 8
FILTER_BAD_NONFINITE, FILTER_BAD_EXTENT, FILTER_BAD_INDEX = 1, 2, 4
FPFH_DIM, FPFH_MAX_NN = 33, 128                  # SLG_FPFH_DIM, SLG_FPFH_MAX_NN
RANSAC_MAX_BATCH, RANSAC_TRIAL_STRIDE, RANSAC_RECORD_STRIDE = 16384, 20, 32
RANSAC_EDGE_OK, RANSAC_DISTANCE_OK = 1, 2
ICP_RESULT_LEN, ICP_LOG_STRIDE = 24, 56          # SLG_ICP_RESULT_LEN, SLG_ICP_LOG_STRIDE
ICP_LOG_STOP, ICP_LOG_SOLVED, ICP_LOG_SINGULAR, ICP_LOG_LAST = 1, 2, 4, 8
GATHER_ID_BYTES = 128


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"slgpu error {code}: {msg}")
        self.code = code
        self.msg = msg


_lib = None
_lib_lock = threading.Lock()


def lib():
    """Load (once) and return the native library; raises if it was not built.  Threads that make
    the first call together load it once: the handle is published only after its prototypes and
    its provenance are set."""
    global _lib
    if _lib is None:
        with _lib_lock:
            if _lib is None:
                _lib = _load()
    return _lib


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; "
                          f"g.build()'` (hipcc --offload-arch=gfx950) first")
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        if AB_LIB is not None and not hasattr(h, name):
            continue                     # an A/B build from an older tree (tools/ab.py)
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = args
    # The second to fifth tables: the digest check below vouches that the product library is the build of
    # sources that hold them (tests/test_surface_host.py, test_band_host.py, test_audit_host.py and test_intersect_host.py look every name up).  A handle without a
    # name gets no prototype, and the first call of that name raises ctypes' AttributeError.
    for name, (res, args) in (*SURFACE_EXPORTS.items(), *BAND_EXPORTS.items(), *AUDIT_EXPORTS.items(),
                              *INTERSECT_EXPORTS.items()):
        if hasattr(h, name):
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
    if h.slg_version() != ABI_VERSION:
        raise ImportError("libslgpu ABI version mismatch")
    if AB_LIB is None:
        # provenance: the product library must be the build of the sources beside it
        from . import build as B
        built, want = h.slg_build_id().decode(), B.BUILD_ID_PREFIX.decode() + B.source_digest()
        if built != want:
            raise ImportError(f"{LIB_PATH} was built from other sources ({built}, sources {want}): "
                              "rebuild it (__graft_entry__.build())")
    return h


def kernel_table() -> dict:
    """``{symbol: present}`` of the fused kernel's instance table (``slg_kernel_table``)."""
    buf = ctypes.create_string_buffer(1 << 16)
    lib().slg_kernel_table(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, flag = line.split("\t")
        out[name] = flag == "1"
    return out


def last_kernel() -> str:
    """Symbol of the fused kernel instance this thread's last fused launch picked
    (``slg_last_kernel``; "" when none)."""
    buf = ctypes.create_string_buffer(512)
    check(lib().slg_last_kernel(buf, len(buf)))
    return buf.value.decode()


def check(rc: int):
    if rc != SLG_OK:
        msg = lib().slg_last_error().decode(errors="replace")
        if rc == SLG_ERR_NOT_ENOUGH:
            raise ValueError(msg)
        if rc == SLG_ERR_INDEX:
            raise IndexError(msg)
        raise NativeError(rc, msg)


def loaded_hip_runtimes() -> list[str]:
    """Paths of every libamdhip64 mapped into this process (must be exactly one)."""
    out = set()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                out.add(line.split()[-1])
    return sorted(out)
