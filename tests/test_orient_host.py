"""Host side of the device tangent-plane orientation (no GPU needed): the exports and their ctypes
signatures, the refusals that never reach the device, and the argument errors raised in Python."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from test_icp_host import ROOT, prototype

NAMES = (("slg_orient_ws_bytes", 2), ("slg_knn_lists", 8), ("slg_emst", 8), ("slg_orient_tangent", 12))


def test_exports_and_signatures():
    from structured_light_for_3d_model_replication_amd import _native as N
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    for name, n_args in NAMES:
        res, args = N.EXPORTS[name]
        c_res, c_args = prototype(name)
        assert len(args) == n_args and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res]
    txt = open(os.path.join(ROOT, "include", "slgpu.h")).read()
    for macro, value in (("SLG_ORIENT_MAX_K", N.ORIENT_MAX_K), ("SLG_ORIENT_STATS_LEN", N.ORIENT_STATS_LEN),
                         ("SLG_ORIENT_STAT_EMST_ROUNDS", N.ORIENT_STAT_EMST_ROUNDS),
                         ("SLG_ORIENT_STAT_TREE_ROUNDS", N.ORIENT_STAT_TREE_ROUNDS),
                         ("SLG_ORIENT_STAT_LIST_FAR", N.ORIENT_STAT_LIST_FAR),
                         ("SLG_ORIENT_STAT_WALKED", N.ORIENT_STAT_WALKED), ("SLG_ORIENT_STAT_FAR", N.ORIENT_STAT_FAR),
                         ("SLG_ORIENT_STAT_SAT_OUT", N.ORIENT_STAT_SAT_OUT),
                         ("SLG_ORIENT_STAT_ROUND_WALKED", N.ORIENT_STAT_ROUND_WALKED),
                         ("SLG_ORIENT_STAT_ROUND_FAR", N.ORIENT_STAT_ROUND_FAR),
                         ("SLG_ORIENT_STAT_ROUND_SAT_OUT", N.ORIENT_STAT_ROUND_SAT_OUT)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    assert N.ORIENT_MAX_K >= 100                                   # the reference's default k


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_orient.hip")) for p in B.SRCS)
    lib = N.lib()
    for name, _ in NAMES:
        assert hasattr(lib, name)
    assert lib.slg_orient_ws_bytes(0, 30) == -N.SLG_ERR_INVALID               # no device needed for the refusals
    assert lib.slg_orient_ws_bytes(8, 0) == -N.SLG_ERR_INVALID
    assert lib.slg_orient_ws_bytes(8, N.ORIENT_MAX_K + 1) == -N.SLG_ERR_UNSUPPORTED
    assert lib.slg_orient_ws_bytes((1 << 30) + 1, 30) == -N.SLG_ERR_UNSUPPORTED
    assert lib.slg_orient_ws_bytes(1 << 31, 30) == -N.SLG_ERR_UNSUPPORTED
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    # slg_knn_lists(xyz, n, k, ws, ws_bytes, idx_out, d2_out, stream)
    assert lib.slg_knn_lists(None, 8, 5, None, 0, p, p, None) == N.SLG_ERR_INVALID
    assert lib.slg_knn_lists(odd, 8, 5, None, 0, p, p, None) == N.SLG_ERR_INVALID      # alignment
    assert lib.slg_knn_lists(p, 0, 5, None, 0, p, p, None) == N.SLG_ERR_INVALID
    assert lib.slg_knn_lists(p, 8, 0, None, 0, p, p, None) == N.SLG_ERR_INVALID
    assert lib.slg_knn_lists(p, 8, 5, None, 0, None, p, None) == N.SLG_ERR_INVALID
    assert lib.slg_knn_lists(p, 8, N.ORIENT_MAX_K + 1, None, 0, p, p, None) == N.SLG_ERR_UNSUPPORTED
    assert lib.slg_knn_lists(p, 1 << 31, 5, None, 0, p, p, None) == N.SLG_ERR_UNSUPPORTED
    # slg_emst(xyz, n, k, ws, ws_bytes, edges_out, stats_out, stream)
    assert lib.slg_emst(None, 8, 5, None, 0, p, None, None) == N.SLG_ERR_INVALID
    assert lib.slg_emst(p, 8, -1, None, 0, p, None, None) == N.SLG_ERR_INVALID
    assert lib.slg_emst(p, 8, 5, None, 0, None, None, None) == N.SLG_ERR_INVALID
    assert lib.slg_emst(p, 8, N.ORIENT_MAX_K + 1, None, 0, p, None, None) == N.SLG_ERR_UNSUPPORTED
    assert lib.slg_emst(p, (1 << 30) + 1, 5, None, 0, p, None, None) == N.SLG_ERR_UNSUPPORTED
    # slg_orient_tangent(xyz, normals, n, k, ws, ws_bytes, normals_out, emst_out, tree_out, root_out, stats_out, stream)
    q = ctypes.c_void_p(p.value + 128)
    tail = (None, None, None, None, None)
    assert lib.slg_orient_tangent(None, p, 8, 5, None, 0, q, *tail) == N.SLG_ERR_INVALID
    assert lib.slg_orient_tangent(p, None, 8, 5, None, 0, q, *tail) == N.SLG_ERR_INVALID      # no normals
    assert lib.slg_orient_tangent(p, p, 8, 5, None, 0, None, *tail) == N.SLG_ERR_INVALID
    assert lib.slg_orient_tangent(p, p, 8, 5, None, 0, p, *tail) == N.SLG_ERR_INVALID         # in place
    assert lib.slg_orient_tangent(p, odd, 8, 5, None, 0, q, *tail) == N.SLG_ERR_INVALID
    assert lib.slg_orient_tangent(p, p, 0, 5, None, 0, q, *tail) == N.SLG_ERR_INVALID
    assert lib.slg_orient_tangent(p, p, 8, 0, None, 0, q, *tail) == N.SLG_ERR_INVALID
    assert lib.slg_orient_tangent(p, p, 8, N.ORIENT_MAX_K + 1, None, 0, q, *tail) == N.SLG_ERR_UNSUPPORTED
    assert lib.slg_orient_tangent(p, p, 1 << 31, 5, None, 0, q, *tail) == N.SLG_ERR_UNSUPPORTED


def test_errors_raised_without_a_device(monkeypatch):
    import torch
    from structured_light_for_3d_model_replication_amd import cloud as CL
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic

    empty = CL.PointCloud(np.zeros((0, 3)))
    for fn in (lambda: CL.knn_lists(empty, 5), lambda: CL.euclidean_mst(empty),
               lambda: CL.orient_normals_consistent_tangent_plane(empty, 5),
               lambda: ProcessingLogic.estimate_oriented_normals(empty, orientation_mode="tangent")):
        with pytest.raises(ValueError, match="Point cloud is empty."):
            fn()
    assert CL.nearest_neighbor_distance(empty).shape == (0,)
    cpu = torch.device("cpu")
    pc = CL.PointCloud(np.arange(15.0).reshape(5, 3) ** 2, device=cpu)
    assert CL.nearest_neighbor_distance(CL.PointCloud(np.ones((1, 3)), device=cpu)).tolist() == [0.0]
    with pytest.raises(RuntimeError, match="has no normals"):
        CL.orient_normals_consistent_tangent_plane(pc, 30)
    with_normals = CL.PointCloud(pc.xyz, normals=np.ones((5, 3)), device=cpu)
    for k in (0, -3):
        with pytest.raises(ValueError, match="k must be >= 1"):
            CL.orient_normals_consistent_tangent_plane(with_normals, k)
        with pytest.raises(ValueError, match="k must be >= 1"):
            CL.knn_lists(pc, k)

    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(CL, "estimate_normals", no_device)
    with pytest.raises(ValueError, match="orientation_mode must be 'radial' or 'tangent'"):
        ProcessingLogic.estimate_oriented_normals(pc, orientation_mode="graph")
    with pytest.raises(ValueError, match="tangent_k must be >= 1"):
        ProcessingLogic.estimate_oriented_normals(pc, orientation_mode="tangent", tangent_k=0)
    with pytest.raises(FileNotFoundError):
        ProcessingLogic.estimate_oriented_normals("/nonexistent/cloud.ply", orientation_mode="tangent")
    sig = inspect.signature(ProcessingLogic.estimate_oriented_normals)
    assert [(p.name, p.default) for p in sig.parameters.values()] == \
        [("input_data", inspect.Parameter.empty), ("save_normals_path", None), ("normal_radius", 0.1),
         ("normal_max_nn", 30), ("outward", True), ("return_obj", False), ("orientation_mode", "radial"),
         ("tangent_k", 100), ("consistency_pass", False), ("consistency_k", 30)]
    sig = inspect.signature(CL.orient_normals_consistent_tangent_plane)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("k", inspect.Parameter.empty), ("return_tree", False), ("stream", None)]
