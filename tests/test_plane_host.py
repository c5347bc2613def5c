"""Host side of the device plane segmentation (no GPU needed): the exports and their ctypes
signatures, the refusals that never reach the device, and the argument errors raised in Python."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_icp_host import ROOT, prototype

NAMES = (("slg_plane_ws_bytes", 2), ("slg_plane_batch", 11), ("slg_plane_finish", 11))


def test_exports_and_signatures():
    from structured_light_for_3d_model_replication_amd import _native as N
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr", ctypes.POINTER(N.c_dbl): "ptr"}
    for name, n_args in NAMES:
        res, args = N.EXPORTS[name]
        c_res, c_args = prototype(name)
        assert len(args) == n_args and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res]
    txt = open(os.path.join(ROOT, "include", "slgpu.h")).read()
    for macro, value in (("SLG_PLANE_MAX_BATCH", N.PLANE_MAX_BATCH), ("SLG_PLANE_RECORD_STRIDE", N.PLANE_RECORD_STRIDE),
                         ("SLG_PLANE_SUMS_LEN", N.PLANE_SUMS_LEN), ("SLG_PLANE_MAX_RANSAC_N", N.PLANE_MAX_RANSAC_N)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    import plane_ref as R
    from structured_light_for_3d_model_replication_amd import cloud as CL
    assert (R.RECORD_STRIDE, R.SUMS_LEN, R.MAX_N, R.BATCH, R.PROBABILITY) == \
        (N.PLANE_RECORD_STRIDE, N.PLANE_SUMS_LEN, N.PLANE_MAX_RANSAC_N, CL.PLANE_BATCH, CL.PLANE_PROBABILITY)
    assert CL.PLANE_BATCH % 64 == 0 and CL.PLANE_BATCH < N.PLANE_MAX_BATCH
    src = open(os.path.join(ROOT, "structured_light_for_3d_model_replication_amd", "csrc", "cloud_grid.h")).read()
    assert re.search(rf"kChunk = {R.CHUNK};", src)


def test_source_is_in_the_build_list_and_the_library_exports_it():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_plane.hip")) for p in B.SRCS)
    lib = N.lib()
    for name, _ in NAMES:
        assert hasattr(lib, name)
    assert lib.slg_plane_ws_bytes(0, 64) == -N.SLG_ERR_INVALID               # no device needed for the refusals
    assert lib.slg_plane_ws_bytes(8, 0) == -N.SLG_ERR_INVALID
    assert lib.slg_plane_ws_bytes(8, N.PLANE_MAX_BATCH + 1) == -N.SLG_ERR_UNSUPPORTED
    assert lib.slg_plane_ws_bytes((1 << 30) + 1, 64) == -N.SLG_ERR_UNSUPPORTED
    assert lib.slg_plane_batch(None, 8, 1.0, 3, 0, 0, 64, None, 0, None, None) == N.SLG_ERR_INVALID
    assert lib.slg_plane_finish(None, 8, None, 1.0, None, 0, None, None, None, None, None) == N.SLG_ERR_INVALID
    # with buffers that look valid: the arguments are still refused before anything is launched
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15), ctypes.c_void_p)
    for n, thr, rn, t0, batch, want in ((8, 1.0, 2, 0, 64, N.SLG_ERR_INVALID), (8, 0.0, 3, 0, 64, N.SLG_ERR_INVALID),
                                        (8, float("inf"), 3, 0, 64, N.SLG_ERR_INVALID), (8, 1.0, 3, -1, 64, N.SLG_ERR_INVALID),
                                        (2, 1.0, 3, 0, 64, N.SLG_ERR_INVALID), (8, 1.0, 9, 0, 64, N.SLG_ERR_UNSUPPORTED),
                                        (8, 1.0, 3, 0, N.PLANE_MAX_BATCH + 1, N.SLG_ERR_UNSUPPORTED),
                                        ((1 << 30) + 1, 1.0, 3, 0, 64, N.SLG_ERR_UNSUPPORTED)):
        assert lib.slg_plane_batch(p, n, thr, rn, 0, t0, batch, None, 0, p, None) == want, (n, thr, rn, t0, batch)
    assert lib.slg_plane_batch(ctypes.c_void_p(p.value + 8), 8, 1.0, 3, 0, 0, 64, None, 0, p, None) == N.SLG_ERR_INVALID   # alignment
    plane = (ctypes.c_double * 4)(0.0, 0.0, float("nan"), 0.0)
    assert lib.slg_plane_finish(p, 8, plane, 1.0, None, 0, p, p, p, p, None) == N.SLG_ERR_INVALID


def test_errors_raised_without_a_device(monkeypatch):
    import torch
    from structured_light_for_3d_model_replication_amd import cloud as CL
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic

    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(CL, "plane_batch", no_device)
    monkeypatch.setattr(CL, "plane_finish", no_device)
    empty = CL.PointCloud(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="Point cloud is empty."):
        CL.segment_plane(empty, 1.0)
    with pytest.raises(ValueError, match="Point cloud is empty."):
        ProcessingLogic.remove_background(empty)
    cpu = torch.device("cpu")
    pc = CL.PointCloud(np.arange(15.0).reshape(5, 3) ** 2, device=cpu)
    with pytest.raises(ValueError, match="fewer points than ransac_n"):
        CL.segment_plane(pc, 1.0, ransac_n=6)
    with pytest.raises(ValueError, match="ransac_n must be >= 3"):
        CL.segment_plane(pc, 1.0, ransac_n=2)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="distance_threshold must be finite and > 0"):
            CL.segment_plane(pc, thr)
    with pytest.raises(ValueError, match="num_iterations must be >= 0"):
        CL.segment_plane(pc, 1.0, num_iterations=-1)
    for pr in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"probability must lie in \(0, 1\]"):
            CL.segment_plane(pc, 1.0, probability=pr)
    with pytest.raises(FileNotFoundError, match="Input file not found"):
        ProcessingLogic.remove_background("/nonexistent/cloud.ply")
    import inspect
    sig = inspect.signature(ProcessingLogic.remove_background)
    assert [(p.name, p.default) for p in sig.parameters.values()] == \
        [("input_data", inspect.Parameter.empty), ("output_path", None), ("distance_threshold", 50), ("ransac_n", 3),
         ("num_iterations", 1000), ("return_obj", False), ("seed", 0)]
    sig = inspect.signature(CL.segment_plane)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("distance_threshold", inspect.Parameter.empty), ("ransac_n", 3), ("num_iterations", 100),
         ("probability", 0.99999999), ("seed", 0), ("stream", None)]
