"""Host side of the device mesher (no GPU needed): the exports and their ctypes signatures, the
workspace formula, and the argument errors of mesh.py and of ProcessingLogic.mesh_360 /
reconstruct_stl, all raised before anything touches a device."""
import os
import re

import numpy as np
import pytest

from test_icp_host import ROOT, prototype

NAMES = (("slg_mesh_ws_bytes", 4), ("slg_mesh_set_header", 6), ("slg_mesh_grid", 7), ("slg_mesh_splat", 9),
         ("slg_mesh_divergence", 5), ("slg_mesh_solve", 7), ("slg_mesh_sample", 6), ("slg_mesh_iso", 6),
         ("slg_mesh_count", 5), ("slg_mesh_emit", 11), ("slg_mesh_quantile", 6), ("slg_mesh_remove", 12),
         ("slg_mesh_triangle_normals", 5), ("slg_mesh_stl_pack", 6))


def test_exports_and_signatures():
    import ctypes
    from structured_light_for_3d_model_replication_amd import _native as N
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr", ctypes.POINTER(N.c_dbl): "ptr"}
    for name, n_args in NAMES:
        res, args = N.EXPORTS[name]
        c_res, c_args = prototype(name)
        assert len(args) == n_args and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res]
    txt = open(os.path.join(ROOT, "include", "slgpu.h")).read()
    for macro, value in (("SLG_MESH_HDR_BYTES", N.MESH_HDR_BYTES), ("SLG_MESH_WS_GRID", N.MESH_WS_GRID),
                         ("SLG_MESH_WS_SPLAT", N.MESH_WS_SPLAT), ("SLG_MESH_WS_SOLVE", N.MESH_WS_SOLVE),
                         ("SLG_MESH_WS_ISO", N.MESH_WS_ISO), ("SLG_MESH_WS_EXTRACT", N.MESH_WS_EXTRACT),
                         ("SLG_MESH_WS_QUANTILE", N.MESH_WS_QUANTILE), ("SLG_MESH_WS_REMOVE", N.MESH_WS_REMOVE),
                         ("SLG_MESH_WS_ALL", N.MESH_WS_ALL)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_mesh.hip")) for p in B.SRCS)
    lib = N.lib()
    for name, _ in NAMES:
        assert hasattr(lib, name)
    assert lib.slg_mesh_ws_bytes(N.MESH_WS_ALL, 2048, 0, 0) == -N.SLG_ERR_INVALID
    assert lib.slg_mesh_ws_bytes(99, 16, 0, 0) == -N.SLG_ERR_INVALID
    assert lib.slg_mesh_ws_bytes(N.MESH_WS_SPLAT, 16, (1 << 30) + 1, 0) == -N.SLG_ERR_UNSUPPORTED
    assert lib.slg_mesh_grid(None, 8, 5, 1.1, None, 0, None) == N.SLG_ERR_INVALID
    assert lib.slg_mesh_solve(None, 16, 1, None, 0, None, None) == N.SLG_ERR_INVALID
    assert lib.slg_mesh_count(None, 16, None, 0, None) == N.SLG_ERR_INVALID
    assert lib.slg_mesh_quantile(None, 0, 0.5, None, 0, None) == N.SLG_ERR_INVALID


def test_workspace_bytes():
    """48 (R+1)^3 for W, V, f, chi plus the largest stage: the extraction's masks, counts and 64-bit
    bases (about 18 bytes per node)."""
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    sizes = [MS.workspace_bytes(d) for d in range(2, 11)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] < 288e9 and MS.workspace_bytes(10, 2_000_000) < 288e9
    assert MS.workspace_bytes(8, 1_000_000) >= MS.workspace_bytes(8)
    lib = N.lib()
    for d in (2, 6, 10):
        R = 1 << d
        stages = [lib.slg_mesh_ws_bytes(s, R, 1, 0) for s in range(N.MESH_WS_GRID, N.MESH_WS_EXTRACT + 1)]
        assert MS.workspace_bytes(d) == 48 * (R + 1) ** 3 + max(stages)
        M, C = (R + 1) ** 3, R ** 3
        assert 9 * M + 9 * C <= stages[N.MESH_WS_EXTRACT] <= 9 * M + 9 * C + M // 4 + (1 << 20) + 6 * 256 + 256
    for bad in (1, 11, 16, 17):
        with pytest.raises(ValueError):
            MS.workspace_bytes(bad)


def test_mesh_arguments():
    from structured_light_for_3d_model_replication_amd import mesh as MS
    cloud = (np.zeros((4, 3)), np.zeros((4, 3), np.uint8))
    for depth in (1, 0, -3, 11, 16):
        with pytest.raises(ValueError, match="depth"):
            MS.poisson_grid(cloud, depth=depth)
    with pytest.raises(ValueError, match="dense grid's limit of 10"):
        MS.poisson_grid(cloud, depth=12)
    for scale in (0.99, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            MS.poisson_grid(cloud, depth=5, scale=scale)
    with pytest.raises(ValueError, match="cycles"):
        MS.poisson_grid(cloud, depth=5, cycles=-1)
    with pytest.raises(ValueError):
        MS.solve_poisson(np.zeros((5, 5, 5)), 1.0)                 # not a device tensor
    with pytest.raises(ValueError):
        MS.extract_isosurface(np.zeros((5, 5, 5)), 0.0, (0, 0, 0), 1.0)
    with pytest.raises(ValueError):
        MS.quantile(np.zeros(5), 0.5)
    with pytest.raises(ValueError, match="stl"):
        MS.check_stl_path("mesh.obj")
    MS.check_stl_path("mesh.STL")


def test_processing_arguments(tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    with pytest.raises(FileNotFoundError):
        PL.mesh_360(src, out)
    with pytest.raises(FileNotFoundError):
        PL.reconstruct_stl(src, out)
    open(src, "w").write("ply\n")
    with pytest.raises(ValueError, match="width"):
        PL.mesh_360(src, out, depth=5, width=0.5)
    with pytest.raises(ValueError, match="linear_fit"):
        PL.mesh_360(src, out, depth=5, linear_fit=True)
    with pytest.raises(ValueError, match="too high"):
        PL.mesh_360(src, out, depth=17)
    with pytest.raises(ValueError, match="dense grid's limit"):
        PL.mesh_360(src, out, depth=11)
    with pytest.raises(ValueError, match="scale"):
        PL.mesh_360(src, out, depth=5, scale=0.5)
    with pytest.raises(ValueError, match="stl"):
        PL.mesh_360(src, str(tmp_path / "mesh.ply"), depth=5)
    with pytest.raises(NotImplementedError, match="reference"):
        PL.reconstruct_stl(src, out, mode="surface")
    with pytest.raises(ValueError, match="Unknown mode"):
        PL.reconstruct_stl(src, out, mode="other")
    with pytest.raises(ValueError, match="too high"):
        PL.reconstruct_stl(src, out, params={"depth": 17})
    with pytest.raises(ValueError, match="dense grid's limit"):
        PL.reconstruct_stl(src, out, params={"depth": 16})
