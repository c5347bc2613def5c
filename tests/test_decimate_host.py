"""Host side of the device mesh decimation (no GPU needed): the exports and their ctypes
signatures, the macros, the library's refusals, and the argument errors of mesh.decimate_quadric,
mesh.check_postprocess and ProcessingLogic.reconstruct_stl, all raised before anything touches a
device."""
import os
import re

import numpy as np
import pytest

from test_icp_host import ROOT, prototype

NAMES = (("slg_mesh_decimate_ws_bytes", 2), ("slg_mesh_decimate_init", 7), ("slg_mesh_decimate_round", 7),
         ("slg_mesh_decimate_emit", 11))


def test_exports_and_signatures():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    for name, n_args in NAMES:
        res, args = N.EXPORTS[name]
        c_res, c_args = prototype(name)
        assert len(args) == n_args and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res]
    txt = open(os.path.join(ROOT, "include", "slgpu.h")).read()
    assert re.search(rf"#define SLG_MESH_DECIMATE_SWEEPS {N.MESH_DECIMATE_SWEEPS}\b", txt)
    for i, name in enumerate(N.MESH_DECIMATE_STATS):
        assert re.search(rf"#define SLG_MESH_DECIMATE_STAT_{name.upper()} {i}\b", txt), name
    assert MS.DECIMATE_SWEEPS == N.MESH_DECIMATE_SWEEPS == 4
    import decimate_ref as R
    assert R.SWEEPS == MS.DECIMATE_SWEEPS and R.STATS == N.MESH_DECIMATE_STATS
    assert MS._DEC_HDR.fields["stats"][1] == 128 and MS._DEC_HDR.itemsize <= N.MESH_HDR_BYTES


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_decimate.hip")) for p in B.SRCS)
    assert os.path.join(B.CSRC, "mesh_keys.h") in B.digest_files()
    lib = N.lib()
    for name, _ in NAMES:
        assert hasattr(lib, name)
    bad = -N.SLG_ERR_INVALID
    assert lib.slg_mesh_decimate_ws_bytes(0, 8) == bad and lib.slg_mesh_decimate_ws_bytes(8, 0) == bad
    assert lib.slg_mesh_decimate_ws_bytes(1 << 31, 8) == bad
    assert lib.slg_mesh_decimate_ws_bytes(8, (1 << 30) // 3 + 1) == bad
    assert lib.slg_mesh_decimate_ws_bytes(8, (1 << 30) // 3) > 0
    need = lib.slg_mesh_decimate_ws_bytes(8, 8)
    inv = N.SLG_ERR_INVALID
    fake = 1 << 20                                                    # aligned, never dereferenced: every call refuses first
    assert lib.slg_mesh_decimate_init(None, 8, None, 8, None, 0, None) == inv
    assert lib.slg_mesh_decimate_init(fake, 8, fake, 8, None, need, None) == inv        # no workspace
    assert lib.slg_mesh_decimate_init(fake, 8, fake, 8, fake, need - 1, None) == inv    # a short one
    assert lib.slg_mesh_decimate_init(fake, 8, fake, 8, fake + 8, need, None) == inv    # a misaligned one
    assert lib.slg_mesh_decimate_init(fake, 0, fake, 8, fake, need, None) == inv
    assert lib.slg_mesh_decimate_round(None, 0, 8, 8, 8, 4, None) == inv
    assert lib.slg_mesh_decimate_round(fake, need - 1, 8, 8, 8, 4, None) == inv
    assert lib.slg_mesh_decimate_round(fake, need, 8, 8, 9, 4, None) == inv             # more alive than there are
    assert lib.slg_mesh_decimate_round(fake, need, 8, 8, 0, 0, None) == inv
    assert lib.slg_mesh_decimate_round(fake, need, 8, 8, 8, -1, None) == inv
    assert lib.slg_mesh_decimate_round(fake, need, 8, 8, 8, 8, None) == inv             # the target is reached already
    assert lib.slg_mesh_decimate_emit(None, 0, 8, 8, None, None, None, 8, None, 8, None) == inv
    assert lib.slg_mesh_decimate_emit(fake, need - 1, 8, 8, None, fake, None, 8, fake, 8, None) == inv
    assert lib.slg_mesh_decimate_emit(fake, need, 8, 8, None, None, None, 8, fake, 8, None) == inv
    assert lib.slg_mesh_decimate_emit(fake, need, 8, 8, None, fake, None, 9, fake, 8, None) == inv
    assert lib.slg_mesh_decimate_emit(fake, need, 8, 8, None, fake, None, 8, fake, 9, None) == inv
    assert lib.slg_mesh_decimate_emit(fake, need, 8, 8, fake, fake, None, 8, fake, 8, None) == inv   # densities in, none out


def test_workspace_bytes():
    """The state (13 doubles per vertex and the triangles twice) and a round's scratch, which grows
    with the triangle count: 50 arrays' worth, the largest the sort's bound of 12 * 6 T bytes."""
    from structured_light_for_3d_model_replication_amd import _native as N
    lib = N.lib()
    sizes = [lib.slg_mesh_decimate_ws_bytes(1000, t) for t in (1, 100, 10_000, 1_000_000)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.slg_mesh_decimate_ws_bytes(1_000_000, 100) > lib.slg_mesh_decimate_ws_bytes(1000, 100)
    V, T = 500_000, 1_000_000
    need = lib.slg_mesh_decimate_ws_bytes(V, T)
    assert need >= 13 * 8 * V + 2 * 12 * T + 12 * 6 * T and need < 1000 * T
    assert need % 256 == 0


def test_decimate_arguments():
    """Argument errors come before the mesh is looked at, so plain arrays do here."""
    from structured_light_for_3d_model_replication_amd import mesh as MS
    mesh = MS.TriangleMesh(np.zeros((4, 3)), np.zeros((2, 3), np.int32))
    for target in (-1, 1.5, float("nan"), float("inf"), "many", None, True):
        with pytest.raises(ValueError, match="target_faces"):
            MS.decimate_quadric(mesh, target)
    for rounds in (-1, 2.5):
        with pytest.raises(ValueError, match="max_rounds"):
            MS.decimate_quadric(mesh, 10, max_rounds=rounds)
    for target in (0, 10, 10.0, np.int64(3)):
        with pytest.raises(ValueError, match="device float64"):      # then the mesh
            MS.decimate_quadric(mesh, target)
    assert MS.check_target_faces(50000.0) == 50000 and MS.DEFAULT_TARGET_FACES == 50000


def test_check_postprocess():
    from structured_light_for_3d_model_replication_amd import mesh as MS
    mesh = MS.TriangleMesh(np.zeros((4, 3)), np.zeros((2, 3), np.int32))
    MS.check_postprocess({"simplify": True, "simplify_rule": "rounds"})
    MS.check_postprocess({"simplify": True, "simplify_rule": "rounds", "target_faces": 1000})
    MS.check_postprocess({"simplify": False, "simplify_rule": "queue", "target_faces": -5})     # not asked for: not looked at
    for rule in ("queue", "Rounds", "", 0, True):
        with pytest.raises(ValueError, match="simplify_rule"):
            MS.check_postprocess({"simplify": True, "simplify_rule": rule})
    for target in (-1, 0.5, "x"):
        with pytest.raises(ValueError, match="target_faces"):
            MS.check_postprocess({"simplify": True, "simplify_rule": "rounds", "target_faces": target})
        with pytest.raises(ValueError, match="target_faces"):
            MS.postprocess(mesh, {"simplify": True, "simplify_rule": "rounds", "target_faces": target})
    with pytest.raises(NotImplementedError, match=r"simplify.*server/processing.py:778-781"):   # as before
        MS.check_postprocess({"simplify": True})
    with pytest.raises(NotImplementedError, match="reference"):
        MS.postprocess(mesh, {"simplify": True, "target_faces": 1000})
    with pytest.raises(ValueError, match="device float64"):          # every key accepted: then the mesh
        MS.postprocess(mesh, {"smooth_iters": 0, "simplify": True, "simplify_rule": "rounds"})


def test_processing_arguments(tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    open(src, "w").write("ply\n")
    dev = {"enabled": True, "backend": "device", "simplify": True}
    with pytest.raises(NotImplementedError, match=r"simplify.*server/processing.py:778-781"):
        PL.reconstruct_stl(src, out, params={"depth": 5}, meshlab_params=dev)
    with pytest.raises(ValueError, match="simplify_rule"):
        PL.reconstruct_stl(src, out, params={"depth": 5}, meshlab_params={**dev, "simplify_rule": "queue"})
    with pytest.raises(ValueError, match="target_faces"):
        PL.reconstruct_stl(src, out, params={"depth": 5}, meshlab_params={**dev, "simplify_rule": "rounds", "target_faces": -3})
    assert not os.path.exists(out)                                    # nothing was loaded or written
