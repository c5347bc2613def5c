"""Host side of the device surface mesher (no GPU needed): the second export table and its ctypes
signatures against include/slgpu_surface.h, the macros, the build list and the digest, the
library's refusals, and the argument errors of mesh.check_radii, mesh.ball_pivot and
ProcessingLogic.reconstruct_stl(mode="surface"), all raised before anything touches a device."""
import os
import re

import numpy as np
import pytest

from test_icp_host import ROOT

HEADER = os.path.join(ROOT, "include", "slgpu_surface.h")
N_ARGS = {"slg_surface_ws_bytes": 4, "slg_surface_begin": 6, "slg_surface_count": 8, "slg_surface_emit": 12,
          "slg_surface_round": 6, "slg_surface_commit": 11}


def declarations():
    """``{name: (result, [i32 / i64 / dbl / ptr ...])}`` of every function the header declares."""
    txt = open(HEADER).read()
    out = {}
    for m in re.finditer(r"^(int32_t|int64_t) (slg_\w+)\(([^;]*)\);", txt, re.M):
        kinds = []
        for arg in m.group(3).split(","):
            arg = re.sub(r"/\*.*?\*/", "", arg).strip()
            kinds.append("ptr" if "*" in arg else {"int32_t": "i32", "int64_t": "i64", "double": "dbl"}[arg.split()[0]])
        out[m.group(2)] = (m.group(1), kinds)
    return out


def test_second_table_equals_the_header():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    decl = declarations()
    assert set(decl) == set(N.SURFACE_EXPORTS) == set(N_ARGS)
    assert not set(N.SURFACE_EXPORTS) & set(N.EXPORTS)
    for name, (res, args) in N.SURFACE_EXPORTS.items():
        c_res, c_args = decl[name]
        assert len(args) == N_ARGS[name] and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res], name
    txt = open(HEADER).read()
    assert '#include "slgpu.h"' in txt
    for macro, value in (("SLG_FILTER_BAD_NEIGHBOURS", N.FILTER_BAD_NEIGHBOURS), ("SLG_SURFACE_MAX_NEIGHBOURS", N.SURFACE_MAX_NEIGHBOURS),
                         ("SLG_SURFACE_MAX_RADII", N.SURFACE_MAX_RADII), ("SLG_SURFACE_WS_GRID", N.SURFACE_WS_GRID),
                         ("SLG_SURFACE_WS_PASS", N.SURFACE_WS_PASS)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    # the new status bit is none of slgpu.h's
    assert N.FILTER_BAD_NEIGHBOURS not in (N.FILTER_BAD_NONFINITE, N.FILTER_BAD_EXTENT, N.FILTER_BAD_INDEX)
    import surface_ref as S
    assert S.CAP == MS.MAX_SURFACE_NEIGHBOURS == N.SURFACE_MAX_NEIGHBOURS and S.MAX_RADII == MS.MAX_RADII == 8
    assert MS._PASS_HDR.fields["live"][1] == 8 and MS._PASS_HDR.fields["accepted"][1] == 16
    assert MS._PASS_HDR.itemsize <= N.MESH_HDR_BYTES


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_surface.hip")) for p in B.SRCS)
    assert HEADER in B.digest_files() and B.HDR in B.digest_files()
    lib = N.lib()
    for name in N.SURFACE_EXPORTS:
        assert hasattr(lib, name)
    bad, inv = -N.SLG_ERR_INVALID, N.SLG_ERR_INVALID
    G, Pw = N.SURFACE_WS_GRID, N.SURFACE_WS_PASS
    assert lib.slg_surface_ws_bytes(G, 2, 0, 0) == bad and lib.slg_surface_ws_bytes(7, 100, 10, 0) == bad
    assert lib.slg_surface_ws_bytes(Pw, 100, 0, 0) == bad and lib.slg_surface_ws_bytes(Pw, 2, 10, 0) == bad
    assert lib.slg_surface_ws_bytes(Pw, 100, 10, -1) == bad
    assert lib.slg_surface_ws_bytes(Pw, 100, (1 << 30) // 3 + 1, 0) == bad
    # (the grid's size asks rocPRIM on a device, as slg_filter_ws_bytes does: tests/test_gpu_surface.py)
    grid, need = 1 << 24, lib.slg_surface_ws_bytes(Pw, 100, 10, 6)
    assert need > 0 and need % 256 == 0
    sizes = [lib.slg_surface_ws_bytes(Pw, 1000, c, 0) for c in (1, 1000, 1_000_000)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.slg_surface_ws_bytes(Pw, 1000, 1000, 30_000) > sizes[1]
    fake = 1 << 20                                                    # aligned, never dereferenced: every call refuses first
    assert lib.slg_surface_begin(None, 100, 1.0, fake, grid, None) == inv
    assert lib.slg_surface_begin(fake, 2, 1.0, fake, grid, None) == inv
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.slg_surface_begin(fake, 100, radius, fake, grid, None) == inv
    assert lib.slg_surface_count(None, fake, 100, 1.0, fake, grid, fake, None) == inv
    assert lib.slg_surface_count(fake, None, 100, 1.0, fake, grid, fake, None) == inv
    assert lib.slg_surface_count(fake, fake, 100, 1.0, fake, grid, None, None) == inv
    assert lib.slg_surface_count(fake, fake, 100, -1.0, fake, grid, fake, None) == inv
    assert lib.slg_surface_emit(fake, fake, 100, 1.0, fake, grid, None, 6, fake, need, 10, None) == inv
    assert lib.slg_surface_emit(fake, fake, 100, 1.0, fake, grid, fake, 6, fake, need - 1, 10, None) == inv
    assert lib.slg_surface_emit(fake, fake, 100, 1.0, fake, grid, fake, 6, fake + 8, need, 10, None) == inv   # misaligned
    assert lib.slg_surface_emit(fake, fake, 100, 1.0, fake, grid, fake, 6, fake, need, 0, None) == inv
    assert lib.slg_surface_round(None, need, 100, 10, 6, None) == inv
    assert lib.slg_surface_round(fake, need - 1, 100, 10, 6, None) == inv
    assert lib.slg_surface_round(fake, need, 100, 0, 6, None) == inv
    assert lib.slg_surface_commit(fake, need, 100, 10, fake, 6, 0, fake, fake, fake, None) == inv      # nothing accepted
    assert lib.slg_surface_commit(fake, need, 100, 10, fake, 6, 11, fake, fake, fake, None) == inv     # more than candidates
    assert lib.slg_surface_commit(fake, need, 100, 10, fake, 6, 5, None, fake, fake, None) == inv
    assert lib.slg_surface_commit(fake, need - 1, 100, 10, fake, 6, 5, fake, fake, fake, None) == inv


def test_check_radii():
    from structured_light_for_3d_model_replication_amd import mesh as MS
    assert MS.check_radii([1, 2.5, 4]) == [1.0, 2.5, 4.0] and MS.check_radii(0.5) == [0.5]
    assert MS.check_radii(np.arange(1, 9)) == [float(i) for i in range(1, 9)]
    for bad in ([], list(range(1, 10)), [2, 1], [1, 1], [0.0], [1.0, float("nan")], [float("inf")], [-1.0], ["x"], None):
        with pytest.raises(ValueError, match="radii"):
            MS.check_radii(bad)
        with pytest.raises(ValueError, match="radii"):                # before the cloud is looked at
            MS.ball_pivot(None, bad)


def test_ball_pivot_arguments():
    """A PointCloud of host tensors (built without its constructor, which moves them to a device):
    every error here comes before a device is needed."""
    import torch
    from structured_light_for_3d_model_replication_amd import cloud as CL
    from structured_light_for_3d_model_replication_amd import mesh as MS
    xyz = torch.zeros((5, 3), dtype=torch.float64)
    pc = CL.PointCloud.__new__(CL.PointCloud)
    pc.xyz, pc.bgr, pc.normals = xyz, torch.zeros((5, 3), dtype=torch.uint8), None
    with pytest.raises(ValueError, match="no normals"):
        MS.ball_pivot(pc, [1.0])
    for rounds in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_rounds"):
            MS.ball_pivot(pc, [1.0], max_rounds=rounds)
    pc.normals = torch.zeros((5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="device float64"):           # then the cloud: a host tensor
        MS.ball_pivot(pc, [1.0])
    for n in (0, 1, 2):                                               # fewer than 3 points: empty, without a device call
        pc.xyz, pc.normals = xyz[:n], torch.zeros((n, 3), dtype=torch.float64)
        mesh, rec = MS.ball_pivot(pc, [1.0, 2.0], return_record=True)
        assert mesh.triangles.shape == (0, 3) and mesh.triangles.dtype == torch.int32 and len(mesh.vertices) == n
        assert rec == [dict(radius=1.0, candidates=0, accepted=0, rounds=0), dict(radius=2.0, candidates=0, accepted=0, rounds=0)]


def test_processing_arguments(tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    open(src, "w").write("ply\n")
    with pytest.raises(NotImplementedError, match=r"ball pivoting.*reference \(server/processing.py:711-728\)"):   # as before
        PL.reconstruct_stl(src, out, mode="surface")
    with pytest.raises(NotImplementedError, match="surface_rule"):
        PL.reconstruct_stl(src, out, mode="surface", params={"radii": "1,2"})
    for rule in ("front", "Empty_ball", "", 0):
        with pytest.raises(ValueError, match="surface_rule"):
            PL.reconstruct_stl(src, out, mode="surface", params={"surface_rule": rule})
    ok = {"surface_rule": "empty_ball"}
    for radii in ("1,x", "", "1,,2", "0,1", "-1", "nan", "1,inf", "1,2,3,4,5,6,7,8,9", 3):
        with pytest.raises(ValueError, match="Invalid radii parameters"):
            PL.reconstruct_stl(src, out, mode="surface", params={**ok, "radii": radii})
    with pytest.raises(ValueError, match="binary .stl"):              # the radii pass: then the output's name
        PL.reconstruct_stl(src, str(tmp_path / "mesh.ply"), mode="surface", params={**ok, "radii": "4, 1,2,1"})
    with pytest.raises(ValueError, match="backend"):                  # and the MeshLab step's keys, as for "watertight"
        PL.reconstruct_stl(src, out, mode="surface", params=ok, meshlab_params={"enabled": True, "backend": "other"})
    assert PL._surface_multipliers("4, 1,2,1") == [4.0, 1.0, 2.0, 1.0]
    assert not os.path.exists(out)                                    # nothing was loaded or written
