"""Host side of the banded cascadic mesher (no GPU needed): the third export table and its ctypes
signatures against include/slgpu_band.h, the macros, the build list and the digest, the library's
refusals, and the argument errors of mesh.check_band_depth, mesh.poisson_band,
ProcessingLogic.reconstruct_stl and ProcessingLogic.mesh_360 with and without the "poisson_rule" key,
all raised before anything touches a device."""
import os
import re

import pytest

from test_icp_host import ROOT

HEADER = os.path.join(ROOT, "include", "slgpu_band.h")
N_ARGS = {"slg_band_ws_bytes": 4, "slg_band_level": 5, "slg_band_blocks": 10, "slg_band_nodes": 8, "slg_band_splat": 15,
          "slg_band_divergence": 9, "slg_band_prolong": 10, "slg_band_smooth": 11, "slg_band_iso": 10, "slg_band_count": 10,
          "slg_band_emit": 16}


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


def test_third_table_equals_the_header():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    decl = declarations()
    assert set(decl) == set(N.BAND_EXPORTS) == set(N_ARGS)
    assert not set(N.BAND_EXPORTS) & (set(N.EXPORTS) | set(N.SURFACE_EXPORTS))
    for name, (res, args) in N.BAND_EXPORTS.items():
        c_res, c_args = decl[name]
        assert len(args) == N_ARGS[name] and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res], name
    txt = open(HEADER).read()
    assert '#include "slgpu.h"' in txt
    for macro, value in (("SLG_BAND_MIN_DEPTH", N.BAND_MIN_DEPTH), ("SLG_BAND_MAX_DEPTH", N.BAND_MAX_DEPTH),
                         ("SLG_BAND_MAX_BASE_DEPTH", N.BAND_MAX_BASE_DEPTH), ("SLG_BAND_BLOCK", N.BAND_BLOCK),
                         ("SLG_BAND_WS_BLOCKS", N.BAND_WS_BLOCKS), ("SLG_BAND_WS_SPLAT", N.BAND_WS_SPLAT),
                         ("SLG_BAND_WS_ISO", N.BAND_WS_ISO), ("SLG_BAND_WS_EXTRACT", N.BAND_WS_EXTRACT)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    for i, name in enumerate(N.BAND_STATS):                           # the header's counts in the record's names
        macro = "SLG_BAND_STAT_" + {"seeded_blocks": "SEEDED", "active_blocks": "ACTIVE"}.get(name, name.upper())
        assert re.search(rf"#define {macro} {i}\b", txt), macro
    import band_ref as BR
    assert (BR.MIN_DEPTH, BR.MAX_DEPTH, BR.MAX_BASE, BR.B) == (MS.BAND_MIN_DEPTH, MS.BAND_MAX_DEPTH, MS.BAND_MAX_BASE_DEPTH, N.BAND_BLOCK)
    assert BR.DEFAULT_BAND_SWEEPS == MS.DEFAULT_BAND_SWEEPS == 16
    assert MS._BAND_HDR.fields["stats"][1] == 128 and MS._BAND_HDR.itemsize <= N.MESH_HDR_BYTES
    assert all(MS._BAND_HDR.fields[k][1] == MS._HDR.fields[k][1] for k in MS._HDR.names)
    assert MS.MAX_DEPTH == N.MESH_MAX_DEPTH == 10                     # the dense mesher's limit is where it was


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_band.hip")) for p in B.SRCS)
    files = B.digest_files()
    assert HEADER in files and B.HDR in files and B.HDR_SURFACE in files
    assert any(p.endswith(os.path.join("csrc", "mesh_rules.h")) for p in files)
    lib = N.lib()
    for name in N.BAND_EXPORTS:
        assert hasattr(lib, name)
    bad, inv = -N.SLG_ERR_INVALID, N.SLG_ERR_INVALID
    Bk, Sp, Is, Ex = N.BAND_WS_BLOCKS, N.BAND_WS_SPLAT, N.BAND_WS_ISO, N.BAND_WS_EXTRACT
    assert lib.slg_band_ws_bytes(-1, 64, 10, 1) == bad and lib.slg_band_ws_bytes(4, 64, 10, 1) == bad
    for R in (0, 4, 48, 8192):
        assert lib.slg_band_ws_bytes(Bk, R, 0, 0) == bad
    assert lib.slg_band_ws_bytes(Sp, 64, -1, 0) == bad and lib.slg_band_ws_bytes(Ex, 64, 0, 0) == bad
    assert lib.slg_band_ws_bytes(Ex, 64, 0, 1 << 31) == bad
    assert lib.slg_band_ws_bytes(Sp, 64, (1 << 30) + 1, 0) == -N.SLG_ERR_UNSUPPORTED
    blocks = [lib.slg_band_ws_bytes(Bk, R, 0, 0) for R in (8, 64, 4096)]
    assert all(0 < a < b for a, b in zip(blocks, blocks[1:])) and all(b % 256 == 0 for b in blocks)
    assert blocks[2] >= 513 ** 3                                      # one byte per node block at depth 12
    sizes = [lib.slg_band_ws_bytes(Ex, 64, 0, nb) for nb in (1, 100, 10000)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and sizes[1] >= 100 * 512 * 19
    assert 0 < lib.slg_band_ws_bytes(Is, 64, 1000, 0) < lib.slg_band_ws_bytes(Sp, 64, 1000, 0)
    fake, ws = 1 << 20, 1 << 30                                       # aligned, never dereferenced: every call refuses first
    assert lib.slg_band_level(None, 16, 64, fake, None) == inv and lib.slg_band_level(fake, 16, 64, fake + 8, None) == inv
    assert lib.slg_band_level(fake, 64, 64, fake, None) == inv and lib.slg_band_level(fake, 24, 64, fake, None) == inv
    assert lib.slg_band_level(fake, 16, 8192, fake, None) == inv
    assert lib.slg_band_blocks(None, 10, 64, fake, fake, fake, fake, fake, ws, None) == inv
    assert lib.slg_band_blocks(fake, 0, 64, fake, fake, fake, fake, fake, ws, None) == inv
    assert lib.slg_band_blocks(fake, 10, 48, fake, fake, fake, fake, fake, ws, None) == inv
    assert lib.slg_band_blocks(fake, 10, 64, fake, fake, fake, fake, fake, blocks[1] - 1, None) == inv
    assert lib.slg_band_blocks(fake, 10, 64, fake, fake, fake, fake, fake + 8, ws, None) == inv       # misaligned
    assert lib.slg_band_blocks(fake, (1 << 30) + 1, 64, fake, fake, fake, fake, fake, ws, None) == N.SLG_ERR_UNSUPPORTED
    assert lib.slg_band_nodes(64, fake, fake, fake, 0, fake, fake, None) == inv
    assert lib.slg_band_nodes(64, fake, fake, fake, 9 ** 3 + 1, fake, fake, None) == inv               # more than (R/8+1)^3 blocks
    assert lib.slg_band_nodes(64, fake, fake, None, 5, fake, fake, None) == inv
    assert lib.slg_band_splat(fake, None, 10, 64, fake, fake, fake, fake, fake, 5, fake, ws, fake, fake, None) == inv
    assert lib.slg_band_splat(fake, fake, 10, 64, fake, fake, fake, fake, fake, 5, fake, 16, fake, fake, None) == inv
    assert lib.slg_band_divergence(None, 64, fake, fake, fake, fake, 5, fake, None) == inv
    assert lib.slg_band_divergence(fake, 64, fake + 8, fake, fake, fake, 5, fake, None) == inv
    assert lib.slg_band_prolong(None, None, 0, 64, fake, fake, fake, 5, fake, None) == inv
    assert lib.slg_band_prolong(fake, fake, 0, 64, fake, fake, fake, 5, fake, None) == inv             # a banded parent without blocks
    assert lib.slg_band_prolong(fake, fake, 5, 8, fake, fake, fake, 1, fake, None) == inv              # no banded level below R = 8
    assert lib.slg_band_smooth(fake, 64, fake, fake, fake, fake, 5, -1, fake, fake + 4096, None) == inv
    assert lib.slg_band_smooth(fake, 64, fake, fake, fake, fake, 5, 2, fake, fake, None) == inv        # u == tmp
    assert lib.slg_band_iso(fake, fake, 0, 64, fake, fake, 5, fake, ws, None) == inv
    assert lib.slg_band_iso(fake, fake, 10, 64, fake, fake, 5, fake, 16, None) == inv
    assert lib.slg_band_count(fake, 64, fake, fake, fake, fake, 5, fake, sizes[0], None) == inv        # sized for 1 block, not 5
    assert lib.slg_band_count(None, 64, fake, fake, fake, fake, 5, fake, ws, None) == inv
    assert lib.slg_band_emit(fake, fake, 64, fake, fake, fake, fake, 5, fake, ws, None, 10, fake, fake, 10, None) == inv
    assert lib.slg_band_emit(fake, fake, 64, fake, fake, fake, fake, 5, fake, ws, fake, 1 << 31, fake, fake, 10,
                             None) == N.SLG_ERR_UNSUPPORTED


def test_check_band_depth():
    from structured_light_for_3d_model_replication_amd import mesh as MS
    assert MS.check_band_depth(11) == (11, 8) and MS.check_band_depth(12) == (12, 8) and MS.check_band_depth(3) == (3, 2)
    assert MS.check_band_depth(6) == (6, 5) and MS.check_band_depth(12, 10) == (12, 10) and MS.check_band_depth(7, 2) == (7, 2)
    for depth in (2, 13, 16, -1):
        with pytest.raises(ValueError, match="depth must be in 3..12"):
            MS.check_band_depth(depth)
    for depth, base in ((6, 6), (6, 1), (12, 11), (5, 7)):
        with pytest.raises(ValueError, match="base_depth must be in 2.."):
            MS.check_band_depth(depth, base)
    with pytest.raises(ValueError, match="dense grid's limit"):       # the dense mesher's check is what it was
        MS.check_depth(11)


def test_poisson_band_arguments():
    """A PointCloud of host tensors (built without its constructor, which moves them to a device):
    every error here comes before a device is needed."""
    import torch
    from structured_light_for_3d_model_replication_amd import cloud as CL
    from structured_light_for_3d_model_replication_amd import mesh as MS
    pc = CL.PointCloud.__new__(CL.PointCloud)
    pc.xyz, pc.bgr, pc.normals = torch.zeros((5, 3), dtype=torch.float64), torch.zeros((5, 3), dtype=torch.uint8), None
    with pytest.raises(ValueError, match="depth must be in 3..12"):
        MS.poisson_band(pc, depth=13)
    with pytest.raises(ValueError, match="base_depth"):
        MS.poisson_band(pc, depth=11, base_depth=11)
    for sweeps in (-1, 2.5):
        with pytest.raises(ValueError, match="sweeps"):
            MS.poisson_band(pc, sweeps=sweeps)
    for scale in (0.9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            MS.poisson_band(pc, scale=scale)
    with pytest.raises(ValueError, match="cycles"):
        MS.poisson_band(pc, cycles=-1)
    with pytest.raises(ValueError, match="no normals"):
        MS.poisson_band(pc)
    pc.normals = torch.zeros((5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="device float64"):           # then the cloud: a host tensor
        MS.poisson_band(pc)
    with pytest.raises(ValueError, match="dense grid's limit"):       # without the key the dense mesher refuses as before
        MS.poisson_grid(pc, depth=11)


def test_processing_arguments(tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    open(src, "w").write("ply\n")
    band = {"poisson_rule": "band"}
    for params in ({"depth": 11}, {"depth": 11, "base_depth": 8, "band_sweeps": 4}):                  # the keys alone change nothing
        with pytest.raises(ValueError, match="dense grid's limit"):
            PL.reconstruct_stl(src, out, params=params)
    with pytest.raises(ValueError, match="dense grid's limit"):
        PL.mesh_360(src, out, depth=11)
    for rule in ("dense", "Band", "", 0):
        with pytest.raises(ValueError, match="poisson_rule"):
            PL.reconstruct_stl(src, out, params={"depth": 8, "poisson_rule": rule})
        with pytest.raises(ValueError, match="poisson_rule"):
            PL.mesh_360(src, out, depth=8, poisson_rule=rule)
    for depth in (17, 40):
        with pytest.raises(ValueError, match="too high! Maximum recommended is 12-14"):
            PL.reconstruct_stl(src, out, params={**band, "depth": depth})
        with pytest.raises(ValueError, match="too high! Maximum recommended is 12-14"):
            PL.mesh_360(src, out, depth=depth, poisson_rule="band")
    for depth in (2, 13, 16):
        with pytest.raises(ValueError, match="depth must be in 3..12"):
            PL.reconstruct_stl(src, out, params={**band, "depth": depth})
        with pytest.raises(ValueError, match="depth must be in 3..12"):
            PL.mesh_360(src, out, depth=depth, poisson_rule="band")
    with pytest.raises(ValueError, match="base_depth"):
        PL.reconstruct_stl(src, out, params={**band, "depth": 11, "base_depth": 11})
    with pytest.raises(ValueError, match="base_depth"):
        PL.mesh_360(src, out, depth=9, poisson_rule="band", base_depth=1)
    for sweeps in (-1, 2.5, "many"):
        with pytest.raises(ValueError, match="band_sweeps"):
            PL.reconstruct_stl(src, out, params={**band, "depth": 11, "band_sweeps": sweeps})
        with pytest.raises(ValueError, match="band_sweeps"):
            PL.mesh_360(src, out, depth=11, poisson_rule="band", band_sweeps=sweeps)
    for kw in (dict(base_depth=8), dict(band_sweeps=4)):              # mesh_360's new keywords belong to the key
        with pytest.raises(ValueError, match="belong to poisson_rule"):
            PL.mesh_360(src, out, depth=8, **kw)
    for kw in (dict(width=0.5), dict(linear_fit=True)):
        with pytest.raises(ValueError, match="not implemented on the dense grid"):
            PL.mesh_360(src, out, depth=11, poisson_rule="band", **kw)
    with pytest.raises(ValueError, match="scale"):
        PL.mesh_360(src, out, depth=11, poisson_rule="band", scale=0.5)
    with pytest.raises(ValueError, match="binary .stl"):              # the depth passes with the key: then the output's name
        PL.reconstruct_stl(src, str(tmp_path / "mesh.ply"), params={**band, "depth": 12, "base_depth": 9, "band_sweeps": 0})
    with pytest.raises(ValueError, match="binary .stl"):
        PL.mesh_360(src, str(tmp_path / "mesh.ply"), depth=11, poisson_rule="band")
    with pytest.raises(ValueError, match="backend"):                  # and the MeshLab step's keys, as without it
        PL.reconstruct_stl(src, out, params={**band, "depth": 11}, meshlab_params={"enabled": True, "backend": "other"})
    assert PL._check_band_poisson("band", 11) == dict(depth=11, base_depth=8, sweeps=16)
    assert PL._check_band_poisson(None, 11) is None
    assert not os.path.exists(out)                                    # nothing was loaded or written
