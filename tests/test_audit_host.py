"""Host side of the mesh audit (no GPU needed): the fourth export table and its ctypes signatures
against include/slgpu_audit.h, the macros, the build list and the digest, the library's refusals, the
sizing function, and the argument errors of mesh.keep_largest_components, mesh.remove_small_components,
mesh.check_postprocess, ProcessingLogic.reconstruct_stl and ProcessingLogic.mesh_360 with and without
the new keys, all raised before anything touches a device."""
import inspect
import os
import re

import pytest

from test_icp_host import ROOT

HEADER = os.path.join(ROOT, "include", "slgpu_audit.h")
N_ARGS = {"slg_audit_ws_bytes": 3, "slg_audit_edges": 8, "slg_audit_components_count": 7, "slg_audit_components_emit": 8,
          "slg_audit_fans": 8, "slg_audit_measure": 8, "slg_audit_keep": 8, "slg_audit_select": 13}


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


def test_fourth_table_equals_the_header():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    import audit_ref as A
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    decl = declarations()
    assert set(decl) == set(N.AUDIT_EXPORTS) == set(N_ARGS)
    assert not set(N.AUDIT_EXPORTS) & (set(N.EXPORTS) | set(N.SURFACE_EXPORTS) | set(N.BAND_EXPORTS))
    for name, (res, args) in N.AUDIT_EXPORTS.items():
        c_res, c_args = decl[name]
        assert len(args) == N_ARGS[name] and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res], name
    txt = open(HEADER).read()
    assert '#include "slgpu.h"' in txt
    for macro, value in (("SLG_AUDIT_WS_AUDIT", N.AUDIT_WS_AUDIT), ("SLG_AUDIT_WS_MEASURE", N.AUDIT_WS_MEASURE),
                         ("SLG_AUDIT_WS_SELECT", N.AUDIT_WS_SELECT), ("SLG_AUDIT_CHUNK", N.AUDIT_CHUNK),
                         ("SLG_AUDIT_VERTEX_REFERENCED", A.REFERENCED), ("SLG_AUDIT_VERTEX_BOUNDARY", A.ON_BOUNDARY),
                         ("SLG_AUDIT_VERTEX_NONMANIFOLD_EDGE", A.ON_NONMANIFOLD_EDGE),
                         ("SLG_AUDIT_VERTEX_INCONSISTENT", A.ON_INCONSISTENT_EDGE),
                         ("SLG_AUDIT_VERTEX_NONMANIFOLD", A.NONMANIFOLD_VERTEX), ("SLG_AUDIT_TRIANGLE_DEGENERATE", A.DEGENERATE),
                         ("SLG_AUDIT_TRIANGLE_DUPLICATE", A.DUPLICATE)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    short = {"edges": "EDGES", "boundary_edges": "BOUNDARY", "manifold_edges": "MANIFOLD", "nonmanifold_edges": "NONMANIFOLD",
             "inconsistent_edges": "INCONSISTENT", "degenerate_triangles": "DEGENERATE", "duplicate_triangles": "DUPLICATES",
             "nonmanifold_vertices": "NONMANIFOLD_VERTICES"}
    for i, name in enumerate(N.AUDIT_STATS):                           # the header's counts in the dict's names
        assert re.search(rf"#define SLG_AUDIT_STAT_{short[name]} {i}\b", txt), name
    assert (N.AUDIT_VERTEX_REFERENCED, N.AUDIT_VERTEX_BOUNDARY, N.AUDIT_VERTEX_NONMANIFOLD_EDGE, N.AUDIT_VERTEX_INCONSISTENT,
            N.AUDIT_VERTEX_NONMANIFOLD, N.AUDIT_TRIANGLE_DEGENERATE, N.AUDIT_TRIANGLE_DUPLICATE) == (1, 2, 4, 8, 16, 1, 2)
    assert A.CHUNK == N.AUDIT_CHUNK and A.COUNTS == MS.AUDIT_COUNTS and A.VERDICTS == MS.AUDIT_VERDICTS
    assert MS._AUDIT_HDR.fields["stats"][1] == 128 and MS._AUDIT_HDR.itemsize <= N.MESH_HDR_BYTES
    assert [MS._AUDIT_HDR.fields[k][1] for k in ("status", "nV", "nT", "nC", "largest")] == [0, 8, 16, 24, 32]
    assert "elf-intersection is" in MS.audit.__doc__ and "not tested" in MS.audit.__doc__


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_audit.hip")) for p in B.SRCS)
    files = B.digest_files()
    assert HEADER in files and B.HDR_AUDIT == HEADER and B.HDR in files and B.HDR_SURFACE in files and B.HDR_BAND in files
    assert any(p.endswith(os.path.join("csrc", "mesh_keys.h")) for p in files)
    lib = N.lib()
    for name in N.AUDIT_EXPORTS:
        assert hasattr(lib, name)
    bad, inv = -N.SLG_ERR_INVALID, N.SLG_ERR_INVALID
    Au, Me, Se = N.AUDIT_WS_AUDIT, N.AUDIT_WS_MEASURE, N.AUDIT_WS_SELECT
    for stage, nv, nt in ((-1, 10, 10), (3, 10, 10), (Au, 0, 10), (Au, 10, 0), (Au, 1 << 31, 10), (Se, 10, (1 << 30) // 3 + 1)):
        assert lib.slg_audit_ws_bytes(stage, nv, nt) == bad
    for stage in (Au, Me, Se):                                        # monotone in nt, whole 256-byte regions
        sizes = [lib.slg_audit_ws_bytes(stage, 1000, nt) for nt in (1, 100, 2048, 2049, 100000, (1 << 30) // 3)]
        assert all(0 < a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1] and all(s % 256 == 0 for s in sizes)
    assert lib.slg_audit_ws_bytes(Au, 1000, 100000) >= 100000 * (3 * 24 + 3 * 12)    # two copies of keys and values, corners
    assert lib.slg_audit_ws_bytes(Me, 10, 2049) - lib.slg_audit_ws_bytes(Me, 10, 2048) in (0, 256)
    fake, big = 1 << 20, 1 << 40                                      # aligned, never dereferenced: every call refuses first
    need = {s: lib.slg_audit_ws_bytes(s, 10, 10) for s in (Au, Me, Se)}
    calls = {
        "slg_audit_edges": lambda ws, nb: lib.slg_audit_edges(fake, 10, 10, ws, nb, fake, fake, None),
        "slg_audit_components_count": lambda ws, nb: lib.slg_audit_components_count(10, 10, ws, nb, fake, fake, None),
        "slg_audit_components_emit": lambda ws, nb: lib.slg_audit_components_emit(10, 10, ws, nb, fake, 2, fake, None),
        "slg_audit_fans": lambda ws, nb: lib.slg_audit_fans(fake, 10, 10, ws, nb, fake, fake, None),
        "slg_audit_measure": lambda ws, nb: lib.slg_audit_measure(fake, 10, fake, 10, ws, nb, fake, None),
        "slg_audit_select": lambda ws, nb: lib.slg_audit_select(fake, None, 10, fake, 10, fake, 1, ws, nb, fake, None, fake, None),
    }
    stage_of = {"slg_audit_measure": Me, "slg_audit_select": Se}
    assert set(calls) | {"slg_audit_ws_bytes", "slg_audit_keep"} == set(N.AUDIT_EXPORTS)
    for name, call in calls.items():
        n = need[stage_of.get(name, Au)]
        assert call(None, big) == inv, name                           # NULL
        assert call(fake + 8, big) == inv, name                       # misaligned
        assert call(fake, n - 1) == inv and call(fake, 0) == inv and call(fake, -1) == inv, name      # short
    assert lib.slg_audit_edges(None, 10, 10, fake, big, fake, fake, None) == inv
    assert lib.slg_audit_edges(fake, 0, 10, fake, big, fake, fake, None) == inv
    assert lib.slg_audit_edges(fake, 10, 1 << 31, fake, big, fake, fake, None) == inv
    assert lib.slg_audit_components_count(10, 10, fake, big, None, fake, None) == inv
    assert lib.slg_audit_components_emit(10, 10, fake, big, fake, 0, fake, None) == inv
    assert lib.slg_audit_components_emit(10, 10, fake, big, fake, 11, fake, None) == inv               # more components than triangles
    assert lib.slg_audit_fans(fake, 10, 10, fake, big, fake, None, None) == inv
    assert lib.slg_audit_measure(fake, 10, fake, 10, fake, big, None, None) == inv
    assert lib.slg_audit_select(fake, fake, 10, fake, 10, fake, 1, fake, big, fake, None, fake, None) == inv  # densities without an output
    assert lib.slg_audit_keep(fake, None, 10, None, 0, 3, None, None) == inv
    assert lib.slg_audit_keep(None, None, 10, None, 0, 3, fake, None) == inv                           # bits to drop without classes
    assert lib.slg_audit_keep(fake, None, 10, fake, 2, 0, fake, None) == inv                           # a table without labels
    assert lib.slg_audit_keep(fake, fake, 0, fake, 2, 0, fake, None) == inv
    assert lib.slg_audit_keep(fake, fake, 10, None, 2, 0, fake, None) == inv


def host_mesh(nt=4):
    import torch
    from structured_light_for_3d_model_replication_amd import mesh as MS
    return MS.TriangleMesh(torch.zeros((4, 3), dtype=torch.float64), torch.zeros((nt, 3), dtype=torch.int32))


def test_python_arguments():
    """Every error here comes before a device is needed: the meshes are host tensors."""
    from structured_light_for_3d_model_replication_amd import mesh as MS
    m = host_mesh()
    for count in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="count must be a whole number >= 1"):
            MS.keep_largest_components(m, count)
    for least in (-1, 2.5, False):
        with pytest.raises(ValueError, match="min_triangles must be a whole number >= 0"):
            MS.remove_small_components(m, least)
    for fn in (MS.audit, MS.connected_components, MS.clean, MS.keep_largest_components,
               lambda x: MS.remove_small_components(x, 3)):
        with pytest.raises(ValueError, match="device float64"):       # then the mesh: a host tensor
            fn(m)
    for name in ("audit", "connected_components", "keep_largest_components", "remove_small_components", "clean"):
        assert "stream" in inspect.signature(getattr(MS, name)).parameters
    counts = dict.fromkeys(MS.AUDIT_COUNTS, 0)
    assert MS.audit_verdict(counts) == dict(closed=True, edge_manifold=True, vertex_manifold=True, oriented=True, watertight=False)
    assert MS.audit_verdict({**counts, "triangles": 4})["watertight"]
    for key in ("boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "inconsistent_edges", "degenerate_triangles",
                "duplicate_triangles"):
        assert not MS.audit_verdict({**counts, "triangles": 4, key: 1})["watertight"], key
    line = MS.format_audit({**counts, "triangles": 4, "signed_volume": 1.0, "area": 2.0, **MS.audit_verdict({**counts, "triangles": 4})})
    assert "watertight" in line and "not watertight" not in line and "self-intersection not tested" in line
    line = MS.format_audit({**counts, "boundary_edges": 3, "signed_volume": 0.0, "area": 0.0,
                            **MS.audit_verdict({**counts, "boundary_edges": 3})})
    assert "not watertight (not closed)" in line


def test_postprocess_keys():
    from structured_light_for_3d_model_replication_amd import mesh as MS
    MS.check_postprocess({})                                          # the old keys as before
    MS.check_postprocess({"smooth_iters": 3, "close_holes": True, "close_max_size": 10})
    with pytest.raises(NotImplementedError):
        MS.check_postprocess({"simplify": True})
    with pytest.raises(ValueError, match="max_size"):
        MS.check_postprocess({"close_holes": True, "close_max_size": 100})
    MS.check_postprocess({"keep_components": 1, "min_component_faces": 0, "clean": True, "audit": True, "backend": "device"})
    MS.check_postprocess({"keep_components": None, "min_component_faces": None, "clean": False, "audit": False})
    for k in (0, -2, 1.5, "two", True):
        with pytest.raises(ValueError, match="keep_components"):
            MS.check_postprocess({"keep_components": k})
    for n in (-1, 0.5, "many"):
        with pytest.raises(ValueError, match="min_component_faces"):
            MS.check_postprocess({"min_component_faces": n})
    for key in ("clean", "audit"):
        for v in (1, "yes", None):
            with pytest.raises(ValueError, match=key):
                MS.check_postprocess({key: v})
    for key, v in (("keep_components", 1), ("min_component_faces", 5), ("clean", True), ("audit", True)):
        with pytest.raises(ValueError, match="belong to"):
            MS.check_postprocess({key: v, "backend": "pymeshlab"})
    with pytest.raises(ValueError, match="keep_components"):          # the new keys are checked before any launch
        MS.postprocess(host_mesh(), {"keep_components": 0})
    with pytest.raises(ValueError, match="device float64"):           # and without them the first step is the smoothing's
        MS.postprocess(host_mesh(), {"smooth_iters": 1})
    src = inspect.getsource(MS.postprocess)                           # the order: components, smoothing, holes, clean, simplify, audit
    order = [src.index(s) for s in ("keep_largest_components(", "remove_small_components(", "smooth_taubin(", "close_holes(mesh",
                                    "clean(mesh", "decimate_quadric(", "audit(mesh")]
    assert order == sorted(order)
    assert list(inspect.signature(MS.postprocess).parameters) == ["mesh", "meshlab_params", "stream", "return_record"]


def test_processing_arguments(tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    open(src, "w").write("ply\n")
    dev = {"enabled": True, "backend": "device"}
    for extra in ({"keep_components": 0}, {"min_component_faces": -1}, {"clean": "yes"}, {"audit": 2}):
        with pytest.raises(ValueError, match=next(iter(extra))):
            PL.reconstruct_stl(src, out, params={"depth": 8}, meshlab_params={**dev, **extra})
    for extra in ({"keep_components": 1}, {"min_component_faces": 10}, {"clean": True}, {"audit": True}):
        for backend in ({"backend": "pymeshlab"}, {}):
            with pytest.raises(ValueError, match="belong to"):
                PL.reconstruct_stl(src, out, params={"depth": 8}, meshlab_params={"enabled": True, **backend, **extra})
    with pytest.raises(ValueError, match="binary .stl"):              # the keys pass with the device backend: then the output's name
        PL.reconstruct_stl(src, str(tmp_path / "mesh.ply"), params={"depth": 8},
                           meshlab_params={**dev, "keep_components": 2, "min_component_faces": 10, "clean": True, "audit": True})
    with pytest.raises(ValueError, match="dense grid's limit"):       # without the keys everything is as it was
        PL.reconstruct_stl(src, out, params={"depth": 11}, meshlab_params=dev)
    with pytest.raises(NotImplementedError):
        PL.reconstruct_stl(src, out, params={"depth": 8}, meshlab_params={**dev, "simplify": True})
    for k in (0, 1.5, "one"):
        with pytest.raises(ValueError, match="keep_components"):
            PL.mesh_360(src, out, depth=8, keep_components=k)
    with pytest.raises(ValueError, match="audit"):
        PL.mesh_360(src, out, depth=8, audit="yes")
    with pytest.raises(ValueError, match="binary .stl"):
        PL.mesh_360(src, str(tmp_path / "mesh.ply"), depth=8, keep_components=1, audit=True)
    with pytest.raises(TypeError):                                    # keyword-only, after the existing parameters
        PL.mesh_360(src, out, 8, 0.01, "tangent", 0.0, 1.1, False, -1, 0.1, 30, None, None, None, None, 1)
    params = list(inspect.signature(PL.mesh_360).parameters.values())
    assert [p.name for p in params[-2:]] == ["keep_components", "audit"] and all(p.kind == p.KEYWORD_ONLY for p in params[-2:])
    assert params[-2].default is None and params[-1].default is False
    assert not os.path.exists(out)                                    # nothing was loaded or written
