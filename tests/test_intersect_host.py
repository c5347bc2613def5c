"""Host side of the self-intersection test (no GPU needed): the fifth export table and its ctypes
signatures against include/slgpu_intersect.h, disjoint from the other four, the macros and the one
bound, the build list and the digest, the sizing function, the library's refusals, and the argument
errors of mesh.self_intersections, mesh.check_postprocess, ProcessingLogic.reconstruct_stl and
ProcessingLogic.mesh_360 with the new key, all raised before anything touches a device."""
import inspect
import os
import re

import pytest

from test_audit_host import host_mesh
from test_icp_host import ROOT

HEADER = os.path.join(ROOT, "include", "slgpu_intersect.h")
N_ARGS = {"slg_isect_ws_bytes": 4, "slg_isect_boxes": 8, "slg_isect_entries": 8, "slg_isect_candidates_count": 9,
          "slg_isect_candidates_emit": 12, "slg_isect_test": 11, "slg_isect_list": 10}


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


def test_fifth_table_equals_the_header():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import mesh as MS
    import intersect_ref as I
    kind = {N.c_i32: "i32", N.c_i64: "i64", N.c_dbl: "dbl", N.c_vp: "ptr"}
    decl = declarations()
    assert set(decl) == set(N.INTERSECT_EXPORTS) == set(N_ARGS)
    assert not set(N.INTERSECT_EXPORTS) & (set(N.EXPORTS) | set(N.SURFACE_EXPORTS) | set(N.BAND_EXPORTS) | set(N.AUDIT_EXPORTS))
    for name, (res, args) in N.INTERSECT_EXPORTS.items():
        c_res, c_args = decl[name]
        assert len(args) == N_ARGS[name] and [kind[a] for a in args] == c_args, name
        assert kind[res] == {"int32_t": "i32", "int64_t": "i64"}[c_res], name
    txt = open(HEADER).read()
    assert '#include "slgpu.h"' in txt
    for macro, value in (("SLG_ISECT_WS_BOXES", N.ISECT_WS_BOXES), ("SLG_ISECT_WS_ENTRIES", N.ISECT_WS_ENTRIES),
                         ("SLG_ISECT_WS_PAIRS", N.ISECT_WS_PAIRS), ("SLG_ISECT_WS_LIST", N.ISECT_WS_LIST),
                         ("SLG_ISECT_SPAN_CAP", N.ISECT_SPAN_CAP), ("SLG_ISECT_MAX_CELLS", N.ISECT_MAX_CELLS),
                         ("SLG_ISECT_TILE", N.ISECT_TILE),
                         ("SLG_ISECT_INTERSECTING", I.INTERSECTING), ("SLG_ISECT_UNCERTAIN", I.UNCERTAIN)):
        assert re.search(rf"#define {macro} {value}\b", txt), macro
    assert (N.ISECT_SPAN_CAP, N.ISECT_MAX_CELLS, N.ISECT_TILE) == (64, 1024, 64)
    assert (N.ISECT_INTERSECTING, N.ISECT_UNCERTAIN) == (I.INTERSECTING, I.UNCERTAIN) == (1, 2)
    # one hex-float constant, shared by the header and the restatement
    assert re.search(rf"#define SLG_ISECT_BOUND {re.escape(I.B_HEX)}\n", txt) and N.ISECT_BOUND_HEX == I.B_HEX
    assert float.fromhex(I.B_HEX) == (7.0 + 56.0 * 2.0 ** -53) * 2.0 ** -53
    unit = open(os.path.join(ROOT, "structured_light_for_3d_model_replication_amd", "csrc", "cloud_intersect.hip")).read()
    assert "SLG_ISECT_BOUND" in unit and "0x1." not in unit                    # the unit has no constant of its own
    short = {"adjacent_pairs": "ADJACENT", "tested_pairs": "TESTED", "intersecting_pairs": "INTERSECTING",
             "uncertain_pairs": "UNCERTAIN", "intersecting_triangles": "INTERSECTING_TRIANGLES",
             "uncertain_triangles": "UNCERTAIN_TRIANGLES"}
    for i, name in enumerate(N.ISECT_STATS):                                   # the header's counts in the dict's names
        assert re.search(rf"#define SLG_ISECT_STAT_{short[name]} {i}\b", txt), name
    assert I.COUNTS == MS.INTERSECTION_COUNTS and set(N.ISECT_STATS) | {"candidate_pairs"} == set(I.COUNTS)
    f = MS._ISECT_HDR.fields
    assert [f[k][1] for k in ("status", "entries", "large", "part", "runs", "candidates", "dims", "origin", "cell", "stats")] == \
        [0, 8, 16, 24, 32, 40, 56, 72, 96, 128] and MS._ISECT_HDR.itemsize <= N.MESH_HDR_BYTES
    # the audit keeps its words and points here
    assert "elf-intersection is" in MS.audit.__doc__ and "not tested" in MS.audit.__doc__
    assert "(see :func:`self_intersections`)" in MS.audit.__doc__


def test_source_is_in_the_build_list_and_the_library_refuses():
    from structured_light_for_3d_model_replication_amd import _native as N
    from structured_light_for_3d_model_replication_amd import build as B
    assert any(p.endswith(os.path.join("csrc", "cloud_intersect.hip")) for p in B.SRCS)
    files = B.digest_files()
    assert HEADER in files and B.HDR_INTERSECT == HEADER
    assert all(h in files for h in (B.HDR, B.HDR_SURFACE, B.HDR_BAND, B.HDR_AUDIT))
    assert any(p.endswith(os.path.join("csrc", "mesh_keys.h")) for p in files)
    lib = N.lib()
    for name in N.INTERSECT_EXPORTS:
        assert hasattr(lib, name)
    bad, inv = -N.SLG_ERR_INVALID, N.SLG_ERR_INVALID
    Bo, En, Pa, Li = N.ISECT_WS_BOXES, N.ISECT_WS_ENTRIES, N.ISECT_WS_PAIRS, N.ISECT_WS_LIST
    for stage, nv, nt, n in ((-1, 10, 10, 0), (4, 10, 10, 1), (Bo, 0, 10, 0), (Bo, 10, 0, 0), (Bo, 1 << 31, 10, 0),
                             (Bo, 10, (1 << 30) // 3 + 1, 0), (Bo, 10, 10, -1), (En, 10, 10, 0), (Pa, 10, 10, -1),
                             (Li, 10, 10, 0), (Pa, 10, 10, (1 << 40) + 1)):
        assert lib.slg_isect_ws_bytes(stage, nv, nt, n) == bad, (stage, nv, nt, n)
    sizes = [lib.slg_isect_ws_bytes(Bo, 1000, nt, 0) for nt in (1, 100, 256, 257, 100000, (1 << 30) // 3)]
    assert all(0 < a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1] and all(s % 256 == 0 for s in sizes)
    for stage in (En, Pa, Li):                                        # monotone in the items, whole 256-byte regions
        sizes = [lib.slg_isect_ws_bytes(stage, 1000, 1000, n) for n in (1, 64, 65, 4096, 1 << 20, 1 << 28)]
        assert all(0 < a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1] and all(s % 256 == 0 for s in sizes)
    assert lib.slg_isect_ws_bytes(Bo, 1000, 100000, 0) >= 100000 * (48 + 24 + 16 + 8 + 3)     # boxes, cell ranges, scans, words
    assert lib.slg_isect_ws_bytes(En, 10, 10, 1 << 20) >= (1 << 20) * (4 * 8 + 1 + 12)         # keys twice, runs, the sort
    assert lib.slg_isect_ws_bytes(Pa, 10, 10, 1 << 20) >= (1 << 20) * (2 * 8 + 2)
    fake, big = 1 << 20, 1 << 50                                      # aligned, never dereferenced: every call refuses first
    need = {s: lib.slg_isect_ws_bytes(s, 10, 10, 5) for s in (Bo, En, Pa, Li)}
    # (the workspace under test, its size) in place of a good one: boxes, entries, pairs, list
    calls = {
        "slg_isect_boxes": {Bo: lambda ws, nb: lib.slg_isect_boxes(fake, 10, fake, 10, 0.0, ws, nb, None)},
        "slg_isect_entries": {Bo: lambda ws, nb: lib.slg_isect_entries(10, 10, ws, nb, 5, fake, big, None),
                              En: lambda ws, nb: lib.slg_isect_entries(10, 10, fake, big, 5, ws, nb, None)},
        "slg_isect_candidates_count": {Bo: lambda ws, nb: lib.slg_isect_candidates_count(10, 10, ws, nb, 5, fake, big, 0, None),
                                       En: lambda ws, nb: lib.slg_isect_candidates_count(10, 10, fake, big, 5, ws, nb, 0, None)},
        "slg_isect_candidates_emit": {
            Bo: lambda ws, nb: lib.slg_isect_candidates_emit(10, 10, ws, nb, 5, fake, big, 0, 5, fake, big, None),
            En: lambda ws, nb: lib.slg_isect_candidates_emit(10, 10, fake, big, 5, ws, nb, 0, 5, fake, big, None),
            Pa: lambda ws, nb: lib.slg_isect_candidates_emit(10, 10, fake, big, 5, fake, big, 0, 5, ws, nb, None)},
        "slg_isect_test": {Bo: lambda ws, nb: lib.slg_isect_test(fake, 10, fake, 10, ws, nb, 5, fake, big, fake, None),
                           Pa: lambda ws, nb: lib.slg_isect_test(fake, 10, fake, 10, fake, big, 5, ws, nb, fake, None)},
        "slg_isect_list": {Pa: lambda ws, nb: lib.slg_isect_list(1, 10, 5, ws, nb, 5, fake, big, fake, None),
                           Li: lambda ws, nb: lib.slg_isect_list(1, 10, 5, fake, big, 5, ws, nb, fake, None)},
    }
    assert set(calls) | {"slg_isect_ws_bytes"} == set(N.INTERSECT_EXPORTS)
    for name, by_stage in calls.items():
        for stage, call in by_stage.items():
            n = need[stage]
            assert call(None, big) == inv, (name, stage)                      # NULL
            assert call(fake + 8, big) == inv, (name, stage)                  # misaligned
            assert call(fake, n - 1) == inv and call(fake, 0) == inv and call(fake, -1) == inv, (name, stage)     # short
    assert lib.slg_isect_boxes(None, 10, fake, 10, 0.0, fake, big, None) == inv
    assert lib.slg_isect_boxes(fake, 10, None, 10, 0.0, fake, big, None) == inv
    assert lib.slg_isect_boxes(fake, 10, fake, 0, 0.0, fake, big, None) == inv
    assert lib.slg_isect_boxes(fake, 1 << 31, fake, 10, 0.0, fake, big, None) == inv
    assert lib.slg_isect_boxes(fake, 10, fake, 10, float("nan"), fake, big, None) == inv
    assert lib.slg_isect_entries(10, 10, fake, big, 0, fake, big, None) == inv
    assert lib.slg_isect_entries(10, 10, fake, big, 64 * 10 + 1, fake, big, None) == inv              # more than the span cap allows
    assert lib.slg_isect_entries(1 << 28, 10, fake, big, 1 << 31, fake, big, None) == inv             # one workgroup per entry at most
    assert lib.slg_isect_candidates_count(10, 10, fake, big, -1, fake, big, 0, None) == inv
    assert lib.slg_isect_candidates_count(10, 10, fake, big, 5, fake, big, 11, None) == inv           # more large triangles than triangles
    assert lib.slg_isect_candidates_emit(10, 10, fake, big, 5, fake, big, 0, 0, fake, big, None) == inv
    assert lib.slg_isect_test(None, 10, fake, 10, fake, big, 5, fake, big, fake, None) == inv
    assert lib.slg_isect_test(fake, 10, fake, 10, fake, big, 5, fake, big, None, None) == inv
    assert lib.slg_isect_test(fake, 10, fake, 10, fake, big, 0, fake, big, fake, None) == inv
    assert lib.slg_isect_list(3, 10, 5, fake, big, 5, fake, big, fake, None) == inv                   # an unknown list
    assert lib.slg_isect_list(1, 10, 5, fake, big, 6, fake, big, fake, None) == inv                   # a list longer than the candidates
    assert lib.slg_isect_list(2, 10, 5, fake, big, 5, fake, big, None, None) == inv


def test_python_arguments():
    """Every error here comes before a device is needed: the meshes are host tensors."""
    from structured_light_for_3d_model_replication_amd import mesh as MS
    m = host_mesh()
    with pytest.raises(ValueError, match="device float64"):
        MS.self_intersections(m)
    sig = inspect.signature(MS.self_intersections)
    assert list(sig.parameters)[:7] == ["mesh", "return_pairs", "return_arrays", "max_pairs", "max_candidates", "stream", "timings"]
    assert [sig.parameters[k].default for k in ("return_pairs", "return_arrays", "max_pairs", "max_candidates", "stream", "timings")] == \
        [False, False, 1 << 20, 1 << 28, None, None]
    assert list(inspect.signature(MS.audit).parameters) == ["mesh", "return_arrays", "stream", "timings"]
    counts = dict.fromkeys((*MS.INTERSECTION_COUNTS, *MS.INTERSECTION_GRID), 0)
    assert MS.intersection_verdict(counts) is True
    assert MS.intersection_verdict({**counts, "intersecting_pairs": 1}) is False
    assert MS.intersection_verdict({**counts, "uncertain_pairs": 1}) is False
    line = MS.format_intersections({**counts, "intersection_free": True})
    assert "\n" not in line and "intersection-free" in line and "not intersection-free" not in line
    line = MS.format_intersections({**counts, "intersecting_pairs": 3, "intersecting_triangles": 5, "intersection_free": False})
    assert "3 intersecting" in line and "not intersection-free" in line
    assert "self-intersection not tested" in MS.format_audit({**dict.fromkeys(MS.AUDIT_COUNTS, 0), "signed_volume": 0.0, "area": 0.0,
                                                              **MS.audit_verdict(dict.fromkeys(MS.AUDIT_COUNTS, 0))})


def test_postprocess_and_processing_keys(tmp_path):
    from structured_light_for_3d_model_replication_amd import mesh as MS
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    MS.check_postprocess({"self_intersections": True, "backend": "device"})
    MS.check_postprocess({"self_intersections": False, "audit": True})
    for v in (1, "yes", None):
        with pytest.raises(ValueError, match="self_intersections"):
            MS.check_postprocess({"self_intersections": v})
    with pytest.raises(ValueError, match="belong to"):
        MS.check_postprocess({"self_intersections": True, "backend": "pymeshlab"})
    with pytest.raises(ValueError, match="self_intersections"):      # checked before any launch
        MS.postprocess(host_mesh(), {"self_intersections": 2})
    src = inspect.getsource(MS.postprocess)                           # after the audit, on the final mesh
    assert src.index("audit(mesh") < src.index("self_intersections(mesh")
    assert list(inspect.signature(MS.postprocess).parameters) == ["mesh", "meshlab_params", "stream", "return_record"]
    src, out = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.stl")
    open(src, "w").write("ply\n")
    dev = {"enabled": True, "backend": "device"}
    with pytest.raises(ValueError, match="self_intersections"):
        PL.reconstruct_stl(src, out, params={"depth": 8}, meshlab_params={**dev, "self_intersections": "yes"})
    for backend in ({"backend": "pymeshlab"}, {}):
        with pytest.raises(ValueError, match="belong to"):
            PL.reconstruct_stl(src, out, params={"depth": 8}, meshlab_params={"enabled": True, **backend, "self_intersections": True})
    with pytest.raises(ValueError, match="binary .stl"):              # the key passes with the device backend: then the output's name
        PL.reconstruct_stl(src, str(tmp_path / "mesh.ply"), params={"depth": 8}, meshlab_params={**dev, "self_intersections": True})
    with pytest.raises(ValueError, match="self_intersections"):
        PL.mesh_360(src, out, depth=8, self_intersections="yes")
    with pytest.raises(ValueError, match="binary .stl"):
        PL.mesh_360(src, str(tmp_path / "mesh.ply"), depth=8, self_intersections=True)
    p = inspect.signature(PL.mesh_360).parameters["self_intersections"]
    assert p.kind == p.KEYWORD_ONLY and p.default is False
    assert "[Mesh] intersections:" in inspect.getsource(PL.reconstruct_stl) and "[Mesh] intersections:" in inspect.getsource(PL.mesh_360)
    assert not os.path.exists(out)                                    # nothing was loaded or written
