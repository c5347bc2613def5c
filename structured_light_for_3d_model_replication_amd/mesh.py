"""Watertight meshing of an oriented device cloud (``csrc/cloud_mesh.hip``): the last
call of the reference's ``mesh_360`` and ``reconstruct_stl(mode="watertight")``
(``server/processing.py:703``, ``:842``) without leaving HBM.

Open3D's mesher is Kazhdan's adaptive-octree screened Poisson solver; this is the same idea on a
dense uniform grid of ``R = 2**depth`` cells per axis, our rule with Open3D parity unpinned: a
trilinear splat of the normals, its divergence, a fixed number of multigrid V(2,2) cycles, the mean
of the solution at the points as iso value, and marching tetrahedra over Kuhn's six tetrahedra per
cell.  Every step is a pure function of its input; ``tests/mesh_ref.py`` restates each in NumPy and
the device equals it bit for bit.  Node fields are float64 ``[R+1, R+1, R+1]`` tensors indexed
``[z, y, x]``.

Behind it, what the device takes of the reference's MeshLab step (``csrc/cloud_meshpost.hip``,
DESIGN.md §17): :func:`vertex_adjacency`, :func:`smooth_laplacian`, :func:`smooth_taubin`,
:func:`close_holes`, :func:`boundary_loops` and :func:`postprocess`, restated in
``tests/meshpost_ref.py``, and :func:`decimate_quadric` (``csrc/cloud_decimate.hip``),
restated in ``tests/decimate_ref.py``; parity with MeshLab / VCGlib is unpinned.

Beside the watertight mesher, the surface mesh of ``reconstruct_stl(mode="surface")`` under the
device's own rule (``csrc/cloud_surface.hip``): :func:`ball_pivot`, the empty-ball
triangles radius by radius, restated in ``tests/surface_ref.py``; parity with Open3D's ball
pivoting is unpinned.

For depths the dense grid cannot hold, the second watertight rule (``csrc/cloud_band.hip``,
DESIGN.md §21): :func:`poisson_band`, a dense solve at a base depth and finer levels only in blocks
of 8^3 cells near the points, depth 3..12, restated in ``tests/band_ref.py``; behind the callers'
``"poisson_rule": "band"``.

Last, whether the result can be printed (``csrc/cloud_audit.hip``): :func:`audit`
(closed, manifold, oriented, components, volume, area; self-intersection is not tested),
:func:`connected_components`, :func:`keep_largest_components`, :func:`remove_small_components` and
:func:`clean`, restated in ``tests/audit_ref.py``; parity with Open3D's counterparts is unpinned.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _native as N
from . import cloud as CL
from . import engine as E

MIN_DEPTH, MAX_DEPTH = 2, N.MESH_MAX_DEPTH
# V(2,2) cycles of poisson_grid: the smallest count at which the restatement's relative residual is
# <= 6e-8 (float32 epsilon: the STL stores float32) on every test cloud at depths 4-6, which is 12,
# plus 2 (tests/test_mesh_ref.py)
DEFAULT_CYCLES = 14
STL_HEADER = b"structured_light_for_3d_model_replication_amd grid Poisson binary STL".ljust(80)
_HDR = np.dtype([("status", "<i4"), ("R", "<i4"), ("nV", "<i8"), ("nT", "<i8"), ("origin", "<f8", 3), ("h", "<f8"),
                 ("iso", "<f8"), ("thr", "<f8")])


class TriangleMesh:
    """A triangle mesh in HBM: ``vertices`` float64 ``[V, 3]``, ``triangles`` int32 ``[T, 3]``,
    ``densities`` float64 ``[V]`` or ``None``, ``triangle_normals`` float64 ``[T, 3]`` or ``None``
    (:func:`compute_triangle_normals`)."""

    def __init__(self, vertices, triangles, densities=None, triangle_normals=None):
        self.vertices, self.triangles = vertices, triangles
        self.densities, self.triangle_normals = densities, triangle_normals

    def __repr__(self):
        return f"TriangleMesh(vertices={len(self.vertices)}, triangles={len(self.triangles)})"


class PoissonField:
    """What ``poisson_grid(..., return_field=True)`` adds: ``origin`` (3 floats), ``h``, ``R``,
    ``iso``, ``cycles`` and the node fields ``W``, ``V`` (``[.., 3]``), ``f`` and ``chi``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ----------------------------------------------------------------------------- plumbing
def _ws_bytes(stage: int, R: int = 0, n: int = 0, m: int = 0) -> int:
    need = int(N.lib().slg_mesh_ws_bytes(stage, R, n, m))
    if need < 0:
        CL._raise(-need)
    return need


def _ws(stage: int, device, R: int = 0, n: int = 0, m: int = 0) -> torch.Tensor:
    return torch.empty(_ws_bytes(stage, R, n, m), dtype=torch.uint8, device=device)


def _header(ws: torch.Tensor):
    """The workspace's header on the host (synchronises the stream)."""
    return np.frombuffer(ws[:_HDR.itemsize].cpu().numpy().tobytes(), dtype=_HDR)[0]


def _check_status(hdr, what: str) -> None:
    status = int(hdr["status"])
    if status & N.FILTER_BAD_NONFINITE:
        raise ValueError(f"{what}: the cloud holds a NaN or infinite coordinate or normal")
    if status & N.FILTER_BAD_EXTENT:
        raise ValueError(f"{what}: the cloud's bounding box has no extent (or one that overflows)")


def _set_header(ws, R: int, origin, h: float, iso: float, stream) -> None:
    o = (N.c_dbl * 3)(*[float(v) for v in origin])
    CL._raise(N.lib().slg_mesh_set_header(E._vp(ws), int(R), o, float(h), float(iso), E._stream(stream)))


def _field(t, what: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.ndim >= 3
            and t.shape[0] == t.shape[1] == t.shape[2] and t.shape[0] >= 2):
        raise ValueError(f"{what} must be a device float64 [R+1, R+1, R+1] tensor")
    return t.contiguous()


def check_depth(depth) -> int:
    depth = int(depth)
    if depth < MIN_DEPTH:
        raise ValueError(f"depth must be at least {MIN_DEPTH}, not {depth}")
    if depth > MAX_DEPTH:
        raise ValueError(f"depth {depth} is above the dense grid's limit of {MAX_DEPTH} "
                         f"({(1 << MAX_DEPTH) + 1}^3 nodes; the adaptive octree stays in the reference)")
    return depth


def workspace_bytes(depth: int, n_points: int = 0) -> int:
    """Bytes :func:`poisson_grid` holds at depth ``depth``: the six node arrays ``W``, ``V``, ``f``,
    ``chi`` (``48 (R+1)^3``) plus the largest stage's scratch (``slg_mesh_ws_bytes``)."""
    return _ws_bytes(N.MESH_WS_ALL, 1 << check_depth(depth), int(n_points))


# ----------------------------------------------------------------------------- the stages
def solve_poisson(f, h: float, cycles: int = DEFAULT_CYCLES, stream=None) -> torch.Tensor:
    """``cycles`` V(2,2) cycles from 0 for the 7-point Laplacian of ``chi`` = ``f`` with ``chi = 0``
    on the boundary nodes; ``f`` is a node field of a grid with ``R`` a power of two, 4..1024."""
    f = _field(f, "f")
    R = f.shape[0] - 1
    if f.ndim != 3 or R < 4 or R & (R - 1) or R > 1 << MAX_DEPTH:
        raise ValueError("solve_poisson: f must be [R+1]^3 with R a power of two in 4..1024")
    if int(cycles) < 0 or not (float(h) > 0.0 and np.isfinite(h)):
        raise ValueError("solve_poisson: cycles must be >= 0 and h finite and > 0")
    with torch.cuda.device(f.device):
        ws = _ws(N.MESH_WS_SOLVE, f.device, R)
        _set_header(ws, R, (0.0, 0.0, 0.0), h, 0.0, stream)
        chi = torch.empty_like(f)
        CL._raise(N.lib().slg_mesh_solve(E._vp(f), R, int(cycles), E._vp(ws), ws.numel(), E._vp(chi), E._stream(stream)))
    return chi


def _extract(ws, chi, W, R, stream, what="extract_isosurface"):
    """count -> header -> allocate -> emit, on a workspace whose header is set."""
    lib, dev = N.lib(), chi.device
    CL._raise(lib.slg_mesh_count(E._vp(chi), R, E._vp(ws), ws.numel(), E._stream(stream)))
    hdr = _header(ws)
    _check_status(hdr, what)
    nv, nt = int(hdr["nV"]), int(hdr["nT"])
    if nv >= 1 << 31:
        raise ValueError(f"the surface has {nv} vertices: 2^31 or more do not fit int32 triangles")
    vert = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    dens = torch.empty(nv, dtype=torch.float64, device=dev) if W is not None else None
    if nv or nt:
        CL._raise(lib.slg_mesh_emit(E._vp(chi), E._vp(W), R, E._vp(ws), ws.numel(), E._vp(vert), nv, E._vp(dens),
                                    E._vp(tris), nt, E._stream(stream)))
    return TriangleMesh(vert, tris, dens), hdr


def extract_isosurface(chi, iso: float, origin, h: float, weights=None, stream=None) -> TriangleMesh:
    """Marching tetrahedra of the node field ``chi`` (``[R+1]^3``, ``R`` in 1..1024) at ``iso``: a node
    is inside when ``chi < iso``.  Vertices in ascending (owner node, edge type), triangles in
    ascending (cell, tetrahedron, triangle) wound so that ``(b - a) x (c - a)`` points outward;
    ``densities`` = trilinear ``weights`` at the vertices when given."""
    chi = _field(chi, "chi")
    R = chi.shape[0] - 1
    if chi.ndim != 3 or R > 1 << MAX_DEPTH:
        raise ValueError("extract_isosurface: chi must be [R+1]^3 with R in 1..1024")
    if weights is not None:
        weights = _field(weights, "weights")
        if weights.shape != chi.shape:
            raise ValueError("extract_isosurface: weights and chi differ in shape")
    with torch.cuda.device(chi.device):
        ws = _ws(N.MESH_WS_EXTRACT, chi.device, R)
        _set_header(ws, R, origin, h, iso, stream)
        return _extract(ws, chi, weights, R, stream)[0]


class _Stages:
    """HIP events around the stages of :func:`poisson_grid` when a ``timings`` dict is asked for."""

    def __init__(self, timings, stream):
        self.timings, self.stream, self.marks = timings, stream, []

    def mark(self, name):
        if self.timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(self.stream if self.stream is not None else torch.cuda.current_stream())
            self.marks.append((name, ev))

    def close(self):
        if self.timings is not None:
            self.marks[-1][1].synchronize()
            for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
                self.timings[name + "_ms"] = a.elapsed_time(b)


def poisson_grid(pc, depth: int = 8, scale: float = 1.1, cycles: int = DEFAULT_CYCLES, return_field: bool = False,
                 stream=None, timings=None):
    """The watertight mesh of an oriented cloud: a :class:`TriangleMesh` with ``densities`` (and a
    :class:`PoissonField` with ``return_field``).  ``2 <= depth <= 10``, ``scale >= 1``.  Raises
    ``ValueError`` for a cloud without normals, a non-finite coordinate or normal, a box without
    extent, or when :func:`workspace_bytes` exceeds the device's free memory.  ``timings``: a dict that
    gets the stages' times in ms by HIP events (``grid``, ``splat``, ``divergence``, ``solve``, ``iso``,
    ``extract``: the count, the header's read-back, the allocation and the emit)."""
    depth = check_depth(depth)
    if not (float(scale) >= 1.0 and np.isfinite(scale)):
        raise ValueError(f"scale must be finite and >= 1, not {scale}")
    if int(cycles) < 0:
        raise ValueError("cycles must be >= 0")
    pc = CL.as_point_cloud(pc)
    if not pc.has_points():
        raise ValueError("Point cloud is empty.")
    if not pc.has_normals():
        raise ValueError("poisson_grid: the cloud has no normals (estimate and orient them first)")
    xyz, nrm = CL._check_xyz(pc.xyz), pc.normals.contiguous()
    n, dev, R = xyz.shape[0], xyz.device, 1 << depth
    lib = N.lib()
    with torch.cuda.device(dev):
        need, free = workspace_bytes(depth, n), int(torch.cuda.mem_get_info(dev)[0])
        if need > free:
            raise ValueError(f"poisson_grid: depth {depth} needs {need} bytes, the device has {free} free")
        st = E._stream(stream)
        ws = torch.empty(need - 48 * (R + 1) ** 3, dtype=torch.uint8, device=dev)
        n1 = R + 1
        W = torch.empty((n1, n1, n1), dtype=torch.float64, device=dev)
        V = torch.empty((n1, n1, n1, 3), dtype=torch.float64, device=dev)
        f, chi = torch.empty_like(W), torch.empty_like(W)
        stages = _Stages(timings, stream)
        stages.mark("start")
        CL._raise(lib.slg_mesh_grid(E._vp(xyz), n, depth, float(scale), E._vp(ws), ws.numel(), st))
        stages.mark("grid")
        CL._raise(lib.slg_mesh_splat(E._vp(xyz), E._vp(nrm), n, R, E._vp(ws), ws.numel(), E._vp(W), E._vp(V), st))
        stages.mark("splat")
        CL._raise(lib.slg_mesh_divergence(E._vp(V), R, E._vp(ws), E._vp(f), st))
        stages.mark("divergence")
        CL._raise(lib.slg_mesh_solve(E._vp(f), R, int(cycles), E._vp(ws), ws.numel(), E._vp(chi), st))
        stages.mark("solve")
        CL._raise(lib.slg_mesh_iso(E._vp(chi), E._vp(xyz), n, E._vp(ws), ws.numel(), st))
        stages.mark("iso")
        mesh, hdr = _extract(ws, chi, W, R, stream, "poisson_grid")
        stages.mark("extract")
        stages.close()
    if not return_field:
        return mesh
    return mesh, PoissonField(origin=tuple(float(v) for v in hdr["origin"]), h=float(hdr["h"]), R=R, iso=float(hdr["iso"]),
                              cycles=int(cycles), W=W, V=V, f=f, chi=chi)


def sample_field(field, points, origin, h: float, stream=None) -> torch.Tensor:
    """Trilinear ``field`` at ``points`` (device float64 ``[n, 3]``), the rule of the iso value and
    of the densities."""
    field = _field(field, "field")
    pts = CL._check_xyz(points)
    R = field.shape[0] - 1
    with torch.cuda.device(field.device):
        ws = _ws(N.MESH_WS_GRID, field.device, 0, 1)
        _set_header(ws, R, origin, h, 0.0, stream)
        out = torch.empty(len(pts), dtype=torch.float64, device=field.device)
        CL._raise(N.lib().slg_mesh_sample(E._vp(field), E._vp(pts), len(pts), E._vp(ws), E._vp(out), E._stream(stream)))
    return out


# ----------------------------------------------------------------------------- trim, normals, STL
def quantile(values, q: float, stream=None) -> float:
    """``np.quantile(values, q)`` (NumPy's default linear rule) of a device float64 vector, bit for
    bit: a radix sort and the interpolation on the device."""
    if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float64 and values.ndim == 1):
        raise ValueError("quantile takes a device float64 vector")
    if values.numel() == 0:
        raise ValueError("quantile of an empty vector")
    if not 0.0 <= float(q) <= 1.0:
        raise ValueError("Quantiles must be in the range [0, 1]")
    values = values.contiguous()
    with torch.cuda.device(values.device):
        ws = _ws(N.MESH_WS_QUANTILE, values.device, 0, values.numel())
        CL._raise(N.lib().slg_mesh_quantile(E._vp(values), values.numel(), float(q), E._vp(ws), ws.numel(),
                                            E._stream(stream)))
        return float(_header(ws)["thr"])


def remove_vertices_by_mask(mesh: TriangleMesh, mask, stream=None) -> TriangleMesh:
    """Open3D ``remove_vertices_by_mask``: a new mesh without the vertices where ``mask`` is set and
    without every triangle that had such a corner, renumbered, order preserved.  Triangle normals
    are not carried over."""
    nv, nt = len(mesh.vertices), len(mesh.triangles)
    if not isinstance(mask, torch.Tensor):
        mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, bool)))
    if mask.numel() != nv:
        raise ValueError("remove_vertices_by_mask: the mask must hold one entry per vertex")
    if nv == 0:
        return TriangleMesh(mesh.vertices, mesh.triangles, mesh.densities)
    dev = mesh.vertices.device
    m8 = mask.to(device=dev).reshape(-1).ne(0).to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        ws = _ws(N.MESH_WS_REMOVE, dev, 0, nv, nt)
        vert, tris = torch.empty_like(mesh.vertices), torch.empty_like(mesh.triangles)
        dens = torch.empty_like(mesh.densities) if mesh.densities is not None else None
        CL._raise(N.lib().slg_mesh_remove(E._vp(mesh.vertices), E._vp(mesh.densities), nv, E._vp(mesh.triangles), nt,
                                          E._vp(m8), E._vp(ws), ws.numel(), E._vp(vert), E._vp(dens), E._vp(tris),
                                          E._stream(stream)))
        hdr = _header(ws)
    kv, kt = int(hdr["nV"]), int(hdr["nT"])
    return TriangleMesh(vert[:kv], tris[:kt], dens[:kv] if dens is not None else None)


def compute_triangle_normals(mesh: TriangleMesh, stream=None) -> TriangleMesh:
    """Sets ``mesh.triangle_normals``: unit ``(b - a) x (c - a)`` in float64, ``(0, 0, 0)`` for a
    zero-area triangle.  Returns the mesh."""
    nt = len(mesh.triangles)
    out = torch.empty((nt, 3), dtype=torch.float64, device=mesh.vertices.device)
    if nt:
        with torch.cuda.device(out.device):
            CL._raise(N.lib().slg_mesh_triangle_normals(E._vp(mesh.vertices), E._vp(mesh.triangles), nt, E._vp(out),
                                                        E._stream(stream)))
    mesh.triangle_normals = out
    return mesh


def stl_records(mesh: TriangleMesh, stream=None) -> torch.Tensor:
    """The 50-byte binary STL records of the triangles, packed on the device: uint8 ``[T, 50]``."""
    if mesh.triangle_normals is None:
        compute_triangle_normals(mesh, stream)
    nt = len(mesh.triangles)
    rec = torch.empty((nt, 50), dtype=torch.uint8, device=mesh.vertices.device)
    if nt:
        with torch.cuda.device(rec.device):
            CL._raise(N.lib().slg_mesh_stl_pack(E._vp(mesh.vertices), E._vp(mesh.triangles), E._vp(mesh.triangle_normals),
                                                nt, E._vp(rec), E._stream(stream)))
    return rec


def check_stl_path(path) -> None:
    if os.path.splitext(os.fspath(path))[1].lower() != ".stl":
        raise ValueError(f"{path}: only binary .stl is written (mesh PLY/OBJ and ASCII STL stay in the reference)")


def write_stl(path, mesh: TriangleMesh, stream=None) -> None:
    """Binary STL: an 80-byte header, the triangle count, then :func:`stl_records`."""
    check_stl_path(path)
    rec = stl_records(mesh, stream).cpu().numpy()
    with open(path, "wb") as fh:
        fh.write(STL_HEADER)
        fh.write(struct.pack("<I", len(rec)))
        fh.write(rec.tobytes())


def read_stl(path):
    """``(normals float32 [T, 3], corners float32 [T, 3, 3])`` of a binary STL."""
    with open(path, "rb") as fh:
        data = fh.read()
    (nt,) = struct.unpack_from("<I", data, 80)
    if len(data) != 84 + 50 * nt:
        raise ValueError(f"{path}: {len(data)} bytes, the header promises {84 + 50 * nt}")
    rec = np.frombuffer(data, dtype=np.dtype([("f", "<f4", 12), ("a", "<u2")]), offset=84, count=nt)
    return rec["f"][:, :3].copy(), rec["f"][:, 3:].reshape(nt, 3, 3).copy()


# ----------------------------------------------------------------------------- post-processing
# What the device takes of the reference's MeshLab step (server/processing.py:742-787): vertex
# adjacency, Laplacian / Taubin smoothing and hole closing (csrc/cloud_meshpost.hip).  Our rules,
# restated in tests/meshpost_ref.py and equal to it bit for bit; parity with MeshLab / VCGlib is
# unpinned.  Quadric edge-collapse decimation follows further down.
_POST_HDR = np.dtype([("status", "<i4"), ("R", "<i4"), ("nV", "<i8"), ("nT", "<i8"), ("unused", "<f8", 13),
                      ("stats", "<i8", 8)])
MIN_HOLE_SIZE, MAX_HOLE_SIZE = 3, N.MESH_HOLES_MAX_SIZE
TAUBIN_LAMBDA, TAUBIN_MU = 0.5, -0.53


class MeshAdjacency:
    """The connectivity of a mesh in HBM: ``offsets`` int64 ``[V+1]`` and ``neighbours`` int32 (the
    unique neighbours of every vertex, ascending), ``boundary`` uint8 ``[V]`` (1: an endpoint of a
    boundary edge) and the boundary CSR ``boundary_offsets`` / ``boundary_neighbours`` (a boundary
    vertex's neighbours along boundary edges in either direction, ascending)."""

    def __init__(self, offsets, neighbours, boundary, boundary_offsets, boundary_neighbours):
        self.offsets, self.neighbours, self.boundary = offsets, neighbours, boundary
        self.boundary_offsets, self.boundary_neighbours = boundary_offsets, boundary_neighbours


def _post_mesh(mesh, what: str):
    v, t = mesh.vertices, mesh.triangles
    if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 and v.ndim == 2 and v.shape[1] == 3):
        raise ValueError(f"{what}: vertices must be a device float64 [V, 3] tensor")
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.ndim == 2 and t.shape[1] == 3):
        raise ValueError(f"{what}: triangles must be a device int32 [T, 3] tensor")
    if len(v) >= 1 << 31 or 3 * len(t) > 1 << 30:
        raise ValueError(f"{what}: 2^31 vertices or more, or more than 2^30 directed triangle edges")
    return v.contiguous(), t.contiguous()


def _post_ws(stage: int, device, nv: int, nt: int) -> torch.Tensor:
    need = int(N.lib().slg_mesh_post_ws_bytes(stage, nv, nt))
    if need < 0:
        CL._raise(-need)
    return torch.empty(need, dtype=torch.uint8, device=device)


def _post_header(ws, what: str):
    hdr = np.frombuffer(ws[:_POST_HDR.itemsize].cpu().numpy().tobytes(), dtype=_POST_HDR)[0]
    if int(hdr["status"]) & N.FILTER_BAD_INDEX:
        raise IndexError(f"{what}: a triangle index lies outside 0 .. V - 1")
    return hdr


def vertex_adjacency(mesh: TriangleMesh, stream=None) -> MeshAdjacency:
    """The :class:`MeshAdjacency` of ``mesh``.  The six directed pairs of every triangle as 64-bit
    keys ``src << 32 | dst``: radix sort, unique, scan.  An unreferenced vertex has an empty row, a
    degenerate triangle gives no self-pair.  A triangle's edge ``(a, b)`` in winding order is a
    boundary edge iff ``(b, a)`` is no triangle's edge in winding order.  Our rule;
    ``IndexError`` for a triangle index outside ``0 .. V - 1``."""
    vert, tris = _post_mesh(mesh, "vertex_adjacency")
    nv, nt, dev = len(vert), len(tris), vert.device
    i64 = dict(dtype=torch.int64, device=dev)
    if nv == 0 or nt == 0:
        return MeshAdjacency(torch.zeros(nv + 1, **i64), torch.empty(0, dtype=torch.int32, device=dev),
                             torch.zeros(nv, dtype=torch.uint8, device=dev), torch.zeros(nv + 1, **i64),
                             torch.empty(0, dtype=torch.int32, device=dev))
    lib, st = N.lib(), E._stream(stream)
    with torch.cuda.device(dev):
        ws = _post_ws(N.MESH_WS_ADJACENCY, dev, nv, nt)
        CL._raise(lib.slg_mesh_adjacency_count(E._vp(tris), nt, nv, E._vp(ws), ws.numel(), st))
        hdr = _post_header(ws, "vertex_adjacency")
        ne, nb = int(hdr["nV"]), int(hdr["nT"])
        adj = MeshAdjacency(torch.empty(nv + 1, **i64), torch.empty(ne, dtype=torch.int32, device=dev),
                            torch.empty(nv, dtype=torch.uint8, device=dev), torch.empty(nv + 1, **i64),
                            torch.empty(nb, dtype=torch.int32, device=dev))
        CL._raise(lib.slg_mesh_adjacency_emit(nt, nv, E._vp(ws), ws.numel(), E._vp(adj.offsets), E._vp(adj.neighbours), ne,
                                              E._vp(adj.boundary), E._vp(adj.boundary_offsets),
                                              E._vp(adj.boundary_neighbours), nb, st))
    return adj


def _check_iterations(iterations, what: str) -> int:
    if isinstance(iterations, float) and not iterations.is_integer():
        raise ValueError(f"{what}: iterations must be a whole number, not {iterations}")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"{what}: iterations must be >= 0, not {iterations}")
    return iterations


def _check_adjacency(adj, vert, what: str):
    """A caller's :class:`MeshAdjacency` must be this mesh's: the kernel gathers by its indices."""
    nv, dev = len(vert), vert.device
    parts = (("offsets", adj.offsets, torch.int64, nv + 1), ("boundary_offsets", adj.boundary_offsets, torch.int64, nv + 1),
             ("boundary", adj.boundary, torch.uint8, nv), ("neighbours", adj.neighbours, torch.int32, None),
             ("boundary_neighbours", adj.boundary_neighbours, torch.int32, None))
    for name, t, dtype, count in parts:
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and t.ndim == 1 and t.is_contiguous()
                and (count is None or t.numel() == count)):
            raise ValueError(f"{what}: adjacency.{name} must be a contiguous {dtype} vector on {dev}"
                             + (f" of {count} entries (the mesh has {nv} vertices)" if count is not None else ""))
    ends = torch.stack([adj.offsets[0], adj.offsets[-1], adj.boundary_offsets[0], adj.boundary_offsets[-1]]).tolist()
    if ends != [0, adj.neighbours.numel(), 0, adj.boundary_neighbours.numel()]:
        raise ValueError(f"{what}: the adjacency's offsets do not span its neighbour lists")
    for name, t in (("neighbours", adj.neighbours), ("boundary_neighbours", adj.boundary_neighbours)):
        if t.numel() and not (0 <= int(t.min()) and int(t.max()) < nv):
            raise ValueError(f"{what}: adjacency.{name} holds an index outside 0 .. {nv - 1}: it belongs to another mesh")
    return adj


def _smooth(mesh, passes, what, adjacency, stream):
    """``passes``: the (mode, factor) of every Jacobi pass, one launch each over ping-pong buffers."""
    vert, _ = _post_mesh(mesh, what)
    cur = vert.clone()
    if len(vert) and passes:
        adj = _check_adjacency(adjacency, vert, what) if adjacency is not None else vertex_adjacency(mesh, stream)
        lib, st = N.lib(), E._stream(stream)
        with torch.cuda.device(vert.device):
            nxt = torch.empty_like(cur)
            for mode, factor in passes:
                CL._raise(lib.slg_mesh_smooth_pass(E._vp(cur), E._vp(nxt), len(cur), E._vp(adj.offsets), E._vp(adj.neighbours),
                                                   E._vp(adj.boundary), E._vp(adj.boundary_offsets),
                                                   E._vp(adj.boundary_neighbours), mode, float(factor), st))
                cur, nxt = nxt, cur
    return TriangleMesh(cur, mesh.triangles, mesh.densities)


def smooth_laplacian(mesh: TriangleMesh, iterations: int, adjacency: MeshAdjacency | None = None, stream=None) -> TriangleMesh:
    """``iterations`` Jacobi passes of the umbrella operator: ``p' = (p + s) / (c + 1)`` with ``s``
    the sum over the neighbour set ``N(v)`` in ascending index, ``((q0 + q1) + q2) + ..``, and
    ``c = |N(v)|``; ``c == 0`` leaves ``p``.  ``N(v)`` is the adjacency row of an interior vertex
    and the boundary row of a boundary vertex, which so slides along the boundary (VCGlib's rule as
    we recall it; parity with MeshLab is unpinned).  A new mesh: ``triangles`` and ``densities`` are
    carried over, ``triangle_normals`` is ``None``.  ``ValueError`` for ``iterations < 0``."""
    iterations = _check_iterations(iterations, "smooth_laplacian")
    return _smooth(mesh, [(N.MESH_SMOOTH_LAPLACIAN, 0.0)] * iterations, "smooth_laplacian", adjacency, stream)


def smooth_taubin(mesh: TriangleMesh, iterations: int, lam: float = TAUBIN_LAMBDA, mu: float = TAUBIN_MU,
                  adjacency: MeshAdjacency | None = None, stream=None) -> TriangleMesh:
    """``iterations`` Taubin iterations, two Jacobi passes each: ``m = s / c``,
    ``p' = p + (m - p) * lam``, then the same with ``mu`` (MeshLab's default of 10 is 20 passes);
    ``s``, ``c`` and ``N(v)`` as in :func:`smooth_laplacian`.  Our rule, MeshLab parity unpinned.
    ``ValueError`` for ``iterations < 0`` or a ``lam`` / ``mu`` that is not finite."""
    iterations = _check_iterations(iterations, "smooth_taubin")
    if not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError(f"smooth_taubin: lam and mu must be finite, not {lam}, {mu}")
    return _smooth(mesh, [(N.MESH_SMOOTH_STEP, lam), (N.MESH_SMOOTH_STEP, mu)] * iterations, "smooth_taubin", adjacency,
                   stream)


def check_hole_size(max_size) -> int:
    max_size = int(max_size)
    if not MIN_HOLE_SIZE <= max_size <= MAX_HOLE_SIZE:
        raise ValueError(f"max_size must be in {MIN_HOLE_SIZE}..{MAX_HOLE_SIZE} on the device (one wavefront per loop), "
                         f"not {max_size}")
    return max_size


_EMPTY_RECORD = dict(boundary_edges=0, closable_loops=0, closable_edges=0, open_by_size_edges=0, blocked_edges=0,
                     new_triangles=0)


def _holes_count(mesh, max_size, what, stream):
    max_size = check_hole_size(max_size)
    vert, tris = _post_mesh(mesh, what)
    if len(vert) == 0 or len(tris) == 0:
        return vert, tris, None, dict(_EMPTY_RECORD)
    with torch.cuda.device(vert.device):
        ws = _post_ws(N.MESH_WS_HOLES, vert.device, len(vert), len(tris))
        CL._raise(N.lib().slg_mesh_holes_count(E._vp(tris), len(tris), len(vert), max_size, E._vp(ws), ws.numel(),
                                               E._stream(stream)))
        hdr = _post_header(ws, what)
    s = hdr["stats"]
    return vert, tris, ws, dict(boundary_edges=int(s[N.MESH_HOLES_STAT_EDGES]), closable_loops=int(s[N.MESH_HOLES_STAT_LOOPS]),
                                closable_edges=int(s[N.MESH_HOLES_STAT_CLOSABLE_EDGES]),
                                open_by_size_edges=int(s[N.MESH_HOLES_STAT_LONG_EDGES]),
                                blocked_edges=int(s[N.MESH_HOLES_STAT_BLOCKED_EDGES]), new_triangles=int(hdr["nT"]))


def boundary_loops(mesh: TriangleMesh, max_size: int = 30, stream=None) -> dict:
    """What :func:`close_holes` would do, as counts: ``boundary_edges``; ``closable_loops`` and the
    ``closable_edges`` on them; ``open_by_size_edges``, the edges whose walk ran ``max_size`` steps
    without coming back (a bounded walk cannot tell where a longer loop ends, so loops left open
    by size are counted by their edges); ``blocked_edges``, those whose walk touched a blocked
    vertex; ``new_triangles``.  ``max_size`` is limited to 3..64 on the device (``ValueError``)."""
    return _holes_count(mesh, max_size, "boundary_loops", stream)[3]


def close_holes(mesh: TriangleMesh, max_size: int = 30, return_record: bool = False, stream=None):
    """Closes every hole of at most ``max_size`` edges.  The boundary edges ``B`` in ascending key
    order, ``next(a, b)`` the boundary edge from ``b``; a vertex is blocked when its in or out
    degree along ``B`` is not 1 or a directed triangle edge through it occurs twice; a loop of
    ``3 <= L <= max_size`` edges without a blocked vertex is filled by ear clipping: ring
    ``r[0..m-1]`` from the source of the loop's lowest edge in walk order, while ``m > 3`` the ``i``
    with the smallest squared diagonal ``(dx dx + dy dy) + dz dz`` between ``r[i-1]`` and ``r[i+1]``
    (ties to the lowest ``i``) gives ``(r[i+1], r[i], r[i-1])`` and leaves, last ``(r[2], r[1], r[0])``:
    the winding of the fill is the reverse of the boundary's, so it agrees with its neighbours.
    There is no self-intersection and no existing-edge check.  The input triangles come first,
    unchanged, then the new ones in ascending (loop, clip step); vertices and densities are
    unchanged, triangle normals are not carried over.  Our rule, MeshLab parity unpinned.
    ``max_size`` is limited to 3..64 on the device (one wavefront per loop): ``ValueError`` otherwise."""
    vert, tris, ws, rec = _holes_count(mesh, max_size, "close_holes", stream)
    new = rec["new_triangles"]
    out = tris
    if new:
        with torch.cuda.device(vert.device):
            out = torch.empty((len(tris) + new, 3), dtype=torch.int32, device=vert.device)
            out[:len(tris)].copy_(tris)
            CL._raise(N.lib().slg_mesh_holes_emit(E._vp(vert), len(vert), len(tris), E._vp(ws), ws.numel(),
                                                  out.data_ptr() + 12 * len(tris), new, E._stream(stream)))
    closed = TriangleMesh(mesh.vertices, out, mesh.densities)
    return (closed, rec) if return_record else closed


# ----------------------------------------------------------------------------- decimation
# Quadric edge collapse in rounds of independent collapses (csrc/cloud_decimate.hip): our rule,
# restated in tests/decimate_ref.py and equal to it bit for bit; parity with MeshLab / VCGlib is
# unpinned.
DECIMATE_SWEEPS = N.MESH_DECIMATE_SWEEPS
DEFAULT_TARGET_FACES = 50000
_DEC_HDR = np.dtype([("status", "<i4"), ("R", "<i4"), ("nV", "<i8"), ("nT", "<i8"), ("nC", "<i8"), ("applied", "<i8"),
                     ("total", "<i8"), ("unused", "<f8", 10), ("stats", "<i8", 8)])


def check_target_faces(target, what: str = "decimate_quadric") -> int:
    """``target`` as an int when it is a whole number >= 0, else ``ValueError``."""
    try:
        whole = not isinstance(target, bool) and float(target) == int(target)
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or int(target) < 0:
        raise ValueError(f"{what}: target_faces must be a whole number >= 0, not {target!r}")
    return int(target)


def decimate_quadric(mesh: TriangleMesh, target_faces, max_rounds: int = 512, return_record: bool = False, stream=None,
                     timings=None):
    """Quadric edge-collapse decimation to ``target_faces`` triangles, in rounds of independent
    collapses.  Every vertex carries the sum of its triangles' plane quadrics (weight (2 area)^2);
    a round builds the adjacency, refuses the candidate edges ``u < v`` that have both ends on the
    boundary, are not shared by exactly two consistently wound triangles, whose ends share other
    than two neighbours or one of valence below 4, whose placement costs a non-finite amount or
    turns a triangle over; places the rest (a boundary end stays put; else the cheapest of the
    quadric's minimiser when it lies within two edge lengths of the midpoint, ``P[u]``, ``P[v]`` and
    the midpoint, ties to the earliest), ranks them by (cost bits, key), selects in
    ``DECIMATE_SWEEPS`` sweeps those that hold the lowest rank on every vertex of their closed
    neighbourhood, and applies the first ``ceil((T - target) / 2)`` of them in rank order: ``u``
    moves to the placement and takes ``Q[u] + Q[v]``, ``v`` leaves, each collapse removes two
    triangles.  It stops at the target (``T_out`` is ``target`` or ``target - 1``), when no edge is
    valid, or after ``max_rounds`` rounds.  Boundary vertices never move.  A pure function of the
    mesh and the target; our rule, MeshLab parity unpinned.

    A new mesh: the vertices a collapse removed are dropped, all others keep their order (and
    ``densities``), triangles keep their order and are renumbered, ``triangle_normals`` is ``None``.
    With ``return_record`` also a dict: ``faces_in``, ``faces_out``, ``rounds``, ``collapses``,
    ``stop`` ("target", "no_valid_edge" or "max_rounds") and the last round's counts ``boundary``,
    ``nonmanifold``, ``link``, ``valence``, ``flip``, ``nan``, ``valid``, ``selected``.
    ``ValueError`` for a target that is no whole number >= 0 or ``max_rounds < 0``, ``IndexError``
    for a triangle index outside ``0 .. V - 1``.  ``timings``: a list that gets one dict per round
    (``triangles`` and ``candidates`` going in, ``valid``, ``applied``, and ``ms`` by HIP events
    around the round and its header read-back)."""
    target = check_target_faces(target_faces)
    if isinstance(max_rounds, float) and not max_rounds.is_integer() or int(max_rounds) < 0:
        raise ValueError(f"decimate_quadric: max_rounds must be a whole number >= 0, not {max_rounds}")
    max_rounds = int(max_rounds)
    vert, tris = _post_mesh(mesh, "decimate_quadric")
    nv, nt, dev = len(vert), len(tris), vert.device
    rec = dict(faces_in=nt, faces_out=nt, rounds=0, collapses=0, stop="target", **{k: 0 for k in N.MESH_DECIMATE_STATS})
    if nv == 0 or nt == 0:
        out = TriangleMesh(vert.clone(), tris.clone(), None if mesh.densities is None else mesh.densities.clone())
        return (out, rec) if return_record else out
    dens = None if mesh.densities is None else mesh.densities.contiguous()
    lib, st = N.lib(), E._stream(stream)
    with torch.cuda.device(dev):
        need = int(lib.slg_mesh_decimate_ws_bytes(nv, nt))
        if need < 0:
            CL._raise(-need)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def header():
            hdr = np.frombuffer(ws[:_DEC_HDR.itemsize].cpu().numpy().tobytes(), dtype=_DEC_HDR)[0]
            if int(hdr["status"]) & N.FILTER_BAD_INDEX:
                raise IndexError("decimate_quadric: a triangle index lies outside 0 .. V - 1")
            return hdr

        CL._raise(lib.slg_mesh_decimate_init(E._vp(vert), nv, E._vp(tris), nt, E._vp(ws), ws.numel(), st))
        hdr = header()
        alive = nt
        while True:
            if alive <= target:
                rec["stop"] = "target"
                break
            if rec["rounds"] >= max_rounds:
                rec["stop"] = "max_rounds"
                break
            marks = _Stages({} if timings is not None else None, stream)
            marks.mark("start")
            CL._raise(lib.slg_mesh_decimate_round(E._vp(ws), ws.numel(), nv, nt, alive, target, st))
            hdr = header()                     # the one read-back per round: the next round's size, and whether there is one
            marks.mark("round")
            marks.close()
            rec["rounds"] += 1
            rec.update({k: int(hdr["stats"][i]) for i, k in enumerate(N.MESH_DECIMATE_STATS)})
            if timings is not None:
                timings.append(dict(triangles=alive, candidates=int(hdr["nC"]), valid=rec["valid"], applied=int(hdr["applied"]),
                                    ms=marks.timings["round_ms"]))
            alive = int(hdr["nT"])
            if int(hdr["applied"]) == 0:
                rec["stop"] = "no_valid_edge"
                break
        kv = int(hdr["nV"])
        rec.update(faces_out=alive, collapses=int(hdr["total"]))
        v_out = torch.empty((kv, 3), dtype=torch.float64, device=dev)
        t_out = torch.empty((alive, 3), dtype=torch.int32, device=dev)
        d_out = torch.empty(kv, dtype=torch.float64, device=dev) if dens is not None else None
        CL._raise(lib.slg_mesh_decimate_emit(E._vp(ws), ws.numel(), nv, nt, E._vp(dens), E._vp(v_out), E._vp(d_out), kv,
                                             E._vp(t_out), alive, st))
    out = TriangleMesh(v_out, t_out, d_out)
    return (out, rec) if return_record else out


# ----------------------------------------------------------------------------- surface meshing
# The empty-ball triangles of an oriented cloud, radius by radius (csrc/cloud_surface.hip): our
# rule, restated in tests/surface_ref.py and equal to it bit for bit; parity with Open3D's ball
# pivoting is unpinned.
MAX_RADII, MAX_SURFACE_NEIGHBOURS = N.SURFACE_MAX_RADII, N.SURFACE_MAX_NEIGHBOURS
DEFAULT_SURFACE_ROUNDS = 64
_PASS_HDR = np.dtype([("status", "<i4"), ("pad", "<i4"), ("live", "<i8"), ("accepted", "<i8"), ("cursor", "<u8")])


def check_radii(radii, what: str = "ball_pivot") -> list:
    """``radii`` as a list of floats when they are 1 to 8 finite, positive, strictly ascending
    numbers, else ``ValueError``."""
    try:
        rs = [float(r) for r in np.asarray(radii, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: radii must be numbers, not {radii!r}") from None
    if not 1 <= len(rs) <= MAX_RADII:
        raise ValueError(f"{what}: between 1 and {MAX_RADII} radii, not {len(rs)}")
    if not all(np.isfinite(r) and r > 0.0 for r in rs):
        raise ValueError(f"{what}: radii must be finite and > 0, not {rs}")
    if any(b <= a for a, b in zip(rs, rs[1:])):
        raise ValueError(f"{what}: radii must be strictly ascending, not {rs}")
    return rs


def ball_pivot(pc, radii, max_rounds: int = DEFAULT_SURFACE_ROUNDS, return_record: bool = False, stream=None, timings=None):
    """The surface mesh of an oriented cloud: the triangles on which a ball of radius ``r`` rests,
    on the normals' side, with no point inside, for ``r`` in ``radii`` in turn (what Open3D's
    ``create_from_point_cloud_ball_pivoting`` converges to, without its front: our rule,
    DESIGN.md §20, Open3D parity unpinned).

    State across the passes: the directed edges ``taken`` and a flag ``closed`` per vertex.  A pass
    takes every triple ``a < b < c`` of vertices that are not closed with squared sides ``< 4 r^2``
    that is not flat, has a circumradius ``rho <= r``, whose three normals lie on one side of its
    plane (that side gives the winding) and whose ball holds no other point ``j`` with
    ``d2(P[j], o) < r^2 (1 - 2^-30)``; ranks them by ``(bits of rho^2, a, b, c)``; and accepts, in
    rank order, those none of whose directed edges is taken (found in rounds of integer minima,
    at most ``max_rounds``: reaching that raises ``RuntimeError``).  Then ``closed[v]`` iff ``v`` has a
    taken edge and every taken edge at ``v`` has its reverse.  No directed edge is used twice, so
    the mesh is orientable and edge-manifold, and every triangle agrees with its three normals;
    vertex-manifoldness is not promised.

    A :class:`TriangleMesh`: ``vertices`` is the cloud's ``xyz`` (all points, as Open3D keeps them),
    ``triangles`` int32 ``[T, 3]``, the passes in order and within a pass in ascending rank.  With
    ``return_record`` also a list with one dict per radius (``radius``, ``candidates``,
    ``accepted``, ``rounds``).  Fewer than 3 points give an empty mesh without a device call.
    ``ValueError`` for a cloud without normals, bad ``radii`` (:func:`check_radii`), a non-finite
    coordinate, 2^21 or more cells of ``2 r`` on an axis, or a point with more than
    ``MAX_SURFACE_NEIGHBOURS`` open neighbours of higher index within ``2 r`` (the message names
    the radius).  ``timings``: a list that gets one dict per pass with the stages' times in ms by
    HIP events (``grid``, ``count``, ``emit``, ``select``: the rounds with their read-backs,
    ``commit``) beside the record's entries."""
    rs = check_radii(radii)
    if isinstance(max_rounds, float) and not max_rounds.is_integer() or int(max_rounds) < 1:
        raise ValueError(f"ball_pivot: max_rounds must be a whole number >= 1, not {max_rounds}")
    max_rounds = int(max_rounds)
    pc = CL.as_point_cloud(pc)
    if pc.normals is None:
        raise ValueError("ball_pivot: the cloud has no normals (estimate and orient them first)")
    n = len(pc)
    record = [dict(radius=r, candidates=0, accepted=0, rounds=0) for r in rs]
    if n < 3:
        out = TriangleMesh(pc.xyz, torch.zeros((0, 3), dtype=torch.int32, device=pc.xyz.device))
        return (out, record) if return_record else out
    xyz, nrm = CL._check_xyz(pc.xyz), pc.normals.contiguous()
    if nrm.dtype != torch.float64 or nrm.shape != xyz.shape or nrm.device != xyz.device:
        raise ValueError("ball_pivot: normals must be a float64 [n, 3] tensor beside the points")
    dev, lib, st = xyz.device, N.lib(), E._stream(stream)
    parts = []
    with torch.cuda.device(dev):
        gws = CL._workspace(dev, lib.slg_surface_ws_bytes(N.SURFACE_WS_GRID, n, 0, 0))
        closed = torch.zeros(n, dtype=torch.uint8, device=dev)
        taken, n_taken = torch.empty(1, dtype=torch.int64, device=dev), 0
        total = torch.empty(1, dtype=torch.int64, device=dev)
        for rec in record:
            r = rec["radius"]
            marks = _Stages({} if timings is not None else None, stream)
            marks.mark("start")
            CL._raise(lib.slg_surface_begin(E._vp(xyz), n, r, E._vp(gws), gws.numel(), st))
            marks.mark("grid")
            CL._raise(lib.slg_surface_count(E._vp(nrm), E._vp(closed), n, r, E._vp(gws), gws.numel(), E._vp(total), st))
            status = int(gws[:4].view(torch.int32).item())          # synchronises the stream
            if status & N.FILTER_BAD_NONFINITE:
                raise ValueError("ball_pivot: the cloud holds a NaN or infinite coordinate")
            if status & N.FILTER_BAD_EXTENT:
                raise ValueError(f"ball_pivot: the cloud spans 2^21 or more cells of twice the radius {r!r} on an axis")
            if status & N.FILTER_BAD_NEIGHBOURS:
                raise ValueError(f"ball_pivot: at radius {r!r} a point has more than {MAX_SURFACE_NEIGHBOURS} open neighbours "
                                 "of higher index within twice the radius (the list is never cut short)")
            nc = int(total.item())
            marks.mark("count")
            if 3 * nc > 1 << 30:
                raise ValueError(f"ball_pivot: {nc} candidate triangles at radius {r!r}: more than 2^30 directed edges")
            rec["candidates"] = nc
            if nc:
                need = int(lib.slg_surface_ws_bytes(N.SURFACE_WS_PASS, n, nc, n_taken))
                if need < 0:
                    CL._raise(-need)
                pws = torch.empty(need, dtype=torch.uint8, device=dev)
                CL._raise(lib.slg_surface_emit(E._vp(nrm), E._vp(closed), n, r, E._vp(gws), gws.numel(), E._vp(taken), n_taken,
                                               E._vp(pws), pws.numel(), nc, st))
                marks.mark("emit")
                while True:
                    if rec["rounds"] >= max_rounds:
                        raise RuntimeError(f"ball_pivot: the selection at radius {r!r} did not end in {max_rounds} rounds")
                    CL._raise(lib.slg_surface_round(E._vp(pws), pws.numel(), n, nc, n_taken, st))
                    hdr = np.frombuffer(pws[:_PASS_HDR.itemsize].cpu().numpy().tobytes(), dtype=_PASS_HDR)[0]
                    rec["rounds"] += 1                 # the one read-back per round: whether there is another
                    if int(hdr["live"]) == 0:
                        break
                marks.mark("select")
                na = rec["accepted"] = int(hdr["accepted"])
                if na:
                    tris = torch.empty((na, 3), dtype=torch.int32, device=dev)
                    merged = torch.empty(n_taken + 3 * na, dtype=torch.int64, device=dev)
                    CL._raise(lib.slg_surface_commit(E._vp(pws), pws.numel(), n, nc, E._vp(taken), n_taken, na, E._vp(tris),
                                                     E._vp(merged), E._vp(closed), st))
                    parts.append(tris)
                    taken, n_taken = merged, n_taken + 3 * na
                marks.mark("commit")
            marks.close()
            if timings is not None:
                timings.append(dict(radius=r, candidates=nc, accepted=rec["accepted"], rounds=rec["rounds"],
                                    **{k[:-3]: v for k, v in marks.timings.items()}))
        triangles = torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.int32, device=dev)
    out = TriangleMesh(xyz, triangles)
    return (out, record) if return_record else out


# ----------------------------------------------------------------------------- banded cascade
# The second watertight rule (csrc/cloud_band.hip): a dense solve at a base depth, finer levels only
# in blocks of 8^3 cells near the points.  Our rule, restated in tests/band_ref.py and equal to it
# bit for bit; parity with Open3D's octree solver is unpinned.
BAND_MIN_DEPTH, BAND_MAX_DEPTH, BAND_MAX_BASE_DEPTH = N.BAND_MIN_DEPTH, N.BAND_MAX_DEPTH, N.BAND_MAX_BASE_DEPTH
# Jacobi sweeps per banded level: 16 bring the mean radial error on the test spheres within 1.053 of
# the dense solve's at the same depth, 8 within 1.12, 32 within 1.017 (tests/test_band_ref.py)
DEFAULT_BAND_SWEEPS = 16
_BAND_HDR = np.dtype([*[(k, _HDR.fields[k][0]) for k in _HDR.names], ("unused", "<f8", 7), ("stats", "<i8", 8),
                      ("pad", "<u1", 64)])                           # one header is N.MESH_HDR_BYTES: an array of them reads as one


def check_band_depth(depth, base_depth=None):
    """``(depth, base_depth)`` of :func:`poisson_band`: ``3 <= depth <= 12``; ``base_depth`` defaults to
    ``min(8, depth - 1)`` and lies in ``2 .. min(10, depth - 1)``.  ``ValueError`` otherwise."""
    depth = int(depth)
    if not BAND_MIN_DEPTH <= depth <= BAND_MAX_DEPTH:
        raise ValueError(f"depth must be in {BAND_MIN_DEPTH}..{BAND_MAX_DEPTH} for the banded mesher, not {depth}")
    base = min(8, depth - 1) if base_depth is None else int(base_depth)
    if not MIN_DEPTH <= base <= min(BAND_MAX_BASE_DEPTH, depth - 1):
        raise ValueError(f"base_depth must be in {MIN_DEPTH}..{min(BAND_MAX_BASE_DEPTH, depth - 1)} at depth {depth}, not {base}")
    return depth, base


def _band_ws_bytes(stage: int, R: int = 8, n: int = 0, n_blocks: int = 0) -> int:
    need = int(N.lib().slg_band_ws_bytes(stage, R, n, n_blocks))
    if need < 0:
        CL._raise(-need)
    return need


def _band_table_bytes(depth: int, base: int) -> int:
    """Headers, seed, active and table of every banded level and the block stage's scratch."""
    sizes = [((1 << l) // N.BAND_BLOCK + 1) ** 3 for l in range(base + 1, depth + 1)]
    return sum(256 + 6 * m for m in sizes) + _band_ws_bytes(N.BAND_WS_BLOCKS, 1 << depth)


def band_workspace_bytes(record: dict) -> int:
    """Bytes :func:`poisson_band` holds at most, from a record's ``depth``, ``base_depth``, ``points``
    and per-level ``node_blocks``: the dense base level (:func:`workspace_bytes`), the block tables of
    every level, per stored block its id and 512 incident bytes, and the larger of a level's solve
    (``W``, ``V``, ``f`` and two ``chi``, 56 bytes per stored node, the sort's scratch and the
    parent's ``chi``) and the finest level's extraction (``W``, ``chi``, the masks, counts and scans)."""
    depth, base, n = int(record["depth"]), int(record["base_depth"]), int(record["points"])
    blocks = [int(lv["node_blocks"]) for lv in record["levels"]]
    fixed = workspace_bytes(base, n) + _band_table_bytes(depth, base) + sum(516 * b for b in blocks)
    sort = _band_ws_bytes(N.BAND_WS_SPLAT, n=n)
    solve = max(56 * 512 * b + sort + 8 * 512 * p for b, p in zip(blocks, [0, *blocks]))
    extract = (16 * 512 * blocks[-1] + _band_ws_bytes(N.BAND_WS_ISO, n=n)
               + (_band_ws_bytes(N.BAND_WS_EXTRACT, n_blocks=blocks[-1]) if blocks[-1] else 0))
    return fixed + max(solve, extract)


def poisson_band(pc, depth: int = 11, base_depth=None, sweeps: int = DEFAULT_BAND_SWEEPS, scale: float = 1.1,
                 cycles: int = DEFAULT_CYCLES, return_record: bool = False, stream=None, timings=None,
                 return_fields: bool = False):
    """The watertight mesh of an oriented cloud by the banded cascade, for depths the
    dense grid cannot hold: a :class:`TriangleMesh` with ``densities``.  :func:`poisson_grid`'s solve at
    ``base_depth`` carries the far field.  Every level ``l`` above it exists only in blocks of 8^3
    cells: a block is seeded when a point's cell lies in it and active when it or one of its 26
    neighbours is seeded; a node is a band node when an incident cell is active and interior when all
    8 are.  The level splats and takes the divergence by §16's rules, starts from
    ``0.125 * P(chi of l - 1)`` (the splat is not normalised by the cell volume) and runs ``sweeps``
    Jacobi sweeps in which interior nodes update and every other node keeps its value.  The iso value
    is §16's on the finest level, and marching tetrahedra run over its active cells only: vertices
    in ascending (block, local node, edge type), triangles in ascending (block, local cell,
    tetrahedron, triangle).  Our rule, Open3D parity unpinned; a pure function of the cloud.

    The mesh is closed wherever the iso surface stays inside the band (8 to 16 finest cells from a
    point); where Poisson would close a hole far from every point it ends at the band's edge in a
    boundary loop, which is what the density trim of the callers removes from a dense solve
    (:func:`boundary_loops` counts the open edges, :func:`close_holes` closes short loops).

    With ``return_record`` also a dict: ``depth``, ``base_depth``, ``sweeps``, ``points``, per banded
    level (``levels``) its ``level``, ``seeded_blocks``, ``active_blocks``, ``node_blocks``,
    ``band_nodes`` and ``interior_nodes``, and ``workspace_bytes`` (:func:`band_workspace_bytes`).  With
    ``return_fields`` also a list with one dict per banded level of the device arrays ``table``,
    ``incident``, ``W``, ``V``, ``f``, ``chi`` (node fields are ``[node_blocks, 8, 8, 8]``) and ``iso``.
    ``ValueError`` for bad arguments (:func:`check_band_depth`), a cloud without normals, a
    non-finite coordinate or normal, a box without extent or 2^31 vertices or more; ``MemoryError``,
    naming the bytes, when the workspace exceeds the device's free memory, before the solve is
    launched.  ``timings``: a dict that gets the stages' times in ms by HIP events (``grid``,
    ``blocks`` with its read-back, ``base``, per level ``L<l>_nodes``, ``L<l>_splat``,
    ``L<l>_divergence``, ``L<l>_prolong``, ``L<l>_sweeps``, then ``iso`` and ``extract``)."""
    depth, base = check_band_depth(depth, base_depth)
    if isinstance(sweeps, float) and not sweeps.is_integer() or int(sweeps) < 0:
        raise ValueError(f"poisson_band: sweeps must be a whole number >= 0, not {sweeps}")
    sweeps = int(sweeps)
    if not (float(scale) >= 1.0 and np.isfinite(scale)):
        raise ValueError(f"scale must be finite and >= 1, not {scale}")
    if int(cycles) < 0:
        raise ValueError("cycles must be >= 0")
    pc = CL.as_point_cloud(pc)
    if not pc.has_points():
        raise ValueError("Point cloud is empty.")
    if not pc.has_normals():
        raise ValueError("poisson_band: the cloud has no normals (estimate and orient them first)")
    xyz, nrm = CL._check_xyz(pc.xyz), pc.normals.contiguous()
    n, dev, Rb = xyz.shape[0], xyz.device, 1 << base
    lib, ls = N.lib(), list(range(base + 1, depth + 1))
    u8, f64 = dict(dtype=torch.uint8, device=dev), dict(dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        first = workspace_bytes(base, n) + _band_table_bytes(depth, base)
        free = int(torch.cuda.mem_get_info(dev)[0])
        if first > free:
            raise MemoryError(f"poisson_band: depth {depth} needs {first} bytes for its base level and block tables alone, "
                              f"the device has {free} free")
        st = E._stream(stream)
        ws = torch.empty(workspace_bytes(base, n) - 48 * (Rb + 1) ** 3, **u8)
        hdrs = torch.empty(256 * len(ls), **u8)
        hdr = [hdrs[256 * k:256 * (k + 1)] for k in range(len(ls))]
        bws = torch.empty(_band_ws_bytes(N.BAND_WS_BLOCKS, 1 << depth), **u8)
        stages = _Stages(timings, stream)
        stages.mark("start")
        CL._raise(lib.slg_mesh_grid(E._vp(xyz), n, base, float(scale), E._vp(ws), ws.numel(), st))
        stages.mark("grid")
        seed, active, table = [], [], []
        for k, l in enumerate(ls):
            m = ((1 << l) // N.BAND_BLOCK + 1) ** 3
            seed.append(torch.empty(m, **u8))
            active.append(torch.empty(m, **u8))
            table.append(torch.empty(m, dtype=torch.int32, device=dev))
            CL._raise(lib.slg_band_level(E._vp(ws), Rb, 1 << l, E._vp(hdr[k]), st))
            CL._raise(lib.slg_band_blocks(E._vp(xyz), n, 1 << l, E._vp(hdr[k]), E._vp(seed[k]), E._vp(active[k]),
                                          E._vp(table[k]), E._vp(bws), bws.numel(), st))
        H = np.frombuffer(hdrs.cpu().numpy().tobytes(), dtype=_BAND_HDR)       # the first read-back: the counts
        _check_status(H[0], "poisson_band")
        del bws
        stages.mark("blocks")
        record = dict(depth=depth, base_depth=base, sweeps=sweeps, points=n,
                      levels=[dict(level=l, **{name: int(H[k]["stats"][i]) for i, name in enumerate(N.BAND_STATS)})
                              for k, l in enumerate(ls)])
        nblk = [lv["node_blocks"] for lv in record["levels"]]
        need = record["workspace_bytes"] = band_workspace_bytes(record)
        if need > free:
            raise MemoryError(f"poisson_band: depth {depth} over base {base} needs {need} bytes ({nblk[-1]} stored blocks on "
                              f"the finest level), the device has {free} free")
        n1 = Rb + 1
        W = torch.empty((n1, n1, n1), **f64)
        V = torch.empty((n1, n1, n1, 3), **f64)
        f, chi = torch.empty_like(W), torch.empty_like(W)
        CL._raise(lib.slg_mesh_splat(E._vp(xyz), E._vp(nrm), n, Rb, E._vp(ws), ws.numel(), E._vp(W), E._vp(V), st))
        CL._raise(lib.slg_mesh_divergence(E._vp(V), Rb, E._vp(ws), E._vp(f), st))
        CL._raise(lib.slg_mesh_solve(E._vp(f), Rb, int(cycles), E._vp(ws), ws.numel(), E._vp(chi), st))
        stages.mark("base")
        del W, V, f
        sws = torch.empty(_band_ws_bytes(N.BAND_WS_SPLAT, n=n), **u8)
        parent, fields = (chi, None, 0), []
        for k, l in enumerate(ls):
            R, nb, h, tb = 1 << l, nblk[k], E._vp(hdr[k]), E._vp(table[k])
            ids = torch.empty(nb, dtype=torch.int32, device=dev)
            inc = torch.empty(nb * 512, **u8)
            CL._raise(lib.slg_band_nodes(R, h, E._vp(active[k]), tb, nb, E._vp(ids), E._vp(inc), st))
            stages.mark(f"L{l}_nodes")
            W, V = torch.empty(nb * 512, **f64), torch.empty(nb * 512 * 3, **f64)
            CL._raise(lib.slg_band_splat(E._vp(xyz), E._vp(nrm), n, R, h, E._vp(seed[k]), tb, E._vp(ids), E._vp(inc), nb,
                                         E._vp(sws), sws.numel(), E._vp(W), E._vp(V), st))
            stages.mark(f"L{l}_splat")
            f = torch.empty(nb * 512, **f64)
            CL._raise(lib.slg_band_divergence(E._vp(V), R, h, tb, E._vp(ids), E._vp(inc), nb, E._vp(f), st))
            stages.mark(f"L{l}_divergence")
            u, tmp = torch.empty(nb * 512, **f64), torch.empty(nb * 512, **f64)
            CL._raise(lib.slg_band_prolong(E._vp(parent[0]), E._vp(parent[1]), parent[2], R, h, E._vp(ids), E._vp(inc), nb,
                                           E._vp(u), st))
            stages.mark(f"L{l}_prolong")
            CL._raise(lib.slg_band_smooth(E._vp(f), R, h, tb, E._vp(ids), E._vp(inc), nb, sweeps, E._vp(u), E._vp(tmp), st))
            stages.mark(f"L{l}_sweeps")
            chi = tmp if sweeps & 1 else u
            if return_fields:
                fields.append(dict(level=l, table=table[k], incident=inc.view(nb, 8, 8, 8), W=W.view(nb, 8, 8, 8),
                                   V=V.view(nb, 8, 8, 8, 3), f=f.view(nb, 8, 8, 8), chi=chi.view(nb, 8, 8, 8)))
            parent = (chi, table[k], nb)
            del V, f, u, tmp
        R, nb, h, tb = 1 << depth, nblk[-1], E._vp(hdr[-1]), E._vp(table[-1])
        iws = torch.empty(_band_ws_bytes(N.BAND_WS_ISO, n=n), **u8)
        CL._raise(lib.slg_band_iso(E._vp(chi), E._vp(xyz), n, R, h, tb, nb, E._vp(iws), iws.numel(), st))
        stages.mark("iso")
        ews = torch.empty(_band_ws_bytes(N.BAND_WS_EXTRACT, n_blocks=nb), **u8)
        CL._raise(lib.slg_band_count(E._vp(chi), R, h, tb, E._vp(ids), E._vp(inc), nb, E._vp(ews), ews.numel(), st))
        H = np.frombuffer(hdrs.cpu().numpy().tobytes(), dtype=_BAND_HDR)       # the second read-back: nV, nT and the node counts
        for k in range(len(ls)):
            _check_status(H[k], "poisson_band")
            record["levels"][k].update({name: int(H[k]["stats"][i]) for i, name in enumerate(N.BAND_STATS)})
        nv, nt = int(H[-1]["nV"]), int(H[-1]["nT"])
        if nv >= 1 << 31:
            raise ValueError(f"the surface has {nv} vertices: 2^31 or more do not fit int32 triangles")
        vert = torch.empty((nv, 3), **f64)
        tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        dens = torch.empty(nv, **f64)
        if nv or nt:
            CL._raise(lib.slg_band_emit(E._vp(chi), E._vp(W), R, h, tb, E._vp(ids), E._vp(inc), nb, E._vp(ews), ews.numel(),
                                        E._vp(vert), nv, E._vp(dens), E._vp(tris), nt, st))
        stages.mark("extract")
        stages.close()
    record.update(vertices=nv, triangles=nt)
    out = [TriangleMesh(vert, tris, dens)]
    if return_record:
        out.append(record)
    if return_fields:
        for fl in fields:
            fl["iso"] = float(H[-1]["iso"])
        out.append(fields)
    return out[0] if len(out) == 1 else tuple(out)


# ----------------------------------------------------------------------------- audit and cleanup
# Whether a mesh is closed, manifold, oriented and one piece, its volume and area, and the two
# repairs that follow: keeping the large components, dropping degenerate and duplicated triangles
# and unreferenced vertices (csrc/cloud_audit.hip).  Our rules, restated in tests/audit_ref.py and
# equal to it bit for bit; parity with Open3D / MeshLab is unpinned.  Self-intersection is not tested.
_AUDIT_HDR = np.dtype([("status", "<i4"), ("R", "<i4"), ("nV", "<i8"), ("nT", "<i8"), ("nC", "<i8"), ("largest", "<i8"),
                       ("best", "<u8"), ("unused", "<f8", 10), ("stats", "<i8", 8)])
AUDIT_COUNTS = ("vertices", "triangles", "unreferenced_vertices", "degenerate_triangles", "duplicate_triangles", "edges",
                "boundary_edges", "manifold_edges", "nonmanifold_edges", "inconsistent_edges", "nonmanifold_vertices",
                "components", "largest_component_triangles")
AUDIT_VERDICTS = ("closed", "edge_manifold", "vertex_manifold", "oriented", "watertight")


def _audit_ws(stage: int, device, nv: int, nt: int) -> torch.Tensor:
    need = int(N.lib().slg_audit_ws_bytes(stage, nv, nt))
    if need < 0:
        CL._raise(-need)
    return torch.empty(need, dtype=torch.uint8, device=device)


def _audit_header(ws, what: str):
    hdr = np.frombuffer(ws[:_AUDIT_HDR.itemsize].cpu().numpy().tobytes(), dtype=_AUDIT_HDR)[0]
    if int(hdr["status"]) & N.FILTER_BAD_INDEX:
        raise IndexError(f"{what}: a triangle index lies outside 0 .. V - 1")
    return hdr


def audit_verdict(counts: dict) -> dict:
    """The booleans of :func:`audit` from its counts: ``closed`` (no boundary edge), ``edge_manifold``
    (no edge with three triangles or more), ``vertex_manifold`` (no vertex with two fans), ``oriented``
    (no edge whose two triangles run along it in the same direction) and ``watertight``: all four, no
    degenerate or duplicate triangle and at least one triangle."""
    v = dict(closed=counts["boundary_edges"] == 0, edge_manifold=counts["nonmanifold_edges"] == 0,
             vertex_manifold=counts["nonmanifold_vertices"] == 0, oriented=counts["inconsistent_edges"] == 0)
    v["watertight"] = (all(v.values()) and counts["degenerate_triangles"] == 0 and counts["duplicate_triangles"] == 0
                       and counts["triangles"] > 0)
    return v


def _audit(mesh, what, stream, fans=True, measure=True, timings=None):
    """The steps of the audit: ``(result dict, vertex_class, triangle_class, labels, sizes)``."""
    vert, tris = _post_mesh(mesh, what)
    nv, nt, dev = len(vert), len(tris), vert.device
    res = dict.fromkeys(AUDIT_COUNTS, 0)
    res.update(vertices=nv, triangles=nt, unreferenced_vertices=nv, signed_volume=0.0, area=0.0)
    u8, i32 = dict(dtype=torch.uint8, device=dev), dict(dtype=torch.int32, device=dev)
    if nv == 0 or nt == 0:
        res.update(audit_verdict(res))
        return (res, torch.zeros(nv, **u8), torch.zeros(nt, **u8), torch.full((nt,), -1, **i32),
                torch.zeros(0, dtype=torch.int64, device=dev))
    lib, st = N.lib(), E._stream(stream)
    with torch.cuda.device(dev):
        ws = _audit_ws(N.AUDIT_WS_AUDIT, dev, nv, nt)
        vclass, tclass = torch.empty(nv, **u8), torch.empty(nt, **u8)
        labels = torch.empty(nt, **i32)
        stages = _Stages(timings, stream)
        stages.mark("start")
        CL._raise(lib.slg_audit_edges(E._vp(tris), nt, nv, E._vp(ws), ws.numel(), E._vp(vclass), E._vp(tclass), st))
        stages.mark("edges")
        CL._raise(lib.slg_audit_components_count(nt, nv, E._vp(ws), ws.numel(), E._vp(tclass), E._vp(labels), st))
        hdr = _audit_header(ws, what)             # the first read-back: the status and the component count
        nc = int(hdr["nC"])
        sizes = torch.empty(nc, dtype=torch.int64, device=dev)
        if nc:
            CL._raise(lib.slg_audit_components_emit(nt, nv, E._vp(ws), ws.numel(), E._vp(labels), nc, E._vp(sizes), st))
        stages.mark("components")
        if fans:
            CL._raise(lib.slg_audit_fans(E._vp(tris), nt, nv, E._vp(ws), ws.numel(), E._vp(tclass), E._vp(vclass), st))
        stages.mark("fans")
        if measure:
            mws = _audit_ws(N.AUDIT_WS_MEASURE, dev, nv, nt)
            out = torch.empty(2, dtype=torch.float64, device=dev)
            CL._raise(lib.slg_audit_measure(E._vp(vert), nv, E._vp(tris), nt, E._vp(mws), mws.numel(), E._vp(out), st))
            vol, area = out.cpu().numpy().tolist()
            res.update(signed_volume=vol, area=area)
        if nc or fans:
            hdr = _audit_header(ws, what)         # the second: the largest component and the fan count
        stages.mark("measure")
        stages.close()
    res.update({name: int(hdr["stats"][i]) for i, name in enumerate(N.AUDIT_STATS)})
    res.update(unreferenced_vertices=nv - int(hdr["nV"]), components=nc, largest_component_triangles=int(hdr["largest"]))
    res.update(audit_verdict(res))
    return res, vclass, tclass, labels, sizes


def audit(mesh: TriangleMesh, return_arrays: bool = False, stream=None, timings=None) -> dict:
    """Whether ``mesh`` can be printed, as counts, two measures and a verdict.

    A triangle with two equal indices is degenerate and takes no part in the rest.  Every other
    triangle gives three undirected edges; an edge with one triangle is a boundary edge, with two a
    manifold edge, with three or more a non-manifold edge; a manifold edge whose two triangles run
    along it in the same direction is inconsistent.  Two triangles with the same three indices in any
    winding are duplicates, the one with the lowest index the original.  Triangles that share an
    edge are one component (sharing a vertex is not enough); a vertex is non-manifold when its
    triangles form more than one fan around it (the pinch of two cones, the middle of a bow tie).

    Integer counts: ``vertices``, ``triangles``, ``unreferenced_vertices`` (on no triangle at all),
    ``degenerate_triangles``, ``duplicate_triangles``, ``edges``, ``boundary_edges``, ``manifold_edges``,
    ``nonmanifold_edges``, ``inconsistent_edges``, ``nonmanifold_vertices``, ``components``,
    ``largest_component_triangles``.  Floats: ``signed_volume``, the sum of ``a . (b x c) / 6``
    (positive for a closed mesh wound outwards), and ``area``, both over the triangles that are not
    degenerate, in a fixed order of additions.  Booleans (:func:`audit_verdict`): ``closed``,
    ``edge_manifold``, ``vertex_manifold``, ``oriented`` and ``watertight``.  **Self-intersection is
    not tested** (see :func:`self_intersections`): a watertight verdict says that the surface is a
    closed, oriented 2-manifold, not that it bounds a solid without overlaps.

    ``return_arrays`` adds, on the device: ``vertex_class`` uint8 ``[V]`` (bit 1 referenced, 2 on a
    boundary edge, 4 on a non-manifold edge, 8 on an inconsistent edge, 16 a non-manifold vertex),
    ``triangle_class`` uint8 ``[T]`` (1 degenerate, 2 duplicate), ``labels`` int32 ``[T]`` (the
    component, numbered by first triangle; -1 for a degenerate triangle) and ``sizes`` int64 ``[C]``.
    An empty mesh gives the empty answers without a launch; ``IndexError`` for a triangle index
    outside ``0 .. V - 1``.  Our rule, Open3D parity (``is_watertight`` and its kin) unpinned.
    ``timings``: a dict that gets the stages' times in ms by HIP events (``edges``; ``components`` with
    the first read-back; ``fans``; ``measure`` with its two read-backs)."""
    res, vclass, tclass, labels, sizes = _audit(mesh, "audit", stream, timings=timings)
    if return_arrays:
        res.update(vertex_class=vclass, triangle_class=tclass, labels=labels, sizes=sizes)
    return res


def connected_components(mesh: TriangleMesh, stream=None):
    """``(labels int32 [T], sizes int64 [C])`` on the device: triangles that share an edge are one
    component, whatever the edge's multiplicity or winding; a component's label is its rank by first
    triangle; a degenerate triangle has the label -1.  ``IndexError`` for a bad triangle index."""
    _, _, _, labels, sizes = _audit(mesh, "connected_components", stream, fans=False, measure=False)
    return labels, sizes


def _select(mesh, vert, tris, keep, drop_unreferenced, what, stream):
    """The triangles with ``keep`` set and, with ``drop_unreferenced``, only the vertices they use."""
    nv, nt, dev = len(vert), len(tris), vert.device
    dens = None if mesh.densities is None else mesh.densities.contiguous()
    with torch.cuda.device(dev):
        ws = _audit_ws(N.AUDIT_WS_SELECT, dev, nv, nt)
        v_out, t_out = torch.empty_like(vert), torch.empty_like(tris)
        d_out = torch.empty_like(dens) if dens is not None else None
        CL._raise(N.lib().slg_audit_select(E._vp(vert), E._vp(dens), nv, E._vp(tris), nt, E._vp(keep),
                                           1 if drop_unreferenced else 0, E._vp(ws), ws.numel(), E._vp(v_out), E._vp(d_out),
                                           E._vp(t_out), E._stream(stream)))
        hdr = _audit_header(ws, what)
    kv, kt = int(hdr["nV"]), int(hdr["nT"])
    return TriangleMesh(v_out[:kv], t_out[:kt], d_out[:kv] if d_out is not None else None)


def _keep_components(mesh, choose, what, return_record, stream):
    """``choose(sizes ndarray) -> bool table``: the components to keep."""
    res, _, tclass, labels, sizes = _audit(mesh, what, stream, fans=False, measure=False)
    vert, tris = _post_mesh(mesh, what)
    nv, nt, nc, dev = len(vert), len(tris), res["components"], vert.device
    table = np.ascontiguousarray(choose(sizes.cpu().numpy()), np.uint8) if nc else np.zeros(0, np.uint8)
    if nc and nv and nt:
        with torch.cuda.device(dev):
            keep = torch.empty(nt, dtype=torch.uint8, device=dev)
            tab = torch.from_numpy(table).to(dev)
            CL._raise(N.lib().slg_audit_keep(E._vp(tclass), E._vp(labels), nt, E._vp(tab), nc, 0, E._vp(keep),
                                             E._stream(stream)))
        out = _select(mesh, vert, tris, keep, True, what, stream)
    else:
        out = TriangleMesh(vert[:0].clone(), tris[:0].clone(), None if mesh.densities is None else mesh.densities[:0].clone())
    rec = dict(components_before=nc, components_after=int(table.sum()), triangles_removed=nt - len(out.triangles),
               vertices_removed=nv - len(out.vertices))
    return (out, rec) if return_record else out


def keep_largest_components(mesh: TriangleMesh, count: int = 1, return_record: bool = False, stream=None):
    """A new mesh of the ``count`` components (:func:`connected_components`) with the most triangles,
    ties going to the lower label: their triangles in input order, the vertices they use in input
    order, renumbered, ``densities`` carried, ``triangle_normals`` not.  Degenerate triangles are
    dropped.  With ``return_record`` also a dict: ``components_before``, ``components_after``,
    ``triangles_removed``, ``vertices_removed``.  ``ValueError`` for ``count < 1``."""
    if isinstance(count, bool) or isinstance(count, float) and not count.is_integer() or int(count) < 1:
        raise ValueError(f"keep_largest_components: count must be a whole number >= 1, not {count!r}")
    count = int(count)

    def choose(sizes):
        order = np.argsort(-sizes, kind="stable")[:count]          # descending size, ties to the lower label
        table = np.zeros(len(sizes), np.uint8)
        table[order] = 1
        return table
    return _keep_components(mesh, choose, "keep_largest_components", return_record, stream)


def remove_small_components(mesh: TriangleMesh, min_triangles: int, return_record: bool = False, stream=None):
    """A new mesh of the components with at least ``min_triangles`` triangles, as
    :func:`keep_largest_components` builds it.  ``ValueError`` for ``min_triangles < 0``."""
    if (isinstance(min_triangles, bool) or isinstance(min_triangles, float) and not min_triangles.is_integer()
            or int(min_triangles) < 0):
        raise ValueError(f"remove_small_components: min_triangles must be a whole number >= 0, not {min_triangles!r}")
    min_triangles = int(min_triangles)
    return _keep_components(mesh, lambda sizes: sizes >= min_triangles, "remove_small_components", return_record, stream)


def clean(mesh: TriangleMesh, degenerate: bool = True, duplicates: bool = True, unreferenced: bool = True,
          return_record: bool = False, stream=None):
    """A new mesh without the degenerate triangles, the duplicated triangles (the original of every
    class, the one with the lowest index, stays) and the vertices no remaining triangle uses, each
    as asked for.  Order and ``densities`` are preserved, ``triangle_normals`` is not carried.  With
    ``return_record`` also a dict: ``degenerate_removed``, ``duplicates_removed``, ``vertices_removed``.
    ``IndexError`` for a triangle index outside ``0 .. V - 1``."""
    vert, tris = _post_mesh(mesh, "clean")
    nv, nt, dev = len(vert), len(tris), vert.device
    rec = dict(degenerate_removed=0, duplicates_removed=0, vertices_removed=0)
    dens = mesh.densities
    if nv == 0 or nt == 0:
        kv = 0 if unreferenced else nv
        out = TriangleMesh(vert[:kv].clone(), tris.clone(), None if dens is None else dens[:kv].clone())
        rec["vertices_removed"] = nv - kv
        return (out, rec) if return_record else out
    lib, st = N.lib(), E._stream(stream)
    bits = (N.AUDIT_TRIANGLE_DEGENERATE if degenerate else 0) | (N.AUDIT_TRIANGLE_DUPLICATE if duplicates else 0)
    with torch.cuda.device(dev):
        ws = _audit_ws(N.AUDIT_WS_AUDIT, dev, nv, nt)
        vclass, tclass = torch.empty(nv, dtype=torch.uint8, device=dev), torch.empty(nt, dtype=torch.uint8, device=dev)
        keep = torch.empty(nt, dtype=torch.uint8, device=dev)
        CL._raise(lib.slg_audit_edges(E._vp(tris), nt, nv, E._vp(ws), ws.numel(), E._vp(vclass), E._vp(tclass), st))
        CL._raise(lib.slg_audit_keep(E._vp(tclass), None, nt, None, 0, bits, E._vp(keep), st))
        hdr = _audit_header(ws, "clean")
    out = _select(mesh, vert, tris, keep, unreferenced, "clean", stream)
    stats = dict(zip(N.AUDIT_STATS, (int(s) for s in hdr["stats"])))
    rec.update(degenerate_removed=stats["degenerate_triangles"] if degenerate else 0,
               duplicates_removed=stats["duplicate_triangles"] if duplicates else 0, vertices_removed=nv - len(out.vertices))
    return (out, rec) if return_record else out


def format_audit(a: dict) -> str:
    """One line of an audit: the counts that say something and the verdict."""
    parts = [f"{a['vertices']} vertices", f"{a['triangles']} triangles", f"{a['components']} components "
             f"(largest {a['largest_component_triangles']})", f"{a['boundary_edges']} boundary", f"{a['nonmanifold_edges']} "
             f"non-manifold and {a['inconsistent_edges']} inconsistent edges", f"{a['nonmanifold_vertices']} non-manifold vertices",
             f"{a['degenerate_triangles']} degenerate", f"{a['duplicate_triangles']} duplicate", f"{a['unreferenced_vertices']} "
             f"unreferenced", f"volume {a['signed_volume']:.6g}", f"area {a['area']:.6g}"]
    missing = ["not " + k.replace("_", "-") for k in AUDIT_VERDICTS[:4] if not a[k]]
    verdict = "watertight" if a["watertight"] else "not watertight (" + ", ".join(
        missing or ["degenerate or duplicate triangles, or none at all"]) + ")"
    return ", ".join(parts) + ": " + verdict + "; self-intersection not tested"


# ----------------------------------------------------------------------------- self-intersection
# Which pairs of triangles cross (csrc/cloud_intersect.hip).  Our rule, restated in
# tests/intersect_ref.py and equal to it exactly; parity with Open3D's is_self_intersecting is unpinned.
_ISECT_HDR = np.dtype([("status", "<i4"), ("R", "<i4"), ("entries", "<i8"), ("large", "<i8"), ("part", "<i8"), ("runs", "<i8"),
                       ("candidates", "<i8"), ("cursor", "<u8"), ("dims", "<i4", 3), ("pad", "<i4"), ("origin", "<f8", 3),
                       ("cell", "<f8"), ("unused", "<f8", 3), ("stats", "<i8", 8), ("ext", "<u8", 6), ("side_sum", "<i8")])
INTERSECTION_COUNTS = ("candidate_pairs", "adjacent_pairs", "tested_pairs", "intersecting_pairs", "uncertain_pairs",
                       "intersecting_triangles", "uncertain_triangles")
INTERSECTION_GRID = ("cells", "entries", "large_triangles")


def _isect_ws(stage: int, device, nv: int, nt: int, items: int = 0) -> torch.Tensor:
    need = int(N.lib().slg_isect_ws_bytes(stage, nv, nt, items))
    if need < 0:
        CL._raise(-need)
    return torch.empty(need, dtype=torch.uint8, device=device)


def _isect_header(ws, what: str):
    hdr = np.frombuffer(ws[:_ISECT_HDR.itemsize].cpu().numpy().tobytes(), dtype=_ISECT_HDR)[0]
    if int(hdr["status"]) & N.FILTER_BAD_INDEX:
        raise IndexError(f"{what}: a triangle index lies outside 0 .. V - 1")
    return hdr


def _isect_list(which, nt, nc, pws, count, max_pairs, dev, st):
    """The int32 ``[count, 2]`` list of the pairs with the verdict bit ``which``, or None above ``max_pairs``."""
    if count > max_pairs:
        return None
    out = torch.empty((count, 2), dtype=torch.int32, device=dev)
    if count:
        lws = _isect_ws(N.ISECT_WS_LIST, dev, 1, nt, count)
        CL._raise(N.lib().slg_isect_list(which, nt, nc, E._vp(pws), pws.numel(), count, E._vp(lws), lws.numel(), E._vp(out), st))
    return out


def self_intersections(mesh: TriangleMesh, return_pairs: bool = False, return_arrays: bool = False, max_pairs: int = 1 << 20,
                       max_candidates: int = 1 << 28, stream=None, timings=None, _cell: float = 0.0) -> dict:
    """Which pairs of triangles of ``mesh`` cross (the rule is ``tests/intersect_ref.py``).

    A triangle with two equal indices, or with a coordinate that is not finite, takes part in
    nothing.  A candidate is a pair ``s < t`` of the others whose closed boxes overlap.  Pairs that share
    two or three vertex *indices* are adjacent: counted, not tested.  With one shared index the two
    edges opposite it are tested against the other triangle, with none all six.  An edge pierces a
    triangle iff its ends lie strictly on opposite sides of the plane and it passes the three edges
    on one strict side; every sign is one fp64 determinant (Shewchuk's ``orient3dfast``), *certain* when
    it exceeds his stage-A bound.  A pair is intersecting iff an edge pierces, and uncertain iff no
    edge test is certainly piercing and one is neither certainly excluded nor certainly piercing.

    Integer counts: ``candidate_pairs``, ``adjacent_pairs``, ``tested_pairs``, ``intersecting_pairs``,
    ``uncertain_pairs``, ``intersecting_triangles``, ``uncertain_triangles``; the boolean
    ``intersection_free`` (no intersecting and no uncertain pair); and ``cells``, ``entries``,
    ``large_triangles``, which describe the uniform grid that found the candidates and are
    informational: nothing else depends on the grid.  ``return_arrays`` adds ``triangle_class`` uint8
    ``[T]`` on the device (1 intersecting, 2 uncertain).  ``return_pairs`` adds ``pairs`` and
    ``uncertain``, int32 ``[K, 2]`` on the device ascending by ``(s, t)``, and ``pairs_truncated``: a list
    longer than ``max_pairs`` is None.  More than ``max_candidates`` candidates are a ``ValueError`` that
    names the count, raised before they are stored.

    What the rule leaves out: coplanar overlaps and coincident but unwelded vertices give zeros and
    show up as uncertain, not as intersecting; a fold across a shared edge is an adjacent pair and is
    not tested; underflow is outside the bound.  Our rule, Open3D parity (``is_self_intersecting``)
    unpinned.  An empty mesh gives the empty answer without a launch; ``IndexError`` for a triangle
    index outside ``0 .. V - 1``.  ``timings``: a dict that gets the stages' times in ms by HIP events
    (``boxes``, ``entries`` with the sort, ``candidates`` with count, read-back and emit, ``test``, ``lists``)."""
    what = "self_intersections"
    vert, tris = _post_mesh(mesh, what)
    for name, value in (("max_pairs", max_pairs), ("max_candidates", max_candidates)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
            raise ValueError(f"{what}: {name} must be a whole number >= 0, not {value!r}")
    if isinstance(_cell, bool) or not isinstance(_cell, (int, float)) or not (np.isfinite(_cell) and _cell >= 0.0):
        raise ValueError(f"{what}: _cell must be a finite number >= 0, not {_cell!r}")
    nv, nt, dev = len(vert), len(tris), vert.device
    res = dict.fromkeys((*INTERSECTION_COUNTS, *INTERSECTION_GRID), 0)
    tclass, nc = None, 0
    pairs = {N.ISECT_INTERSECTING: None, N.ISECT_UNCERTAIN: None}
    if nv and nt:
        lib, st = N.lib(), E._stream(stream)
        with torch.cuda.device(dev):
            ws = _isect_ws(N.ISECT_WS_BOXES, dev, nv, nt)
            stages = _Stages(timings, stream)
            stages.mark("start")
            CL._raise(lib.slg_isect_boxes(E._vp(vert), nv, E._vp(tris), nt, float(_cell), E._vp(ws), ws.numel(), st))
            hdr = _isect_header(ws, what)             # the first read-back: the status, the entries, the large list
            ne, nl = int(hdr["entries"]), int(hdr["large"])
            res.update(cells=int(np.prod(hdr["dims"].astype(np.int64))), entries=ne, large_triangles=nl)
            stages.mark("boxes")
            ews = None
            if ne:
                ews = _isect_ws(N.ISECT_WS_ENTRIES, dev, nv, nt, ne)
                CL._raise(lib.slg_isect_entries(nt, nv, E._vp(ws), ws.numel(), ne, E._vp(ews), ews.numel(), st))
            stages.mark("entries")
            ewb = ews.numel() if ews is not None else 0
            CL._raise(lib.slg_isect_candidates_count(nt, nv, E._vp(ws), ws.numel(), ne, E._vp(ews), ewb, nl, st))
            nc = int(_isect_header(ws, what)["candidates"])       # the second: the candidates
            res["candidate_pairs"] = nc
            if nc > max_candidates:
                raise ValueError(f"{what}: {nc} candidate pairs, max_candidates is {max_candidates}")
            pws = None
            if nc:
                pws = _isect_ws(N.ISECT_WS_PAIRS, dev, nv, nt, nc)
                CL._raise(lib.slg_isect_candidates_emit(nt, nv, E._vp(ws), ws.numel(), ne, E._vp(ews), ewb, nl, nc, E._vp(pws),
                                                        pws.numel(), st))
            stages.mark("candidates")
            if nc:
                tclass = torch.empty(nt, dtype=torch.uint8, device=dev)
                CL._raise(lib.slg_isect_test(E._vp(vert), nv, E._vp(tris), nt, E._vp(ws), ws.numel(), nc, E._vp(pws), pws.numel(),
                                             E._vp(tclass), st))
                hdr = _isect_header(ws, what)         # the third: the counts
                res.update({name: int(hdr["stats"][i]) for i, name in enumerate(N.ISECT_STATS)})
            stages.mark("test")
            if return_pairs and nc:
                for which, key in ((N.ISECT_INTERSECTING, "intersecting_pairs"), (N.ISECT_UNCERTAIN, "uncertain_pairs")):
                    pairs[which] = _isect_list(which, nt, nc, pws, res[key], max_pairs, dev, st)
            stages.mark("lists")
            stages.close()
    res["intersection_free"] = intersection_verdict(res)
    if return_arrays:
        res["triangle_class"] = tclass if tclass is not None else torch.zeros(nt, dtype=torch.uint8, device=dev)
    if return_pairs:
        for which, name in ((N.ISECT_INTERSECTING, "pairs"), (N.ISECT_UNCERTAIN, "uncertain")):
            res[name] = pairs[which] if nc else torch.zeros((0, 2), dtype=torch.int32, device=dev)
        res["pairs_truncated"] = res["intersecting_pairs"] > max_pairs or res["uncertain_pairs"] > max_pairs
    return res


def intersection_verdict(counts: dict) -> bool:
    """``intersection_free`` of :func:`self_intersections`: no intersecting and no uncertain pair."""
    return counts["intersecting_pairs"] == 0 and counts["uncertain_pairs"] == 0


def format_intersections(r: dict) -> str:
    """One line of a :func:`self_intersections` record."""
    verdict = "intersection-free" if r["intersection_free"] else "not intersection-free"
    return (f"{r['candidate_pairs']} candidate pairs ({r['adjacent_pairs']} adjacent, {r['tested_pairs']} tested), "
            f"{r['intersecting_pairs']} intersecting and {r['uncertain_pairs']} uncertain pairs on {r['intersecting_triangles']} and "
            f"{r['uncertain_triangles']} triangles: {verdict}; coplanar overlaps and folds over a shared edge not tested")


_AUDIT_KEYS = ("keep_components", "min_component_faces", "clean", "audit", "self_intersections")


def _whole(value, least: int, what: str) -> int:
    try:
        whole = not isinstance(value, bool) and float(value) == int(value)
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or int(value) < least:
        raise ValueError(f"postprocess: {what} must be a whole number >= {least}, not {value!r}")
    return int(value)


def check_postprocess(params) -> None:
    """What :func:`postprocess` takes of the reference's ``meshlab_params``: raises before any launch."""
    if any(k in params for k in _AUDIT_KEYS):
        if params.get("backend", "device") != "device":
            raise ValueError(f"postprocess: {', '.join(k for k in _AUDIT_KEYS if k in params)} belong to \"backend\": \"device\", "
                             f"not {params.get('backend')!r}")
        if params.get("keep_components") is not None:
            _whole(params["keep_components"], 1, "keep_components")
        if params.get("min_component_faces") is not None:
            _whole(params["min_component_faces"], 0, "min_component_faces")
        for k in ("clean", "audit", "self_intersections"):
            if not isinstance(params.get(k, False), (bool, np.bool_)):
                raise ValueError(f"postprocess: {k} must be True or False, not {params[k]!r}")
    _check_iterations(params.get("smooth_iters", 10), "postprocess")
    if params.get("close_holes"):
        check_hole_size(params.get("close_max_size", 30))
    if params.get("simplify"):
        rule = params.get("simplify_rule")
        if rule is None:
            raise NotImplementedError("simplify (quadric edge-collapse decimation) is a global priority queue and stays in the "
                                      "reference (server/processing.py:778-781); \"simplify_rule\": \"rounds\" asks for the "
                                      "device's own rule instead (mesh.decimate_quadric)")
        if rule != "rounds":
            raise ValueError(f"postprocess: unknown simplify_rule {rule!r} (\"rounds\": mesh.decimate_quadric)")
        check_target_faces(params.get("target_faces", DEFAULT_TARGET_FACES), "postprocess")


def postprocess(mesh: TriangleMesh, meshlab_params: dict, stream=None, return_record: bool = False):
    """The reference's MeshLab step (``server/processing.py:742-787``) on the device, in its order and
    from its keys: ``smooth_type`` ("laplacian", anything else Taubin) with ``smooth_iters``
    (default 10), then ``close_holes`` with ``close_max_size`` (default 30), then ``simplify`` with
    ``"simplify_rule": "rounds"``: :func:`decimate_quadric` to ``target_faces`` (default 50,000).
    ``simplify`` alone names MeshLab's sequential queue, which is another rule, and raises
    ``NotImplementedError``; any other ``simplify_rule`` is a ``ValueError``.  Our rules on the
    float64 mesh in memory; MeshLab parity unpinned.

    Keys of the device's own (with a ``"backend"`` other than ``"device"`` they are a
    ``ValueError``): ``"keep_components": k`` (:func:`keep_largest_components`) and / or
    ``"min_component_faces": n`` (:func:`remove_small_components`, after it) before the smoothing;
    ``"clean": True`` (:func:`clean`) after the hole closing, whose fill is what can double a face, and
    before ``simplify``; ``"audit": True`` audits the final mesh (:func:`audit`);
    ``"self_intersections": True`` tests it for crossing triangles (:func:`self_intersections`,
    DESIGN.md §23).  With ``return_record`` the result is ``(mesh, audit dict or None)``; the
    intersection record is the dict's ``"self_intersections"`` (a dict with that key alone without
    ``"audit"``).  Without these keys nothing changes."""
    params = dict(meshlab_params or {})
    check_postprocess(params)
    if params.get("keep_components") is not None:
        mesh = keep_largest_components(mesh, int(params["keep_components"]), stream=stream)
    if params.get("min_component_faces") is not None:
        mesh = remove_small_components(mesh, int(params["min_component_faces"]), stream=stream)
    iters = int(params.get("smooth_iters", 10))
    if str(params.get("smooth_type", "taubin")) == "laplacian":
        mesh = smooth_laplacian(mesh, iters, stream=stream)
    else:
        mesh = smooth_taubin(mesh, iters, stream=stream)
    if params.get("close_holes"):
        mesh = close_holes(mesh, int(params.get("close_max_size", 30)), stream=stream)
    if params.get("clean"):
        mesh = clean(mesh, stream=stream)
    if params.get("simplify"):
        mesh = decimate_quadric(mesh, int(params.get("target_faces", DEFAULT_TARGET_FACES)), stream=stream)
    record = audit(mesh, stream=stream) if params.get("audit") else None
    if params.get("self_intersections"):
        record = {**(record or {}), "self_intersections": self_intersections(mesh, stream=stream)}
    return (mesh, record) if return_record else mesh
