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
