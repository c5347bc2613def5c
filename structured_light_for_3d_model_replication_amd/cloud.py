"""Point clouds on the device and their cleanup filters (``csrc/cloud_*.hip``).

``PointCloud`` is a packed float64 ``xyz`` + uint8 BGR ``bgr`` pair in HBM; :func:`radius_outlier`,
:func:`statistical_outlier` and :func:`largest_cluster` are the three deterministic neighbour
steps of the reference's cleanup tab (``ProcessingLogic.remove_radius_outlier``,
``server/processing.py:430-448``, ``ProcessingLogic.remove_outliers``, ``:367-388``, and
``ProcessingLogic.keep_largest_cluster``, ``:391-427``), run on that cloud without the PLY round
trip through the host.  Semantics: ``include/slgpu.h`` and DESIGN.md §9 (Open3D's published rules
restated; parity with an installed Open3D is unpinned).

The same grid carries the Open3D steps of the merge tail and of the front of both meshing methods
(``server/processing.py:605-628``, ``:653-670``, ``:804-837``): :func:`voxel_down_sample`,
:func:`uniform_down_sample`, :func:`estimate_normals`, :func:`orient_normals_towards` and
:func:`centroid`.

The loop body of ``merge_pro_360`` (``:549-603``) has its deterministic part here as well:
:func:`registration_icp` (point to plane), :func:`evaluate_registration`, :func:`transform` and
:func:`concat`.  The initial pose the reference finds per pair is here too:
:func:`compute_fpfh_feature`, :func:`correspondences_from_features` and the seeded
:func:`registration_ransac_based_on_feature_matching` (``server/processing.py:451-486``;
DESIGN.md §13).

The cleanup tab's first step, ``ProcessingLogic.remove_background`` (``:337-364``), is here as the
seeded :func:`segment_plane` and :func:`remove_plane`.

The PLY reader takes exactly the file ``ProcessingLogic._save_ply`` writes (``ply.header``): ASCII,
``x y z red green blue``, or the same with ``nx ny nz`` after ``z`` (a cloud with normals).
Anything else raises ``ValueError`` saying what differs.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading

import numpy as np
import torch

from . import _native as N
from . import engine as E
from . import ply as PLY

MAX_NEIGHBORS = 64          # kMaxK of csrc/cloud_grid.h
RANSAC_BATCH = 4096         # trials per slg_ransac_batch: one read-back of the evaluated trials' records each
RANSAC_MAX_EVAL = 64        # evaluations per batch: where more trials pass, the batch ends early (K shrinks fast there)

_HEADER_TAIL = PLY.header(0).decode().split("\n")[3:-1]      # the property lines + end_header


_NORMAL_LINES = ["property float nx", "property float ny", "property float nz"]
_HEADER_TAIL_NORMALS = _HEADER_TAIL[:3] + _NORMAL_LINES + _HEADER_TAIL[3:]


def read_ply(path, normals: bool = False):
    """``(P float64 [n, 3], C uint8 [n, 3] BGR)`` of an ASCII PLY in ``_save_ply``'s layout, or in
    the layout with normals (``x y z nx ny nz red green blue``).  With ``normals=True`` the
    result is ``(P, C, normals float64 [n, 3] or None)``."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n"):
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic line)")
    if end < 0:
        raise ValueError(f"{path}: PLY header has no end_header line")
    lines = data[:end + len(b"end_header")].decode("ascii", errors="replace").split("\n")
    if len(lines) < 3 or lines[1] != "format ascii 1.0":
        raise ValueError(f"{path}: only 'format ascii 1.0' PLY files are read, this one says "
                         f"{lines[1] if len(lines) > 1 else ''!r}")
    parts = lines[2].split()
    if len(parts) != 3 or parts[:2] != ["element", "vertex"] or not parts[2].isdigit():
        raise ValueError(f"{path}: expected 'element vertex <n>' as the third header line, got {lines[2]!r}")
    n = int(parts[2])
    if lines[3:] == _HEADER_TAIL:
        width = 6
    elif lines[3:] == _HEADER_TAIL_NORMALS:
        width = 9
    else:
        raise ValueError(f"{path}: the vertex layout must be exactly {_HEADER_TAIL[:-1]} "
                         f"(what _save_ply writes) or {_HEADER_TAIL_NORMALS[:-1]} (with normals), "
                         f"got {lines[3:-1]}")
    body = data[end + len(b"end_header\n"):]
    try:
        vals = np.array(body.split(), dtype=np.float64)
    except ValueError as e:
        raise ValueError(f"{path}: a vertex line holds something that is not a number ({e})") from None
    if vals.size != width * n:
        raise ValueError(f"{path}: header promises {n} vertices of {width} values, body holds {vals.size} values")
    vals = vals.reshape(n, width)
    rgb = vals[:, width - 3:]
    if n and not (np.all(rgb == np.floor(rgb)) and rgb.min() >= 0 and rgb.max() <= 255):
        raise ValueError(f"{path}: colours must be integers 0..255")
    P, C = np.ascontiguousarray(vals[:, :3]), np.ascontiguousarray(rgb[:, ::-1].astype(np.uint8))
    if not normals:
        return P, C
    return P, C, (np.ascontiguousarray(vals[:, 3:6]) if width == 9 else None)


def write_ply_normals(path, points, colors, normals) -> None:
    """The layout with normals on the host: ``_save_ply``'s header with the three normal
    properties after ``z``, positions as ``%.4f``, normals as ``%.6f``, BGR swapped to RGB."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    Nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    C = np.asarray(colors, np.uint8).reshape(-1, 3)
    if not len(P) == len(Nrm) == len(C):
        raise ValueError("points, normals and colors differ in length")
    head = PLY.header(len(P)).decode().split("\n")
    head = head[:6] + _NORMAL_LINES + head[6:]
    with open(path, "wb") as f:
        f.write("\n".join(head).encode())
        np.savetxt(f, np.hstack([P, Nrm, C[:, ::-1].astype(np.float64)]),
                   fmt="%.4f %.4f %.4f %.6f %.6f %.6f %d %d %d")


class PointCloud:
    """A cloud in HBM: ``xyz`` float64 ``[n, 3]``, ``bgr`` uint8 ``[n, 3]`` and ``normals``
    float64 ``[n, 3]`` or ``None`` (an empty cloud holds empty host tensors and needs no device).

    Build it from ``(P, C)`` arrays or tensors, from an ``engine.Cloud`` (:meth:`from_cloud`, the
    points stay on the device) or from a PLY written by ``_save_ply`` (:meth:`from_file`)."""

    def __init__(self, points, colors=None, device=None, normals=None):
        def as_tensor(a, dt, np_dt):
            if isinstance(a, torch.Tensor):
                return a.reshape(-1, 3).to(dt)
            a = np.ascontiguousarray(np.asarray(a, dtype=np_dt).reshape(-1, 3))
            return torch.from_numpy(a if a.flags.writeable else a.copy())

        xyz = as_tensor(points, torch.float64, np.float64)
        if colors is None:
            colors = np.zeros((len(xyz), 3), np.uint8)
        bgr = as_tensor(colors, torch.uint8, np.uint8)
        if len(xyz) != len(bgr):
            raise ValueError("points and colors differ in length")
        if len(xyz):
            dev = device or (xyz.device if xyz.is_cuda else E.default_device())
            xyz, bgr = xyz.to(dev).contiguous(), bgr.to(dev).contiguous()
        self.xyz, self.bgr = xyz, bgr
        self.normals = None
        if normals is not None:
            nrm = as_tensor(normals, torch.float64, np.float64)
            if len(nrm) != len(xyz):
                raise ValueError("points and normals differ in length")
            self.normals = nrm.to(xyz.device).contiguous()

    @classmethod
    def from_cloud(cls, cloud: "E.Cloud") -> "PointCloud":
        """From a reconstructed view (``Reconstructor.reconstruct(..., xyz_f64=True)``): reads the
        point count, copies no point."""
        if not cloud.xyz_f64:
            raise ValueError("PointCloud needs a float64 cloud (reconstruct with xyz_f64=True)")
        P, C = cloud.result()
        return cls(P, C)

    @classmethod
    def from_file(cls, path) -> "PointCloud":
        P, C, nrm = read_ply(path, normals=True)
        return cls(P, C, normals=nrm)

    def has_points(self) -> bool:
        return len(self) > 0

    def has_normals(self) -> bool:
        return self.normals is not None and len(self) > 0

    def __len__(self) -> int:
        return int(self.xyz.shape[0])

    def numpy(self):
        """Host ``(P float64 [n, 3], C uint8 [n, 3] BGR)``."""
        return self.xyz.cpu().numpy(), self.bgr.cpu().numpy()

    def save(self, path) -> None:
        """ASCII PLY as ``_save_ply`` writes it; a cloud with normals is written by the host
        writer in the layout with normals (:func:`write_ply_normals`)."""
        if self.normals is None:
            PLY.write_ascii(path, *self.numpy())
        else:
            write_ply_normals(path, *self.numpy(), self.normals.cpu().numpy())


def as_point_cloud(obj) -> PointCloud:
    if isinstance(obj, PointCloud):
        return obj
    if isinstance(obj, E.Cloud):
        return PointCloud.from_cloud(obj)
    if isinstance(obj, (str, os.PathLike)):
        return PointCloud.from_file(obj)
    if isinstance(obj, (tuple, list)) and len(obj) == 2:
        return PointCloud(*obj)
    raise TypeError(f"cannot make a PointCloud from {type(obj).__name__}")


def _nonempty(pc) -> PointCloud:
    pc = as_point_cloud(pc)
    if not pc.has_points():
        raise ValueError("Point cloud is empty.")
    return pc


# ----------------------------------------------------------------------------- filters
_WS = threading.local()     # .by_device: the calling thread's workspace per device


def _workspaces() -> dict:
    """``{device: workspace}`` of the calling thread.  A step's kernels keep the grid, the status
    word and, between the calls of a multi-call step, its state in the workspace, and the wrappers
    run with the GIL released: a workspace is never shared between threads, and ends with its
    thread."""
    by_device = getattr(_WS, "by_device", None)
    if by_device is None:
        by_device = _WS.by_device = {}
    return by_device


def _workspace(device, need) -> torch.Tensor:
    """The calling thread's workspace on the device, grown to ``need`` bytes (what the step's
    ``slg_*_ws_bytes`` returned; a negative size is that call's error code)."""
    need = int(need)
    if need < 0:
        N.check(-need)
    by_device = _workspaces()
    ws = by_device.get(device)
    if ws is None or ws.numel() < need:
        ws = by_device[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _check_xyz(xyz: torch.Tensor) -> torch.Tensor:
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda and xyz.dtype == torch.float64
            and xyz.ndim == 2 and xyz.shape[1] == 3):
        raise ValueError("the cloud filters take a device float64 [n, 3] tensor")
    if xyz.shape[0] == 0:
        raise ValueError("Point cloud is empty.")
    return xyz.contiguous()


def _check_status(ws: torch.Tensor, what: str) -> None:
    """Reads the status word at the front of the workspace (synchronises the stream)."""
    status = int(ws[:4].view(torch.int32).item())
    if status & N.FILTER_BAD_NONFINITE:
        raise ValueError(f"{what}: the cloud holds a NaN or infinite coordinate")
    if status & N.FILTER_BAD_EXTENT:
        raise ValueError(f"{what}: the cloud spans 2^21 or more cells of the radius or voxel size on an axis")
    if status & N.FILTER_BAD_INDEX:
        raise ValueError(f"{what}: a correspondence names a point outside its cloud")


def far_count(device) -> int:
    """Points the calling thread's last :func:`statistical_mask` or :func:`normal_covariances` on
    ``device`` sent to the whole-cloud kernel (the ring walk reached its cap): the int32 at byte 8
    of that thread's workspace.  After :func:`registration_icp` or :func:`evaluate_registration`:
    the source points sent to the whole-target kernel, summed over the evaluations.  A test hook."""
    return int(_workspaces()[device][8:12].view(torch.int32).item())


def _filter_ws(xyz: torch.Tensor, k: int):
    """The sizing call of the steps whose workspace is the grid's alone (for :func:`_call`)."""
    return lambda: N.lib().slg_filter_ws_bytes(xyz.shape[0], k)


def _call(fn, device, need, head, outs, stream, what=None, *, sized=True) -> torch.Tensor:
    """What every wrapper of a workspace call shares: the device guard, the workspace of ``need()``
    bytes (the step's own sizing call, made under the guard: rocPRIM's size query runs on the
    cloud's device), ``fn(*head, ws, ws_bytes, *outs, stream)`` (``ws`` alone with ``sized=False``:
    ``slg_cloud_select`` takes no size), the error, and (with ``what``) the status word.  Tensors and ``None`` in
    ``head`` and ``outs`` go as pointers, everything else as it is.  Returns the workspace: a
    caller whose own read-back comes before the status word passes no ``what`` and checks after."""
    def arg(a):
        return E._vp(a) if a is None or isinstance(a, torch.Tensor) else a
    with torch.cuda.device(device):
        ws = _workspace(device, need())
        size = (ws.numel(),) if sized else ()
        _raise(fn(*map(arg, head), E._vp(ws), *size, *map(arg, outs), E._stream(stream)))
        if what:
            _check_status(ws, what)
    return ws


def radius_mask(xyz: torch.Tensor, nb_points: int, radius: float, stream=None):
    """``(keep uint8 [n], counts int32 [n])`` on the device: ``counts[i]`` = points with
    ``d2 < radius**2`` (``i`` included), ``keep = counts > nb_points``."""
    xyz = _check_xyz(xyz)
    n = xyz.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    counts = torch.empty(n, dtype=torch.int32, device=xyz.device)
    _call(N.lib().slg_radius_outlier, xyz.device, _filter_ws(xyz, 0), (xyz, n, float(radius), int(nb_points)),
          (keep, counts), stream, "radius_outlier")
    return keep, counts


def statistical_mask(xyz: torch.Tensor, nb_neighbors: int, std_ratio: float, stream=None):
    """``(keep uint8 [n], avg float64 [n], stats float64 [3] = mean, std, thr)`` on the device."""
    xyz = _check_xyz(xyz)
    n = xyz.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    avg = torch.empty(n, dtype=torch.float64, device=xyz.device)
    stats = torch.empty(3, dtype=torch.float64, device=xyz.device)
    _call(N.lib().slg_statistical_outlier, xyz.device, _filter_ws(xyz, min(int(nb_neighbors), MAX_NEIGHBORS)),
          (xyz, n, int(nb_neighbors), float(std_ratio)), (keep, avg, stats), stream, "statistical_outlier")
    return keep, avg, stats


def dbscan_labels(xyz: torch.Tensor, eps: float, min_points: int, stream=None):
    """``(labels int32 [n], keep uint8 [n], info int32 [4])`` on the device: Open3D's
    ``cluster_dbscan`` labels in closed form (``-1`` noise, else ``0..n_clusters-1`` in ascending
    order of each cluster's smallest core index), ``keep = labels == largest label``, and
    ``info = (n_clusters, largest_label, largest_count, n_noise)``."""
    xyz = _check_xyz(xyz)
    n = xyz.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=xyz.device)
    keep = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    info = torch.empty(4, dtype=torch.int32, device=xyz.device)
    _call(N.lib().slg_dbscan, xyz.device, _filter_ws(xyz, 0), (xyz, n, float(eps), int(min_points)),
          (labels, keep, info), stream, "dbscan")
    return labels, keep, info


def _raise(rc: int) -> None:
    if rc == N.SLG_ERR_INVALID:
        raise ValueError(N.lib().slg_last_error().decode(errors="replace"))
    N.check(rc)


def select(pc: PointCloud, keep: torch.Tensor, stream=None):
    """``(PointCloud of the points with keep != 0 in input order, their indices int64)``.  The
    result has no normals."""
    n = len(pc)
    dev = pc.xyz.device
    out = E.Cloud(n, 0, True, dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    o = out.struct()
    _call(N.lib().slg_cloud_select, dev, _filter_ws(pc.xyz, 0),
          (pc.xyz, pc.bgr, n, keep.contiguous(), ctypes.byref(o), index), (), stream, sized=False)
    P, C = out._launched_on(stream).result()
    return PointCloud(P, C), index[:len(P)]


def radius_outlier(pc, nb_points: int, radius: float, return_index: bool = False):
    """Open3D ``remove_radius_outlier`` + ``select_by_index`` on the device: a new ``PointCloud``
    of the points with more than ``nb_points`` points (itself included) closer than ``radius``.
    Normals are not carried over: the result has none."""
    pc = _nonempty(pc)
    keep, _ = radius_mask(pc.xyz, nb_points, radius)
    out, idx = select(pc, keep)
    return (out, idx) if return_index else out


def statistical_outlier(pc, nb_neighbors: int, std_ratio: float, return_index: bool = False):
    """Open3D ``remove_statistical_outlier`` + ``select_by_index`` on the device
    (``nb_neighbors`` <= 64).  Normals are not carried over: the result has none."""
    pc = _nonempty(pc)
    keep, _, _ = statistical_mask(pc.xyz, nb_neighbors, std_ratio)
    out, idx = select(pc, keep)
    return (out, idx) if return_index else out


def largest_cluster(pc, eps: float, min_points: int, return_index: bool = False):
    """Open3D ``cluster_dbscan`` + the largest-label pick of ``keep_largest_cluster`` +
    ``select_by_index`` on the device: a new ``PointCloud`` of the largest cluster's points in
    input order (the lowest label among equally large ones).  When every point is noise the input
    cloud itself comes back, with indices ``arange(n)``.  Normals are not carried over: a
    selected result has none."""
    pc = _nonempty(pc)
    _, keep, info = dbscan_labels(pc.xyz, eps, min_points)
    if int(info[0].item()) == 0:
        return (pc, torch.arange(len(pc), dtype=torch.int64, device=pc.xyz.device)) if return_index else pc
    out, idx = select(pc, keep)
    return (out, idx) if return_index else out


# ----------------------------------------------------------------------------- merge / mesh tail
def voxel_down_sample(pc, voxel_size: float, return_index: bool = False, stream=None):
    """Open3D ``voxel_down_sample`` on the device: one point per occupied voxel of
    ``floor((p - (min_bound - voxel_size / 2)) / voxel_size)``, the mean of its members summed left
    to right in ascending index; colours the exact mean rounded half up; voxels in ascending order
    of their smallest member index.  The result has no normals.  With ``return_index``:
    ``(cloud, first_index int64 [m], count int32 [m])``."""
    pc = _nonempty(pc)
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    oxyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    obgr = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    first = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    m = torch.empty(1, dtype=torch.int64, device=dev)           # written by the call (as every output here)
    _call(N.lib().slg_voxel_downsample, dev, _filter_ws(xyz, 0), (xyz, pc.bgr, n, float(voxel_size)),
          (oxyz, obgr, first, count, m), stream, "voxel_down_sample")
    m = int(m.item())
    out = PointCloud(oxyz[:m], obgr[:m])
    return (out, first[:m], count[:m]) if return_index else out


def uniform_down_sample(pc, every_k: int):
    """Open3D ``uniform_down_sample``: the points ``0, k, 2k, ...`` (normals too, when present)."""
    pc = as_point_cloud(pc)
    every_k = int(every_k)
    if every_k < 1:
        raise ValueError("every_k must be >= 1")
    return PointCloud(pc.xyz[::every_k].contiguous(), pc.bgr[::every_k].contiguous(),
                      normals=None if pc.normals is None else pc.normals[::every_k].contiguous())


def normal_covariances(xyz: torch.Tensor, radius: float, max_nn: int, stream=None):
    """``(cov float64 [n, 6] = xx, xy, xz, yy, yz, zz, m int32 [n], normals float64 [n, 3])`` on
    the device: the hybrid search's neighbour count, their covariance and the normal."""
    xyz = _check_xyz(xyz)
    n, dev = xyz.shape[0], xyz.device
    nrm = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cov = torch.empty((n, 6), dtype=torch.float64, device=dev)
    m = torch.empty(n, dtype=torch.int32, device=dev)
    _call(N.lib().slg_estimate_normals, dev, _filter_ws(xyz, 0), (xyz, n, float(radius), int(max_nn)),
          (nrm, cov, m), stream, "estimate_normals")
    return cov, m, nrm


def estimate_normals(pc, radius: float, max_nn: int = 30):
    """Open3D ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`` on the device
    (``3 <= max_nn <= 64``): a ``PointCloud`` sharing ``xyz`` / ``bgr`` with ``normals`` set."""
    pc = _nonempty(pc)
    _, _, nrm = normal_covariances(pc.xyz, radius, max_nn)
    return PointCloud(pc.xyz, pc.bgr, normals=nrm)


def centroid(pc, stream=None) -> torch.Tensor:
    """Per-axis mean of the points, float64 ``[3]`` on the device (``get_center()``)."""
    pc = _nonempty(pc)
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    out = torch.empty(3, dtype=torch.float64, device=dev)
    _call(N.lib().slg_cloud_centroid, dev, _filter_ws(xyz, 0), (xyz, n), (out,), stream)
    return out


def orient_normals_towards(pc, location, outward: bool = False, stream=None):
    """Open3D ``orient_normals_towards_camera_location(location)``: a normal with
    ``normal . (location - p) < 0`` is negated; ``outward`` then negates every normal (the
    reference's ``* -1.0``).  ``location``: three numbers or a device tensor.  A new ``PointCloud``
    sharing ``xyz`` / ``bgr``."""
    pc = as_point_cloud(pc)
    if not pc.has_normals():
        raise ValueError("the cloud has no normals")
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    if isinstance(location, torch.Tensor):
        loc = location.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    else:
        loc = torch.tensor([float(v) for v in np.asarray(location, np.float64).reshape(-1)], dtype=torch.float64,
                           device=dev)
    if loc.numel() != 3:
        raise ValueError("location must hold three numbers")
    with torch.cuda.device(dev):
        nrm = pc.normals.clone()
        _raise(N.lib().slg_orient_normals(E._vp(xyz), E._vp(nrm), n, E._vp(loc), int(bool(outward)),
                                          E._stream(stream)))
    return PointCloud(pc.xyz, pc.bgr, normals=nrm)


# ----------------------------------------------------------------------------- registration / merge loop
class RegistrationResult:
    """What :func:`registration_icp` and :func:`evaluate_registration` return: ``transformation``
    (4x4 NumPy array), ``fitness``, ``inlier_rmse``, ``iterations`` (updates made), ``converged``
    (the stop test ended the loop), ``correspondence_set`` (device int64 ``[m, 2]``: source index,
    target index, in source order) and ``log`` (NumPy ``[iterations + 1, ICP_LOG_STRIDE]``, one
    record per evaluation as ``include/slgpu.h`` lays it out, or ``None``).

    From :func:`registration_ransac_based_on_feature_matching`: ``iterations`` is the final ``K``
    (the trials the choice ran over), ``converged`` says whether ``K`` ended below
    ``max_iteration``, ``log`` holds one record per evaluated trial below ``K``
    (``[*, RANSAC_RECORD_STRIDE]``: trial, the three draws, T, n_corr, err2, fitness, rmse,
    inliers), and ``trial`` is the winner's trial number (-1: none passed)."""

    trial = None

    def __init__(self, transformation, fitness, inlier_rmse, iterations, converged, correspondence_set, log):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.iterations = iterations
        self.converged = converged
        self.correspondence_set = correspondence_set
        self.log = log

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.6f}, inlier_rmse={self.inlier_rmse:.6g}, "
                f"correspondences={len(self.correspondence_set)}, iterations={self.iterations}, "
                f"converged={self.converged})")


def _matrix4(T, what: str) -> np.ndarray:
    """A copy of ``T`` as a C-ordered float64 4x4 whose last row is exactly ``0 0 0 1``
    (``None``: the identity)."""
    if T is None:
        return np.eye(4)
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    T = np.array(T, dtype=np.float64, order="C")
    if T.shape != (4, 4):
        raise ValueError(f"{what}: the transformation must be a 4x4 matrix, got shape {T.shape}")
    if not np.isfinite(T).all() or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{what}: the transformation needs finite entries and a last row of 0 0 0 1")
    return T


def _dbl16(T: np.ndarray):
    return T.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _register(what, source, target, max_correspondence_distance, init, relative_fitness, relative_rmse,
              max_iteration, return_log, need_normals, stream) -> RegistrationResult:
    source, target = _nonempty(source), _nonempty(target)
    if need_normals and not target.has_normals():
        raise ValueError(f"{what}: point-to-plane ICP needs target normals (estimate_normals)")
    d, rf, rr, it = float(max_correspondence_distance), float(relative_fitness), float(relative_rmse), int(max_iteration)
    if not d > 0.0:
        raise ValueError(f"{what}: max_correspondence_distance must be > 0")
    if not (rf >= 0.0 and rr >= 0.0):
        raise ValueError(f"{what}: relative_fitness and relative_rmse must be >= 0")
    if it < 0:
        raise ValueError(f"{what}: max_iteration must be >= 0")
    T0 = _matrix4(init, what)
    src, tgt = _check_xyz(source.xyz), _check_xyz(target.xyz)
    dev = src.device
    if tgt.device != dev:
        raise ValueError(f"{what}: source and target live on different devices")
    nrm = target.normals.contiguous() if target.has_normals() else None
    ns, nt = src.shape[0], tgt.shape[0]
    L = N.lib()
    out = torch.empty(N.ICP_RESULT_LEN + (it + 1) * N.ICP_LOG_STRIDE, dtype=torch.float64, device=dev)
    corr = torch.empty(ns, dtype=torch.int32, device=dev)
    _call(L.slg_icp_point_to_plane, dev, lambda: L.slg_icp_ws_bytes(ns, nt, it),
          (src, ns, tgt, nrm, nt, d, _dbl16(T0), rf, rr, it), (out, corr, out[N.ICP_RESULT_LEN:]), stream, what)
    host = out.cpu().numpy()                                 # the one read-back: result and log
    res = host[:N.ICP_RESULT_LEN]
    iterations = int(res[19])
    log = host[N.ICP_RESULT_LEN:].reshape(it + 1, N.ICP_LOG_STRIDE)[:iterations + 1].copy() if return_log else None
    si = torch.nonzero(corr >= 0).reshape(-1)
    pairs = torch.stack([si, corr[si].to(torch.int64)], 1)
    return RegistrationResult(res[:16].reshape(4, 4).copy(), float(res[16]), float(res[17]), iterations,
                              bool(res[20]), pairs, log)


def registration_icp(source, target, max_correspondence_distance, init=None, relative_fitness=1e-6,
                     relative_rmse=1e-6, max_iteration=30, return_log=False, stream=None) -> RegistrationResult:
    """Open3D ``registration_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationPointToPlane(), ICPConvergenceCriteria(relative_fitness, relative_rmse,
    max_iteration))`` on the device (``csrc/cloud_icp.hip``; rules: DESIGN.md §12).  Every
    iteration is enqueued at once and the result is read back once.  ``target`` needs normals
    (``ValueError`` otherwise); ``init``: a 4x4 with a last row of ``0 0 0 1`` (default: the
    identity)."""
    return _register("registration_icp", source, target, max_correspondence_distance, init, relative_fitness,
                     relative_rmse, max_iteration, return_log, True, stream)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None,
                          stream=None) -> RegistrationResult:
    """Open3D ``evaluate_registration``: fitness, inlier rmse and correspondences at
    ``transformation``, with no update (``registration_icp`` with ``max_iteration=0``; the target
    needs no normals)."""
    return _register("evaluate_registration", source, target, max_correspondence_distance, transformation, 0.0, 0.0,
                     0, False, False, stream)


def transform(pc, T, stream=None) -> PointCloud:
    """Open3D ``PointCloud.transform`` into a new cloud: ``p' = ((T[a][0] x + T[a][1] y) + T[a][2] z)
    + T[a][3]``; normals, when present, by the 3x3 block; colours are kept (shared)."""
    pc = as_point_cloud(pc)
    M = _matrix4(T, "transform")
    if not pc.has_points():
        return pc
    xyz = _check_xyz(pc.xyz)
    n = xyz.shape[0]
    oxyz = torch.empty_like(xyz)
    nrm = pc.normals.contiguous() if pc.has_normals() else None
    onrm = torch.empty_like(nrm) if nrm is not None else None
    with torch.cuda.device(xyz.device):
        _raise(N.lib().slg_cloud_transform(E._vp(xyz), E._vp(nrm), n, _dbl16(M), E._vp(oxyz), E._vp(onrm),
                                           E._stream(stream)))
    return PointCloud(oxyz, pc.bgr, normals=onrm)


def concat(a, b) -> PointCloud:
    """Open3D ``a += b`` into a new cloud: ``a``'s points, then ``b``'s (two device copies per
    array); normals are kept only when both clouds have them."""
    a, b = as_point_cloud(a), as_point_cloud(b)
    if not b.has_points():
        return a
    if not a.has_points():
        return b
    if a.xyz.device != b.xyz.device:
        raise ValueError("concat: the clouds live on different devices")
    both = a.has_normals() and b.has_normals()
    return PointCloud(torch.cat([a.xyz, b.xyz]), torch.cat([a.bgr, b.bgr]),
                      normals=torch.cat([a.normals, b.normals]) if both else None)


# ----------------------------------------------------------------------------- global registration
def _check_features(f, what: str) -> torch.Tensor:
    if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.float64 and f.ndim == 2
            and f.shape[1] == N.FPFH_DIM):
        raise ValueError(f"{what}: features are device float64 [n, {N.FPFH_DIM}] tensors")
    if f.shape[0] == 0:
        raise ValueError(f"{what}: a feature tensor is empty")
    return f.contiguous()


def fpfh_features(pc, radius: float, max_nn: int = 100, stream=None):
    """``(fpfh float64 [n, 33], spfh float64 [n, 33], m int32 [n])`` on the device: the feature,
    the simplified histogram it is built from, and the hybrid search's neighbour count (the point
    included)."""
    pc = _nonempty(pc)
    if not pc.has_normals():
        raise ValueError("compute_fpfh_feature: the cloud has no normals (estimate_normals)")
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    fpfh = torch.empty((n, N.FPFH_DIM), dtype=torch.float64, device=dev)
    spfh = torch.empty((n, N.FPFH_DIM), dtype=torch.float64, device=dev)
    m = torch.empty(n, dtype=torch.int32, device=dev)
    L = N.lib()
    _call(L.slg_fpfh, dev, lambda: L.slg_fpfh_ws_bytes(n, int(max_nn)),
          (xyz, pc.normals.contiguous(), n, float(radius), int(max_nn)), (fpfh, spfh, m), stream,
          "compute_fpfh_feature")
    return fpfh, spfh, m


def compute_fpfh_feature(pc, radius: float, max_nn: int = 100, stream=None) -> torch.Tensor:
    """Open3D ``compute_fpfh_feature(pc, KDTreeSearchParamHybrid(radius, max_nn))`` on the device
    (``csrc/cloud_feature.hip``; rules: DESIGN.md §13): float64 ``[n, 33]``, one row per point
    (Open3D's ``Feature.data`` is the transpose).  ``2 <= max_nn <= 128``; the cloud needs normals
    (``ValueError`` otherwise)."""
    return fpfh_features(pc, radius, max_nn, stream)[0]


def feature_nearest(source_feature: torch.Tensor, target_feature: torch.Tensor, mutual_filter: bool = False, stream=None):
    """``(pairs int64 [m, 2], nn_source int32 [n_source], nn_target int32 [n_target] or None)`` on
    the device: per source row the target row with the smallest (d2, index), the reverse search
    (with ``mutual_filter`` only) and the kept pairs in source order."""
    a = _check_features(source_feature, "correspondences_from_features")
    b = _check_features(target_feature, "correspondences_from_features")
    dev = a.device
    if b.device != dev:
        raise ValueError("correspondences_from_features: the features live on different devices")
    ns, nt = a.shape[0], b.shape[0]
    pairs = torch.empty((ns, 2), dtype=torch.int64, device=dev)
    nn_s = torch.empty(ns, dtype=torch.int32, device=dev)
    nn_t = torch.empty(nt, dtype=torch.int32, device=dev) if mutual_filter else None
    m = torch.empty(1, dtype=torch.int64, device=dev)
    L = N.lib()
    _call(L.slg_feature_match, dev, lambda: L.slg_feature_match_ws_bytes(ns, nt),
          (a, ns, b, nt, int(bool(mutual_filter))), (nn_s, nn_t, pairs, m), stream)
    return pairs[:int(m.item())], nn_s, nn_t


def correspondences_from_features(source_feature, target_feature, mutual_filter: bool = False, stream=None) -> torch.Tensor:
    """Open3D ``CorrespondencesFromFeatures``: device int64 ``[m, 2]`` (source row, target row) in
    source order.  Per source row the target row with the smallest ``(d2, index)``,
    ``d2 = sum_j (a_j - b_j)^2`` summed left to right, by exact brute force; with ``mutual_filter``
    only the pairs the reverse search confirms."""
    return feature_nearest(source_feature, target_feature, mutual_filter, stream)[0]


def ransac_max_trials(confidence: float, ratio: float):
    """``ceil(log(1 - confidence) / log(1 - ratio^3))``; ``0`` for ``ratio >= 1``; ``None`` where
    the expression bounds nothing (``confidence`` 1, or a ratio whose cube vanishes beside 1)."""
    if ratio >= 1.0:
        return 0
    den = math.log(1.0 - (ratio * ratio) * ratio)
    if not den < 0.0 or confidence >= 1.0:
        return None
    return int(math.ceil(math.log(1.0 - confidence) / den))


class RansacChoice:
    """The sequential choice of the RANSAC, fed with the evaluated trials' records
    in ascending trial order: a record replaces the best when its fitness is larger, or equal with
    a smaller rmse (ties keep the earlier trial); on a replacement with
    ``r = inliers / n_pairs > 0``, ``K = min(K, max(t + 1, ransac_max_trials(confidence, r)))``.
    Records at or past ``K`` are ignored."""

    def __init__(self, n_pairs: int, max_iteration: int, confidence: float):
        self.n_pairs, self.confidence, self.K = int(n_pairs), float(confidence), int(max_iteration)
        self.best = None            # the winner's record

    def offer(self, rec) -> bool:
        """False once the record lies at or past ``K`` (so do all later ones)."""
        t = int(rec[0])
        if t >= self.K:
            return False
        fitness, rmse = float(rec[22]), float(rec[23])
        if self.best is None or fitness > self.best[22] or (fitness == self.best[22] and rmse < self.best[23]):
            self.best = rec
            r = float(rec[24]) / self.n_pairs
            if r > 0.0:
                k = ransac_max_trials(self.confidence, r)
                if k is not None:
                    self.K = min(self.K, max(t + 1, k))
        return True


def ransac_batch(source, target, pairs: torch.Tensor, max_correspondence_distance, first_trial: int, count: int,
                 edge_length=0.9, confidence=0.999, seed=0, ransac_n=3, prepare=True, return_trials=False,
                 corr_cap=0, max_eval=RANSAC_MAX_EVAL, stream=None):
    """One batch of trials (``first_trial .. first_trial + count - 1``) on the device:
    ``(records [n_eval, RANSAC_RECORD_STRIDE] NumPy, trials [count, RANSAC_TRIAL_STRIDE] NumPy or
    None, corr int32 [min(n_eval, corr_cap), n_source] device or None, consumed)``.  At most
    ``max_eval`` trials are evaluated; ``consumed`` is the number of trials the batch dealt with
    (``count``, or up to the first passing trial left out, where the next batch starts).
    ``prepare``: build the target's grid first (needed once per registration while nothing else
    uses the workspace)."""
    src, tgt = _check_xyz(as_point_cloud(source).xyz), _check_xyz(as_point_cloud(target).xyz)
    dev = src.device
    ns, nt, count = src.shape[0], tgt.shape[0], int(count)
    pairs = pairs.to(device=dev, dtype=torch.int64).contiguous()
    L = N.lib()

    def need():
        return L.slg_ransac_ws_bytes(ns, nt, max(count, RANSAC_BATCH))

    if prepare:
        _call(L.slg_ransac_prepare, dev, need, (tgt, nt), (), stream)
    records = torch.empty((count, N.RANSAC_RECORD_STRIDE), dtype=torch.float64, device=dev)
    n_eval = torch.empty(2, dtype=torch.int32, device=dev)
    trials = torch.empty((count, N.RANSAC_TRIAL_STRIDE), dtype=torch.float64, device=dev) if return_trials else None
    corr = torch.empty((int(corr_cap), ns), dtype=torch.int32, device=dev) if corr_cap else None
    ws = _call(L.slg_ransac_batch, dev, need,
               (src, ns, tgt, nt, pairs, pairs.shape[0], int(ransac_n), float(edge_length),
                float(max_correspondence_distance), float(confidence), _seed_i64(seed), int(first_trial), count),
               (int(max_eval), records, n_eval, trials, corr, int(corr_cap)), stream)
    k, consumed = (int(v) for v in n_eval.cpu())
    _check_status(ws, "registration_ransac_based_on_feature_matching")
    return (records[:k].cpu().numpy(), trials.cpu().numpy() if trials is not None else None,
            corr[:min(k, int(corr_cap))] if corr is not None else None, consumed)


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, ransac_n=3, edge_length=0.9,
                                                  max_iteration=100000, confidence=0.999, seed=0,
                                                  stream=None) -> RegistrationResult:
    """Open3D ``registration_ransac_based_on_feature_matching(source, target, source_feature,
    target_feature, mutual_filter, max_correspondence_distance,
    TransformationEstimationPointToPoint(False), 3, [CorrespondenceCheckerBasedOnEdgeLength(
    edge_length), CorrespondenceCheckerBasedOnDistance(max_correspondence_distance)],
    RANSACConvergenceCriteria(max_iteration, confidence))`` on the device, as a pure function of the
    clouds, the features and ``seed`` (``csrc/cloud_ransac.hip``; rules: DESIGN.md §13).

    The correspondences come from :func:`correspondences_from_features` (without the mutual filter
    when it leaves fewer than three).  The device runs the trials in batches of ``RANSAC_BATCH``
    (a batch ends early once ``RANSAC_MAX_EVAL`` of its trials have passed both checkers); per
    batch the records of the trials that passed are read back and :class:`RansacChoice` scans
    them in trial order.  With no passing trial the result is the
    identity with fitness 0."""
    what = "registration_ransac_based_on_feature_matching"
    source, target = _nonempty(source), _nonempty(target)
    d, e, c, it = float(max_correspondence_distance), float(edge_length), float(confidence), int(max_iteration)
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError(f"{what}: max_correspondence_distance must be finite and > 0")
    if not 0.0 <= e <= 1.0:
        raise ValueError(f"{what}: edge_length must lie in [0, 1]")
    if not 0.0 <= c <= 1.0:
        raise ValueError(f"{what}: confidence must lie in [0, 1]")
    if it < 0:
        raise ValueError(f"{what}: max_iteration must be >= 0")
    a, b = _check_features(source_feature, what), _check_features(target_feature, what)
    if a.shape[0] != len(source) or b.shape[0] != len(target):
        raise ValueError(f"{what}: one feature row per point is needed")
    if int(ransac_n) != 3:
        N.lib()
        raise N.NativeError(N.SLG_ERR_UNSUPPORTED, f"{what}: ransac_n must be 3")
    pairs = correspondences_from_features(a, b, bool(mutual_filter), stream)
    if mutual_filter and len(pairs) < 3:
        pairs = correspondences_from_features(a, b, False, stream)
    choice = RansacChoice(len(pairs), it, c)
    log, t0 = [], 0
    while t0 < choice.K:
        count = min(RANSAC_BATCH, it - t0)
        records, _, _, consumed = ransac_batch(source, target, pairs, d, t0, count, e, c, seed, 3, prepare=t0 == 0,
                                               stream=stream)
        for rec in records:
            if not choice.offer(rec):
                break
            log.append(rec)
        t0 += consumed
    log = np.stack(log) if log else np.zeros((0, N.RANSAC_RECORD_STRIDE))
    if choice.best is None:
        res = RegistrationResult(np.eye(4), 0.0, 0.0, choice.K, choice.K < it,
                                 torch.zeros((0, 2), dtype=torch.int64, device=source.xyz.device), log)
        res.trial = -1
        return res
    w = choice.best
    T = w[4:20].reshape(4, 4).copy()
    ev = evaluate_registration(source, target, d, T, stream)         # the winner's correspondences
    res = RegistrationResult(T, float(w[22]), float(w[23]), choice.K, choice.K < it, ev.correspondence_set, log)
    res.trial = int(w[0])
    return res


# ----------------------------------------------------------------------------- plane segmentation
PLANE_BATCH = 256           # trials per slg_plane_batch: one workgroup column of the evaluation, one read-back each
PLANE_PROBABILITY = 0.99999999      # Open3D's default


def plane_max_trials(probability: float, fitness: float, ransac_n: int):
    """``ceil(log(1 - probability) / log(1 - fitness^ransac_n))`` with the power by repeated
    multiplication; ``None`` where the expression bounds nothing (``probability`` 1, or a
    denominator that is not ``< 0``).  For ``0 < fitness < 1``."""
    p = fitness
    for _ in range(int(ransac_n) - 1):
        p = p * fitness
    den = math.log(1.0 - p)
    if not den < 0.0 or probability >= 1.0:
        return None
    return int(math.ceil(math.log(1.0 - probability) / den))


class PlaneChoice:
    """The sequential choice of the plane RANSAC, a sibling of :class:`RansacChoice`,
    fed with every trial's record in ascending trial order: a valid record replaces the best when
    its fitness is larger, or equal with a smaller rmse (ties keep the earlier trial); on a
    replacement, ``fitness == 1`` gives ``K = min(K, t + 1)`` and ``0 < fitness < 1`` gives
    ``K = min(K, max(t + 1, plane_max_trials(probability, fitness, ransac_n)))``.  Records at or
    past ``K`` are ignored."""

    def __init__(self, num_iterations: int, probability: float, ransac_n: int):
        self.K, self.probability, self.ransac_n = int(num_iterations), float(probability), int(ransac_n)
        self.best = None            # the winner's record

    def offer(self, rec) -> bool:
        """False once the record lies at or past ``K`` (so do all later ones)."""
        t = int(rec[0])
        if t >= self.K:
            return False
        if rec[1] == 0.0:
            return True
        fitness, rmse = float(rec[8]), float(rec[9])
        if self.best is None or fitness > self.best[8] or (fitness == self.best[8] and rmse < self.best[9]):
            self.best = rec
            if fitness >= 1.0:
                self.K = min(self.K, t + 1)
            elif fitness > 0.0:
                k = plane_max_trials(self.probability, fitness, self.ransac_n)
                if k is not None:
                    self.K = min(self.K, max(t + 1, k))
        return True


class PlaneSegmentation(tuple):
    """What :func:`segment_plane` returns: the pair ``(plane_model, inliers)`` (NumPy ``[4]``,
    device int64 ascending), which also carries ``trial`` (the winner's trial number, -1: no valid
    trial), ``iterations`` (the final ``K``), ``log`` (NumPy ``[*, PLANE_RECORD_STRIDE]``: the
    record of every trial below ``K``), ``sample_plane`` (the winner's own plane, before the refit),
    ``fitness`` and ``inlier_rmse`` of the winner, and ``sums`` (NumPy ``[PLANE_SUMS_LEN]``: the
    refit's nine sums, centroid and count, or ``None``)."""

    def __new__(cls, plane_model, inliers, trial, iterations, log, sample_plane, fitness, inlier_rmse, sums):
        self = super().__new__(cls, (plane_model, inliers))
        self.plane_model, self.inliers = plane_model, inliers
        self.trial, self.iterations, self.log = trial, iterations, log
        self.sample_plane, self.fitness, self.inlier_rmse, self.sums = sample_plane, fitness, inlier_rmse, sums
        return self


def _seed_i64(seed) -> int:
    sd = int(seed) & 0xFFFFFFFFFFFFFFFF                      # the seed's 64 bits as the int64 the C ABI takes
    return sd - (1 << 64) if sd >> 63 else sd


def _plane_xyz(pc) -> torch.Tensor:
    xyz = _check_xyz(as_point_cloud(pc).xyz)
    return xyz if xyz.data_ptr() % 16 == 0 else xyz.clone()      # the evaluation stages with 16-byte loads


def plane_batch(pc, distance_threshold, first_trial: int, count: int, ransac_n=3, seed=0, stream=None) -> np.ndarray:
    """One batch of trials (``first_trial .. first_trial + count - 1``) on the device: their
    records, NumPy ``[count, PLANE_RECORD_STRIDE]`` (one read-back)."""
    xyz = _plane_xyz(pc)
    n, dev, count = xyz.shape[0], xyz.device, int(count)
    L = N.lib()
    records = torch.empty((count, N.PLANE_RECORD_STRIDE), dtype=torch.float64, device=dev)
    ws = _call(L.slg_plane_batch, dev, lambda: L.slg_plane_ws_bytes(n, max(count, PLANE_BATCH)),
               (xyz, n, float(distance_threshold), int(ransac_n), _seed_i64(seed), int(first_trial), count),
               (records,), stream)
    host = records.cpu().numpy()
    _check_status(ws, "segment_plane")
    return host


def plane_finish(pc, plane, distance_threshold, stream=None):
    """``(inliers int64 device ascending, sums NumPy [PLANE_SUMS_LEN], refitted plane NumPy [4])``
    of a plane: the points with ``dist < distance_threshold`` and ``GetPlaneFromPoints`` over them."""
    xyz = _plane_xyz(pc)
    n, dev = xyz.shape[0], xyz.device
    pl = np.ascontiguousarray(np.asarray(plane, np.float64).reshape(4))
    L = N.lib()
    index = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(N.PLANE_SUMS_LEN + 4, dtype=torch.float64, device=dev)
    ws = _call(L.slg_plane_finish, dev, lambda: L.slg_plane_ws_bytes(n, PLANE_BATCH),
               (xyz, n, _dbl16(pl), float(distance_threshold)), (index, count, out, out[N.PLANE_SUMS_LEN:]), stream)
    host = out.cpu().numpy()
    m = int(count.item())
    _check_status(ws, "segment_plane")
    return index[:m], host[:N.PLANE_SUMS_LEN].copy(), host[N.PLANE_SUMS_LEN:].copy()


def segment_plane(pc, distance_threshold, ransac_n=3, num_iterations=100, probability=PLANE_PROBABILITY, seed=0,
                  stream=None) -> PlaneSegmentation:
    """Open3D ``PointCloud.segment_plane(distance_threshold, ransac_n, num_iterations, probability)``
    on the device, as a pure function of the cloud and ``seed`` (``csrc/cloud_plane.hip``; rules:
    DESIGN.md §14): ``(plane_model, inliers)`` with the plane refitted over the inliers.

    The device runs the trials in batches of ``PLANE_BATCH``; per batch every trial's record is
    read back and :class:`PlaneChoice` scans them in trial order.  With no valid trial the result
    is the plane ``(0, 0, 0, 0)`` with no inliers.  ``3 <= ransac_n <= 8``."""
    what = "segment_plane"
    pc = _nonempty(pc)
    d, rn, it, pr = float(distance_threshold), int(ransac_n), int(num_iterations), float(probability)
    if rn < 3:
        raise ValueError(f"{what}: ransac_n must be >= 3")
    if len(pc) < rn:
        raise ValueError(f"{what}: the cloud has fewer points than ransac_n")
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError(f"{what}: distance_threshold must be finite and > 0")
    if it < 0:
        raise ValueError(f"{what}: num_iterations must be >= 0")
    if not 0.0 < pr <= 1.0:
        raise ValueError(f"{what}: probability must lie in (0, 1]")
    if rn > N.PLANE_MAX_RANSAC_N:
        N.lib()
        raise N.NativeError(N.SLG_ERR_UNSUPPORTED, f"{what}: ransac_n must be <= {N.PLANE_MAX_RANSAC_N}")
    choice = PlaneChoice(it, pr, rn)
    log, t0 = [], 0
    while t0 < choice.K:
        count = min(PLANE_BATCH, choice.K - t0)
        for rec in plane_batch(pc, d, t0, count, rn, seed, stream):
            if not choice.offer(rec):
                break
            log.append(rec)
        t0 += count
    log = np.stack(log) if log else np.zeros((0, N.PLANE_RECORD_STRIDE))
    if choice.best is None:
        return PlaneSegmentation(np.zeros(4), torch.zeros(0, dtype=torch.int64, device=pc.xyz.device), -1, choice.K, log,
                                 np.zeros(4), 0.0, 0.0, None)
    w = choice.best
    inliers, sums, plane = plane_finish(pc, w[2:6], d, stream)
    return PlaneSegmentation(plane, inliers, int(w[0]), choice.K, log, w[2:6].copy(), float(w[8]), float(w[9]), sums)


def remove_plane(pc, distance_threshold, ransac_n=3, num_iterations=1000, seed=0):
    """``segment_plane`` + ``select_by_index(inliers, invert=True)``: ``(the cloud without the
    plane's inliers, the segmentation)``.  Colours are kept, and normals when present; with no
    inliers the input cloud itself comes back."""
    pc = as_point_cloud(pc)
    seg = segment_plane(pc, distance_threshold, ransac_n, num_iterations, seed=seed)
    if len(seg.inliers) == 0:
        return pc, seg
    keep = torch.ones(len(pc), dtype=torch.uint8, device=pc.xyz.device)
    keep[seg.inliers] = 0
    if len(seg.inliers) == len(pc):
        dev = pc.xyz.device
        return PointCloud(torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev),
                          normals=None), seg
    out, idx = select(pc, keep)
    if pc.has_normals():
        out.normals = pc.normals[idx].contiguous()
    return out, seg


# ----------------------------------------------------------------------------- tangent-plane orientation
EMST_LIST_K = 16            # length of the lists euclidean_mst's rounds start from (the tree does not depend on it)


def _check_k(k, what: str) -> int:
    k = int(k)
    if k < 1:
        raise ValueError(f"{what}: k must be >= 1")
    return k


def _sorted_edges(edges: torch.Tensor) -> torch.Tensor:
    """The rows ``(a, b)``, ``a < b < 2^31``, in ascending ``(a, b)`` order."""
    if edges.shape[0] == 0:
        return edges
    key, _ = torch.sort(edges[:, 0] * (1 << 32) + edges[:, 1])
    return torch.stack((key >> 32, key & 0xFFFFFFFF), dim=1)


def knn_lists_raw(pc, k: int, stream=None):
    """``(idx int32 [n, kk], d2 float64 [n, kk])``, ``kk = min(k, n)``, on the device: for every
    point all points in ascending ``(d2, input index)`` order, the point itself included."""
    pc = _nonempty(pc)
    k = _check_k(k, "knn_lists")
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    kk = min(k, n)
    idx = torch.empty((n, kk), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, kk), dtype=torch.float64, device=dev)
    L = N.lib()
    _call(L.slg_knn_lists, dev, lambda: L.slg_orient_ws_bytes(n, k), (xyz, n, k), (idx, d2), stream, "knn_lists")
    return idx, d2


def knn_lists(pc, k: int, stream=None):
    """``(idx int32 [n, k'], d2 float64 [n, k'])``, ``k' = min(k, n) - 1``, on the device: the first
    ``min(k, n)`` points in ascending ``(d2, input index)`` order with the point itself removed
    (Open3D's ``search_knn`` as the orientation uses it).  A row in which the point is not among
    those (``min(k, n)`` or more duplicates with lower indices) loses its last entry instead."""
    idx, d2 = knn_lists_raw(pc, k, stream)
    n, kk = idx.shape
    keep = idx != torch.arange(n, dtype=torch.int32, device=idx.device)[:, None]
    keep[:, kk - 1] &= ~keep.all(dim=1)
    return idx[keep].reshape(n, kk - 1), d2[keep].reshape(n, kk - 1)


def nearest_neighbor_distance(pc, stream=None) -> torch.Tensor:
    """Open3D ``compute_nearest_neighbor_distance``: float64 ``[n]`` on the device, the distance to
    the nearest other point (``0`` for a cloud of fewer than two points)."""
    pc = as_point_cloud(pc)
    if len(pc) < 2:
        return torch.zeros(len(pc), dtype=torch.float64, device=pc.xyz.device)
    return torch.sqrt(knn_lists(pc, 2, stream)[1][:, 0])


def euclidean_mst(pc, return_stats: bool = False, list_k: int = EMST_LIST_K, stream=None):
    """The Euclidean minimum spanning tree under the total edge order ``(d2, a, b)``: int64
    ``[n - 1, 2]`` on the device, rows ``(a, b)`` with ``a < b`` in ascending order.  With
    ``return_stats`` also the int32 ``[ORIENT_STATS_LEN]`` counters of the rounds (host)."""
    pc = _nonempty(pc)
    k = _check_k(list_k, "euclidean_mst")
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    buf = torch.empty((max(n - 1, 1), 2), dtype=torch.int64, device=dev)     # never a NULL buffer
    stats = torch.empty(N.ORIENT_STATS_LEN, dtype=torch.int32, device=dev)
    L = N.lib()
    _call(L.slg_emst, dev, lambda: L.slg_orient_ws_bytes(n, k), (xyz, n, k), (buf, stats), stream, "euclidean_mst")
    edges = _sorted_edges(buf[:n - 1])
    return (edges, stats.cpu().numpy()) if return_stats else edges


def orient_normals_consistent_tangent_plane(pc, k: int, return_tree: bool = False, stream=None):
    """Open3D ``orient_normals_consistent_tangent_plane(k)`` on the device
    (``csrc/cloud_orient.hip``; rules: DESIGN.md §15): a new ``PointCloud`` sharing ``xyz`` /
    ``bgr`` whose normals are the input's, each negated as a whole or left alone.  ``1 <= k <=
    128``; a cloud without normals raises ``RuntimeError`` as Open3D does.  With ``return_tree``:
    ``(cloud, tree int64 [n - 1, 2], root int, info)`` with the Riemannian tree's edges in
    ascending ``(a, b)`` order and ``info = {"emst": edges, "stats": int32 counters}``."""
    pc = _nonempty(pc)
    if not pc.has_normals():
        raise RuntimeError("orient_normals_consistent_tangent_plane: the cloud has no normals (estimate_normals)")
    k = _check_k(k, "orient_normals_consistent_tangent_plane")
    xyz = _check_xyz(pc.xyz)
    n, dev = xyz.shape[0], xyz.device
    nrm = pc.normals.contiguous()
    out = torch.empty_like(nrm)
    emst = torch.empty((n - 1, 2), dtype=torch.int64, device=dev)            # optional outputs: a single point has none
    tree = torch.empty((n - 1, 2), dtype=torch.int64, device=dev)
    root = torch.empty(1, dtype=torch.int64, device=dev)
    stats = torch.empty(N.ORIENT_STATS_LEN, dtype=torch.int32, device=dev)
    L = N.lib()
    _call(L.slg_orient_tangent, dev, lambda: L.slg_orient_ws_bytes(n, k), (xyz, nrm, n, k),
          (out, emst, tree, root, stats), stream, "orient_normals_consistent_tangent_plane")
    res = PointCloud(pc.xyz, pc.bgr, normals=out)
    if not return_tree:
        return res
    return res, _sorted_edges(tree), int(root.item()), {"emst": _sorted_edges(emst), "stats": stats.cpu().numpy()}
