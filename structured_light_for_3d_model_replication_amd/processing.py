"""Drop-in for the hot path of ``server/processing.py`` (class ``ProcessingLogic``).

Same names, signatures, return types and error behaviour as the reference
(``server/processing.py:27-334``); the arithmetic runs in the HIP kernels of ``libslgpu.so``.
The reconstruction path is provided, and of the Open3D post-processing methods of the
reference class (``remove_background`` ... ``mesh_360``, processing.py:336-860) the
deterministic neighbour steps, which run on the device (``cloud.py``): ``remove_outliers``,
``remove_radius_outlier`` and ``keep_largest_cluster``, the post-processing tail of
``merge_pro_360`` (:605-628: voxel down-sample, uniform sample, outlier removal, normals) as
``merge_postprocess``, and the normal estimation and radial orientation that open
``reconstruct_stl`` and ``mesh_360`` (:653-670, :804-837) as ``estimate_oriented_normals``.
``merge_pro_360`` itself (:489-629) runs on the device: point-to-plane ICP, ``transform`` and
``+=`` from initial poses that are given, or, with ``init_transforms="ransac"``,
found as the reference finds them, by FPFH features and a seeded RANSAC global registration
(``preprocess_point_cloud(..., features=True)``, ``execute_global_registration``).
Tangent-plane orientation, Poisson, ball pivoting and RANSAC plane removal are out of scope
(DESIGN.md §Scope).
"""
from __future__ import annotations

import collections
import glob
import os
import threading

import numpy as np
import torch

from . import engine as E
from . import frames as FR
from . import ply as PLY

_TLS = threading.local()                    # .engines: this thread's Reconstructors
_CALIBS: "collections.OrderedDict" = collections.OrderedDict()
_CALIBS_LOCK = threading.Lock()
_CALIBS_MAX = 4


def _engine(h, w):
    """The calling thread's engine for one geometry on the current GPU.  An engine owns a
    workspace that ``slg_decode_stats`` arms for the launch after it, so no two threads may share
    one: each thread gets its own, freed with the thread."""
    engines = getattr(_TLS, "engines", None)
    if engines is None:
        engines = _TLS.engines = {}
    key = (h, w, torch.cuda.current_device())
    if key not in engines:
        engines[key] = E.Reconstructor(h, w)
    return engines[key]


def _hasher():
    try:
        import xxhash
        return xxhash.xxh3_64()
    except ImportError:                     # pragma: no cover - xxhash ships with the image
        import hashlib
        return hashlib.blake2b(digest_size=16)


_NC_SAMPLE = 1 << 16                        # Nc elements hashed by the cheap fingerprint


def _logical_sample(a: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """``a.reshape(-1)[idx]`` (C order) without copying ``a``: a flat view when ``a`` is
    C-contiguous, its transpose's flat view when it is a Fortran-ordered 2-D table."""
    if a.flags.c_contiguous:
        return a.reshape(-1)[idx]
    if a.ndim == 2 and a.flags.f_contiguous:
        r, c = np.divmod(idx, a.shape[1])
        return a.T.reshape(-1)[c * a.shape[0] + r]
    return a[np.unravel_index(idx, a.shape)]


def calib_fingerprint(calib, full: bool = False) -> str:
    """Digest of the calibration arrays the path reads (xxh3 over shapes, dtypes and bytes).

    ``cam_K``, ``Oc`` and the plane tables (<= 131 KB) are always hashed whole.  ``Nc`` (3 x H*W
    float64: 50 MB at 1080p, 576 MB at 24 MP) is hashed whole only with ``full=True``; the cheap
    form hashes its shape, dtype and a strided sample of 65536 elements (first and last
    included, taken by logical index so a Fortran-ordered table -- what ``scipy.io.loadmat``
    returns -- is neither copied nor hashed differently from its C-ordered twin), which costs
    well under a millisecond at any size.  The full form hashes a Fortran-ordered table through
    its C-contiguous transpose (no copy either) and tags the order in the digest."""
    h = _hasher()
    for k in ("cam_K", "Oc", "wPlaneCol", "wPlaneRow", "Nc"):
        a = calib.get(k) if hasattr(calib, "get") else None
        if a is None:
            h.update(f"{k}:none;".encode())
            continue
        a = np.asarray(a)
        h.update(f"{k}:{a.shape}:{a.dtype.str};".encode())
        if k == "Nc" and a.size > _NC_SAMPLE:
            if not full:
                a = _logical_sample(a, np.linspace(0, a.size - 1, _NC_SAMPLE).astype(np.int64))
            elif a.ndim == 2 and not a.flags.c_contiguous and a.flags.f_contiguous:
                h.update(b"F;")
                a = a.T                                # C-contiguous view of the same bytes
        h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    return h.hexdigest()


def _ref(obj):
    import weakref
    try:
        return weakref.ref(obj)
    except TypeError:
        return None


def _device_calib(calib, h, w):
    """Device tables of ``calib`` for one geometry on the current GPU: a small LRU keyed on
    (device, geometry, cheap content digest), so it neither pins callers' dicts nor grows
    without bound, and an edited calibration is uploaded afresh.

    A hit with the very ``Nc`` object of the cached entry costs only the cheap digest.  A hit
    with another ``Nc`` object (e.g. the same ``.mat`` loaded again) is confirmed by the full
    digest of its ``Nc`` against the one taken when the entry was made; a mismatch replaces the
    entry.  (An in-place edit of ``Nc`` entries outside the sample, on the same object, is not
    seen: edit a copy.)

    Threads share the cache: a ``DeviceCalib`` is only read on the device, and its constructor
    returns with the upload finished.  One lock covers the lookup, the upload, the insert and the
    eviction, so two threads that miss on one calibration upload it once."""
    key = (torch.cuda.current_device(), h, w, calib_fingerprint(calib))
    nc = calib.get("Nc") if hasattr(calib, "get") else None
    with _CALIBS_LOCK:
        ent = _CALIBS.get(key)
        if ent is not None:
            dc, ref, full = ent
            if nc is not None and ref is not None and ref() is nc:
                _CALIBS.move_to_end(key)
                return dc
            if calib_fingerprint(calib, full=True) == full:
                _CALIBS[key] = (dc, _ref(nc), full)
                _CALIBS.move_to_end(key)
                return dc
        dc = E.DeviceCalib(calib, h, w)
        _CALIBS[key] = (dc, _ref(nc), calib_fingerprint(calib, full=True))
        _CALIBS.move_to_end(key)
        while len(_CALIBS) > _CALIBS_MAX:
            _CALIBS.popitem(last=False)
        return dc


def _needed_frames(n_files, cfg: E.DecodeConfig):
    """Frame indices the reference reads (processing.py:59-60,88-105)."""
    Bc, Br = E.n_bits(cfg.n_cols), E.n_bits(cfg.n_rows)
    need = [0, 1]
    nc = max(1, min(int(cfg.n_sets_col), Bc))
    nr = max(1, min(int(cfg.n_sets_row), Br))
    idx = 2
    for max_bits, n_use in ((Bc, nc), (Br, nr)):
        for b in range(max_bits):
            if idx + 1 < n_files and b < n_use:
                need += [idx, idx + 1]
            idx += 2
    return need


def read_capture(source, cfg: E.DecodeConfig, order=("bmp", "png")):
    """Discover and decode (host thread pool) one capture: ``(frame stack, texture)``; frames
    the decode does not read stay ``None``.  Host work only (safe on a prefetch thread)."""
    files = FR.discover(source, order)
    if len(files) < 4:
        raise ValueError(f"Not enough images (got {len(files)}, need at least 4).")
    need = _needed_frames(len(files), cfg) if cfg.variant == "processing" else list(range(len(files)))
    imgs, texture = FR.load_frames(files, need, texture=True)
    stack = [None] * len(files)
    for i, im in zip(need, imgs):
        stack[i] = im
    return stack, texture


def has_images(folder: str) -> bool:
    """Batch mode's folder filter (processing.py:320-321)."""
    return bool(glob.glob(os.path.join(folder, "*.bmp")) or glob.glob(os.path.join(folder, "*.png")))


def run_view_folders(subfolders, log, reconstruct, read=None, write=None) -> int:
    """The per-folder loop of batch mode (processing.py:314-334) as a three-stage pipeline.

    ``read(folder) -> host`` (frame read + PNG decode) runs one folder ahead on a prefetch
    thread; ``reconstruct(folder, get_host) -> result`` (H2D, kernels, D2H) on the calling
    thread, where ``get_host()`` waits for that folder's read (so the stage can log its
    progress line first, as the reference does before reading);
    ``write(folder, result) -> out_name`` (ASCII PLY) on a writer thread while the next folder is
    reconstructed.  At most one folder is in each stage.  Per-folder isolation as in the
    reference: an exception in any stage is logged as ``❌ Error in <folder>`` at that folder's
    turn and the loop goes on; folders without images are skipped.  Log order differs from the
    serial loop only in that a folder's ``✔ Saved`` line comes after the next folder's first
    progress lines.  Returns the number of folders that succeeded."""
    from concurrent.futures import ThreadPoolExecutor
    with_imgs = [f for f in subfolders if has_images(f)]
    success = 0
    with ThreadPoolExecutor(max_workers=1) as pre, ThreadPoolExecutor(max_workers=1) as wr:
        pending = {}
        writing = []

        def prefetch(i):
            if read is not None and i < len(with_imgs) and with_imgs[i] not in pending:
                pending[with_imgs[i]] = pre.submit(read, with_imgs[i])

        def drain():
            nonlocal success
            while writing:
                folder, fut = writing.pop()
                try:
                    name = fut.result()
                    success += 1
                    log(f"  ✔ Saved: {name}\n")
                except Exception as e:  # noqa: BLE001 - per-folder isolation like the reference
                    log(f"  ❌ Error in {os.path.basename(folder)}: {e}\n")

        prefetch(0)
        k = 0
        for folder in subfolders:
            if not (k < len(with_imgs) and with_imgs[k] == folder):
                log(f"  Skipping {os.path.basename(folder)} (No images found).")
                continue
            k += 1
            prefetch(k)                                  # the next folder with images
            try:
                fut = pending.pop(folder) if read is not None else None
                result = reconstruct(folder, fut.result if fut is not None else (lambda: None))
            except Exception as e:  # noqa: BLE001
                drain()
                log(f"  ❌ Error in {os.path.basename(folder)}: {e}\n")
                continue
            drain()
            if write is None:
                success += 1
            else:
                writing.append((folder, wr.submit(write, folder, result)))
        drain()
    return success


def load_capture(source, cfg: E.DecodeConfig, order=("bmp", "png"), host=None):
    """Discover, decode and upload one capture: ``(DeviceFrames, texture)``.  ``host``: the
    result of :func:`read_capture` when it was already done (e.g. prefetched)."""
    stack, texture = host if host is not None else read_capture(source, cfg, order)
    return E.DeviceFrames(stack, E.GRAY if _is_frame0(texture, stack) else texture), texture


def _is_frame0(texture, stack) -> bool:
    """Whether the BGR texture is frame 0 replicated (an 8-bit gray capture): the device copy
    then runs in GRAY texture mode and the texture is never uploaded."""
    t = np.asarray(texture)
    f0 = stack[0]
    if f0 is None or t.ndim != 3 or t.shape[2] != 3:
        return False
    f0 = np.asarray(f0)
    return t.shape[:2] == f0.shape and all(np.array_equal(t[..., c], f0) for c in range(3))


def extract_degree(filepath) -> int:
    """Sort key of ``merge_pro_360``'s files (``server/processing.py:499-517``): the integer of the
    first ``_``-separated part of the file name that contains ``deg`` (``doraemon_30deg_scan.ply``
    -> 30); without such a part the last number in the name; 0 when neither parses."""
    import re
    filename = os.path.basename(filepath)
    try:
        for part in filename.split('_'):
            if 'deg' in part:
                return int(part.replace('deg', ''))
        numbers = re.findall(r'\d+', filename)
        if numbers:
            return int(numbers[-1])
    except ValueError:
        pass
    return 0


class ProcessingLogic:
    """Reconstruction half of the reference's ``ProcessingLogic`` (processing.py:12-334)."""

    # --- Multi PLY Processing Functions ---
    @staticmethod
    def _gray_decode(source, n_cols=1920, n_rows=1080,
                     n_sets_col=11, n_sets_row=11,
                     thresh_mode='otsu', shadow_val=40, contrast_val=10):
        """Decode Gray-code images (server/processing.py:28-124).

        ``source``: folder path or sorted file list, as in the reference; additionally a
        ``DeviceFrames`` or a uint8 ``[F, H, W]`` array/tensor already in memory.
        Returns ``(col int32[H,W], row int32[H,W], mask bool[H,W], texture uint8[H,W,3])``.
        """
        cfg = E.DecodeConfig(n_cols, n_rows, n_sets_col, n_sets_row, thresh_mode, shadow_val,
                             contrast_val, "processing")
        if isinstance(source, E.DeviceFrames):
            dev = source
            texture = source.texture_bgr().reshape(dev.height, dev.width, 3).cpu().numpy()
        elif isinstance(source, (np.ndarray, torch.Tensor)) and source.ndim == 3:
            dev = E.DeviceFrames(source)
            texture = dev.texture.reshape(dev.height, dev.width, 3).cpu().numpy()
        else:
            dev, texture = load_capture(source, cfg)
        eng = _engine(dev.height, dev.width)
        col, row, mask = eng.decode(dev, cfg)
        shape = (dev.height, dev.width)
        return (col.reshape(shape).cpu().numpy(), row.reshape(shape).cpu().numpy(),
                mask.reshape(shape).cpu().numpy().astype(bool), texture)

    @staticmethod
    def _reconstruct_point_cloud(col_map, row_map, mask, texture, calib,
                                 row_mode=1, epipolar_tol=2.0):
        """Ray-plane triangulation (server/processing.py:127-234).

        Returns ``(P float64[N,3], C uint8[N,3] BGR)``; ``None`` for a ``row_mode`` other than
        0/1/2 (the reference falls through its if-chain).
        """
        if row_mode not in (0, 1, 2):
            return None
        h, w = np.asarray(col_map).shape
        eng = _engine(h, w)
        dev = eng.device

        def up(a, dt):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
            return t.reshape(-1).to(device=dev, dtype=torch.int32 if dt == np.int32 else torch.uint8)

        col = up(col_map, np.int32)
        row = up(row_map, np.int32) if row_mode != 0 else None
        m = up(np.asarray(mask).astype(np.uint8) if not isinstance(mask, torch.Tensor) else mask, np.uint8)
        tex = up(np.asarray(texture).reshape(-1, 3) if not isinstance(texture, torch.Tensor) else texture, np.uint8)
        dc = _device_calib(calib, h, w)
        out = eng.triangulate(col, row, m, tex, dc, row_mode, epipolar_tol, xyz_f64=True)
        P, C = out.result()
        return P.cpu().numpy(), C.cpu().numpy()

    @staticmethod
    def _save_ply(points, colors, filename):
        """ASCII PLY, byte-identical to server/processing.py:236-248."""
        PLY.write_ascii(filename, points, colors)

    @staticmethod
    def process_multi_ply(calib_path, target_path, mode, log_callback=None,
                          n_sets_col=11, n_sets_row=11,
                          row_mode=1, epipolar_tol=2.0,
                          thresh_mode='otsu', shadow_val=40, contrast_val=10,
                          file_list=None, out_path_override=None):
        """Process structured-light images -> .ply point cloud (server/processing.py:251-334).

        Each view runs the fused decode+triangulate kernel (maps never leave the chip)."""
        def log(msg):
            if log_callback: log_callback(msg)
            else: print(msg)

        log("Loading Calibration Data...")
        import scipy.io
        data = scipy.io.loadmat(calib_path)
        calib_data = {
            "Nc": data["Nc"], "Oc": data["Oc"],
            "wPlaneCol": data["wPlaneCol"], "wPlaneRow": data["wPlaneRow"],
            "cam_K": data["cam_K"]
        }
        cfg = E.DecodeConfig(1920, 1080, n_sets_col, n_sets_row, thresh_mode, shadow_val,
                             contrast_val, "processing")

        def _process_source(source, out_path, label, host=None):
            log(f"  -> Decoding {label}  "
                f"[col-sets={n_sets_col}  row-sets={n_sets_row}]...")
            dev, _ = load_capture(source, cfg, host=None if host is None else host.result())
            log("  -> Reconstructing 3D points...")
            points, colors = reconstruct_view(dev, cfg, calib_data, row_mode, epipolar_tol)
            log(f"  -> Saving {len(points)} points...")
            ProcessingLogic._save_ply(points, colors, out_path)
            log(f"  ✔ Saved: {os.path.basename(out_path)}\n")

        if mode == "files":
            if not file_list:
                raise ValueError("mode='files' requires a non-empty file_list.")
            if not out_path_override:
                raise ValueError("mode='files' requires out_path_override.")
            _process_source(file_list, out_path_override,
                            f"{len(file_list)} selected files")

        elif mode == "single":
            ply_name = os.path.basename(target_path) + ".ply"
            out_path = os.path.join(target_path, ply_name)
            _process_source(target_path, out_path,
                            f"folder '{os.path.basename(target_path)}'")

        else:  # batch
            subfolders = [f.path for f in os.scandir(target_path) if f.is_dir()]
            log(f"Found {len(subfolders)} subfolders to process.")

            # A host/GPU pipeline (pipeline.BatchPipeline): frames decoded ahead into pinned
            # memory, groups of views uploaded asynchronously and reconstructed by one batched
            # launch, PLYs written on a writer thread; per-folder errors and log lines as in
            # the reference.
            from .pipeline import BatchPipeline
            success_count = BatchPipeline(cfg, calib_data, row_mode, epipolar_tol, group=batch_views(),
                                          log=log).run(subfolders, batch_write_stage())
            log(f"=== Batch Complete: {success_count}/{len(subfolders)} succeeded ===")

    # --- Cleanup filters (device; cloud.py) ---
    @staticmethod
    def _load_pcd(input_data):
        """``server/processing.py:15-24``: a path is read (``FileNotFoundError`` when missing),
        anything else is taken as a cloud already in memory."""
        from . import cloud as CL
        if isinstance(input_data, str):
            if not os.path.exists(input_data):
                raise FileNotFoundError(f"Input file not found: {input_data}")
            return CL.PointCloud.from_file(input_data)
        return CL.as_point_cloud(input_data)

    @staticmethod
    def remove_background(input_data, output_path=None, distance_threshold=50, ransac_n=3, num_iterations=1000,
                          return_obj=False, seed=0):
        """Back-wall removal on the device (``server/processing.py:337-364``): the seeded RANSAC
        plane segmentation of ``cloud.segment_plane``, then the cloud without the
        plane's inliers, with its colours (and normals, when it has them).

        The reference's signature plus ``seed`` (the result is a pure function of the cloud and
        the seed), its print lines and exceptions; the same two differences from the reference as
        :meth:`remove_outliers`."""
        from . import cloud as CL
        print(f"[BG Remove] Processing...")
        pcd = ProcessingLogic._load_pcd(input_data)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        object_cloud, _ = CL.remove_plane(pcd, distance_threshold, ransac_n, num_iterations, seed=seed)
        print(f"[BG Remove] Original: {len(pcd)}, Remaining: {len(object_cloud)} pts")
        if output_path:
            ProcessingLogic._save_ply(*object_cloud.numpy(), output_path)
            print(f"[BG Remove] Saved to {output_path}")
        return object_cloud if return_obj else None

    @staticmethod
    def remove_outliers(input_data, output_path=None, nb_neighbors=20, std_ratio=2.0, return_obj=False):
        """Statistical outlier removal on the device (``server/processing.py:367-388``).

        Same signature, print lines and exceptions as the reference.  Two differences: the object
        taken and returned is a ``cloud.PointCloud`` (not an Open3D one), and ``output_path`` is
        written by ``_save_ply`` (ASCII PLY, which Open3D reads) instead of Open3D's binary PLY.
        ``input_data``: a path to a PLY that ``_save_ply`` wrote, or a ``PointCloud``."""
        from . import cloud as CL
        print(f"[Outlier] Processing...")
        pcd = ProcessingLogic._load_pcd(input_data)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        inlier_cloud = CL.statistical_outlier(pcd, nb_neighbors, std_ratio)
        print(f"[Outlier] Keeping: {len(inlier_cloud)} pts")
        if output_path:
            ProcessingLogic._save_ply(*inlier_cloud.numpy(), output_path)
            print(f"[Outlier] Saved to {output_path}")
        return inlier_cloud if return_obj else None

    @staticmethod
    def remove_radius_outlier(input_data, output_path=None, nb_points=100, radius=5.0, return_obj=False):
        """Radius outlier removal on the device (``server/processing.py:430-448``); the same two
        differences from the reference as :meth:`remove_outliers`."""
        from . import cloud as CL
        print(f"[Radius Outlier] Processing...")
        pcd = ProcessingLogic._load_pcd(input_data)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        inlier_cloud = CL.radius_outlier(pcd, nb_points, radius)
        print(f"[Radius Outlier] Keeping: {len(inlier_cloud)} pts")
        if output_path:
            ProcessingLogic._save_ply(*inlier_cloud.numpy(), output_path)
            print(f"[Radius Outlier] Saved to {output_path}")
        return inlier_cloud if return_obj else None

    @staticmethod
    def keep_largest_cluster(input_data, output_path=None, eps=5.0, min_points=200, return_obj=False):
        """DBSCAN on the device, then only the largest cluster (``server/processing.py:391-427``);
        the same two differences from the reference as :meth:`remove_outliers`.  When every point
        is noise the input cloud comes back before any save, as in the reference."""
        from . import cloud as CL
        print(f"[Cluster] Processing...")
        pcd = ProcessingLogic._load_pcd(input_data)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        cleaned_pcd = CL.largest_cluster(pcd, eps, min_points)
        if cleaned_pcd is pcd:               # no cluster at all
            return pcd if return_obj else None
        print(f"[Cluster] Kept largest group: {len(cleaned_pcd)} pts")
        if output_path:
            ProcessingLogic._save_ply(*cleaned_pcd.numpy(), output_path)
            print(f"[Cluster] Saved to {output_path}")
        return cleaned_pcd if return_obj else None

    # --- Merge tail and mesh front (device; cloud.py) ---
    @staticmethod
    def merge_postprocess(merged, output_path=None, voxel_size=0.02, outlier_nb=20, outlier_std=2.0,
                          sample_after=1, final_voxel=0.5, return_obj=False):
        """The post-processing tail of ``merge_pro_360`` (``server/processing.py:605-628``) on the
        device; the reference has no stand-alone method for it.  Same order of steps, conditions
        and print lines: final voxel down-sample when ``final_voxel > 0``, uniform sample when
        ``sample_after > 1``, statistical outlier removal (``outlier_nb``, ``outlier_std``), normals
        with ``radius = voxel_size * 2`` and ``max_nn = 30``, then the save.  ``merged``: a path,
        a ``PointCloud`` or ``(P, C)``.  ``output_path`` is written as ASCII PLY with normals (the
        reference writes Open3D's binary PLY)."""
        from . import cloud as CL
        pcd_combined_down = ProcessingLogic._load_pcd(merged)
        if not pcd_combined_down.has_points():
            raise ValueError("Point cloud is empty.")
        print(f"[Merge 360] Post-processing (Final Voxel: {final_voxel}, Outlier removal)...")
        if final_voxel > 0:
            pcd_combined_down = CL.voxel_down_sample(pcd_combined_down, final_voxel)
            print(f"  After final voxel down-sample: {len(pcd_combined_down)} points")
        if sample_after > 1:
            pcd_combined_down = CL.uniform_down_sample(pcd_combined_down, int(sample_after))
            print(f"  After uniform sample-after: {len(pcd_combined_down)} points")
        pcd_final = CL.statistical_outlier(pcd_combined_down, outlier_nb, outlier_std)
        print(f"  After outlier removal: {len(pcd_final)} points (removed {len(pcd_combined_down) - len(pcd_final)})")
        if pcd_final.has_points():
            pcd_final = CL.estimate_normals(pcd_final, voxel_size * 2, 30)
        if output_path:
            pcd_final.save(output_path)
            print(f"[Merge 360] Saved merged cloud to {output_path}")
        return pcd_final if return_obj else None

    # --- 360-degree merge (device; cloud.py) ---
    @staticmethod
    def preprocess_point_cloud(pcd, voxel_size, features=False):
        """The reference's ``preprocess_point_cloud`` (``server/processing.py:451-468``) on the
        device: voxel down-sample at ``voxel_size``, normals with ``radius = voxel_size * 2`` and
        ``max_nn = 30``, and, with ``features=True``, the FPFH features with
        ``radius = voxel_size * 5`` and ``max_nn = 100`` (device float64 ``[n, 33]``).  Returns
        ``(pcd_down, fpfh)``; without ``features`` (the default, for scans whose poses are known)
        ``None`` stands in the feature's place."""
        from . import cloud as CL
        pcd_down = CL.voxel_down_sample(pcd, voxel_size)
        pcd_down = CL.estimate_normals(pcd_down, voxel_size * 2, 30)
        return pcd_down, (CL.compute_fpfh_feature(pcd_down, voxel_size * 5, 100) if features else None)

    @staticmethod
    def execute_global_registration(source_down, target_down, source_fpfh, target_fpfh, voxel_size, icp_dist_ratio=1.5,
                                    seed=0):
        """The reference's ``execute_global_registration`` (``server/processing.py:470-486``) on
        the device with its fixed parameters: the mutual filter, the distance
        ``voxel_size * icp_dist_ratio`` for the correspondences and the distance checker, three
        points per trial, the edge-length checker at 0.9, and the criteria (100000, 0.999).  The
        result is a function of the inputs and ``seed``."""
        from . import cloud as CL
        distance_threshold = voxel_size * icp_dist_ratio
        return CL.registration_ransac_based_on_feature_matching(
            source_down, target_down, source_fpfh, target_fpfh, True, distance_threshold, ransac_n=3, edge_length=0.9,
            max_iteration=100000, confidence=0.999, seed=seed)

    @staticmethod
    def merge_pro_360(input_folder, output_path, voxel_size=0.02, icp_dist_ratio=1.5, outlier_nb=20, outlier_std=2.0,
                      sample_before=1, sample_after=1, final_voxel=0.5, step_callback=None, init_transforms=None,
                      seed=0):
        """Sequential merge of a folder of per-view PLY files (``server/processing.py:489-629``)
        on the device.

        File discovery, the degree sort, the errors and the print lines are the reference's.  Per
        step both clouds are pre-processed (:meth:`preprocess_point_cloud`), the initial transform
        of scan ``i`` onto scan ``i - 1`` is found, point-to-plane ICP runs on the device with
        ``voxel_size`` as the correspondence distance, the transform is accumulated, and the
        full-resolution source is transformed and appended.

        ``init_transforms="ransac"`` finds the initial transform as the reference does: FPFH
        features and :meth:`execute_global_registration` with the distance
        ``voxel_size * icp_dist_ratio``, printing the reference's ``[RANSAC]`` lines.  Step ``i``
        uses the seed ``seed + i``, so a merge is a function of its files and ``seed``.  Otherwise
        the transform is taken from ``init_transforms`` (a sequence of 4x4 matrices, entry
        ``i - 1`` for step ``i``, or a callable ``(i, source_down, target_down) -> 4x4``; ``None``:
        the identity, for scans already posed) and ``icp_dist_ratio`` and ``seed`` are unused.
        ``step_callback(i, total_steps, accumulated_cloud)`` gets a ``cloud.PointCloud``.  The tail
        is :meth:`merge_postprocess`; ``output_path`` is ASCII PLY with normals."""
        from . import cloud as CL
        use_ransac = isinstance(init_transforms, str)
        if use_ransac and init_transforms != "ransac":
            raise ValueError(f"init_transforms: {init_transforms!r} is not 'ransac', a sequence, a callable or None")
        print(f"[Merge 360] Loading clouds from {input_folder}...")
        ply_files = sorted(glob.glob(os.path.join(input_folder, "*.ply")), key=extract_degree)
        print(f"[Merge 360] Sorted file order:")
        for idx, f in enumerate(ply_files):
            print(f"  [{idx}] {os.path.basename(f)}")
        if len(ply_files) < 2:
            raise ValueError("Need at least 2 .ply files to merge.")
        pcds = []
        for path in ply_files:
            pcd = CL.PointCloud.from_file(path)
            if not pcd.has_points():
                raise ValueError(f"Loaded empty point cloud from: {path}")
            if sample_before > 1:
                pcd = CL.uniform_down_sample(pcd, int(sample_before))
            pcds.append(pcd)
            print(f"  Loaded: {os.path.basename(path)} ({len(pcd)} points)")
        total_steps = len(pcds) - 1
        print(f"[Merge 360] Loaded {len(pcds)} clouds. Running Sequential Registration ({total_steps} steps)...")
        merged_cloud = pcds[0]
        max_accum_T = np.identity(4)
        for i in range(1, len(pcds)):
            print(f"\n[Merge 360] === Step {i}/{total_steps}: Aligning Scan {i} -> Scan {i-1} ===")
            source, target = pcds[i], pcds[i - 1]
            source_down, source_fpfh = ProcessingLogic.preprocess_point_cloud(source, voxel_size, features=use_ransac)
            target_down, target_fpfh = ProcessingLogic.preprocess_point_cloud(target, voxel_size, features=use_ransac)
            print(f"  Preprocessed: source={len(source_down)} pts, target={len(target_down)} pts (voxel={voxel_size})")
            if use_ransac:
                ransac_result = ProcessingLogic.execute_global_registration(
                    source_down, target_down, source_fpfh, target_fpfh, voxel_size, icp_dist_ratio, seed=seed + i)
                print(f"  [RANSAC] Fitness: {ransac_result.fitness:.4f} | RMSE: {ransac_result.inlier_rmse:.6f}")
                if ransac_result.fitness < 0.05:
                    print(f"  [WARNING] Step {i}: RANSAC fitness is very low ({ransac_result.fitness:.4f})! "
                          f"Alignment may be unreliable. Try lowering Voxel Size or increasing ICP Dist Ratio.")
                init = ransac_result.transformation
            else:
                if init_transforms is None:
                    init = np.identity(4)
                elif callable(init_transforms):
                    init = init_transforms(i, source_down, target_down)
                else:
                    init = init_transforms[i - 1]
                print("  [RANSAC] skipped: initial transform given")
            icp_result = CL.registration_icp(source_down, target_down, voxel_size, init)
            print(f"  [ICP]    Fitness: {icp_result.fitness:.4f} | RMSE: {icp_result.inlier_rmse:.6f}")
            if icp_result.fitness < 0.05:
                print(f"  [WARNING] Step {i}: ICP fitness is very low ({icp_result.fitness:.4f})! "
                      f"This step's alignment is likely incorrect and WILL corrupt all subsequent steps. "
                      f"Consider adjusting parameters or checking if all PLY files are valid.")
            max_accum_T = np.dot(max_accum_T, icp_result.transformation)
            merged_cloud = CL.concat(merged_cloud, CL.transform(source, max_accum_T))
            print(f"  [Merge 360] Step {i}/{total_steps} complete. Accumulated cloud: {len(merged_cloud)} points total.")
            if step_callback is not None:
                step_callback(i, total_steps, merged_cloud)      # concat made a new cloud: nothing to protect
        print(f"\n[Merge 360] All {total_steps} steps complete. Running post-processing...")
        ProcessingLogic.merge_postprocess(merged_cloud, output_path, voxel_size, outlier_nb, outlier_std, sample_after,
                                          final_voxel)

    @staticmethod
    def estimate_oriented_normals(input_data, save_normals_path=None, normal_radius=0.1, normal_max_nn=30,
                                  outward=True, return_obj=False, orientation_mode="radial", tangent_k=100,
                                  consistency_pass=False, consistency_k=30):
        """Steps 1-2b of ``mesh_360`` (``server/processing.py:804-837``) on the device; the
        reference has no stand-alone method for them.  Normals by the hybrid search
        (``normal_radius``, ``normal_max_nn``), then, by ``orientation_mode``: ``"radial"``: oriented
        towards the cloud's centre and then, with ``outward``, negated (with ``normal_radius=10``
        this is ``reconstruct_stl``'s centroid branch, ``:653-670``); ``"tangent"``: the reference's
        default, ``orient_normals_consistent_tangent_plane(tangent_k)`` (``:823``, ``:675``), with
        the reference's fall-back to radial when that raises.  ``consistency_pass`` runs the
        tangent-plane orientation once more afterwards with ``consistency_k`` neighbours (30 when
        not positive), as ``reconstruct_stl`` does (``:682-686``).  Raises ``FileNotFoundError`` for
        a missing path, ``ValueError("Point cloud is empty.")`` as the reference does, and
        ``ValueError`` for an unknown mode.  ``save_normals_path`` is written as ASCII PLY with
        normals."""
        from . import cloud as CL
        if orientation_mode not in ("radial", "tangent"):
            raise ValueError(f"orientation_mode must be 'radial' or 'tangent', not {orientation_mode!r}")
        if orientation_mode == "tangent" and int(tangent_k) < 1:
            raise ValueError("tangent_k must be >= 1")
        pcd = ProcessingLogic._load_pcd(input_data)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        print(f"[360 Mesh] Estimating normals (radius={normal_radius}, max_nn={normal_max_nn})...")
        pcd = CL.estimate_normals(pcd, normal_radius, normal_max_nn)
        print(f"[360 Mesh] Re-orienting normals (Mode: {orientation_mode})...")
        if orientation_mode == "tangent":
            try:
                pcd = CL.orient_normals_consistent_tangent_plane(pcd, int(tangent_k))
                print("[360 Mesh] Consistent tangent plane orientation applied.")
            except Exception as e:
                print(f"[360 Mesh] Warning: Tangent plane failed ({e}). Fallback to radial.")
                pcd = CL.orient_normals_towards(pcd, CL.centroid(pcd), outward=True)
        else:
            pcd = CL.orient_normals_towards(pcd, CL.centroid(pcd), outward=outward)
            if outward:
                print("[360 Mesh] Radial orientation applied (Outwards).")
        if consistency_pass:
            k = int(consistency_k) if consistency_k > 0 else 30
            print(f"[Recon] Consistency pass: orient_normals_consistent_tangent_plane(k={k})...")
            pcd = CL.orient_normals_consistent_tangent_plane(pcd, k)
            print("[Recon] Consistency pass applied.")
        if save_normals_path:
            print(f"[360 Mesh] Saving normals point cloud to {save_normals_path}...")
            pcd.save(save_normals_path)
            print(f"[360 Mesh] Normals point cloud saved ({len(pcd)} points).")
        return pcd if return_obj else None

    @staticmethod
    def _check_grid_poisson(depth, width=0.0, linear_fit=False):
        """What the dense grid takes of ``create_from_point_cloud_poisson``'s arguments."""
        from . import mesh as MS
        depth = int(depth)
        if depth > 16:
            raise ValueError(f"Depth {depth} is too high! Maximum recommended is 12-14. >16 will freeze your PC.")
        if float(width) != 0.0 or linear_fit:
            raise ValueError("width != 0 and linear_fit=True are not implemented on the dense grid")
        return MS.check_depth(depth)

    @staticmethod
    def _check_band_poisson(rule, depth, base_depth=None, band_sweeps=None, width=0.0, linear_fit=False):
        """The arguments of ``mesh.poisson_band`` when ``rule`` is ``"band"``: the depth in
        3..12, the reference's message above 16 and the grid's ``width`` / ``linear_fit`` refusal as
        they are.  ``None`` without the key; any other rule is a ``ValueError``."""
        from . import mesh as MS
        if rule is None:
            return None
        if rule != "band":
            raise ValueError(f"unknown poisson_rule {rule!r} (\"band\": mesh.poisson_band)")
        depth = int(depth)
        if depth > 16:
            raise ValueError(f"Depth {depth} is too high! Maximum recommended is 12-14. >16 will freeze your PC.")
        if float(width) != 0.0 or linear_fit:
            raise ValueError("width != 0 and linear_fit=True are not implemented on the dense grid")
        depth, base = MS.check_band_depth(depth, base_depth)
        sweeps = MS.DEFAULT_BAND_SWEEPS if band_sweeps is None else band_sweeps
        if isinstance(sweeps, bool) or not isinstance(sweeps, (int, float)) or float(sweeps) != int(sweeps) or int(sweeps) < 0:
            raise ValueError(f"band_sweeps must be a whole number >= 0, not {band_sweeps!r}")
        return dict(depth=depth, base_depth=base, sweeps=int(sweeps))

    @staticmethod
    def _surface_multipliers(radii_str):
        """``params["radii"]`` parsed as the reference does (``server/processing.py:720``), and what
        ``mesh.check_radii`` will ask of their multiples of a positive distance, asked here."""
        from . import mesh as MS
        try:
            multipliers = [float(x) for x in radii_str.split(',')]
            MS.check_radii(sorted(set(multipliers)), "reconstruct_stl")
        except Exception as e:
            raise ValueError(f"Invalid radii parameters: {e}")
        return multipliers

    @staticmethod
    def _write_mesh(mesh, output_path, tag):
        from . import mesh as MS
        MS.compute_triangle_normals(mesh)
        MS.write_stl(output_path, mesh)
        print(f"[{tag}] Saved STL to {output_path}")

    @staticmethod
    def reconstruct_stl(input_path, output_path, mode="watertight", params=None, centroid_orient=True,
                        consistency_pass=False, consistency_k=30, meshlab_params=None, save_normals_path=None):
        """``server/processing.py:632-787`` on the device: normals (estimated at radius 10 / 30
        when the file has none), the centroid or tangent-plane orientation, the optional consistency
        pass, then ``mesh.poisson_grid`` at ``params["depth"]`` (default 10), the 0.02 density
        quantile trim and a binary STL.  The mesher is the dense grid's, so a depth
        above 10 raises ``ValueError`` unless ``params["poisson_rule"] == "band"`` asks for
        ``mesh.poisson_band`` (the banded cascade, depth 3..12, with the optional
        ``params["base_depth"]`` and ``params["band_sweeps"]``; closed wherever the surface stays within
        the band around the points, and the trim applies as before; any other rule is a
        ``ValueError``); ``mode="surface"`` (ball pivoting) raises
        ``NotImplementedError``: Open3D's front stays in the reference.  With
        ``params["surface_rule"] == "empty_ball"`` it runs ``mesh.ball_pivot`` instead (DESIGN.md
        §20: the empty-ball triangles, our rule and not Open3D's front) at the radii
        ``np.mean(nearest_neighbor_distance) * m`` for the multipliers ``m`` of ``params["radii"]``
        (default ``"1,2,4"``), sorted ascending without duplicates; what goes wrong there is a
        ``ValueError("Invalid radii parameters: ...")`` as in the reference, a mesh without a
        triangle ``ValueError("Generated mesh is empty.")``, any other rule a ``ValueError``.
        The MeshLab step is restated literally
        (it needs ``pymeshlab``) unless ``meshlab_params["backend"] == "device"``: then the STL is
        written first as always, ``mesh.postprocess`` (smoothing and hole closing,
        our rules) runs on the float64 mesh in memory and the file is overwritten.  MeshLab would
        reload the STL's float32 vertices instead.  ``simplify`` with this backend and
        ``"simplify_rule": "rounds"`` runs ``mesh.decimate_quadric`` to ``target_faces`` (default
        50,000) after the hole closing (quadric edge collapse in independent rounds,
        our rule and not MeshLab's sequential queue); ``simplify`` without that key raises
        ``NotImplementedError`` (``server/processing.py:778-781``), any other rule or a bad
        ``target_faces`` ``ValueError``, all before anything is loaded.  The device backend also
        takes ``"keep_components"``, ``"min_component_faces"``, ``"clean"`` and ``"audit"``
        (``mesh.postprocess``); with ``"audit": True`` one ``[Mesh] audit: ...`` line
        gives the final mesh's counts and verdict, and with ``"self_intersections": True`` a second
        ``[Mesh] intersections: ...`` line says which of its triangles cross (``mesh.self_intersections``,
        DESIGN.md §23).  With another backend these keys are a ``ValueError``."""
        from . import cloud as CL
        from . import mesh as MS
        if not os.path.exists(input_path):
            raise FileNotFoundError(f"Input file not found: {input_path}")
        params = params or {}
        if mode == "watertight":
            band = ProcessingLogic._check_band_poisson(params.get("poisson_rule"), params.get("depth", 10),
                                                       params.get("base_depth"), params.get("band_sweeps"))
            depth = band["depth"] if band else ProcessingLogic._check_grid_poisson(params.get("depth", 10))
            MS.check_stl_path(output_path)
        elif mode == "surface":
            rule = params.get("surface_rule")
            if rule is None:
                raise NotImplementedError("mode='surface' (ball pivoting) is a sequential front propagation and stays in the "
                                          "reference (server/processing.py:711-728); \"surface_rule\": \"empty_ball\" asks for "
                                          "the device's own rule instead (mesh.ball_pivot)")
            if rule != "empty_ball":
                raise ValueError(f"reconstruct_stl: unknown surface_rule {rule!r} (\"empty_ball\": mesh.ball_pivot)")
            multipliers = ProcessingLogic._surface_multipliers(params.get("radii", "1,2,4"))
            MS.check_stl_path(output_path)
        else:
            raise ValueError(f"Unknown mode: {mode}")
        backend = meshlab_params.get("backend", "pymeshlab") if meshlab_params and meshlab_params.get("enabled") else None
        if backend not in (None, "pymeshlab", "device"):
            raise ValueError(f"Unknown meshlab_params backend: {backend!r} (\"pymeshlab\" or \"device\")")
        device_post = backend == "device"
        if device_post:
            MS.check_postprocess(meshlab_params)
        elif backend is not None and any(k in meshlab_params for k in MS._AUDIT_KEYS):
            raise ValueError("meshlab_params: keep_components, min_component_faces, clean, audit and self_intersections belong to "
                             "\"backend\": \"device\" (mesh.postprocess)")
        print(f"[Recon] Loading {input_path}...")
        pcd = CL.PointCloud.from_file(input_path)
        if not pcd.has_points():
            raise ValueError("Point cloud is empty.")
        if not pcd.has_normals():
            print("[Recon] Estimating normals...")
            pcd = CL.estimate_normals(pcd, 10, 30)
        if centroid_orient:
            pcd = CL.orient_normals_towards(pcd, CL.centroid(pcd), outward=True)
            print("[Recon] Centroid-based outward orientation applied.")
        else:
            print("[Recon] Using tangent-plane graph consistency for normal orientation...")
            pcd = CL.orient_normals_consistent_tangent_plane(pcd, 100)
            print("[Recon] Graph orientation applied.")
        if consistency_pass:
            k = int(consistency_k) if consistency_k > 0 else 30
            print(f"[Recon] Consistency pass: orient_normals_consistent_tangent_plane(k={k})...")
            pcd = CL.orient_normals_consistent_tangent_plane(pcd, k)
            print("[Recon] Consistency pass applied.")
        if save_normals_path:
            print(f"[Recon] Saving normals point cloud to {save_normals_path}...")
            pcd.save(save_normals_path)
            print(f"[Recon] Normals point cloud saved ({len(pcd)} points).")
        if mode == "watertight":
            print(f"[Recon] Poisson Reconstruction (depth={depth})...")
            mesh = MS.poisson_band(pcd, **band) if band else MS.poisson_grid(pcd, depth=depth)
            if len(mesh.vertices):
                mesh = MS.remove_vertices_by_mask(mesh, mesh.densities < MS.quantile(mesh.densities, 0.02))
        else:
            try:
                avg_dist = np.mean(CL.nearest_neighbor_distance(pcd).cpu().numpy())
                radii = sorted({avg_dist * m for m in multipliers})
                print(f"[Recon] Ball Pivoting (radii={radii})...")
                mesh = MS.ball_pivot(pcd, radii)
            except Exception as e:
                raise ValueError(f"Invalid radii parameters: {e}")
        # Open3D keeps every point as a vertex, so does ball_pivot: without a triangle the mesh is empty.
        # mesh.postprocess takes unreferenced vertices as they are (empty adjacency rows).
        if len(mesh.vertices) == 0 or (mode == "surface" and len(mesh.triangles) == 0):
            raise ValueError("Generated mesh is empty.")
        print("[Recon] Computing normals and saving...")
        ProcessingLogic._write_mesh(mesh, output_path, "Recon")
        if device_post:
            print("[MeshLab] Starting post-processing (device backend)...")
            mesh, audit = MS.postprocess(mesh, meshlab_params, return_record=True)
            ProcessingLogic._write_mesh(mesh, output_path, "MeshLab")
            if audit is not None and "watertight" in audit:
                print(f"[Mesh] audit: {MS.format_audit(audit)}")
            if audit is not None and "self_intersections" in audit:
                print(f"[Mesh] intersections: {MS.format_intersections(audit['self_intersections'])}")
            print(f"[MeshLab] Post-processing complete. Final: {len(mesh.vertices)} vertices, "
                  f"{len(mesh.triangles)} faces. Saved to {output_path}")
        elif meshlab_params and meshlab_params.get("enabled"):
            print("[MeshLab] Starting post-processing...")
            try:
                import pymeshlab
            except ImportError:
                raise ImportError(
                    "pymeshlab is not installed. Run: pip install pymeshlab\n"
                    "The STL has already been saved using Open3D only (without MeshLab improvements)."
                )
            ms = pymeshlab.MeshSet()
            ms.load_new_mesh(output_path)
            smooth_type = str(meshlab_params.get("smooth_type", "taubin"))
            smooth_iters = int(meshlab_params.get("smooth_iters", 10))
            if smooth_type == "laplacian":
                ms.apply_coord_laplacian_smoothing(stepsmoothnum=smooth_iters)
            else:
                ms.apply_coord_taubin_smoothing(stepsmoothnum=smooth_iters)
            if meshlab_params.get("close_holes"):
                ms.meshing_close_holes(maxholesize=int(meshlab_params.get("close_max_size", 30)))
            if meshlab_params.get("simplify"):
                ms.meshing_decimation_quadric_edge_collapse(targetfacenum=int(meshlab_params.get("target_faces", 50000)))
            ms.save_current_mesh(output_path)
            final = ms.current_mesh()
            print(f"[MeshLab] Post-processing complete. Final: {final.vertex_number()} vertices, "
                  f"{final.face_number()} faces. Saved to {output_path}")

    @staticmethod
    def mesh_360(input_path, output_path, depth=10, density_trim=0.01, orientation_mode="tangent", width=0.0,
                 scale=1.1, linear_fit=False, n_threads=-1, normal_radius=0.1, normal_max_nn=30,
                 save_normals_path=None, poisson_rule=None, base_depth=None, band_sweeps=None, *, self_intersections=False,
                 keep_components=None, audit=False):
        """``server/processing.py:790-860`` on the device: :meth:`estimate_oriented_normals`
        (``"radial"``, or the tangent-plane orientation with its fall-back for any other mode, as
        the reference's ``else``), ``mesh.poisson_grid(depth, scale)``, the ``density_trim`` quantile
        trim when positive, and a binary STL.  ``width != 0`` and ``linear_fit=True`` raise
        ``ValueError`` (not implemented on the grid), as does a depth above 10; ``n_threads`` is
        ignored.  ``poisson_rule="band"`` runs ``mesh.poisson_band(depth, base_depth, band_sweeps,
        scale)`` instead (depth 3..12); ``base_depth`` or ``band_sweeps`` without it, or any
        other rule, is a ``ValueError``.  ``keep_components=k`` keeps the ``k`` largest connected
        components of the trimmed mesh (``mesh.keep_largest_components``: the trim tears scraps off
        the closure) and ``audit=True`` prints one ``[Mesh] audit: ...`` line with the counts and the
        verdict of the mesh that is written (``mesh.audit``); a ``keep_components``
        that is no whole number >= 1 is a ``ValueError``.  ``self_intersections=True`` prints a
        ``[Mesh] intersections: ...`` line for that mesh (``mesh.self_intersections``)."""
        from . import mesh as MS
        if not os.path.exists(input_path):
            raise FileNotFoundError(f"Input file not found: {input_path}")
        if poisson_rule is None and (base_depth is not None or band_sweeps is not None):
            raise ValueError("base_depth and band_sweeps belong to poisson_rule=\"band\"")
        band = ProcessingLogic._check_band_poisson(poisson_rule, depth, base_depth, band_sweeps, width, linear_fit)
        depth = band["depth"] if band else ProcessingLogic._check_grid_poisson(depth, width, linear_fit)
        if not (float(scale) >= 1.0):
            raise ValueError(f"scale must be >= 1 on the dense grid, not {scale}")
        MS.check_postprocess({k: v for k, v in (("keep_components", keep_components), ("audit", audit),
                                                  ("self_intersections", self_intersections)) if v is not None})
        MS.check_stl_path(output_path)
        print(f"[360 Mesh] Loading {input_path}...")
        pcd = ProcessingLogic.estimate_oriented_normals(
            input_path, save_normals_path, normal_radius, normal_max_nn, outward=True, return_obj=True,
            orientation_mode="radial" if orientation_mode == "radial" else "tangent")
        print(f"[360 Mesh] Poisson Reconstruction (depth={depth}, width={width}, scale={scale}, linear={linear_fit}, "
              f"threads={n_threads})...")
        mesh = MS.poisson_band(pcd, scale=scale, **band) if band else MS.poisson_grid(pcd, depth=depth, scale=scale)
        if density_trim > 0.0 and len(mesh.vertices):
            print(f"[360 Mesh] Trimming low density vertices (threshold={density_trim})...")
            mesh = MS.remove_vertices_by_mask(mesh, mesh.densities < MS.quantile(mesh.densities, density_trim))
        else:
            print("[360 Mesh] Density trim is 0.0 -> Keeping watertight result.")
        if keep_components is not None:
            mesh = MS.keep_largest_components(mesh, int(keep_components))
        ProcessingLogic._write_mesh(mesh, output_path, "360 Mesh")
        if audit:
            print(f"[Mesh] audit: {MS.format_audit(MS.audit(mesh))}")
        if self_intersections:
            print(f"[Mesh] intersections: {MS.format_intersections(MS.self_intersections(mesh))}")


def batch_views() -> int:
    """Views per batched launch in batch mode: ``SLG_BATCH_VIEWS`` (1..16), default 1.  The file
    path is bound by the host PNG decode (~70 C2 views/s on 16 CPUs), not by the GPU, and a
    group waits for all its reads before its launch: over 36 C2 folders, groups of 1 / 4 / 8
    measured 0.0135-0.0149 / 0.0138-0.0144 / 0.0143-0.0163 s/view with the device taking its
    share of the PNGs, 0.0157 / 0.0161-0.0166 host-only (profiles/r5t/e2e.json).  Groups pay
    off for in-memory sources (BatchReconstructor, bench.py)."""
    try:
        return max(1, min(16, int(os.environ.get("SLG_BATCH_VIEWS", "1"))))
    except ValueError:
        return 1


def batch_reconstruct_stage(cfg, calib, row_mode, epipolar_tol, log):
    """``reconstruct`` stage of :func:`run_view_folders`: upload + fused kernels -> host cloud,
    with the reference's progress lines (processing.py:264-272).  The device tables are made
    once per geometry for the whole batch."""
    tables = {}

    def stage(folder, get_host):
        log(f"  -> Decoding folder '{os.path.basename(folder)}'  "
            f"[col-sets={cfg.n_sets_col}  row-sets={cfg.n_sets_row}]...")
        dev, _ = load_capture(folder, cfg, host=get_host())
        log("  -> Reconstructing 3D points...")
        geom = (dev.height, dev.width, torch.cuda.current_device())
        if geom not in tables:
            tables[geom] = E.DeviceCalib(calib, dev.height, dev.width)
        points, colors = reconstruct_view(dev, cfg, calib, row_mode, epipolar_tol, dc=tables[geom])
        log(f"  -> Saving {len(points)} points...")
        return points, colors
    return stage


def batch_write_stage():
    """``write`` stage of :func:`run_view_folders`: ``<folder>/<folder name>.ply``."""
    from .pipeline import FormattedCloud

    def stage(folder, result):
        name = os.path.basename(folder) + ".ply"
        if isinstance(result, FormattedCloud):          # body formatted on the device
            result.write(os.path.join(folder, name))
        else:
            ProcessingLogic._save_ply(result[0], result[1], os.path.join(folder, name))
        return name
    return stage


def reconstruct_view(dev: E.DeviceFrames, cfg: E.DecodeConfig, calib: dict, row_mode=1,
                     epipolar_tol=2.0, xyz_f64=True, dc: E.DeviceCalib | None = None):
    """Fused decode + triangulate of one in-HBM capture -> host ``(P, C)`` like the reference
    pair ``_gray_decode`` + ``_reconstruct_point_cloud``.  ``dc``: device tables of ``calib``
    already made for this geometry (else looked up in the module cache)."""
    if row_mode not in (0, 1, 2):
        return None
    eng = _engine(dev.height, dev.width)
    dc = dc if dc is not None else _device_calib(calib, dev.height, dev.width)
    out = eng.reconstruct(dev, cfg, dc, row_mode, epipolar_tol, xyz_f64=xyz_f64)
    P, C = out.result()
    return P.cpu().numpy(), C.cpu().numpy()
