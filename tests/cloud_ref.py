"""NumPy restatement of the two cloud filters (test helper, like ``png_ref.py``).

Open3D's ``RemoveRadiusOutliers`` / ``RemoveStatisticalOutliers`` as published, restated; parity
with an installed Open3D is unpinned.  Each rule is one function here, as it is one
``__device__`` function in ``csrc/cloud_grid.h`` or ``csrc/cloud_filter.hip``.  ``cKDTree`` only
proposes candidates (a slightly larger radius, ``k + 8`` neighbours); every distance is then recomputed with :func:`d2`.
"""
import math

import numpy as np
from scipy.spatial import cKDTree


def d2(a, b):
    """Squared distance, fp64, in this order (no FMA in NumPy; the device builds with
    -ffp-contract=off)."""
    dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def radius_neighbour(dd, radius):
    return dd < radius * radius


def radius_keep(counts, nb_points):
    return counts > nb_points


def avg_of(dd_sorted, kk):
    """Mean of sqrt over ascending d2, summed left to right (np.add.accumulate is sequential)."""
    return np.add.accumulate(np.sqrt(dd_sorted), axis=-1)[..., -1] / kk


def stat_threshold(avg, std_ratio):
    """(mean, std, thr) with exactly rounded sums (``math.fsum``)."""
    n = len(avg)
    pos = avg[avg > 0]
    mean = math.fsum(pos) / n
    with np.errstate(all="ignore"):
        std = float(np.sqrt(np.float64(math.fsum((pos - mean) ** 2)) / np.float64(n - 1)))
    return mean, std, mean + std_ratio * std


def stat_keep(avg, thr):
    return (avg > 0) & (avg < thr)


# ------------------------------------------------------------------ the filters
def radius_counts(P, radius, workers=1):
    P = np.ascontiguousarray(P, np.float64)
    tree = cKDTree(P)
    hi = tree.query_ball_point(P, radius * (1 + 1e-9), workers=workers, return_length=True)
    lo = tree.query_ball_point(P, radius * (1 - 1e-9), workers=workers, return_length=True)
    counts = np.asarray(lo, np.int32).copy()  # nothing between the two radii: the tree's count is exact
    for i in np.flatnonzero(np.asarray(hi) != np.asarray(lo)):
        nb = np.asarray(tree.query_ball_point(P[i], radius * (1 + 1e-9)), np.int64)
        counts[i] = np.count_nonzero(radius_neighbour(d2(P[i], P[nb]), radius))
    return counts


def radius_filter(P, nb_points, radius, workers=1):
    counts = radius_counts(P, radius, workers)
    return radius_keep(counts, nb_points), counts


def knn_avg(P, k, workers=1):
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    kk = min(k, n)
    kq = min(k + 8, n)
    _, idx = cKDTree(P).query(P, k=kq, workers=workers)
    idx = idx.reshape(n, kq)
    # the tree ranks by its own distances; 8 spare candidates cover any rank its rounding swaps
    avg = np.empty(n)
    for s in range(0, n, 1 << 17):            # in blocks: P[idx] of a whole 1080p cloud is ~1 GB
        e = min(n, s + (1 << 17))
        dd = np.sort(d2(P[s:e, None, :], P[idx[s:e]]), axis=1)
        avg[s:e] = avg_of(dd[:, :kk], kk)
    return avg


def statistical_filter(P, k, std_ratio, workers=1):
    avg = knn_avg(P, k, workers)
    mean, std, thr = stat_threshold(avg, std_ratio)
    return stat_keep(avg, thr), avg, (mean, std, thr)


# ------------------------------------------------------------------ plain O(N^2) evaluation
def brute_radius_counts(P, radius):
    P = np.asarray(P, np.float64)
    return np.array([np.count_nonzero(radius_neighbour(d2(p, P), radius)) for p in P], np.int32)


def brute_knn_avg(P, k):
    P = np.asarray(P, np.float64)
    kk = min(k, len(P))
    return np.array([avg_of(np.sort(d2(p, P))[:kk], kk) for p in P])
