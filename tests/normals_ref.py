"""NumPy restatement of the voxel down-sample, the normal estimation, the orientation and the
centroid of ``csrc/cloud_normals.hip`` (test helper, like ``cloud_ref.py``).

Open3D's ``VoxelDownSample``, ``EstimateNormals`` (``KDTreeSearchParamHybrid``) and
``OrientNormalsTowardsCameraLocation`` as published, restated; parity with an installed Open3D is
unpinned.  Each rule is one function here, as it is one ``__device__`` function in
the HIP source.  The neighbour search is brute force: every distance is computed with
``cloud_ref.d2`` and ranked by ``np.lexsort`` on (d2, index), so ties are exact.
"""
import math

import numpy as np

from cloud_ref import d2

CELL_LIMIT = 1 << 21
JACOBI_SWEEPS = 5          # kJacobiSweeps of csrc/cloud_normals.hip


# ------------------------------------------------------------------ voxel down-sample
def voxel_origin(P, voxel_size):
    return P.min(0) - voxel_size * 0.5


def voxel_coords(P, voxel_size):
    """floor((p - vmin) / voxel_size): IEEE subtraction and division."""
    return np.floor((P - voxel_origin(P, voxel_size)) / voxel_size)


def colour_mean(csum, count):
    """The exact mean of a channel, rounded half up, in integers."""
    return (2 * csum + count) // (2 * count)


def ordered_sums(P, order, start, count):
    """Per segment ``order[start[v] : start[v] + count[v]]`` the left-to-right sum of ``P``: rank
    r of every segment at once, sequential in r."""
    acc = P[order[start]].copy()
    by_count = np.argsort(-count, kind="stable")          # the segments longer than r are a prefix
    neg = -count[by_count]
    for r in range(1, int(count.max())):
        v = by_count[:np.searchsorted(neg, -r, side="left")]
        acc[v] += P[order[start[v] + r]]
    return acc


def voxel_down_sample(P, C, voxel_size):
    """``(points float64 [m, 3], colours uint8 [m, 3], first_index int64 [m], count int32 [m])``,
    voxels in ascending order of their smallest member index."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    if not (np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("voxel_size must be finite and > 0")
    if not np.isfinite(P).all():
        raise ValueError("NaN or infinite coordinate")
    ijk = voxel_coords(P, voxel_size)
    if ijk.max() >= CELL_LIMIT:
        raise ValueError("2^21 or more voxels on an axis")
    ijk = ijk.astype(np.int64)
    order = np.lexsort((np.arange(n), ijk[:, 0], ijk[:, 1], ijk[:, 2]))     # by voxel, then by index
    s = ijk[order]
    start = np.concatenate([[0], np.flatnonzero(np.any(s[1:] != s[:-1], axis=1)) + 1])
    count = np.diff(np.concatenate([start, [n]]))
    first = order[start]
    pts = ordered_sums(P, order, start, count) / count[:, None]
    csum = np.add.reduceat(np.asarray(C)[order].astype(np.int64), start, axis=0)
    col = colour_mean(csum, count[:, None]).astype(np.uint8)
    o = np.argsort(first)
    return pts[o], col[o], first[o].astype(np.int64), count[o].astype(np.int32)


def uniform_down_sample(P, C, every_k):
    if every_k < 1:
        raise ValueError("every_k must be >= 1")
    return P[::every_k], C[::every_k]


# ------------------------------------------------------------------ neighbours
def neighbour_lists(P, k, block=512, workers=1):
    """``(idx int64 [n, kk], dd float64 [n, kk])``: for every point the first ``kk = min(k, n)`` of
    all points (itself included) in ascending (d2, index) order.  Brute force, ``block`` query
    points at a time (on ``workers`` threads).  The lists for a smaller k are prefixes of these."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    kk = min(k, n)
    idx = np.empty((n, kk), np.int64)
    dd = np.empty((n, kk))

    def one(s):
        e = min(n, s + block)
        D = d2(P[s:e, None, :], P[None, :, :])
        kth = np.partition(D, kk - 1, axis=1)[:, kk - 1]
        rows, cols = np.nonzero(D <= kth[:, None])        # every candidate, ties at the cut included
        vals = D[rows, cols]
        o = np.lexsort((cols, vals, rows))
        rows, cols, vals = rows[o], cols[o], vals[o]
        first = np.searchsorted(rows, np.arange(e - s))
        take = (first[:, None] + np.arange(kk)[None, :]).reshape(-1)
        idx[s:e] = cols[take].reshape(e - s, kk)
        dd[s:e] = vals[take].reshape(e - s, kk)

    if workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(one, range(0, n, block)))
    else:
        for s0 in range(0, n, block):
            one(s0)
    return idx, dd


def neighbour_lists_tree(P, k, workers=1, spare=8, block=1 << 17):
    """:func:`neighbour_lists` for clouds too large for brute force (tools/cloud_filter_bench.py):
    ``cKDTree`` proposes ``k + spare`` candidates, every distance is recomputed with ``d2`` and the
    candidates are ranked by (d2, index).  Also returns ``resolved bool [n]``: False where a tie at
    the cut runs to the end of the candidates, so the proposal may have missed a tied point."""
    from scipy.spatial import cKDTree
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    kk, kq = min(k, n), min(k + spare, n)
    cand = cKDTree(P).query(P, k=kq, workers=workers)[1].reshape(n, kq)
    idx = np.empty((n, kk), np.int64)
    dd = np.empty((n, kk))
    resolved = np.ones(n, bool)
    for s in range(0, n, block):
        e = min(n, s + block)
        c = cand[s:e]
        D = d2(P[s:e, None, :], P[c])
        o = np.lexsort((c, D), axis=1)
        c, D = np.take_along_axis(c, o, 1), np.take_along_axis(D, o, 1)
        idx[s:e], dd[s:e] = c[:, :kk], D[:, :kk]
        if kq < n:
            resolved[s:e] = D[:, kk - 1] < D[:, kq - 1]
    return idx, dd, resolved


def hybrid_neighbours(idx, dd, radius, max_nn):
    """The hybrid search on lists from :func:`neighbour_lists`: the first ``max_nn`` entries, of
    those the ones with d2 < radius^2 (strict).  ``(idx [n, kk], inside bool [n, kk], m int32)``;
    the entries inside are a prefix of each row."""
    kk = min(max_nn, idx.shape[1])
    inside = dd[:, :kk] < radius * radius
    return idx[:, :kk], inside, inside.sum(1).astype(np.int32)


# ------------------------------------------------------------------ covariance and normal
def covariances(P, idx, inside):
    """cov float64 [n, 6] = (xx, xy, xz, yy, yz, zz): nine running sums over the neighbours in
    list order, each divided by m, then E[ab] - E[a] E[b]."""
    n = len(P)
    S = np.zeros((n, 9))
    for r in range(idx.shape[1]):
        a = inside[:, r]
        x, y, z = P[idx[a, r]].T
        for j, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            S[a, j] += v
    m = inside.sum(1)
    with np.errstate(all="ignore"):
        E = S / m[:, None].astype(np.float64)
    cov = np.stack([E[:, 3] - E[:, 0] * E[:, 0], E[:, 4] - E[:, 0] * E[:, 1], E[:, 5] - E[:, 0] * E[:, 2],
                    E[:, 6] - E[:, 1] * E[:, 1], E[:, 7] - E[:, 1] * E[:, 2], E[:, 8] - E[:, 2] * E[:, 2]], 1)
    cov[m == 0] = 0.0
    return cov


def _rotate(A, V, p, q, r):
    """One Jacobi rotation in the (p, q) plane on a batch (A: dict of the six entries by index
    pair, V: [n, 3, 3] eigenvector columns); rows with a_pq == 0 are left alone."""
    app, aqq, apq = A[p, p], A[q, q], A[min(p, q), max(p, q)]
    arp, arq = A[min(r, p), max(r, p)], A[min(r, q), max(r, q)]
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = {(p, p): app - t * apq, (q, q): aqq + t * apq, (min(p, q), max(p, q)): np.zeros_like(apq),
               (min(r, p), max(r, p)): c * arp - s * arq, (min(r, q), max(r, q)): s * arp + c * arq}
        vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
        np_, nq_ = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    for key, val in new.items():
        A[key] = np.where(on, val, A[key])
    V[:, :, p] = np.where(on[:, None], np_, vp)
    V[:, :, q] = np.where(on[:, None], nq_, vq)


def sign_rule(Nrm):
    """The first non-zero of (nz, ny, nx) is positive."""
    x, y, z = Nrm[:, 0], Nrm[:, 1], Nrm[:, 2]
    flip = np.where(z != 0.0, z < 0.0, np.where(y != 0.0, y < 0.0, x < 0.0))
    return np.where(flip[:, None], -Nrm, Nrm)


def normals_of(cov, m):
    """Unit eigenvector of the smallest eigenvalue by JACOBI_SWEEPS sweeps of cyclic Jacobi in the
    order (0,1), (0,2), (1,2); (0, 0, 1) when m < 3 or cov is identically zero."""
    n = len(cov)
    A = {(0, 0): cov[:, 0].copy(), (0, 1): cov[:, 1].copy(), (0, 2): cov[:, 2].copy(),
         (1, 1): cov[:, 3].copy(), (1, 2): cov[:, 4].copy(), (2, 2): cov[:, 5].copy()}
    V = np.tile(np.eye(3), (n, 1, 1))
    for _ in range(JACOBI_SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    vec, lam = V[:, :, 0].copy(), A[0, 0].copy()
    b = A[1, 1] < lam
    vec[b], lam[b] = V[b, :, 1], A[1, 1][b]
    b = A[2, 2] < lam
    vec[b] = V[b, :, 2]
    with np.errstate(all="ignore"):
        length = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
        out = sign_rule(vec / length[:, None])
    out[(m < 3) | ~cov.any(1)] = (0.0, 0.0, 1.0)
    return out


def estimate_normals(P, radius, max_nn, lists=None):
    """``(cov [n, 6], m int32 [n], normals [n, 3])``; ``lists``: :func:`neighbour_lists` of at
    least ``max_nn`` entries, when already computed."""
    P = np.ascontiguousarray(P, np.float64)
    idx, dd = lists if lists is not None else neighbour_lists(P, max_nn)
    idx, inside, m = hybrid_neighbours(idx, dd, radius, max_nn)
    cov = covariances(P, idx, inside)
    return cov, m, normals_of(cov, m)


def full(cov):
    """[n, 3, 3] symmetric matrices of the six entries."""
    return cov[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def rayleigh_excess(cov, Nrm):
    """``(n' cov n - l0) / l2`` per point with ``l0 <= l1 <= l2`` of ``np.linalg.eigh``: how far the
    normal is from the smallest eigenvector, as a residual (0 where l2 is 0)."""
    M = full(cov)
    lam = np.linalg.eigh(M)[0]
    q = np.einsum("ni,nij,nj->n", Nrm, M, Nrm)
    with np.errstate(all="ignore"):
        return np.where(lam[:, 2] > 0, (q - lam[:, 0]) / lam[:, 2], 0.0)


# ------------------------------------------------------------------ orientation and centroid
def orient(P, Nrm, location, outward=False):
    """Negated where normal . (location - p) < 0; ``outward`` then negates every normal."""
    ref = np.asarray(location, np.float64)[None, :] - P
    dot = (Nrm[:, 0] * ref[:, 0] + Nrm[:, 1] * ref[:, 1]) + Nrm[:, 2] * ref[:, 2]
    out = np.where((dot < 0.0)[:, None], -Nrm, Nrm)
    return -out if outward else out


def centroid(P):
    """Per-axis mean with exactly rounded sums (``math.fsum``)."""
    return np.array([math.fsum(P[:, a]) / len(P) for a in range(3)])


# ------------------------------------------------------------------ PLY with normals
def ply_bytes(P, C, Nrm=None):
    """The file ``PointCloud.save`` writes, by a pure-Python formatter."""
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if Nrm is not None else [])
    lines = ["ply", "format ascii 1.0", f"element vertex {len(P)}"] + [f"property float {p}" for p in props]
    lines += ["property uchar red", "property uchar green", "property uchar blue", "end_header"]
    for i in range(len(P)):
        row = "%.4f %.4f %.4f" % tuple(P[i])
        if Nrm is not None:
            row += " %.6f %.6f %.6f" % tuple(Nrm[i])
        lines.append(row + " %d %d %d" % (C[i][2], C[i][1], C[i][0]))
    return ("\n".join(lines) + "\n").encode()


# ------------------------------------------------------------------ the base inputs
def smoke_cloud(row_mode):
    """The smoke view as ``test_gpu_cloud_filter.py`` builds it: 12,532 points in row_mode 1,
    25,064 in row_mode 2."""
    from test_gpu_cloud_filter import oracle_cloud
    (P, C), _ = oracle_cloud((192, 128), 25.0, 1, row_mode)
    return P, C
