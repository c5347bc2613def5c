"""NumPy restatement of the seeded RANSAC plane segmentation of ``csrc/cloud_plane.hip`` (test
helper, like ``feature_ref.py`` and ``icp_ref.py``).

Open3D's ``PointCloud::SegmentPlane`` as published, restated; parity with an installed Open3D is
unpinned and the places where the rule is ours are listed in DESIGN.md §14.  Each rule is one
function here, as it is one ``__device__`` function in the HIP source.  NumPy does not fuse
multiplies and adds and the device builds with ``-ffp-contract=off``, so every rule is the same
sequence of IEEE operations on both sides; ``sqrt`` and the division are correctly rounded on both.
"""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from feature_ref import MASK, draw_rule, draw_table  # noqa: F401  (MASK: the tests' 64-bit seeds)

CHUNK = 2048                        # kChunk of csrc/cloud_grid.h: the order of err
BATCH = 256                         # cloud.PLANE_BATCH
RECORD_STRIDE, SUMS_LEN = 16, 16    # SLG_PLANE_RECORD_STRIDE, SLG_PLANE_SUMS_LEN
MIN_N, MAX_N = 3, 8
PROBABILITY = 0.99999999


# ------------------------------------------------------------------ draws
def plane_draw_rule(seed, t, k, n):
    """Draw ``k`` of trial ``t`` on Python integers: an index below ``n`` (a trial reserves
    ``MAX_N`` draws)."""
    return draw_rule(seed, t, k, n, MAX_N)


def draws(seed, t0, count, ransac_n, n):
    """int64 [count, ransac_n]: :func:`plane_draw_rule` for the trials ``t0 .. t0 + count - 1``."""
    return draw_table(seed, t0, count, ransac_n, n, MAX_N)


def distinct(c):
    """Rows of ``c`` whose draws are pairwise different."""
    s = np.sort(c, axis=1)
    return (s[:, 1:] != s[:, :-1]).all(axis=1)


# ------------------------------------------------------------------ models
def normalise(abc, at):
    """``(plane [m, 4], valid [m])``: abc / norm and d from the point ``at``; the zero plane where
    the norm is zero."""
    x, y, z = abc[:, 0], abc[:, 1], abc[:, 2]
    norm = np.sqrt((x * x + y * y) + z * z)
    ok = ~(norm == 0.0)
    with np.errstate(all="ignore"):
        u = abc / norm[:, None]
        d = -((u[:, 0] * at[:, 0] + u[:, 1] * at[:, 1]) + u[:, 2] * at[:, 2])
    pl = np.concatenate([u, d[:, None]], 1)
    pl[~ok] = 0.0
    return pl, ok


def triangle_plane(T):
    """``ComputeTrianglePlane`` for triples ``T`` ``[m, 3, 3]``."""
    e0, e1 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    abc = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                    e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], 1)
    return normalise(abc, T[:, 0])


def plane_from_sums(cen, S):
    """``GetPlaneFromPoints`` from centroids ``[m, 3]`` and centred sums ``[m, 6]`` = xx xy xz yy yz zz."""
    xx, xy, xz, yy, yz, zz = (S[:, k] for k in range(6))
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    ax = np.stack([det_x, xz * yz - xy * zz, xy * yz - xz * yy], 1)
    ay = np.stack([xz * yz - xy * zz, det_y, xy * xz - yz * xx], 1)
    az = np.stack([xy * yz - xz * yy, xy * xz - yz * xx, det_z], 1)
    use_x = (det_x > det_y) & (det_x > det_z)
    use_y = ~use_x & (det_y > det_z)
    abc = np.where(use_x[:, None], ax, np.where(use_y[:, None], ay, az))
    return normalise(abc, cen)


def centred_sums(Q):
    """``(centroid [m, 3], sums [m, 6])`` of point sets ``Q`` ``[m, k, 3]``, both in draw order."""
    k = Q.shape[1]
    cen = np.zeros((len(Q), 3))
    for j in range(k):
        cen = cen + Q[:, j]
    cen = cen / float(k)
    S = np.zeros((len(Q), 6))
    for j in range(k):
        r = Q[:, j] - cen
        S = S + np.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 0] * r[:, 2], r[:, 1] * r[:, 1], r[:, 1] * r[:, 2],
                          r[:, 2] * r[:, 2]], 1)
    return cen, S


def plane_from_points(Q):
    return plane_from_sums(*centred_sums(Q))


def trials(P, seed, t0, count, ransac_n):
    """``(draws [count, ransac_n], planes [count, 4], valid [count])``.  A trial with two equal
    draws or a zero norm is invalid and has the zero plane."""
    c = draws(seed, t0, count, ransac_n, len(P))
    Q = P[c]
    pl, ok = triangle_plane(Q) if ransac_n == 3 else plane_from_points(Q)
    ok = ok & distinct(c)
    pl[~ok] = 0.0
    return c, pl, ok


# ------------------------------------------------------------------ evaluation
def distances(P, pl):
    return np.abs(((pl[0] * P[:, 0] + pl[1] * P[:, 1]) + pl[2] * P[:, 2]) + pl[3])


def chunked_sum(terms):
    """Left to right within each chunk of CHUNK consecutive terms, then the chunks left to right."""
    n = len(terms)
    nb = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(nb * CHUNK)
    pad[:n] = terms
    part = np.add.accumulate(pad.reshape(nb, CHUNK), axis=1)[:, -1]
    return float(np.add.accumulate(part)[-1])


def evaluate(P, pl, thr):
    """``(count, err, fitness, rmse)`` of ``EvaluateRANSACBasedOnDistance`` (err: the distances, in
    the chunked order)."""
    dist = distances(P, pl)
    inl = dist < thr
    count = int(inl.sum())
    err = chunked_sum(np.where(inl, dist, 0.0))
    return count, err, count / float(len(P)), (err / math.sqrt(float(count)) if count else 0.0)


def records(P, seed, t0, count, ransac_n, thr, workers=1):
    """float64 [count, RECORD_STRIDE] as ``slg_plane_batch`` lays the records out: trial, valid,
    a b c d, count, err, fitness, rmse, 6 unused."""
    _, pl, ok = trials(P, seed, t0, count, ransac_n)
    R = np.zeros((count, RECORD_STRIDE))
    R[:, 0] = np.arange(t0, t0 + count)
    R[:, 1] = ok
    R[:, 2:6] = pl

    def one(g):
        if ok[g]:
            R[g, 6:10] = evaluate(P, pl[g], thr)
    if workers > 1:
        with ThreadPoolExecutor(workers) as ex:
            list(ex.map(one, range(count)))
    else:
        for g in range(count):
            one(g)
    return R


# ------------------------------------------------------------------ the choice
def max_trials(probability, fitness, ransac_n):
    """ceil(log(1 - probability) / log(1 - fitness^ransac_n)), the power by repeated multiplication;
    None where that bounds nothing."""
    p = fitness
    for _ in range(ransac_n - 1):
        p = p * fitness
    den = math.log(1.0 - p)
    if not den < 0.0 or probability >= 1.0:
        return None
    return int(math.ceil(math.log(1.0 - probability) / den))


def scan(recs, num_iterations, probability, ransac_n):
    """The sequential choice over records in ascending trial order: ``(position of the winner in
    recs or -1, final K)``."""
    K, best = int(num_iterations), -1
    for pos, r in enumerate(recs):
        t = int(r[0])
        if t >= K:
            break
        if r[1] == 0.0:
            continue
        f, rmse = float(r[8]), float(r[9])
        if best < 0 or f > recs[best][8] or (f == recs[best][8] and rmse < recs[best][9]):
            best = pos
            if f >= 1.0:
                K = min(K, t + 1)
            elif f > 0.0:
                k = max_trials(probability, f, ransac_n)
                if k is not None:
                    K = min(K, max(t + 1, k))
    return best, K


# ------------------------------------------------------------------ final inliers and the refit
def inliers(P, pl, thr):
    return np.flatnonzero(distances(P, pl) < thr)


def refit_terms(P, idx):
    """The nine refit sums' terms ``[m, 9]`` (x y z, then the centred products about the fsum
    centroid) for an exact reference."""
    Q = P[idx]
    cen = np.array([math.fsum(Q[:, a]) for a in range(3)]) / float(len(Q))
    return np.concatenate([Q, centred_terms(Q, cen)], 1)


def centred_terms(Q, cen):
    r = Q - cen
    return np.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 0] * r[:, 2], r[:, 1] * r[:, 1], r[:, 1] * r[:, 2],
                     r[:, 2] * r[:, 2]], 1)


def plane_from_nine(sums, m):
    """The returned plane from the nine sums (x y z, xx xy xz yy yz zz) and the inlier count."""
    s = np.asarray(sums, np.float64)
    cen = (s[:3] / float(m))[None, :] if m else np.zeros((1, 3))
    pl, _ = plane_from_sums(cen, s[None, 3:9])
    return pl[0]


def segment(P, thr, ransac_n=3, num_iterations=100, probability=PROBABILITY, seed=0, batch=BATCH, workers=1):
    """The whole segmentation: ``dict(plane (the winner's own), trial, K, records, inliers, fitness,
    rmse)``; the refitted plane is :func:`plane_from_nine` of sums taken over ``inliers``."""
    recs, K, best, t0 = [], int(num_iterations), -1, 0
    while t0 < K:
        count = min(batch, K - t0)
        recs.extend(records(P, seed, t0, count, ransac_n, thr, workers))
        best, K = scan(recs, num_iterations, probability, ransac_n)
        t0 += count
    recs = [r for r in recs if r[0] < K]
    if best < 0:
        return dict(plane=np.zeros(4), trial=-1, K=K, records=recs, inliers=np.zeros(0, np.int64), fitness=0.0, rmse=0.0)
    w = recs[best]
    return dict(plane=w[2:6].copy(), trial=int(w[0]), K=K, records=recs, inliers=inliers(P, w[2:6], thr),
                fitness=float(w[8]), rmse=float(w[9]))


# ------------------------------------------------------------------ the base case
WALL_NORMAL = (0.28, -0.16, 0.9466)     # normalised below: a wall tilted against every axis
WALL_BEHIND = 400.0                     # the wall's centre lies this far behind the cloud's centroid, along the normal
WALL_GRID = (125, 100)                  # 12,500 wall points
WALL_PITCH = 2.0
WALL_JITTER = 0.75                      # the offsets along the normal are uniform in [-WALL_JITTER, WALL_JITTER]
BASE_THRESHOLD = 1.5
BASE_ITERATIONS = 1000


def plant_wall(P, seed=20260814, behind=WALL_BEHIND, grid=WALL_GRID, pitch=WALL_PITCH, jitter=WALL_JITTER):
    """``(points with the wall appended, wall mask)``: a ``grid`` of pitch ``pitch`` on the plane
    through ``centroid + behind * normal``, each point moved along the normal by a fixed-seed
    offset below ``jitter``."""
    nrm = np.array(WALL_NORMAL)
    nrm = nrm / np.sqrt(nrm @ nrm)
    u = np.cross(nrm, [0.0, 1.0, 0.0])
    u = u / np.sqrt(u @ u)
    v = np.cross(nrm, u)
    c = P.mean(0) + behind * nrm
    gu, gv = np.meshgrid((np.arange(grid[0]) - (grid[0] - 1) / 2.0) * pitch,
                         (np.arange(grid[1]) - (grid[1] - 1) / 2.0) * pitch, indexing="ij")
    off = np.random.default_rng(seed).uniform(-jitter, jitter, gu.size)
    W = c + gu.reshape(-1, 1) * u + gv.reshape(-1, 1) * v + off[:, None] * nrm
    out = np.ascontiguousarray(np.concatenate([P, W]))
    wall = np.zeros(len(out), bool)
    wall[len(P):] = True
    return out, wall


@functools.lru_cache(maxsize=1)
def base_case():
    """The row_mode 1 smoke cloud (12,532 points) plus the planted wall behind it:
    ``dict(P, C, wall, thr, num_iterations)``."""
    import normals_ref as NR
    P, C = NR.smoke_cloud(1)
    P, wall = plant_wall(np.ascontiguousarray(P, np.float64))
    C = np.ascontiguousarray(np.concatenate([np.asarray(C, np.uint8), np.full((int(wall.sum()), 3), 200, np.uint8)]))
    for a in (P, C, wall):
        a.setflags(write=False)
    return dict(P=P, C=C, wall=wall, thr=BASE_THRESHOLD, num_iterations=BASE_ITERATIONS)


@functools.lru_cache(maxsize=4)
def base_segment(seed=0):
    b = base_case()
    return segment(b["P"], b["thr"], 3, b["num_iterations"], seed=seed)
