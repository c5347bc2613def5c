"""NumPy restatement of the FPFH features, the feature matching and the seeded RANSAC global
registration of ``csrc/cloud_feature.hip`` and ``csrc/cloud_ransac.hip`` (test helper, like
``normals_ref.py`` and ``icp_ref.py``).

Open3D's ``ComputePairFeatures``, ``ComputeSPFHFeature``, ``ComputeFPFHFeature`` and
``RegistrationRANSACBasedOnFeatureMatching`` as published, restated; parity with an installed
Open3D is unpinned and the places where the rule is ours are listed in DESIGN.md §13.  Each rule is
one function here, as it is one ``__device__`` function in the HIP sources.  NumPy does not fuse
multiplies and adds and the device builds with ``-ffp-contract=off``, so everything but ``atan2``
is the same sequence of IEEE operations on both sides; :func:`near_edge` marks the pairs
whose bin an ``atan2`` that differs in the last place could change.
"""
import functools
import math

import numpy as np

import icp_ref as IR
import normals_ref as NR

DIM, BINS = 33, 11                  # SLG_FPFH_DIM
HORN_SWEEPS = 6                     # kHornSweeps of csrc/cloud_ransac.hip
BATCH = 4096                        # cloud.RANSAC_BATCH
TRIAL_STRIDE, RECORD_STRIDE = 20, 32
EDGE_OK, DISTANCE_OK = 1, 2
MASK = (1 << 64) - 1


def dot3(a, b):
    """Summed x, y, z left to right."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


# ------------------------------------------------------------------ FPFH
def pair_features(p1, n1, p2, n2):
    """``(theta, alpha, phi)`` of Open3D's pair feature for rows of points and normals.  Ours: the
    roles swap when ``|a1| < |a2|`` (Open3D compares the ``acos`` of the two).  A zero distance,
    or a zero ``|dp x n1|`` after the swap, gives the all-zero triple."""
    dp = p2 - p1
    with np.errstate(all="ignore"):
        dist = np.sqrt(dot3(dp, dp))
        a1, a2 = dot3(n1, dp) / dist, dot3(n2, dp) / dist
        swap = np.abs(a1) < np.abs(a2)
        na, nb = np.where(swap[:, None], n2, n1), np.where(swap[:, None], n1, n2)
        dp = np.where(swap[:, None], -dp, dp)
        phi = np.where(swap, -a2, a1)
        v = cross3(dp, na)
        vn = np.sqrt(dot3(v, v))
        v = v / vn[:, None]
        w = cross3(na, v)
        alpha = dot3(v, nb)
        theta = np.arctan2(dot3(w, nb), dot3(na, nb))
    zero = (dist == 0.0) | (vn == 0.0)
    return np.where(zero, 0.0, theta), np.where(zero, 0.0, alpha), np.where(zero, 0.0, phi)


def bin_coords(theta, alpha, phi):
    """The three coordinates in [0, 11] whose floors are the bins."""
    return 11.0 * (theta + math.pi) / (2.0 * math.pi), 11.0 * (alpha + 1.0) * 0.5, 11.0 * (phi + 1.0) * 0.5


def bin_of(c):
    return np.clip(np.floor(c), 0, BINS - 1).astype(np.int64)


def near_edge(c, eps=1e-9):
    """A coordinate within ``eps`` of an interior integer (1..10)."""
    k = np.rint(c)
    return (np.abs(c - k) < eps) & (k >= 1) & (k <= BINS - 1)


def spfh_increment(m):
    return 100.0 / (m - 1).astype(np.float64)


def spfh_of(P, Nrm, idx, inside, m):
    """``(spfh float64 [n, 33], edge_pairs)``: per point, over its list in order and leaving itself
    out by index, each pair adds 100 / (m - 1) to one bin per third."""
    n = len(P)
    S = np.zeros((n, DIM))
    rows = np.arange(n)
    edge = 0
    with np.errstate(all="ignore"):
        inc = spfh_increment(m)
    for r in range(idx.shape[1]):
        a = inside[:, r] & (idx[:, r] != rows) & (m > 1)
        i, j = rows[a], idx[a, r]
        cs = bin_coords(*pair_features(P[i], Nrm[i], P[j], Nrm[j]))
        edge += int((near_edge(cs[0]) | near_edge(cs[1]) | near_edge(cs[2])).sum())
        for third, c in enumerate(cs):
            S[i, third * BINS + bin_of(c)] += inc[i]
    return S, edge


def fpfh_of(S, idx, dd, inside, m):
    """Over the same list in order, skipping d2 == 0: spfh[neighbour] / d2 into the feature and
    into its third's sum (bin by bin); each third scaled by 100 / sum where the sum is not zero;
    plus the point's own SPFH."""
    n = len(S)
    F = np.zeros((n, DIM))
    sums = np.zeros((n, 3))
    for r in range(idx.shape[1]):
        a = inside[:, r] & (dd[:, r] != 0.0) & (m > 1)
        val = S[idx[a, r]] / dd[a, r][:, None]
        F[a] += val
        for j in range(DIM):
            sums[a, j // BINS] += val[:, j]
    with np.errstate(all="ignore"):
        scale = np.where(sums != 0.0, 100.0 / sums, 1.0)
    return F * np.repeat(scale, BINS, axis=1) + S


def compute_fpfh(P, Nrm, radius, max_nn, lists=None, workers=8):
    """``dict(spfh, fpfh, m, edge_pairs, idx, dd, inside)``; ``lists``: ``normals_ref.neighbour_lists``
    of at least ``max_nn`` entries, when already computed."""
    P, Nrm = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Nrm, np.float64)
    idx, dd = lists if lists is not None else NR.neighbour_lists(P, max_nn, workers=workers)
    idx, inside, m = NR.hybrid_neighbours(idx, dd, radius, max_nn)
    dd = dd[:, :idx.shape[1]]
    S, edge = spfh_of(P, Nrm, idx, inside, m)
    return dict(spfh=S, fpfh=fpfh_of(S, idx, dd, inside, m), m=m, edge_pairs=edge, idx=idx, dd=dd, inside=inside)


def compute_fpfh_loop(P, Nrm, radius, max_nn):
    """The same rules as a plain loop over the points (small clouds): ``(spfh, fpfh)``."""
    n = len(P)
    idx, dd = NR.neighbour_lists(P, max_nn)
    S = np.zeros((n, DIM))
    lists = []
    for i in range(n):
        lst = [(int(idx[i, r]), float(dd[i, r])) for r in range(idx.shape[1]) if dd[i, r] < radius * radius]
        lists.append(lst)
        m = len(lst)
        if m <= 1:
            continue
        inc = 100.0 / float(m - 1)
        for j, _ in lst:
            if j == i:
                continue
            cs = bin_coords(*pair_features(P[i:i + 1], Nrm[i:i + 1], P[j:j + 1], Nrm[j:j + 1]))
            for third, c in enumerate(cs):
                S[i, third * BINS + int(bin_of(c)[0])] += inc
    F = np.zeros((n, DIM))
    for i in range(n):
        lst = lists[i]
        if len(lst) <= 1:
            continue
        f, sums = [0.0] * DIM, [0.0, 0.0, 0.0]
        for j, d in lst:
            if d == 0.0:
                continue
            for b in range(DIM):
                val = float(np.float64(S[j, b]) / np.float64(d))
                f[b] += val
                sums[b // BINS] += val
        for b in range(DIM):
            s = sums[b // BINS]
            F[i, b] = (f[b] * float(np.float64(100.0) / np.float64(s)) if s != 0.0 else f[b]) + S[i, b]
    return S, F


# ------------------------------------------------------------------ matching
def feature_d2(a, B):
    """Squared feature distance of row(s) ``a`` to the rows of ``B``, summed j = 0..32 left to right."""
    d = np.zeros(np.broadcast_shapes(a.shape[:-1], B.shape[:-1]))
    for j in range(a.shape[-1]):
        x = a[..., j] - B[..., j]
        d = d + x * x
    return d


def nearest_rows_brute(A, B):
    """Per row of ``A`` the row of ``B`` with the smallest (d2, index): every distance by the rule."""
    out = np.empty(len(A), np.int32)
    for i in range(len(A)):
        D = feature_d2(A[i], B)
        out[i] = int(np.lexsort((np.arange(len(B)), D))[0])
    return out


def nearest_rows(A, B, block=2048):
    """:func:`nearest_rows_brute` at size: a matrix product proposes every row whose approximate
    distance is within a relative 1e-7 of the row's smallest, the rule then ranks the proposals by
    (d2, index).  (The product's error is some 1e-13 of |a|^2 + |b|^2.)"""
    A, B = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(B, np.float64)
    out = np.empty(len(A), np.int32)
    b2 = (B * B).sum(1)
    for s in range(0, len(A), block):
        a = A[s:s + block]
        a2 = (a * a).sum(1)
        D = a2[:, None] + b2[None, :] - 2.0 * (a @ B.T)
        cut = D.min(1) + 1e-7 * (a2 + b2.max()) + 1e-300
        rows, cols = np.nonzero(D <= cut[:, None])
        exact = feature_d2(a[rows], B[cols])
        o = np.lexsort((cols, exact, rows))
        rows, cols = rows[o], cols[o]
        first = np.searchsorted(rows, np.arange(len(a)))
        out[s:s + block] = cols[first]
    return out


def correspondences(A, B, mutual_filter=False, nn=None):
    """int64 [m, 2]: (i, nearest row of B to A[i]) in source order; with ``mutual_filter`` only
    where the reverse search from that row returns i.  ``nn``: ``(nn_source, nn_target)`` when
    already computed."""
    nn_s = nn[0] if nn is not None else nearest_rows(A, B)
    i = np.arange(len(nn_s), dtype=np.int64)
    if mutual_filter:
        nn_t = nn[1] if nn is not None else nearest_rows(B, A)
        i = i[nn_t[nn_s] == i]
    return np.stack([i, nn_s[i].astype(np.int64)], 1)


# ------------------------------------------------------------------ RANSAC: draws and checkers
def mix64(z):
    """The finaliser of SplitMix64 (Stafford's mix 13) on Python integers."""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw_rule(seed, t, k, m, stride):
    """Draw ``k`` of trial ``t``, with ``stride`` draws reserved per trial (``draw_rule<kStride>`` of
    ``csrc/cloud_grid.h``): an index below ``m`` from the upper 32 bits by a multiply-high."""
    h = mix64(mix64(seed + 0x9E3779B97F4A7C15) + (t * stride + k))
    return ((h >> 32) * m) >> 32


def draw_table(seed, t0, count, width, m, stride):
    """int64 [count, width]: :func:`draw_rule` for the draws ``0 .. width - 1`` of the trials
    ``t0 .. t0 + count - 1``, on uint64 arrays."""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        base = np.uint64(mix64(seed + 0x9E3779B97F4A7C15))
        tk = (np.arange(t0, t0 + count, dtype=np.uint64)[:, None] * np.uint64(stride)
              + np.arange(width, dtype=np.uint64)[None, :])
        h = mix(base + tk)
        return (((h >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


DRAW_STRIDE = 4                     # kDrawStride of csrc/cloud_ransac.hip


def draw(seed, t, k, m):
    """The registration RANSAC's draw ``k`` of trial ``t``."""
    return draw_rule(seed, t, k, m, DRAW_STRIDE)


def draws(seed, t0, count, m):
    """int64 [count, 3]: :func:`draw` for the trials ``t0 .. t0 + count - 1``."""
    return draw_table(seed, t0, count, 3, m, DRAW_STRIDE)


def edge_ok(S, D, e):
    """The edge-length checker on squares for triples ``S``, ``D`` ``[n, 3, 3]`` (ours: Open3D
    compares lengths): every pair of the three has ds2 >= dt2 * e^2 and dt2 >= ds2 * e^2."""
    ok = np.ones(len(S), bool)
    e2 = e * e
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ds2, dt2 = IR.d2(S[:, b], S[:, a]), IR.d2(D[:, b], D[:, a])
        ok &= (ds2 >= dt2 * e2) & (dt2 >= ds2 * e2)
    return ok


# ------------------------------------------------------------------ RANSAC: the estimate
def _rotate4(A, V, p, q):
    apq = A[:, p, q].copy()
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = {(p, p): A[:, p, p] - t * apq, (q, q): A[:, q, q] + t * apq, (p, q): np.zeros_like(apq)}
        for r in range(4):
            if r not in (p, q):
                arp, arq = A[:, r, p], A[:, r, q]
                new[(r, p)], new[(r, q)] = c * arp - s * arq, s * arp + c * arq
        vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
        nvp, nvq = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    for (a, b), val in new.items():
        A[:, a, b] = A[:, b, a] = np.where(on, val, A[:, a, b])
    V[:, :, p] = np.where(on[:, None], nvp, vp)
    V[:, :, q] = np.where(on[:, None], nvq, vq)


def estimate(S, D, sweeps=HORN_SWEEPS):
    """The rigid least-squares transform of triples ``S -> D`` ``[n, 3, 3]`` by Horn's quaternion
    (``estimate_rule``): float64 ``[n, 4, 4]``."""
    n = len(S)
    cs = ((S[:, 0] + S[:, 1]) + S[:, 2]) / 3.0
    ct = ((D[:, 0] + D[:, 1]) + D[:, 2]) / 3.0
    a, b = S - cs[:, None, :], D - ct[:, None, :]
    M = np.empty((n, 3, 3))
    for i in range(3):
        for j in range(3):
            M[:, i, j] = (a[:, 0, i] * b[:, 0, j] + a[:, 1, i] * b[:, 1, j]) + a[:, 2, i] * b[:, 2, j]
    A = np.empty((n, 4, 4))
    A[:, 0, 0] = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    A[:, 1, 1] = (M[:, 0, 0] - M[:, 1, 1]) - M[:, 2, 2]
    A[:, 2, 2] = (M[:, 1, 1] - M[:, 0, 0]) - M[:, 2, 2]
    A[:, 3, 3] = (M[:, 2, 2] - M[:, 0, 0]) - M[:, 1, 1]
    A[:, 0, 1] = A[:, 1, 0] = M[:, 1, 2] - M[:, 2, 1]
    A[:, 0, 2] = A[:, 2, 0] = M[:, 2, 0] - M[:, 0, 2]
    A[:, 0, 3] = A[:, 3, 0] = M[:, 0, 1] - M[:, 1, 0]
    A[:, 1, 2] = A[:, 2, 1] = M[:, 0, 1] + M[:, 1, 0]
    A[:, 1, 3] = A[:, 3, 1] = M[:, 2, 0] + M[:, 0, 2]
    A[:, 2, 3] = A[:, 3, 2] = M[:, 1, 2] + M[:, 2, 1]
    V = np.tile(np.eye(4), (n, 1, 1))
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate4(A, V, p, q)
    lam, vec = A[:, 0, 0].copy(), V[:, :, 0].copy()
    for k in (1, 2, 3):
        better = A[:, k, k] > lam
        lam = np.where(better, A[:, k, k], lam)
        vec = np.where(better[:, None], V[:, :, k], vec)
    w, x, y, z = vec[:, 0], vec[:, 1], vec[:, 2], vec[:, 3]
    length = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / length, x / length, y / length, z / length
    T = np.zeros((n, 4, 4))
    T[:, 3, 3] = 1.0
    T[:, 0, 0], T[:, 0, 1], T[:, 0, 2] = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)
    T[:, 1, 0], T[:, 1, 1], T[:, 1, 2] = 2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)
    T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] = 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)
    for r in range(3):
        T[:, r, 3] = ct[:, r] - ((T[:, r, 0] * cs[:, 0] + T[:, r, 1] * cs[:, 1]) + T[:, r, 2] * cs[:, 2])
    return T


def kabsch_svd(S, D):
    """The same transform of one triple by the SVD (``np.linalg.svd``), for comparison."""
    cs, ct = S.mean(0), D.mean(0)
    U, _, Vt = np.linalg.svd((D - ct).T @ (S - cs))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, ct - R @ cs
    return T


def pair_d2(T, s, d):
    """d2(T s - t) for rows of pairs; ``T`` one 4x4 or ``[n, 4, 4]``."""
    T = np.asarray(T)
    q = [((T[..., r, 0] * s[:, 0] + T[..., r, 1] * s[:, 1]) + T[..., r, 2] * s[:, 2]) + T[..., r, 3] for r in range(3)]
    dx, dy, dz = q[0] - d[:, 0], q[1] - d[:, 1], q[2] - d[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def trials(src, tgt, C, seed, t0, count, edge_length, dist, sweeps=HORN_SWEEPS):
    """``(picks int64 [count, 3], flags int64 [count], T [count, 4, 4])`` of the trials
    ``t0 .. t0 + count - 1``: the three draws (which must be distinct: ours), EDGE_OK, the estimate
    (the identity where the edge checker failed) and DISTANCE_OK (all three pairs have
    d2(T s - t) <= dist^2)."""
    picks = draws(seed, t0, count, len(C))
    S, D = src[C[picks, 0]], tgt[C[picks, 1]]
    distinct = (picks[:, 0] != picks[:, 1]) & (picks[:, 0] != picks[:, 2]) & (picks[:, 1] != picks[:, 2])
    edge = distinct & edge_ok(S, D, edge_length)
    T = np.tile(np.eye(4), (count, 1, 1))
    T[edge] = estimate(S[edge], D[edge], sweeps)
    near = edge.copy()
    for k in range(3):
        near &= pair_d2(T, S[:, k], D[:, k]) <= dist * dist
    return picks, edge * EDGE_OK + near * DISTANCE_OK, T


def inlier_count(src, tgt, C, T, dist):
    """Pairs of ``C`` with d2(T s - t) < dist^2 (strict)."""
    return int((pair_d2(T, src[C[:, 0]], tgt[C[:, 1]]) < dist * dist).sum())


# ------------------------------------------------------------------ RANSAC: the choice
def max_trials(confidence, ratio):
    """ceil(log(1 - confidence) / log(1 - ratio^3)), or None where that bounds nothing."""
    if ratio >= 1.0:
        return 0
    den = math.log(1.0 - (ratio * ratio) * ratio)
    if not den < 0.0:
        return None
    if confidence >= 1.0:
        return None
    return int(math.ceil(math.log(1.0 - confidence) / den))


def scan(records, n_pairs, max_iteration, confidence):
    """The sequential choice over evaluation records in ascending trial order, each ``(t, fitness,
    rmse, inliers)``: ``(position of the winner in records or -1, final K)``.  A record replaces
    the best when its fitness is larger, or equal with a smaller rmse; on a replacement with
    r = inliers / n_pairs > 0, K = min(K, max(t + 1, max_trials(confidence, r))).  Records at or
    past K are ignored."""
    K, best, best_fit, best_rmse = int(max_iteration), -1, 0.0, 0.0
    for pos, (t, fitness, rmse, inliers) in enumerate(records):
        if t >= K:
            break
        if best < 0 or fitness > best_fit or (fitness == best_fit and rmse < best_rmse):
            best, best_fit, best_rmse = pos, fitness, rmse
            r = inliers / n_pairs
            if r > 0.0:
                k = max_trials(confidence, r)
                if k is not None:
                    K = min(K, max(int(t) + 1, k))
    return best, K


def ransac(src, tgt, C, dist, edge_length=0.9, max_iteration=100000, confidence=0.999, seed=0, batch=BATCH,
           workers=1):
    """The whole registration: ``dict(T, fitness, rmse, trial, K, records)`` with one record per
    evaluated trial (``dict(t, picks, T, n_corr, err2, fitness, rmse, inliers)``)."""
    from scipy.spatial import cKDTree
    tree = cKDTree(tgt)
    records, K, best, t0 = [], int(max_iteration), -1, 0
    while t0 < K:
        count = min(batch, max_iteration - t0)
        picks, flags, T = trials(src, tgt, C, seed, t0, count, edge_length, dist)
        for g in np.flatnonzero(flags & DISTANCE_OK):           # one at a time: K may shrink after any of them
            if t0 + int(g) >= K:
                break
            ev = IR.evaluate(src, tgt, T[g], dist, tree, workers)
            records.append(dict(t=t0 + int(g), picks=picks[g], T=T[g], n_corr=ev["n_corr"], err2=ev["err2"],
                                fitness=ev["fitness"], rmse=ev["rmse"], inliers=inlier_count(src, tgt, C, T[g], dist)))
            best, K = scan([(r["t"], r["fitness"], r["rmse"], r["inliers"]) for r in records], len(C), max_iteration,
                           confidence)
        t0 += count
    records = [r for r in records if r["t"] < K]
    if best < 0:
        return dict(T=np.eye(4), fitness=0.0, rmse=0.0, trial=-1, K=K, records=records)
    w = records[best]
    return dict(T=w["T"], fitness=w["fitness"], rmse=w["rmse"], trial=w["t"], K=K, records=records)


# ------------------------------------------------------------------ the base case
BASE_ANGLES_DEG = (25.0, -10.0, 15.0)
BASE_TRANSLATION = (30.0, -20.0, 12.0)
BASE_DIST = 6.0
BASE_RADIUS, BASE_MAX_NN = 22.5, 100
NORMAL_RADIUS, NORMAL_MAX_NN = 9.0, 30


@functools.lru_cache(maxsize=1)
def base_case():
    """Target: the row_mode 1 smoke cloud (12,532 points).  Source: its points with
    ``index % 3 != 1`` and x above the cloud's 20 % quantile (6,681 points), moved by the inverse of
    ``T_true`` (BASE_ANGLES_DEG about the centroid plus BASE_TRANSLATION).  Normals of both at
    radius 9, max_nn 30, each cloud's own.  ``dict(tgt, tgt_nrm, src, src_nrm, T_true, keep)``."""
    P, _ = NR.smoke_cloud(1)
    P = np.ascontiguousarray(P, np.float64)
    keep = (np.arange(len(P)) % 3 != 1) & (P[:, 0] > np.quantile(P[:, 0], 0.2))
    T_true = IR.motion_about(P.mean(0), BASE_ANGLES_DEG, BASE_TRANSLATION)
    src = np.ascontiguousarray(IR.transform_points(IR.inverse_rigid(T_true), P[keep]))
    out = dict(tgt=P, src=src, T_true=T_true, keep=keep)
    for name, X in (("tgt", P), ("src", src)):
        lists = NR.neighbour_lists(X, BASE_MAX_NN, workers=8)
        out[name + "_lists"] = lists
        out[name + "_nrm"] = np.ascontiguousarray(NR.estimate_normals(X, NORMAL_RADIUS, NORMAL_MAX_NN, lists)[2])
    for a in out.values():
        for x in (a if isinstance(a, tuple) else (a,)):
            x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def base_features():
    """The base case's features and correspondences: ``dict(tgt, src (compute_fpfh results), nn_s,
    nn_t, C (mutual), C_all)``."""
    b = base_case()
    out = {name: compute_fpfh(b[name], b[name + "_nrm"], BASE_RADIUS, BASE_MAX_NN, b[name + "_lists"])
           for name in ("tgt", "src")}
    out["nn_s"] = nearest_rows(out["src"]["fpfh"], out["tgt"]["fpfh"])
    out["nn_t"] = nearest_rows(out["tgt"]["fpfh"], out["src"]["fpfh"])
    out["C"] = correspondences(None, None, True, (out["nn_s"], out["nn_t"]))
    out["C_all"] = np.stack([np.arange(len(b["src"]), dtype=np.int64), out["nn_s"].astype(np.int64)], 1)
    return out
