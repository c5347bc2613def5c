"""NumPy restatement of the point-to-plane ICP, the rigid transform and the concatenation of
``csrc/cloud_icp.hip`` (test helper, like ``cloud_ref.py`` and ``normals_ref.py``).

Open3D's ``PointCloud::Transform``, ``GetRegistrationResultAndCorrespondences``,
``TransformationEstimationPointToPlane::ComputeTransformation``, ``TransformVector6dToMatrix4d``
and ``RegistrationICP`` as published, restated; parity with an installed Open3D is unpinned
(DESIGN.md §12).  Each rule is one function here, as it is one ``__device__`` function in the HIP
source.  ``cKDTree`` only proposes candidates: every distance is recomputed with ``cloud_ref.d2``
and the candidates are ranked by (d2, index).  The sums are exactly rounded (``math.fsum``); the
LDL' solve repeats the device's operation order in Python floats (IEEE doubles, no FMA), so it
is bit-equal to the device.
"""
import math

import numpy as np
from scipy.spatial import cKDTree

from cloud_ref import d2

LOG_STRIDE = 56            # SLG_ICP_LOG_STRIDE: T 0:16, n_corr, err2, fitness, rmse, sums 20:47, x 47:53, flags 53
LOG_STOP, LOG_SOLVED, LOG_SINGULAR, LOG_LAST = 1, 2, 4, 8


# ------------------------------------------------------------------ transform and concat
def transform_points(T, P):
    """p'[a] = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3]."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


def transform_normals(T, Nrm):
    """The 3x3 block, no translation."""
    x, y, z = Nrm[:, 0], Nrm[:, 1], Nrm[:, 2]
    return np.stack([(T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z for a in range(3)], 1)


def matrix_ok(T):
    T = np.asarray(T, np.float64)
    return T.shape == (4, 4) and bool(np.isfinite(T).all()) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def concat(a, b):
    return np.concatenate([a, b])


# ------------------------------------------------------------------ correspondence
def brute_correspondence(q, tgt, d):
    """``(index, d2)`` of the smallest (d2, index) among d2 < d*d for one query, or ``(-1, inf)``."""
    D = d2(q, tgt)
    D = np.where(D < d * d, D, np.inf)
    j = int(np.lexsort((np.arange(len(tgt)), D))[0])
    return (j, float(D[j])) if np.isfinite(D[j]) else (-1, np.inf)


def correspondences(Q, tgt, d, tree=None, kq=16, workers=1):
    """``(corr int32 [n], dd float64 [n])``: per query the target point with the smallest
    (d2, target index) among those with d2 < d*d (strict), ``-1`` / ``inf`` with none.  A query
    whose tie at the front could run past the ``kq`` proposed candidates is redone by brute
    force."""
    Q = np.ascontiguousarray(Q, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    n, nt = len(Q), len(tgt)
    kq = min(kq, nt)
    tree = tree if tree is not None else cKDTree(tgt)
    finite = np.isfinite(Q).all(1)
    cand = np.full((n, kq), nt, np.int64)
    if finite.any():
        cand[finite] = tree.query(Q[finite], k=kq, distance_upper_bound=d * (1 + 1e-9), workers=workers)[1].reshape(-1, kq)
    valid = cand < nt
    c = np.where(valid, cand, 0)
    with np.errstate(all="ignore"):
        D = d2(Q[:, None, :], tgt[c])
    inside = valid & (D < d * d)
    D = np.where(inside, D, np.inf)
    c = np.where(inside, c, nt)
    o = np.lexsort((c, D), axis=1)
    c, D = np.take_along_axis(c, o, 1), np.take_along_axis(D, o, 1)
    corr, dd = np.where(np.isfinite(D[:, 0]), c[:, 0], -1), D[:, 0].copy()
    if kq < nt:
        for i in np.flatnonzero(valid.all(1) & (D[:, kq - 1] <= D[:, 0] * (1 + 1e-12))):
            corr[i], dd[i] = brute_correspondence(Q[i], tgt, d)
    return corr.astype(np.int32), dd


def evaluate(src, tgt, T, d, tree=None, workers=1):
    """The evaluation at ``T``: ``dict(corr, dd, n_corr, err2, fitness, rmse, S)`` with ``S`` the
    transformed source."""
    S = transform_points(np.asarray(T, np.float64), np.ascontiguousarray(src, np.float64))
    corr, dd = correspondences(S, tgt, d, tree, workers=workers)
    m = corr >= 0
    n_corr = int(m.sum())
    err2 = math.fsum(dd[m])
    return dict(corr=corr, dd=dd, n_corr=n_corr, err2=err2, fitness=n_corr / len(src),
                rmse=math.sqrt(err2 / n_corr) if n_corr else 0.0, S=S)


# ------------------------------------------------------------------ linear system
def ut(a, b):
    """Index of entry (a, b), a <= b, of a 6x6 upper triangle stored row by row."""
    return a * 6 - a * (a - 1) // 2 + (b - a)


def terms(s, t, n):
    """float64 [m, 27]: per correspondence the 21 upper-triangle entries of J J' and the 6 of J r,
    with r = ((s - t) . n) summed x, y, z and J = [s x n, n]."""
    dx, dy, dz = s[:, 0] - t[:, 0], s[:, 1] - t[:, 1], s[:, 2] - t[:, 2]
    r = (dx * n[:, 0] + dy * n[:, 1]) + dz * n[:, 2]
    J = [s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2],
         s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
    out = np.empty((len(s), 27))
    for a in range(6):
        for b in range(a, 6):
            out[:, ut(a, b)] = J[a] * J[b]
        out[:, 21 + a] = J[a] * r
    return out


def sums(ev, tgt, nrm):
    """``(sums [27], abs_sums [27])`` of an evaluation: ``math.fsum`` of the terms and of their
    magnitudes (the scale of the fixed tree's error bound)."""
    m = ev["corr"] >= 0
    c = ev["corr"][m]
    tm = terms(ev["S"][m], tgt[c], nrm[c])
    return (np.array([math.fsum(tm[:, k]) for k in range(27)]),
            np.array([math.fsum(np.abs(tm[:, k])) for k in range(27)]))


def ldlt_solve(S):
    """``(x [6], ok)``: JTJ x = -JTr by LDL' without pivoting in the device's operation order
    (``ldlt_solve_rule``).  ``S``: the 27 sums.  ``ok`` is False, and x zero, when a pivot is <= 0
    or not finite."""
    S = [float(v) for v in S]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    ok = True

    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    for j in range(6):
        dj = S[ut(j, j)]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        ok = ok and dj > 0.0 and math.isfinite(dj)
        D[j] = dj
        for i in range(j + 1, 6):
            v = S[ut(j, i)]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = div(v, dj)
    y = [0.0] * 6
    for i in range(6):
        v = -S[21 + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = div(y[i], D[i])
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    return (np.array(x), True) if ok else (np.zeros(6), False)


def full_system(S):
    """``(JTJ [6, 6], JTr [6])`` of the 27 sums."""
    A = np.empty((6, 6))
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = S[ut(a, b)]
    return A, np.asarray(S[21:27], np.float64)


# ------------------------------------------------------------------ update and loop
def update_matrix(x):
    """TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]) multiplied out, t = x[3:6]."""
    ca, sa, cb, sb, cg, sg = (math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]),
                              math.sin(x[2]))
    return np.array([[cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa, x[3]],
                     [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def apply_update(x, T):
    """T <- U T, each entry summed left to right; the last row stays 0 0 0 1."""
    U = update_matrix(x)
    out = np.array(T, np.float64)
    for a in range(3):
        for b in range(4):
            out[a, b] = ((U[a, 0] * T[0, b] + U[a, 1] * T[1, b]) + U[a, 2] * T[2, b]) + U[a, 3] * T[3, b]
    return out


def stop_rule(fitness, prev_fitness, rmse, prev_rmse, relative_fitness, relative_rmse):
    return abs(fitness - prev_fitness) < relative_fitness and abs(rmse - prev_rmse) < relative_rmse


def step(ev, tgt, nrm):
    """``(x, ok, S27, abs27)`` of the step after an evaluation: the identity (x = 0, ok False)
    without correspondences, without normals or with a bad pivot."""
    if nrm is None or ev["n_corr"] == 0:
        return np.zeros(6), False, np.zeros(27), np.zeros(27)
    S, A = sums(ev, tgt, nrm)
    x, ok = ldlt_solve(S)
    return x, ok, S, A


def registration_icp(src, tgt, nrm, d, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                     workers=1):
    """The loop: evaluate at ``init``; then up to ``max_iteration`` times solve, update, evaluate,
    stopping after an evaluation that meets :func:`stop_rule`.  ``dict(T, fitness, rmse, n_corr,
    iterations, converged, corr, log)``; ``log`` holds one dict per evaluation (``T, n_corr, err2,
    fitness, rmse, S, x, ok``)."""
    src = np.ascontiguousarray(src, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    tree = cKDTree(tgt)
    ev = evaluate(src, tgt, T, d, tree, workers)
    log, converged, it = [], False, 0
    while True:
        rec = dict(T=T.copy(), n_corr=ev["n_corr"], err2=ev["err2"], fitness=ev["fitness"], rmse=ev["rmse"], S=None,
                   x=np.zeros(6), ok=False)
        log.append(rec)
        if converged or it == max_iteration:
            break
        rec["x"], rec["ok"], rec["S"], _ = step(ev, tgt, nrm)
        if rec["ok"]:
            T = apply_update(rec["x"], T)
        prev, ev = ev, evaluate(src, tgt, T, d, tree, workers)
        it += 1
        converged = stop_rule(ev["fitness"], prev["fitness"], ev["rmse"], prev["rmse"], relative_fitness, relative_rmse)
    return dict(T=T, fitness=ev["fitness"], rmse=ev["rmse"], n_corr=ev["n_corr"], iterations=it, converged=converged,
                corr=ev["corr"], log=log)


# ------------------------------------------------------------------ the base case
BASE_ANGLES_DEG = (1.0, -1.5, 0.7)
BASE_TRANSLATION = (1.2, -0.8, 0.9)
BASE_DIST = 6.0
BASE_DISPLACED_EVERY = 13          # every 13th source point is moved 50 mm away: no match


def motion_about(centre, angles_deg, translation):
    """The 4x4 of a rotation Rz Ry Rx (degrees) about ``centre`` plus a translation."""
    M = update_matrix([math.radians(a) for a in angles_deg] + [0.0, 0.0, 0.0])
    c = np.asarray(centre, np.float64)
    M[:3, 3] = c - M[:3, :3] @ c + np.asarray(translation, np.float64)
    return M


def inverse_rigid(M):
    out = np.eye(4)
    out[:3, :3] = M[:3, :3].T
    out[:3, 3] = -M[:3, :3].T @ M[:3, 3]
    return out


def base_case(displaced=True):
    """Target: the row_mode 1 smoke cloud (12,532 points) with normals at radius 9, max_nn 30.
    Source: every third target point moved by the inverse of ``T_true`` (BASE_ANGLES_DEG about the
    centroid plus BASE_TRANSLATION), every BASE_DISPLACED_EVERY-th of them first pushed 50 mm
    along -z (towards the camera, at least 17 mm from every target point).  ``dict(tgt, nrm, src, T_true, moved bool [n_source], d)``."""
    import normals_ref as NR
    P, _ = NR.smoke_cloud(1)
    P = np.ascontiguousarray(P, np.float64)
    nrm = NR.estimate_normals(P, 9.0, 30, NR.neighbour_lists(P, 30, workers=8))[2]
    T_true = motion_about(P.mean(0), BASE_ANGLES_DEG, BASE_TRANSLATION)
    S = P[::3].copy()
    moved = np.zeros(len(S), bool)
    if displaced:
        moved[::BASE_DISPLACED_EVERY] = True
        S[moved] += [0.0, 0.0, -50.0]
    src = transform_points(inverse_rigid(T_true), S)
    return dict(tgt=P, nrm=np.ascontiguousarray(nrm), src=np.ascontiguousarray(src), T_true=T_true, moved=moved,
                d=BASE_DIST)


def motion_error(T_est, T_true, src):
    """max_i |T_est p_i - T_true p_i| over the given source points."""
    return float(np.linalg.norm(transform_points(T_est, src) - transform_points(T_true, src), axis=1).max())
