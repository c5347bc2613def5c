"""NumPy restatement of the device self-intersection test (``csrc/cloud_intersect.hip``):
which pairs of triangles of an indexed mesh cross.  This file is the definition; the device is
expected to equal it exactly, every count, both class arrays and both pair lists.

The rule.  A triangle with two equal indices (degenerate) or with a coordinate that is not finite
takes part in nothing.  A candidate pair is ``(s, t)``, ``s < t``, whose closed boxes overlap on all
three axes; the set is grid-free.  Pairs are classed by the vertex *indices* they share: 2 or 3,
adjacent (counted, not tested); 1, both triangles are rotated so that ``a0 == b0`` and only the two
opposite edges are tested; 0, all six edges.  Every sign comes from one expression, :func:`o3`:
Shewchuk's ``orient3dfast`` in fp64 without contraction, with its permanent; a determinant is
*certain* when ``|det| > B * permanent`` (Shewchuk's stage-A bound; no underflow assumed).  An edge
pierces the other triangle iff its two end points lie strictly on opposite sides of the other's
plane and the edge passes the other's three edges on the same strict side.  A zero is never a sign.

What the rule leaves out: coplanar overlaps and coincident but unwelded vertices give zeros, so they
show up as *uncertain*, not as intersecting; a fold across a shared edge is an adjacent pair and is
not tested; Open3D's ``is_self_intersecting`` parity is unpinned.  Also the meshes the tests are
built from.
"""
import numpy as np

import audit_ref as A

B_HEX = "0x1.c000000000007p-51"          # (7 + 56 E) E, E = 2^-53: SLG_ISECT_BOUND of include/slgpu_intersect.h
B = float.fromhex(B_HEX)
INTERSECTING, UNCERTAIN = 1, 2           # the bits of the class byte per triangle and of a pair's verdict
COUNTS = ("candidate_pairs", "adjacent_pairs", "tested_pairs", "intersecting_pairs", "uncertain_pairs",
          "intersecting_triangles", "uncertain_triangles")
CHUNK = 1 << 21                          # pairs per vectorised step (memory only)


# ------------------------------------------------------------------ candidates
def takes_part(V, T):
    """Not degenerate, every coordinate finite."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    return ~A.is_degenerate(T) & np.isfinite(V[T]).all(axis=(1, 2))


def boxes(V, T):
    P = V[np.asarray(T, np.int64)]
    return P.min(axis=1), P.max(axis=1)


def candidates(V, T):
    """int64 ``[n, 2]``: the pairs ``s < t`` of triangles that take part whose boxes overlap in the
    closed sense on all three axes, ascending by ``(s, t)``.  A sweep along x; no grid."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    idx = np.flatnonzero(takes_part(V, T))
    if len(idx) < 2:
        return np.zeros((0, 2), np.int64)
    lo, hi = boxes(V, T[idx])
    order = np.argsort(lo[:, 0], kind="stable")
    idx, lo, hi = idx[order], lo[order], hi[order]
    end = np.searchsorted(lo[:, 0], hi[:, 0], side="right")          # lo_x[j] <= hi_x[i] for i < j < end[i]
    n = np.maximum(end - np.arange(len(idx)) - 1, 0)
    out, i0 = [], 0
    while i0 < len(idx):
        i1 = i0 + 1
        total = int(n[i0])
        while i1 < len(idx) and total + int(n[i1]) <= CHUNK:
            total += int(n[i1])
            i1 += 1
        i = np.repeat(np.arange(i0, i1), n[i0:i1])
        starts = np.cumsum(n[i0:i1]) - n[i0:i1]
        j = np.arange(total) - np.repeat(starts, n[i0:i1]) + i + 1
        ok = np.ones(total, bool)
        for a in range(3):
            ok &= (lo[i, a] <= hi[j, a]) & (lo[j, a] <= hi[i, a])
        out.append(np.stack([np.minimum(idx[i[ok]], idx[j[ok]]), np.maximum(idx[i[ok]], idx[j[ok]])], axis=1))
        i0 = i1
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def candidates_quadratic(V, T):
    """The same set by the O(T^2) loop over all pairs (the check of :func:`candidates`)."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    part = takes_part(V, T)
    lo, hi = boxes(V, T)
    out = []
    for s in range(len(T)):
        for t in range(s + 1, len(T)):
            if part[s] and part[t] and all(lo[s, a] <= hi[t, a] and lo[t, a] <= hi[s, a] for a in range(3)):
                out.append((s, t))
    return np.array(out, np.int64).reshape(-1, 2)


# ------------------------------------------------------------------ the one determinant
def o3(a, b, c, d):
    """``(det, permanent)`` of the points ``[n, 3]``: nine rounded differences, six products, every
    sum in the order written."""
    adx, ady, adz = a[:, 0] - d[:, 0], a[:, 1] - d[:, 1], a[:, 2] - d[:, 2]
    bdx, bdy, bdz = b[:, 0] - d[:, 0], b[:, 1] - d[:, 1], b[:, 2] - d[:, 2]
    cdx, cdy, cdz = c[:, 0] - d[:, 0], c[:, 1] - d[:, 1], c[:, 2] - d[:, 2]
    m1, m2 = bdy * cdz, bdz * cdy
    m3, m4 = cdy * adz, cdz * ady
    m5, m6 = ady * bdz, adz * bdy
    det = (adx * (m1 - m2) + bdx * (m3 - m4)) + cdx * (m5 - m6)
    perm = ((np.abs(m1) + np.abs(m2)) * np.abs(adx) + (np.abs(m3) + np.abs(m4)) * np.abs(bdx)) + \
        (np.abs(m5) + np.abs(m6)) * np.abs(cdx)
    return det, perm


class Sign:
    """A determinant's strict sign and whether it is certain."""

    def __init__(self, det, perm):
        self.pos, self.neg = det > 0.0, det < 0.0
        self.certain = np.abs(det) > B * perm


def opposite(p, q):
    return (p.pos & q.neg) | (p.neg & q.pos)


def edge_test(p1, p2, e):
    """``(pierces, certainly excluded, certainly piercing)`` of one edge against one triangle: the
    plane sides ``p1``, ``p2`` of its end points and its sides ``e[0..2]`` of the triangle's edges."""
    pierces = opposite(p1, p2) & ((e[0].pos & e[1].pos & e[2].pos) | (e[0].neg & e[1].neg & e[2].neg))
    excluded = p1.certain & p2.certain & ((p1.pos & p2.pos) | (p1.neg & p2.neg))
    for k, l in ((0, 1), (0, 2), (1, 2)):
        excluded = excluded | (e[k].certain & e[l].certain & opposite(e[k], e[l]))
    piercing = pierces & p1.certain & p2.certain & e[0].certain & e[1].certain & e[2].certain
    return pierces, excluded, piercing


def rotate_to_shared(Ta, Tb):
    """``(shared count, Ta, Tb)`` with the triangles of one shared index rotated cyclically so that
    ``Ta[:, 0] == Tb[:, 0]``."""
    eq = Ta[:, :, None] == Tb[:, None, :]
    shared = eq.any(axis=2).sum(axis=1)
    one = shared == 1
    ia = np.where(one, eq.any(axis=2).argmax(axis=1), 0)
    ib = np.where(one, eq.any(axis=1).argmax(axis=1), 0)
    k = np.arange(3)[None, :]
    rows = np.arange(len(Ta))[:, None]
    return shared, Ta[rows, (ia[:, None] + k) % 3], Tb[rows, (ib[:, None] + k) % 3]


def pair_verdicts(V, T, pairs, sign=None):
    """``(shared, verdict)`` per candidate pair: ``verdict`` has INTERSECTING and / or UNCERTAIN, 0
    for an adjacent pair.  ``sign(a, b, c, d) -> Sign`` replaces the fp64 determinant (the exact
    check of tests/test_intersect_ref.py)."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    sign = sign or (lambda a, b, c, d: Sign(*o3(a, b, c, d)))
    shared, Ta, Tb = rotate_to_shared(T[pairs[:, 0]], T[pairs[:, 1]])
    a, b = [V[Ta[:, i]] for i in range(3)], [V[Tb[:, j]] for j in range(3)]
    alpha = [sign(a[0], a[1], a[2], b[j]) for j in range(3)]
    beta = [sign(b[0], b[1], b[2], a[i]) for i in range(3)]
    eps = [[sign(a[i], a[(i + 1) % 3], b[j], b[(j + 1) % 3]) for j in range(3)] for i in range(3)]
    tested = shared <= 1
    hit = np.zeros(len(pairs), bool)
    sure = np.zeros(len(pairs), bool)
    open_ = np.zeros(len(pairs), bool)
    for k in range(3):
        on = tested & ((shared == 0) | (k == 1))
        for p1, p2, e in ((beta[k], beta[(k + 1) % 3], eps[k]),                               # edge a_k a_k+1 against B
                          (alpha[k], alpha[(k + 1) % 3], [eps[i][k] for i in range(3)])):      # edge b_k b_k+1 against A
            pierces, excluded, piercing = edge_test(p1, p2, e)
            hit |= on & pierces
            sure |= on & piercing
            open_ |= on & ~excluded & ~piercing
    verdict = np.where(hit, INTERSECTING, 0) | np.where(~sure & open_, UNCERTAIN, 0)
    return shared, verdict.astype(np.uint8)


# ------------------------------------------------------------------ the whole answer
def verdict(counts):
    return counts["intersecting_pairs"] == 0 and counts["uncertain_pairs"] == 0


def self_intersections(V, T):
    """The record of ``mesh.self_intersections(m, return_pairs=True, return_arrays=True)`` without
    the grid's informational counts: COUNTS, ``intersection_free``, ``triangle_class`` uint8 ``[T]``,
    ``pairs`` and ``uncertain`` int32 ``[K, 2]`` ascending by ``(s, t)``."""
    V = np.ascontiguousarray(V, np.float64).reshape(-1, 3)
    T = A.check_indices(T, len(V))
    res = dict.fromkeys(COUNTS, 0)
    tclass = np.zeros(len(T), np.uint8)
    lists = {INTERSECTING: [], UNCERTAIN: []}
    if len(V) and len(T):
        cand = candidates(V, T)
        res["candidate_pairs"] = len(cand)
        for c0 in range(0, len(cand), CHUNK):
            pairs = cand[c0:c0 + CHUNK]
            shared, v = pair_verdicts(V, T, pairs)
            res["adjacent_pairs"] += int((shared >= 2).sum())
            res["tested_pairs"] += int((shared <= 1).sum())
            for bit in (INTERSECTING, UNCERTAIN):
                on = (v & bit) != 0
                lists[bit].append(pairs[on])
                np.bitwise_or.at(tclass, pairs[on].ravel(), np.uint8(bit))
    both = {bit: (np.concatenate(l) if l else np.zeros((0, 2), np.int64)).astype(np.int32) for bit, l in lists.items()}
    res.update(intersecting_pairs=len(both[INTERSECTING]), uncertain_pairs=len(both[UNCERTAIN]),
               intersecting_triangles=int(((tclass & INTERSECTING) != 0).sum()),
               uncertain_triangles=int(((tclass & UNCERTAIN) != 0).sum()))
    res["intersection_free"] = verdict(res)
    res.update(triangle_class=tclass, pairs=both[INTERSECTING], uncertain=both[UNCERTAIN])
    return res


# ------------------------------------------------------------------ meshes: (V float64 [n, 3], T int32 [m, 3])
def _mesh(V, T):
    return np.ascontiguousarray(V, np.float64).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)


def merge(*meshes):
    V, T, base = [], [], 0
    for v, t in meshes:
        V.append(v)
        T.append(np.asarray(t, np.int64) + base)
        base += len(v)
    return _mesh(np.concatenate(V), np.concatenate(T))


def hand(case):
    """The issue's hand cases."""
    flat = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    if case in ("pierced", "lifted"):
        dz = 2.0 if case == "lifted" else 0.0
        return _mesh(flat + [[1, 1, -1 + dz], [1, 1, 1 + dz], [5, 5, 1 + dz]], [[0, 1, 2], [3, 4, 5]])
    if case == "shared_vertex":                     # vertex 0 shared; the edge 3-4 opposite it goes through the first triangle
        return _mesh(flat + [[1, 1, -1], [1, 1, 1]], [[0, 1, 2], [3, 4, 0]])
    if case == "flat_grid":                         # 3 x 3 quads in the plane z = 0: neighbours coplanar and disjoint
        n = 4
        V = [[x, y, 0] for y in range(n) for x in range(n)]
        T = []
        for y in range(n - 1):
            for x in range(n - 1):
                a = y * n + x
                T += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
        return _mesh(V, T)
    if case == "edge_sharing":                      # a fold over the shared edge 0-1: adjacent, not tested
        return _mesh(flat + [[1, 3, 0.5]], [[0, 1, 2], [1, 0, 3]])
    raise KeyError(case)


def soup(seed, nt=60, nv=45, flat=12, span=50):
    """``nt`` triangles over a pool of ``nv`` vertices with integer coordinates in ``-span .. span``, the
    first ``flat`` of them in the plane z = 0 (coplanar pairs and exact zeros), indices drawn so that
    triangles share none, one, two or three of them; one in ten is degenerate."""
    g = np.random.default_rng(seed)
    V = g.integers(-span, span + 1, size=(nv, 3)).astype(np.float64)
    V[:flat, 2] = 0.0
    T = np.stack([g.permutation(nv)[:3] for _ in range(nt)])
    low = g.random(nt) < 0.3                        # some triangles wholly in the plane
    T[low] = np.stack([g.permutation(flat)[:3] for _ in range(int(low.sum()))]) if low.any() else T[low]
    deg = g.random(nt) < 0.1
    T[deg, 2] = T[deg, 0]
    return _mesh(V, T)


def two_spheres():
    """The closed depth-5 sphere and a copy shifted by half its radius along x."""
    V, T = A.BUILDERS["sphere5"]()
    V = np.asarray(V, np.float64)
    r = 0.5 * float((V.max(axis=0) - V.min(axis=0)).max())
    return merge((V, T), (V + [0.5 * r, 0.0, 0.0], T))


def fan(n, center=(0.0, 0.0, 0.0), size=1e-3, tilt=0.0):
    """``n`` small triangles around ``center`` that share no index: a stack of slightly rotated
    triangles whose boxes all overlap, inside one grid cell when the cell is larger than ``size``."""
    ang = np.linspace(0.0, np.pi, n, endpoint=False) + tilt
    k = np.arange(n)
    c = np.asarray(center, np.float64)
    p0 = c + size * np.stack([np.cos(ang), np.sin(ang), 0.2 * (k / max(n, 1) - 0.5)], axis=1)
    p1 = c + size * np.stack([np.cos(ang + 2.1), np.sin(ang + 2.1), 0.2 * (k / max(n, 1) - 0.5)], axis=1)
    p2 = c + size * np.stack([np.cos(ang + 4.2), np.sin(ang + 4.2), 0.3 + 0.0 * ang], axis=1)
    V = np.stack([p0, p1, p2], axis=1).reshape(-1, 3)
    return _mesh(V, np.arange(3 * n).reshape(n, 3))


def runs(n):
    """A fan of ``n`` triangles in one cell and, far away, a few more, so that the default cell stays
    near the fan's size and the grid has other cells."""
    return merge(fan(n), fan(3, center=(0.05, 0.02, 0.01)), fan(2, center=(-0.035, 0.04, 0.0)))


def carpet(nx, ny, h=1.0, z=0.0):
    """``nx * ny`` small separate triangles, one per unit square of the plane ``z``."""
    xs, ys = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="xy")
    o = np.stack([xs.ravel(), ys.ravel(), np.full(nx * ny, z)], axis=1)
    V = np.stack([o + [0.2 * h, 0.2 * h, 0.0], o + [0.8 * h, 0.3 * h, 0.0], o + [0.4 * h, 0.8 * h, 0.0]], axis=1).reshape(-1, 3)
    return _mesh(V, np.arange(3 * nx * ny).reshape(-1, 3))


def blade(x0, x1, y, z0, z1):
    """One long thin upright triangle through the plane z = 0 along x."""
    return _mesh([[x0, y, z0], [x1, y + 0.05, z0], [0.5 * (x0 + x1), y + 0.02, z1]], [[0, 1, 2]])


def large_mesh():
    """1,000 small triangles (a 40 x 25 carpet), one blade crossing a row of them, and several large
    blades crossing each other and the carpet, the last one slanted through all of it: the large list and its ownership rule."""
    big = [blade(-1.0, 41.0, 3.5, -0.5, 0.6), blade(-1.0, 41.0, 10.5, -0.4, 0.5),
           _mesh([[5.1, -1.0, -0.3], [5.3, 26.0, -0.3], [5.2, 12.0, 0.7]], [[0, 1, 2]]),
           _mesh([[20.1, -1.0, -0.3], [20.4, 26.0, -0.2], [20.2, 12.0, 0.9]], [[0, 1, 2]]),
           _mesh([[-1.0, -1.0, -0.3], [41.0, 0.0, -0.2], [20.0, 26.0, 0.5]], [[0, 1, 2]])]
    return merge(big[0], carpet(40, 25), *big[1:])


def span_mesh(cells):
    """A carpet with unit cells (``_cell=1``) and one flat sliver spanning exactly ``cells`` cells of
    one row, dipping through the carpet's plane."""
    sliver = _mesh([[0.1, 0.5, -0.01], [cells - 0.5, 0.52, -0.01], [0.5 * cells, 0.51, 0.01]], [[0, 1, 2]])
    return merge(carpet(max(cells, 2), 2), sliver)


def wide_pair():
    """Two crossing triangles whose boxes overlap in 3 x 3 x 3 cells of a unit grid, and a far one."""
    return _mesh([[0.1, 0.1, 0.1], [2.9, 0.2, 1.5], [1.5, 2.9, 2.9], [0.2, 2.8, 0.2], [2.8, 2.9, 1.4], [1.4, 0.1, 2.8],
                  [9.0, 9.0, 9.0], [9.5, 9.0, 9.0], [9.0, 9.5, 9.2]], [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
