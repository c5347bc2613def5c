"""NumPy restatement of the tangent-plane normal orientation of ``csrc/cloud_orient.hip`` (test
helper, like ``plane_ref.py``): Open3D's ``orient_normals_consistent_tangent_plane`` in closed form
(parity with an installed Open3D is unpinned).  Each rule is one function here, as
it is one ``__device__`` function there.  Everything is fp64 with separate multiplies and adds and
the device builds with ``-ffp-contract=off``, so every rule is the same sequence of IEEE operations
on both sides.

The formulation is deliberately not the device's: Kruskal over sorted edge lists instead of
Boruvka rounds, and a literal queue traversal from the root that applies the sign rule edge by
edge instead of parities in a union-find.  Brute force over all pairs: use ``N <= ~3000``;
:func:`emst_delaunay` proposes candidates from ``scipy.spatial.Delaunay`` for larger clouds
without cospherical ties."""
from collections import deque

import numpy as np

from cloud_ref import d2


# ------------------------------------------------------------------ the rules
def neighbour_lists(P, k, block=256):
    """``(idx int64 [n, kk], dd float64 [n, kk])``, ``kk = min(k, n)``: every point's first ``kk``
    points in ascending ``(d2, input index)`` order, the point itself included."""
    P = np.asarray(P, np.float64)
    n = len(P)
    kk = min(int(k), n)
    idx = np.empty((n, kk), np.int64)
    dd = np.empty((n, kk), np.float64)
    for s in range(0, n, block):
        D = d2(P[s:s + block, None, :], P[None, :, :])
        order = np.argsort(D, axis=1, kind="stable")[:, :kk]         # stable: ties by ascending index
        idx[s:s + block] = order
        dd[s:s + block] = np.take_along_axis(D, order, axis=1)
    return idx, dd


def drop_self(idx, dd):
    """The lists with the point itself removed; a row without it loses its last entry (cloud.knn_lists)."""
    n, kk = idx.shape
    keep = idx != np.arange(n)[:, None]
    keep[:, kk - 1] &= ~keep.all(axis=1)
    return idx[keep].reshape(n, kk - 1), dd[keep].reshape(n, kk - 1)


def edge_weight(Nrm, a, b):
    """The Riemannian weight ``1 - |na . nb|``, the dot product summed x, y, z."""
    return 1.0 - np.abs((Nrm[a, 0] * Nrm[b, 0] + Nrm[a, 1] * Nrm[b, 1]) + Nrm[a, 2] * Nrm[b, 2])


def edge_sign(Nrm, a, b):
    """``sgn(na . nb)`` on the input normals with ``sgn(0) = +1`` (ours)."""
    return -1 if (Nrm[a, 0] * Nrm[b, 0] + Nrm[a, 1] * Nrm[b, 1]) + Nrm[a, 2] * Nrm[b, 2] < 0.0 else 1


def root_of(P):
    """The lowest index among the points of largest z."""
    return int(np.flatnonzero(P[:, 2] == P[:, 2].max())[0])


# ------------------------------------------------------------------ Kruskal
def kruskal(n, a, b, w):
    """The minimum spanning forest of the undirected edges ``(a, b)``, ``a < b``, under the total
    order ``(w, a, b)``: its edges, int64 ``[m, 2]`` sorted by ``(a, b)``."""
    order = np.lexsort((b, a, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for e in order:
        ra, rb = find(int(a[e])), find(int(b[e]))
        if ra != rb:
            parent[ra] = rb
            out.append((int(a[e]), int(b[e])))
            if len(out) == n - 1:
                break
    return np.array(sorted(out), np.int64).reshape(-1, 2)


def emst_from_candidates(P, a, b):
    a, b = np.minimum(a, b), np.maximum(a, b)
    return kruskal(len(P), a, b, d2(P[a], P[b]))


def emst_brute(P):
    """The Euclidean minimum spanning tree over all ``n (n - 1) / 2`` pairs in ``(d2, a, b)`` order."""
    P = np.asarray(P, np.float64)
    a, b = np.triu_indices(len(P), 1)
    return emst_from_candidates(P, a, b)


def emst_delaunay(P):
    """The same tree from the Delaunay edges (the EMST is a subgraph of the Delaunay graph).  Valid
    for clouds in general position only: with cospherical ties qhull's choice of diagonal may
    leave out an edge the total order would take."""
    from scipy.spatial import Delaunay
    P = np.asarray(P, np.float64)
    T = Delaunay(P).simplices
    pairs = np.concatenate([T[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    return emst_from_candidates(P, pairs[:, 0], pairs[:, 1])


def riemannian_edges(idx, emst):
    """EMST edges and every ``(i, j)``, ``j`` in ``i``'s list and not ``i``: undirected, unique."""
    n, kk = idx.shape
    i = np.repeat(np.arange(n), kk)
    j = idx.reshape(-1)
    keep = i != j
    pairs = np.stack((np.minimum(i, j)[keep], np.maximum(i, j)[keep]), axis=1)
    pairs = np.unique(np.concatenate((pairs, emst.reshape(-1, 2))), axis=0)
    return pairs[:, 0], pairs[:, 1]


def riemannian_mst(Nrm, idx, emst):
    a, b = riemannian_edges(idx, emst)
    return kruskal(len(Nrm), a, b, edge_weight(Nrm, a, b))


# ------------------------------------------------------------------ the traversal
def propagate(P, Nrm, tree):
    """A literal breadth-first traversal of the tree from the root: the root's normal is negated
    iff its z is negative, and a child's sign is its parent's times the edge's sign."""
    n = len(P)
    adj = [[] for _ in range(n)]
    for a, b in tree:
        adj[a].append(int(b))
        adj[b].append(int(a))
    root = root_of(P)
    sign = np.zeros(n, np.int64)
    sign[root] = -1 if Nrm[root, 2] < 0.0 else 1
    queue = deque([root])
    while queue:
        v = queue.popleft()
        for c in adj[v]:
            if sign[c] == 0:
                sign[c] = sign[v] * edge_sign(Nrm, v, c)
                queue.append(c)
    assert (sign != 0).all()
    out = Nrm.copy()
    out[sign < 0] = -Nrm[sign < 0]
    return out, root


def orient(P, Nrm, k, emst=None):
    """``(normals, tree, root, emst, (idx, dd))`` of the whole procedure."""
    P, Nrm = np.asarray(P, np.float64), np.asarray(Nrm, np.float64)
    idx, dd = neighbour_lists(P, k)
    if emst is None:
        emst = emst_brute(P)
    tree = riemannian_mst(Nrm, idx, emst)
    out, root = propagate(P, Nrm, tree)
    return out, tree, root, emst, (idx, dd)


# ------------------------------------------------------------------ inputs
def sphere_case(n, seed):
    """Unit-sphere points with normals ``+-p / |p|`` (seeded signs): ``(P, signed, outward)``.  The
    point of largest z has ``outward.z > 0``, so orientation gives ``outward``."""
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(n, 3))
    P /= np.sqrt((P * P).sum(axis=1))[:, None]
    out = P / np.sqrt((P * P).sum(axis=1))[:, None]
    flip = rng.random(n) < 0.5
    signed = out.copy()
    signed[flip] = -out[flip]
    return P, signed, out


def random_cloud(n, seed=5):
    """A random cloud with random unit normals (no zero dot products, no ties)."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-30.0, 30.0, (n, 3))
    Nrm = rng.normal(size=(n, 3))
    Nrm /= np.sqrt((Nrm * Nrm).sum(axis=1))[:, None]
    return np.ascontiguousarray(P), np.ascontiguousarray(Nrm)
