"""Two independent restatements of Open3D's ``ClusterDBSCAN`` (test helper, beside ``cloud_ref.py``).

:func:`sequential_labels` is Open3D's published loop, literally: clusters grown one at a time from
seeds taken in index order, the expansion kept in sets.  :func:`closed_labels` is the closed form
the device computes: core counts, connected components of the core-core graph,
components ranked by their smallest core index, a non-core point taking the lowest label among its
core neighbours.  That the two agree is the claim that the labels are a pure function of the input
(``test_cluster_ref.py``).  Parity with an installed Open3D is unpinned.

Both read one neighbour graph: ``cKDTree`` only proposes candidates at ``eps * (1 + 1e-9)``, every
distance is then recomputed with ``cloud_ref.d2`` and judged by ``cloud_ref.radius_neighbour``
(strict; a point is its own neighbour), as in ``cloud_ref.py``.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import cloud_ref as R


def neighbour_graph(P, eps):
    """CSR ``(indptr, indices)``: row i lists the points with ``d2(i, j) < eps**2``, i included,
    ascending.  (``query_pairs`` hands the candidate pairs back as one array; it takes no
    ``workers``, and needs none at these sizes.)"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    pairs = cKDTree(P).query_pairs(eps * (1 + 1e-9), output_type="ndarray").astype(np.int64, copy=False)
    ok = np.empty(len(pairs), bool)
    for s in range(0, len(pairs), 1 << 22):
        e = s + (1 << 22)
        ok[s:e] = R.radius_neighbour(R.d2(P[pairs[s:e, 0]], P[pairs[s:e, 1]]), eps)
    a, b = pairs[ok, 0], pairs[ok, 1]
    self_ = np.flatnonzero(R.radius_neighbour(R.d2(P, P), eps))          # every point, as eps > 0
    rows, cols = np.concatenate([a, b, self_]), np.concatenate([b, a, self_])
    g = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
    g.sort_indices()
    return g.indptr.astype(np.int64), g.indices.astype(np.int64)


def brute_graph(P, eps):
    """The same graph by plain O(N^2) evaluation."""
    P = np.asarray(P, np.float64)
    nb = [np.flatnonzero(R.radius_neighbour(R.d2(p, P), eps)) for p in P]
    indptr = np.zeros(len(P) + 1, np.int64)
    np.cumsum([len(a) for a in nb], out=indptr[1:])
    return indptr, np.concatenate(nb).astype(np.int64) if len(P) else np.zeros(0, np.int64)


def sequential_labels(graph, min_points):
    """Open3D's loop: ``-2`` unvisited, ``-1`` noise; seeds in index order; a noise point reached
    by an expansion becomes a border point of that cluster and is never overwritten."""
    indptr, indices = graph
    n = len(indptr) - 1
    nbs = [indices[indptr[i]:indptr[i + 1]].tolist() for i in range(n)]
    labels = [-2] * n
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            labels[idx] = -1
            continue
        nbs_next = set(nbs[idx])
        nbs_visited = {idx}
        labels[idx] = cluster
        while nbs_next:
            nb = nbs_next.pop()
            nbs_visited.add(nb)
            if labels[nb] == -1:
                labels[nb] = cluster
            if labels[nb] != -2:
                continue
            labels[nb] = cluster
            if len(nbs[nb]) >= min_points:
                for q in nbs[nb]:
                    if q not in nbs_visited:
                        nbs_next.add(q)
        cluster += 1
    return np.array(labels, np.int32)


def core_mask(graph, min_points):
    return np.diff(graph[0]) >= min_points


def closed_labels(graph, min_points):
    indptr, indices = graph
    n = len(indptr) - 1
    core = core_mask(graph, min_points)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    labels = np.full(n, -1, np.int32)
    if not core.any():
        return labels
    cc = core[rows] & core[indices]
    g = csr_matrix((np.ones(int(cc.sum()), np.int8), (rows[cc], indices[cc])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    core_idx = np.flatnonzero(core)
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp[core_idx], core_idx)
    order = np.argsort(smallest, kind="stable")                 # components without a core point sort last
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    labels[core_idx] = rank[comp[core_idx]]
    cb = ~core[rows] & core[indices]                            # non-core point -> core neighbour
    low = np.full(n, np.iinfo(np.int32).max, np.int32)
    np.minimum.at(low, rows[cb], labels[indices[cb]])
    border = ~core & (low != np.iinfo(np.int32).max)
    labels[border] = low[border]
    return labels


def _block_edges(tree, P, queries, eps, workers):
    """(query index, neighbour index) pairs of the rule for the listed query points."""
    lists = tree.query_ball_point(P[queries], eps * (1 + 1e-9), workers=workers)
    lens = np.fromiter((len(l) for l in lists), np.int64, len(queries))
    cols = np.fromiter((j for l in lists for j in l), np.int64, int(lens.sum()))
    rows = np.repeat(queries, lens)
    ok = R.radius_neighbour(R.d2(P[rows], P[cols]), eps)
    return rows[ok], cols[ok]


def closed_labels_blocked(P, eps, min_points, workers=1, block=1 << 14):
    """:func:`closed_labels` for clouds whose whole graph does not fit in memory (a 1080p view
    at eps 5 has 8.6e8 edges): the same closed form, with the core-core edges folded into the
    components one block of query points at a time, and the border points in a last pass."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    core = R.radius_counts(P, eps, workers) >= min_points
    labels = np.full(n, -1, np.int32)
    core_idx = np.flatnonzero(core)
    if not len(core_idx):
        return labels
    tree = cKDTree(P)
    comp = np.arange(n, dtype=np.int64)                         # current component id of every point
    for s in range(0, len(core_idx), block):
        rows, cols = _block_edges(tree, P, core_idx[s:s + block], eps, workers)
        cc = core[cols] & (cols < rows)
        g = csr_matrix((np.ones(int(cc.sum()), np.int32), (comp[rows[cc]], comp[cols[cc]])), shape=(n, n))   # sums repeats
        comp = connected_components(g, directed=False)[1].astype(np.int64)[comp]
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp[core_idx], core_idx)
    order = np.argsort(smallest, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    labels[core_idx] = rank[comp[core_idx]]
    rest = np.flatnonzero(~core)
    for s in range(0, len(rest), block):
        rows, cols = _block_edges(tree, P, rest[s:s + block], eps, workers)
        cb = core[cols]
        low = np.full(n, np.iinfo(np.int32).max, np.int32)
        np.minimum.at(low, rows[cb], labels[cols[cb]])
        hit = np.flatnonzero(low != np.iinfo(np.int32).max)
        labels[hit] = low[hit]
    return labels


def contested(graph, min_points, labels):
    """Non-core points whose core neighbours carry more than one label."""
    indptr, indices = graph
    n = len(indptr) - 1
    core = core_mask(graph, min_points)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cb = ~core[rows] & core[indices]
    lo = np.full(n, np.iinfo(np.int32).max, np.int64)
    hi = np.full(n, -1, np.int64)
    np.minimum.at(lo, rows[cb], labels[indices[cb]])
    np.maximum.at(hi, rows[cb], labels[indices[cb]])
    return int(np.count_nonzero((hi >= 0) & (lo != hi)))


def largest(labels):
    """``(label, member count)`` as ``keep_largest_cluster`` picks it (``np.unique`` sorts,
    ``argmax`` takes the first of equals); ``(-1, 0)`` when there is no cluster."""
    unique_labels, counts = np.unique(labels, return_counts=True)
    valid = unique_labels != -1
    unique_labels, counts = unique_labels[valid], counts[valid]
    if len(unique_labels) == 0:
        return -1, 0
    return int(unique_labels[counts.argmax()]), int(counts.max())


def info(labels):
    """``(n_clusters, largest_label, largest_count, n_noise)``, as ``slg_dbscan`` reports it."""
    lab, cnt = largest(labels)
    return [int(labels.max()) + 1 if len(labels) else 0, lab, cnt, int(np.count_nonzero(labels == -1))]
