"""The restatement of the mesh audit (tests/audit_ref.py) against independent facts:
SciPy's connected components over the triangle edge-adjacency graph, the closed forms of the small
solids, and what flipping, removing, pinching and repeating a face must do to the counts."""
import numpy as np
import pytest

import audit_ref as A
import meshpost_ref as P


def scipy_components(T):
    """Labels by first triangle from scipy.sparse.csgraph over "share an undirected edge"."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    T = np.asarray(T, np.int64).reshape(-1, 3)
    live = np.flatnonzero(~A.is_degenerate(T))
    by_edge = {}
    for t in live:
        for e in range(3):
            a, b = int(T[t, e]), int(T[t, (e + 1) % 3])
            by_edge.setdefault((min(a, b), max(a, b)), []).append(int(t))
    rows, cols = [], []
    for ts in by_edge.values():
        for u in ts[1:]:
            rows.append(ts[0])
            cols.append(u)
    n = len(T)
    _, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)
    out, rank = np.full(n, -1, np.int32), {}
    for t in live:                                           # relabel by first triangle
        out[t] = rank.setdefault(int(lab[t]), len(rank))
    return out


@pytest.mark.parametrize("name", ("tetrahedron", "octahedron", "open_strip", "bow_tie", "duplicated", "fan", "strip257",
                                  "tetrahedra1000", "book80", "two_tetrahedra_vertex", "two_tetrahedra_edge", "moebius",
                                  "octahedron_degenerate", "trimmed5"))
def test_components_equal_scipy(name):
    V, T = A.BUILDERS[name]()
    labels, sizes = A.connected_components(V, T)
    want = scipy_components(T)
    assert np.array_equal(labels, want)
    assert np.array_equal(sizes, np.bincount(want[want >= 0], minlength=want.max() + 1))
    if name == "tetrahedra1000":
        assert len(sizes) == 1000 and (sizes == 4).all()


def test_tetrahedron_and_its_defects():
    V, T = P.tetrahedron()
    a = A.audit(V, T)
    assert a["signed_volume"] == 1.0 / 6.0 and a["watertight"] and a["components"] == 1 and a["edges"] == 6
    assert a["area"] == pytest.approx(1.5 + 0.5 * np.sqrt(3.0), rel=1e-15)
    flipped = T.copy()
    flipped[2] = flipped[2, ::-1]
    f = A.audit(V, flipped)
    assert f["inconsistent_edges"] == 3 and f["closed"] and not f["oriented"] and not f["watertight"]
    assert int((f["vertex_class"] & A.ON_INCONSISTENT_EDGE != 0).sum()) == 3
    o = A.audit(V, T[:3])
    assert o["boundary_edges"] == 3 and not o["closed"] and o["oriented"] and o["manifold_edges"] == 3
    assert A.audit(V, T[:, ::-1])["signed_volume"] == -1.0 / 6.0


def test_small_meshes():
    m = A.audit(*A.moebius())
    assert m["inconsistent_edges"] >= 1 and m["nonmanifold_edges"] == 0 and m["nonmanifold_vertices"] == 0 and m["components"] == 1
    p = A.audit(*A.two_tetrahedra(1))
    assert (p["nonmanifold_vertices"], p["components"], p["nonmanifold_edges"], p["boundary_edges"]) == (1, 2, 0, 0)
    assert p["edge_manifold"] and p["closed"] and p["oriented"] and not p["vertex_manifold"] and not p["watertight"]
    assert p["vertex_class"][0] & A.NONMANIFOLD_VERTEX and p["signed_volume"] == pytest.approx(1.0 / 3.0, rel=1e-15)
    e = A.audit(*A.two_tetrahedra(2))
    assert e["nonmanifold_edges"] == 1 and e["components"] == 1 and e["nonmanifold_vertices"] == 0
    b = A.audit(*A.book(3))
    assert b["nonmanifold_edges"] == 1 and b["boundary_edges"] == 6 and b["components"] == 1
    tie = A.audit(*P.bow_tie())
    assert tie["nonmanifold_vertices"] == 1 and tie["components"] == 1
    one = A.audit(*A.BUILDERS["one_vertex"]())
    assert one["unreferenced_vertices"] == 1 and not one["watertight"] and one["closed"]
    u = A.audit(*P.unreferenced_vertex())
    assert u["unreferenced_vertices"] == 1 and u["watertight"] and u["signed_volume"] == pytest.approx(4.0 / 3.0, rel=1e-15)


def test_duplicates_and_clean():
    V, T = A.octahedron_variant("reversed_repeat")
    a = A.audit(V, T)
    assert a["duplicate_triangles"] == 1 and a["triangle_class"][8] == A.DUPLICATE and a["nonmanifold_edges"] == 3
    Vc, Tc, _, rec = A.clean(V, T)
    V0, T0 = P.octahedron()
    assert np.array_equal(Vc, V0) and np.array_equal(Tc, T0) and rec == dict(degenerate_removed=0, duplicates_removed=1,
                                                                               vertices_removed=0)
    r = A.audit(*A.octahedron_variant("repeated"))
    assert r["duplicate_triangles"] == 2 and list(np.flatnonzero(r["triangle_class"])) == [8, 9]
    d = A.audit(*A.octahedron_variant("degenerate"))
    assert d["degenerate_triangles"] == 2 and list(d["labels"][8:]) == [-1, -1] and d["components"] == 1 and not d["watertight"]
    assert d["closed"] and d["edges"] == 12
    bk = A.audit(*A.BUILDERS["book80"]())
    assert bk["duplicate_triangles"] == 5 and bk["nonmanifold_edges"] == 3 and bk["triangles"] == 85
    Vk, Tk, Dk, rec = A.clean(*A.BUILDERS["book80"](), np.arange(82.0))
    assert len(Tk) == 80 and np.array_equal(Dk, np.arange(82.0)) and rec["duplicates_removed"] == 5


def test_keep_components():
    V, T = A.disjoint_tetrahedra(5)
    T = np.concatenate([T, [[0, 1, 2]]]).astype(np.int32)                # the first tetrahedron gets a fifth triangle
    Vk, Tk, _, rec = A.keep_largest_components(V, T, None, 1)
    assert len(Vk) == 4 and len(Tk) == 5 and rec == dict(components_before=5, components_after=1, triangles_removed=16,
                                                        vertices_removed=16)
    Vk, Tk, _, rec = A.keep_largest_components(V, T, None, 2)             # the tie among the others: the lower label
    assert sorted(set(Tk.reshape(-1))) == list(range(8)) and len(Vk) == 8
    Vk, Tk, _, rec = A.remove_small_components(V, T, None, 5)
    assert len(Tk) == 5 and rec["components_after"] == 1
    assert len(A.remove_small_components(V, T, None, 0)[1]) == 21


def test_tree_sum_is_the_fixed_shape():
    g = np.random.default_rng(1)
    for n in (1, 8, 9, A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 1):
        x = g.standard_normal(n)
        assert A.tree_sum(x) == pytest.approx(float(np.sum(x)), abs=1e-10)
    assert A.tree_sum(np.array([1.0, 2.0 ** -53, 2.0 ** -53])) == 1.0     # ((0 + 1) + e) + e stays 1: one thread's order
    y = np.zeros(16)
    y[0], y[8], y[9] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert A.tree_sum(y) == 1.0 + 2.0 ** -52                              # the second thread sums e + e first
