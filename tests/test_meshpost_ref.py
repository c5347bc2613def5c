"""Properties of the post-processing rules themselves, on the NumPy restatement (no GPU): the
adjacency is symmetric and sorted, Taubin shrinks less than Laplacian, boundary vertices slide
along the boundary, holes close into closed manifolds, and what stays open is counted."""
import numpy as np
import pytest

import mesh_ref as MR
import meshpost_ref as P


def rows(off, nbr, v):
    return nbr[off[v]:off[v + 1]]


@pytest.mark.parametrize("name", sorted(P.BUILDERS))
def test_adjacency_is_symmetric_and_sorted(name):
    V, T = P.BUILDERS[name]()
    adj = P.adjacency(T, len(V))
    for off, nbr in ((adj["offsets"], adj["neighbours"]), (adj["boundary_offsets"], adj["boundary_neighbours"])):
        assert off[0] == 0 and off[-1] == len(nbr) and (np.diff(off) >= 0).all()
        pairs = set()
        for v in range(len(V)):
            r = rows(off, nbr, v)
            assert (np.diff(r) > 0).all() and v not in r
            pairs.update((v, int(q)) for q in r)
        assert all((b, a) in pairs for a, b in pairs)
    used = np.unique(T)
    assert set(np.flatnonzero(np.diff(adj["offsets"]) == 0)) == set(range(len(V))) - set(used.tolist())
    assert np.array_equal(adj["boundary"] != 0, np.diff(adj["boundary_offsets"]) > 0)
    closed = len(P.boundary_edges(T)) == 0
    assert closed == (not adj["boundary"].any())
    if name in ("tetrahedron", "octahedron", "unreferenced", "sphere4", "sphere5"):
        assert closed
    if name == "single_triangle":
        assert adj["boundary"].all() and np.array_equal(adj["neighbours"], adj["boundary_neighbours"])


def test_unreferenced_and_degenerate():
    V, T = P.unreferenced_vertex()
    adj = P.adjacency(T, len(V))
    assert len(rows(adj["offsets"], adj["neighbours"], 3)) == 0
    Vo, To = P.octahedron()
    Td = np.concatenate([To, [[2, 2, 4]]]).astype(np.int32)
    a, b = P.adjacency(To, 6), P.adjacency(Td, 6)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_taubin_shrinks_less_than_laplacian():
    V, T = P.BUILDERS["sphere5"]()
    v0 = MR.signed_volume(V, T)
    lap = MR.signed_volume(P.smooth_laplacian(V, T, 10), T)
    tau = MR.signed_volume(P.smooth_taubin(V, T, 10), T)
    assert v0 > 0 and abs(tau - v0) < abs(lap - v0) and lap < v0           # Laplacian shrinks; Taubin nearly keeps the volume
    assert np.array_equal(P.smooth_taubin(V, T, 0), V) and np.array_equal(P.smooth_laplacian(V, T, 0), V)


def test_strip_boundary_stays_in_its_plane():
    """Every vertex of a one-quad-high planar strip is a boundary vertex: it moves along the boundary
    polyline only, so z stays 0 and the strip stays inside its bounding rectangle."""
    V, T = P.open_strip()
    adj = P.adjacency(T, len(V))
    assert adj["boundary"].all()
    for out in (P.smooth_laplacian(V, T, 5), P.smooth_taubin(V, T, 5)):
        assert (out[:, 2] == 0.0).all()
    out = P.smooth_laplacian(V, T, 5)
    assert out[:, 0].min() >= V[:, 0].min() and out[:, 0].max() <= V[:, 0].max()
    # an interior vertex next to a boundary does not pull the boundary off its polyline
    V, T = P.grid_patch(4, 4)
    V = V.copy()
    V[12, 2] = 5.0                                    # the centre vertex (2, 2), lifted
    out = P.smooth_laplacian(V, T, 3)
    b = P.adjacency(T, len(V))["boundary"].astype(bool)
    assert (out[b, 2] == 0.0).all() and (out[~b, 2] > 0.0).all()


def test_close_holes_on_closed_meshes_adds_nothing():
    for name in ("tetrahedron", "octahedron", "unreferenced", "sphere4"):
        V, T = P.BUILDERS[name]()
        T2, rec = P.close_holes(V, T, 30)
        assert np.array_equal(T2, T) and rec == dict(boundary_edges=0, closable_loops=0, closable_edges=0, open_by_size_edges=0,
                                                     blocked_edges=0, new_triangles=0)


@pytest.mark.parametrize("L", (3, 4, 5, 30))
def test_punched_sphere_closes(L):
    V, T = P.cone_with_hole(L, seed=L)
    assert MR.topology(T)[1] and len(P.boundary_edges(T)) == L
    T2, rec = P.close_holes(V, T, 30)
    assert rec["closable_loops"] == 1 and rec["new_triangles"] == L - 2 and np.array_equal(T2[:len(T)], T)
    assert MR.topology(T2) == (True, True, 2)
    # the fill faces the way its neighbours do: the closed surface keeps a volume of one sign
    assert MR.signed_volume(V, T2) * MR.signed_volume(V, np.concatenate([T, T2[len(T):]])) > 0


def test_what_stays_open_is_counted():
    V, T = P.cone_with_hole(31)
    T2, rec = P.close_holes(V, T, 30)
    assert np.array_equal(T2, T) and rec["closable_loops"] == 0 and rec["open_by_size_edges"] == 31 and rec["blocked_edges"] == 0
    assert P.close_holes(V, T, 31)[1]["closable_loops"] == 1
    V, T = P.bow_tie()
    T2, rec = P.close_holes(V, T, 3)
    # the two triangular holes share a vertex with two outgoing boundary edges: blocked, both stay open
    assert np.array_equal(T2, T) and rec["blocked_edges"] == 6 and rec["closable_loops"] == 0 and rec["open_by_size_edges"] == 16
    V, T = P.duplicated_triangle()
    rec = P.close_holes(V, T, 30)[1]
    assert rec["closable_loops"] == 0 and rec["blocked_edges"] == rec["boundary_edges"] == 12
    with pytest.raises(AssertionError):
        P.boundary_loops(T, len(V), 65)


def test_tied_diagonals():
    """The hexagon's first clip is decided by the tie rule: four of the inner ring's six short
    diagonals share the smallest squared length, exactly, and the lowest i among them wins."""
    V, T = P.hexagon_hole()
    _, loops = P.boundary_loops(T, len(V), 6)
    ring = [r for _, r in loops if max(r) < 6][0]
    d = [float(((V[ring[(i + 1) % 6]] - V[ring[i - 1]]) ** 2).sum()) for i in range(6)]
    assert sorted(d) == [13.0] * 4 + [16.0] * 2
    i = d.index(13.0)
    assert P.clip_ring(V, ring)[0] == (ring[(i + 1) % 6], ring[i], ring[i - 1])


def test_many_holes_lattice():
    V, T = P.punched_lattice()
    T2, rec = P.close_holes(V, T, 8)
    assert rec["closable_loops"] == 600 and rec["new_triangles"] == 1200 and rec["open_by_size_edges"] == 300
    assert rec["boundary_edges"] == 2700 and rec["blocked_edges"] == 0
    rest = P.boundary_loops(T2, len(V), 8)[0]
    assert rest["boundary_edges"] == 300 and P.directed_unique(T2)


def test_trimmed_sphere_closes():
    """The depth-5 sphere of ``TRIM_N`` = 8000 points, seed ``TRIM_SEED`` = 29, after the 0.02 trim:
    678 boundary edges, 59 closable loops (all of at most 64 edges), 456 new triangles, and every
    directed edge of the closed mesh is unique.  104 boundary edges stay: they lie on walks through
    blocked vertices (holes that share a vertex), which the rule leaves open whatever their size.
    A fill can repeat a directed edge, since there is no existing-edge check: a triangle that juts
    into a hole with two boundary edges is clipped first (its diagonal is short) and the ear lands on
    its back.  Every other cloud searched (300 .. 16,000 points, seeds 0 .. 109, some 490 in all)
    showed 2 to 52 such repeated edges, so no cloud was found that also has no blocked walk."""
    V, T, _ = P.trimmed_sphere()
    assert P.directed_unique(T)
    T2, rec = P.close_holes(V, T, 64)
    assert rec == dict(boundary_edges=678, closable_loops=59, closable_edges=574, open_by_size_edges=0, blocked_edges=104,
                       new_triangles=456)
    assert P.directed_unique(T2) and len(T2) == len(T) + 456
    rest = P.boundary_loops(T2, len(V), 64)[0]
    assert rest["boundary_edges"] == rest["blocked_edges"] == 104 and rest["closable_loops"] == 0
    d = P.winding_pairs(T2)                         # closed wherever it was closable: the rest is the blocked walks' edges
    assert len(P.boundary_edges(T2)) == 104 and len(d) == 3 * len(T2)
