"""Properties of the decimation rule itself, on the NumPy restatement (decimate_ref.py; no GPU
needed): what a collapse in rounds must keep (topology, winding, boundaries), where it must stop,
and that the placement guard holds.  The device is compared with the restatement bit for bit in
test_gpu_decimate.py."""
import numpy as np
import pytest

import decimate_ref as R
import meshpost_ref as P


def boundary_positions(V, T):
    """The positions of the boundary vertices as bit patterns, in lexicographic order: a collapse of
    (u, v) with v on the boundary keeps v's position under u's id, so ids and order may change."""
    bits = np.ascontiguousarray(V[np.unique(P.boundary_edges(T))]).view(np.uint64).reshape(-1, 3)
    return bits[np.lexsort((bits[:, 2], bits[:, 1], bits[:, 0]))]


@pytest.mark.parametrize("name,target", (("octahedron", 4), ("octahedron", 6), ("sphere4", 200), ("sphere4", 201),
                                         ("sphere4", 1000), ("bipyramid", 40), ("bipyramid", 101)))
def test_closed_meshes_keep_their_topology(name, target):
    V, T, _ = R.built(name)
    Vo, To, _, rec = R.reference(name, target)
    assert R.euler(To) == R.euler(T) == 2
    assert P.directed_unique(To) and len(P.boundary_edges(To)) == 0
    assert rec["stop"] == "target" and rec["faces_out"] == len(To) and len(To) in (target, target - 1)
    assert rec["faces_in"] == len(T) and rec["collapses"] == (len(T) - len(To)) // 2 == len(V) - len(Vo)


def test_octahedron_ends_as_a_tetrahedron():
    Vo, To, _, rec = R.reference("octahedron", 4)
    assert len(Vo) == 4 and len(To) == 4 and sorted(np.unique(To)) == [0, 1, 2, 3]
    assert sorted(map(tuple, np.sort(To, axis=1))) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]


@pytest.mark.parametrize("name,target", (("trimmed5", 15000), ("lattice", 6000)))
def test_open_meshes_keep_their_boundaries(name, target):
    V, T, _ = R.built(name)
    Vo, To, _, rec = R.reference(name, target)
    assert rec["stop"] == "target" and len(To) in (target, target - 1)
    assert len(P.boundary_edges(To)) == len(P.boundary_edges(T)) > 0
    assert R.euler(To) == R.euler(T) and P.directed_unique(To)
    assert np.array_equal(boundary_positions(V, T), boundary_positions(Vo, To))       # bit-equal: none moved


def test_lattice_counts():
    Vo, To, _, rec = R.reference("lattice", 6000)
    assert len(P.boundary_edges(To)) == 2700 and rec["rounds"] == 6 and len(To) == 6000


@pytest.mark.parametrize("name", ("tetrahedron", "open_strip", "fan", "hexagon", "disc_hole5", "single_triangle"))
def test_nothing_valid(name):
    """The tetrahedron's every common neighbour has valence 3; the others' vertices are all on the
    boundary (the fan's hub is not, but its rim vertices have valence 3)."""
    V, T, D = R.built(name)
    Vo, To, Do, rec = R.reference(name, 2 if name == "tetrahedron" else 0)
    assert rec["stop"] == "no_valid_edge" and rec["rounds"] == 1 and rec["collapses"] == 0 and rec["valid"] == 0
    assert np.array_equal(To, T) and np.array_equal(Vo.view(np.uint64), V.view(np.uint64)) and np.array_equal(Do, D)
    assert sum(rec[k] for k in R.REASONS) == len(P.adjacency(T, len(V))["neighbours"]) // 2


def test_duplicated_triangle_is_never_collapsed_across():
    V, T, _ = R.built("duplicated")
    assert R.reference("duplicated", 0, 1)[3]["nonmanifold"] > 0
    Vo, To, _, rec = R.reference("duplicated", 0)
    assert rec["stop"] == "no_valid_edge" and rec["collapses"] > 0
    rows, counts = np.unique(To, axis=0, return_counts=True)
    assert sorted(counts)[-2:] == [1, 2]                              # the doubled triangle is still there, twice


def test_target_at_or_above_the_count_and_max_rounds():
    V, T, D = R.built("sphere4")
    for target in (len(T), len(T) + 5):
        Vo, To, Do, rec = R.decimate(V, T, target, D=D)
        assert rec["rounds"] == 0 and rec["stop"] == "target" and np.array_equal(To, T) and np.array_equal(Vo, V)
    assert R.reference("sphere4", 200, 0)[3]["stop"] == "max_rounds"
    prev = len(T)
    for rounds in (1, 2, 3):
        rec = R.reference("sphere4", 200, rounds)[3]
        assert rec["stop"] == "max_rounds" and rec["rounds"] == rounds and rec["faces_out"] < prev
        assert rec["selected"] > 100                                 # many collapses per round: the sweeps matter
        prev = rec["faces_out"]
    with pytest.raises(IndexError):
        R.decimate(V, np.concatenate([T, [[0, 1, len(V)]]]), 10)


def test_last_round_applies_a_prefix_of_the_selected():
    rec = R.reference("sphere4", 200)[3]
    need_last = rec["collapses"] - R.reference("sphere4", 200, rec["rounds"] - 1)[3]["collapses"]
    assert 0 < need_last < rec["selected"]


def test_planar_patch_falls_to_the_tie_rules():
    """Every cost is exactly 0 and every det 0: the rank is the key, the placement P[u]."""
    V, T, _ = R.built("planar")
    Q = R.vertex_quadrics(V, T)
    assert not Q[:, [0, 1, 2, 3, 4, 5, 6, 8, 9]].any() and (Q[:, 7] > 0).all()
    Vo, To, _, rec = R.reference("planar", 20)
    assert rec["collapses"] > 0
    have = {tuple(p) for p in V}
    assert all(tuple(p) in have for p in Vo)                         # no vertex moved anywhere new


def test_sphere_radii_stay_within_the_guard():
    """A sanity bound from the input: r in [rmin - w, rmax + w] with w = rmax - rmin about the input's
    centroid.  It catches a placement that escapes the two-edge-lengths guard."""
    V, T, _ = R.built("sphere4")
    Vo = R.reference("sphere4", 200)[0]
    c = V.mean(axis=0)
    r, ro = np.linalg.norm(V - c, axis=1), np.linalg.norm(Vo - c, axis=1)
    w = r.max() - r.min()
    assert r.min() - w <= ro.min() and ro.max() <= r.max() + w


def test_nan_vertex_is_left_alone():
    V, T, _ = R.built("nan_vertex")
    assert R.reference("nan_vertex", 0, 1)[3]["nan"] > 0
    Vo, To, _, rec = R.reference("nan_vertex", 0)
    assert rec["collapses"] > 0 and np.isnan(Vo).any(axis=1).sum() == 1
    nan_id = int(np.flatnonzero(np.isnan(Vo).any(axis=1))[0])
    assert (To == nan_id).any(axis=1).sum() == (T == 24).any(axis=1).sum()      # its fan is untouched


def test_builders():
    V, T = R.bipyramid(80)
    adj = P.adjacency(T, len(V))
    deg = np.diff(adj["offsets"])
    assert len(T) == 160 and deg[0] == deg[1] == 80 and (deg[2:] == 4).all() and R.euler(T) == 2 and P.directed_unique(T)
    counts = {n: (len(R.built(n)[1]), len(P.adjacency(R.built(n)[1], len(R.built(n)[0]))["neighbours"]) // 2)
              for n in ("patch8x16cut", "patch8x16", "patch3x43", "patch7x11", "patch9x9", "patch24x24")}
    assert [counts[n][0] for n in ("patch8x16cut", "patch8x16", "patch3x43")] == [255, 256, 258]
    assert [counts[n][1] for n in ("patch7x11", "patch9x9")] == [249, 261] and counts["patch24x24"] == (1152, 1776)
