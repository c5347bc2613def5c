"""The surface mesher's rule, on the restatement alone (no GPU): what tests/surface_ref.py gives
on clouds whose answer is known in closed form, that the greedy selection and its round form are
one set, and what the geometry of a triple refuses."""
import numpy as np
import pytest

import surface_ref as S


@pytest.fixture(scope="module")
def sphere():
    P, Nrm = S.fibonacci_sphere(400)
    r = S.mean_nn(P)
    return P, Nrm, r, S.ball_pivot(P, Nrm, [r])


def test_sphere_closes_in_one_pass(sphere):
    P, Nrm, r, (T, rec, closed) = sphere
    assert rec == [dict(radius=r, candidates=796, accepted=796, rounds=1)]
    assert len(T) == 2 * len(P) - 4
    assert S.topology(T, len(P)) == (True, 0, 2)             # no edge twice, no boundary edge, Euler characteristic 2
    assert S.agrees_with_normals(P, Nrm, T) and closed.all()
    T3, rec3, _ = S.ball_pivot(P, Nrm, [r, 2 * r, 4 * r])    # every vertex is closed: later passes find nothing
    assert np.array_equal(T3, T) and [p["candidates"] for p in rec3] == [796, 0, 0]


def test_noisy_sphere_closes():
    P, Nrm = S.fibonacci_sphere(600, 0.01, seed=1)
    T, rec, closed = S.ball_pivot(P, Nrm, [S.mean_nn(P)])
    assert len(T) == 1196 and S.topology(T, 600) == (True, 0, 2) and closed.all()


@pytest.mark.parametrize("jitter, candidates, rounds", [(0.0, 484, 2), (0.2, 242, 1)])
def test_lattice(jitter, candidates, rounds):
    """The exact lattice: four cospherical points per square, both diagonals are candidates, the
    selection keeps one; the jittered one has one empty ball per triangle."""
    P, Nrm = S.lattice(12, 12, jitter, seed=2)
    T, rec, _ = S.ball_pivot(P, Nrm, [1.0])
    assert rec == [dict(radius=1.0, candidates=candidates, accepted=242, rounds=rounds)]
    once, boundary, euler = S.topology(T, len(P))
    assert once and boundary == 44 and euler == 1 and S.agrees_with_normals(P, Nrm, T)
    Tr, recr, _ = S.ball_pivot(P, Nrm, [1.0], form="rounds")
    assert np.array_equal(Tr, T) and recr == rec
    Tn, recn, _ = S.ball_pivot(P, -Nrm, [1.0])                # the same triangles, wound the other way
    assert np.array_equal(Tn, T[:, [0, 2, 1]]) and recn == rec


def test_holed_plane_later_passes_only_touch_open_vertices():
    P, Nrm = S.lattice(14, 14, 0.15, seed=3, hole=(5, 5, 4))
    T1, rec1, closed1 = S.ball_pivot(P, Nrm, [1.0])
    T, rec, closed = S.ball_pivot(P, Nrm, [1.0, 2.0])
    assert np.array_equal(T[:len(T1)], T1) and rec[0] == rec1[0] and rec[1]["accepted"] > 0
    later = T[len(T1):]
    assert not closed1[later.reshape(-1)].any()
    assert S.topology(T, len(P))[0] and S.agrees_with_normals(P, Nrm, T)
    taken = set(S.directed_edges(T).tolist())
    assert np.array_equal(closed, S.closed_rule(taken, len(P))) and closed[closed1].all() and closed.sum() > closed1.sum()
    Tr, recr, closedr = S.ball_pivot(P, Nrm, [1.0, 2.0], form="rounds")
    assert np.array_equal(Tr, T) and recr == rec and np.array_equal(closedr, closed)


def test_rounds_equal_greedy_against_taken_edges():
    P, Nrm = S.lattice(12, 12, 0.0)
    tri, rho = S.candidates(P, Nrm, 1.0, np.zeros(len(P), bool))
    assert len(tri) == 484 and (np.diff(rho.astype(np.float64)) >= 0).all()
    taken = set(S.edge_keys(tri[::7]).reshape(-1).tolist())
    acc, rounds = S.select_rounds(tri, taken)
    assert np.array_equal(acc, S.select_greedy(tri, taken)) and rounds >= 1 and not acc[::7].any()
    none, no_round = S.select_rounds(tri[:0], taken)
    assert len(none) == 0 and no_round == 0
    with pytest.raises(RuntimeError, match="rounds"):
        S.select_rounds(tri, set(), max_rounds=1)


def triple(pa, pb, pc, normals, r):
    P = np.array([pa, pb, pc], np.float64)
    Nn = np.array(normals, np.float64)
    ok, sign, rho2, o = S.triple_rule(P[:1], P[1:2], P[2:], Nn[:1], Nn[1:2], Nn[2:], r * r)
    return bool(ok[0]), int(sign[0]), float(rho2[0]), o[0]


def test_triple_rule_refusals():
    up = [[0, 0, 1]] * 3
    ok, sign, rho2, o = triple([0, 0, 0], [1, 0, 0], [0, 1, 0], up, 1.0)
    assert ok and sign == 1 and rho2 == 0.5 and np.allclose(o, [0.5, 0.5, np.sqrt(0.5)])
    ok, sign, _, o = triple([0, 0, 0], [1, 0, 0], [0, 1, 0], [[0, 0, -1]] * 3, 1.0)
    assert ok and sign == -1 and np.allclose(o, [0.5, 0.5, -np.sqrt(0.5)])
    assert not triple([0, 0, 0], [1, 0, 0], [2, 0, 0], up, 4.0)[0]                      # flat
    assert not triple([0, 0, 0], [0, 0, 0], [0, 1, 0], up, 4.0)[0]                      # a duplicate point
    assert not triple([0, 0, 0], [np.nan, 0, 0], [0, 1, 0], up, 4.0)[0]
    assert not triple([0, 0, 0], [1, 0, 0], [0, 1, 0], up, 0.7)[0]                      # h^2 < 0: rho^2 = 0.5 > 0.49
    assert triple([0, 0, 0], [1, 0, 0], [0, 1, 0], up, np.sqrt(0.5) * (1 + 1e-12))[0]
    assert not triple([0, 0, 0], [1, 0, 0], [0, 1, 0], [[0, 0, 1], [0, 0, 1], [0, 0, -1]], 1.0)[0]   # mixed signs
    assert not triple([0, 0, 0], [1, 0, 0], [0, 1, 0], [[0, 0, 1], [0, 0, 1], [1, 0, 0]], 1.0)[0]    # one in the plane
    # through the whole rule: three points give their one triangle, a flat or mixed triple nothing
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    T, rec, _ = S.ball_pivot(P, np.array(up, np.float64), [1.0])
    assert T.tolist() == [[0, 1, 2]] and rec[0]["candidates"] == 1
    assert len(S.ball_pivot(P, np.array([[0, 0, 1], [0, 0, 1], [0, 0, -1]], np.float64), [1.0])[0]) == 0
    assert len(S.ball_pivot(P[:2], np.array(up[:2], np.float64), [1.0])[0]) == 0


def test_square_and_duplicate():
    """Four cospherical points: four candidates, two kept.  A duplicated point: both copies get
    their candidates (each is outside the other's ball by the slack), one triangle per directed edge."""
    P, Nrm = S.lattice(2, 2)
    T, rec, _ = S.ball_pivot(P, Nrm, [1.0])
    assert rec[0]["candidates"] == 4 and rec[0]["accepted"] == 2 and S.topology(T, 4)[0]
    P, Nrm = S.lattice(5, 5, 0.1, seed=4)
    Pd, Nd = np.concatenate([P, P[12:13]]), np.concatenate([Nrm, Nrm[12:13]])
    T, rec, _ = S.ball_pivot(Pd, Nd, [1.0])
    assert rec[0]["candidates"] > rec[0]["accepted"] and S.topology(T, len(Pd))[0] and S.agrees_with_normals(Pd, Nd, T)


def test_refusals_of_the_whole_rule():
    P, Nrm = S.lattice(3, 3)
    for bad in ([], [1.0] * 9, [2.0, 1.0], [1.0, 1.0], [0.0], [np.nan], [np.inf], [-1.0]):
        with pytest.raises(ValueError, match="radii"):
            S.ball_pivot(P, Nrm, bad)
    Pn = P.copy()
    Pn[4, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        S.ball_pivot(Pn, Nrm, [1.0])
    rng = np.random.default_rng(5)                             # CAP + 2 points within 2 r of each other
    Pc = rng.uniform(-0.5, 0.5, (S.CAP + 2, 3)) / np.sqrt(3.0)
    with pytest.raises(ValueError, match="neighbours"):
        S.ball_pivot(Pc, np.tile([0.0, 0.0, 1.0], (len(Pc), 1)), [1.0])
