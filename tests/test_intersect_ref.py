"""The restatement of the self-intersection rule (tests/intersect_ref.py) against independent facts:
exact rational arithmetic on integer soups, hand cases, the closed sphere and two overlapping
spheres, and the candidate set against the loop over all pairs.  No GPU."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import audit_ref as A
import intersect_ref as I

SOUP_SEEDS = (1, 2, 3, 4)


# ------------------------------------------------------------------ exact arithmetic
class ExactSign:
    """What intersect_ref.Sign is, from the exact determinant: certain means not zero."""

    def __init__(self, a, b, c, d):
        det = []
        for k in range(len(a)):
            p = [[Fraction(float(x[k, j])) - Fraction(float(d[k, j])) for j in range(3)] for x in (a, b, c)]
            det.append(p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) + p[1][0] * (p[2][1] * p[0][2] - p[2][2] * p[0][1])
                       + p[2][0] * (p[0][1] * p[1][2] - p[0][2] * p[1][1]))
        self.pos = np.array([x > 0 for x in det], bool)
        self.neg = np.array([x < 0 for x in det], bool)
        self.certain = self.pos | self.neg


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    V, T = I.soup(seed)
    return V, T, I.self_intersections(V, T)


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_soup_against_exact_arithmetic(seed):
    """With exact signs "certain" means "not zero", so the exact run's INTERSECTING bit is the exact
    proper-piercing verdict and its UNCERTAIN bit says that a zero determinant decides the pair."""
    V, T, ref = soup_case(seed)
    cand = I.candidates(V, T)
    shared, fp = I.pair_verdicts(V, T, cand)
    shared_x, exact = I.pair_verdicts(V, T, cand, sign=ExactSign)
    assert np.array_equal(shared, shared_x)
    tested = shared <= 1
    decided = tested & ((fp & I.UNCERTAIN) == 0)
    assert np.array_equal(fp[decided] & I.INTERSECTING, exact[decided] & I.INTERSECTING)
    needs_zero = tested & ((exact & I.UNCERTAIN) != 0)
    assert ((fp[needs_zero] & I.UNCERTAIN) != 0).all()
    # integer coordinates of this size make every fp64 operation exact: the two runs agree altogether
    assert np.array_equal(fp, exact)
    assert ref["tested_pairs"] == int(tested.sum()) and ref["adjacent_pairs"] == int((~tested).sum())
    assert ref["intersecting_pairs"] >= 1 and ref["uncertain_pairs"] >= 1 and ref["adjacent_pairs"] >= 1
    assert int((tested & (fp == 0)).sum()) >= 1                                   # excluded pairs
    assert int((shared == 1).sum()) >= 1 and int((shared == 0).sum()) >= 1
    assert A.is_degenerate(T).any() and not ref["triangle_class"][A.is_degenerate(T)].any()
    assert not ref["intersection_free"]


def test_the_bound_is_one_constant():
    E = 2.0 ** -53
    assert I.B == (7.0 + 56.0 * E) * E and float.hex(I.B) == I.B_HEX


# ------------------------------------------------------------------ hand cases
def counts(V, T):
    r = I.self_intersections(V, T)
    return r, {k: r[k] for k in I.COUNTS}


def test_hand_cases():
    r, c = counts(*I.hand("pierced"))
    assert c == dict(candidate_pairs=1, adjacent_pairs=0, tested_pairs=1, intersecting_pairs=1, uncertain_pairs=0,
                     intersecting_triangles=2, uncertain_triangles=0)
    assert r["pairs"].tolist() == [[0, 1]] and r["pairs"].dtype == np.int32 and r["uncertain"].shape == (0, 2)
    assert r["triangle_class"].tolist() == [1, 1] and not r["intersection_free"]
    r, c = counts(*I.hand("lifted"))
    assert c["intersecting_pairs"] == 0 and c["uncertain_pairs"] == 0 and r["intersection_free"]
    r, c = counts(*I.hand("shared_vertex"))
    assert c["candidate_pairs"] == 1 and c["tested_pairs"] == 1 and c["intersecting_pairs"] == 1 and c["uncertain_pairs"] == 0
    V, T = I.hand("shared_vertex")
    for ra in range(3):                             # wherever the shared index stands in either triangle
        for rb in range(3):
            T2 = np.stack([np.roll(T[0], ra), np.roll(T[1], rb)])
            assert counts(V, T2)[1] == c, (ra, rb)
    r, c = counts(*I.hand("flat_grid"))
    assert c["intersecting_pairs"] == 0 and c["adjacent_pairs"] > 0 and c["tested_pairs"] > 0
    assert c["uncertain_pairs"] > 0                 # coplanar neighbours: zeros, never signs
    r, c = counts(*I.hand("edge_sharing"))
    assert c == dict(candidate_pairs=1, adjacent_pairs=1, tested_pairs=0, intersecting_pairs=0, uncertain_pairs=0,
                     intersecting_triangles=0, uncertain_triangles=0) and r["intersection_free"]


def test_what_takes_no_part():
    V, T = I.hand("pierced")
    assert counts(V, np.concatenate([T, [[3, 3, 4]]]))[1] == counts(V, T)[1]
    V2 = V.copy()
    V2[5, 0] = np.nan
    assert counts(V2, T)[1]["candidate_pairs"] == 0
    assert counts(np.zeros((0, 3)), np.zeros((0, 3), np.int32))[1]["candidate_pairs"] == 0
    assert counts(V, T[:1])[1]["candidate_pairs"] == 0
    with pytest.raises(IndexError):
        I.self_intersections(V, [[0, 1, 6]])


# ------------------------------------------------------------------ spheres
def test_sphere_and_two_spheres():
    V, T = A.BUILDERS["sphere5"]()
    r, c = counts(V, T)
    assert c["intersecting_pairs"] == 0 and c["adjacent_pairs"] >= 3 * len(T) // 2 and c["tested_pairs"] > 0
    V2, T2 = I.two_spheres()
    r, c = counts(V2, T2)
    n = len(T)
    assert len(T2) == 2 * n and c["intersecting_pairs"] > 0
    assert (r["pairs"][:, 0] < n).all() and (r["pairs"][:, 1] >= n).all()          # only across the two components
    hit = (r["triangle_class"] & I.INTERSECTING) != 0
    assert hit[:n].any() and hit[n:].any() and c["intersecting_triangles"] == int(hit.sum())
    assert sorted(map(tuple, r["pairs"].tolist())) == list(map(tuple, r["pairs"].tolist()))


# ------------------------------------------------------------------ candidates
def test_candidates_equal_the_quadratic_loop():
    g = np.random.default_rng(300)
    c = g.random((300, 1, 3)) * 4.0
    V = (c + (g.random((300, 3, 3)) - 0.5) * g.choice([0.2, 0.8, 3.0], size=(300, 1, 1))).reshape(-1, 3)
    T = np.arange(900, dtype=np.int32).reshape(300, 3)
    T[7, 2] = T[7, 0]                               # a degenerate one
    V[3 * 11, 1] = np.inf                           # and one that is not finite
    fast, slow = I.candidates(V, T), I.candidates_quadratic(V, T)
    assert len(slow) > 300 and np.array_equal(fast, slow)
    assert not ((fast == 7) | (fast == 11)).any()
    Vt = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [2, 0, 0], [1, 1, 0]], np.float64)     # boxes that touch: closed
    assert I.candidates(Vt, [[0, 1, 2], [3, 4, 5]]).tolist() == [[0, 1]]
