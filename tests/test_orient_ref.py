"""The NumPy restatement of the tangent-plane orientation (orient_ref.py) against independent
checks, without a GPU: scipy's minimum spanning tree, the sphere whose answer is known, the
invariance under negating input normals, the sgn(0) rule and the Delaunay candidates."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import minimum_spanning_tree

import orient_ref as R
from cloud_ref import d2


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_emst_weight_equals_scipy():
    P, _ = R.random_cloud(300, seed=11)
    tree = R.emst_brute(P)
    assert tree.shape == (299, 2) and (tree[:, 0] < tree[:, 1]).all()
    a, b = np.triu_indices(len(P), 1)
    G = coo_matrix((np.sqrt(d2(P[a], P[b])), (a, b)), shape=(len(P), len(P)))
    want = minimum_spanning_tree(G).sum()
    got = np.sqrt(d2(P[tree[:, 0]], P[tree[:, 1]])).sum()
    assert abs(got - want) <= 1e-9 * want


def test_lists_are_sorted_and_start_with_the_point():
    P, _ = R.random_cloud(200, seed=2)
    idx, dd = R.neighbour_lists(P, 7)
    assert idx.shape == (200, 7) and (idx[:, 0] == np.arange(200)).all() and (dd[:, 0] == 0).all()
    assert (np.diff(dd, axis=1) >= 0).all()
    i2, d2_ = R.drop_self(idx, dd)
    assert i2.shape == (200, 6) and np.array_equal(i2, idx[:, 1:]) and np.array_equal(d2_, dd[:, 1:])
    idx, _ = R.neighbour_lists(P[:3], 100)           # k > n
    assert idx.shape == (3, 3)


def test_sphere_comes_out_outward():
    P, signed, outward = R.sphere_case(600, seed=4)
    assert outward[R.root_of(P), 2] > 0
    for k in (1, 8):
        got, tree, root, _, _ = R.orient(P, signed, k)
        assert root == R.root_of(P) and tree.shape == (599, 2)
        assert np.array_equal(bits(got), bits(outward))


def test_invariant_under_negating_inputs():
    P, Nrm = R.random_cloud(400, seed=9)
    assert Nrm[R.root_of(P), 2] != 0
    base, tree, _, _, _ = R.orient(P, Nrm, 6)
    rng = np.random.default_rng(1)
    for _ in range(3):
        flip = rng.random(len(P)) < 0.5
        N2 = Nrm.copy()
        N2[flip] = -Nrm[flip]
        got, tree2, _, _, _ = R.orient(P, N2, 6)
        assert np.array_equal(tree, tree2)
        assert np.array_equal(bits(got), bits(base))


def orthogonal_pair():
    """Three points on a line; the middle normal is exactly orthogonal to the top one's."""
    P = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -0.5]])
    Nrm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    return P, Nrm


def test_sign_of_zero_is_plus():
    P, Nrm = orthogonal_pair()
    got, tree, root, _, _ = R.orient(P, Nrm, 1)
    assert root == 0 and tree.tolist() == [[0, 1], [1, 2]]
    assert R.edge_sign(Nrm, 0, 1) == 1 and R.edge_weight(Nrm, 0, 1) == 1.0
    assert np.array_equal(got, [[0, 0, 1], [1, 0, 0], [1, 0, 0]])       # 1 kept (dot = 0), 2 negated
    # the root's input negated: its sign is -1 and crosses the zero edge as it is (sgn(0) = +1),
    # whatever the direction a traversal would take the edge in
    got, _, _, _, _ = R.orient(P, Nrm * [[-1.0], [1.0], [1.0]], 1)
    assert np.array_equal(got, [[0, 0, 1], [-1, 0, 0], [-1, 0, 0]])


def test_delaunay_candidates_give_the_same_tree():
    P, _ = R.random_cloud(500, seed=21)
    assert np.array_equal(R.emst_delaunay(P), R.emst_brute(P))
