"""Device tangent-plane normal orientation (csrc/cloud_orient.hip, cloud.py) against the NumPy
restatement (orient_ref.py): neighbour lists, the Euclidean minimum spanning tree, the Riemannian
tree, the root and the output normals.  Every comparison is exact: index lists and edge sets as
integers, distances and normals bit for bit.  Both edge orders are total, so the trees are unique
and the device's Boruvka rounds must give the edge sets of the restatement's Kruskal; the signs are
the restatement's literal traversal against the device's parities.

The shapes are the smallest at which each part can go wrong: sizes around the 64-point list blocks
and the 256-thread kernels, k above n, k = 1 (the EMST alone), a lattice where everything ties, a
path of depth n (hook chains), blobs further apart than the ring limit (the far list and the
largest component sitting out), duplicates (d2 = 0) and an exactly orthogonal pair.  The brute-force
restatement stays at or below about 4,000 points; the smoke cloud uses the Delaunay candidates.
"""
import functools

import numpy as np
import pytest

import orient_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 257, 2000)
KS = (1, 2, 5, 30, 100)


@pytest.fixture(scope="module")
def CL():
    from structured_light_for_3d_model_replication_amd import cloud
    return cloud


@pytest.fixture(scope="module")
def NAT():
    from structured_light_for_3d_model_replication_amd import _native
    return _native


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def random_ref(n):
    """The random cloud of n points with its lists at k = 100 and its EMST (shared, read-only)."""
    P, Nrm = R.random_cloud(n, seed=100 + n)
    idx, dd = R.neighbour_lists(P, max(KS))
    return frozen(P, Nrm, idx, dd, R.emst_brute(P))


def check_against_ref(CL, P, Nrm, k, idx=None, dd=None, emst=None):
    """One device orientation and the lists of the same k against the restatement; returns the
    device's stats."""
    n = len(P)
    kk = min(k, n)
    if idx is None:
        idx, dd = R.neighbour_lists(P, k)
    idx, dd = idx[:, :kk], dd[:, :kk]
    if emst is None:
        emst = R.emst_brute(P)
    tree = R.riemannian_mst(Nrm, idx, emst)
    want, root = R.propagate(P, Nrm, tree)
    pc = CL.PointCloud(np.array(P), normals=np.array(Nrm))
    gi, gd = CL.knn_lists_raw(pc, k)
    assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(bits(gd.cpu().numpy()), bits(dd))
    si, sd = CL.knn_lists(pc, k)
    wi, wd = R.drop_self(idx, dd)
    assert si.shape == (n, kk - 1) and np.array_equal(si.cpu().numpy(), wi) and np.array_equal(bits(sd.cpu().numpy()), bits(wd))
    out, gtree, groot, info = CL.orient_normals_consistent_tangent_plane(pc, k, return_tree=True)
    assert np.array_equal(info["emst"].cpu().numpy(), emst)
    assert np.array_equal(gtree.cpu().numpy(), tree)
    assert groot == root
    assert out.xyz.data_ptr() == pc.xyz.data_ptr() and out.bgr.data_ptr() == pc.bgr.data_ptr()      # shared, not copied
    assert np.array_equal(bits(out.normals.cpu().numpy()), bits(want))
    assert np.array_equal(bits(pc.normals.cpu().numpy()), bits(Nrm))        # the input is left alone
    return info["stats"]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_random_cloud(CL, NAT, n, k):
    P, Nrm, idx, dd, emst = random_ref(n)
    stats = check_against_ref(CL, P, Nrm, k, idx, dd, emst)
    bound = 0 if n < 2 else int(np.ceil(np.log2(n))) + 1
    assert stats[NAT.ORIENT_STAT_EMST_ROUNDS] <= bound and stats[NAT.ORIENT_STAT_TREE_ROUNDS] <= bound
    assert (n < 2) == (stats[NAT.ORIENT_STAT_EMST_ROUNDS] == 0)


@pytest.mark.parametrize("n", SIZES)
def test_euclidean_mst_alone(CL, n):
    P, _, _, _, emst = random_ref(n)
    pc = CL.PointCloud(np.array(P))
    got = CL.euclidean_mst(pc)
    assert got.dtype.is_floating_point is False and got.shape == (n - 1, 2)
    assert np.array_equal(got.cpu().numpy(), emst)
    for list_k in (1, 3):                            # the tree does not depend on the lists it starts from
        assert np.array_equal(CL.euclidean_mst(pc, list_k=list_k).cpu().numpy(), emst)


@pytest.mark.parametrize("k", (7, 30))
def test_lattice_where_everything_ties(CL, k):
    g = np.arange(8.0)
    P = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    Nrm = np.tile([[0.0, 0.6, 0.8]], (len(P), 1))
    check_against_ref(CL, P, Nrm, k)


def test_path_of_depth_n(CL, NAT):
    n = 4096
    x = np.cumsum(1.0 + 0.001 * np.arange(n))        # strictly growing spacing: each point's nearest is the one before
    P = np.ascontiguousarray(np.stack((x, np.zeros(n), np.zeros(n)), axis=1))
    _, Nrm = R.random_cloud(n, seed=8)
    emst = np.stack((np.arange(n - 1), np.arange(1, n)), axis=1)          # the path, read off the spacing
    stats = check_against_ref(CL, P, Nrm, 5, emst=emst)
    assert stats[NAT.ORIENT_STAT_EMST_ROUNDS] == 1   # one round: the chain 4095 -> ... -> 1 -> 0 and one flatten


def far_blobs():
    rng = np.random.default_rng(17)
    # the kNN grid's cell comes out at a few thousand units here (the box spans 1.6e5 and the cell is
    # refined twice from the occupancy), so gaps of 5e4 and more lie beyond its six rings
    blobs = [rng.normal(size=(300, 3)), rng.normal(size=(300, 3)) + [60000.0, 0.0, 0.0],
             rng.normal(size=(20, 3)) + [0.0, 50000.0, 3000.0]]
    lone = np.array([[9e4, 0, 0], [0, -8e4, 10], [-7e4, 6e4, 0], [100.0, 100.0, 9e4], [-5e4, -5e4, -5e4]])
    P = np.ascontiguousarray(np.concatenate(blobs + [lone]))
    return P, R.random_cloud(len(P), seed=3)[1]


def test_blobs_beyond_the_ring_limit(CL, NAT):
    P, Nrm = far_blobs()
    stats = check_against_ref(CL, P, Nrm, 30)
    print("lists far", stats[NAT.ORIENT_STAT_LIST_FAR], "walked", stats[NAT.ORIENT_STAT_WALKED], "far",
          stats[NAT.ORIENT_STAT_FAR], "sat out", stats[NAT.ORIENT_STAT_SAT_OUT])
    assert stats[NAT.ORIENT_STAT_WALKED] > 0 and stats[NAT.ORIENT_STAT_FAR] > 0     # the far path ran
    assert stats[NAT.ORIENT_STAT_SAT_OUT] > 0                                       # and the largest component sat out
    per_round = stats[NAT.ORIENT_STAT_ROUND_FAR:NAT.ORIENT_STAT_ROUND_FAR + 32]
    assert per_round.sum() == stats[NAT.ORIENT_STAT_FAR]
    check_against_ref(CL, P, Nrm, 1)


@pytest.mark.parametrize("k", (1, 2, 5))
def test_every_point_twice(CL, k):
    Q, Nq = R.random_cloud(200, seed=12)
    P = np.ascontiguousarray(np.concatenate((Q, Q)))
    Nrm = np.ascontiguousarray(np.concatenate((Nq, R.random_cloud(200, seed=13)[1])))
    idx, dd = R.neighbour_lists(P, 2)
    assert (idx[200:, 0] == np.arange(200)).all() and (dd[:, :2] == 0).all()     # self is not first in its own list
    check_against_ref(CL, P, Nrm, k)


@pytest.mark.parametrize("k", (1, 3))
def test_orthogonal_tree_neighbours(CL, k):
    P = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -0.5]])
    Nrm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    pc = CL.PointCloud(P, normals=Nrm)
    out, tree, root, _ = CL.orient_normals_consistent_tangent_plane(pc, k, return_tree=True)
    assert root == 0 and tree.tolist() == [[0, 1], [1, 2]]
    assert np.array_equal(out.normals.cpu().numpy(), [[0, 0, 1], [1, 0, 0], [1, 0, 0]])      # sgn(0) = +1
    check_against_ref(CL, P, Nrm, k)
    check_against_ref(CL, P, Nrm * [[-1.0], [1.0], [1.0]], k)


def test_sphere_comes_out_outward(CL):
    P, signed, outward = R.sphere_case(2000, seed=6)
    assert outward[R.root_of(P), 2] > 0
    for k in (1, 12):
        out = CL.orient_normals_consistent_tangent_plane(CL.PointCloud(P, normals=signed), k)
        assert np.array_equal(bits(out.normals.cpu().numpy()), bits(outward))


def test_invariant_under_negating_inputs_and_repeatable(CL):
    P, Nrm, _, _, _ = random_ref(2000)
    assert Nrm[R.root_of(P), 2] != 0
    base, tree, root, _ = CL.orient_normals_consistent_tangent_plane(CL.PointCloud(np.array(P), normals=np.array(Nrm)), 30,
                                                                    return_tree=True)
    base = base.normals.cpu().numpy()
    rng = np.random.default_rng(2)
    for _ in range(2):
        flip = rng.random(len(P)) < 0.5
        N2 = np.array(Nrm)
        N2[flip] = -N2[flip]
        for _ in range(2):                           # twice: the same bits
            got, tree2, root2, _ = CL.orient_normals_consistent_tangent_plane(CL.PointCloud(np.array(P), normals=N2), 30,
                                                                             return_tree=True)
            assert root2 == root and np.array_equal(tree2.cpu().numpy(), tree.cpu().numpy())
            assert np.array_equal(bits(got.normals.cpu().numpy()), bits(base))


@pytest.fixture(scope="module")
def smoke(CL):
    import normals_ref as NR
    P, C = NR.smoke_cloud(1)
    return CL.estimate_normals(CL.PointCloud(P, C), 9.0, 30)


def test_smoke_cloud(CL, smoke):
    n = len(smoke)
    assert n == 12532
    P = smoke.numpy()[0]
    Nrm = smoke.normals.cpu().numpy()
    base, tree, root, info = CL.orient_normals_consistent_tangent_plane(smoke, 30, return_tree=True)
    flip = np.random.default_rng(30).random(n) < 0.5
    N2 = Nrm.copy()
    N2[flip] = -N2[flip]
    got, tree2, root2, info2 = CL.orient_normals_consistent_tangent_plane(CL.PointCloud(smoke.xyz, smoke.bgr, normals=N2), 30,
                                                                         return_tree=True)
    assert np.array_equal(bits(got.normals.cpu().numpy()), bits(base.normals.cpu().numpy()))
    assert root2 == root == R.root_of(P) and np.array_equal(tree2.cpu().numpy(), tree.cpu().numpy())
    emst = R.emst_delaunay(P)
    assert np.array_equal(info["emst"].cpu().numpy(), emst) and np.array_equal(info2["emst"].cpu().numpy(), emst)
    assert np.array_equal(CL.euclidean_mst(smoke).cpu().numpy(), emst)
    # the signs along the device's tree, by the literal traversal
    want, _ = R.propagate(P, Nrm, tree.cpu().numpy())
    assert np.array_equal(bits(base.normals.cpu().numpy()), bits(want))
    assert np.array_equal(np.abs(base.normals.cpu().numpy()), np.abs(Nrm))


def test_status_word(CL):
    P, Nrm, _, _, _ = random_ref(257)
    bad = np.array(P)
    bad[100, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.orient_normals_consistent_tangent_plane(CL.PointCloud(bad, normals=np.array(Nrm)), 5)
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.knn_lists(CL.PointCloud(bad), 5)
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.euclidean_mst(CL.PointCloud(bad))
    badn = np.array(Nrm)
    badn[7, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.orient_normals_consistent_tangent_plane(CL.PointCloud(np.array(P), normals=badn), 5)
    with pytest.raises(RuntimeError, match="no normals"):
        CL.orient_normals_consistent_tangent_plane(CL.PointCloud(np.array(P)), 5)


@pytest.mark.parametrize("n", (1, 2, 65, 2000))
def test_nearest_neighbor_distance(CL, n):
    P, _, idx, dd, _ = random_ref(n)
    got = CL.nearest_neighbor_distance(CL.PointCloud(np.array(P))).cpu().numpy()
    want = np.zeros(n) if n < 2 else np.sqrt(R.drop_self(idx[:, :2], dd[:, :2])[1][:, 0])
    assert got.shape == (n,) and np.array_equal(bits(got), bits(want))


def test_estimate_oriented_normals_tangent(CL, smoke, tmp_path, capsys):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    raw = CL.PointCloud(smoke.xyz, smoke.bgr)
    dst = str(tmp_path / "normals.ply")
    out = ProcessingLogic.estimate_oriented_normals(raw, dst, normal_radius=9.0, normal_max_nn=30, return_obj=True,
                                                    orientation_mode="tangent", tangent_k=30)
    log = capsys.readouterr().out
    assert "[360 Mesh] Re-orienting normals (Mode: tangent)..." in log
    assert "[360 Mesh] Consistent tangent plane orientation applied." in log and "Warning" not in log
    want = CL.orient_normals_consistent_tangent_plane(smoke, 30)
    assert np.array_equal(bits(out.normals.cpu().numpy()), bits(want.normals.cpu().numpy()))
    Pr, Cr, Nr = CL.read_ply(dst, normals=True)
    assert np.abs(Nr - want.normals.cpu().numpy()).max() <= 0.5e-6 + 1e-12 and np.array_equal(Cr, out.numpy()[1])
    assert np.abs(Pr - out.numpy()[0]).max() <= 0.5e-4 + 1e-9
    # the consistency pass after either mode (k <= 0 means 30)
    radial = ProcessingLogic.estimate_oriented_normals(raw, normal_radius=9.0, return_obj=True)
    both = ProcessingLogic.estimate_oriented_normals(raw, normal_radius=9.0, return_obj=True, consistency_pass=True,
                                                     consistency_k=0)
    log = capsys.readouterr().out
    assert "(Mode: radial)" in log and "[Recon] Consistency pass: orient_normals_consistent_tangent_plane(k=30)..." in log
    assert "[Recon] Consistency pass applied." in log
    want = CL.orient_normals_consistent_tangent_plane(radial, 30)
    assert np.array_equal(bits(both.normals.cpu().numpy()), bits(want.normals.cpu().numpy()))
    both = ProcessingLogic.estimate_oriented_normals(raw, normal_radius=9.0, return_obj=True, orientation_mode="tangent",
                                                     tangent_k=30, consistency_pass=True, consistency_k=12)
    want = CL.orient_normals_consistent_tangent_plane(CL.orient_normals_consistent_tangent_plane(smoke, 30), 12)
    assert np.array_equal(bits(both.normals.cpu().numpy()), bits(want.normals.cpu().numpy()))
    # an orientation that raises falls back to radial, with the reference's warning
    import unittest.mock as mock
    with mock.patch.object(CL, "orient_normals_consistent_tangent_plane", side_effect=RuntimeError("boom")):
        fell = ProcessingLogic.estimate_oriented_normals(raw, normal_radius=9.0, return_obj=True, orientation_mode="tangent")
    assert "[360 Mesh] Warning: Tangent plane failed (boom). Fallback to radial." in capsys.readouterr().out
    assert np.array_equal(bits(fell.normals.cpu().numpy()), bits(radial.normals.cpu().numpy()))
