"""The NumPy restatement (normals_ref.py) against independent formulations, the PLY layout with
normals, and argument validation.  No GPU."""
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

import normals_ref as NR
from test_gpu_cloud_normals import CPU_EXCESS, MAX_NN, RADIUS, TOL, lattice_3d, lattice_z7, plane_111


@pytest.fixture(scope="module")
def clouds():
    out = {}
    for rm in (1, 2):
        P, C = NR.smoke_cloud(rm)
        out[rm] = (P, C, NR.neighbour_lists(P, max(MAX_NN) + 1, workers=min(8, os.cpu_count() or 1)))
    return out


@pytest.fixture(scope="module")
def CL():
    from structured_light_for_3d_model_replication_amd import cloud
    return cloud


@pytest.mark.parametrize("vs", [10.0, 100.0])
@pytest.mark.parametrize("rm", [1, 2])
def test_voxel_means_against_reduceat(clouds, rm, vs):
    P, C, _ = clouds[rm]
    pts, col, first, count = NR.voxel_down_sample(P, C, vs)
    ijk = np.floor((P - (P.min(0) - vs / 2)) / vs).astype(np.int64)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
    s = ijk[order]
    start = np.concatenate([[0], np.flatnonzero(np.any(s[1:] != s[:-1], axis=1)) + 1])
    cnt = np.diff(np.concatenate([start, [len(P)]]))
    mean = np.add.reduceat(P[order], start, axis=0) / cnt[:, None]
    fst = np.minimum.reduceat(order, start)
    o = np.argsort(fst)
    assert np.array_equal(first, fst[o]) and np.array_equal(count, cnt[o])
    assert np.allclose(pts, mean[o], rtol=1e-12, atol=0)
    cmean = np.add.reduceat(C[order].astype(np.float64), start, axis=0) / cnt[:, None]
    assert np.array_equal(col, np.floor(cmean[o] + 0.5).astype(np.uint8))
    assert np.all(np.diff(first) > 0) and count.sum() == len(P)


@pytest.mark.parametrize("max_nn", MAX_NN)
@pytest.mark.parametrize("rm", [1, 2])
def test_neighbour_sets_against_ckdtree(clouds, rm, max_nn):
    """Wherever no tie exists at the cut (and no distance within 1e-9 of the radius), the hybrid
    search's set is the tree's."""
    P, _, (idx, dd) = clouds[rm]
    nidx, inside, m = NR.hybrid_neighbours(idx, dd, RADIUS, max_nn)
    d, j = cKDTree(P).query(P, k=max_nn, distance_upper_bound=RADIUS)
    clear = (dd[:, max_nn - 1] < dd[:, max_nn]) & (np.abs(np.sqrt(dd[:, :max_nn + 1]) - RADIUS) > 1e-9 * RADIUS).all(1)
    assert clear.mean() > 0.9
    assert np.array_equal(np.isfinite(d).sum(1)[clear], m[clear])
    got = np.where(inside, nidx, len(P))
    assert np.array_equal(np.sort(got[clear], axis=1), np.sort(j[clear], axis=1))


def test_solver_excess_on_the_base_clouds(clouds):
    """The restated Jacobi solver against np.linalg.eigh: the figure TOL is derived from."""
    worst = 0.0
    for rm in (1, 2):
        P, _, lists = clouds[rm]
        for max_nn in MAX_NN:
            cov, m, nrm = NR.estimate_normals(P, RADIUS, max_nn, lists)
            ok = (m >= 3) & cov.any(1)
            assert np.abs(np.linalg.norm(nrm[ok], axis=1) - 1).max() <= 1e-15
            assert np.array_equal(nrm[~ok], np.tile([0.0, 0.0, 1.0], (int((~ok).sum()), 1)))
            worst = max(worst, NR.rayleigh_excess(cov[ok], nrm[ok]).max())
    print("largest excess of the restated solver over eigh:", worst)
    assert worst <= CPU_EXCESS and TOL == 8 * CPU_EXCESS


def test_crafted_clouds_on_the_restatement():
    cov, m, nrm = NR.estimate_normals(lattice_z7(), 1.5, 30)
    assert not cov[:, [2, 4, 5]].any() and np.abs(nrm - [0, 0, 1]).max() <= 1e-12
    cov, m, nrm = NR.estimate_normals(plane_111(), 2.0, 30)
    assert np.abs(nrm @ (np.ones(3) / np.sqrt(3.0))).min() >= 1 - 1e-12
    assert NR.rayleigh_excess(cov, nrm).max() <= CPU_EXCESS
    P = lattice_3d(6)
    cov, m, nrm = NR.estimate_normals(P, 2.0, 64)
    assert m.max() == 27 and m.min() == 8                  # d2 == 4 exactly is outside
    assert np.array_equal(NR.sign_rule(nrm), nrm)
    assert NR.sign_rule(np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 1.0, -1.0]])).tolist() == \
        [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [-1.0, -1.0, 1.0]]


def test_orient_and_centroid_restatement():
    P = np.array([[0.0, 0, 0], [1.0, 1, 1], [2.0, 0, 0]])
    nrm = np.array([[0.0, 0, 1], [0.0, 0, 1], [1.0, 0, 0]])
    assert NR.orient(P, nrm, [5.0, 0, 0]).tolist() == [[0, 0, 1], [-0.0, -0.0, -1], [1, 0, 0]]
    assert NR.orient(P, nrm, [5.0, 0, 0], outward=True)[2].tolist() == [-1, -0.0, -0.0]
    assert np.array_equal(NR.centroid(P), [1.0, 1 / 3, 1 / 3])


# ------------------------------------------------------------------ PLY with normals
def test_ply_with_normals(CL, clouds, tmp_path):
    P, C, _ = clouds[1]
    P, C = P[:500], C[:500]
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=(500, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[0] = [0.0, -0.0, 1.0]
    path = str(tmp_path / "n.ply")
    CL.write_ply_normals(path, P, C, nrm)
    data = open(path, "rb").read()
    assert data == NR.ply_bytes(P, C, nrm)
    from structured_light_for_3d_model_replication_amd import ply as PLY
    head = PLY.header(500).decode().split("\n")
    assert data.decode().split("\n")[:13] == head[:6] + ["property float nx", "property float ny",
                                                         "property float nz"] + head[6:10]
    Pr, Cr, Nr = CL.read_ply(path, normals=True)
    assert np.array_equal(Pr, np.array([[float("%.4f" % v) for v in row] for row in P]))
    assert np.array_equal(Nr, np.array([[float("%.6f" % v) for v in row] for row in nrm]))
    assert np.array_equal(Cr, C)
    assert len(CL.read_ply(path)) == 2 and np.array_equal(CL.read_ply(path)[0], Pr)


def test_old_layout_is_unchanged(CL, clouds, tmp_path):
    from structured_light_for_3d_model_replication_amd import ply as PLY
    P, C, _ = clouds[1]
    P, C = P[:500], C[:500]
    path = str(tmp_path / "o.ply")
    PLY.write_ascii(path, P, C)
    assert open(path, "rb").read() == NR.ply_bytes(P, C)
    Pr, Cr = CL.read_ply(path)
    assert np.array_equal(Pr, np.array([[float("%.4f" % v) for v in row] for row in P])) and np.array_equal(Cr, C)
    Pn, Cn, Nn = CL.read_ply(path, normals=True)
    assert Nn is None and np.array_equal(Pn, Pr)


def test_malformed_normals_header(CL, tmp_path):
    good = NR.ply_bytes(np.zeros((1, 3)), np.zeros((1, 3), np.uint8), np.array([[0.0, 0.0, 1.0]]))
    for old, new in ((b"property float nz\n", b""), (b"property float ny", b"property double ny"),
                     (b"property float nx\nproperty float ny", b"property float ny\nproperty float nx")):
        path = str(tmp_path / "bad.ply")
        with open(path, "wb") as f:
            f.write(good.replace(old, new))
        with pytest.raises(ValueError, match="vertex layout must be exactly") as e:
            CL.read_ply(path, normals=True)
        assert "nx" in str(e.value) and "got [" in str(e.value)
    path = str(tmp_path / "short.ply")
    with open(path, "wb") as f:
        f.write(good.replace(b"0.000000 0.000000 1.000000 ", b"0.000000 1.000000 "))
    with pytest.raises(ValueError, match="9 values"):
        CL.read_ply(path)


# ------------------------------------------------------------------ arguments
def test_uniform_down_sample_and_validation(CL):
    P = np.arange(30, dtype=np.float64).reshape(10, 3)
    C = np.arange(30, dtype=np.uint8).reshape(10, 3)
    assert np.array_equal(NR.uniform_down_sample(P, C, 3)[0], P[[0, 3, 6, 9]])
    with pytest.raises(ValueError):
        NR.uniform_down_sample(P, C, 0)
    empty = CL.PointCloud(np.zeros((0, 3)))
    assert not empty.has_normals() and empty.normals is None
    for k in (0, -2):
        with pytest.raises(ValueError, match="every_k"):
            CL.uniform_down_sample(empty, k)
    assert len(CL.uniform_down_sample(empty, 2)) == 0
    for fn, args in ((CL.voxel_down_sample, (1.0,)), (CL.estimate_normals, (1.0, 30)), (CL.centroid, ())):
        with pytest.raises(ValueError, match="empty"):
            fn(empty, *args)
    with pytest.raises(ValueError, match="no normals"):
        CL.orient_normals_towards(empty, [0, 0, 0])
    with pytest.raises(ValueError):
        NR.voxel_down_sample(P, C, 0.0)
    with pytest.raises(ValueError):
        NR.voxel_down_sample(np.array([[0.0, 0, 0], [2.2, 0, 0]]), np.zeros((2, 3), np.uint8), 1e-6)
    with pytest.raises(ValueError, match="differ in length"):
        CL.PointCloud(np.zeros((0, 3)), None, normals=np.zeros((2, 3)))
