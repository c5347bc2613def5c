"""Device seeded RANSAC plane segmentation (csrc/cloud_plane.hip, cloud.py) against the NumPy
restatement (plane_ref.py), on the base case of plane_ref.py (the smoke cloud plus a planted wall,
threshold 1.5) and on small clouds at the chunk edges.

Device records equal the restatement's bits for the trial, the valid flag, a b c d, count, err,
fitness and rmse: every rule is the same sequence of IEEE operations on both sides, err included
(its order is part of the rule).  The result, the winner and K equal the restated sequential scan
over the device's own records; the final inliers equal the restatement's exactly; each of the nine
refit sums lies within 1e-12 * fsum(|terms|) of math.fsum (the fixed tree's bound),
and the returned plane equals, bit for bit, the restated formula on the device's own nine sums.
"""
import math

import numpy as np
import pytest

import plane_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def CL():
    from structured_light_for_3d_model_replication_amd import cloud
    return cloud


@pytest.fixture(scope="module")
def base():
    return R.base_case()


@pytest.fixture(scope="module")
def dev(CL, base):
    return CL.PointCloud(np.array(base["P"]), np.array(base["C"]))


@pytest.fixture(scope="module")
def run0(CL, dev, base):
    return CL.segment_plane(dev, base["thr"], 3, base["num_iterations"], seed=0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def assert_records(got, want):
    assert got.shape == want.shape
    for col, name in enumerate(("trial", "valid", "a", "b", "c", "d", "count", "err", "fitness", "rmse")):
        bad = np.flatnonzero(bits(got[:, col]) != bits(want[:, col]))
        assert bad.size == 0, (name, bad[:5], got[bad[:5], col], want[bad[:5], col])
    assert not got[:, 10:].any()


def small_cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-40.0, 40.0, (n, 3))
    P[: n // 2, 2] = 0.25 * P[: n // 2, 0] + rng.uniform(-0.4, 0.4, n // 2)
    return np.ascontiguousarray(P)


def check_refit(CL, P, seg, thr):
    """The inliers, the nine sums and the returned plane of a finished segmentation."""
    idx = seg.inliers.cpu().numpy()
    assert np.array_equal(idx, R.inliers(P, seg.sample_plane, thr)) and (np.diff(idx) > 0).all()
    m = len(idx)
    assert seg.sums[12] == m
    Q = P[idx]
    cen_dev = seg.sums[9:12]
    assert np.array_equal(bits(cen_dev), bits(seg.sums[:3] / float(m)))
    terms = np.concatenate([Q, R.centred_terms(Q, cen_dev)], 1)          # the centred products about the device's own centroid
    for k in range(9):
        exact, scale = math.fsum(terms[:, k]), math.fsum(np.abs(terms[:, k]))
        assert abs(seg.sums[k] - exact) <= 1e-12 * scale, (k, seg.sums[k], exact, scale)
    assert np.array_equal(bits(seg.plane_model), bits(R.plane_from_nine(seg.sums[:9], m)))


# ------------------------------------------------------------------ records
def test_first_batch_records(CL, dev, base):
    got = CL.plane_batch(dev, base["thr"], 0, CL.PLANE_BATCH, 3, 0)
    assert_records(got, R.records(base["P"], 0, 0, CL.PLANE_BATCH, 3, base["thr"]))
    assert got[:, 1].all() and (got[:, 8] > 0.4).sum() >= 2


@pytest.mark.parametrize("t0,count", [(256, 1), (300, 63), (977, 65), (512, 257)])
def test_partial_batches(CL, dev, base, t0, count):
    """A later batch of 1, 63, 65 and PLANE_BATCH + 1 trials (the last: two workgroup columns)."""
    assert count != 257 or count == CL.PLANE_BATCH + 1
    got = CL.plane_batch(dev, base["thr"], t0, count, 3, 0)
    assert_records(got, R.records(base["P"], 0, t0, count, 3, base["thr"]))


def test_num_iterations_not_a_multiple_of_the_batch(CL, dev, base):
    """probability = 1 bounds nothing: 300 trials are a full batch and one of 44."""
    seg = CL.segment_plane(dev, base["thr"], 3, 300, probability=1.0, seed=0)
    assert seg.iterations == 300 and len(seg.log) == 300
    assert_records(seg.log, R.records(base["P"], 0, 0, 300, 3, base["thr"]))
    assert int(seg.log[R.scan(list(seg.log), 300, 1.0, 3)[0], 0]) == seg.trial == R.segment(base["P"], base["thr"], 3, 300, 1.0)["trial"]


@pytest.mark.parametrize("ransac_n", [4, 8])
def test_ransac_n(CL, dev, base, ransac_n):
    got = CL.plane_batch(dev, base["thr"], 0, 128, ransac_n, 9)
    want = R.records(base["P"], 9, 0, 128, ransac_n, base["thr"])
    assert_records(got, want)
    assert want[:, 1].sum() > 100


def test_ransac_n_9_is_unsupported(CL, dev, base):
    from structured_light_for_3d_model_replication_amd import _native as N
    with pytest.raises(N.NativeError) as e:
        CL.segment_plane(dev, base["thr"], ransac_n=9)
    assert e.value.code == N.SLG_ERR_UNSUPPORTED
    with pytest.raises(N.NativeError) as e:
        CL.plane_batch(dev, base["thr"], 0, 64, 9, 0)
    assert e.value.code == N.SLG_ERR_UNSUPPORTED


@pytest.mark.parametrize("n", [3, 64, 2047, 2048, 2049, 4097])
def test_chunk_edges(CL, n):
    P = small_cloud(n)
    pc = CL.PointCloud(P)
    for rn in (3, 4):
        if n < rn:
            continue
        got = CL.plane_batch(pc, 0.75, 0, 96, rn, 2)
        assert_records(got, R.records(P, 2, 0, 96, rn, 0.75))
    seg = CL.segment_plane(pc, 0.75, 3, 200, seed=2)
    want = R.segment(P, 0.75, 3, 200, seed=2)
    assert (seg.trial, seg.iterations) == (want["trial"], want["K"]) and seg.trial >= 0
    check_refit(CL, P, seg, 0.75)


def test_a_point_at_the_threshold_is_no_inlier(CL):
    """Plane z = 0, threshold 0.5: z = 0.5 is out (strict), z = 0.25 is in; all values exact in binary."""
    g = np.arange(8.0)
    X, Y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), np.zeros(64)], 1)
    P = np.concatenate([P, [[1.0, 1.0, 0.5], [2.0, 3.0, -0.5], [3.0, 2.0, 0.25], [4.0, 4.0, -0.25]]])
    pc = CL.PointCloud(P)
    idx, sums, plane = CL.plane_finish(pc, [0.0, 0.0, 1.0, 0.0], 0.5)
    assert idx.cpu().tolist() == list(range(64)) + [66, 67] and sums[12] == 66
    recs = CL.plane_batch(pc, 0.5, 0, 64, 3, 0)
    assert_records(recs, R.records(P, 0, 0, 64, 3, 0.5))
    flat = recs[(recs[:, 1] == 1.0) & (np.abs(recs[:, 4]) == 1.0) & (recs[:, 5] == 0.0)]      # trials that drew the plane z = 0
    assert len(flat) and (flat[:, 6] == 66).all() and (flat[:, 7] == 0.5).all()


def test_duplicate_points(CL):
    P = np.repeat(small_cloud(20), 100, axis=0)
    pc = CL.PointCloud(P)
    got = CL.plane_batch(pc, 0.75, 0, 128, 3, 1)
    want = R.records(P, 1, 0, 128, 3, 0.75)
    assert_records(got, want)
    assert (want[:, 1] == 0.0).any()                     # distinct draws of coincident points: a zero norm


def test_all_points_coplanar(CL):
    rng = np.random.default_rng(5)
    P = np.concatenate([rng.integers(-64, 64, (3000, 2)).astype(np.float64), np.full((3000, 1), 8.0)], 1)
    seg = CL.segment_plane(CL.PointCloud(P), 0.5, 3, 1000, seed=0)
    first = int(np.flatnonzero(seg.log[:, 1])[0])
    assert seg.fitness == 1.0 and seg.trial == first and seg.iterations == first + 1 < CL.PLANE_BATCH
    assert len(seg.log) == first + 1                     # the loop ended after one batch
    assert len(seg.inliers) == 3000 and abs(abs(seg.plane_model[2]) - 1.0) < 1e-12
    assert abs(seg.plane_model[3] + 8.0 * seg.plane_model[2]) < 1e-9


def test_all_points_collinear(CL):
    t = np.arange(500.0)
    P = np.stack([t, 2.0 * t, -0.5 * t], 1)              # exact products: every triangle's cross product is zero
    pc = CL.PointCloud(P, np.full((500, 3), 7, np.uint8))
    seg = CL.segment_plane(pc, 0.5, 3, 300, seed=0)
    assert seg.trial == -1 and seg.iterations == 300 and not seg.plane_model.any() and len(seg.inliers) == 0
    assert len(seg.log) == 300 and not seg.log[:, 1:].any()
    out, _ = CL.remove_plane(pc, 0.5, 3, 300)
    assert out is pc
    zero = CL.segment_plane(pc, 0.5, 3, 0)
    assert zero.trial == -1 and zero.iterations == 0 and len(zero.log) == 0 and len(zero.inliers) == 0


# ------------------------------------------------------------------ the whole segmentation
def test_result_equals_the_scan_of_the_device_records(CL, base, run0):
    want = R.base_segment(0)
    pos, K = R.scan(list(run0.log), base["num_iterations"], R.PROBABILITY, 3)
    assert (int(run0.log[pos, 0]), K) == (run0.trial, run0.iterations) == (want["trial"], want["K"])
    assert len(run0.log) == K and np.array_equal(run0.log[:, 0], np.arange(K))
    assert_records(run0.log, np.stack(want["records"]))
    assert np.array_equal(bits(run0.sample_plane), bits(want["plane"]))
    assert (run0.fitness, run0.inlier_rmse) == (want["fitness"], want["rmse"])
    plane_model, inliers = run0
    assert plane_model is run0.plane_model and inliers is run0.inliers and plane_model.shape == (4,)


def test_final_inliers_and_refit(CL, base, run0):
    import torch
    assert run0.inliers.dtype == torch.int64 and run0.inliers.is_cuda
    assert np.array_equal(run0.inliers.cpu().numpy(), R.base_segment(0)["inliers"])
    assert np.array_equal(run0.inliers.cpu().numpy(), np.flatnonzero(base["wall"]))
    check_refit(CL, base["P"], run0, base["thr"])


def test_same_call_same_bits_and_another_seed(CL, dev, base, run0):
    again = CL.segment_plane(dev, base["thr"], 3, base["num_iterations"], seed=0)
    assert np.array_equal(bits(again.log), bits(run0.log)) and np.array_equal(bits(again.plane_model), bits(run0.plane_model))
    assert np.array_equal(bits(again.sums), bits(run0.sums)) and again.inliers.equal(run0.inliers)
    other = CL.segment_plane(dev, base["thr"], 3, base["num_iterations"], seed=5)
    assert other.trial != run0.trial and other.trial == R.base_segment(5)["trial"] and other.inliers.equal(run0.inliers)


def test_nan_sets_the_status_word(CL, base):
    P = np.array(base["P"][:5000])
    P[4321, 1] = np.nan
    pc = CL.PointCloud(P)
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.segment_plane(pc, base["thr"])
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.plane_finish(pc, [0.0, 0.0, 1.0, -800.0], 5.0)
    P[4321, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.plane_batch(CL.PointCloud(P), base["thr"], 0, 64)


# ------------------------------------------------------------------ remove_background
def test_remove_background(CL, dev, base, tmp_path, capsys):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    P, C, wall = base["P"], base["C"], base["wall"]
    n, m = len(P), int((~wall).sum())
    out = ProcessingLogic.remove_background(dev, distance_threshold=base["thr"], return_obj=True)
    assert isinstance(out, CL.PointCloud) and out.xyz.is_cuda
    oP, oC = out.numpy()
    assert np.array_equal(oP, P[~wall]) and np.array_equal(oC, C[~wall])
    assert capsys.readouterr().out == f"[BG Remove] Processing...\n[BG Remove] Original: {n}, Remaining: {m} pts\n"
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    ProcessingLogic._save_ply(P, C, src)
    fP, fC = CL.read_ply(src)                            # what the file holds (positions as %.4f)
    assert ProcessingLogic.remove_background(src, dst, distance_threshold=base["thr"]) is None
    assert capsys.readouterr().out == (f"[BG Remove] Processing...\n[BG Remove] Original: {n}, Remaining: {m} pts\n"
                                       f"[BG Remove] Saved to {dst}\n")
    want = str(tmp_path / "want.ply")
    ProcessingLogic._save_ply(fP[~wall], fC[~wall], want)
    assert open(dst, "rb").read() == open(want, "rb").read()
    rP, rC = CL.read_ply(dst)
    assert np.array_equal(rP, fP[~wall]) and np.array_equal(rC, fC[~wall])
    # normals, when present, follow the points
    nrm = np.ascontiguousarray(np.arange(3.0 * n).reshape(n, 3))
    with_n = ProcessingLogic.remove_background(CL.PointCloud(dev.xyz, dev.bgr, normals=nrm), distance_threshold=base["thr"],
                                               return_obj=True, seed=5)
    assert np.array_equal(with_n.normals.cpu().numpy(), nrm[~wall]) and np.array_equal(with_n.numpy()[0], P[~wall])


def test_cleanup_chain_stays_on_the_device(CL, dev, base):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    a = ProcessingLogic.remove_background(dev, distance_threshold=base["thr"], return_obj=True)
    b = ProcessingLogic.keep_largest_cluster(a, eps=10.0, min_points=16, return_obj=True)
    c = ProcessingLogic.remove_radius_outlier(b, nb_points=16, radius=10.0, return_obj=True)
    for pc in (a, b, c):
        assert isinstance(pc, CL.PointCloud) and pc.xyz.is_cuda and pc.bgr.is_cuda
    assert len(a) == 12532 and 0 < len(c) <= len(b) <= len(a)
    want_b = CL.largest_cluster(CL.PointCloud(np.array(base["P"][~base["wall"]]), np.array(base["C"][~base["wall"]])), 10.0, 16)
    assert np.array_equal(b.numpy()[0], want_b.numpy()[0])
