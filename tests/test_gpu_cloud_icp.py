"""Device point-to-plane ICP, transform, concat and merge_pro_360 (csrc/cloud_icp.hip) against the
NumPy restatement (icp_ref.py).

Base case (icp_ref.base_case): the row_mode 1 smoke cloud (12,532 points, normals at radius 9,
max_nn 30) as the target; every third point, moved by the inverse of a rotation of (1, -1.5, 0.7)
degrees about the centroid plus (1.2, -0.8, 0.9) mm, as the source, 322 of them first pushed 50 mm
away so that they end without a match; d = 6.

Per logged evaluation the device is checked at its own logged T, so no error accumulates over the
iterations: n_corr exact; err2 and the 27 sums within 1e-12 * fsum(|terms|) of math.fsum (the
bound of the fixed tree); x bit-equal to the restated LDL' of the device's sums; the
next T within 1e-13 * max(1, max|T|) of the restated update from that x (three 2x2 rotations
multiplied out: under 100 roundings of entries bounded by 1 plus a few ulps per sin / cos, so under
2.3e-14; the bound leaves 4x); the stop flag equal to the rule on the logged fitness and rmse.

CPU_ERR = 2.6e-13 mm is what the restatement reaches on the base case after 30 iterations
(measured 2.56e-13; test_icp_ref.py asserts it); the device gets 8 times that for its sqrt,
division, sin and cos differing from libm by ulps."""
import ctypes
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_ref as R

pytestmark = pytest.mark.gpu

CPU_ERR = 2.6e-13
TOL = 8 * CPU_ERR


@pytest.fixture(scope="module")
def base():
    b = R.base_case()
    for a in (b["tgt"], b["nrm"], b["src"], b["T_true"], b["moved"]):
        a.setflags(write=False)
    b["tree"] = cKDTree(b["tgt"])
    return b


@pytest.fixture(scope="module")
def CL():
    from structured_light_for_3d_model_replication_amd import cloud
    return cloud


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def far_count(CL):
    import torch
    return CL.far_count(torch.device("cuda", torch.cuda.current_device()))


def pairs_of(corr):
    i = np.flatnonzero(corr >= 0)
    return np.stack([i, corr[i].astype(np.int64)], 1)


def check_evaluation(res_pairs, rec, src, tgt, d, tree=None):
    """One record's evaluation against the restatement at the record's T."""
    T = rec[:16].reshape(4, 4)
    ev = R.evaluate(src, tgt, T, d, tree)
    assert rec[16] == ev["n_corr"]
    assert abs(rec[17] - ev["err2"]) <= 1e-12 * ev["err2"]
    assert rec[18] == ev["n_corr"] / len(src)
    want = math.sqrt(rec[17] / rec[16]) if rec[16] else 0.0
    assert abs(rec[19] - want) <= 4 * np.spacing(want)
    if res_pairs is not None:
        assert np.array_equal(res_pairs, pairs_of(ev["corr"]))
    return ev


def check_log(res, src, tgt, nrm, d, rel=(1e-6, 1e-6), tree=None):
    """Every record of a result's log (see the module docstring)."""
    log = res.log
    assert len(log) == res.iterations + 1 and log.shape[1] == R.LOG_STRIDE
    for k, rec in enumerate(log):
        last = k == len(log) - 1
        flags = int(rec[53])
        ev = check_evaluation(res.correspondence_set.cpu().numpy() if last else None, rec, src, tgt, d, tree)
        stop = k > 0 and R.stop_rule(rec[18], log[k - 1][18], rec[19], log[k - 1][19], *rel)
        assert bool(flags & R.LOG_STOP) == stop
        assert bool(flags & (R.LOG_SOLVED | R.LOG_SINGULAR)) == (not last)
        if last:
            assert stop or flags & R.LOG_LAST
            assert not rec[47:53].any()
            continue
        S_ref, A_ref = R.sums(ev, tgt, nrm) if ev["n_corr"] else (np.zeros(27), np.zeros(27))
        S = rec[20:47]
        print(k, "n_corr", ev["n_corr"], "max sum error / bound", np.max(np.abs(S - S_ref) / np.maximum(1e-12 * A_ref, 1e-300)))
        assert np.all(np.abs(S - S_ref) <= 1e-12 * A_ref)
        x_ref, ok = R.ldlt_solve(S)
        ok = ok and ev["n_corr"] > 0
        assert bool(flags & R.LOG_SOLVED) == ok
        assert np.array_equal(bits(rec[47:53]), bits(x_ref if ok else np.zeros(6)))
        T, T_next = rec[:16].reshape(4, 4), log[k + 1][:16].reshape(4, 4)
        T_ref = R.apply_update(rec[47:53], T) if ok else T
        print(k, "max |T_next - T_ref|", np.abs(T_next - T_ref).max())
        assert np.abs(T_next - T_ref).max() <= 1e-13 * max(1.0, np.abs(T_next).max())
    assert np.array_equal(bits(res.transformation), bits(log[-1][:16].reshape(4, 4)))
    assert res.fitness == log[-1][18] and res.inlier_rmse == log[-1][19]
    assert res.converged == bool(int(log[-1][53]) & R.LOG_STOP)


def cloud_of(CL, P, nrm=None):
    return CL.PointCloud(np.array(P, np.float64), None, normals=None if nrm is None else np.array(nrm, np.float64))


# ------------------------------------------------------------------ the base case
def test_base_log_and_default_criteria(CL, base):
    b = base
    res = CL.registration_icp(cloud_of(CL, b["src"]), cloud_of(CL, b["tgt"], b["nrm"]), b["d"], return_log=True)
    check_log(res, b["src"], b["tgt"], b["nrm"], b["d"], tree=b["tree"])
    ref = R.registration_icp(b["src"], b["tgt"], b["nrm"], b["d"])
    assert (res.iterations, res.converged) == (ref["iterations"], ref["converged"]) == (4, True)
    assert np.array_equal(res.correspondence_set.cpu().numpy(), pairs_of(ref["corr"]))
    assert res.correspondence_set.dtype.is_floating_point is False and len(res.correspondence_set) == int((~b["moved"]).sum())
    assert res.fitness < 1.0                                   # the displaced points have no match


def test_recovered_motion(CL, base):
    """Both criteria 0: exactly 30 iterations on both sides."""
    b = base
    res = CL.registration_icp(cloud_of(CL, b["src"]), cloud_of(CL, b["tgt"], b["nrm"]), b["d"], relative_fitness=0.0,
                              relative_rmse=0.0, return_log=True)
    assert res.iterations == 30 and not res.converged and len(res.log) == 31
    assert int(res.log[-1][53]) == R.LOG_LAST
    err = R.motion_error(res.transformation, b["T_true"], b["src"][~b["moved"]])
    print("motion error", err, "allowed", TOL)
    assert err <= TOL


def test_non_identity_init(CL, base):
    b = base
    init = R.motion_about(b["tgt"].mean(0), (0.6, -1.0, 0.3), (0.5, -0.5, 0.5))
    res = CL.registration_icp(cloud_of(CL, b["src"]), cloud_of(CL, b["tgt"], b["nrm"]), b["d"], init=init, return_log=True)
    assert np.array_equal(bits(res.log[0][:16].reshape(4, 4)), bits(init))
    check_log(res, b["src"], b["tgt"], b["nrm"], b["d"], tree=b["tree"])
    ref = R.registration_icp(b["src"], b["tgt"], b["nrm"], b["d"], init=init)
    assert (res.iterations, res.converged) == (ref["iterations"], ref["converged"])
    assert R.motion_error(res.transformation, b["T_true"], b["src"][~b["moved"]]) <= 1e-9


def test_two_runs_give_the_same_bits(CL, base):
    b = base
    src, tgt = cloud_of(CL, b["src"]), cloud_of(CL, b["tgt"], b["nrm"])
    runs = [CL.registration_icp(src, tgt, b["d"], return_log=True) for _ in range(2)]
    assert np.array_equal(bits(runs[0].transformation), bits(runs[1].transformation))
    assert np.array_equal(bits(runs[0].log), bits(runs[1].log))
    assert np.array_equal(runs[0].correspondence_set.cpu().numpy(), runs[1].correspondence_set.cpu().numpy())
    assert (runs[0].fitness, runs[0].inlier_rmse) == (runs[1].fitness, runs[1].inlier_rmse)


def test_max_iteration_zero_is_evaluate_registration(CL, base):
    b = base
    src, tgt = cloud_of(CL, b["src"]), cloud_of(CL, b["tgt"], b["nrm"])
    init = R.motion_about(b["tgt"].mean(0), (0.9, -1.4, 0.6), (1.0, -1.0, 1.0))
    a = CL.registration_icp(src, tgt, b["d"], init=init, max_iteration=0, return_log=True)
    e = CL.evaluate_registration(src, cloud_of(CL, b["tgt"]), b["d"], init)          # no normals needed
    assert a.iterations == e.iterations == 0 and not a.converged and not e.converged and e.log is None
    assert (a.fitness, a.inlier_rmse) == (e.fitness, e.inlier_rmse) and 0.5 < a.fitness < 1.0
    assert np.array_equal(bits(a.transformation), bits(init)) and np.array_equal(bits(e.transformation), bits(init))
    assert np.array_equal(a.correspondence_set.cpu().numpy(), e.correspondence_set.cpu().numpy())
    assert len(a.log) == 1 and int(a.log[0][53]) == R.LOG_LAST
    check_evaluation(e.correspondence_set.cpu().numpy(), a.log[0], b["src"], b["tgt"], b["d"], b["tree"])


# ------------------------------------------------------------------ crafted cases
def lattice_3d(n):
    g = np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def evaluate_equals_brute(CL, src, tgt, d, T=None):
    res = CL.evaluate_registration(cloud_of(CL, src), cloud_of(CL, tgt), d, T)
    S = R.transform_points(np.eye(4) if T is None else T, src)
    want = np.array([R.brute_correspondence(q, tgt, d)[0] for q in S])
    assert np.array_equal(res.correspondence_set.cpu().numpy(), pairs_of(want))
    return res, want


def test_lowest_index_wins_at_exact_midpoints(CL):
    """Cube centres (8 equidistant targets), face centres (4) and edge midpoints (2) of an integer
    lattice; the same cloud with the target order reversed picks the other end of every tie."""
    tgt = lattice_3d(5)
    cells = lattice_3d(4)
    src = np.vstack([cells + 0.5, cells + [0.5, 0.5, 0.0], cells + [0.0, 0.0, 0.5]])
    res, want = evaluate_equals_brute(CL, src, tgt, 2.0)
    assert res.fitness == 1.0 and np.all(want[:64] == (cells @ [25, 5, 1]).astype(np.int64))
    _, rev = evaluate_equals_brute(CL, src, tgt[::-1].copy(), 2.0)
    assert np.all(len(tgt) - 1 - rev != want)                  # every query had a tie


def test_strict_distance(CL):
    tgt = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])
    src = np.array([[0.0, 0.0, -2.0], [10.0, 1.5, 0.0]])
    res, want = evaluate_equals_brute(CL, src, tgt, 2.0)
    assert want.tolist() == [-1, 1] and res.fitness == 0.5 and res.inlier_rmse == 1.5
    res, want = evaluate_equals_brute(CL, src, tgt, float(np.nextafter(2.0, 3.0)))
    assert want.tolist() == [0, 1] and res.fitness == 1.0


def test_queries_outside_the_target_box(CL, base):
    """Source points beyond each of the six faces of the target's box, 5 mm and 300 mm out (the
    cells are a few mm), with d = 400: the far ones are still open after kMaxRing rings and take
    the whole-target kernel."""
    tgt = base["tgt"]
    lo, hi, mid = tgt.min(0), tgt.max(0), tgt.mean(0)
    src = []
    for a in range(3):
        for out in (5.0, 300.0):
            for side, edge in ((-1.0, lo), (1.0, hi)):
                p = mid.copy()
                p[a] = edge[a] + side * out
                src.append(p)
                q = np.where(np.arange(3) == a, p, edge)       # also beyond a corner of the box
                src.append(q)
    src = np.array(src)
    res, want = evaluate_equals_brute(CL, src, tgt, 400.0)
    assert far_count(CL) > 0 and np.count_nonzero(want >= 0) >= 12 and np.count_nonzero(want < 0) >= 1
    res, want = evaluate_equals_brute(CL, src, tgt, 4.0)       # a small d: the walk ends at the radius
    assert far_count(CL) == 0 and np.all(want < 0)


def test_no_correspondence_at_all(CL, base):
    b = base
    init = R.motion_about([0.0, 0.0, 0.0], (3.0, 2.0, 1.0), (1e4, 0.0, 0.0))
    res = CL.registration_icp(cloud_of(CL, b["src"][:500]), cloud_of(CL, b["tgt"], b["nrm"]), 1.0, init=init, return_log=True)
    assert res.fitness == 0.0 and res.inlier_rmse == 0.0 and len(res.correspondence_set) == 0
    assert np.array_equal(bits(res.transformation), bits(init))
    assert res.converged and res.iterations == 1
    assert int(res.log[0][53]) == R.LOG_SINGULAR and int(res.log[1][53]) == R.LOG_STOP


def test_plane_target_has_a_zero_pivot(CL):
    """z = 0 on an integer lattice with normals (0, 0, 1) and dyadic source coordinates: every
    term is exact, J = (sy, -sx, 0, 0, 0, 1), so the third pivot is exactly zero and the update is
    the identity."""
    g = np.arange(12, dtype=np.float64)
    tgt = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3)
    nrm = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    src = tgt[::2] + [0.25, 0.125, 0.5]
    res = CL.registration_icp(cloud_of(CL, src), cloud_of(CL, tgt, nrm), 1.0, return_log=True)
    check_log(res, src, tgt, nrm, 1.0)
    rec = res.log[0]
    ev = R.evaluate(src, tgt, np.eye(4), 1.0)
    S_ref, _ = R.sums(ev, tgt, nrm)
    assert np.array_equal(rec[20:47], S_ref) and rec[20 + R.ut(2, 2)] == 0.0 and rec[20] > 0 and rec[20 + R.ut(1, 1)] > 0
    assert int(rec[53]) == R.LOG_SINGULAR and not rec[47:53].any()
    assert np.isfinite(res.log).all() and np.array_equal(res.transformation, np.eye(4))
    assert res.converged and res.iterations == 1 and res.fitness == 1.0


@pytest.mark.parametrize("nt", [1, 2, 3])
def test_one_source_point(CL, nt):
    tgt = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0], [40.0, 2.0, 3.0]])[:nt]
    nrm = np.array([[0.0, 0.6, 0.8], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])[:nt]
    src = np.array([[1.3, 2.1, 3.2]])
    res = CL.registration_icp(cloud_of(CL, src), cloud_of(CL, tgt, nrm), 5.0, max_iteration=1, return_log=True)
    rec = res.log[0]
    ev = check_evaluation(None, rec, src, tgt, 5.0)
    assert ev["corr"].tolist() == [0 if nt == 1 else 1]
    S_ref, _ = R.sums(ev, tgt, nrm)
    assert np.array_equal(rec[20:47], S_ref)                   # one term: nothing to round
    x_ref, ok = R.ldlt_solve(rec[20:47])
    assert bool(int(rec[53]) & R.LOG_SOLVED) == ok and np.array_equal(bits(rec[47:53]), bits(x_ref))
    assert res.iterations == 1 and len(res.log) == 2


def test_target_without_normals_and_bad_inputs(CL, base):
    from structured_light_for_3d_model_replication_amd import _native as N
    b = base
    src, tgt = cloud_of(CL, b["src"][:300]), cloud_of(CL, b["tgt"][:2000], b["nrm"][:2000])
    with pytest.raises(ValueError, match="normals"):
        CL.registration_icp(src, cloud_of(CL, b["tgt"][:2000]), 6.0)
    for kw in (dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")),
               dict(max_iteration=-1), dict(relative_fitness=-1.0), dict(relative_rmse=float("nan")),
               dict(init=np.zeros((4, 4))), dict(init=np.eye(3))):
        args = dict(max_correspondence_distance=6.0)
        args.update(kw)
        with pytest.raises(ValueError):
            CL.registration_icp(src, tgt, **args)
    with pytest.raises(N.NativeError):
        CL.registration_icp(src, tgt, 6.0, max_iteration=1001)
    bad = b["src"][:300].copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.registration_icp(cloud_of(CL, bad), tgt, 6.0)
    bad_t = b["tgt"][:2000].copy()
    bad_t[5, 0] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        CL.evaluate_registration(src, cloud_of(CL, bad_t), 6.0)
    res = CL.registration_icp(src, tgt, 6.0, return_log=True)                     # the process goes on
    check_log(res, b["src"][:300], b["tgt"][:2000], b["nrm"][:2000], 6.0)


def test_c_abi_return_codes(CL):
    import torch
    from structured_light_for_3d_model_replication_amd import _native as N
    L = N.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")          # the workspace
    io = torch.zeros(1 << 10, dtype=torch.float64, device="cuda")         # every other buffer: zeros in, scratch out
    p, q = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(io.data_ptr())
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    need = L.slg_icp_ws_bytes(4, 4, 3)
    assert 0 < need <= buf.numel() and L.slg_icp_ws_bytes(4, 4, 30) > need
    assert L.slg_icp_ws_bytes(0, 4, 3) == -N.SLG_ERR_INVALID and L.slg_icp_ws_bytes(4, 0, 3) == -N.SLG_ERR_INVALID
    assert L.slg_icp_ws_bytes(4, 4, -1) == -N.SLG_ERR_INVALID
    assert L.slg_icp_ws_bytes((1 << 30) + 1, 4, 3) == -N.SLG_ERR_UNSUPPORTED
    assert L.slg_icp_ws_bytes(4, (1 << 30) + 1, 3) == -N.SLG_ERR_UNSUPPORTED
    assert L.slg_icp_ws_bytes(4, 4, 1001) == -N.SLG_ERR_UNSUPPORTED

    def icp(src=q, ns=4, tgt=q, nrm=q, nt=4, d=1.0, T=eye, rf=1e-6, rr=1e-6, it=3, ws=p, wsb=need, res=q):
        return L.slg_icp_point_to_plane(src, ns, tgt, nrm, nt, d, T, rf, rr, it, ws, wsb, res, None, None, None)

    nan = float("nan")
    bad_row, bad_nan = np.eye(4), np.eye(4)
    bad_row[3, 3] = 2.0
    bad_nan[0, 1] = nan
    for kw in (dict(ns=0), dict(nt=0), dict(ns=-3), dict(d=0.0), dict(d=-1.0), dict(d=nan), dict(it=-1), dict(rf=-1e-9),
               dict(rr=-1.0), dict(rf=nan), dict(rr=nan), dict(src=None), dict(tgt=None), dict(T=None), dict(res=None),
               dict(ws=None), dict(wsb=need - 1), dict(wsb=-1),
               dict(T=(ctypes.c_double * 16)(*bad_row.reshape(-1))), dict(T=(ctypes.c_double * 16)(*bad_nan.reshape(-1)))):
        assert icp(**kw) == N.SLG_ERR_INVALID, kw
    for kw in (dict(ns=(1 << 30) + 1), dict(nt=(1 << 30) + 1), dict(it=1001)):
        assert icp(**kw) == N.SLG_ERR_UNSUPPORTED, kw

    def tr(xyz=q, nrm=None, n=4, T=eye, out=q, nout=None):
        return L.slg_cloud_transform(xyz, nrm, n, T, out, nout, None)

    for kw in (dict(n=0), dict(xyz=None), dict(out=None), dict(T=None), dict(nrm=q, nout=None),
               dict(T=(ctypes.c_double * 16)(*bad_row.reshape(-1))), dict(T=(ctypes.c_double * 16)(*bad_nan.reshape(-1)))):
        assert tr(**kw) == N.SLG_ERR_INVALID, kw
    assert tr(n=(1 << 30) + 1) == N.SLG_ERR_UNSUPPORTED
    assert icp(nrm=None, it=0) == N.SLG_OK and tr() == N.SLG_OK     # zeros in, nothing faults
    torch.cuda.synchronize()


# ------------------------------------------------------------------ transform and concat
def test_transform_and_concat(CL, base):
    import torch
    b = base
    rng = np.random.default_rng(11)
    C = rng.integers(0, 256, (len(b["tgt"]), 3), dtype=np.uint8)
    T = R.motion_about([10.0, -20.0, 700.0], (25.0, -40.0, 110.0), (3.0, -4.0, 5.5))
    T[:3, :3] *= 1.25                                          # any last-row-0001 matrix, not only rigid ones
    pc = CL.PointCloud(b["tgt"], C, normals=b["nrm"])
    out = CL.transform(pc, T)
    assert np.array_equal(bits(out.xyz.cpu().numpy()), bits(R.transform_points(T, b["tgt"])))
    assert np.array_equal(bits(out.normals.cpu().numpy()), bits(R.transform_normals(T, b["nrm"])))
    assert np.array_equal(out.bgr.cpu().numpy(), C)
    assert np.array_equal(bits(pc.xyz.cpu().numpy()), bits(b["tgt"]))            # the input is left alone
    plain = CL.transform(CL.PointCloud(b["tgt"][:777], C[:777]), T)               # no normals, odd size
    assert plain.normals is None and np.array_equal(bits(plain.xyz.cpu().numpy()), bits(R.transform_points(T, b["tgt"][:777])))
    with pytest.raises(ValueError, match="transformation"):
        CL.transform(pc, np.ones((4, 4)))
    both = CL.concat(pc, out)
    assert len(both) == 2 * len(pc) and both.has_normals()
    assert np.array_equal(bits(both.xyz.cpu().numpy()), bits(R.concat(b["tgt"], R.transform_points(T, b["tgt"]))))
    assert np.array_equal(bits(both.normals.cpu().numpy()), bits(R.concat(b["nrm"], R.transform_normals(T, b["nrm"]))))
    assert np.array_equal(both.bgr.cpu().numpy(), R.concat(C, C))
    mixed = CL.concat(pc, plain)
    assert mixed.normals is None and len(mixed) == len(pc) + 777
    assert np.array_equal(mixed.bgr.cpu().numpy(), R.concat(C, C[:777]))
    assert isinstance(both.xyz, torch.Tensor) and both.xyz.is_cuda


# ------------------------------------------------------------------ merge_pro_360
def test_merge_pro_360(CL, base, tmp_path, capsys):
    """Three files: the base cloud, and the same cloud under the inverses of two known small
    motions (under 2 mm on the points), so step i must find motion i composed with the inverse of
    motion i - 1 and the accumulated transform is motion i.  voxel_size 2.0 is below the cloud's
    smallest spacing, so the down-sample keeps every point; the PLY's 4 decimals quantise the
    points by 5e-5 mm, and the poses are asked to 1e-3 mm on the points."""
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    P = base["tgt"]
    C = np.full((len(P), 3), 128, np.uint8)
    c = P.mean(0)
    motions = [np.eye(4), R.motion_about(c, (0.1, -0.15, 0.08), (0.15, -0.1, 0.12)),
               R.motion_about(c, (-0.12, 0.1, 0.15), (-0.1, 0.15, -0.15))]
    folder = tmp_path / "views"
    folder.mkdir()
    for deg, M in zip((240, 0, 120), (motions[2], motions[0], motions[1])):       # written out of order
        ProcessingLogic._save_ply(R.transform_points(R.inverse_rigid(M), P), C, str(folder / f"obj_{deg}deg_scan.ply"))
    out_path = str(tmp_path / "merged.ply")
    steps = []
    ProcessingLogic.merge_pro_360(str(folder), out_path, voxel_size=2.0, final_voxel=0,
                                  step_callback=lambda i, total, pc: steps.append((i, total, pc)))
    log = capsys.readouterr().out
    assert "[Merge 360] Sorted file order:\n  [0] obj_0deg_scan.ply\n  [1] obj_120deg_scan.ply\n  [2] obj_240deg_scan.ply" in log
    assert f"  Loaded: obj_120deg_scan.ply ({len(P)} points)" in log
    assert "[Merge 360] Loaded 3 clouds. Running Sequential Registration (2 steps)..." in log
    assert "\n[Merge 360] === Step 2/2: Aligning Scan 2 -> Scan 1 ===" in log
    assert f"  Preprocessed: source={len(P)} pts, target={len(P)} pts (voxel=2.0)" in log
    assert log.count("  [RANSAC] skipped: initial transform given") == 2 and log.count("  [ICP]    Fitness: 1.0000 | RMSE: 0.000") == 2
    assert "[WARNING]" not in log
    assert f"  [Merge 360] Step 2/2 complete. Accumulated cloud: {3 * len(P)} points total." in log
    assert "\n[Merge 360] All 2 steps complete. Running post-processing..." in log
    assert "[Merge 360] Post-processing (Final Voxel: 0, Outlier removal)..." in log
    assert f"[Merge 360] Saved merged cloud to {out_path}" in log
    assert [(i, total, len(pc)) for i, total, pc in steps] == [(1, 2, 2 * len(P)), (2, 2, 3 * len(P))]
    merged = steps[-1][2].xyz.cpu().numpy()
    for i in (1, 2):
        err = np.linalg.norm(merged[i * len(P):(i + 1) * len(P)] - P, axis=1).max()
        print("step", i, "pose error on the points", err)
        assert err <= 1e-3
    Pm, Cm, Nm = CL.read_ply(out_path, normals=True)
    assert Nm is not None and len(Pm) == len(Nm) > 2 * len(P) and np.abs(np.linalg.norm(Nm, axis=1) - 1).max() <= 2e-6
    seq = []
    ProcessingLogic.merge_pro_360(str(folder), str(tmp_path / "m2.ply"), voxel_size=2.0, final_voxel=0,
                                  init_transforms=[np.linalg.inv(motions[0]) @ motions[1], np.linalg.inv(motions[1]) @ motions[2]],
                                  step_callback=lambda i, total, pc: seq.append(pc))
    assert np.abs(seq[-1].xyz.cpu().numpy()[2 * len(P):] - P).max() <= 1e-3
    called = []
    ProcessingLogic.merge_pro_360(str(folder), str(tmp_path / "m3.ply"), voxel_size=2.0, final_voxel=0,
                                  init_transforms=lambda i, s, t: (called.append((i, len(s), t.has_normals())), np.eye(4))[1])
    assert called == [(1, len(P), True), (2, len(P), True)]
