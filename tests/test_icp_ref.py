"""The NumPy restatement of the point-to-plane ICP (icp_ref.py) on its own (no GPU needed): the
restated LDL' against np.linalg.solve, the loop on the base case of test_gpu_cloud_icp.py, and
the margins that test relies on.

CPU_ERR is what the restatement reaches on the base case after exactly 30 iterations (both
criteria 0): max_i |T_est p_i - T_true p_i| over the undisplaced source points, measured as
2.56e-13 mm.  test_gpu_cloud_icp.py gives the device 8 times that; asserting it here keeps the
margin from eroding unseen."""
import numpy as np
import pytest

import icp_ref as R

CPU_ERR = 2.6e-13


@pytest.fixture(scope="module")
def base():
    b = R.base_case()
    for a in (b["tgt"], b["nrm"], b["src"], b["T_true"], b["moved"]):
        a.setflags(write=False)
    b["default"] = R.registration_icp(b["src"], b["tgt"], b["nrm"], b["d"])
    return b


def test_base_case_is_what_the_gpu_test_describes(base):
    assert len(base["tgt"]) == 12532 and len(base["src"]) == 4178
    assert 300 <= int(base["moved"].sum()) <= 400
    log = base["default"]["log"]
    # the displaced points end without a match, every other point with one
    assert base["default"]["n_corr"] == int((~base["moved"]).sum())
    assert np.array_equal(base["default"]["corr"] >= 0, ~base["moved"])
    assert 0.55 <= log[0]["fitness"] <= 0.65
    err = [R.motion_error(l["T"], base["T_true"], base["src"][~base["moved"]]) for l in log]
    print("motion error per evaluation", err, "rmse", [l["rmse"] for l in log])
    assert 10.0 < err[0] < 20.0 and all(b < a for a, b in zip(err, err[1:]))


def test_ldlt_agrees_with_linalg_solve(base):
    """Relative residual 1e-9 on the base case's systems (condition number about 1e7)."""
    n = 0
    for rec in base["default"]["log"]:
        if rec["S"] is None:
            continue
        A, b = R.full_system(rec["S"])
        x, ok = R.ldlt_solve(rec["S"])
        want = np.linalg.solve(A, -b)
        cond = np.linalg.cond(A)
        print("cond", cond, "residual", np.linalg.norm(A @ x + b) / np.linalg.norm(b))
        assert ok and np.array_equal(x, rec["x"]) and 1e6 < cond < 1e8
        assert np.linalg.norm(A @ x + b) <= 1e-9 * np.linalg.norm(b)
        assert np.linalg.norm(x - want) <= 1e-9 * np.linalg.norm(want)
        n += 1
    assert n == 4


def test_ldlt_refuses_bad_pivots():
    S = np.zeros(27)
    for a, v in enumerate((4.0, 3.0, 0.0, 2.0, 1.0, 5.0)):        # the third pivot is exactly zero
        S[R.ut(a, a)] = v
    S[21:] = 1.0
    x, ok = R.ldlt_solve(S)
    assert not ok and not x.any()
    S[R.ut(2, 2)] = -1.0
    assert not R.ldlt_solve(S)[1]
    S[R.ut(2, 2)] = np.nan
    assert not R.ldlt_solve(S)[1]
    S[R.ut(2, 2)] = 2.0
    x, ok = R.ldlt_solve(S)
    assert ok and np.array_equal(x, [-0.25, -1.0 / 3.0, -0.5, -0.5, -1.0, -0.2])


def test_loop_recovers_the_base_motion(base):
    r = base["default"]
    assert r["converged"] and r["iterations"] == 4            # it stops at the fifth evaluation
    ok = ~base["moved"]
    assert R.motion_error(r["T"], base["T_true"], base["src"][ok]) <= 1e-11
    r30 = R.registration_icp(base["src"], base["tgt"], base["nrm"], base["d"], relative_fitness=0.0, relative_rmse=0.0)
    assert r30["iterations"] == 30 and not r30["converged"] and len(r30["log"]) == 31
    err = R.motion_error(r30["T"], base["T_true"], base["src"][ok])
    print("CPU_ERR measured", err)
    assert err <= CPU_ERR


def test_stop_decisions_are_far_from_the_thresholds(base):
    """Every |difference| the stop test looks at lies a factor 100 or more away from 1e-6, so the
    device's last-bit differences in fitness and rmse cannot change a decision."""
    log = base["default"]["log"]
    for a, b in zip(log, log[1:]):
        for key in ("fitness", "rmse"):
            diff = abs(b[key] - a[key])
            print(key, diff)
            assert diff >= 1e-4 or diff <= 1e-8
    assert abs(log[-1]["rmse"] - log[-2]["rmse"]) <= 1e-8 < 1e-4 <= abs(log[-2]["rmse"] - log[-3]["rmse"])


def test_correspondence_rules():
    """Strict radius, lowest index among equals, and the brute-force fallback for long ties."""
    g = np.arange(4, dtype=np.float64)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    Q = np.array([[0.5, 0.5, 0.5], [1.5, 1.0, 2.0], [0.0, 0.0, -2.0], [0.0, 0.0, np.nextafter(-2.0, 0.0)]])
    corr, dd = R.correspondences(Q, tgt, 2.0)
    assert corr.tolist() == [0, 22, -1, 0] and dd[0] == 0.75 and dd[1] == 0.25 and np.isinf(dd[2])
    same = np.zeros((40, 3))                                   # 40 equal candidates: more than the tree proposes
    corr, _ = R.correspondences(np.array([[0.1, 0.0, 0.0]]), same, 1.0)
    assert corr.tolist() == [0]
    for q in Q:
        j, v = R.brute_correspondence(q, tgt, 2.0)
        c, d = R.correspondences(q[None, :], tgt, 2.0)
        assert c[0] == j and (d[0] == v or (np.isinf(v) and np.isinf(d[0])))


def test_transform_and_update_rules():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 0.3, 6)
    U = R.update_matrix(x)
    assert np.abs(U[:3, :3] @ U[:3, :3].T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(U[:3, :3]) - 1) <= 1e-15
    T = R.motion_about([1.0, 2.0, 3.0], (10.0, 20.0, -30.0), (4.0, 5.0, 6.0))
    assert np.abs(R.apply_update(x, T) - U @ T).max() <= 1e-14 and R.matrix_ok(R.apply_update(x, T))
    P = rng.normal(0, 50.0, (100, 3))
    assert np.abs(R.transform_points(T, P) - (P @ T[:3, :3].T + T[:3, 3])).max() <= 1e-12
    assert np.abs(R.transform_points(R.inverse_rigid(T), R.transform_points(T, P)) - P).max() <= 1e-12
    assert np.abs(R.transform_normals(T, P) - P @ T[:3, :3].T).max() <= 1e-12
    assert not R.matrix_ok(np.full((4, 4), np.nan)) and not R.matrix_ok(np.ones((4, 4))) and R.matrix_ok(np.eye(4))
