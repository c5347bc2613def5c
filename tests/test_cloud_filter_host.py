"""Host side of the cloud filters: the NumPy restatement against a plain O(N^2) evaluation, the
PLY reader, and the exceptions of the ProcessingLogic drop-ins (no GPU needed)."""
import re

import numpy as np
import pytest

import cloud_ref as R


def small_cloud(n=400, seed=5):
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, 6.0, (n, 3))
    P[:40] = np.round(P[:40])                 # integer points: exact distances, ties
    P[40:48] = P[0]                           # duplicates
    P[48:52] += 500.0                         # far outliers
    return P


def test_restatement_equals_plain_evaluation():
    P = small_cloud()
    for radius in (2.0, 5.0):
        assert np.array_equal(R.radius_counts(P, radius), R.brute_radius_counts(P, radius))
    for k in (1, 5, 20):
        assert np.array_equal(R.knn_avg(P, k), R.brute_knn_avg(P, k))
    keep, avg, (mean, std, thr) = R.statistical_filter(P, 5, 2.0)
    pos = avg[avg > 0]
    assert mean == pytest.approx(pos.sum() / len(P), rel=1e-13)
    assert std == pytest.approx(np.sqrt(((pos - mean) ** 2).sum() / (len(P) - 1)), rel=1e-13)
    assert np.array_equal(keep, (avg > 0) & (avg < thr)) and not keep[48:52].any()


def test_strict_comparison_and_edges():
    P = np.array([[0, 0, 0], [3, 4, 0], [5, 0, 0], [-5, 0, 0]], float)
    assert R.radius_counts(P, 5.0).tolist() == [1, 2, 2, 1]            # the origin's pairs sit at d2 == r^2
    assert R.radius_counts(P, 5.0 + 1e-9).tolist() == [4, 3, 3, 2]
    keep, avg, (mean, std, thr) = R.statistical_filter(np.zeros((1, 3)), 20, 2.0)
    assert avg.tolist() == [0.0] and np.isnan(thr) and not keep.any()
    keep, avg, _ = R.statistical_filter(np.vstack([np.ones((25, 3)), small_cloud(100)]), 20, 2.0)
    assert np.all(avg[:25] == 0) and not keep[:25].any()


def test_ply_round_trip_is_exact(tmp_path):
    from structured_light_for_3d_model_replication_amd import cloud as CL, ply as PLY
    rng = np.random.default_rng(2)
    P = rng.normal(0, 300.0, (500, 3))
    P[0] = [0.00004, -0.00005, 123456.78905]
    C = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    path = tmp_path / "a.ply"
    try:
        PLY.write_ascii(str(path), P, C)
    except ImportError:                       # the native writer is not built: same bytes from Python
        with open(path, "wb") as f:
            f.write(PLY.header(len(P)))
            for p, c in zip(P, C):
                f.write(f"{p[0]:.4f} {p[1]:.4f} {p[2]:.4f} {c[2]} {c[1]} {c[0]}\n".encode())
    P2, C2 = CL.read_ply(str(path))
    want = np.array([[float(f"{v:.4f}") for v in p] for p in P])
    assert P2.dtype == np.float64 and np.array_equal(P2, want)
    assert C2.dtype == np.uint8 and np.array_equal(C2, C)


def test_ply_reader_refuses_other_layouts(tmp_path):
    from structured_light_for_3d_model_replication_amd import cloud as CL, ply as PLY
    hdr = PLY.header(1).decode()
    cases = {
        "binary.ply": (hdr.replace("format ascii 1.0", "format binary_little_endian 1.0").encode()
                       + np.zeros(3, "<f4").tobytes() + b"\0\0\0", "ascii"),
        "extra.ply": (hdr.replace("end_header", "property float nx\nend_header") + "1 2 3 4 5 6 7\n", "layout"),
        "short.ply": (PLY.header(2).decode() + "1 2 3 4 5 6\n", "2 vertices"),
        "colour.ply": (hdr + "1 2 3 4.5 5 6\n", "integers"),
        "magic.ply": ("solid\n" + hdr, "PLY"),
    }
    for name, (data, why) in cases.items():
        p = tmp_path / name
        p.write_bytes(data if isinstance(data, bytes) else data.encode())
        with pytest.raises(ValueError, match=why):
            CL.read_ply(str(p))


def test_drop_ins_raise_the_reference_exceptions(tmp_path):
    from structured_light_for_3d_model_replication_amd import ply as PLY
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    missing = str(tmp_path / "nope.ply")
    empty = tmp_path / "empty.ply"
    empty.write_bytes(PLY.header(0))
    for fn in (ProcessingLogic.remove_radius_outlier, ProcessingLogic.remove_outliers):
        with pytest.raises(FileNotFoundError, match=re.escape("Input file not found: " + missing)):
            fn(missing)
        with pytest.raises(ValueError, match="Point cloud is empty."):
            fn(str(empty), return_obj=True)
