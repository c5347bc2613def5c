"""Input clouds of the DBSCAN tests (test helper): the base table and the crafted cases, shared by
``test_cluster_ref.py`` (CPU) and ``test_gpu_cloud_cluster.py``."""
import numpy as np

# (row_mode, eps, min_points) -> points, clusters, (largest label, size) or None where the table
# leaves it open, noise, contested border points.  Computed on the CPU with both restatements of
# cluster_ref.py on the smoke view (test_gpu_cloud_filter.oracle_cloud((192, 128), 25.0, 1, rm)).
BASE = {
    (1, 10.0, 16): (12532, 5, (0, 4570), 120, 0),
    (1, 8.0, 12): (12532, 2, (1, 4294), 6398, 0),
    (1, 5.0, 200): (12532, 0, (-1, 0), 12532, 0),          # the reference's defaults: all noise
    (2, 10.0, 16): (25064, 5, (2, 8837), 5656, 0),
    (2, 6.0, 20): (25064, 7, (None, 5918), 19034, 30),
    (2, 4.0, 12): (25064, 84, None, 22695, 261),
}


def blob(centre, arm_dx):
    """12 points inside a cube of side 0.1 and one arm point 0.9 along x: at eps 1 all 13 are
    mutual neighbours."""
    rng = np.random.default_rng(3)
    c = np.asarray(centre, np.float64)
    return np.vstack([c + rng.uniform(-0.05, 0.05, (12, 3)), c + [arm_dx, 0.0, 0.0]])


BRIDGE_EPS, BRIDGE_MIN = 1.0, 5


def bridge(first):
    """Two blobs whose arms reach towards each other, and one point 0.9 from either arm and 1.8
    from everything else: 3 neighbours, so not core at min_points 5, and within eps of a core
    point of each cluster.  The blob at the larger x holds the lower indices, so the smallest
    index and the smallest sorted position belong to different clusters.  Returns (P, index of
    the bridge point); ``first`` puts it at index 0 (Open3D marks it noise first), else last."""
    hi, lo = blob([10.0, 0.0, 0.0], -0.9), blob([6.4, 0.0, 0.0], 0.9)
    b = np.array([[8.2, 0.0, 0.0]])
    return (np.vstack([b, hi, lo]), 0) if first else (np.vstack([hi, lo, b]), 26)


def tie():
    """Two congruent blobs of 20 points, 50 apart; the one at the larger x comes first."""
    rng = np.random.default_rng(4)
    a = rng.uniform(-0.15, 0.15, (20, 3))
    return np.vstack([a + [50.0, 0.0, 0.0], a])


def lattice5():
    g = np.arange(0, 25, 5, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def decimal_lattice():
    """The cloud of test_gpu_cloud_filter.test_decimal_lattice."""
    g = 0.3 + 0.1 * np.arange(12)
    return np.stack(np.meshgrid(g, g - 7.7, g + 1e3, indexing="ij"), -1).reshape(-1, 3)


HELIX_EPS, HELIX_MIN = 1.0, 3


def helix(n=20000, drop=None, seed=7):
    """``n`` points along a helix (radius 20, 3.14 between turns) at arc spacing 0.6 eps: every
    point's neighbours are itself and the next one either way.  ``drop`` removes one position of
    the chain; the index order is then shuffled with a fixed seed."""
    s = 0.6 * HELIX_EPS * np.arange(n)
    t = s / np.sqrt(20.0 ** 2 + 0.5 ** 2)
    P = np.stack([20.0 * np.cos(t), 20.0 * np.sin(t), 0.5 * t], 1)
    if drop is not None:
        P = np.delete(P, drop, 0)
    return P[np.random.default_rng(seed).permutation(len(P))]
