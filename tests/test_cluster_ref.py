"""Open3D's DBSCAN loop, restated literally, equals the closed form the device computes: the
labels are a pure function of the input.  No GPU needed."""
import numpy as np
import pytest

import cluster_cases as K
import cluster_ref as CR


def both(graph, min_points):
    seq, closed = CR.sequential_labels(graph, min_points), CR.closed_labels(graph, min_points)
    assert np.array_equal(seq, closed)
    return closed


@pytest.fixture(scope="module")
def clouds():
    from test_gpu_cloud_filter import oracle_cloud
    return {rm: oracle_cloud((192, 128), 25.0, 1, rm)[0][0] for rm in (1, 2)}


@pytest.mark.parametrize("case", sorted(K.BASE))
def test_base_table(clouds, case):
    rm, eps, mp = case
    points, clusters, big, noise, contested = K.BASE[case]
    g = CR.neighbour_graph(clouds[rm], eps)
    labels = both(g, mp)
    n_clusters, label, count, n_noise = CR.info(labels)
    assert (len(labels), n_clusters, n_noise) == (points, clusters, noise)
    if big is not None:
        assert count == big[1] and big[0] in (None, label)
    assert CR.contested(g, mp, labels) == contested


def test_blocked_form_equals_closed_form(clouds):
    """The memory-lean form tools/cloud_filter_bench.py runs on a 1080p view, in small blocks."""
    for rm, eps, mp in ((1, 10.0, 16), (2, 6.0, 20), (2, 4.0, 12), (1, 5.0, 200)):
        want = CR.closed_labels(CR.neighbour_graph(clouds[rm], eps), mp)
        assert np.array_equal(CR.closed_labels_blocked(clouds[rm], eps, mp, workers=2, block=1000), want)


def test_graph_equals_plain_evaluation(clouds):
    P = clouds[1][:1500]
    for eps in (4.0, 10.0):
        a, b = CR.neighbour_graph(P, eps), CR.brute_graph(P, eps)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    P = K.decimal_lattice()
    a, b = CR.neighbour_graph(P, 0.3), CR.brute_graph(P, 0.3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("first", [True, False])
def test_bridge(first):
    P, b = K.bridge(first)
    g = CR.neighbour_graph(P, K.BRIDGE_EPS)
    labels = both(g, K.BRIDGE_MIN)
    assert not CR.core_mask(g, K.BRIDGE_MIN)[b] and CR.contested(g, K.BRIDGE_MIN, labels) == 1
    hi = 1 if first else 0                                   # first index of the blob at x = 10
    assert labels[hi] == 0 and labels[hi + 13] == 1 and labels[b] == 0
    assert P[hi, 0] > P[hi + 13, 0]                          # label 0 comes second in x
    assert CR.largest(labels) == (0, 14)


def test_tie_goes_to_the_lower_label():
    labels = both(CR.neighbour_graph(K.tie(), 1.0), 5)
    assert labels.tolist() == [0] * 20 + [1] * 20 and CR.largest(labels) == (0, 20)


def test_strict_lattice():
    P = K.lattice5()
    assert np.array_equal(both(CR.neighbour_graph(P, 5.0), 1), np.arange(len(P)))
    assert CR.largest(np.arange(len(P), dtype=np.int32)) == (0, 1)
    assert np.all(both(CR.neighbour_graph(P, 5.0), 2) == -1)
    assert np.all(both(CR.neighbour_graph(P, 5.000001), 2) == 0)
    assert CR.largest(np.full(5, -1, np.int32)) == (-1, 0)


def test_helix_chain():
    P = K.helix(2000)
    g = CR.neighbour_graph(P, K.HELIX_EPS)
    counts = np.diff(g[0])
    assert np.count_nonzero(counts == 2) == 2 and np.count_nonzero(counts == 3) == len(P) - 2
    assert np.all(both(g, K.HELIX_MIN) == 0)
    P = K.helix(2000, drop=700)
    labels = both(CR.neighbour_graph(P, K.HELIX_EPS), K.HELIX_MIN)
    assert labels.min() == 0 and labels.max() == 1 and sorted(np.bincount(labels).tolist()) == [700, 1299]
