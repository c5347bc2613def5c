"""The banded cascadic mesher's rule, on the restatement alone (no GPU): tests/band_ref.py on clouds
whose answer is known.  The bands nest, the mesh is a closed 2-manifold wherever the surface stays
inside the band and ends at the band's edge where it does not, and the default number of sweeps
brings the cascade within a tenth of the dense solve's radial error."""
import functools

import numpy as np
import pytest

import band_ref as BR
import mesh_ref as M


@functools.lru_cache(maxsize=None)
def band(name, depth, base, sweeps=BR.DEFAULT_BAND_SWEEPS):
    P, Nrm = cloud(name)
    return BR.poisson_band(P, Nrm, depth, base, sweeps)


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "two":
        return M.two_spheres(4000, 3)
    if name == "open":
        return BR.open_sphere(60000, 1)
    return M.sphere(int(name), 1)


def radial_error(res):
    V, T = res["vertices"], res["triangles"]
    used = np.unique(T)
    return float(np.abs(np.linalg.norm(V[used], axis=1) - 1.0).mean())


def test_the_bands_nest():
    res = band("two", 7, 5)
    assert [lv["R"] for lv in res["levels"]] == [64, 128]
    assert BR.nested(res["levels"])
    lo, hi = res["levels"]
    assert 0 < hi["cells"].mean() < lo["cells"].mean() < 1          # both levels are sparse, the finer one more so
    for lv in res["levels"]:                                         # every point's cell is active, its 8 corners band nodes
        i, _ = M.cell_of(cloud("two")[0], res["origin"], lv["h"], lv["R"])
        assert lv["cells"][i[:, 2], i[:, 1], i[:, 0]].all()
        assert (lv["incident"] == 255).sum() == lv["record"]["interior_nodes"] < lv["record"]["band_nodes"]
        assert lv["chi"][lv["incident"] == 0].max() == 0.0 == lv["chi"][lv["incident"] == 0].min()


@pytest.mark.parametrize("name, depth, base", [("60000", 7, 5), ("two", 7, 5)])
def test_closed_two_manifold(name, depth, base):
    res = band(name, depth, base)
    T = res["triangles"]
    assert len(T) and len(np.unique(T)) == len(res["vertices"])
    closed, oriented, euler = M.topology(T)
    assert closed and oriented and euler == (4 if name == "two" else 2)
    assert M.signed_volume(res["vertices"], T) > 0.0


def test_open_sphere_ends_at_the_band():
    """Every boundary edge lies on a face between an active and an inactive cell."""
    res = band("open", 7, 4)
    V, T = res["vertices"], res["triangles"].astype(np.int64)
    cells, R = res["levels"][-1]["cells"], res["R"]
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    lo, hi = d.min(axis=1), d.max(axis=1)
    key, count = np.unique(lo * len(V) + hi, return_counts=True)
    assert count.max() == 2
    open_edges = key[count == 1]
    assert 300 < len(open_edges) < 900                                # one loop where the closure leaves the band
    a, b = V[open_edges // len(V)], V[open_edges % len(V)]
    ua, ub = (a - res["origin"]) / res["h"], (b - res["origin"]) / res["h"]
    on_face = (np.abs(ua - np.round(ua)) < 1e-9) & (np.abs(ub - np.round(ub)) < 1e-9) & (np.round(ua) == np.round(ub))
    assert on_face.any(axis=1).all()
    mid = np.floor((ua + ub) / 2.0).astype(np.int64)

    def is_active(c):
        inside = ((c >= 0) & (c < R)).all(axis=1)
        cc = np.clip(c, 0, R - 1)
        return inside & cells[cc[:, 2], cc[:, 1], cc[:, 0]]
    between = np.zeros(len(open_edges), bool)
    for axis in range(3):
        hi_c = mid.copy()
        hi_c[:, axis] = np.round(ua[:, axis]).astype(np.int64)
        lo_c = hi_c.copy()
        lo_c[:, axis] -= 1
        between |= on_face[:, axis] & (is_active(lo_c) != is_active(hi_c))
    assert between.all()
    below = V[np.unique(T)]
    below = below[below[:, 2] < 0.5]
    assert np.abs(np.linalg.norm(below, axis=1) - 1.0).mean() < 2e-3  # below the cut the surface is the sphere's


@pytest.mark.parametrize("name, depth, base", [("60000", 7, 5), ("20000", 6, 4)])
def test_default_sweeps_reach_the_dense_accuracy(name, depth, base):
    """mean | |v| - 1 | over the used vertices is at most 1.10 times the dense restatement's at the
    same depth: measured 1.053 (depth 7 / base 5) and 1.024 (depth 6 / base 4) at 16 sweeps; 8 sweeps
    give 1.12 on the first, which the margin refuses."""
    P, Nrm = cloud(name)
    dense = radial_error(M.poisson(P, Nrm, depth))
    ratio = radial_error(band(name, depth, base)) / dense
    print(f"band / dense radial error at depth {depth} / base {base}: {ratio:.4f} (dense {dense:.4e})")
    assert ratio <= 1.10


def test_counts_are_unchanged_when_run_twice():
    P, Nrm = cloud("two")
    a, b = band("two", 7, 5), BR.poisson_band(np.array(P), np.array(Nrm), 7, 5)
    assert a["record"] == b["record"]
    assert a["vertices"].shape == b["vertices"].shape and a["triangles"].shape == b["triangles"].shape
    assert np.array_equal(a["triangles"], b["triangles"])
    assert np.array_equal(a["vertices"].view(np.uint64), b["vertices"].view(np.uint64))


def test_blocked_layout_and_arguments():
    res = band("20000", 6, 4)
    lv = res["levels"][-1]
    nblk = BR.node_blocks(lv["active"])
    assert nblk.shape == (9, 9, 9) and nblk.sum() == lv["record"]["node_blocks"]
    blk = BR.blocked(lv["chi"], nblk)
    assert blk.shape == (nblk.sum(), 8, 8, 8)
    bz, by, bx = [int(v[0]) for v in np.nonzero(nblk)]
    assert blk[0, 1, 2, 3] == lv["chi"][8 * bz + 1, 8 * by + 2, 8 * bx + 3]
    assert np.count_nonzero(blk) == np.count_nonzero(lv["chi"])        # every band node is in a stored block
    assert BR.blocked(lv["V"], nblk).shape == (nblk.sum(), 8, 8, 8, 3)
    assert BR.check_depths(11) == (11, 8) and BR.check_depths(4) == (4, 3) and BR.check_depths(12, 10) == (12, 10)
    for depth, base in ((2, None), (13, None), (6, 6), (6, 1), (12, 11)):
        with pytest.raises(ValueError):
            BR.check_depths(depth, base)
