"""Device banded cascadic meshing (csrc/cloud_band.hip, mesh.poisson_band) against the NumPy
restatement (band_ref.py on mesh_ref.py).  Every comparison is exact: index arrays as integers,
float64 bit for bit, and the record.

The shapes are the smallest at which each part can go wrong: depth 4 over base 3 (one block, a band
that is the whole grid, the far node layer alone in its blocks), depth 6 over base 4 (an all-active
level 5 under a sparse level 6), depth 7 over base 5 on two spheres (a sparse level prolonged from
a sparse level, disjoint band pieces, the halo clipped at the box faces); point counts around the
256-thread kernels; points exactly on block faces and on the box's max corner, duplicates, one
crowded cell; 0, 1 and 16 sweeps (the result in either ping-pong buffer).
"""
import functools

import numpy as np
import pytest

import band_ref as BR
import mesh_ref as R
from test_gpu_mesh import check_file, crowded_cloud, duplicate_cloud, host, lattice_cloud, same

pytestmark = pytest.mark.gpu

CLOUDS = {
    **{f"sphere{n}": (lambda n=n: R.sphere(n, 20 + n)) for n in (4, 64, 65, 2000)},
    "lattice": lattice_cloud, "duplicates": duplicate_cloud, "crowded": crowded_cloud,
    "two": lambda: R.two_spheres(4000, 3),
}


@pytest.fixture(scope="module")
def MS():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


@pytest.fixture(scope="module")
def CL():
    from structured_light_for_3d_model_replication_amd import cloud
    return cloud


@functools.lru_cache(maxsize=None)
def reference(name, depth, base, sweeps=BR.DEFAULT_BAND_SWEEPS, scale=1.1):
    """The restatement's whole run for one case (shared, read-only)."""
    P, N = CLOUDS[name]()
    out = BR.poisson_band(P, N, depth, base, sweeps, scale)
    out["P"], out["N"] = P, N
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def table_of(nblocks):
    flat = nblocks.ravel()
    return np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32)


def check(ref, mesh, rec, fields, depth, base, sweeps):
    """Every stage of a device run against the restatement."""
    assert rec["depth"] == depth and rec["base_depth"] == base and rec["sweeps"] == sweeps and rec["points"] == len(ref["P"])
    assert rec["levels"] == ref["record"] and len(fields) == depth - base
    assert rec["vertices"] == len(ref["vertices"]) and rec["triangles"] == len(ref["triangles"])
    assert rec["workspace_bytes"] > 56 * 512 * rec["levels"][-1]["node_blocks"]
    for lv, fl in zip(ref["levels"], fields):
        nblk = BR.node_blocks(lv["active"])
        assert fl["level"] == lv["record"]["level"]
        assert np.array_equal(host(fl["table"]), table_of(nblk))
        assert np.array_equal(host(fl["incident"]), BR.blocked(lv["incident"], nblk))
        for name in ("W", "V", "f", "chi"):
            assert same(host(fl[name]), BR.blocked(lv[name], nblk)), (lv["R"], name)
    assert same(fields[-1]["iso"], ref["iso"])
    assert host(mesh.triangles).dtype == np.int32 and np.array_equal(host(mesh.triangles), ref["triangles"])
    assert same(host(mesh.vertices), ref["vertices"]) and same(host(mesh.densities), ref["densities"])


def run(MS, CL, name, depth, base, sweeps=BR.DEFAULT_BAND_SWEEPS, scale=1.1):
    ref = reference(name, depth, base, sweeps, scale)
    pc = CL.PointCloud(ref["P"].copy(), None, normals=ref["N"].copy())
    mesh, rec, fields = MS.poisson_band(pc, depth=depth, base_depth=base, sweeps=sweeps, scale=scale, return_record=True,
                                        return_fields=True)
    check(ref, mesh, rec, fields, depth, base, sweeps)
    return ref, pc, mesh, rec


# ------------------------------------------------------------------ every stage
@pytest.mark.parametrize("name", ("sphere4", "sphere64", "sphere65", "sphere2000", "lattice", "duplicates", "crowded"))
def test_one_block(MS, CL, name):
    """Depth 4 over base 3: the level's 2^3 cell blocks are all active, 3^3 node blocks are stored."""
    ref, _, _, rec = run(MS, CL, name, 4, 3, scale=1.0 if name in ("lattice", "crowded") else 1.1)
    assert rec["levels"] == [dict(level=4, seeded_blocks=rec["levels"][0]["seeded_blocks"], active_blocks=8, node_blocks=27,
                                  band_nodes=17 ** 3, interior_nodes=15 ** 3)]
    if name == "lattice":                                             # integer points: on cell and block faces, and the max corner
        i, t = R.cell_of(ref["P"], ref["origin"], ref["h"], 16)
        assert (t == 0.0).sum() > 100 and (t == 1.0).any() and i.max() == 15 and (i % 8 == 0).any()


def test_smallest_and_three_levels(MS, CL):
    """Depth 3 over base 2 (one cell block, 2^3 node blocks, the R = 4 base solve) and depth 6 over
    base 3 (three banded levels, the defaults' parents in turn)."""
    _, _, _, rec = run(MS, CL, "sphere64", 3, 2)
    assert rec["levels"] == [dict(level=3, seeded_blocks=1, active_blocks=1, node_blocks=8, band_nodes=729, interior_nodes=343)]
    _, _, _, rec = run(MS, CL, "sphere65", 6, 3)
    assert [lv["level"] for lv in rec["levels"]] == [4, 5, 6]


@pytest.mark.parametrize("sweeps", (0, 1, 16))
def test_sparse_over_full(MS, CL, sweeps):
    """Depth 6 over base 4: level 5 is all active, level 6 is sparse."""
    ref, _, mesh, rec = run(MS, CL, "sphere2000", 6, 4, sweeps)
    lo, hi = rec["levels"]
    assert lo["active_blocks"] == 4 ** 3 and lo["band_nodes"] == 33 ** 3 and lo["interior_nodes"] == 31 ** 3
    assert 0 < hi["seeded_blocks"] < hi["active_blocks"] < 8 ** 3 and hi["node_blocks"] < 9 ** 3
    if sweeps == 16:
        assert R.topology(host(mesh.triangles)) == (True, True, 2)


def test_sparse_over_sparse(MS, CL):
    """Depth 7 over base 5 on two spheres: both levels sparse, the band in two pieces that reach the box."""
    ref, _, mesh, rec = run(MS, CL, "two", 7, 5)
    lo, hi = rec["levels"]
    assert lo["active_blocks"] < 8 ** 3 and hi["active_blocks"] < 16 ** 3 and BR.nested(ref["levels"])
    assert R.topology(host(mesh.triangles)) == (True, True, 4)


# ------------------------------------------------------------------ calling and refusals
def test_twice_and_the_input_is_untouched(MS, CL):
    ref, pc, mesh, rec = run(MS, CL, "sphere65", 6, 4)
    again, rec2 = MS.poisson_band(pc, depth=6, base_depth=4, return_record=True)
    assert rec2 == rec
    assert same(host(again.vertices), host(mesh.vertices)) and np.array_equal(host(again.triangles), host(mesh.triangles))
    assert same(host(again.densities), host(mesh.densities))
    assert same(host(pc.xyz), ref["P"]) and same(host(pc.normals), ref["N"])
    plain = MS.poisson_band(pc, depth=6, base_depth=4)                # without the record: the mesh alone
    assert isinstance(plain, MS.TriangleMesh) and same(host(plain.vertices), ref["vertices"])
    assert MS.band_workspace_bytes(rec) == rec["workspace_bytes"]


def test_bad_clouds_then_a_good_one(MS, CL):
    ref = reference("sphere2000", 6, 4)
    P, N = ref["P"], ref["N"]
    with pytest.raises(ValueError, match="no normals"):
        MS.poisson_band(CL.PointCloud(P.copy(), None), depth=6)
    bad = P.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        MS.poisson_band(CL.PointCloud(bad, None, normals=N.copy()), depth=6, base_depth=4)
    badn = N.copy()
    badn[7, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        MS.poisson_band(CL.PointCloud(P.copy(), None, normals=badn), depth=6, base_depth=4)
    with pytest.raises(ValueError, match="no extent"):
        MS.poisson_band(CL.PointCloud(np.ones((5, 3)), None, normals=N[:5].copy()), depth=6)
    run(MS, CL, "sphere2000", 6, 4)                                   # a good call of the same size follows


# ------------------------------------------------------------------ ProcessingLogic
def restated_stl(P, N, depth, base, scale, q):
    out = BR.poisson_band(P, N, depth, base, BR.DEFAULT_BAND_SWEEPS, scale)
    V, T, D = out["vertices"], out["triangles"], out["densities"]
    if q > 0.0:
        V, T, D = R.remove_vertices_by_mask(V, T, D, D < R.quantile(D, q))
    return V, T, R.stl_bytes(V, T, R.triangle_normals(V, T))


def test_mesh_360(MS, CL, tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    P, _ = R.sphere(1500, 31, radius=2.0)
    src, out = tmp_path / "merged.ply", tmp_path / "mesh.stl"
    CL.PointCloud(P, None).save(str(src))
    kw = dict(normal_radius=0.6, normal_max_nn=30, orientation_mode="radial")
    PL.mesh_360(str(src), str(out), depth=6, density_trim=0.01, poisson_rule="band", base_depth=4, **kw)
    pcd = PL.estimate_oriented_normals(str(src), return_obj=True, **kw)
    V, T, data = restated_stl(host(pcd.xyz), host(pcd.normals), 6, 4, 1.1, 0.01)
    check_file(MS, out, V, T, data)
    assert len(T) and R.signed_volume(V, T) > 0.0


def test_reconstruct_stl(MS, CL, tmp_path):
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    P, N = R.sphere(1500, 32, radius=2.0)
    src, out, nrm = tmp_path / "cloud.ply", tmp_path / "mesh.stl", tmp_path / "normals.ply"
    CL.PointCloud(P, None, normals=-N).save(str(src))          # inward normals: the centroid branch turns them
    PL.reconstruct_stl(str(src), str(out), params={"depth": 6, "poisson_rule": "band"}, save_normals_path=str(nrm))
    pcd = CL.PointCloud.from_file(str(nrm))
    V, T, data = restated_stl(host(pcd.xyz), host(pcd.normals), 6, 5, 1.1, 0.02)     # base_depth defaults to depth - 1
    check_file(MS, out, V, T, data)
    CL.PointCloud(P, None, normals=np.zeros_like(N)).save(str(src))
    with pytest.raises(ValueError, match="Generated mesh is empty."):
        PL.reconstruct_stl(str(src), str(out), params={"depth": 4, "poisson_rule": "band"})
