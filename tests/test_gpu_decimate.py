"""Device mesh decimation (csrc/cloud_decimate.hip, mesh.decimate_quadric) against the NumPy
restatement (decimate_ref.py).  Every comparison is exact: triangles as integers, float64 bit for
bit, the record key by key.

The shapes are the smallest at which each part can go wrong: every builder mesh (closed, open, one
triangle, an unreferenced vertex, a doubled triangle, two holes sharing a vertex, rows longer than
a wavefront), targets that force 0, 1 and "until nothing is valid" rounds, triangle and
candidate-edge counts around one 256-thread block and over several, the planar patch where only
the tie rules decide, the last round's budget prefix and the odd remainder, a NaN vertex, and the
depth-5 sphere and the lattice over many workgroups.  References are computed once
(decimate_ref.reference) and shared."""
import threading

import numpy as np
import pytest

import decimate_ref as R
import mesh_ref as MR
import meshpost_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MS():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def host(t):
    return t.cpu().numpy()


def device_mesh(MS, V, T, D=None):
    import torch
    return MS.TriangleMesh(torch.from_numpy(np.array(V, np.float64)).cuda(), torch.from_numpy(np.array(T, np.int32)).cuda(),
                           None if D is None else torch.from_numpy(np.array(D, np.float64)).cuda())


def check(MS, name, target, max_rounds=512):
    V, T, D = R.built(name)
    Vr, Tr, Dr, rec_ref = R.reference(name, target, max_rounds)
    mesh = device_mesh(MS, V, T, D)
    out, rec = MS.decimate_quadric(mesh, target, max_rounds=max_rounds, return_record=True)
    print(name, target, max_rounds, rec)
    assert rec == rec_ref
    got = host(out.triangles)
    assert got.dtype == np.int32 and got.shape == Tr.shape and np.array_equal(got, Tr)
    assert same(host(out.vertices), Vr) and same(host(out.densities), Dr) and out.triangle_normals is None
    assert same(host(mesh.vertices), V) and np.array_equal(host(mesh.triangles), T)      # the input is untouched
    return rec


ALL = ("tetrahedron", "octahedron", "single_triangle", "open_strip", "disc_hole5", "bow_tie", "unreferenced", "duplicated",
       "fan", "hexagon", "bipyramid", "planar", "nan_vertex", "patch8x16cut", "patch8x16", "patch3x43", "patch7x11",
       "patch9x9", "patch24x24")


@pytest.mark.parametrize("name", ALL)
def test_builders_zero_one_and_all_rounds(MS, name):
    nt = len(R.built(name)[1])
    assert check(MS, name, nt)["rounds"] == 0                        # target >= T: an equal mesh
    assert check(MS, name, nt + 7)["rounds"] == 0
    assert check(MS, name, 0, max_rounds=0)["stop"] == "max_rounds"
    check(MS, name, 0, max_rounds=1)
    rec = check(MS, name, 0)                                         # until nothing is valid
    assert rec["stop"] == "no_valid_edge" and rec["valid"] == 0


def test_builder_outcomes(MS):
    for name in ("open_strip", "fan", "hexagon", "disc_hole5", "single_triangle", "tetrahedron"):
        assert check(MS, name, 0)["collapses"] == 0
    assert check(MS, "octahedron", 4)["faces_out"] == 4
    assert check(MS, "duplicated", 0, max_rounds=1)["nonmanifold"] > 0
    assert check(MS, "nan_vertex", 0, max_rounds=1)["nan"] > 0 and check(MS, "nan_vertex", 0)["collapses"] > 0
    assert check(MS, "bipyramid", 40)["stop"] == "target"
    assert check(MS, "planar", 20)["collapses"] > 0


@pytest.mark.parametrize("max_rounds", (1, 2, 3))
def test_sphere_round_by_round(MS, max_rounds):
    rec = check(MS, "sphere4", 200, max_rounds=max_rounds)
    assert rec["rounds"] == max_rounds and rec["stop"] == "max_rounds"


@pytest.mark.parametrize("target", (200, 201, 1000))
def test_sphere_to_target(MS, target):
    rec = check(MS, "sphere4", target)
    assert rec["stop"] == "target" and rec["faces_out"] == target - target % 2
    if target == 200:                                                # the last round applied a prefix of the selected
        before = R.reference("sphere4", 200, rec["rounds"] - 1)[3]["collapses"]
        assert 0 < rec["collapses"] - before < rec["selected"]


def test_lattice(MS):
    rec = check(MS, "lattice", 6000)
    assert rec["stop"] == "target" and rec["rounds"] == 6


def test_trimmed_sphere(MS):
    rec = check(MS, "trimmed5", 0, max_rounds=3)
    assert rec["rounds"] == 3 and rec["collapses"] > 1000
    check(MS, "trimmed5", 15000)


def test_bad_index_and_no_densities(MS):
    V, T, _ = R.built("octahedron")
    for bad in (6, -1):
        Tb = T.copy()
        Tb[3, 1] = bad
        for target in (4, 100):                                      # also when no round would run
            with pytest.raises(IndexError):
                MS.decimate_quadric(device_mesh(MS, V, Tb), target)
    out = MS.decimate_quadric(device_mesh(MS, V, T), 4)
    Vr, Tr, _, _ = R.reference("octahedron", 4)
    assert out.densities is None and same(host(out.vertices), Vr) and np.array_equal(host(out.triangles), Tr)
    import torch
    empty = MS.TriangleMesh(torch.zeros((3, 3), dtype=torch.float64).cuda(), torch.zeros((0, 3), dtype=torch.int32).cuda())
    out, rec = MS.decimate_quadric(empty, 0, return_record=True)
    assert len(out.vertices) == 3 and len(out.triangles) == 0 and rec["rounds"] == 0 and rec["stop"] == "target"


def test_postprocess_with_simplify_rule(MS):
    V, T, D = P.trimmed_sphere()
    params = {"smooth_type": "taubin", "smooth_iters": 2, "close_holes": True, "close_max_size": 30, "simplify": True,
              "simplify_rule": "rounds", "target_faces": 20000}
    V1, T1 = P.postprocess(V, T, params)
    assert len(T1) > 20000
    Vr, Tr, Dr, rec = R.decimate(V1, T1, 20000, D=D)
    out = MS.postprocess(device_mesh(MS, V, T, D), params)
    assert len(Tr) == 20000 and np.array_equal(host(out.triangles), Tr)
    assert same(host(out.vertices), Vr) and same(host(out.densities), Dr)


def test_reconstruct_stl_device_backend_simplify(MS, tmp_path):
    from structured_light_for_3d_model_replication_amd import cloud as CL
    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic as PL
    Pts, Nrm = MR.sphere(500, 3)
    src, out, nrm = tmp_path / "cloud.ply", tmp_path / "mesh.stl", tmp_path / "normals.ply"
    CL.PointCloud(Pts, None, normals=Nrm).save(str(src))
    params = {"enabled": True, "backend": "device", "smooth_type": "taubin", "smooth_iters": 2, "close_holes": True,
              "close_max_size": 30, "simplify": True, "simplify_rule": "rounds", "target_faces": 1500}
    PL.reconstruct_stl(str(src), str(out), params={"depth": 4}, meshlab_params=params, save_normals_path=str(nrm))
    pcd = CL.PointCloud.from_file(str(nrm))
    res = MR.poisson(host(pcd.xyz), host(pcd.normals), 4)
    V, T, D = res["vertices"], res["triangles"], res["densities"]
    V, T, D = MR.remove_vertices_by_mask(V, T, D, D < MR.quantile(D, 0.02))
    V1, T1 = P.postprocess(V, T, params)
    assert len(T1) > 1500
    V2, T2, _, rec = R.decimate(V1, T1, 1500)
    assert rec["stop"] == "target"
    assert out.read_bytes() == MR.stl_bytes(V2, T2, MR.triangle_normals(V2, T2))


def test_two_threads(MS):
    """Each call has its own workspace: two threads decimating different meshes at once get the
    single-thread results."""
    jobs = (("sphere4", 1000), ("lattice", 6000))
    refs = [R.reference(*j) for j in jobs]
    meshes = [device_mesh(MS, *R.built(j[0])) for j in jobs]
    got, errors = [None, None], []

    def work(i):
        try:
            import torch
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(2):
                    got[i] = MS.decimate_quadric(meshes[i], jobs[i][1], return_record=True,
                                                 stream=torch.cuda.current_stream())
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (out, rec), (Vr, Tr, Dr, rec_ref) in zip(got, refs):
        assert rec == rec_ref and np.array_equal(host(out.triangles), Tr)
        assert same(host(out.vertices), Vr) and same(host(out.densities), Dr)
