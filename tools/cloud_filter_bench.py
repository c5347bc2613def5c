#!/usr/bin/env python
"""Device cloud filters on one C2 view's cloud against the CPU restatement -- reported in
DESIGN.md §9, never the bench metric.  One 1080p view (11+10 sets, Otsu) is reconstructed on the
device (float64 XYZ); the radius filter and the statistical filter run on that device cloud at the
reference's defaults, (nb_points 100, radius 5.0) and (nb_neighbors 20, std_ratio 2.0), timed with
HIP events around mask + select (status and count are read once per call, as a user's call does).
Beside that, the same rules on the host: tests/cloud_ref.py over scipy's cKDTree with
``workers`` threads, on the same points, in the same run.  The two masks are compared.

The cluster step (DBSCAN + largest cluster, timed around labels + select) runs on the same cloud at
the reference's defaults (eps 5.0, min_points 200) and at a second setting that splits the view
into many clusters (``--cluster-multi``, default 1.0 16); the host side is the closed form of
tests/cluster_ref.py folded block by block (the whole graph of a 1080p view does not fit in
memory), and the labels are compared.  Read the cluster times against the radius filter's of the
same run: the cluster step is the radius count plus two more neighbourhood walks.

``--voxel SIZE`` and ``--normals RADIUS MAX_NN`` add the voxel down-sample and the normal
estimation, timed the same way; beside the normals the statistical mask at
``k = MAX_NN`` is timed in the same run (the same walk without indices, moments and solve).  The
host side is tests/normals_ref.py, its neighbour lists proposed by cKDTree and ranked by
(d2, index); positions, colours, counts, ``m`` and ``cov`` are compared, not just timed.
``--skip-cluster`` leaves the cluster step out.

``--icp DIST`` adds the point-to-plane ICP.  Target: the view's cloud with normals
(radius ``2 * DIST``, max_nn 30: the merge loop's relation between the two).  Source: the same
cloud moved by the inverse of a fixed small motion (a rotation about the centroid and a translation,
together about ``0.5 * DIST`` on the points).  HIP events go around the whole registration at the
reference's defaults (1e-6, 1e-6, 30), status and result read-back included; the host side is
tests/icp_ref.py over cKDTree with ``workers`` threads, and iterations, convergence, the final
correspondences and the transform are compared.  ``--icp-only`` leaves everything else out.

``--fpfh RADIUS MAX_NN`` and ``--global-reg DIST`` add the global registration,
each stage between HIP events of its own: the FPFH features of the view (normals at radius
``0.4 * RADIUS``, max_nn 30: the merge's relation between the two), the feature matching with the
mutual filter, and the seeded RANSAC.  The registration is of a moved part of the view (as in
tests/feature_ref.py's base case: the points with ``index % 3 != 1`` and x above the 20 %
quantile, under the inverse of a rotation of (25, -10, 15) degrees about the centroid plus a
translation of about ``5 * DIST``, with its own normals and features) onto the view.  The host side is
tests/feature_ref.py: features from cKDTree-proposed lists are compared for equality where the
proposal resolved every tie; the brute-force matching restatement is not affordable at a whole
view (1.2 M x 1.2 M rows), so ``--match-sample`` rows (default 64) are compared and the count
is reported; the RANSAC restatement runs on the device's correspondences.  ``--gr-only`` leaves
every other step out.

``--plane DIST [ITERATIONS]`` adds the seeded RANSAC plane segmentation on the
view's cloud with a planted wall behind it (tests/plane_ref.py's ``plant_wall``: as many points
again on a tilted plane ``4 * DIST`` behind the farthest point, offsets below ``DIST / 2``).  HIP
events go around one batch's launches alone (trials, evaluation, records), around a batch with
its read-back, around the finish, and around the whole ``segment_plane`` and ``remove_plane``; the
per-kernel split comes from a kernel trace of the same command.  The host side is
tests/plane_ref.py on ``workers`` threads; the winner, ``K``, every record's bits and the inlier
set are compared.  ``--plane-only`` leaves every other step out.

``--orient K`` adds the tangent-plane normal orientation: normals of the view at
``--orient-normals RADIUS MAX_NN`` (default 5.0 30), a seeded random half of them negated, then
``orient_normals_consistent_tangent_plane(K)``.  HIP events go around the whole call and around
the calls that end after its first and second stage (``slg_knn_lists``, ``slg_emst``), so the three
stages are differences; the counters of the rounds (rounds per Boruvka, points that walked and
far-list entries per round) come from the call itself.  The host side is tests/orient_ref.py with
the EMST's candidates from ``scipy.spatial.Delaunay``, which is valid only without cospherical
ties: it runs on the view voxel-down-sampled to at most ``--orient-cpu-points`` points (the size is
recorded), the device runs on that cloud too, and the tool asserts that the trees agree.
``--orient-only`` leaves every other step out.

``--mesh DEPTH`` adds the watertight mesher: normals of the view at radius 5.0 / 30
oriented outward from the centroid, then ``mesh.poisson_grid(depth=DEPTH)`` with HIP events around
its stages, the 0.02 quantile trim, the triangle normals and the STL records.  It reports the mean
per-stage times, ``V``, ``T``, the cycles, the workspace, and the solve's rate against a byte model
(per cycle and node of the finest level 4 sweeps and a residual at 24 B, 8 B for the restriction and
16 B for the prolongation, times 8/7 for the coarser levels).  ``--mesh-only`` leaves every other
step out.  ``--post`` adds the mesh post-processing on the mesh trimmed at
``--post-trim`` (default 0.02, the reference's; ``--post-punch K`` also drops every K-th vertex,
since the trim of an open view removes nothing and leaves no hole): ``vertex_adjacency``, 10 Taubin iterations with
that adjacency (20 passes), ``boundary_loops`` and ``close_holes`` at 30 edges.  It reports ``V``,
``T``, the mean degree, the loop counts and the smoothing pass's rate against the byte model of a
pass, ``V (24 (deg + 1) + 4 deg + 16 + 24)`` bytes with ``deg`` the mean row length used.
``--audit`` (with ``--mesh``) adds ``mesh.audit`` of the meshed view before and after
the trim and, with ``--post``, after the hole closing and after ``mesh.clean`` of that: the stage times
(HIP events), the counts, the verdict line, the five largest components, the edges step against its
byte model, and the times of ``mesh.keep_largest_components`` and ``mesh.clean``.
``--intersect`` (with ``--mesh`` and ``--post``) adds ``mesh.self_intersections`` of the
view's mesh, of the punched and hole-closed mesh and, with ``--decimate``, of the decimated mesh: the
call's time, the stage times by HIP events (``boxes``, ``entries`` with the sort, ``candidates``, ``test``,
``lists``), every count, the one-line form, and the test kernel's determinant rate, ``tested_pairs x 15
x 40`` flop over the ``test`` stage, against the 78.6 TFLOP/s vector fp64 peak.
``--decimate TARGET`` (with ``--post``) adds ``mesh.decimate_quadric`` of the
hole-closed mesh to ``TARGET`` faces: per-call time, rounds, collapses, the stop reason, ``V`` and
``T`` in and out, the time of every round, and the byte model of the candidate evaluation summed
over the rounds, ``candidates (350 + 192 deg)`` bytes with ``deg`` the mean valence (per edge two
neighbour and two incidence rows with their triangles' corners and positions, two quadrics, the
outputs), beside its compulsory traffic.  ``--kernel-stats CSV`` takes a ``rocprofv3 --kernel-trace
--stats`` kernel table of a run of this very command and reports the evaluation kernel's time per
call and its rate against the model.

``--mesh-band DEPTH [--mesh-base D]`` adds the banded cascadic mesher on the same
oriented view: ``mesh.poisson_band`` with HIP events around the block tables, the dense base level,
every banded level's stages (node classification, splat, divergence, prolongation, sweeps), the
iso value and the extraction; per level the blocks and nodes, and the smoother's rate against its
byte model (24 B per stored node and sweep); the workspace's bytes, ``V`` / ``T`` and the open
boundary edges (``mesh.boundary_loops``) before and after the 0.02 trim.  A workspace beyond the free
memory is reported with the bytes it asked for.  ``--mesh-only`` applies.

``--surface RADII`` adds the surface mesher: normals of the view at
``--surface-normals`` (default radius 1.0 / 30) oriented by the tangent-plane orientation with
``--surface-orient`` neighbours, then ``mesh.ball_pivot`` at ``RADII`` (multiples of the mean
nearest-neighbour distance, e.g. ``1,2,4``).  It reports the call's time and per pass the stages'
times by HIP events (``grid``, ``count``, ``emit``, ``select``, ``commit``) with the candidates, the
accepted and the rounds.  The CPU side is ``tests/surface_ref.py`` on the view voxel-down-sampled to
at most ``--surface-cpu-points`` points; the device runs on that cloud too and the tool asserts that
the triangles and the record are equal.  ``--surface-only`` leaves every other step out.

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--row-mode", type=int, default=1)
    ap.add_argument("--cam", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--cluster-multi", type=float, nargs=2, default=(1.0, 16), metavar=("EPS", "MIN_POINTS"),
                    help="the second cluster setting (one that splits the view into several clusters)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cKDTree side")
    ap.add_argument("--voxel", type=float, metavar="SIZE", help="also time voxel_down_sample at this size")
    ap.add_argument("--normals", nargs=2, metavar=("RADIUS", "MAX_NN"),
                    help="also time the normal estimation at this radius and max_nn")
    ap.add_argument("--skip-cluster", action="store_true", help="leave the cluster step out")
    ap.add_argument("--icp", type=float, metavar="DIST", help="also time the point-to-plane ICP at this distance")
    ap.add_argument("--icp-only", action="store_true", help="with --icp: leave every other step out")
    ap.add_argument("--fpfh", nargs=2, metavar=("RADIUS", "MAX_NN"), help="also time the FPFH features and the matching")
    ap.add_argument("--global-reg", type=float, metavar="DIST",
                    help="with --fpfh: also time the RANSAC registration of a moved copy at this distance")
    ap.add_argument("--match-sample", type=int, default=64, help="rows of the matching compared with the restatement")
    ap.add_argument("--seed", type=int, default=0, help="the RANSAC's seed")
    ap.add_argument("--gr-only", action="store_true", help="with --fpfh: leave every other step out")
    ap.add_argument("--plane", nargs="+", metavar="DIST [ITERATIONS]",
                    help="also time the plane segmentation at this distance threshold (default 1000 iterations)")
    ap.add_argument("--plane-only", action="store_true", help="with --plane: leave every other step out")
    ap.add_argument("--orient", type=int, metavar="K", help="also time the tangent-plane normal orientation with K neighbours")
    ap.add_argument("--orient-normals", nargs=2, default=("5.0", "30"), metavar=("RADIUS", "MAX_NN"),
                    help="with --orient: the normal estimation before it")
    ap.add_argument("--orient-cpu-points", type=int, default=20000, help="with --orient: the size the host side runs at")
    ap.add_argument("--orient-only", action="store_true", help="with --orient: leave every other step out")
    ap.add_argument("--mesh", type=int, metavar="DEPTH", help="also time the watertight mesher at this depth")
    ap.add_argument("--mesh-only", action="store_true", help="with --mesh or --mesh-band: leave every other step out")
    ap.add_argument("--mesh-band", type=int, metavar="DEPTH", help="also time the banded cascadic mesher at this depth (3..12)")
    ap.add_argument("--mesh-base", type=int, metavar="D", help="with --mesh-band: the dense base depth (default min(8, DEPTH - 1))")
    ap.add_argument("--post", action="store_true", help="with --mesh: also time adjacency, Taubin smoothing and hole closing")
    ap.add_argument("--post-trim", type=float, default=0.02, help="with --post: the density quantile trimmed before it")
    ap.add_argument("--post-punch", type=int, default=0, metavar="K",
                    help="with --post: also drop every K-th vertex (an open view's trim removes nothing, so this makes the holes)")
    ap.add_argument("--audit", action="store_true",
                    help="with --mesh: audit the mesh before and after the trim (and after --post), keep the largest component, clean")
    ap.add_argument("--intersect", action="store_true",
                    help="with --mesh --post: test the view's mesh, the hole-closed mesh and the decimated mesh for crossing triangles")
    ap.add_argument("--decimate", type=int, metavar="TARGET", help="with --post: also time decimate_quadric to this many faces")
    ap.add_argument("--kernel-stats", metavar="CSV", help="with --decimate: rocprofv3's kernel stats of a run of this command")
    ap.add_argument("--surface", metavar="RADII", help="also time the surface mesher at these multiples of the mean "
                                                      "nearest-neighbour distance, e.g. 1,2,4")
    ap.add_argument("--surface-normals", nargs=2, default=("1.0", "30"), metavar=("RADIUS", "MAX_NN"),
                    help="with --surface: the normal estimation before it")
    ap.add_argument("--surface-orient", type=int, default=30, metavar="K", help="with --surface: the tangent-plane orientation's K")
    ap.add_argument("--surface-cpu-points", type=int, default=20000, help="with --surface: the size the restatement runs at")
    ap.add_argument("--surface-only", action="store_true", help="with --surface: leave every other step out")
    args = ap.parse_args()

    import numpy as np
    import torch
    from structured_light_for_3d_model_replication_amd import cloud as CL, engine as E, synth

    assert torch.cuda.is_available(), "cloud_filter_bench needs a GPU"
    W, H = args.cam
    rig = synth.default_rig(W, H, 1920, 1080)
    v = synth.render_view(rig, 25.0, seed=1, n_present=44)
    frames = E.DeviceFrames(list(v.frames), v.texture)
    eng = E.Reconstructor(H, W)
    cfg = E.DecodeConfig(1920, 1080, 11, 10, "otsu")
    dc = E.DeviceCalib(rig.tables(), H, W)
    pc = CL.PointCloud.from_cloud(eng.reconstruct(frames, cfg, dc, row_mode=args.row_mode, xyz_f64=True))
    n = len(pc)

    def timed(fn):
        ms = []
        out = None
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return out, ms

    res = {"tool": "cloud_filter_bench", "points": n, "row_mode": args.row_mode, "cam": [W, H],
           "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    if args.surface:
        import surface_ref as SR
        from structured_light_for_3d_model_replication_amd import mesh as MS
        mult = sorted({float(x) for x in args.surface.split(",")})
        nr, nk, ok = float(args.surface_normals[0]), int(args.surface_normals[1]), int(args.surface_orient)
        mean = lambda v: sum(v) / len(v)

        def oriented(cloud, radius):
            return CL.orient_normals_consistent_tangent_plane(CL.estimate_normals(cloud, radius, nk), ok)

        def radii_of(cloud):
            avg = float(np.mean(CL.nearest_neighbor_distance(cloud).cpu().numpy()))
            return avg, [avg * m for m in mult]

        src = oriented(pc, nr)
        avg, radii = radii_of(src)
        passes = []

        def run():
            t = []
            out = MS.ball_pivot(src, radii, return_record=True, timings=t)
            passes.append(t)
            return out

        (mesh, rec), ms = timed(run)
        print(f"[device] ball_pivot done {ms}", file=sys.stderr, flush=True)
        passes = passes[args.warmup:]
        stage_keys = ("grid", "count", "emit", "select", "commit")
        per_pass = [{**rec[k], **{s + "_ms": mean([p[k].get(s, 0.0) for p in passes]) for s in stage_keys}} for k in range(len(radii))]
        res["surface"] = {
            "multipliers": mult, "mean_nn": avg, "radii": radii, "points": n, "normal_radius": nr, "normal_max_nn": nk,
            "orient_k": ok, "triangles": len(mesh.triangles), "device_ms": ms, "passes": per_pass,
            "what_is_timed": "device_ms: ball_pivot with its allocations and read-backs (the status and the count per pass, "
                             "the header per round); passes: HIP events around the stages, the read-back inside the stage it ends",
            "grid_workspace_bytes": int(CL.N.lib().slg_surface_ws_bytes(CL.N.SURFACE_WS_GRID, n, 0, 0))}
        if not args.no_cpu:
            voxel, small = 0.0, pc
            while len(small) > args.surface_cpu_points:
                voxel = 1.0 if voxel == 0.0 else voxel * 1.25
                small = CL.voxel_down_sample(pc, voxel)
            small = oriented(small, max(nr, 2.5 * voxel))
            s_avg, s_radii = radii_of(small)
            (s_mesh, s_rec), s_ms = timed(lambda: MS.ball_pivot(small, s_radii, return_record=True))
            P, Nrm = small.xyz.cpu().numpy(), small.normals.cpu().numpy()
            t0 = time.perf_counter()
            want, w_rec, _ = SR.ball_pivot(P, Nrm, s_radii)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            same = {"triangles": bool(np.array_equal(s_mesh.triangles.cpu().numpy(), want)), "record": s_rec == w_rec}
            res["surface"].update({
                "cpu_points": len(small), "cpu_voxel": voxel, "cpu_radii": s_radii, "cpu_ms": cpu_ms, "cpu_record": w_rec,
                "device_ms_at_cpu_points": s_ms, "cpu_what": "tests/surface_ref.py: cKDTree lists, the triples of an anchor "
                                                             "vectorised in NumPy, the greedy selection in Python",
                "equal_cpu": same, "speedup_vs_cpu_at_cpu_points": cpu_ms / mean(s_ms)})
            assert all(same.values()), f"the device and the restatement differ: {same}"
        if args.surface_only:
            print(json.dumps(res))
            return
    if args.mesh_band:
        from structured_light_for_3d_model_replication_amd import mesh as MS
        depth, base = MS.check_band_depth(args.mesh_band, args.mesh_base)
        src = CL.orient_normals_towards(CL.estimate_normals(pc, 5.0, 30), CL.centroid(pc), outward=True)
        mean = lambda v: sum(v) / len(v)
        band = {"depth": depth, "base_depth": base, "sweeps": MS.DEFAULT_BAND_SWEEPS, "points": n, "normal_radius": 5.0,
                "normal_max_nn": 30, "free_bytes": int(torch.cuda.mem_get_info()[0])}
        stages = []

        def run():
            t = {}
            out = MS.poisson_band(src, depth=depth, base_depth=base, return_record=True, timings=t)
            stages.append(t)
            return out

        try:
            (mesh, rec), ms = timed(run)
        except MemoryError as e:                              # the bytes it asked for are the result
            band["memory_error"] = str(e)
            mesh = None
        if mesh is not None:
            print(f"[device] poisson_band done {ms}", file=sys.stderr, flush=True)
            stages = stages[args.warmup:]
            stage_ms = {k: mean([t[k] for t in stages]) for k in stages[0]}
            levels = []
            for lv in rec["levels"]:
                l, nodes = lv["level"], 512 * lv["node_blocks"]
                sweeps_ms = stage_ms[f"L{l}_sweeps_ms"]
                model = 24 * nodes * rec["sweeps"]            # u and f read, u written, per stored node and sweep
                levels.append({**lv, **{k: stage_ms[f"L{l}_{k}_ms"] for k in ("nodes", "splat", "divergence", "prolong", "sweeps")},
                               "stored_nodes": nodes, "smooth_model_bytes": model,
                               "smooth_model_tb_per_s": model / (sweeps_ms * 1e-3) / 1e12 if sweeps_ms > 0 else None})
            loops, ms_loops = timed(lambda: MS.boundary_loops(mesh, 30))
            thr = MS.quantile(mesh.densities, 0.02)
            trimmed = MS.remove_vertices_by_mask(mesh, mesh.densities < thr)
            band.update({
                "device_ms": ms, "grid_ms": stage_ms["grid_ms"], "blocks_ms": stage_ms["blocks_ms"], "base_ms": stage_ms["base_ms"],
                "levels": levels, "iso_ms": stage_ms["iso_ms"], "extract_ms": stage_ms["extract_ms"],
                "what_is_timed": "device_ms: poisson_band with its allocations and two read-backs; the rest: HIP events; blocks_ms "
                                 "covers the block tables of every level and the first read-back, extract_ms the count, the second "
                                 "read-back, the allocation and the emit",
                "vertices": len(mesh.vertices), "triangles": len(mesh.triangles), "workspace_bytes": rec["workspace_bytes"],
                "dense_workspace_bytes_same_depth": 48 * ((1 << depth) + 1) ** 3,
                "open_boundary_edges": loops["boundary_edges"], "boundary_loops": loops, "boundary_loops_ms": mean(ms_loops),
                "vertices_after_trim": len(trimmed.vertices), "triangles_after_trim": len(trimmed.triangles),
                "open_boundary_edges_after_trim": MS.boundary_loops(trimmed, 30)["boundary_edges"]})
            del mesh, trimmed
        res["mesh_band"] = band
        if args.mesh_only and not args.mesh:
            print(json.dumps(res))
            return
    if args.mesh:
        from structured_light_for_3d_model_replication_amd import mesh as MS
        depth = int(args.mesh)
        src = CL.orient_normals_towards(CL.estimate_normals(pc, 5.0, 30), CL.centroid(pc), outward=True)
        stages = []

        def run():
            t = {}
            m = MS.poisson_grid(src, depth=depth, timings=t)
            stages.append(t)
            return m

        mesh, ms = timed(run)
        print(f"[device] poisson_grid done {ms}", file=sys.stderr, flush=True)
        stages = stages[args.warmup:]
        mean = lambda v: sum(v) / len(v)
        stage_ms = {k: mean([t[k] for t in stages]) for k in stages[0]}
        thr, ms_q = timed(lambda: MS.quantile(mesh.densities, 0.02))
        trimmed, ms_rm = timed(lambda: MS.remove_vertices_by_mask(mesh, mesh.densities < thr))
        _, ms_nrm = timed(lambda: MS.compute_triangle_normals(trimmed))
        _, ms_stl = timed(lambda: MS.stl_records(trimmed))
        nodes = ((1 << depth) + 1) ** 3
        model = MS.DEFAULT_CYCLES * nodes * (4 * 24 + 24 + 8 + 16) * 8 / 7
        res["mesh"] = {
            "depth": depth, "points": n, "cycles": MS.DEFAULT_CYCLES, "normal_radius": 5.0, "normal_max_nn": 30,
            "device_ms": ms, **{"stage_" + k: v for k, v in stage_ms.items()},
            "stage_quantile_ms": mean(ms_q), "stage_remove_ms": mean(ms_rm), "stage_triangle_normals_ms": mean(ms_nrm),
            "stage_stl_records_ms": mean(ms_stl),
            "what_is_timed": "device_ms: poisson_grid with its allocations and the header's read-back; stage_*: HIP events",
            "vertices": len(mesh.vertices), "triangles": len(mesh.triangles),
            "vertices_after_trim": len(trimmed.vertices), "triangles_after_trim": len(trimmed.triangles),
            "workspace_bytes": MS.workspace_bytes(depth, n),
            "solve_model_bytes": model, "solve_model_tb_per_s": model / (stage_ms["solve_ms"] * 1e-3) / 1e12}
        def audited(m):
            """mesh.audit of ``m``: the counts, the mean stage times and the five largest components."""
            stages_a = []

            def run_a():
                t = {}
                a = MS.audit(m, return_arrays=True, timings=t)
                stages_a.append(t)
                return a

            a, ms_a = timed(run_a)
            sizes = a.pop("sizes")
            for k in ("vertex_class", "triangle_class", "labels"):
                a.pop(k)
            nt = max(a["triangles"], 1)
            out = {"audit": a, "device_ms": ms_a, "line": MS.format_audit(a),
                   "largest_components": torch.sort(sizes, descending=True)[0][:5].tolist(),
                   "workspace_bytes": int(CL.N.lib().slg_audit_ws_bytes(CL.N.AUDIT_WS_AUDIT, max(a["vertices"], 1), nt))}
            for k in stages_a[args.warmup:][0] if a["triangles"] and a["vertices"] else ():
                out["stage_" + k] = mean([t[k] for t in stages_a[args.warmup:]])
            if "stage_edges_ms" in out and out["stage_edges_ms"] > 0:          # DESIGN.md §22's byte model of the edges step
                passes = -(-(32 + int(a["vertices"]).bit_length()) // 8)       # radix passes of 8 bits over the key's bits
                out["edges_sort_passes_assumed"] = passes
                out["edges_model_bytes"] = (98 + 72 * passes) * nt
                out["edges_model_tb_per_s"] = out["edges_model_bytes"] / (out["stage_edges_ms"] * 1e-3) / 1e12
            print(f"[device] audit: {out['line']}", file=sys.stderr, flush=True)
            return out

        def intersected(m):
            """mesh.self_intersections of ``m``: the counts, the mean stage times, the determinant rate."""
            stages_i = []

            def run_i():
                t = {}
                r = MS.self_intersections(m, return_pairs=True, return_arrays=True, timings=t)
                stages_i.append(t)
                return r

            r, ms_i = timed(run_i)
            for k in ("triangle_class", "pairs", "uncertain"):
                r.pop(k)
            out = {"record": r, "device_ms": ms_i, "line": MS.format_intersections(r), "vertices": len(m.vertices),
                   "triangles": len(m.triangles)}
            for k in stages_i[args.warmup:][0] if stages_i[args.warmup:] and stages_i[args.warmup:][0] else ():
                out["stage_" + k] = mean([t[k] for t in stages_i[args.warmup:]])
            if out.get("stage_test_ms", 0) > 0:                                # DESIGN.md §23's flop model of the test kernel
                out["test_model_flop"] = r["tested_pairs"] * 15 * 40
                out["test_model_tflop_per_s"] = out["test_model_flop"] / (out["stage_test_ms"] * 1e-3) / 1e12
                out["test_fraction_of_78_6_tflop_per_s"] = out["test_model_tflop_per_s"] / 78.6
            print(f"[device] intersections: {out['line']}", file=sys.stderr, flush=True)
            return out

        if args.intersect:
            res["mesh_intersect"] = {"what_is_timed": "device_ms: mesh.self_intersections(return_pairs=True, return_arrays=True) "
                                                      "with its allocations and three read-backs; stage_*: HIP events (boxes "
                                                      "holds the first read-back, candidates the second, test the third)",
                                     "view": intersected(trimmed)}
        if args.audit:
            aud = {"what_is_timed": "device_ms: mesh.audit(return_arrays=True) with its allocations and three read-backs; "
                                    "stage_*: HIP events (components holds the first read-back, measure the other two)",
                   "before_trim": audited(mesh), "after_trim": audited(trimmed)}
            (kept, krec), ms_keep = timed(lambda: MS.keep_largest_components(trimmed, 1, return_record=True))
            (cleaned, crec), ms_clean = timed(lambda: MS.clean(trimmed, return_record=True))
            aud.update(keep_largest_ms=ms_keep, keep_largest_record=krec, clean_ms=ms_clean, clean_record=crec)
            res["mesh_audit"] = aud
            del kept, cleaned
        if args.post:
            if args.post_trim != 0.02:
                trimmed = MS.remove_vertices_by_mask(mesh, mesh.densities < MS.quantile(mesh.densities, args.post_trim))
            if args.post_punch > 0:
                punch = (torch.arange(len(trimmed.vertices), device=trimmed.vertices.device) % args.post_punch) == args.post_punch // 2
                trimmed = MS.remove_vertices_by_mask(trimmed, punch)
            adj, ms_adj = timed(lambda: MS.vertex_adjacency(trimmed))
            _, ms_tau = timed(lambda: MS.smooth_taubin(trimmed, 10, adjacency=adj))
            loops, ms_loops = timed(lambda: MS.boundary_loops(trimmed, 30))
            closed, ms_close = timed(lambda: MS.close_holes(trimmed, 30))
            nv = len(trimmed.vertices)
            nb = int(adj.boundary.sum().item())
            # the rows the passes walk: the boundary row of a boundary vertex, the adjacency row otherwise
            deg_rows = (adj.offsets[1:] - adj.offsets[:-1])[adj.boundary == 0].sum().item() + len(adj.boundary_neighbours)
            deg = deg_rows / max(nv, 1)
            pass_bytes = nv * (24 * (deg + 1) + 4 * deg + 16 + 24)
            pass_ms = mean(ms_tau) / 20

            def passes_alone(count=200):          # the launches back to back on two buffers: no clone, no allocation
                lib, a, b = CL.N.lib(), trimmed.vertices.clone(), torch.empty_like(trimmed.vertices)
                for _ in range(count):
                    CL._raise(lib.slg_mesh_smooth_pass(E._vp(a), E._vp(b), nv, E._vp(adj.offsets), E._vp(adj.neighbours),
                                                       E._vp(adj.boundary), E._vp(adj.boundary_offsets),
                                                       E._vp(adj.boundary_neighbours), 1, 0.5, E._stream(None)))
                    a, b = b, a

            passes_alone(20)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            passes_alone(200)
            t1.record()
            t1.synchronize()
            alone_ms = t0.elapsed_time(t1) / 200
            res["mesh_post"] = {
                "trim_quantile": args.post_trim, "punch_every": args.post_punch, "vertices": nv, "triangles": len(trimmed.triangles),
                "adjacency_entries": len(adj.neighbours), "boundary_vertices": nb, "mean_row": deg,
                "adjacency_ms": ms_adj, "taubin10_ms": ms_tau, "boundary_loops_ms": ms_loops, "close_holes_ms": ms_close,
                "loops": loops, "triangles_after_close": len(closed.triangles),
                "what_is_timed": "HIP events around each call with its allocations and header read-backs; taubin10 "
                                 "includes the clone of the vertices and reuses the adjacency",
                "pass_model_bytes": pass_bytes, "pass_ms": pass_ms,
                "pass_model_tb_per_s": pass_bytes / (pass_ms * 1e-3) / 1e12 if pass_ms > 0 else None,
                "pass_fraction_of_8_tb_per_s": pass_bytes / (pass_ms * 1e-3) / 8e12 if pass_ms > 0 else None,
                "pass_alone_ms": alone_ms, "pass_alone_what": "200 launches back to back between two HIP events (includes one "
                                                              "clone of the vertices), divided by 200",
                "pass_alone_model_tb_per_s": pass_bytes / (alone_ms * 1e-3) / 1e12,
                "pass_alone_compulsory_tb_per_s": nv * (48 + 4 * deg + 17) / (alone_ms * 1e-3) / 1e12}
            if args.audit:
                res["mesh_audit"]["after_post"] = audited(closed)
                (cleaned, crec), ms_clean = timed(lambda: MS.clean(closed, return_record=True))
                res["mesh_audit"].update(clean_after_post_ms=ms_clean, clean_after_post_record=crec,
                                         after_post_clean=audited(cleaned))
                del cleaned
            if args.intersect:
                res["mesh_intersect"]["after_post"] = intersected(closed)
            if args.decimate is not None:
                rounds = []

                def run_dec():
                    rounds.clear()
                    return MS.decimate_quadric(closed, args.decimate, return_record=True, timings=rounds)

                (small, rec), ms_dec = timed(run_dec)
                print(f"[device] decimate_quadric done {ms_dec}", file=sys.stderr, flush=True)
                vin, tin = len(closed.vertices), len(closed.triangles)
                deg_all = len(adj.neighbours) / max(nv, 1)
                cands = sum(r["candidates"] for r in rounds)
                model = cands * (350 + 192 * deg_all)
                # read once: per vertex position, quadric, two offsets and the flag; per triangle its corners and
                # three incidence and three winding keys; per edge the key, two neighbour entries and the outputs
                compulsory = sum(r["triangles"] * (121 / 2 + 12 + 48) + r["candidates"] * (8 + 8 + 36) for r in rounds)
                dec = {"target": args.decimate, "vertices_in": vin, "triangles_in": tin, "vertices_out": len(small.vertices),
                       "triangles_out": len(small.triangles), "record": rec, "device_ms": ms_dec,
                       "what_is_timed": "HIP events around decimate_quadric with its allocations, one header read-back "
                                        "per round and the emit; rounds: the last call's, each round with its read-back",
                       "rounds": rounds, "round_first_ms": rounds[0]["ms"] if rounds else None,
                       "round_last_ms": rounds[-1]["ms"] if rounds else None,
                       "workspace_bytes": int(CL.N.lib().slg_mesh_decimate_ws_bytes(vin, tin)), "mean_valence": deg_all,
                       "eval_candidates_all_rounds": cands, "eval_model_bytes": model, "eval_compulsory_bytes": compulsory}
                if args.kernel_stats:
                    import csv
                    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "evaluate_kernel" in r.get("Name", "")]
                    calls = args.warmup + args.steps
                    if rows:
                        eval_ms = sum(float(r["TotalDurationNs"]) for r in rows) / calls * 1e-6
                        dec.update(eval_kernel_ms_per_call=eval_ms, eval_model_tb_per_s=model / (eval_ms * 1e-3) / 1e12,
                                   eval_compulsory_tb_per_s=compulsory / (eval_ms * 1e-3) / 1e12)
                res["mesh_decimate"] = dec
                if args.intersect:
                    res["mesh_intersect"]["after_decimate"] = intersected(small)
                del small
            del adj, closed
        del mesh, trimmed
        if args.mesh_only:
            print(json.dumps(res))
            return
    if args.orient:
        import orient_ref as OR
        NAT = CL.N
        k = int(args.orient)
        nr, nk = float(args.orient_normals[0]), int(args.orient_normals[1])

        def half_negated(cloud):
            nrm = cloud.normals.clone()
            flip = torch.from_numpy(np.random.default_rng(args.seed).random(len(cloud)) < 0.5).to(nrm.device)
            nrm[flip] = -nrm[flip]
            return CL.PointCloud(cloud.xyz, cloud.bgr, normals=nrm)

        with_n = CL.estimate_normals(pc, nr, nk)
        src = half_negated(with_n)
        _, ms_lists = timed(lambda: CL.knn_lists_raw(src, k))
        print(f"[device] lists done {ms_lists}", file=sys.stderr, flush=True)
        _, ms_emst = timed(lambda: CL.euclidean_mst(src, list_k=k))
        print(f"[device] EMST done {ms_emst}", file=sys.stderr, flush=True)
        (out, tree, root, info), ms = timed(lambda: CL.orient_normals_consistent_tangent_plane(src, k, return_tree=True))
        print(f"[device] orientation done {ms}", file=sys.stderr, flush=True)
        st = info["stats"]
        mean = lambda v: sum(v) / len(v)
        rounds = int(st[NAT.ORIENT_STAT_EMST_ROUNDS])
        plain = CL.orient_normals_consistent_tangent_plane(with_n, k)
        res["orient"] = {
            "k": k, "normal_radius": nr, "normal_max_nn": nk, "seed": args.seed, "points": n,
            "device_ms": ms, "device_lists_ms": ms_lists, "device_lists_and_emst_ms": ms_emst,
            "stage_lists_ms": mean(ms_lists), "stage_emst_ms": mean(ms_emst) - mean(ms_lists),
            "stage_tree_and_signs_ms": mean(ms) - mean(ms_emst),
            "what_is_timed": "each line: the call with its output allocation, edge sort, status and counter read-back",
            "emst_rounds": rounds, "tree_rounds": int(st[NAT.ORIENT_STAT_TREE_ROUNDS]),
            "lists_whole_cloud_points": int(st[NAT.ORIENT_STAT_LIST_FAR]),
            "walked_per_round": st[NAT.ORIENT_STAT_ROUND_WALKED:NAT.ORIENT_STAT_ROUND_WALKED + rounds].tolist(),
            "far_per_round": st[NAT.ORIENT_STAT_ROUND_FAR:NAT.ORIENT_STAT_ROUND_FAR + rounds].tolist(),
            "largest_sat_out_per_round": st[NAT.ORIENT_STAT_ROUND_SAT_OUT:NAT.ORIENT_STAT_ROUND_SAT_OUT + rounds].tolist(),
            "root": root, "negated": int((out.normals[:, 0] != src.normals[:, 0]).sum().item()),
            "equal_to_the_run_without_negation": bool(torch.equal(out.normals, plain.normals)),
            "workspace_bytes": int(NAT.lib().slg_orient_ws_bytes(n, k))}
        if not args.no_cpu:
            voxel, small = 0.0, pc
            while len(small) > args.orient_cpu_points:
                voxel = 1.0 if voxel == 0.0 else voxel * 1.25
                small = CL.voxel_down_sample(pc, voxel)
            small = half_negated(CL.estimate_normals(small, max(nr, 2.5 * voxel), nk))
            (s_out, s_tree, s_root, s_info), s_ms = timed(
                lambda: CL.orient_normals_consistent_tangent_plane(small, k, return_tree=True))
            P, Nrm = small.xyz.cpu().numpy(), small.normals.cpu().numpy()
            t0 = time.perf_counter()
            want, w_tree, w_root, w_emst, _ = OR.orient(P, Nrm, k, emst=OR.emst_delaunay(P))
            cpu_ms = (time.perf_counter() - t0) * 1e3
            same = {"emst": bool(np.array_equal(s_info["emst"].cpu().numpy(), w_emst)),
                    "tree": bool(np.array_equal(s_tree.cpu().numpy(), w_tree)), "root": s_root == w_root,
                    "normals": bool(np.array_equal(s_out.normals.cpu().numpy().view(np.uint64), want.view(np.uint64)))}
            res["orient"].update({
                "cpu_points": len(small), "cpu_voxel": voxel, "cpu_ms": cpu_ms, "device_ms_at_cpu_points": s_ms,
                "cpu_what": "tests/orient_ref.py: brute-force lists, Kruskal over scipy Delaunay candidates and over the "
                            "Riemannian edges, queue traversal (one thread)",
                "equal_cpu": same, "speedup_vs_cpu_at_cpu_points": cpu_ms / mean(s_ms)})
            assert all(same.values()), f"the device and the Delaunay-based restatement differ: {same}"
        if args.orient_only:
            print(json.dumps(res))
            return
    if args.plane:
        import plane_ref as PR
        d = float(args.plane[0])
        iters = int(args.plane[1]) if len(args.plane) > 1 else 1000
        P0, C0 = pc.numpy()
        nrm = np.array(PR.WALL_NORMAL) / np.linalg.norm(PR.WALL_NORMAL)
        along = (P0 - P0.mean(0)) @ nrm
        side = int(np.sqrt(n))
        pitch = float(np.ptp(P0, axis=0).max()) / side
        P, wall = PR.plant_wall(P0, behind=float(along.max()) + 4.0 * d, grid=(side, side), pitch=pitch, jitter=0.5 * d)
        wpc = CL.PointCloud(P, np.concatenate([C0, np.full((int(wall.sum()), 3), 200, np.uint8)]))
        nw, dev = len(wpc), wpc.xyz.device
        L, B = CL.N.lib(), CL.PLANE_BATCH
        ws = CL._workspace(dev, L.slg_plane_ws_bytes(nw, B))
        recs = torch.empty((B, CL.N.PLANE_RECORD_STRIDE), dtype=torch.float64, device=dev)

        def launch():                                        # the batch's three kernels, no read-back
            CL._raise(L.slg_plane_batch(E._vp(wpc.xyz), nw, d, 3, args.seed, 0, B, E._vp(ws), ws.numel(), E._vp(recs),
                                        E._stream(None)))
        _, ms_launch = timed(launch)
        _, ms_batch = timed(lambda: CL.plane_batch(wpc, d, 0, B, 3, args.seed))
        seg, ms = timed(lambda: CL.segment_plane(wpc, d, 3, iters, seed=args.seed))
        _, ms_finish = timed(lambda: CL.plane_finish(wpc, seg.sample_plane, d))
        (obj, _), ms_remove = timed(lambda: CL.remove_plane(wpc, d, 3, iters, seed=args.seed))
        evals = float(B) * nw
        mean_launch = sum(ms_launch) / args.steps
        res["plane"] = {
            "dist": d, "num_iterations": iters, "seed": args.seed, "points": nw, "wall_points": int(wall.sum()), "batch": B,
            "device_segment_ms": ms, "device_batch_launch_ms": ms_launch, "device_batch_with_readback_ms": ms_batch,
            "device_finish_ms": ms_finish, "device_remove_plane_ms": ms_remove,
            "winner_trial": seg.trial, "K": seg.iterations, "fitness": seg.fitness, "inliers": len(seg.inliers),
            "inliers_are_the_wall": bool(np.array_equal(seg.inliers.cpu().numpy(), np.flatnonzero(wall))),
            "remaining": len(obj), "plane": seg.plane_model.tolist(),
            # per evaluation: 3 mul + 3 add for the distance, 1 add for err (|.|, the compare, the select and the
            # integer count are not floating-point operations)
            "evaluations_per_batch": evals, "fp64_ops_per_evaluation": 7,
            "evaluations_per_s_from_batch_launch": evals / (mean_launch * 1e-3),
            "fp64_tflops_from_batch_launch": 7.0 * evals / (mean_launch * 1e-3) / 1e12}
        if not args.no_cpu:
            t0 = time.perf_counter()
            ref = PR.segment(P, d, 3, iters, seed=args.seed, workers=args.workers)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            res["plane"].update({
                "cpu_ms": cpu_ms, "cpu_what": f"tests/plane_ref.py segment, {args.workers} threads",
                "winner_and_K_equal_cpu": bool((ref["trial"], ref["K"]) == (seg.trial, seg.iterations)),
                "records_equal_cpu": bool(np.array_equal(np.stack(ref["records"]).view(np.uint64), seg.log.view(np.uint64))),
                "inliers_equal_cpu": bool(np.array_equal(ref["inliers"], seg.inliers.cpu().numpy())),
                "speedup_vs_cpu": cpu_ms / (sum(ms) / args.steps)})
        if args.plane_only:
            print(json.dumps(res))
            return
    if args.icp:
        import icp_ref as IR
        d = float(args.icp)
        tgt = CL.estimate_normals(pc, 2 * d, 30)
        P = pc.xyz.cpu().numpy()
        reach = float(np.linalg.norm(P - P.mean(0), axis=1).max())
        angles = np.degrees(0.3 * d / reach) * np.array([1.0, -1.5, 0.7]) / 1.5
        T_true = IR.motion_about(P.mean(0), angles, d * np.array([0.2, -0.15, 0.1]))
        src = CL.transform(CL.PointCloud(pc.xyz, pc.bgr), IR.inverse_rigid(T_true))
        reg, ms = timed(lambda: CL.registration_icp(src, tgt, d))
        _, ms_eval = timed(lambda: CL.evaluate_registration(src, tgt, d))
        S = src.xyz.cpu().numpy()
        res["icp"] = {"dist": d, "normal_radius": 2 * d, "source_points": len(src), "target_points": len(tgt),
                      "device_ms": ms, "device_evaluate_only_ms": ms_eval, "iterations": reg.iterations,
                      "converged": reg.converged, "fitness": reg.fitness, "inlier_rmse": reg.inlier_rmse,
                      "whole_target_queries": CL.far_count(pc.xyz.device),
                      "motion_error": IR.motion_error(reg.transformation, T_true, S)}
        if not args.no_cpu:
            nrm = tgt.normals.cpu().numpy()
            t0 = time.perf_counter()
            ref = IR.registration_icp(S, P, nrm, d, workers=args.workers)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            at_dev = IR.evaluate(S, P, reg.transformation, d, workers=args.workers)["corr"]
            i = np.flatnonzero(at_dev >= 0)
            res["icp"].update({
                "cpu_ms": cpu_ms, "cpu_what": f"tests/icp_ref.py, scipy cKDTree(workers={args.workers})",
                "iterations_equal_cpu": bool(ref["iterations"] == reg.iterations and ref["converged"] == reg.converged),
                "correspondences_equal_cpu": bool(np.array_equal(reg.correspondence_set.cpu().numpy(),
                                                                 np.stack([i, at_dev[i].astype(np.int64)], 1))),
                "max_transform_difference_cpu": float(np.abs(ref["T"] - reg.transformation).max()),
                "speedup_vs_cpu": cpu_ms / (sum(ms) / args.steps)})
        if args.icp_only:
            print(json.dumps(res))
            return
    if args.global_reg and not args.fpfh:
        raise SystemExit("--global-reg needs --fpfh RADIUS MAX_NN")
    if args.fpfh:
        import feature_ref as FR
        import icp_ref as IR
        import normals_ref as NR
        fr, fk = float(args.fpfh[0]), int(args.fpfh[1])
        tgt = CL.estimate_normals(pc, 0.4 * fr, 30)
        (ft, _, fm), ms = timed(lambda: CL.fpfh_features(tgt, fr, fk))
        print(f"[device] fpfh done {ms}", file=sys.stderr, flush=True)
        res["fpfh"] = {"radius": fr, "max_nn": fk, "normal_radius": 0.4 * fr, "device_ms": ms,
                       "whole_cloud_points": CL.far_count(pc.xyz.device), "capped": float((fm == fk).double().mean().item()),
                       "alone": int((fm <= 1).sum().item()),
                       "workspace_bytes": int(CL.N.lib().slg_fpfh_ws_bytes(n, fk))}
        P = pc.xyz.cpu().numpy()
        d = float(args.global_reg) if args.global_reg else 0.0
        T_true = IR.motion_about(P.mean(0), FR.BASE_ANGLES_DEG, 5.0 * d * np.array([1.0, -0.7, 0.4]))
        part = torch.from_numpy((np.arange(n) % 3 != 1) & (P[:, 0] > np.quantile(P[:, 0], 0.2))).to(pc.xyz.device)
        moved = CL.transform(CL.PointCloud(pc.xyz[part], pc.bgr[part]), IR.inverse_rigid(T_true))
        src = CL.estimate_normals(moved, 0.4 * fr, 30)
        fs = CL.compute_fpfh_feature(src, fr, fk)
        (pairs, nn_s, nn_t), ms = timed(lambda: CL.feature_nearest(fs, ft, True))
        mean_ms = sum(ms) / args.steps
        print(f"[device] match done {ms}", file=sys.stderr, flush=True)
        res["match"] = {"source_rows": len(src), "target_rows": n, "mutual_pairs": len(pairs), "device_ms": ms,
                        "fp64_ops": 2 * 66.0 * len(src) * n, "fp64_tflops": 2 * 66.0 * len(src) * n / (mean_ms * 1e-3) / 1e12}
        if args.global_reg:
            reg, ms = timed(lambda: CL.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, d, seed=args.seed))
            S = src.xyz.cpu().numpy()
            print(f"[device] global registration done {ms}", file=sys.stderr, flush=True)
            res["global_reg"] = {"dist": d, "seed": args.seed, "device_ms": ms, "winner_trial": reg.trial, "K": reg.iterations,
                                 "evaluated_trials": len(reg.log), "fitness": reg.fitness, "inlier_rmse": reg.inlier_rmse,
                                 "whole_target_queries": CL.far_count(pc.xyz.device),
                                 "motion_error": IR.motion_error(reg.transformation, T_true, S)}
        if not args.no_cpu:
            N_t = tgt.normals.cpu().numpy()
            t0 = time.perf_counter()
            idx, dd, resolved = NR.neighbour_lists_tree(P, fk, workers=args.workers)
            ref = FR.compute_fpfh(P, N_t, fr, fk, (idx, dd))
            cpu_ms = (time.perf_counter() - t0) * 1e3
            # a point's feature needs its own list and its neighbours' lists resolved
            ok = resolved & np.all(resolved[ref["idx"]] | ~ref["inside"], axis=1)
            dft = ft.cpu().numpy()
            res["fpfh"].update({
                "cpu_ms": cpu_ms, "cpu_what": f"tests/feature_ref.py, lists proposed by scipy cKDTree(workers={args.workers})",
                "unresolved_ties_cpu": int((~ok).sum()), "edge_bin_pairs_cpu": ref["edge_pairs"],
                "m_equal_cpu": bool(np.array_equal(fm.cpu().numpy()[resolved], ref["m"][resolved])),
                "fpfh_equal_cpu": bool(np.array_equal(dft[ok].view(np.uint64), ref["fpfh"][ok].view(np.uint64))),
                "rows_differing_cpu": int((dft[ok] != ref["fpfh"][ok]).any(1).sum()),
                "speedup_vs_cpu": cpu_ms / (sum(res["fpfh"]["device_ms"]) / args.steps)})
            print("[cpu] fpfh done", file=sys.stderr, flush=True)
            dfs = fs.cpu().numpy()
            rows = np.linspace(0, len(dfs) - 1, min(args.match_sample, len(dfs))).astype(np.int64)
            t0 = time.perf_counter()
            want = FR.nearest_rows_brute(dfs[rows], dft)
            res["match"].update({"cpu_sample_rows": len(rows), "cpu_sample_ms": (time.perf_counter() - t0) * 1e3,
                                 "sample_equal_cpu": bool(np.array_equal(nn_s.cpu().numpy()[rows], want))})
            if args.global_reg:
                t0 = time.perf_counter()
                rr = FR.ransac(S, P, pairs.cpu().numpy(), d, seed=args.seed, workers=args.workers)
                cpu_ms = (time.perf_counter() - t0) * 1e3
                res["global_reg"].update({
                    "cpu_ms": cpu_ms, "cpu_what": "tests/feature_ref.py ransac on the device's correspondences",
                    "winner_and_K_equal_cpu": bool((rr["trial"], rr["K"]) == (reg.trial, reg.iterations)),
                    "max_transform_difference_cpu": float(np.abs(rr["T"] - reg.transformation).max()),
                    "speedup_vs_cpu": cpu_ms / (sum(res["global_reg"]["device_ms"]) / args.steps)})
        if args.gr_only:
            print(json.dumps(res))
            return
    (rad, rad_idx), ms = timed(lambda: CL.radius_outlier(pc, 100, 5.0, return_index=True))
    res["radius"] = {"nb_points": 100, "radius": 5.0, "kept": len(rad), "device_ms": ms}
    (_, counts), ms = timed(lambda: CL.radius_mask(pc.xyz, 100, 5.0))
    res["radius"]["device_mask_only_ms"] = ms
    res["radius"]["mean_candidates_in_radius"] = float(counts.double().mean().item())
    (sta, sta_idx), ms = timed(lambda: CL.statistical_outlier(pc, 20, 2.0, return_index=True))
    res["statistical"] = {"nb_neighbors": 20, "std_ratio": 2.0, "kept": len(sta), "device_ms": ms,
                          "whole_cloud_points": CL.far_count(pc.xyz.device)}
    _, ms = timed(lambda: CL.statistical_mask(pc.xyz, 20, 2.0))
    res["statistical"]["device_mask_only_ms"] = ms
    if args.voxel:
        (vox, vfirst, vcount), ms = timed(lambda: CL.voxel_down_sample(pc, args.voxel, return_index=True))
        res["voxel"] = {"voxel_size": args.voxel, "voxels": len(vox), "largest": int(vcount.max().item()),
                        "device_ms": ms}
    if args.normals:
        nr, nk = float(args.normals[0]), int(args.normals[1])
        (ncov, nm, nnrm), ms = timed(lambda: CL.normal_covariances(pc.xyz, nr, nk))
        res["normals"] = {"radius": nr, "max_nn": nk, "device_ms": ms, "whole_cloud_points": CL.far_count(pc.xyz.device),
                          "capped": float((nm == nk).double().mean().item()),
                          "fewer_than_3": int((nm < 3).sum().item())}
        _, ms_s = timed(lambda: CL.statistical_mask(pc.xyz, nk, 2.0))
        res["normals"]["statistical_mask_same_k_ms"] = ms_s
        res["normals"]["ratio_to_statistical_mask"] = sum(ms) / sum(ms_s)
    clusters = {} if args.skip_cluster else {"cluster": (5.0, 200), "cluster_multi": tuple(args.cluster_multi)}
    labels = {}
    for name, (eps, mp) in clusters.items():
        (big, _), ms = timed(lambda: CL.largest_cluster(pc, eps, int(mp), return_index=True))
        (labels[name], _, info), ms_l = timed(lambda: CL.dbscan_labels(pc.xyz, eps, int(mp)))
        info = info.cpu().tolist()
        res[name] = {"eps": eps, "min_points": int(mp), "kept": len(big), "clusters": info[0], "largest_label": info[1],
                     "largest_count": info[2], "noise": info[3], "device_ms": ms, "device_labels_only_ms": ms_l}

    if not args.no_cpu:
        import cloud_ref as R
        P = pc.xyz.cpu().numpy()
        t0 = time.perf_counter()
        keep_r, _ = R.radius_filter(P, 100, 5.0, workers=args.workers)
        t1 = time.perf_counter()
        keep_s, _, _ = R.statistical_filter(P, 20, 2.0, workers=args.workers)
        t2 = time.perf_counter()
        res["cpu"] = {"what": f"tests/cloud_ref.py, scipy cKDTree(workers={args.workers})",
                      "radius_ms": (t1 - t0) * 1e3, "statistical_ms": (t2 - t1) * 1e3}
        if args.voxel or args.normals:
            import normals_ref as NR
            C = pc.bgr.cpu().numpy()

            def same(a, b):
                return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))
        if args.voxel:
            t0 = time.perf_counter()
            pts, col, first, count = NR.voxel_down_sample(P, C, args.voxel)
            res["cpu"]["voxel_ms"] = (time.perf_counter() - t0) * 1e3
            Pv, Cv = vox.numpy()
            res["voxel"]["equal_cpu"] = bool(len(Pv) == len(pts) and same(Pv, pts) and np.array_equal(Cv, col)
                                             and np.array_equal(vfirst.cpu().numpy(), first)
                                             and np.array_equal(vcount.cpu().numpy(), count))
            res["voxel"]["speedup_vs_cpu"] = res["cpu"]["voxel_ms"] / (sum(res["voxel"]["device_ms"]) / args.steps)
        if args.normals:
            t0 = time.perf_counter()
            idx, dd, resolved = NR.neighbour_lists_tree(P, nk, workers=args.workers)
            cov, m, nrm = NR.estimate_normals(P, nr, nk, (idx, dd))
            res["cpu"]["normals_ms"] = (time.perf_counter() - t0) * 1e3
            dcov, dm, dn = ncov.cpu().numpy(), nm.cpu().numpy(), nnrm.cpu().numpy()
            ok = resolved & (m >= 3) & cov.any(1)
            res["normals"].update({
                "unresolved_ties_cpu": int((~resolved).sum()),
                "m_equal_cpu": bool(np.array_equal(dm[resolved], m[resolved])),
                "cov_equal_cpu": same(dcov[resolved], cov[resolved]),
                "normals_equal_cpu": same(dn[resolved], nrm[resolved]),
                "max_rayleigh_excess": float(NR.rayleigh_excess(cov[ok], dn[ok]).max()) if ok.any() else 0.0,
                "speedup_vs_cpu": res["cpu"]["normals_ms"] / (sum(res["normals"]["device_ms"]) / args.steps)})
        import cluster_ref as CR
        for name, (eps, mp) in clusters.items():
            t0 = time.perf_counter()
            ref = CR.closed_labels_blocked(P, eps, int(mp), workers=args.workers)
            res["cpu"][name + "_ms"] = (time.perf_counter() - t0) * 1e3
            print(f"[cpu] {name} done", file=sys.stderr, flush=True)
            res[name]["labels_equal_cpu"] = bool(np.array_equal(labels[name].cpu().numpy(), ref))
            res[name]["speedup_vs_cpu"] = res["cpu"][name + "_ms"] / (sum(res[name]["device_ms"]) / args.steps)
        res["cpu"]["cluster_what"] = (f"tests/cluster_ref.py closed_labels_blocked, scipy cKDTree(workers={args.workers}) "
                                      "+ csgraph.connected_components")
        res["radius"]["mask_equal_cpu"] = bool(np.array_equal(rad_idx.cpu().numpy(), np.flatnonzero(keep_r)))
        res["statistical"]["mask_equal_cpu"] = bool(np.array_equal(sta_idx.cpu().numpy(), np.flatnonzero(keep_s)))
        res["radius"]["speedup_vs_cpu"] = res["cpu"]["radius_ms"] / (sum(res["radius"]["device_ms"]) / args.steps)
        res["statistical"]["speedup_vs_cpu"] = (res["cpu"]["statistical_ms"]
                                                / (sum(res["statistical"]["device_ms"]) / args.steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
