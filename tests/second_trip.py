"""The ledger of capped loops (test helper), as ``stale_memory.COVER`` is for
the exports.

Every cloud, mesh and PLY step bounds some loop with a cap: a one-workgroup finaliser walks its
partials ``t, t + 256, ..``; a list kernel walks its list from ``blockIdx.x`` in strides of a grid
capped at 256, 1,024 or more workgroups; the cell walk is capped at 8,192 workgroups; the PLY offset
scan takes 1,024 chunks a trip.  A second trip reuses the thread's accumulator, the workgroup's LDS
or scratch, or a carry, and only an input past the cap takes it: 524,288 elements for a finaliser,
more list entries than workgroups, more occupied cells than workgroups, more than 1,024 x 1,024
points.

:data:`COVER` maps ``(source file under csrc/, kernel)`` to the case that takes the kernel's second
trip (a test of tests/test_gpu_second_trip.py, which asserts first that its input is past the cap),
or to one of the written :data:`REASONS` why none does.  tests/test_second_trip_cover.py keeps the
names true: a kernel that is renamed or removed, or a case that no longer exists, fails there
without a GPU.  A new capped loop belongs here with its case.
"""
REFERENCE_TOO_SLOW = "the host reference of an input past the cap takes many seconds"
LIBRARY = "rocPRIM's own loops: the library's, exercised at these sizes by every case here"
REASONS = (REFERENCE_TOO_SLOW, LIBRARY)

CASES = "test_gpu_second_trip"          # the module the named cases live in

COVER = {
    # finalisers: thread t sums the partials t, t + 256, ... (cap: 256 partials of 2,048 elements)
    ("cloud_grid.hip", "bbox_final_kernel"): "test_radius_filter_box",
    ("cloud_filter.hip", "sum_final_kernel"): "test_statistical_filter_finalisers",
    ("cloud_normals.hip", "axis_sum_final_kernel"): "test_centroid_tree",
    ("cloud_plane.hip", "plane_refit_final_kernel"): "test_plane_records_and_refit",
    ("cloud_icp.hip", "icp_solve_kernel"): "test_icp_sums",
    ("cloud_mesh.hip", "iso_final_kernel"): "test_mesh_iso_tree",
    ("cloud_band.hip", "iso_final_kernel"): "test_band_iso_tree",
    ("cloud_audit.hip", "measure_final_kernel"): "test_audit_measures",
    # list kernels: workgroup b takes the entries b, b + gridDim.x, ... (cap: 1,024 or 256 workgroups)
    ("cloud_filter.hip", "knn_far_kernel"): "test_far_knn_means",
    ("cloud_normals.hip", "normals_far_kernel"): "test_far_normals",
    ("cloud_normals.hip", "voxel_long_kernel"): "test_far_voxel_long_list",
    ("cloud_icp.hip", "icp_far_kernel"): "test_far_icp_correspondences",
    ("cloud_feature.hip", "fpfh_far_kernel"): "test_far_fpfh_lists",
    ("cloud_orient.hip", "orient_lists_far_kernel"): "test_far_knn_lists",
    ("cloud_grid.h", "lists_far_body"): "test_far_knn_lists",
    ("cloud_orient.hip", "emst_far_kernel"): REFERENCE_TOO_SLOW,          # cap 16,384: the brute EMST takes 8 s at 14,000 points
    ("cloud_surface.hip", "candidates_kernel"): REFERENCE_TOO_SLOW,       # cap 2^20 anchors: the reference takes 2 s at 14,000 points
    # the cell walk: workgroup b takes the occupied cells b, b + gridDim.x, ... (cap: 8,192 workgroups)
    ("cloud_grid.h", "cell_batches"): "test_cell_walk_radius_filter",
    ("cloud_filter.hip", "radius_count_kernel"): "test_cell_walk_radius_filter",
    ("cloud_cluster.hip", "dbscan_subcell_kernel"): "test_cell_walk_dbscan",
    ("cloud_cluster.hip", "dbscan_union_kernel"): "test_cell_walk_dbscan",
    ("cloud_cluster.hip", "dbscan_border_kernel"): "test_cell_walk_dbscan",
    # the RANSAC's evaluation: 32 rows and 256 workgroups over the passing trials
    ("cloud_ransac.hip", "ransac_eval_kernel"): "test_ransac_many_passing_trials",
    ("cloud_ransac.hip", "ransac_records_kernel"): "test_ransac_many_passing_trials",
    # the PLY offset scan: 1,024 chunks a trip, a carry between trips
    ("ply.hip", "ply_scan_kernel"): "test_ply_scan_second_trip",
    # the sorts and scans every grid build runs
    ("cloud_grid.hip", "rocprim::radix_sort_pairs"): LIBRARY,
    ("cloud_grid.hip", "rocprim::exclusive_scan"): LIBRARY,
}
