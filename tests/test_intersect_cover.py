"""Every export of the intersect table (``_native.INTERSECT_EXPORTS``, include/slgpu_intersect.h) is
mapped to the case of tests/test_gpu_intersect_stale.py that runs it under the three fills of
tests/stale_memory.py, or to the reason none does: what tests/test_audit_cover.py keeps for the fourth
table, kept here for the fifth."""
import ast
import os

import stale_memory as SM
import test_audit_cover as AC
import test_band_cover as BC
import test_surface_cover as SC

COVER = {
    "slg_isect_ws_bytes": SM.SIZING,
    "slg_isect_boxes": "test_self_intersections",
    "slg_isect_entries": "test_self_intersections",
    "slg_isect_candidates_count": "test_self_intersections",
    "slg_isect_candidates_emit": "test_self_intersections",
    "slg_isect_test": "test_self_intersections",
    "slg_isect_list": "test_self_intersections",
}
STALE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_intersect_stale.py")


def test_every_intersect_export_is_covered():
    from structured_light_for_3d_model_replication_amd import _native as N
    assert set(COVER) == set(N.INTERSECT_EXPORTS)
    assert not set(COVER) & (set(SM.COVER) | set(SC.COVER) | set(BC.COVER) | set(AC.COVER))
    cases = {n.name for n in ast.parse(open(STALE).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for name, where in COVER.items():
        assert where in cases or where in SM.REASONS, name
        if name.endswith("_ws_bytes"):
            assert where == SM.SIZING, name


def test_the_case_calls_what_it_covers():
    """test_self_intersections goes through mesh.self_intersections with the lists, which names every
    covered export (the sizing call through its helper)."""
    import inspect
    from structured_light_for_3d_model_replication_amd import mesh as MS
    src = (inspect.getsource(MS.self_intersections) + inspect.getsource(MS._isect_list)).replace("lib().", "lib.")
    for name, where in COVER.items():
        if where != SM.SIZING:
            assert f"lib.{name}(" in src, name
    assert "lib().slg_isect_ws_bytes(" in inspect.getsource(MS._isect_ws) and "_isect_ws(" in src
    stale = open(STALE).read()
    assert "MS.self_intersections(" in stale and "return_pairs=True" in stale and "return_arrays=True" in stale
    # the run that makes the tile loop's third trip, the large list and the one-triangle mesh are among the cases
    from test_gpu_intersect_stale import CASES
    assert set(CASES.values()) == {"run129", "large", "one_triangle"}
