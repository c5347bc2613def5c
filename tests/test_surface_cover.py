"""Every export of the surface table (``_native.SURFACE_EXPORTS``, include/slgpu_surface.h) is
mapped to the case of tests/test_gpu_surface_stale.py that runs it under the three fills of
tests/stale_memory.py, or to the reason none does: what tests/test_stale_memory_cover.py keeps for
the first table, kept here for the second until the two are folded together."""
import ast
import os

import stale_memory as SM

COVER = {
    "slg_surface_ws_bytes": SM.SIZING,
    "slg_surface_begin": "test_ball_pivot",
    "slg_surface_count": "test_ball_pivot",
    "slg_surface_emit": "test_ball_pivot",
    "slg_surface_round": "test_ball_pivot",
    "slg_surface_commit": "test_ball_pivot",
}


def test_every_surface_export_is_covered():
    from structured_light_for_3d_model_replication_amd import _native as N
    assert set(COVER) == set(N.SURFACE_EXPORTS)
    assert not set(COVER) & set(SM.COVER)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_surface_stale.py")
    cases = {n.name for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for name, where in COVER.items():
        assert where in cases or where in SM.REASONS, name
        if name.endswith("_ws_bytes"):
            assert where == SM.SIZING, name


def test_the_case_calls_what_it_covers():
    """The covered case goes through mesh.ball_pivot, and that names every covered export."""
    import inspect
    from structured_light_for_3d_model_replication_amd import mesh as MS
    src = inspect.getsource(MS.ball_pivot)
    for name, where in COVER.items():
        assert f"lib.{name}(" in src, name
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_surface_stale.py")
    assert "MS.ball_pivot(" in open(path).read()
