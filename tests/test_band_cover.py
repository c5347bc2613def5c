"""Every export of the band table (``_native.BAND_EXPORTS``, include/slgpu_band.h) is mapped to the
case of tests/test_gpu_band_stale.py that runs it under the three fills of tests/stale_memory.py, or
to the reason none does: what tests/test_stale_memory_cover.py keeps for the first table and
tests/test_surface_cover.py for the second, kept here for the third."""
import ast
import os

import stale_memory as SM
import test_surface_cover as SC

COVER = {
    "slg_band_ws_bytes": SM.SIZING,
    "slg_band_level": "test_poisson_band",
    "slg_band_blocks": "test_poisson_band",
    "slg_band_nodes": "test_poisson_band",
    "slg_band_splat": "test_poisson_band",
    "slg_band_divergence": "test_poisson_band",
    "slg_band_prolong": "test_poisson_band",
    "slg_band_smooth": "test_poisson_band",
    "slg_band_iso": "test_poisson_band",
    "slg_band_count": "test_poisson_band",
    "slg_band_emit": "test_poisson_band",
}
STALE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_band_stale.py")


def test_every_band_export_is_covered():
    from structured_light_for_3d_model_replication_amd import _native as N
    assert set(COVER) == set(N.BAND_EXPORTS)
    assert not set(COVER) & (set(SM.COVER) | set(SC.COVER))
    cases = {n.name for n in ast.parse(open(STALE).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for name, where in COVER.items():
        assert where in cases or where in SM.REASONS, name
        if name.endswith("_ws_bytes"):
            assert where == SM.SIZING, name


def test_the_case_calls_what_it_covers():
    """The covered case goes through mesh.poisson_band, and that names every covered export (the
    sizing call through its helper)."""
    import inspect
    from structured_light_for_3d_model_replication_amd import mesh as MS
    src = inspect.getsource(MS.poisson_band)
    for name, where in COVER.items():
        if where != SM.SIZING:
            assert f"lib.{name}(" in src, name
    assert "lib().slg_band_ws_bytes(" in inspect.getsource(MS._band_ws_bytes) and "_band_ws_bytes(" in src
    assert "MS.poisson_band(" in open(STALE).read()
    # both parents of the cascade and both ping-pong buffers are among the cases
    from test_gpu_band_stale import CASES
    assert any(d - b >= 2 for _, d, b, _ in CASES.values()) and {s & 1 for *_, s in CASES.values()} == {0, 1}
