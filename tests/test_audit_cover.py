"""Every export of the audit table (``_native.AUDIT_EXPORTS``, include/slgpu_audit.h) is mapped to the
case of tests/test_gpu_audit_stale.py that runs it under the three fills of tests/stale_memory.py, or
to the reason none does: what tests/test_stale_memory_cover.py keeps for the first table,
tests/test_surface_cover.py for the second and tests/test_band_cover.py for the third, kept here for
the fourth."""
import ast
import os

import stale_memory as SM
import test_band_cover as BC
import test_surface_cover as SC

COVER = {
    "slg_audit_ws_bytes": SM.SIZING,
    "slg_audit_edges": "test_audit",
    "slg_audit_components_count": "test_audit",
    "slg_audit_components_emit": "test_audit",
    "slg_audit_fans": "test_audit",
    "slg_audit_measure": "test_audit",
    "slg_audit_keep": "test_clean_and_keep",
    "slg_audit_select": "test_clean_and_keep",
}
STALE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_audit_stale.py")


def test_every_audit_export_is_covered():
    from structured_light_for_3d_model_replication_amd import _native as N
    assert set(COVER) == set(N.AUDIT_EXPORTS)
    assert not set(COVER) & (set(SM.COVER) | set(SC.COVER) | set(BC.COVER))
    cases = {n.name for n in ast.parse(open(STALE).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for name, where in COVER.items():
        assert where in cases or where in SM.REASONS, name
        if name.endswith("_ws_bytes"):
            assert where == SM.SIZING, name


def test_the_cases_call_what_they_cover():
    """test_audit goes through mesh.audit, test_clean_and_keep through mesh.clean and
    mesh.keep_largest_components, and those name every covered export (the sizing call through its
    helper)."""
    import inspect
    from structured_light_for_3d_model_replication_amd import mesh as MS
    audit = inspect.getsource(MS._audit)
    select = inspect.getsource(MS.clean) + inspect.getsource(MS._keep_components) + inspect.getsource(MS._select)
    for name, where in COVER.items():
        if where != SM.SIZING:
            assert f"lib.{name}(" in (audit if where == "test_audit" else select).replace("lib().", "lib."), name
    assert "lib().slg_audit_ws_bytes(" in inspect.getsource(MS._audit_ws) and "_audit_ws(" in audit and "_audit_ws(" in select
    assert "_audit(mesh" in inspect.getsource(MS.audit) and "_keep_components(" in inspect.getsource(MS.keep_largest_components)
    stale = open(STALE).read()
    assert "MS.audit(" in stale and "MS.clean(" in stale and "MS.keep_largest_components(" in stale
    # the long union-find chains, the run longer than a wavefront and the one-triangle mesh are among the cases
    from test_gpu_audit_stale import CASES
    assert set(CASES.values()) == {"strip20000_shuffled", "book80", "single_triangle"}
