"""Every export of the C ABI is either run under the three fills of tests/stale_memory.py by a
named case of tests/test_gpu_stale_memory.py, or has one of a few written reasons why none does.
No GPU call: a new export forces a decision here, as test_cases_cover_the_instance_table does for
the fused kernel's instances."""
import stale_memory as SM


def test_every_export_is_covered_or_excused():
    from structured_light_for_3d_model_replication_amd import _native as N
    assert set(SM.COVER) == set(N.EXPORTS), (sorted(set(N.EXPORTS) - set(SM.COVER)), sorted(set(SM.COVER) - set(N.EXPORTS)))


def test_every_named_case_exists():
    import test_gpu_stale_memory as T
    cases = {v for v in SM.COVER.values() if v not in SM.REASONS}
    assert cases and all(v.startswith("test_") for v in cases)
    missing = sorted(c for c in cases if not callable(getattr(T, c, None)))
    assert not missing, missing
    assert T.pytestmark.name == "gpu"                     # the cases need the device; this file does not


def test_reasons_are_the_written_ones():
    assert SM.REASONS == ("no device memory", "sizing call", "fused workspace: zeroed by contract", "needs several GPUs")
    assert SM.FILLS == (0x00, "stale", 0xFF)             # the order the fills run in
    assert {v for v in SM.COVER.values() if not v.startswith("test_")} <= set(SM.REASONS)
