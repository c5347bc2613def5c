"""The mesh audit reads no stale memory (DESIGN.md sections 18 and 22): mesh.audit, mesh.clean and
mesh.keep_largest_components under the three fills of tests/stale_memory.py, by the plumbing of
tests/test_gpu_stale_memory.py.  The 0x00 run is compared with the restatement exactly as
tests/test_gpu_audit.py does; the "stale" and 0xFF runs must equal it bit for bit, every array
included.  Before every run the same step refuses a mesh of the same size with a bad index in it, so
what a refused call leaves behind is part of the poison.

tests/test_audit_cover.py maps every export of the audit table to a case of this file."""
import numpy as np
import pytest

import audit_ref as A
from test_gpu_audit import ARRAYS, built, check_audit, device_mesh, host, ref_audit
from test_gpu_stale_memory import three_fills

pytestmark = pytest.mark.gpu

CASES = {"big": "strip20000_shuffled", "book": "book80", "one": "single_triangle"}


@pytest.fixture(scope="module")
def MS():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


def refused(MS, fn, name):
    V, T = built(name)
    T = T.copy()
    T[len(T) // 2, 2] = len(V)
    with pytest.raises(IndexError):
        fn(device_mesh(MS, V, T, np.arange(float(len(V)))))


def test_audit(MS):
    """edges, components (count and emit), fans and measure at 20,000, 85 and 1 triangles."""
    def step(case):
        name = CASES[case]
        refused(MS, lambda m: MS.audit(m, return_arrays=True), name)
        a = MS.audit(device_mesh(MS, *built(name)), return_arrays=True)
        arrays = [host(a.pop(k)) for k, _ in ARRAYS]
        return [dict(a), np.float64(a["signed_volume"]), np.float64(a["area"]), *arrays]

    def check_first(case, res):
        got = dict(res[0], **{k: _Dev(v) for (k, _), v in zip(ARRAYS, res[3:])})
        check_audit(got, ref_audit(CASES[case]), case)

    three_fills(step, ("big", "book", "one"), check_first)


class _Dev:
    """A host array behind the ``.cpu().numpy()`` that check_audit asks of a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_clean_and_keep(MS):
    """edges, keep (by class bits and by a component table) and select, with densities."""
    def step(case):
        name = CASES[case]
        V, T = built(name)
        D = np.arange(float(len(V)))
        refused(MS, MS.clean, name)
        c, crec = MS.clean(device_mesh(MS, V, T, D), return_record=True)
        refused(MS, MS.keep_largest_components, name)
        k, krec = MS.keep_largest_components(device_mesh(MS, V, T, D), 1, return_record=True)
        u = MS.clean(device_mesh(MS, V, T, D), unreferenced=False)
        return [host(c.vertices), host(c.triangles), host(c.densities), crec, host(k.vertices), host(k.triangles),
                host(k.densities), krec, host(u.vertices), host(u.triangles)]

    def check_first(case, res):
        V, T = built(CASES[case])
        D = np.arange(float(len(V)))
        for got, want in ((res[0:4], A.clean(V, T, D)), (res[4:8], A.keep_largest_components(V, T, D, 1))):
            assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])
            assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64)) and got[3] == want[3]
        Vu, Tu, _, _ = A.clean(V, T, None, unreferenced=False)
        assert np.array_equal(res[8].view(np.uint64), Vu.view(np.uint64)) and np.array_equal(res[9], Tu)

    three_fills(step, ("big", "book", "one"), check_first)
