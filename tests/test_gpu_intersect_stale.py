"""The self-intersection test reads no stale memory (DESIGN.md sections 18 and 23):
mesh.self_intersections with arrays and lists under the three fills of tests/stale_memory.py, by the
plumbing of tests/test_gpu_stale_memory.py.  The 0x00 run is compared with the restatement exactly as
tests/test_gpu_intersect.py does; the "stale" and 0xFF runs must equal it bit for bit, the grid's
informational counts and every array included.  Before every run the call refuses a mesh of the same
size with a bad index in it, so what a refused call leaves behind is part of the poison.

tests/test_intersect_cover.py maps every export of the intersect table to the case of this file."""
import numpy as np
import pytest

from test_gpu_audit import device_mesh, host
from test_gpu_intersect import CELL, built, check, ref
from test_gpu_stale_memory import three_fills

pytestmark = pytest.mark.gpu

CASES = {"run": "run129", "large": "large", "one": "one_triangle"}


@pytest.fixture(scope="module")
def MS():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


class _Dev:
    """A host array behind the ``.cpu().numpy()`` that check asks of a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_self_intersections(MS):
    """boxes, entries, candidates (count and emit), test and both lists at 134, 1,005 and 1 triangles."""
    def step(case):
        name = CASES[case]
        V, T = built(name)
        Tb = T.copy()
        Tb[len(Tb) // 2, 2] = len(V)
        with pytest.raises(IndexError):
            MS.self_intersections(device_mesh(MS, V, Tb), return_pairs=True, return_arrays=True, _cell=CELL.get(name, 0.0))
        r = MS.self_intersections(device_mesh(MS, V, T), return_pairs=True, return_arrays=True, _cell=CELL.get(name, 0.0))
        arrays = [host(r.pop(k)) for k in ("triangle_class", "pairs", "uncertain")]
        return [dict(r), *arrays]

    def check_first(case, res):
        got = dict(res[0], triangle_class=_Dev(res[1]), pairs=_Dev(res[2]), uncertain=_Dev(res[3]))
        check(got, ref(CASES[case]), case)

    three_fills(step, ("run", "large", "one"), check_first)
