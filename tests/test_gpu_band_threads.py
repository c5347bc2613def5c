"""Two threads mesh at once with the banded cascade (DESIGN.md sections 18 and 21): every buffer of
mesh.poisson_band is the call's own, so concurrent callers on their own streams both equal the
restatement bit for bit."""
import threading

import pytest

import band_ref as BR
from test_gpu_band import CL, MS, check, reference  # noqa: F401 (the fixtures)

pytestmark = pytest.mark.gpu


def test_two_threads(MS, CL):
    """poisson_band from two threads at depth 6, each on its own stream: both equal the restatement."""
    import torch
    names, out, errors = ("sphere2000", "sphere65"), {}, []
    refs = {name: reference(name, 6, 4) for name in names}

    def work(name):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                pc = CL.PointCloud(refs[name]["P"].copy(), None, normals=refs[name]["N"].copy())
                out[name] = MS.poisson_band(pc, depth=6, base_depth=4, return_record=True, return_fields=True)
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                        # noqa: BLE001 (reported below)
            errors.append((name, e))
    threads = [threading.Thread(target=work, args=(name,)) for name in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for name in names:
        check(refs[name], *out[name], 6, 4, BR.DEFAULT_BAND_SWEEPS)
