"""The Python layer's state under concurrent callers, on the CPU.

The reference's GUI calls its static hot-path methods from daemon threads, so the drop-in is
called that way too.  A workspace holds what one call leaves for the next (``slg_decode_stats``
arms ``slg_decode``; a cloud step's grid, status word and far count), and the ctypes calls run
with the GIL released, so two threads must never be handed one workspace.  These tests put two
threads inside the calls at the same moment against a fake native library that records
``(thread, function, pointer arguments)``, and check the engines, the cloud workspaces, the
calibration cache and the library load.  Nothing here touches a GPU.
"""
import collections
import ctypes
import threading
import time

import numpy as np
import pytest
import torch

from structured_light_for_3d_model_replication_amd import _native as N
from structured_light_for_3d_model_replication_amd import cloud as CL
from structured_light_for_3d_model_replication_amd import engine as E
from structured_light_for_3d_model_replication_amd import processing as PR

JOIN_S = 30.0
H, W = 4, 8


def run_threads(bodies, timeout=JOIN_S):
    """Runs each body on a daemon thread; a body's exception is re-raised here, and a thread
    still alive after ``timeout`` fails the test instead of blocking it.  Returns the results."""
    errors, results = [], [None] * len(bodies)

    def wrap(i, body):
        try:
            results[i] = body()
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=wrap, args=(i, b), daemon=True) for i, b in enumerate(bodies)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    if errors:
        raise errors[0]
    return results


class FakeLib:
    """Stands in for ``libslgpu.so``: every export returns ``SLG_OK`` and is recorded as
    ``(thread id, name, tuple of the c_void_p arguments' values, None for the others)``.
    ``hooks[name]()`` runs inside that call, after it is recorded."""

    WS_BYTES = 4096

    def __init__(self, hooks=None):
        self.calls = []
        self.hooks = hooks or {}
        self._lock = threading.Lock()

    def __getattr__(self, name):
        if not name.startswith("slg_"):
            raise AttributeError(name)

        def call(*args):
            ptrs = tuple(a.value if isinstance(a, ctypes.c_void_p) else None for a in args)
            with self._lock:
                self.calls.append((threading.get_ident(), name, ptrs))
            if name in self.hooks:
                self.hooks[name]()
            return self.WS_BYTES if name == "slg_workspace_bytes" else N.SLG_OK
        return call

    def of(self, tid, name):
        return [c[2] for c in self.calls if c[0] == tid and c[1] == name]


class StubStream:
    cuda_stream = 0

    def synchronize(self):
        pass


class StubFrames:
    height, width = H, W

    def capture(self):
        return N.Capture(frames=0, frame_stride=H * W, n_frames=4, height=H, width=W, reserved=0, texture=0)


class StubCalib:
    height, width = H, W

    def struct(self):
        return N.Calib()


@pytest.fixture
def fake(monkeypatch):
    """The four patches with which a ``Reconstructor`` constructs and launches on the CPU."""
    lib = FakeLib()
    stream = StubStream()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: stream)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(E, "default_device", lambda: torch.device("cpu"))
    return lib


WS_ARG = {"slg_decode_stats": 2, "slg_decode": 2, "slg_reconstruct": 4}     # the workspace's place in each call


def test_engine_workspaces_decode(fake):
    """Two threads between ``slg_decode_stats`` and ``slg_decode`` at the same moment: each has
    its own engine and workspace, each ``slg_decode`` gets the workspace its own thread's
    ``slg_decode_stats`` armed, and a thread's second call reuses its engine."""
    barrier = threading.Barrier(2, timeout=10)
    fake.hooks["slg_decode_stats"] = barrier.wait
    cfg = E.DecodeConfig(1920, 1080, 11, 11, "otsu")

    def body():
        engines = []
        for _ in range(2):
            eng = PR._engine(H, W)
            eng.decode(StubFrames(), cfg)
            engines.append(eng)
        return threading.get_ident(), engines

    (ta, ea), (tb, eb) = run_threads([body, body])
    assert ea[0].workspace.data_ptr() != eb[0].workspace.data_ptr()
    assert ea[0] is not eb[0]
    assert ea[0] is ea[1] and eb[0] is eb[1]                      # one engine per thread, reused
    for tid, engs in ((ta, ea), (tb, eb)):
        stats = [p[WS_ARG["slg_decode_stats"]] for p in fake.of(tid, "slg_decode_stats")]
        dec = [p[WS_ARG["slg_decode"]] for p in fake.of(tid, "slg_decode")]
        assert len(stats) == len(dec) == 2
        assert stats == dec == [engs[0].workspace.data_ptr()] * 2   # decode reads what its own stats wrote
    ws_a = {p[2] for p in fake.of(ta, "slg_decode_stats")}
    ws_b = {p[2] for p in fake.of(tb, "slg_decode_stats")}
    assert ws_a.isdisjoint(ws_b)


def test_engine_workspaces_reconstruct(fake):
    """The same for the fused call, where the drop-in reaches it (``reconstruct_view``): two
    threads inside ``slg_reconstruct`` at the same moment pass different workspaces."""
    barrier = threading.Barrier(2, timeout=10)
    fake.hooks["slg_reconstruct"] = barrier.wait
    cfg = E.DecodeConfig(1920, 1080, 11, 11, "otsu")

    def body():
        for _ in range(2):
            P, C = PR.reconstruct_view(StubFrames(), cfg, {}, row_mode=1, dc=StubCalib())
            assert P.shape == (0, 3) and C.shape == (0, 3)
        return threading.get_ident(), PR._engine(H, W)

    (ta, ea), (tb, eb) = run_threads([body, body])
    assert ea is not eb
    got = {}
    for tid, eng in ((ta, ea), (tb, eb)):
        got[tid] = [p[WS_ARG["slg_reconstruct"]] for p in fake.of(tid, "slg_reconstruct")]
        assert got[tid] == [eng.workspace.data_ptr()] * 2
    assert got[ta][0] != got[tb][0]


def test_cloud_workspaces(fake):
    """``cloud._workspace`` gives each thread its own tensor (kept for a smaller need, replaced
    for a larger one), and ``far_count`` reads the calling thread's bytes 8..12."""
    cpu = torch.device("cpu")
    barrier = threading.Barrier(2, timeout=10)

    def body(value):
        def run():
            ws = CL._workspace(cpu, 1024)
            ptr = ws.data_ptr()
            assert ws.numel() >= 1024 and ws.dtype == torch.uint8
            barrier.wait()                                        # both workspaces are alive here
            assert CL._workspace(cpu, 512) is ws                  # a smaller need: the same tensor
            big = CL._workspace(cpu, 4096)
            assert big is not ws and big.numel() >= 4096          # a larger need: a new one
            assert CL._workspace(cpu, 1024) is big
            big.zero_()
            big[8:12].view(torch.int32)[0] = value
            barrier.wait()                                        # both far counts are written here
            far = CL.far_count(cpu)
            barrier.wait()
            return ptr, big.data_ptr(), far
        return run

    (pa, ba, fa), (pb, bb, fb) = run_threads([body(3), body(77)])
    assert pa != pb and ba != bb
    assert (fa, fb) == (3, 77)


def _small_calib(seed):
    rng = np.random.default_rng(seed)
    return {"cam_K": np.array([[100.0, 0, W / 2], [0, 100.0, H / 2], [0, 0, 1]]), "Oc": np.zeros((3, 1)),
            "wPlaneCol": rng.standard_normal((4, 16)), "wPlaneRow": rng.standard_normal((4, 8)),
            "Nc": rng.standard_normal((3, H * W))}


def test_calibration_cache_under_eviction(fake, monkeypatch):
    """8 threads x 200 lookups over 6 calibrations, more than the cache holds, so entries are
    inserted and evicted all the time: nothing raises, every answer belongs to the calibration
    asked for, and the cache stays within its bound.  A guard: without the lock the failure
    (a ``KeyError`` from ``move_to_end`` or ``popitem`` on an entry another thread just evicted)
    needs a thread switch between two statements and does not show on every run."""
    class RecordingCalib:
        def __init__(self, calib, h, w):
            self.fp = PR.calib_fingerprint(calib, full=True)
            time.sleep(0)                                          # lets another thread in, as an upload would

    monkeypatch.setattr(E, "DeviceCalib", RecordingCalib)
    monkeypatch.setattr(PR, "_CALIBS", collections.OrderedDict())
    calibs = [_small_calib(s) for s in range(6)]
    assert len(calibs) > PR._CALIBS_MAX
    want = [PR.calib_fingerprint(c, full=True) for c in calibs]
    assert len(set(want)) == len(calibs)

    def body(t):
        def run():
            rng = np.random.default_rng(100 + t)
            for i in range(200):
                k = int(rng.integers(len(calibs)))
                cal = calibs[k]
                if i % 3 == 0:                                     # equal content in other objects: the full-digest hit
                    cal = {name: a.copy() for name, a in cal.items()}
                assert PR._device_calib(cal, H, W).fp == want[k]
        return run

    run_threads([body(t) for t in range(8)])
    assert 0 < len(PR._CALIBS) <= PR._CALIBS_MAX


def test_library_loads_once(monkeypatch, tmp_path):
    """8 threads make the first ``lib()`` call at once: one load, one object for all."""
    from structured_light_for_3d_model_replication_amd import build as B
    build_id = B.BUILD_ID_PREFIX + B.source_digest().encode()
    loads = []

    class Fn:
        def __init__(self, result):
            self.result = result

        def __call__(self, *args):
            return self.result

    class FakeCDLL:
        def __init__(self, path):
            loads.append(path)
            time.sleep(0.05)                                       # the others arrive while this one loads
            for name in N.EXPORTS:
                setattr(self, name, Fn({"slg_version": N.ABI_VERSION, "slg_build_id": build_id}.get(name, 0)))

    path = tmp_path / N.LIB_NAME
    path.write_bytes(b"")
    monkeypatch.setattr(N, "LIB_PATH", str(path))
    monkeypatch.setattr(N, "AB_LIB", None)
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", FakeCDLL)
    barrier = threading.Barrier(8, timeout=10)

    def body():
        barrier.wait()
        return N.lib()

    got = run_threads([body] * 8)
    assert len(loads) == 1, loads
    assert all(g is got[0] for g in got) and isinstance(got[0], FakeCDLL)
