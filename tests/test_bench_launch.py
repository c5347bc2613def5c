"""CPU tests of bench.py's launch handling: ``--gpus N`` runs N rank processes itself when no
launcher set WORLD_SIZE, a launcher's WORLD_SIZE must agree with ``--gpus``, and rank 0's
stdout is the only stdout (the driver parses one JSON line)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_launch_mode_rules():
    assert bench.launch_mode(1, {}) == "single"
    assert bench.launch_mode(4, {}) == "spawn"
    assert bench.launch_mode(8, {"WORLD_SIZE": "8"}) == "rank"
    assert bench.launch_mode(1, {"WORLD_SIZE": "1"}) == "single"
    for gpus, env in ((2, {"WORLD_SIZE": "1"}), (1, {"WORLD_SIZE": "8"}), (0, {})):
        with pytest.raises(SystemExit):
            bench.launch_mode(gpus, env)


def test_world_size_mismatch_exits_nonzero():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "disagrees" in r.stderr and r.stdout == ""


def test_spawn_ranks_env_and_stdout(tmp_path):
    """Two ranks through a gloo rendezvous on 127.0.0.1: each sees RANK/LOCAL_RANK/WORLD_SIZE,
    an all-reduce crosses the ranks, only rank 0's line reaches stdout."""
    script = tmp_path / "rank.py"
    script.write_text(
        "import json, os, sys, torch, torch.distributed as dist\n"
        "dist.init_process_group('gloo')\n"
        "t = torch.tensor([float(os.environ['RANK']) + 1.0]); dist.all_reduce(t)\n"
        "print(json.dumps({'rank': int(os.environ['RANK']), 'local': int(os.environ['LOCAL_RANK']),\n"
        "                  'world': dist.get_world_size(), 'sum': float(t.item()), 'argv': sys.argv[1:]}))\n"
        "dist.destroy_process_group()\n")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import bench\n"
            f"sys.exit(bench.spawn_ranks(2, ['--gpus', '2'], script={str(script)!r}))\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    # (gloo prints its peer banner on fd 1; bench.py moves such banners to stderr itself)
    lines = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert lines == [{"rank": 0, "local": 0, "world": 2, "sum": 3.0, "argv": ["--gpus", "2"]}]
    assert '"rank": 1' in r.stderr


@pytest.mark.parametrize("config", ["c2", "c3"])
def test_spawned_two_rank_line_carries_cpu_baseline(config):
    """``bench.py --gpus 2`` (self-spawned ranks, the driver's N>1 lines): rank 0 times the
    reference CPU path before touching the GPU, so the N>1 line carries ``cpu_baseline`` too
    (the CPU baseline belongs to ``--full``; ``--cpu-baseline-only`` stops there; no GPU is needed)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", config, "--full",
                        "--views", "1" if config == "c2" else "2", "--cpu-seconds", "0.2", "--cpu-baseline-only"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2
    cpu = lines[0]["cpu_baseline"]
    assert cpu is not None and cpu["value"] > 0 and cpu["kind"] == "port" and cpu["cores"] >= 1
    assert "sl_refseq" in cpu["what"]


def test_spawn_ranks_propagates_failure(tmp_path):
    script = tmp_path / "fail.py"
    script.write_text("import os, sys\nsys.exit(3 if os.environ['RANK'] == '1' else 0)\n")
    assert bench.spawn_ranks(2, [], script=str(script)) == 3


def _fake_clouds(counts, dtype, seed=3):
    import torch
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(seed)
    return [SimpleNamespace(xyz=torch.randn((n + 5, 3), generator=g).to(dtype),
                            bgr=torch.randint(0, 256, (n + 5, 3), generator=g, dtype=torch.uint8),
                            count=torch.tensor([n], dtype=torch.int64)) for n in counts]


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """bench.dump_outputs (``--dump-outputs``): float32 / float64 ``.npy`` files of the views'
    counts, full-cloud sums and the clouds' rows -- all of them under the byte bound, a sorted
    sample drawn with a fixed seed above it (the same rows on every run), never past the bound."""
    import numpy as np
    import torch
    for dtype in (torch.float32, torch.float64):
        clouds = _fake_clouds([7, 0, 12], dtype)
        info = bench.dump_outputs(str(tmp_path / f"all_{dtype}"), clouds)
        z = {n[:-4]: np.load(tmp_path / f"all_{dtype}" / n) for n in os.listdir(tmp_path / f"all_{dtype}")}
        assert sorted(z) == ["bgr", "bgr_sum", "counts", "rows", "xyz", "xyz_sum"]
        assert all(a.dtype in (np.float32, np.float64) for a in z.values())
        assert z["counts"].tolist() == [7.0, 0.0, 12.0] and info["points"] == info["rows"] == 19
        want = torch.cat([c.xyz[:n] for c, n in zip(clouds, (7, 0, 12))]).numpy()
        assert z["xyz"].dtype == want.dtype and np.array_equal(z["xyz"], want)
        assert np.array_equal(z["bgr"], torch.cat([c.bgr[:n] for c, n in zip(clouds, (7, 0, 12))]).numpy())
        assert np.array_equal(z["rows"], np.arange(19))
        assert np.array_equal(z["xyz_sum"][2], clouds[2].xyz[:12].double().sum(0).numpy())
        assert np.array_equal(z["xyz_sum"][1], np.zeros(3))
    # above the bound: 32 B per float32 row (xyz + bgr + rows) -> 10 of the 19 rows
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 32 + 31)
    clouds = _fake_clouds([7, 0, 12], torch.float32)
    a = bench.dump_outputs(str(tmp_path / "s1"), clouds)
    b = bench.dump_outputs(str(tmp_path / "s2"), clouds)
    assert a["rows"] == b["rows"] == 10 and a["points"] == 19 and a["bytes"] == b["bytes"]
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert len(set(rows.tolist())) == 10 and np.all(np.diff(rows) > 0) and rows.max() < 19
    full = torch.cat([c.xyz[:n] for c, n in zip(clouds, (7, 0, 12))]).numpy()
    assert np.array_equal(np.load(tmp_path / "s1" / "xyz.npy"), full[rows.astype(np.int64)])
    for n in ("rows", "xyz", "bgr", "counts", "xyz_sum", "bgr_sum"):
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "xyz_sum.npy")[0], clouds[0].xyz[:7].double().sum(0).numpy())
    assert sum(np.load(tmp_path / "s1" / f"{n}.npy").nbytes for n in ("rows", "xyz", "bgr")) <= 10 * 32 + 31


def test_dump_of_large_clouds_stays_within_64_mb(tmp_path):
    """Clouds past the bound at its real value (2 x 1.3 M fp64 points, 44 B a row): the dump is
    sampled, and everything it writes -- arrays and files -- is at most 64 MB."""
    import numpy as np
    import torch
    clouds = _fake_clouds([1_300_000, 1_299_999], torch.float64)
    info = bench.dump_outputs(str(tmp_path / "big"), clouds)
    assert info["points"] == 2_599_999 and info["rows"] == bench.DUMP_MAX_BYTES // 44 < info["points"]
    assert info["bytes"] <= 64_000_000
    assert sum(os.path.getsize(tmp_path / "big" / n) for n in os.listdir(tmp_path / "big")) <= 64_000_000
    rows = np.load(tmp_path / "big" / "rows.npy").astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < info["points"]
    full = torch.cat([clouds[0].xyz[:1_300_000], clouds[1].xyz[:1_299_999]]).numpy()
    assert np.array_equal(np.load(tmp_path / "big" / "xyz.npy"), full[rows])


def test_full_gates_baseline_verify_and_models():
    """bench.parse_args: a plain command line leaves out the CPU baseline, the verification and
    the traffic models; ``--full`` turns them on, ``--no-cpu-baseline`` / ``--no-verify`` take one
    out again; ``--cpu-baseline-only`` implies ``--full``."""
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.no_cpu_baseline, a.no_verify, a.dump_outputs) == (False, True, True, None)
    assert (a.steps, a.warmup, a.config) == (7, 2, "c2")
    a = bench.parse_args(["--no-verify", "--dump-outputs", "d"])          # no --full: still plain
    assert (a.full, a.no_cpu_baseline, a.no_verify, a.dump_outputs) == (False, True, True, "d")
    a = bench.parse_args(["--full"])
    assert (a.full, a.no_cpu_baseline, a.no_verify) == (True, False, False)
    a = bench.parse_args(["--full", "--no-verify"])
    assert (a.full, a.no_cpu_baseline, a.no_verify) == (True, False, True)
    a = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert (a.full, a.no_cpu_baseline, a.no_verify) == (True, True, False)
    a = bench.parse_args(["--cpu-baseline-only"])
    assert (a.full, a.no_cpu_baseline, a.cpu_baseline_only) == (True, False, True)


def test_plain_run_skips_the_cpu_baseline():
    """rank0_cpu_baseline with a plain command line returns None without timing anything."""
    assert bench.rank0_cpu_baseline(bench.parse_args([]), 0, None, None, None) is None


def test_dump_outputs_refused_for_job_configs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c3", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and r.stdout == ""


def test_mask_first_segments_count():
    """bench.segments_holding (the mask-first algorithmic bytes): 64-byte segments of each frame
    that hold a valid pixel, checked against a brute-force count, with frames at offsets that
    are and are not multiples of 64."""
    import numpy as np
    import torch
    rng = np.random.default_rng(5)
    n_px = 5000
    mask = rng.random(n_px) < 0.05
    mask[:70] = True                                   # a run across a segment boundary
    for stride, frames in ((5056, [0, 2, 3]), (5008, [0, 1, 2, 5])):
        want = 0
        for f in frames:
            segs = set(((f * stride + np.nonzero(mask)[0]) >> 6).tolist())
            want += len(segs)
        assert bench.segments_holding(torch.from_numpy(mask), stride, frames) == want
    assert bench.segments_holding(torch.zeros(n_px, dtype=torch.bool), 5056, [0, 1]) == 0
