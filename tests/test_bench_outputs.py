"""bench.py's plain run: the headline alone (what --full adds is absent), and --dump-outputs
writes what the last timed step returned."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

FULL_ONLY = ("roofline", "c1", "c5", "c3", "c4", "reference_mode", "poses_per_s_reference_mode",
             "cpu_baseline", "cpu_baseline_mt", "cpu_baseline_kdtree")


def test_dump_outputs_writes_float64_npy(tmp_path):
    blocked = np.array([7, 0, 2**32 - 1], np.uint32)
    units = np.array([2**52 + 1, 3, 0], np.uint64)
    bench._dump_outputs(tmp_path / "a" / "b", {"blocked": blocked, "units": units})
    got = {p.name: np.load(p) for p in (tmp_path / "a" / "b").iterdir()}
    assert sorted(got) == ["blocked.npy", "units.npy"]
    assert got["blocked.npy"].dtype == np.float64 and got["units.npy"].dtype == np.float64
    assert np.array_equal(got["blocked.npy"].astype(np.uint32), blocked)
    assert np.array_equal(got["units.npy"].astype(np.uint64), units)


def test_dump_outputs_bounded(tmp_path):
    big = np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, np.float64)
    with pytest.raises(SystemExit):
        bench._dump_outputs(tmp_path, {"big": big})


def test_dump_outputs_is_the_fan_search_only(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--mode", "c1",
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path, scene):
    """A small fan search (8 poses x 128 x 32 rays on the 1M-point terrain) through bench.py
    with no --full: the line holds the headline's keys and none of --full's, --steps is the
    number of timed steps, and the dumped arrays are the library's answer for the same seeded
    poses in this process."""
    from pointcloud_processor_amd import _abi

    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--poses-per-gpu", "8", "--n-az", "128", "--n-el", "32",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "ray-hit tests/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64 march / f32 point test"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in out]
    blocked, units, best = (np.load(d / f"{n}.npy") for n in ("blocked", "units", "best_pose"))
    assert blocked.dtype == units.dtype == best.dtype == np.float64
    # value = the ray-hit tests of the K steps over their time
    assert out["value"] == pytest.approx(units.sum() * 2 / (out["ms_per_step"] * 2e-3), rel=1e-9)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        poses, _ = bench._poses_for(ctx, bench._grid_bbox(scene.area), scene.zx120_pose5, 8)
        rb, ru, _, rbest = ctx.raycast_fan(poses, _abi.fan_params(n_az=128, n_el=32))
    assert np.array_equal(blocked, rb.astype(np.float64))
    assert np.array_equal(units, ru.astype(np.float64))
    assert best.tolist() == [float(rbest)] and out["best_pose"] == rbest
