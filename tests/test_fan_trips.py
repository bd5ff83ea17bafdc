"""The fan march's dependent round trips ("round trips") on the GPU: the wave
prologue that loads the step table, the pose rows and the direction tables before one wait, and the
production kernels' walk over two packed window entries per trip (pcp_walk_pair.hpp).  Every case
compares blocked, units and first_hit bit for bit with the oracle, which probes every sample, over
the fine-window copy (PCP_TERRAIN_BLOCKS=2, built at the first query), and runs the plain call
without first hits as well; the mounted case compares with the NumPy restatement of its definition
(tests/mount_ref.py).

Prologue: a 64 x 8 fan over the small lattice with 8, 16, 32 and 64 poses (1, 2, 4 and 8 poses per
wave), 128 poses at PCP_FAN_NPW=16 and 256 at 32 (16 and 32 per wave: up to eight row loads per
lane), step tables of 1, 63, 64, 65, 128, 255 and 256 samples (every trip count of the staging and
both sides of each 64-lane boundary) and 64 tilted mounts (rows of 12 doubles).

Walk: terrains of a few dozen points (tests/fan_trips_cases.py) whose windows hold runs of 0, 1,
2, 3, 4 and more entries, at 64 poses (the production kernel with eight poses per wave) and 8
(one).  Beside the oracle, the march's counters of every walk case are the parent build's
(tests/golden/fan_trips_stats.json, written by tools/gen/fan_trips_stats.py): the statistics
kernels keep the one-entry walk, so the paired walk must leave what they count unchanged."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

import fan_trips_cases as cases
import mount_ref
from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "fan_trips_stats.json"


def _context(terrain):
    """A context over the fine copy (the knobs are read when the context is made)."""
    old = os.environ.get("PCP_TERRAIN_BLOCKS")
    os.environ["PCP_TERRAIN_BLOCKS"] = "2"
    try:
        ctx = _abi.Context(0)
        ctx.set_terrain(terrain, point_step=32)
    finally:
        if old is None:
            os.environ.pop("PCP_TERRAIN_BLOCKS", None)
        else:
            os.environ["PCP_TERRAIN_BLOCKS"] = old
    return ctx


def _check(oracle, ctx, terrain, poses, fan):
    poses = np.ascontiguousarray(poses, np.float64)
    oracle.set_threads(8)
    try:
        rb, ru, rfh = oracle.raycast_fan(oracle.Cloud(terrain), poses, fan.n_az, fan.n_el,
                                         fan.el_min, fan.el_max, fan.max_distance)
    finally:
        oracle.set_threads(1)
    b, u, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
    assert ctx.terrain_info()["scan_layout"] == "fine"
    b2, u2, _, _ = ctx.raycast_fan(poses, fan)      # (the benchmark's call: no first hits)
    np.testing.assert_array_equal(fh, rfh)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(b2, rb)
    np.testing.assert_array_equal(u2, ru)
    return rb, ru, rfh


def lattice_poses(n, z=1.1):
    """n poses spread over the small scene's 10 m x 10 m lattice (x -2..8, y -4..6), every fourth
    one 6 m up (only its steep rings live), yaws all around."""
    k = np.arange(n)
    p = np.stack([-1.0 + (k * 2.3) % 8.0, -3.0 + (k * 3.1) % 8.0, np.full(n, z),
                  -0.4 + 0.001 * k, 0.7 * k - 2.0], axis=1)
    p[3::4, 2] = 6.0
    return p


# ---- prologue ----

@pytest.mark.parametrize("n_poses,npw", [(8, None), (16, None), (32, None), (64, None),
                                         (128, "16"), (256, "32")])
def test_prologue_poses_per_wave(oracle, small_scene, monkeypatch, n_poses, npw):
    """1, 2, 4, 8, 16 and 32 rows of 16 doubles staged per wave: 16 lanes of one load up to eight
    loads per lane."""
    if npw:
        monkeypatch.setenv("PCP_FAN_NPW", npw)
    ctx = _context(small_scene.terrain)
    try:
        rb, _, _ = _check(oracle, ctx, small_scene.terrain, lattice_poses(n_poses),
                          cases.fan_64x8())
    finally:
        ctx.close()
    assert rb.sum() > 0


@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 255, 256])
def test_prologue_step_table_lengths(oracle, small_scene, K):
    """Step tables of exactly K samples (257 leaves the LDS kernels: test_long_range_fan): one to
    four staging loads per lane, the last one partial, full or absent."""
    fan = cases.fan_64x8(cases.max_distance_for(K))
    poses = lattice_poses(16, z=0.45)   # (the first sample, 0.5 m out, reaches the ground)
    ctx = _context(small_scene.terrain)
    try:
        rb, _, _ = _check(oracle, ctx, small_scene.terrain, poses, fan)
    finally:
        ctx.close()
    assert rb.sum() > 0


def test_prologue_mounted_rows(small_scene):
    """64 tilted mounts, eight per wave: rows of 12 doubles, 96 per wave, through the same
    staging; against the NumPy restatement of the mounted march."""
    rng = np.random.default_rng(31)
    P = 64
    poses6 = np.ascontiguousarray(np.column_stack([
        rng.uniform(-1.0, 7.0, P), rng.uniform(-3.0, 5.0, P), rng.uniform(0.8, 1.6, P),
        rng.uniform(-0.15, 0.15, P), rng.uniform(-0.6, -0.1, P), rng.uniform(-3.1, 3.1, P)]))
    fan = cases.fan_64x8()
    rfh, rb, ru = mount_ref.first_hits(small_scene.terrain, poses6, fan)
    ctx = _context(small_scene.terrain)
    try:
        ctx.raycast_fan_mounted(poses6, fan)     # (the second query builds the fine copy)
        b, u, fh, _ = ctx.raycast_fan_mounted(poses6, fan, None, want_first_hit=True)
        assert ctx.terrain_info()["scan_layout"] == "fine"
        b2, u2, _, _ = ctx.raycast_fan_mounted(poses6, fan)
    finally:
        ctx.close()
    np.testing.assert_array_equal(fh, rfh)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(b2, rb)
    np.testing.assert_array_equal(u2, ru)
    assert rb.sum() > 0


# ---- walk ----

def _run_lengths(ctx):
    """The lengths of every window's run, from the packed entry array as built."""
    geo, _, wpts, _ = ctx.debug_fine_copy()
    assert geo["built"] == 1 and geo["packed"] == 1 and geo["tile"] == 2 and geo["skip"] == 2
    ent = wpts[:geo["n_entries"] * 12].view(np.float32).reshape(-1, 3)
    sentinel = np.nonzero(np.isneginf(ent[:, 2]))[0]
    assert sentinel.size == geo["fnx"] * geo["fny"] and sentinel[-1] == ent.shape[0] - 1
    return np.diff(np.concatenate([[-1], sentinel])) - 1


@pytest.mark.parametrize("name", sorted(cases.WALK_CASES))
def test_walk_small_scenes(oracle, name):
    terrain, poses, fan = cases.walk_case(name)
    golden = json.loads(GOLDEN.read_text())["cases"][name]["stats"]
    ctx = _context(terrain)
    try:
        rb, _, rfh = _check(oracle, ctx, terrain, poses, fan)
        runs = _run_lengths(ctx)
        got = ctx.raycast_fan_stats(poses, fan)
    finally:
        ctx.close()
    print(name, "blocked", int(rb.sum()), "runs", np.bincount(runs)[:8].tolist(), got)
    scene = cases.WALK_CASES[name][0]
    # the aimed rays: some hit, some pass (the offsets straddle the radius)
    assert 0 < rb.sum()
    assert runs.max() == {"single": 1, "pair": 2, "corner": 4}.get(scene, runs.max())
    if scene == "strip":
        assert {1, 2, 3, 4} <= set(runs.tolist())
    if scene == "wall":
        assert runs.max() >= 12
    if scene == "corner":   # the last non-empty run, then only empty windows to the array's end
        last = np.nonzero(runs)[0][-1]
        assert runs[last] >= 1 and (runs[last + 1:] == 0).all() and last + 1 < runs.size
    assert got["scanned_stencils"] > 0 and got["directory_loads"] == 0
    assert got == golden


def test_walk_scenes_cover_the_run_lengths():
    """Over the five scenes the windows hold runs of 0, 1, 2, 3, 4 and more entries."""
    seen = set()
    for scene in cases.SCENES:
        terrain = cases.terrain_of(cases.scene_xyz(scene))
        ctx = _context(terrain)
        try:   # (the first query builds the copy)
            ctx.raycast_fan(np.array([[2.0, 1.0, 1.5, -0.4, 0.3]]), _abi.fan_params(n_az=8, n_el=4))
            seen |= set(_run_lengths(ctx).tolist())
        finally:
            ctx.close()
    assert {0, 1, 2, 3, 4} <= seen and max(seen) > 4
