"""The march's jump over empty ground (DESIGN.md §5 Skip 5, pcp_fan_clear.hpp) on the GPU: a
descending ray whose sample reads an empty probe record jumps by the record's clearance code.
Every case compares blocked, units and first_hit bit for bit with the oracle, which probes every
sample, with PCP_FAN_CLEAR=1 and =0, over the fine-window copy (built at the first query here).
The fan is 128 x 64; 64 poses run the 8-poses-per-wave kernel, 8 poses one pose per wave."""
import os

import numpy as np
import pytest

import fine_ref
from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

N_AZ, N_EL = 128, 64


def _context(terrain, clear):
    """A context with the knob set (read when the context is created) and the terrain's fine
    copy built at its first query."""
    env = {"PCP_FAN_CLEAR": clear, "PCP_TERRAIN_BLOCKS": "2"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = _abi.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    ctx.set_terrain(terrain, point_step=32)
    return ctx


def _run(oracle, terrain, poses, fan, stats=False):
    """Both knob settings against the oracle; returns the oracle's arrays and, when asked, the
    two settings' march counters."""
    poses = np.ascontiguousarray(poses, np.float64)
    oracle.set_threads(8)
    try:
        rb, ru, rfh = oracle.raycast_fan(oracle.Cloud(terrain), poses, fan.n_az, fan.n_el,
                                         fan.el_min, fan.el_max, fan.max_distance)
    finally:
        oracle.set_threads(1)
    counters = {}
    for clear in ("1", "0"):
        ctx = _context(terrain, clear)
        try:
            b, u, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
            assert ctx.terrain_info()["scan_layout"] == "fine"
            b2, u2, _, _ = ctx.raycast_fan(poses, fan)   # (the benchmark's call: no first hits)
            if stats:
                counters[clear] = ctx.raycast_fan_stats(poses, fan)
                counters["copy" + clear] = ctx.debug_fine_copy()
        finally:
            ctx.close()
        np.testing.assert_array_equal(fh, rfh, err_msg=f"PCP_FAN_CLEAR={clear}")
        np.testing.assert_array_equal(b, rb, err_msg=f"PCP_FAN_CLEAR={clear}")
        np.testing.assert_array_equal(u, ru, err_msg=f"PCP_FAN_CLEAR={clear}")
        np.testing.assert_array_equal(b2, rb)
        np.testing.assert_array_equal(u2, ru)
    return rb, ru, rfh, counters


def _hit_heights(oracle, poses, fan, fh):
    """z of every ray's first-hit sample (NaN: not blocked) and of every sample, per ring."""
    _, _, _, se = oracle.fan_tables(fan.n_az, fan.n_el, fan.el_min, fan.el_max)
    s = np.asarray(_abi.step_table(fan.max_distance - 0.08))
    zs = poses[:, 2][:, None, None] + np.asarray(se)[None, :, None] * s[None, None, :]  # P, el, K
    k = np.clip(fh, 0, s.size - 1)
    zh = np.take_along_axis(np.broadcast_to(zs[:, :, None, :], fh.shape + (s.size,)),
                            k[..., None].astype(np.int64), axis=3)[..., 0]
    return np.where(fh >= 0, zh, np.nan), zs, s


def _lattice_poses(n, z=1.1):
    """n poses spread over the small scene's 10 m x 10 m lattice (x -2..8, y -4..6)."""
    k = np.arange(n)
    x = -1.0 + (k * 2.3) % 8.0
    y = -3.0 + (k * 3.1) % 8.0
    return np.stack([x, y, np.full(n, z), -0.4 + 0.01 * k, 0.7 * k - 2.0], axis=1)


def _sheet(x0, x1, y0, y1, z, d=0.05):
    xs, ys = np.arange(x0, x1 - 1e-9, d), np.arange(y0, y1 - 1e-9, d)
    X, Y = np.meshgrid(xs, ys)
    return np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1)


def _cloud(xyz):
    """(N, 8) float32 PointXYZRGB image of the points."""
    return synth._pack(np.asarray(xyz, np.float32), (255, 0, 0))


def test_standard(oracle, small_scene):
    """Poses 1.1 m over the lattice: the jump removes probes and nothing else."""
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    rb, _, _, st = _run(oracle, small_scene.terrain, _lattice_poses(64), fan, stats=True)
    assert rb.sum() > 0
    assert st["1"]["samples_visited"] < st["0"]["samples_visited"]
    assert st["1"]["scanned_stencils"] == st["0"]["scanned_stencils"]
    assert st["1"]["point_tests"] == st["0"]["point_tests"]
    # the knob changes the march alone: both contexts built the same copy, byte for byte, and
    # the jump had codes to read -- a share of the empty interior records carries one
    (g1, frec1, wpts1, _), (g0, frec0, wpts0, _) = st["copy1"], st["copy0"]
    assert g1 == g0 and g1["built"] == 1 and g1["tile"] == 2
    assert np.array_equal(frec1, frec0) and np.array_equal(wpts1, wpts0)
    f = fine_ref.features(g1, frec1)
    assert f["empty_interior"] > 0 and f["code_ge1"] / f["empty_interior"] > 0.0
    assert f["code_ge2"] > 0


def test_one_pose_per_wave(oracle, small_scene):
    """8 poses: one per XCD chunk, poses per wave falls to 1."""
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    rb, _, _, _ = _run(oracle, small_scene.terrain, _lattice_poses(8), fan)
    assert rb.sum() > 0


def test_beside_the_pit(oracle, small_scene):
    """Poses 0.3 m outside the pit's rim (the L-pit at (4, 1): top outline x 3.13..6.27,
    y -1.27..1.27), facing it: rays go underground beside the pit and come out through the slope
    into it, where they are blocked after their first underground sample."""
    t = np.linspace(0.0, 1.0, 22)
    west = np.stack([np.full(22, 3.13 - 0.3), -1.0 + 2.0 * t], 1)
    south = np.stack([3.4 + 2.6 * t[:21], np.full(21, -1.27 - 0.3)], 1)
    east = np.stack([np.full(21, 6.27 + 0.3), -1.0 + 1.2 * t[:21]], 1)
    xy = np.concatenate([west, south, east], 0)
    yaw = np.arctan2(-0.2 - xy[:, 1], 4.6 - xy[:, 0])
    poses = np.stack([xy[:, 0], xy[:, 1], np.full(64, 1.1), np.full(64, -0.4), yaw], 1)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    _, _, rfh, _ = _run(oracle, small_scene.terrain, poses, fan)
    zh, zs, _ = _hit_heights(oracle, poses, fan, rfh)
    under = zs < -0.15                                   # below the ground sheet (z ~ 0 +- 0.04)
    first_under = np.where(under.any(2), under.argmax(2), zs.shape[2])     # P, el
    later = (rfh >= 0) & (rfh > first_under[:, :, None])
    assert later.sum() > 100   # not vacuous: hits found after marching underground


def test_buried_layer(oracle):
    """A flat sheet at z = 0 with a second one at z = -0.6 under half of it: the rays that step
    through the top sheet must hit the buried one."""
    top = _sheet(0.0, 8.0, 0.0, 8.0, 0.0)
    low = _sheet(0.0, 4.0, 0.0, 8.0, -0.6)
    terrain = _cloud(np.concatenate([top, low], 0))
    k = np.arange(64)
    poses = np.stack([0.7 + (k * 1.3) % 6.6, 0.7 + (k * 2.9) % 6.6, np.full(64, 1.1),
                      np.full(64, -0.4), 0.37 * k], 1)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    _, _, rfh, _ = _run(oracle, terrain, poses, fan)
    zh, _, _ = _hit_heights(oracle, poses, fan, rfh)
    assert (zh < -0.5).sum() > 100 and (np.abs(zh) < 0.06).sum() > 100


def test_upward_and_mixed_rings(oracle, small_scene):
    """Poses inside the pit (z = -0.5) and below everything (z = -2.5): the rings that look up
    are live and must not jump."""
    k = np.arange(32)
    inside = np.stack([3.6 + (k * 0.13) % 0.8, -0.8 + (k * 0.37) % 1.6, np.full(32, -0.5)], 1)
    below = _lattice_poses(32, z=-2.5)[:, :3]
    xyz = np.concatenate([inside, below], 0)
    poses = np.concatenate([xyz, np.full((64, 1), -0.3), (0.5 * np.arange(64))[:, None]], 1)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    rb, _, rfh, _ = _run(oracle, small_scene.terrain, poses, fan)
    assert (rfh[:32, N_EL // 2 + 4:, :] >= 0).any() and (rfh[32:, N_EL // 2 + 4:, :] >= 0).any()


def test_saturation(oracle):
    """A 45 m x 4 m strip, flat but for a 1 m-deep trench at x = 30 m, and a 40 m march.  Poses
    under the sheet look along it: their slightly descending rays cross far more than 255 cells
    (15.3 m) of empty records, whose codes saturate, and must still hit the trench's wall."""
    flat_a = _sheet(0.0, 30.0, 0.0, 4.0, 0.0)
    flat_b = _sheet(31.0, 45.0, 0.0, 4.0, 0.0)
    floor = _sheet(30.0, 31.0, 0.0, 4.0, -1.0)
    zw, yw = np.meshgrid(np.arange(-1.0, 0.0, 0.05), np.arange(0.0, 4.0 - 1e-9, 0.05))
    walls = [np.stack([np.full(zw.size, x), yw.ravel(), zw.ravel()], 1) for x in (30.0, 31.0)]
    terrain = _cloud(np.concatenate([flat_a, flat_b, floor] + walls, 0))
    k = np.arange(64)
    poses = np.stack([1.0 + (k * 0.17) % 10.0, 1.5 + (k * 0.07) % 1.0, np.full(64, -0.3),
                      np.full(64, -0.1), 0.02 * (k % 5 - 2)], 1)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL, max_distance=40.0)
    _, _, rfh, _ = _run(oracle, terrain, poses, fan)
    zh, _, s = _hit_heights(oracle, poses, fan, rfh)
    _, _, _, se = oracle.fan_tables(fan.n_az, fan.n_el, fan.el_min, fan.el_max)
    down = (np.asarray(se) < 0)[None, :, None]
    far = (rfh >= 0) & down & (s[np.clip(rfh, 0, s.size - 1)] > 17.0) & (zh < -0.2)
    assert far.sum() >= 8   # descending rays blocked by the wall after > 255 cells underground


def test_float_margins(oracle, small_scene):
    """Terrain and poses shifted by kilometres, where float spacing (2.4e-4 m) is no longer small
    against the millimetre margins."""
    shift = np.array([3000.0, -2000.0, 1500.0])
    terr = np.ascontiguousarray(small_scene.terrain.copy())
    terr[:, :3] += shift.astype(np.float32)
    poses = _lattice_poses(64)
    poses[:, :3] += shift
    rb, _, _, _ = _run(oracle, terr, poses, _abi.fan_params(n_az=N_AZ, n_el=N_EL))
    assert rb.sum() > 0


def test_edges(oracle, small_scene):
    """Poses within 0.3 m of the terrain's edge, inside and outside it: samples beyond the grid
    read clamped records and must not jump."""
    t = np.linspace(0.0, 1.0, 16)
    x0, x1, y0, y1 = -2.0, 7.95, -4.0, 5.95
    off = np.where(np.arange(16) % 2 == 0, 0.25, -0.25)     # inside / outside, alternating
    xy = np.concatenate([np.stack([x0 + off, y0 + (y1 - y0) * t], 1),
                         np.stack([x1 - off, y0 + (y1 - y0) * t], 1),
                         np.stack([x0 + (x1 - x0) * t, y0 + off], 1),
                         np.stack([x0 + (x1 - x0) * t, y1 - off], 1)], 0)
    poses = np.stack([xy[:, 0], xy[:, 1], np.full(64, 1.1), np.full(64, -0.4),
                      0.41 * np.arange(64)], 1)
    rb, _, _, _ = _run(oracle, small_scene.terrain, poses, _abi.fan_params(n_az=N_AZ, n_el=N_EL))
    assert rb.sum() > 0
