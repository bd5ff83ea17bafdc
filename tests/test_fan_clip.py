"""The march's clip interval with its slack as a value (DESIGN.md §5 Skip 3, pcp_fan_clip.hpp) on
the GPU: the default drops the two slack samples the whole-sample rule (PCP_FAN_CLIP=0) still
probed.  Every case compares blocked, units and first_hit bit for bit with the oracle, which
probes every sample, under both settings, over the fine-window copy (built at the first query
here).  Fans are 64 x 8 and 96 x 6 (96 is no multiple of 64: the non-uniform kernels); 3, 8 and 64
poses run the interleaved kernel, one pose per wave and eight per wave."""
import os

import numpy as np
import pytest

from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

FANS = {"64x8": (64, 8), "96x6": (96, 6)}
COMBOS = [(f, n) for f in ("64x8", "96x6") for n in (3, 8, 64)]     # every kernel of the launcher
R_Q, MARGIN = 0.08 * 0.7, 1e-3      # the terrain index's query radius and margin


def _fan(name, el_min=-85.0 * np.pi / 180.0, el_max=85.0 * np.pi / 180.0, max_distance=15.0):
    n_az, n_el = FANS[name]
    return _abi.FanParams(n_az, n_el, el_min, el_max, max_distance)


def _context(terrain, clip):
    """A context with the knob set or left alone (it is read when the context is created) and the
    terrain's fine copy built at its first query."""
    env = {"PCP_TERRAIN_BLOCKS": "2"}
    if clip is not None:
        env["PCP_FAN_CLIP"] = clip
    old = {k: os.environ.get(k) for k in list(env) + ["PCP_FAN_CLIP"]}
    os.environ.pop("PCP_FAN_CLIP", None)
    os.environ.update(env)
    try:
        ctx = _abi.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.set_terrain(terrain, point_step=32)
    return ctx


def _run(oracle, terrain, poses, fan, stats=False):
    """The default and PCP_FAN_CLIP=0 against the oracle; returns the oracle's arrays and, when
    asked, the two settings' march counters."""
    poses = np.ascontiguousarray(poses, np.float64)
    oracle.set_threads(8)
    try:
        rb, ru, rfh = oracle.raycast_fan(oracle.Cloud(terrain), poses, fan.n_az, fan.n_el,
                                         fan.el_min, fan.el_max, fan.max_distance)
    finally:
        oracle.set_threads(1)
    counters = {}
    for clip in (None, "0"):
        ctx = _context(terrain, clip)
        try:
            b, u, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
            assert ctx.terrain_info()["scan_layout"] == "fine"
            b2, u2, _, _ = ctx.raycast_fan(poses, fan)   # (the benchmark's call: no first hits)
            if stats:
                counters[clip] = ctx.raycast_fan_stats(poses, fan)
        finally:
            ctx.close()
        np.testing.assert_array_equal(fh, rfh, err_msg=f"PCP_FAN_CLIP={clip}")
        np.testing.assert_array_equal(b, rb, err_msg=f"PCP_FAN_CLIP={clip}")
        np.testing.assert_array_equal(u, ru, err_msg=f"PCP_FAN_CLIP={clip}")
        np.testing.assert_array_equal(b2, rb)
        np.testing.assert_array_equal(u2, ru)
    return rb, ru, rfh, counters


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


def _box_top(terrain):
    """The clip box's float top face, as GridIndex::view computes it."""
    t = terrain[:, :3].astype(np.float64)
    amax = np.abs(t).max()
    return float(np.float32(t[:, 2].max() + R_Q + MARGIN + 1e-6 * amax))


def _steps(n):
    s = [0.5]
    while len(s) < n:
        s.append(s[-1] + 0.3)
    return np.array(s)


# (a) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_lattice(oracle, small_scene, fan_name, n_poses):
    """Poses 1.1 m over the lattice: nearly every live ray enters through the top face, so its
    sample klo of the whole-sample rule lies above the box.  The probes fall, nothing else rises."""
    rb, _, _, st = _run(oracle, small_scene.terrain, _lattice_poses(n_poses), _fan(fan_name),
                        stats=True)
    assert rb.sum() > 0
    new, old = st[None], st["0"]
    print("PCP_FAN_CLIP default", new, "=0", old)
    assert new["samples_visited"] < old["samples_visited"]
    assert new["scanned_stencils"] <= old["scanned_stencils"]
    assert new["point_tests"] <= old["point_tests"]


# (b) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_entry_on_a_sample(oracle, small_scene, fan_name, n_poses):
    """Pose heights at which a descending ring of a custom elevation table enters the box's top
    face at t = 0.5 + 0.3 k: (t0 - 0.5) / 0.3 is an integer up to float rounding, on either side
    of it across the poses, and that sample must stay in."""
    fan = _fan(fan_name, el_min=-1.2, el_max=0.4)
    _, _, _, se = oracle.fan_tables(fan.n_az, fan.n_el, fan.el_min, fan.el_max)
    se = np.asarray(se)
    down = np.nonzero(se < -0.05)[0]
    top = _box_top(small_scene.terrain)
    s = _steps(8)
    poses = _lattice_poses(n_poses)
    i = np.arange(n_poses)
    poses[:, 2] = top - se[down[i % down.size]] * s[(i // down.size) % 6]
    rb, _, rfh, _ = _run(oracle, small_scene.terrain, poses, fan)
    assert rb.sum() > 0 and (rfh >= 0).any()


# (c) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_spike_sets_the_box_top(oracle, fan_name, n_poses):
    """A flat sheet with one point 0.5 m above it: the spike alone sets the box's top, so a ray
    aimed at it has its first hit at its first sample inside the box."""
    spike = np.array([2.0, 2.0, 0.5])
    terrain = _cloud(np.concatenate([_sheet(0.0, 4.0, 0.0, 4.0, 0.0, d=0.08), spike[None]], 0))
    fan = _fan(fan_name)
    _, _, ce, se = oracle.fan_tables(fan.n_az, fan.n_el, fan.el_min, fan.el_max)
    ce, se = np.asarray(ce), np.asarray(se)
    s = _steps(8)
    i = np.arange(n_poses)
    j = i % 3                                   # the three steepest descending rings
    k = (i // 3) % 6
    yaw = 0.5 * i
    d = np.stack([ce[j] * np.cos(yaw), ce[j] * np.sin(yaw), se[j]], 1)     # azimuth 0 of ring j
    xyz = spike[None, :] - d * s[k][:, None]
    poses = np.concatenate([xyz, np.zeros((n_poses, 1)), yaw[:, None]], 1)
    _, _, rfh, _ = _run(oracle, terrain, poses, fan)
    aimed = rfh[i, j, 0]
    assert np.array_equal(aimed, k), (aimed, k)   # hit at the spike, no sample before it


# (d) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_inside_and_below(oracle, small_scene, fan_name, n_poses):
    """Poses inside the box (in the pit, z = -0.5) and below the terrain looking up (z = -2.5):
    t0 = 0 for the former, ascending entries through the bottom face for the latter."""
    i = np.arange(n_poses)
    inside = np.stack([3.6 + (i * 0.13) % 0.8, -0.8 + (i * 0.37) % 1.6, np.full(n_poses, -0.5)], 1)
    below = _lattice_poses(n_poses, z=-2.5)[:, :3]
    xyz = np.where((i % 2 == 0)[:, None], inside, below)
    poses = np.concatenate([xyz, np.full((n_poses, 1), -0.3), (0.5 * i)[:, None]], 1)
    fan = _fan(fan_name)
    _, _, rfh, _ = _run(oracle, small_scene.terrain, poses, fan)
    up = fan.n_el // 2
    assert (rfh[0::2] >= 0).any() and (rfh[1::2, up:, :] >= 0).any()


# (e) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_level_ring_inside_the_box(oracle, small_scene, fan_name, n_poses):
    """An elevation table with a ring at exactly el = 0 and rings mirrored about it, poses at
    heights inside the box, yaw in multiples of 90 degrees: direction components that are 0 (the
    z slab's times are infinite) or 6e-17 (cos of pi / 2)."""
    n_az, n_el = FANS[fan_name]
    span = 1.5                                           # radians: (span (j0 + 0.5)) / n_el is exact
    j0 = n_el // 2 - 1
    el_min = -(span * (j0 + 0.5)) / n_el
    fan = _fan(fan_name, el_min=el_min, el_max=el_min + span)
    _, _, _, se = oracle.fan_tables(n_az, n_el, fan.el_min, fan.el_max)
    assert np.asarray(se)[j0] == 0.0
    i = np.arange(n_poses)
    poses = _lattice_poses(n_poses)
    poses[:, 2] = np.array([0.02, 0.06, -0.02, -0.5])[i % 4]
    poses[:, 3] = 0.0
    poses[:, 4] = (np.pi / 2) * (i % 4)
    rb, _, rfh, _ = _run(oracle, small_scene.terrain, poses, fan)
    assert rb.sum() > 0 and (rfh[:, j0, :] >= 0).any()


# (f) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_three_kilometres_out(oracle, small_scene, fan_name, n_poses):
    """The lattice shifted 3 km in x, y and z: float spacing there is 2.4e-4 m, the part of the
    rule's bound that the box's own 1e-6 |coord| carries."""
    shift = np.array([3000.0, 3000.0, 3000.0])
    terr = np.ascontiguousarray(small_scene.terrain.copy())
    terr[:, :3] += shift.astype(np.float32)
    poses = _lattice_poses(n_poses)
    poses[:, :3] += shift
    rb, _, _, _ = _run(oracle, terr, poses, _fan(fan_name))
    assert rb.sum() > 0


# (g) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [256, 257, 365])
@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_long_marches(oracle, fan_name, n_poses, n_steps):
    """max_distance giving K = 256, 257 and 365 samples over a 112 m strip: rays that run along
    the strip are blocked near their last samples, where khi meets K - 1."""
    terrain = _cloud(_sheet(0.0, 112.0, -0.25, 0.25, 0.0, d=0.1))
    end = 0.5 + 0.3 * (n_steps - 1) + 0.15          # s_(K-1) < end < s_K
    fan = _fan(fan_name, el_min=-0.012, el_max=0.004, max_distance=end + 0.08)
    assert _abi.step_table(end).size == n_steps
    i = np.arange(n_poses)
    poses = np.stack([0.3 + 0.37 * i, 0.02 * (i % 3 - 1), 0.45 + 0.05 * i, np.zeros(n_poses),
                      np.zeros(n_poses)], 1)
    _, _, rfh, _ = _run(oracle, terrain, poses, fan)
    assert (rfh >= 150).any()                        # hits deep into the march
