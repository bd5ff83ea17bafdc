"""The fan march with its pose-uniform terms taken from the pose row (pcp_fan_row.hpp) and the
production kernel's layout facts fixed at compile time ("VALU diet 2") on the GPU.
Every case compares blocked, units and first_hit bit for bit with the oracle, which probes every
sample, over the fine-window copy (PCP_TERRAIN_BLOCKS=2, built at the first query), and runs the
plain call without first hits as well.  Fans are 64 x 8 and 96 x 6 (96 is no multiple of 64: the
non-uniform kernels); 3, 8, 16 and 64 poses run the interleaved kernel and one, two and eight poses
per wave -- every kernel of the launcher at its smallest shape.  The probe arithmetic itself is
pinned by the march counters of two cases, recorded from the parent build
(tests/golden/fan_valu_stats.json)."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

FANS = {"64x8": (64, 8), "96x6": (96, 6)}
COMBOS = [(f, n) for f in ("64x8", "96x6") for n in (3, 8, 16, 64)]
GOLDEN = Path(__file__).resolve().parent / "golden" / "fan_valu_stats.json"
SHIFT = np.array([3000.0, 3000.0, 3000.0])


def _fan(name, el_min=-85.0 * np.pi / 180.0, el_max=85.0 * np.pi / 180.0, max_distance=15.0):
    n_az, n_el = FANS[name]
    return _abi.FanParams(n_az, n_el, el_min, el_max, max_distance)


def _level_fan(name):
    """A fan with a ring at exactly el = 0 (sin = 0: the z slab's reciprocal is infinite) and
    rings mirrored about it, as tests/test_fan_clip.py builds it."""
    n_el = FANS[name][1]
    span = 1.5
    j0 = n_el // 2 - 1
    el_min = -(span * (j0 + 0.5)) / n_el
    return _fan(name, el_min=el_min, el_max=el_min + span), j0


def _far(terrain):
    t = np.ascontiguousarray(terrain.copy())
    t[:, :3] += SHIFT.astype(np.float32)
    return t


def _context(terrain):
    """A context over the fine copy (the knob is read when the terrain is set)."""
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


@pytest.fixture(scope="module")
def contexts(small_scene):
    """One context per terrain for the module: the lattice and the lattice 3 km out."""
    made = {}

    def get(key):
        if key not in made:
            terrain = small_scene.terrain if key == "near" else _far(small_scene.terrain)
            made[key] = (terrain, _context(terrain))
        return made[key]

    yield get
    for _, ctx in made.values():
        ctx.close()


def _check(oracle, contexts, key, poses, fan):
    terrain, ctx = contexts(key)
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
    """n poses spread over the small scene's 10 m x 10 m lattice (x -2..8, y -4..6); every second
    yaw is a multiple of 90 degrees: sin(0) = 0 exactly, so azimuth 0 of those poses runs along
    an axis with a direction component of exactly 0, the others' components are 6e-17."""
    k = np.arange(n)
    x = -1.0 + (k * 2.3) % 8.0
    y = -3.0 + (k * 3.1) % 8.0
    yaw = np.where(k % 2 == 0, (np.pi / 2) * ((k // 2) % 4), 0.7 * k - 2.0)
    return np.stack([x, y, np.full(n, z), -0.4 + 0.01 * k, yaw], axis=1)


def mixed_height_poses(n):
    """Heights from inside the pit to far above the fan's range in one call: at 30 m and -25 m
    no ring reaches the box (all dead), at 6 m and 11 m only the steep descending ones do."""
    p = lattice_poses(n)
    p[:, 2] = np.array([1.1, 30.0, 6.0, -0.5, 11.0, -25.0, 0.4, 14.9])[np.arange(n) % 8]
    return p


def in_out_below_poses(n):
    """Outside the box in xy (20 m off: the x or y slab is entered late or never), inside the box
    (in the pit) and below the terrain looking up, by turns."""
    i = np.arange(n)
    p = lattice_poses(n)
    outside = np.stack([np.where(i % 2 == 0, -12.0, 3.0 + 0.1 * i),
                        np.where(i % 2 == 0, 1.0 + 0.1 * i, 18.0), np.full(n, 1.5)], 1)
    inside = np.stack([3.6 + (i * 0.13) % 0.8, -0.8 + (i * 0.37) % 1.6, np.full(n, -0.5)], 1)
    below = np.stack([p[:, 0], p[:, 1], np.full(n, -2.5)], 1)
    p[:, :3] = np.where((i % 3 == 0)[:, None], outside,
                        np.where((i % 3 == 1)[:, None], inside, below))
    return p


# the two cases whose march counters the parent build recorded (GOLDEN): name -> terrain key,
# fan, poses
STATS_CASES = {
    "lattice_64x8_64": ("near", "64x8", lambda: lattice_poses(64)),
    "far_mixed_96x6_16": ("far", "96x6",
                          lambda: mixed_height_poses(16) + np.concatenate([SHIFT, [0.0, 0.0]])),
}


@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_lattice_axis_rays(oracle, contexts, fan_name, n_poses):
    """Poses 1.1 m over the lattice, a yaw sweep with rays along the axes, and a ring at el = 0:
    zero direction components in x or y and in z, whose clip reciprocals are infinite."""
    rb, _, rfh = _check(oracle, contexts, "near", lattice_poses(n_poses), _fan(fan_name))
    assert rb.sum() > 0
    fan, j0 = _level_fan(fan_name)
    poses = lattice_poses(n_poses)
    poses[:, 2] = np.array([0.02, 0.06, -0.02, -0.5])[np.arange(n_poses) % 4]
    rb, _, rfh = _check(oracle, contexts, "near", poses, fan)
    assert rb.sum() > 0 and (rfh[:, j0, :] >= 0).any()


@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_dead_and_live_poses_in_one_call(oracle, contexts, fan_name, n_poses):
    """Poses of different heights: some poses' rings are all dead, others' partly, others' all
    live -- the per-pose dead test reads the live-ring pair from its slot of the wider row."""
    poses = mixed_height_poses(n_poses)
    rb, ru, rfh = _check(oracle, contexts, "near", poses, _fan(fan_name))
    high = np.nonzero(poses[:, 2] == 30.0)[0]
    assert rb[poses[:, 2] == 1.1].sum() > 0
    # (a pose out of reach: nothing blocked, every ray its K samples)
    assert (rb[high] == 0).all() and (rfh[high] == -1).all() and (ru[high] == ru[high][0]).all()


@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_outside_inside_below(oracle, contexts, fan_name, n_poses):
    rb, _, rfh = _check(oracle, contexts, "near", in_out_below_poses(n_poses), _fan(fan_name))
    assert (rfh[1::3] >= 0).any() and (rfh[2::3] >= 0).any()


@pytest.mark.parametrize("fan_name,n_poses", COMBOS)
def test_three_kilometres_out(oracle, contexts, fan_name, n_poses):
    """The lattice shifted 3 km in x, y and z: the row's host floats at large magnitudes (float
    spacing 2.4e-4 m), mixed heights among them."""
    poses = lattice_poses(n_poses)
    poses[1::4, 2] = 6.0
    poses[:, :3] += SHIFT
    rb, _, _ = _check(oracle, contexts, "far", poses, _fan(fan_name))
    assert rb.sum() > 0


@pytest.mark.parametrize("case", sorted(STATS_CASES))
def test_probe_arithmetic_unchanged(contexts, case):
    """The march's counters -- probes, walk starts, point tests, directory loads -- are the
    parent build's to the unit: the probe visits the same samples and reads the same records."""
    golden = json.loads(GOLDEN.read_text())
    key, fan_name, make = STATS_CASES[case]
    _, ctx = contexts(key)
    got = ctx.raycast_fan_stats(np.ascontiguousarray(make(), np.float64), _fan(fan_name))
    print(case, got)
    assert got == golden["cases"][case]["stats"]
