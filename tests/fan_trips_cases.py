"""The scenes and poses of tests/test_fan_trips.py, shared with tools/gen/fan_trips_stats.py (which
records tests/golden/fan_trips_stats.json from a build): terrains of a few dozen points whose fine
windows hold runs of 0 to 4 and more entries, and poses that each aim one ray of a 64 x 8 fan at a
point of the terrain, from dead on to just past its radius."""
import numpy as np

import mount_ref
import scan_ref

R = 0.08 * 0.7                     # the march's radius
SHIFT = np.array([3000.0, 3000.0, 3000.0])
BASE = np.array([2.013, 1.017, 0.2])   # where every scene stands


def terrain_of(xyz):
    out = np.zeros((len(xyz), 8), np.float32)
    out[:, :3] = np.asarray(xyz, np.float64)
    out[:, 3] = 1.0
    return np.ascontiguousarray(out)


def _single():
    """One point: its window and the windows around it hold runs of one entry."""
    return [BASE]


def _pair():
    """Two points 3 cm apart in z, 2 mm apart in x and y: one fine cell, runs of two."""
    return [BASE, BASE + [0.002, 0.002, 0.03]]


def _strip():
    """A level strip, one row of 30 points 5 cm apart: a window spans three or four of them, the
    ends one and two.  Grazing rays pass above and below without a hit and walk to the sentinel."""
    k = np.arange(30)
    return np.stack([BASE[0] + 0.05 * k, BASE[1] + 0.004 * (k % 3), BASE[2] + 0.002 * (k % 2)], 1)


def _wall():
    """A wall: three columns 6 cm apart, 12 points each every 5 cm in z -- windows over several
    z levels with non-zero skip counts, odd and even walk starts."""
    c, k = np.meshgrid(np.arange(3), np.arange(12), indexing="ij")
    return np.stack([BASE[0] + 0.003 * (k.ravel() % 2), BASE[1] + 0.06 * c.ravel(),
                     BASE[2] + 0.05 * k.ravel()], 1)


def _corner():
    """Every point in one fine cell: the grid is its bounding box plus a coarse cell each side, so
    its windows' runs are the last non-empty ones of the entry array and every window beyond, to
    the largest (wx, wy), is empty; the aimed rays march on through those."""
    return [BASE + [0.001 * i, 0.001 * (i % 2), 0.012 * i] for i in range(4)]


SCENES = {"single": _single, "pair": _pair, "strip": _strip, "wall": _wall, "corner": _corner}


def scene_xyz(name):
    return np.asarray(SCENES[name](), np.float64).reshape(-1, 3)


def fan_64x8(max_distance=15.0):
    from pointcloud_processor_amd import _abi

    return _abi.FanParams(64, 8, -85.0 * np.pi / 180.0, 85.0 * np.pi / 180.0, max_distance)


def max_distance_for(K):
    """A range whose step table has exactly K samples: s_k = 0.5 + 0.3 k < max_distance - 0.08 for
    k < K, with half a step of room either side of the end."""
    d = 0.08 + 0.5 + 0.3 * (K - 1) + 0.15
    assert scan_ref.step_table(d - 0.08).size == K
    return d


# the aimed ray's miss distances: dead on, inside, at the radius' edge either side, past it
OFFSETS = np.array([0.0, 0.02, 0.045, R - 0.002, R + 0.002, 0.075])


def aimed_poses(xyz, n, fan):
    """n level poses; pose p aims ray (ring 1 + p % 6, azimuth 5 p % 64) at sample 2 + p % 5 at
    point p % len(xyz), missing it by OFFSETS[p % 6] along a direction that turns with p -- above,
    below, beside: hits in the first entries of a run, grazes between and past its points."""
    xyz = np.asarray(xyz, np.float64)
    poses = np.zeros((n, 5))
    steps = scan_ref.step_table(fan.max_distance - mount_ref.KVIS)
    for p in range(n):
        yaw = 0.37 * p - 1.0
        d = mount_ref.directions(np.array([[0.0, 0.0, 0.0, 0.0, 0.0, yaw]]), fan)[0]
        j, i, k = 1 + p % 6, (5 * p) % 64, min(2 + p % 5, steps.size - 1)
        a = 2.1 * p
        off = OFFSETS[p % 6] * np.array([np.cos(a) * np.cos(0.7 * p), np.sin(a) * np.cos(0.7 * p),
                                         np.sin(0.7 * p)])
        poses[p, :3] = xyz[p % len(xyz)] + off - d[j, i] * steps[k]
        poses[p, 3] = -0.4
        poses[p, 4] = yaw
    return np.ascontiguousarray(poses)


def shifted(terrain):
    t = np.ascontiguousarray(terrain.copy())
    t[:, :3] += SHIFT.astype(np.float32)
    return t


# name -> (scene, poses, shifted): the walk cases, each at 64 poses (eight per wave) and 8 (one)
WALK_CASES = {f"{s}_{n}": (s, n, False) for s in SCENES for n in (64, 8)}
WALK_CASES["wall_far_64"] = ("wall", 64, True)


def walk_case(name):
    """-> (terrain [n, 8] float32, poses [P, 5], fan)."""
    scene, n, far = WALK_CASES[name]
    fan = fan_64x8()
    terrain = terrain_of(scene_xyz(scene))
    if far:
        terrain = shifted(terrain)
    # (aimed at the float32 points the terrain really holds)
    return terrain, aimed_poses(terrain[:, :3].astype(np.float64), n, fan), fan
