"""The fan march's pivot test (DESIGN.md §5 Skip 6, pcp_fan_pivot.hpp) on the GPU: a candidate
sample first tests the point of its window nearest its fine cell's centre and is blocked if that
point is within r; otherwise it walks the window as before.  Every parity case compares blocked,
units and first_hit bit for bit with the oracle with PCP_FAN_PIVOT=1 and =0; the table is read
back with pcp_debug_fine_pivot and checked against the window rule of tests/fine_ref.py.

Every context has PCP_TERRAIN_BLOCKS=2, so the first query builds the fine copy.  64 poses x
(64 x 16) run the 8-poses-per-wave kernel; 3 poses x (40 x 9) the non-uniform-ring kernels."""
import os

import numpy as np
import pytest

import fine_ref
from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

SHAPES = {"p64_64x16": (64, 64, 16), "p3_40x9": (3, 40, 9)}


def _context(terrain, pivot):
    """A context with the knob set (read when the context is created)."""
    env = {"PCP_FAN_PIVOT": pivot, "PCP_TERRAIN_BLOCKS": "2"}
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


def _cloud(xyz):
    """(N, 8) float32 PointXYZRGB image of the points."""
    return synth._pack(np.asarray(xyz, np.float32), (255, 0, 0))


def _level_sheet(n=60, d=0.05, sigma=0.01, seed=7):
    rng = np.random.default_rng(seed)
    s = fine_ref.sheet(0.0, n * d, 0.0, n * d, 0.0, d)
    s[:, 2] = rng.normal(0.0, sigma, s.shape[0])
    return s


def _two_sheets():
    """A 3 m sheet at z = 0, a 2 m sheet 1 m above its middle, and a wall beside it: the columns
    under the upper sheet hold both levels, so about half their pivots lie on the level a ray
    does not reach."""
    return np.concatenate([fine_ref.sheet(0.0, 3.0, 0.0, 3.0, 0.0),
                           fine_ref.sheet(0.5, 2.5, 0.5, 2.5, 1.0) + [0.013, 0.021, 0.0],
                           fine_ref.wall(2.7, 0.5, 2.5, 0.0, 0.6, per_step=12)], 0)


def _holed_sheet():
    s = _level_sheet(seed=11)
    keep = (np.abs(s[:, 0] - 1.5) > 0.25) | (np.abs(s[:, 1] - 1.4) > 0.25)   # a 0.5 m hole
    return s[keep]


@pytest.fixture(scope="module")
def scenes(small_scene):
    t = small_scene.terrain
    keep = (t[:, 0] >= 2.5) & (t[:, 0] < 6.5) & (t[:, 1] >= -2.0) & (t[:, 1] < 2.0)
    cut = np.ascontiguousarray(t[keep])
    assert cut.shape[0] >= 6000
    far = _level_sheet() + np.array([3000.0, -2000.0, 1000.0])
    return {"cut": cut, "level": _cloud(_level_sheet()), "two_sheets": _cloud(_two_sheets()),
            "hole": _cloud(_holed_sheet()), "far": _cloud(far)}


def _poses(terrain, n):
    """n poses 0.3 .. 1.5 m above the scene's top, spread over its extent and 0.4 m beyond it,
    pitched down, every yaw: most rays meet the terrain, some leave it."""
    xyz = terrain[:, :3].astype(np.float64)
    lo, hi = xyz.min(0), xyz.max(0)
    k = np.arange(n)
    u, v = (k * 0.618034) % 1.0, (k * 0.414214 + 0.3) % 1.0
    x = lo[0] - 0.4 + (hi[0] - lo[0] + 0.8) * u
    y = lo[1] - 0.4 + (hi[1] - lo[1] + 0.8) * v
    z = hi[2] + 0.3 + 1.2 * ((k * 0.29) % 1.0)
    return np.ascontiguousarray(np.stack([x, y, z, -0.5 + 0.02 * (k % 11), 0.7 * k - 2.0], 1))


@pytest.fixture(scope="module")
def reference(oracle, scenes):
    """The oracle's answer per (scene, shape), computed once and left unchanged."""
    cache = {}

    def get(scene, shape):
        if (scene, shape) not in cache:
            P, n_az, n_el = SHAPES[shape]
            fan = _abi.fan_params(n_az=n_az, n_el=n_el)
            poses = _poses(scenes[scene], P)
            oracle.set_threads(8)
            try:
                rb, ru, rfh = oracle.raycast_fan(oracle.Cloud(scenes[scene]), poses, fan.n_az,
                                                 fan.n_el, fan.el_min, fan.el_max,
                                                 fan.max_distance)
            finally:
                oracle.set_threads(1)
            for a in (rb, ru, rfh):
                a.flags.writeable = False
            cache[scene, shape] = (poses, fan, rb, ru, rfh)
        return cache[scene, shape]
    return get


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("scene", ["cut", "level", "two_sheets", "hole", "far"])
def test_parity(scenes, reference, scene, shape):
    poses, fan, rb, ru, rfh = reference(scene, shape)
    assert rb.sum() > 0 and (rfh < 0).any()   # rays that hit and rays that leave the terrain
    for pivot in ("1", "0"):
        ctx = _context(scenes[scene], pivot)
        try:
            b, u, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
            info = ctx.terrain_info()
            b2, u2, _, _ = ctx.raycast_fan(poses, fan)   # (the benchmark's call: no first hits)
            geo, _ = ctx.debug_fine_pivot()
        finally:
            ctx.close()
        assert info["scan_layout"] == "fine" and info["fine_pivot"] == 1
        assert geo["built"] == 1 and geo["enabled"] == int(pivot)
        np.testing.assert_array_equal(fh, rfh, err_msg=f"PCP_FAN_PIVOT={pivot}")
        np.testing.assert_array_equal(b, rb, err_msg=f"PCP_FAN_PIVOT={pivot}")
        np.testing.assert_array_equal(u, ru, err_msg=f"PCP_FAN_PIVOT={pivot}")
        np.testing.assert_array_equal(b2, rb)
        np.testing.assert_array_equal(u2, ru)


@pytest.mark.parametrize("scene", ["cut", "two_sheets"])
def test_table(scenes, scene):
    """Every cell's pivot is a member of its window, no member is strictly nearer the cell's
    centre in double, and empty windows and padding slots hold the sentinel."""
    terrain = scenes[scene]
    ctx = _context(terrain, "1")
    try:
        assert ctx.debug_fine_pivot()[0]["built"] == 0          # nothing before the first query
        ctx.raycast_fan(_poses(terrain, 1), _abi.fan_params(n_az=8, n_el=4))
        pg, piv = ctx.debug_fine_pivot()
        geo, _, _, pts = ctx.debug_fine_copy()
    finally:
        ctx.close()
    assert pg["built"] == 1 and geo["built"] == 1 and geo["tile"] == 2
    fnx, fny = geo["fnx"], geo["fny"]
    assert (pg["fnx"], pg["fny"], pg["ox"], pg["oy"], pg["cf"]) == \
        (fnx, fny, geo["ox"], geo["oy"], geo["cf"])
    tx, ty = -(-fnx // 8), -(-fny // 8)
    assert (pg["tx"], pg["ty"], pg["n_slots"], pg["bytes"]) == (tx, ty, tx * ty * 64, tx * ty * 768)
    assert piv.shape == (tx * ty * 64, 3)
    wy, wx = np.divmod(np.arange(fnx * fny, dtype=np.int64), fnx)
    slot = ((wy // 8) * tx + wx // 8) * 64 + (wy % 8) * 8 + wx % 8
    cell = piv[slot]                                               # per window, x-fastest
    # the windows' members, by fine_ref's rule
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    ws, ps, _, _ = fine_ref._window_pairs(geo, x, y)

    def d2(w, px, py):
        dx = px - (geo["ox"] + ((w % fnx).astype(np.float64) + 0.5) * geo["cf"])
        dy = py - (geo["oy"] + ((w // fnx).astype(np.float64) + 0.5) * geo["cf"])
        return dx * dx + dy * dy
    best = np.full(fnx * fny, np.inf)
    np.minimum.at(best, ws, d2(ws, x[ps], y[ps]))
    count = np.bincount(ws, minlength=fnx * fny)
    full = count > 0
    is_pivot = (pts[ps, :3] == cell[ws, :3]).all(1)
    member = np.zeros(fnx * fny, bool)
    member[ws[is_pivot]] = True
    assert member[full].all(), np.nonzero(full & ~member)[0][:5]
    got = d2(np.arange(fnx * fny), cell[:, 0].astype(np.float64), cell[:, 1].astype(np.float64))
    assert (got[full] <= best[full]).all(), np.nonzero(full & ~(got <= best))[0][:5]

    def sentinel(a):
        return np.isnan(a[:, 0]) & np.isnan(a[:, 1]) & np.isneginf(a[:, 2])
    assert sentinel(cell[~full]).all() and not sentinel(cell[full]).any()
    pad = np.ones(piv.shape[0], bool)
    pad[slot] = False
    assert sentinel(piv[pad]).all()
    print(scene, "windows", int(full.sum()), "empty", int((~full).sum()), "padding", int(pad.sum()))
    assert full.any() and (~full).any() and pad.any()
    if scene == "two_sheets":   # columns that hold both sheets, and pivots on either of them
        zc = cell[full, 2]
        assert (zc > 0.9).sum() > 100 and (zc < 0.1).sum() > 100


def test_not_vacuous(scenes, reference):
    """On the level sheet the pivot settles candidates: the same samples are probed, fewer walk
    starts are loaded, and points are still tested."""
    poses, fan, _, _, _ = reference("level", "p64_64x16")
    st = {}
    ctxs = {p: _context(scenes["level"], p) for p in ("1", "0")}
    try:
        for p, ctx in ctxs.items():
            ctx.raycast_fan(poses, fan)
            st[p] = ctx.raycast_fan_stats(poses, fan)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    print(st)
    assert st["1"]["samples_visited"] == st["0"]["samples_visited"]
    assert st["1"]["scanned_stencils"] < st["0"]["scanned_stencils"]
    assert st["1"]["point_tests"] > 0


def test_score_poses_unaffected(scenes, small_scene):
    """Cell scoring's kernels do not take the pivot: its totals, covered counts and flags on the
    cut scene are the same with the knob 1 and 0."""
    cells = synth.excavation_cells(small_scene.area)
    params = _abi.default_vl_params()
    k = np.arange(12)
    poses = np.stack([4.6 + 1.9 * np.cos(0.55 * k), 0.0 + 1.7 * np.sin(0.55 * k),
                      np.full(12, 1.1), np.full(12, -0.4), 0.55 * k + np.pi], 1)
    res = {}
    for pivot in ("1", "0"):
        ctx = _context(scenes["cut"], pivot)
        try:
            ctx.set_cells(cells.xyz, cells.normals)
            ctx.raycast_fan(poses[:1], _abi.fan_params(n_az=8, n_el=4))   # builds the copy
            assert ctx.terrain_info()["scan_layout"] == "fine"
            fl = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, small_scene.zx120_pose5, params, fl)
            res[pivot] = (tot, cov, rep.best_idx, fl)
        finally:
            ctx.close()
    assert (res["1"][1] > 0).any()
    assert res["1"][0].tobytes() == res["0"][0].tobytes()
    np.testing.assert_array_equal(res["1"][1], res["0"][1])
    assert res["1"][2] == res["0"][2]
    np.testing.assert_array_equal(res["1"][3], res["0"][3])
