"""The tight twin of the split records' probe thresholds (DESIGN.md §5 Skip 7, pcp_fan_band.hpp)
on the GPU: the twin is read back with pcp_debug_fine_band and checked against the rule in
tests/band_ref.py; every fan case compares blocked, units and first_hit bit for bit with the
oracle with PCP_FAN_BAND=1 and =0; the specified copy is byte-identical between the two.

Every context has PCP_TERRAIN_BLOCKS=2, so the first query builds the fine copy.  Terrains of at
most 4 k points, fans of at most 128 x 16, at most 16 poses."""
import os

import numpy as np
import pytest

import band_ref
import fine_ref
from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu


def _context(terrain, band):
    """A context with the knob set (read when the context is created)."""
    env = {"PCP_FAN_BAND": band, "PCP_TERRAIN_BLOCKS": "2"}
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


def _noisy(s, sigma, seed):
    s = s.copy()
    s[:, 2] += np.random.default_rng(seed).normal(0.0, sigma, s.shape[0])
    return s


def _step_slope():
    """A level sheet, a sheet 0.3 m above it (the step), and a 45 degree slope up from there:
    3000 points, 37 x 33 coarse cells (no multiple of 4 in fine cells either way)."""
    lvl = fine_ref.sheet(0.0, 1.5, 0.0, 2.5, 0.0)
    stp = fine_ref.sheet(1.5, 2.0, 0.0, 2.5, 0.3)
    slp = fine_ref.sheet(2.0, 3.0, 0.0, 2.5, 0.0)
    slp[:, 2] = 0.3 + (slp[:, 0] - 2.0)
    return _noisy(np.concatenate([lvl, stp, slp], 0), 0.004, 3)


def _strip():
    """A level strip (noise 0.01 m) of 0.3 m x 28 m along x, 8 m .. 36 m out: what a ray from
    1.1 m above its level meets at 2 .. 8 degrees below the horizon."""
    return _noisy(fine_ref.sheet(8.0, 36.0, 0.0, 0.3, 0.0), 0.01, 7)


@pytest.fixture(scope="module")
def scenes():
    ss = _step_slope()
    sc = {"slope": ss, "lifted": ss + np.array([0.0, 0.0, 1000.0]), "grazing": _strip(),
          "wall": fine_ref.wall_terrain(2.0), "one_point": np.array([[0.3, -0.2, 0.1]])}
    assert all(v.shape[0] <= 4096 for v in sc.values())
    return {k: _cloud(v) for k, v in sc.items()}


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


def _case(scenes, scene):
    """(poses, fan) of a scene's fan case."""
    if scene == "grazing":
        # 16 poses 1.1 m above the strip's level at its near side, level, looking along it (the
        # azimuth 0 column of each runs down the strip); rings from 1.9 to 5.7 degrees below
        # the horizon: sin(el) 0.3 m = 1 .. 3 cm of descent per sample, the ground met 11 m ..
        # 33 m out
        k = np.arange(16)
        poses = np.stack([-1.5 + 0.09 * k, 0.06 + 0.012 * k, np.full(16, 1.1), np.zeros(16),
                          0.003 * (k % 5 - 2)], 1)
        return np.ascontiguousarray(poses), _abi.fan_params(n_az=128, n_el=16, el_min_deg=-5.7,
                                                            el_max_deg=-1.9, max_distance=40.0)
    return _poses(scenes[scene], 16), _abi.fan_params(n_az=64, n_el=16)


@pytest.fixture(scope="module")
def reference(oracle, scenes):
    """The oracle's answer per scene, computed once and left unchanged."""
    cache = {}

    def get(scene):
        if scene not in cache:
            poses, fan = _case(scenes, scene)
            oracle.set_threads(8)
            try:
                rb, ru, rfh = oracle.raycast_fan(oracle.Cloud(scenes[scene]), poses, fan.n_az,
                                                 fan.n_el, fan.el_min, fan.el_max,
                                                 fan.max_distance)
            finally:
                oracle.set_threads(1)
            for a in (rb, ru, rfh):
                a.flags.writeable = False
            cache[scene] = (poses, fan, rb, ru, rfh)
        return cache[scene]
    return get


@pytest.fixture(scope="module")
def runs(scenes, reference):
    """Per scene and knob setting: the fan's outputs, its stats, the copy's bytes, the twin."""
    cache = {}

    def get(scene):
        if scene not in cache:
            poses, fan, _, _, _ = reference(scene)
            out = {}
            for band in ("1", "0"):
                ctx = _context(scenes[scene], band)
                try:
                    assert ctx.debug_fine_band()[1] is None   # nothing before the first query
                    b, u, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
                    b2, u2, _, _ = ctx.raycast_fan(poses, fan)   # (the benchmark's call)
                    st = ctx.raycast_fan_stats(poses, fan)
                    info = ctx.terrain_info()
                    geo, frec, wpts, pts = ctx.debug_fine_copy()
                    enabled, twin = ctx.debug_fine_band()
                finally:
                    ctx.close()
                assert info["scan_layout"] == "fine" and geo["tile"] == 2 and enabled == int(band)
                out[band] = dict(b=b, u=u, fh=fh, b2=b2, u2=u2, st=st, geo=geo, frec=frec,
                                 wpts=wpts, pts=pts, twin=twin)
            cache[scene] = out
        return cache[scene]
    return get


@pytest.mark.parametrize("scene", ["slope", "lifted", "one_point"])
def test_twin(runs, scene):
    """The twin as built against the rule, whatever the knob: sound, within a step of the
    real-number bound, never looser than the specified copy, empty and padding records copied."""
    for band in ("1", "0"):
        r = runs(scene)[band]
        assert r["twin"] is not None
        assert band_ref.check_band(r["pts"], r["geo"], r["frec"], r["twin"]) == []
    r = runs(scene)["1"]
    np.testing.assert_array_equal(r["twin"], runs(scene)["0"]["twin"])
    idx, _ = fine_ref.record_index(r["geo"])
    s = band_ref.spec_words(r["geo"], r["frec"])[idx].astype(np.int64)
    t = r["twin"][idx].astype(np.int64)
    live = (s & 255) != 255
    lower_hi, higher_lo = int(((t >> 8) < (s >> 8))[live].sum()), int(((t & 255) > (s & 255))[live].sum())
    print(scene, "records", int(live.sum()), "hi tightened", lower_hi, "lo tightened", higher_lo,
          "mean steps", float(((s >> 8) - (t >> 8))[live].mean()), float(((t & 255) - (s & 255))[live].mean()))
    assert live.any() and (~live).any() and r["twin"].size > idx.size
    if scene != "one_point":
        # the step and the slope: windows whose extreme entries lie at the rim
        assert lower_hi > live.sum() // 4 and higher_lo > live.sum() // 8
        assert ((s >> 8) - (t >> 8))[live].max() >= 10
    else:
        # one point: the grid's origin lies one coarse cell from it, so it sits on a corner of
        # four fine cells, at distance 0 from each, and no other window holds it: the full reach
        # in all 4 x 2 records, and the twin is the copy up to the rounding
        assert int(live.sum()) == 8 and ((s >> 8) - (t >> 8))[live].max() <= 1


def test_no_points():
    """No terrain points: no fine copy and no twin, and the fan sees nothing."""
    ctx = _context(np.zeros((0, 8), np.float32), "1")
    try:
        poses = np.array([[0.0, 0.0, 1.0, -0.4, 0.0]])
        b, u, _, _ = ctx.raycast_fan(poses, _abi.fan_params(n_az=8, n_el=4))
        ctx.raycast_fan(poses, _abi.fan_params(n_az=8, n_el=4))
        enabled, twin = ctx.debug_fine_band()
    finally:
        ctx.close()
    assert enabled == 1 and twin is None and int(b.sum()) == 0


@pytest.mark.parametrize("scene", ["grazing", "wall", "slope", "lifted"])
def test_parity(reference, runs, scene):
    poses, fan, rb, ru, rfh = reference(scene)
    assert rb.sum() > 0 and (rfh < 0).any()   # rays that hit and rays that leave the terrain
    if scene == "grazing":
        assert (rfh >= 36).sum() >= 100       # hits after 1.1 m of descent at <= 3 cm a sample
    for band in ("1", "0"):
        r = runs(scene)[band]
        np.testing.assert_array_equal(r["fh"], rfh, err_msg=f"PCP_FAN_BAND={band}")
        np.testing.assert_array_equal(r["b"], rb, err_msg=f"PCP_FAN_BAND={band}")
        np.testing.assert_array_equal(r["u"], ru, err_msg=f"PCP_FAN_BAND={band}")
        np.testing.assert_array_equal(r["b2"], rb)
        np.testing.assert_array_equal(r["u2"], ru)


@pytest.mark.parametrize("scene", ["grazing", "wall", "slope", "lifted"])
def test_stats(runs, scene):
    """The same samples are probed; the twin takes candidates away and never adds one."""
    on, off = runs(scene)["1"]["st"], runs(scene)["0"]["st"]
    print(scene, "on", on, "off", off)
    assert on["samples_visited"] == off["samples_visited"] > 0
    assert on["scanned_stencils"] <= off["scanned_stencils"]
    assert on["point_tests"] <= off["point_tests"]
    assert on["point_tests"] > 0
    if scene == "grazing":
        assert on["scanned_stencils"] < off["scanned_stencils"]
        assert on["point_tests"] < off["point_tests"]


@pytest.mark.parametrize("scene", ["slope", "wall"])
def test_copy_unchanged(runs, scene):
    """pcp_debug_fine_copy returns the same bytes with the knob 1 and 0."""
    on, off = runs(scene)["1"], runs(scene)["0"]
    assert on["geo"] == off["geo"]
    assert on["frec"].tobytes() == off["frec"].tobytes()
    assert on["wpts"].tobytes() == off["wpts"].tobytes()
    assert on["pts"].tobytes() == off["pts"].tobytes()


def test_score_poses_equal(scenes):
    """Cell scoring's march reads the twin too: totals, covered counts, best pose and flags of a
    small case over the step and the slope are the same with the knob 1 and 0."""
    xyz = scenes["slope"][::7, :3].astype(np.float64)
    normals = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (xyz.shape[0], 1))
    params = _abi.default_vl_params()
    k = np.arange(12)
    poses = np.stack([1.5 + 1.9 * np.cos(0.55 * k), 1.25 + 1.7 * np.sin(0.55 * k),
                      np.full(12, 1.1), np.full(12, -0.4), 0.55 * k + np.pi], 1)
    zx = np.array([-1.0, 1.2, 1.5, -0.3, 0.0])
    res = {}
    for band in ("1", "0"):
        ctx = _context(scenes["slope"], band)
        try:
            ctx.set_cells(xyz, normals)
            ctx.raycast_fan(poses[:1], _abi.fan_params(n_az=8, n_el=4))   # builds the copy
            assert ctx.terrain_info()["scan_layout"] == "fine"
            fl = np.zeros(xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, zx, params, fl)
            res[band] = (tot, cov, rep.best_idx, fl)
        finally:
            ctx.close()
    assert (res["1"][1] > 0).any()
    assert res["1"][0].tobytes() == res["0"][0].tobytes()
    np.testing.assert_array_equal(res["1"][1], res["0"][1])
    assert res["1"][2] == res["0"][2]
    np.testing.assert_array_equal(res["1"][3], res["0"][3])
