"""pcp_raycast_fan_mounted / pcp_simulate_scan_mounted on the GPU: first hits, blocked counts, units
and every scan output bit for bit against the NumPy restatement of the definition
(tests/mount_ref.py), never against the device -- except the zero-tilt identity with the level
calls, the direction-table cache check and the CLI's comparison with the binding."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import mount_ref
import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"
SCAN_KEYS = ("offsets", "hit_point", "range", "first_hit", "point_mask", "seen_points")


def _check(ctx, poses6, fan, table, case):
    fh, blocked, units, ref = case
    b, u, f, best = ctx.raycast_fan_mounted(poses6, fan, table, want_first_hit=True)
    np.testing.assert_array_equal(f, fh)
    np.testing.assert_array_equal(b, blocked)
    np.testing.assert_array_equal(u, units)
    assert best == int(np.argmin(blocked))      # ties to the lowest index
    got = ctx.simulate_scan_mounted(poses6, fan, table, want_dense=True)
    np.testing.assert_array_equal(got["first_hit"], fh)
    scan_ref.assert_scan_equal(got, ref)
    assert got["n_returns"] == int(ref["offsets"][-1])
    return got


def _same_bytes(a, b):
    assert a["returns"].tobytes() == b["returns"].tobytes()
    for k in SCAN_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["n_seen_any"] == b["n_seen_any"] and a["n_returns"] == b["n_returns"]


@pytest.mark.parametrize("n_az,n_el,dmax", [(100, 37, 15.0), (64, 3, 110.0)])
def test_clutter_tilted(n_az, n_el, dmax):
    """The six clutter poses with roll / pitch pairs -- level, the zx120 Velodyne's -0.4363, a
    rolled mount, -1.5 (whole rings leave the clip box): P no multiple of 8, a partial last wave,
    an empty segment, at 110 m a step table past the LDS copy.  Two calls give the same bytes."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=n_az, n_el=n_el, max_distance=dmax)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("clutter", n_az, n_el, dmax), cloud, poses6, fan)
    assert int(case[1].sum()) > 0
    if dmax > 100.0:
        assert scan_ref.step_table(dmax - mount_ref.KVIS).size > 256
    else:
        assert (case[1] == 0).any()
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = _check(ctx, poses6, fan, None, case)
        again = ctx.simulate_scan_mounted(poses6, fan, None, want_dense=True)
        _same_bytes(again, got)
        r1 = ctx.raycast_fan_mounted(poses6, fan, None, want_first_hit=True)
        r2 = ctx.raycast_fan_mounted(poses6, fan, None, want_first_hit=True)
        assert [x.tobytes() for x in r1[:3]] == [x.tobytes() for x in r2[:3]] and r1[3] == r2[3]
    finally:
        ctx.close()


TABLE = [-0.4, 0.1, -0.05, 0.26, -1.2]


def test_non_monotone_beam_table():
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    assert int(case[1].sum()) > 0
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        _check(ctx, poses6, fan, TABLE, case)
    finally:
        ctx.close()


@pytest.mark.parametrize("n_az,n_el,dmax", [(100, 37, 15.0), (64, 3, 110.0)])
def test_zero_tilt_is_the_level_call(n_az, n_el, dmax):
    """roll = pitch = 0 and no table: the bytes of raycast_fan / simulate_scan on the same context,
    units included."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=n_az, n_el=n_el, max_distance=dmax)
    p5 = scan_ref.CLUTTER_POSES
    z = np.zeros(p5.shape[0])
    p6 = np.column_stack([p5[:, :3], z, z, p5[:, 4]])
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        lb, lu, lf, lbest = ctx.raycast_fan(p5, fan, want_first_hit=True)
        mb, mu, mf, mbest = ctx.raycast_fan_mounted(p6, fan, None, want_first_hit=True)
        assert (lb.tobytes(), lu.tobytes(), lf.tobytes(), lbest) == \
               (mb.tobytes(), mu.tobytes(), mf.tobytes(), mbest)
        assert int(lb.sum()) > 0
        _same_bytes(ctx.simulate_scan_mounted(p6, fan, None, want_dense=True),
                    ctx.simulate_scan(p5, fan, want_dense=True))
    finally:
        ctx.close()


def test_table_does_not_stay_in_the_direction_cache():
    """A level call, a mounted call with a table of the same shape, the level call again, then two
    different tables in turn: no call sees another's rings."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    p5 = scan_ref.CLUTTER_POSES
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    other = [0.05, -0.3, -0.8, 0.0, -0.1]
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        first = ctx.raycast_fan(p5, fan, want_first_hit=True)
        t1 = ctx.raycast_fan_mounted(poses6, fan, TABLE, want_first_hit=True)
        second = ctx.raycast_fan(p5, fan, want_first_hit=True)
        t2 = ctx.raycast_fan_mounted(poses6, fan, other, want_first_hit=True)
        t3 = ctx.raycast_fan_mounted(poses6, fan, TABLE, want_first_hit=True)
        m0 = ctx.raycast_fan_mounted(poses6, fan, None, want_first_hit=True)
    finally:
        ctx.close()
    assert [x.tobytes() for x in first[:3]] == [x.tobytes() for x in second[:3]]
    np.testing.assert_array_equal(t1[2], case[0])
    np.testing.assert_array_equal(t3[2], case[0])
    assert t2[2].tobytes() != t1[2].tobytes() and m0[2].tobytes() != t1[2].tobytes()


def _scene_poses6(P):
    """P tilted mounts 1.5 to 2.5 m above the 1M-point scene's lattice (x -20 .. 30, y -25 .. 25),
    pitched down between 0.1 and 0.6 rad, rolled a little, every yaw."""
    rng = np.random.default_rng(29)
    return np.ascontiguousarray(np.column_stack([
        rng.uniform(-12.0, 22.0, P), rng.uniform(-17.0, 17.0, P), rng.uniform(1.5, 2.5, P),
        rng.uniform(-0.15, 0.15, P), rng.uniform(-0.6, -0.1, P), rng.uniform(-3.1, 3.1, P)]))


@pytest.mark.parametrize("layout", ["cells", "blocks", "fine"])
@pytest.mark.parametrize("npw", ["1", "2", "8"])
@pytest.mark.parametrize("P", [8, 16])
def test_scene_production_paths(scene, P, npw, layout, monkeypatch):
    """8 and 16 tilted mounts on the 1M-point scene, a 64 x 8 fan: the XCD-chunk kernels with 1, 2
    and 8 poses per wave over the fine copy, the interleaved ones over the coarse layouts."""
    monkeypatch.setenv("PCP_FAN_NPW", npw)
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "0" if layout == "cells" else "2")
    if layout == "blocks":
        monkeypatch.setenv("PCP_TERRAIN_FINE", "0")
    fan = _abi.fan_params(n_az=64, n_el=8)
    poses6 = _scene_poses6(P)
    case = mount_ref.mount_case(("scene", P), scene.terrain, poses6, fan)
    assert (case[1] > 0).all()
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.raycast_fan_mounted(poses6, fan)     # (the second query builds the fine copy)
        got = _check(ctx, poses6, fan, None, case)
        assert ctx.terrain_info()["scan_layout"] == layout
    finally:
        ctx.close()
    assert got["n_returns"] > 0


def test_scene_eight_poses_per_wave(scene, monkeypatch):
    """64 mounts (the scan's bound; bit 63 of the mask) and a 64 x 2 fan: the only pose count of a
    scan whose XCD chunk of 8 poses is marched by one wave (fan_npw(64, 8) = 8), so each wave's
    eight 12-double pose rows come from its LDS copy."""
    monkeypatch.setenv("PCP_FAN_NPW", "8")
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "2")
    fan = _abi.fan_params(n_az=64, n_el=2, el_min_deg=-60.0, el_max_deg=10.0)
    poses6 = _scene_poses6(64)
    case = mount_ref.mount_case(("scene", 64), scene.terrain, poses6, fan)
    assert (case[1] > 0).all()
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.raycast_fan_mounted(poses6, fan)     # (the second query builds the fine copy)
        got = _check(ctx, poses6, fan, None, case)
        assert ctx.terrain_info()["scan_layout"] == "fine"
    finally:
        ctx.close()
    assert (got["point_mask"] >> np.uint64(63)).any()


def test_refusals_leave_the_outputs_alone():
    """65 poses to the scan and a NaN table entry: PCP_E_INVALID, the sentinel bytes stay, and a
    valid call afterwards succeeds."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    p65 = np.ascontiguousarray(np.resize(poses6, (65, 6)))
    bad = np.array(TABLE)
    bad[3] = np.nan
    good = np.ascontiguousarray(TABLE, np.float64)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        for poses, n, tab in ((p65, 65, good), (poses6, 6, bad)):
            ret = np.full(16, 0xAB, np.uint8).repeat(24).view(_abi.SCAN_RETURN_DTYPE)
            off = np.full(66, 77, np.uint64)
            mask = np.full(cloud.shape[0], 5, np.uint64)
            seen = np.full(65, 9, np.uint32)
            fh = np.full(65 * 500, -9, np.int16)
            nret, npts, nany = C.c_uint64(123), C.c_uint64(456), C.c_uint64(789)
            keep = [a.tobytes() for a in (ret, off, mask, seen, fh)]
            rc = ctx.lib.pcp_simulate_scan_mounted(
                ctx.h, _abi._ptr(poses), n, C.byref(fan), _abi._ptr(tab), _abi._ptr(ret), 16,
                C.byref(nret), _abi._ptr(off), None, None, _abi._ptr(fh), _abi._ptr(mask),
                mask.size, C.byref(npts), _abi._ptr(seen), C.byref(nany))
            assert rc == _abi.PCP_E_INVALID
            assert [a.tobytes() for a in (ret, off, mask, seen, fh)] == keep
            assert (nret.value, npts.value, nany.value) == (123, 456, 789)
        blocked = np.full(6, 0xCDCDCDCD, np.uint32)
        units = np.full(6, 31, np.uint64)
        fh = np.full(6 * 500, -9, np.int16)
        best = C.c_int64(55)
        rc = ctx.lib.pcp_raycast_fan_mounted(ctx.h, _abi._ptr(poses6), 6, C.byref(fan),
                                             _abi._ptr(bad), _abi._ptr(blocked), _abi._ptr(units),
                                             _abi._ptr(fh), C.byref(best))
        assert rc == _abi.PCP_E_INVALID
        assert (blocked == 0xCDCDCDCD).all() and (units == 31).all() and (fh == -9).all()
        assert best.value == 55
        for tab in (bad, np.array([0.0, 0.1, np.inf, 0.2, 0.3])):
            with pytest.raises(_abi.PcpError) as ei:
                ctx.simulate_scan_mounted(poses6, fan, tab)
            assert ei.value.code == _abi.PCP_E_INVALID
        with pytest.raises(_abi.PcpError) as ei:
            ctx.simulate_scan_mounted(p65, fan, TABLE)
        assert ei.value.code == _abi.PCP_E_INVALID
        _check(ctx, poses6, fan, TABLE, case)
    finally:
        ctx.close()


def test_cli_scan_mounted_is_the_bindings_records(tmp_path: Path):
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        want = {t: ctx.simulate_scan_mounted(poses6, fan, tab)
                for t, tab in (("table", TABLE), ("-", None))}
    finally:
        ctx.close()
    rec = np.zeros((cloud.shape[0], 8), np.float32)
    rec[:, :3] = cloud[:, :3]
    rec[:, 4] = np.arange(cloud.shape[0], dtype=np.float32)
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    out = [tmp_path / n for n in ("scans.bin", "offsets.u64", "blind.f32", "mask.u64")]
    for t, ref in want.items():
        arg = ",".join(repr(float(v)) for v in TABLE) if t == "table" else "-"
        r = subprocess.run([str(CLI), "scan_mounted", str(tmp_path / "terrain.f32"),
                            str(cloud.shape[0]), ",".join(repr(float(v)) for v in poses6.ravel()),
                            "100", "5", "15.0", arg] + [str(o) for o in out],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        info = json.loads(r.stdout.strip().splitlines()[-1])
        assert np.fromfile(out[0], _abi.SCAN_RETURN_DTYPE).tobytes() == ref["returns"].tobytes()
        np.testing.assert_array_equal(np.fromfile(out[1], np.uint64), ref["offsets"])
        np.testing.assert_array_equal(np.fromfile(out[3], np.uint64), ref["point_mask"])
        blind = np.fromfile(out[2], np.float32).reshape(-1, 8)
        assert blind.tobytes() == rec[ref["point_mask"] == 0].tobytes()
        assert info["n_sensors"] == 6 and info["n_returns"] == ref["n_returns"] > 0
        assert info["n_seen_any"] == ref["n_seen_any"]
    assert want["table"]["returns"].tobytes() != want["-"]["returns"].tobytes()
    # six numbers per sensor, and a table of NEL entries
    base = [str(CLI), "scan_mounted", str(tmp_path / "terrain.f32"), str(cloud.shape[0])]
    tail = ["100", "5", "15.0"]
    outs = [str(o) for o in out]
    assert subprocess.run(base + ["1,2,3,0,0"] + tail + ["-"] + outs,
                          capture_output=True).returncode == 2
    assert subprocess.run(base + ["1,2,3,0,0,0"] + tail + ["0.1,0.2"] + outs,
                          capture_output=True).returncode == 2
