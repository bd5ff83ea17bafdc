"""pcp_simulate_scan on the GPU: every output -- records, offsets, dense images, masks, counts --
bit for bit against the NumPy restatement of the definition (tests/scan_ref.py) on the ORACLE's
first hits, over every production path of the fan that feeds the resolve."""
import ctypes as C

import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu


def _check_all(ctx, oracle, cloud, poses, fan, fh, ref):
    got = ctx.simulate_scan(poses, fan, want_dense=True)
    np.testing.assert_array_equal(got["first_hit"], fh)
    scan_ref.assert_scan_equal(got, ref)
    assert got["n_returns"] == int(ref["offsets"][-1])
    return got


@pytest.mark.parametrize("n_az,n_el,dmax", [(100, 37, 15.0), (64, 3, 110.0)])
def test_clutter_and_duplicates(oracle, n_az, n_el, dmax):
    """The volumetric cloud with duplicated rows and the six poses: rings spanning waves, a
    partial last wave, P no multiple of 8, an empty segment (15 m) and ties; at 110 m a step table
    outside the fan kernels' LDS copy."""
    cloud, poses, fan, fh, blocked, ref = scan_ref.clutter_case(oracle, n_az, n_el, dmax)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = _check_all(ctx, oracle, cloud, poses, fan, fh, ref)
        d_blocked, _, _, _ = ctx.raycast_fan(poses, fan)
        np.testing.assert_array_equal(np.diff(got["offsets"].astype(np.int64)),
                                      d_blocked.astype(np.int64))
        np.testing.assert_array_equal(d_blocked, blocked)
        assert ref["ties"] >= 1
        # two identical calls give identical bytes
        again = ctx.simulate_scan(poses, fan, want_dense=True)
        assert again["returns"].tobytes() == got["returns"].tobytes()
        for k in ("offsets", "hit_point", "range", "first_hit", "point_mask", "seen_points"):
            assert again[k].tobytes() == got[k].tobytes(), k
        assert again["n_seen_any"] == got["n_seen_any"]
    finally:
        ctx.close()


def _scene_case(oracle, scene, cells, P):
    def build():
        g = _abi.Context(0)
        try:
            g.set_terrain(scene.terrain, point_step=32)
            p = _abi.default_vl_params(num_candidates=100)
            poses = g.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)
        finally:
            g.close()
        poses = np.ascontiguousarray(np.resize(poses, (P, 5)))
        fan = _abi.fan_params(n_az=256, n_el=32)
        oracle.set_threads(8)
        _, _, fh = oracle.raycast_fan(oracle.Cloud(scene.terrain), poses, 256, 32, fan.el_min,
                                      fan.el_max, fan.max_distance)
        oracle.set_threads(1)
        return poses, fan, fh, scan_ref.resolve(oracle, scene.terrain, poses, fan, fh)

    return scan_ref.cached(("scene", P), build)


@pytest.mark.parametrize("layout", ["cells", "blocks", "fine"])
@pytest.mark.parametrize("npw,tile,skip", [("1", "2", "1"), ("2", "2", "1"), ("8", "2", "1"),
                                           ("8", "1", "1"), ("8", "2", "2")])
@pytest.mark.parametrize("P", [8, 16])
def test_synthetic_scene_every_fan_path(oracle, scene, cells, P, npw, tile, skip, layout,
                                        monkeypatch):
    """8 and 16 poses on the 1M-point scene (the XCD-chunk kernels on the fine copy), the knobs of
    test_raycast_fan_poses_per_wave (poses per wave, fine tile, skip thresholds) and the three
    index layouts: whichever fan path wrote the first hits, the resolve walks the cell-major copy
    and gives the restatement's outputs."""
    monkeypatch.setenv("PCP_FAN_NPW", npw)
    monkeypatch.setenv("PCP_FINE_SKIP", skip)
    monkeypatch.setenv("PCP_FINE_TILE", tile)
    monkeypatch.setenv("PCP_FINE_PACK", "1")
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "0" if layout == "cells" else "2")
    if layout == "blocks":
        monkeypatch.setenv("PCP_TERRAIN_FINE", "0")
    poses, fan, fh, ref = _scene_case(oracle, scene, cells, P)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        got = ctx.simulate_scan(poses, fan, want_dense=True)
        info = ctx.terrain_info()
        assert info["scan_layout"] == layout
        if layout == "fine":
            assert info["fine_tile"] == int(tile)
    finally:
        ctx.close()
    np.testing.assert_array_equal(got["first_hit"], fh)
    scan_ref.assert_scan_equal(got, ref)
    assert int(ref["offsets"][-1]) > 0


def test_sixty_four_poses_and_sixty_five(oracle):
    """64 poses use bit 63 of the mask; 65 are refused before anything is launched, the outputs
    stay untouched and a following valid call succeeds."""
    cloud = scan_ref.clutter_cloud()
    rng = np.random.default_rng(5)
    poses = np.column_stack([rng.uniform(-3, 3, 65), rng.uniform(-3, 3, 65),
                             rng.uniform(0.0, 1.5, 65), np.zeros(65), rng.uniform(-3, 3, 65)])
    fan = _abi.fan_params(n_az=64, n_el=4)
    _, _, fh = oracle.raycast_fan(oracle.Cloud(cloud), poses[:64], 64, 4, fan.el_min, fan.el_max,
                                  fan.max_distance)
    ref = scan_ref.resolve(oracle, cloud, poses[:64], fan, fh)
    assert (ref["point_mask"] >> np.uint64(63)).any() and ref["seen_points"][63] > 0
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        # 65 poses: nothing written
        ret = np.full(16, 0xAB, np.uint8).repeat(24).view(_abi.SCAN_RETURN_DTYPE)
        off = np.full(66, 77, np.uint64)
        mask = np.full(cloud.shape[0], 5, np.uint64)
        seen = np.full(65, 9, np.uint32)
        nret, npts, nany = C.c_uint64(123), C.c_uint64(456), C.c_uint64(789)
        keep = [ret.tobytes(), off.tobytes(), mask.tobytes(), seen.tobytes()]
        p65 = np.ascontiguousarray(poses)
        rc = ctx.lib.pcp_simulate_scan(ctx.h, _abi._ptr(p65), 65, C.byref(fan), _abi._ptr(ret), 16,
                                       C.byref(nret), _abi._ptr(off), None, None, None,
                                       _abi._ptr(mask), mask.size, C.byref(npts), _abi._ptr(seen),
                                       C.byref(nany))
        assert rc == _abi.PCP_E_INVALID
        assert [ret.tobytes(), off.tobytes(), mask.tobytes(), seen.tobytes()] == keep
        assert (nret.value, npts.value, nany.value) == (123, 456, 789)
        with pytest.raises(_abi.PcpError) as ei:
            ctx.simulate_scan(poses, fan)
        assert ei.value.code == _abi.PCP_E_INVALID
        # a bad fan and a step table past PCP_MAX_STEPS are refused the same way
        for bad in (_abi.fan_params(n_az=0, n_el=4),
                    _abi.fan_params(n_az=64, n_el=4, max_distance=0.5 + 0.3 * 5000)):
            with pytest.raises(_abi.PcpError) as ei:
                ctx.simulate_scan(poses[:2], bad)
            assert ei.value.code == _abi.PCP_E_INVALID
        got = ctx.simulate_scan(poses[:64], fan, want_dense=True)
    finally:
        ctx.close()
    np.testing.assert_array_equal(got["first_hit"], fh)
    scan_ref.assert_scan_equal(got, ref)


def test_non_finite_rows(oracle):
    """Non-finite rows at the front of the cloud and in the middle: `point` and hit_point are
    input indices, the masks of those rows are zero, n_points counts them."""
    cloud = scan_ref.clutter_cloud().copy()
    cloud[:5, 0] = np.nan
    cloud[70_000:70_010, 2] = np.inf
    cloud[70_010, 1] = -np.inf
    fan = _abi.fan_params(n_az=100, n_el=9)
    poses = scan_ref.CLUTTER_POSES
    _, _, fh = oracle.raycast_fan(oracle.Cloud(cloud), poses, 100, 9, fan.el_min, fan.el_max,
                                  fan.max_distance)
    ref = scan_ref.resolve(oracle, cloud, poses, fan, fh)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = _check_all(ctx, oracle, cloud, poses, fan, fh, ref)
    finally:
        ctx.close()
    bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
    assert bad.sum() == 16 and got["n_points"] == cloud.shape[0]
    assert not got["point_mask"][bad].any()
    pts = got["returns"]["point"]
    assert pts.size and not bad[pts].any() and (pts > 70_010).any() and (pts < 70_000).any()
    # the records carry the input rows' own bits
    np.testing.assert_array_equal(got["returns"]["x"].view(np.uint32),
                                  cloud[pts, 0].view(np.uint32))
    np.testing.assert_array_equal(got["returns"]["z"].view(np.uint32),
                                  cloud[pts, 2].view(np.uint32))


def test_short_capacities(oracle):
    """returns_cap = total - 1 and mask_cap = N - 1: PCP_E_CAPACITY with the counts, offsets and
    dense outputs right, and the row after returns_cap untouched."""
    cloud, poses, fan, fh, blocked, ref = scan_ref.clutter_case(oracle, 100, 37, 15.0)
    total, N, P = int(ref["offsets"][-1]), cloud.shape[0], poses.shape[0]
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        p = np.ascontiguousarray(poses, np.float64)
        for rcap, mcap in ((total - 1, N), (total, N - 1), (total - 1, N - 1), (0, N)):
            ret = np.full((total + 1) * 24, 0xCD, np.uint8).view(_abi.SCAN_RETURN_DTYPE)
            guard = ret[rcap:].tobytes()
            off = np.zeros(P + 1, np.uint64)
            hp = np.zeros((P, fan.n_el, fan.n_az), np.int32)
            rg = np.zeros(hp.shape, np.float32)
            mask = np.full(N, 3, np.uint64)
            seen = np.zeros(P, np.uint32)
            nret, npts, nany = C.c_uint64(), C.c_uint64(), C.c_uint64()
            rc = ctx.lib.pcp_simulate_scan(ctx.h, _abi._ptr(p), P, C.byref(fan), _abi._ptr(ret),
                                           rcap, C.byref(nret), _abi._ptr(off), _abi._ptr(hp),
                                           _abi._ptr(rg), None, _abi._ptr(mask), mcap,
                                           C.byref(npts), _abi._ptr(seen), C.byref(nany))
            assert rc == _abi.PCP_E_CAPACITY, (rcap, mcap)
            assert nret.value == total and npts.value == N
            np.testing.assert_array_equal(off, ref["offsets"])
            np.testing.assert_array_equal(hp, ref["hit_point"])
            np.testing.assert_array_equal(rg.view(np.uint32), ref["range"].view(np.uint32))
            np.testing.assert_array_equal(seen, ref["seen_points"])
            assert nany.value == ref["n_seen_any"]
            assert ret[rcap:].tobytes() == guard
            # what was written in front of the capacity is the first records
            assert ret[:rcap].tobytes() == ref["returns"][:rcap].tobytes()
            if mcap >= N:
                np.testing.assert_array_equal(mask, ref["point_mask"])
            else:
                assert (mask[mcap:] == 3).all()
        # the Python call reports the same through PcpError.partial
        with pytest.raises(_abi.PcpError) as ei:
            ctx.simulate_scan(poses, fan, returns_cap=total - 1)
        assert ei.value.code == _abi.PCP_E_CAPACITY
        assert ei.value.partial["n_returns"] == total
        got = ctx.simulate_scan(poses, fan, want_dense=True, returns_cap=total)
        scan_ref.assert_scan_equal(got, ref)
    finally:
        ctx.close()


def test_no_poses_no_terrain_and_stale_index(oracle):
    """n == 0; no terrain index (every ray misses, N = 0); pcp_set_terrain with an empty cloud
    after a real one keeps the index, so the indices refer to the old cloud."""
    cloud, poses, fan, fh, blocked, ref = scan_ref.clutter_case(oracle, 100, 37, 15.0)
    ctx = _abi.Context(0)
    try:
        got = ctx.simulate_scan(poses, fan, want_dense=True)      # no terrain
        assert got["n_points"] == 0 and got["n_returns"] == 0 and got["returns"].size == 0
        assert not got["offsets"].any() and got["point_mask"].size == 0
        assert (got["hit_point"] == -1).all() and (got["range"] == -1.0).all()
        assert (got["first_hit"] == -1).all()
        assert not got["seen_points"].any() and got["n_seen_any"] == 0
        got = ctx.simulate_scan(np.zeros((0, 5)), fan)            # no terrain, no poses
        assert got["n_points"] == 0 and got["n_returns"] == 0 and got["offsets"].tolist() == [0]
        ctx.set_terrain(cloud)
        got = ctx.simulate_scan(np.zeros((0, 5)), fan)            # n == 0
        assert got["n_returns"] == 0 and got["offsets"].tolist() == [0]
        assert got["n_points"] == cloud.shape[0] and got["point_mask"].size == cloud.shape[0]
        assert not got["point_mask"].any() and got["n_seen_any"] == 0
        with pytest.raises(_abi.PcpError) as ei:                  # n == 0 still checks the fan
            ctx.simulate_scan(np.zeros((0, 5)), _abi.fan_params(n_az=-1, n_el=4))
        assert ei.value.code == _abi.PCP_E_INVALID
        ctx.set_terrain(np.zeros((0, 4), np.float32))             # keeps the stale index
        _check_all(ctx, oracle, cloud, poses, fan, fh, ref)
    finally:
        ctx.close()


def test_other_queries_are_not_disturbed(oracle, scene, cells, aux):
    """A raycast_fan and a score_poses after simulate_scan give what they gave before it (the
    scan's buffers are its own) -- and the scan between them is still right."""
    poses, fan, fh, ref = _scene_case(oracle, scene, cells, 8)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        p = _abi.default_vl_params(num_candidates=100)
        ctx.raycast_fan(poses, fan)     # (the second query builds the fine copy: settle first)
        ctx.raycast_fan(poses, fan)

        def others():
            b, u, f, best = ctx.raycast_fan(poses, fan, want_first_hit=True)
            flags = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, p, flags)
            return [b.tobytes(), u.tobytes(), f.tobytes(), best, tot.tobytes(), cov.tobytes(),
                    flags.tobytes(), rep.best_idx, rep.green]

        before = others()
        got = ctx.simulate_scan(poses, fan, want_dense=True)
        after = others()
        again = ctx.simulate_scan(poses, fan, want_dense=True)
    finally:
        ctx.close()
    assert before == after
    scan_ref.assert_scan_equal(got, ref)
    scan_ref.assert_scan_equal(again, ref)
