"""The C++ host layer above the C ABI (pointcloud_processor_amd/csrc/host/pcp_nodes.*), driven
through pcp_nodes_cli, against the oracle and the golden fixtures: the node callbacks with the
reference's names produce the reference's outputs, headers, early returns and log tables."""
import math
import subprocess
from pathlib import Path

import numpy as np
import parity
import pytest

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "pointcloud_processor_amd" / "_lib" / "pcp_nodes_cli"
GOLD = ROOT / "tests" / "golden"

pytestmark = pytest.mark.gpu


def _run(*args, timeout=300, env=None):
    import os

    assert CLI.exists(), "build first (__graft_entry__.build())"
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True,
                       timeout=timeout, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, (r.returncode, r.stderr)
    import json

    return json.loads(r.stdout.strip().splitlines()[-1])


def _t(v):
    return ",".join(repr(float(x)) for x in v)


def test_filter_node(tmp_path, oracle):
    d = np.load(GOLD / "crop.npz")
    cloud = np.ascontiguousarray(d["cloud"])            # (N, 4) float32, point_step 16
    cloud.tofile(tmp_path / "in.f32")
    res = _run("filter", tmp_path / "in.f32", cloud.shape[0], 16, 0.2, 15.0, 10.0, 10.0,
               tmp_path / "out.f32")
    kept = oracle.crop_box(cloud, d["box"])
    ref, _, _, _ = oracle.voxel_grid(cloud[kept], 0.2)
    out = np.fromfile(tmp_path / "out.f32", np.float32).reshape(-1, 4)
    assert res["n_cropped"] == kept.size and res["n_out"] == ref.shape[0]
    np.testing.assert_array_equal(out[:, :3], ref)


def test_merger_node(tmp_path, oracle):
    d = np.load(GOLD / "voxel.npz")
    a = np.zeros((d["xyz_a"].shape[0], 4), np.float32)
    a[:, :3] = d["xyz_a"]
    b = np.zeros((d["xyz_b"].shape[0], 4), np.float32)
    b[:, :3] = d["xyz_b"]
    a.tofile(tmp_path / "r.f32")
    b.tofile(tmp_path / "z.f32")
    yaw = math.radians(30.0)
    tr = [8.0, -3.0, 0.0, 0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)]
    tz = [0.55, 0.4, 3.5, 0.0, math.sin(0.4363 / 2), 0.0, math.cos(0.4363 / 2)]
    res = _run("merge", tmp_path / "r.f32", a.shape[0], tmp_path / "z.f32", b.shape[0], _t(tr),
               _t(tz), tmp_path / "m.f32")
    ref = np.concatenate([oracle.transform_rgb(a, tr[:3], tr[3:], (255, 0, 0)),
                          oracle.transform_rgb(b, tz[:3], tz[3:], (0, 0, 255))])
    out = np.fromfile(tmp_path / "m.f32", np.float32).reshape(-1, 8)
    assert res["robot"] == a.shape[0] and res["backhoe"] == b.shape[0]
    np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))


@pytest.mark.parametrize("devices", [None, "0", "0,0,0"])
def test_virtual_lidar_node(tmp_path, devices):
    """SimplifiedDualLidarOptimizer on one device, and with its candidate loop sharded over a
    MultiDevice (pcp_multi: RCCL over device 0, or three ranks sharing device 0): the same
    totals, stale flags, best pose and log tables."""
    d = np.load(GOLD / "score.npz")
    np.ascontiguousarray(d["terrain"]).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(d["aux"]).tofile(tmp_path / "a.f32")
    np.ascontiguousarray(d["cells"], np.float64).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(d["normals"], np.float32).tofile(tmp_path / "n.f32")
    zx = d["zx"]
    base = [zx[0] - 0.4, zx[1] - 0.5, zx[2] - 3.5]      # getZX120Position adds the offsets
    res = _run("vlidar", tmp_path / "t.f32", d["terrain"].shape[0], tmp_path / "a.f32",
               d["aux"].shape[0], tmp_path / "c.f64", tmp_path / "n.f32", d["cells"].shape[0],
               _t(d["grid_bbox"]), _t(base), int(d["num_candidates"]), float(d["max_distance"]),
               tmp_path / "tot.f64", tmp_path / "flags.u8", tmp_path / "log.txt",
               env=None if devices is None else {"PCP_DEVICES": devices})
    if devices is not None:
        assert res["devices"] == len(devices.split(","))
        assert res["rccl"] == (1 if devices == "0" else 0)
    tot = np.fromfile(tmp_path / "tot.f64", np.float64)
    flags = np.fromfile(tmp_path / "flags.u8", np.uint8)
    parity.assert_totals(tot, d["total"])
    np.testing.assert_array_equal(flags, d["flags"])
    assert res["best_idx"] == int(d["report"][0])
    best = d["candidates"][res["best_idx"]]
    assert res["best"] == [float(best[0]), float(best[1]), float(best[2])]
    log = (tmp_path / "log.txt").read_text()
    rep = d["report"]
    assert f"  Total cells: {int(rep[1])}" in log
    assert f"  Green (Observable): {int(rep[2])} cells" in log
    assert f"Total Score: {float(d['best_score']):.2f}" in log


def test_streaming_replay(tmp_path, scene, cells):
    """BASELINE configs[4] on one GPU: per frame filter both 60k-pt scans, merge, and run the
    full pose search; reports end-to-end latency percentiles."""
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(cells.xyz).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals).tofile(tmp_path / "n.f32")
    res = _run("replay", tmp_path / "t.f32", scene.terrain.shape[0], tmp_path / "c.f64",
               tmp_path / "n.f32", cells.xyz.shape[0], _t(cells.grid_bbox), 20, 60032)
    assert res["frames"] == 20 and res["merged_points"] > 0 and res["best_idx"] >= 0
    assert 0 < res["p50_ms"] <= res["p99_ms"]


def test_excavation_area_node(tmp_path, oracle, small_scene):
    """virtual_lidar from its /excavation_area message: the node's excavationAreaCallback (GPU
    normals + cell grid) then one runOptimization tick, against the oracle pipeline run on its
    own (its own normals and cells).  Cells and cell normals bit-exact; the per-candidate totals
    match the oracle's reference loop within the totals' parity bar (tests/parity.py: glibc vs
    ocml acos / sin in the score) and the best index exactly."""
    area = np.ascontiguousarray(small_scene.area)
    terr = np.ascontiguousarray(small_scene.terrain)
    area.tofile(tmp_path / "a.f32")
    terr.tofile(tmp_path / "t.f32")
    res = _run("area", tmp_path / "a.f32", area.shape[0], tmp_path / "t.f32", terr.shape[0],
               "0,0,0", 36, 12.0, tmp_path / "tot.f64", tmp_path / "c.f64", tmp_path / "n.f32")
    xyz = np.fromfile(tmp_path / "c.f64", np.float64).reshape(-1, 3)
    cn = np.fromfile(tmp_path / "n.f32", np.float32).reshape(-1, 3)
    r_n = oracle.area_normals(area, 1.5)
    r_xyz, r_cn, bb, _ = oracle.excavation_grid(area, 0.1, 10, r_n)
    assert res["n_cells"] == r_xyz.shape[0]
    np.testing.assert_array_equal(xyz, r_xyz)
    np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))
    T = oracle.Cloud(terr)
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])   # getZX120Position offsets on (0, 0, 0)
    params = oracle.vl_params(num_candidates=36, max_distance=12.0)
    cand = oracle.generate_candidates(T, bb, params, zx)
    flags = np.zeros(xyz.shape[0], np.uint8)
    tot, _, rep = oracle.score_poses(T, None, r_xyz, r_cn, cand, zx, params, flags)
    got = np.fromfile(tmp_path / "tot.f64", np.float64)
    parity.assert_totals(got, tot)
    assert res["best_idx"] == rep.best_idx


@pytest.mark.parametrize("zc,area_async,front,carve,zx,defer", [
    ("1", "1", "1", "1", "0", "1"), ("0", "1", "1", "1", "0", "1"), ("1", "1", "1", "0", "0", "1"),
    ("1", "0", "0", "0", "0", "1"), ("1", "1", "1", "1", "1", "1"), ("1", "0", "1", "1", "0", "1"),
    ("1", "1", "1", "1", "0", "0")])
def test_streaming_replay_full_chain(tmp_path, oracle, scene, cells, zc, area_async, front, carve,
                                     zx, defer):
    """C5 with the launch file's whole chain per frame: filter x2 -> merge ->
    excavated_surface_generator (/excavated_terrain, /excavation_area) -> virtual_lidar
    (terrain index, normals + cell grid, pose search).  Frames 0, 1, 2 and the last one are
    re-run through the oracle chain ON ITS OWN from their raw scans -- every stage fed by the
    oracle's previous stage, never by a GPU dump: filtered clouds, merged cloud, carved terrain,
    excavation area, cells and cell normals bit-exact; candidate poses exact (angles: tests/parity.py);
    totals within the parity bar (tests/parity.py: glibc vs ocml acos in the score) and the best pose exact, with the frame's
    top-2 score gap printed.  Scratch reallocations settle after the first frames.  Both staging
    modes: message-sized data read / stored in place in pinned memory (PCP_ZC_IN=1, the
    default) and DMA'd both ways (0); the grid setup deferred to the tick (PCP_AREA_ASYNC=1, the
    composed chain's default: one wait for both) and settled in the area callback (0); the
    filter and merger nodes composed in one call (PCP_FRONT_FUSED=1, default) and as the three
    node callbacks (0); the carve node and virtual_lidar's area + terrain callbacks composed
    (PCP_CARVE_FUSED=1, default: pcp_excavate_area_async, the carve's landed records feeding the
    setup and the index in place) and as the three callbacks (0); with the carve composed, the
    zx120 cloud's callback made inside that call, the messages copied from the landing after its
    index is enqueued (PCP_CARVE_ZX=1; with the grid not deferred: the node's three callbacks,
    then the zx120 one) or after the call (0, default); the front's messages copied out of their
    landing after the composed carve read the merged cloud in place (PCP_FRONT_DEFER=1, default
    where every composition applies) or by the front call (0)."""
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(cells.xyz).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals).tofile(tmp_path / "n.f32")
    frames = 8
    res = _run("replay", tmp_path / "t.f32", scene.terrain.shape[0], tmp_path / "c.f64",
               tmp_path / "n.f32", cells.xyz.shape[0], _t(cells.grid_bbox), frames, 60032, 1,
               tmp_path, env={"PCP_ZC_IN": zc, "PCP_AREA_ASYNC": area_async,
                              "PCP_FRONT_FUSED": front, "PCP_CARVE_FUSED": carve,
                              "PCP_CARVE_ZX": zx, "PCP_FRONT_DEFER": defer})
    assert res["frames"] == frames and res["chain"] == 1
    assert res["cells"] > 0 and res["merged_points"] > 0 and res["best_idx"] >= 0
    assert 0 < res["p50_ms"] <= res["p99_ms"]
    assert len(res["lat_ms"]) == frames
    assert [d["frame"] for d in res["dumped"]] == [0, 1, 2, frames + 1]
    box = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])     # pointcloud_filter.cpp:30-36
    rt = ((8.0, -3.0, 2.0), (0.0, 0.0, 0.2588190451025208, 0.9659258262890683))
    zt = ((0.55, 0.4, 3.5), (0.0, 0.21633, 0.0, 0.97632))
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])   # getZX120Position on the origin

    def ld(name, dt, cols):
        return np.fromfile(tmp_path / name, dt).reshape(-1, cols)

    for d in res["dumped"]:
        pre = f"f{d['frame']}_"
        r_filtered = []
        for tag in ("rscan", "zscan"):
            scan = ld(pre + tag + ".f32", np.float32, 4)      # the raw scan (input, not a result)
            kept = oracle.crop_box(scan, box)
            vox, _, _, _ = oracle.voxel_grid(scan[kept], 0.2)
            got = ld(pre + tag[0] + "f.bin", np.float32, 4)
            np.testing.assert_array_equal(got[:, :3], vox)
            r_filtered.append(vox)
        ref = np.concatenate([oracle.transform_rgb(r_filtered[0], rt[0], rt[1], (255, 0, 0)),
                              oracle.transform_rgb(r_filtered[1], zt[0], zt[1], (0, 0, 255))])
        merged = ld(pre + "merged.bin", np.float32, 8)
        np.testing.assert_array_equal(merged[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
        keep, surf, area, _ = oracle.excavate(ref, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
        terr = ld(pre + "terrain.bin", np.float32, 8)
        nk = int(keep.sum())
        r_terr = np.concatenate([ref[keep][:, [0, 1, 2, 4]], surf])
        assert terr.shape[0] == r_terr.shape[0]
        np.testing.assert_array_equal(terr[:, [0, 1, 2, 4]].view(np.uint32), r_terr.view(np.uint32))
        assert nk <= terr.shape[0]
        got_area = ld(pre + "area.bin", np.float32, 8)
        np.testing.assert_array_equal(got_area[:, [0, 1, 2, 4]].view(np.uint32), area.view(np.uint32))
        r_xyz, r_cn, bb, _ = oracle.excavation_grid(area, 0.1, 10, oracle.area_normals(area, 1.5))
        cx, cn = ld(pre + "cells.f64", np.float64, 3), ld(pre + "cnrm.f32", np.float32, 3)
        np.testing.assert_array_equal(cx, r_xyz)
        np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))
        T = oracle.Cloud(r_terr)
        poses = ld(pre + "poses.f64", np.float64, 5)
        r_poses = oracle.generate_candidates(T, bb, oracle.vl_params(), zx)
        assert poses.shape == r_poses.shape
        np.testing.assert_array_equal(poses[:, :3], r_poses[:, :3])
        parity.assert_angles(poses[:, 3:], r_poses[:, 3:])
        aux = np.zeros((r_filtered[1].shape[0], 4), np.float32)
        aux[:, :3] = r_filtered[1]
        flags = np.zeros(r_xyz.shape[0], np.uint8)
        tot, _, rep = oracle.score_poses(T, oracle.Cloud(aux), r_xyz, r_cn, r_poses, zx,
                                         oracle.vl_params(), flags)
        parity.assert_totals(np.fromfile(tmp_path / (pre + "tot.f64"), np.float64), tot)
        assert d["best_idx"] == rep.best_idx
        if tot.size >= 2:
            top = np.sort(tot)[::-1]
            print(f"frame {d['frame']}: best {rep.best_idx} of {tot.size}, top-2 gap "
                  f"{(top[0] - top[1]) / abs(top[0]):.3e} (relative)")
    # scratch grows with 25 % headroom: a few reallocations while the sizes settle, not one
    # per frame (each frees a buffer: a device synchronization in the frame)
    assert res["reallocs_after_warmup"] <= 8, res["reallocs_after_warmup"]


def test_drivable_area_node(tmp_path, oracle):
    """DrivableAreaMapper::robotCloudCallback (calc_drivable_area.cpp:67-226): the skipped
    callbacks leave the start unset; the first published frame fixes the start-clear centre,
    which the second frame (robot moved) keeps. Grids and origins bit-exact vs the oracle."""
    rng = np.random.default_rng(4)
    n = 120_000
    c = np.zeros((n, 4), np.float32)
    c[:, 0] = rng.uniform(-40, 40, n)
    c[:, 1] = rng.uniform(-40, 40, n)
    c[:, 2] = rng.normal(-1.6, 0.04, n)
    wall = (c[:, 1] > 8) & (c[:, 1] < 12)
    c[wall, 2] += rng.uniform(0, 2.0, wall.sum())
    c.tofile(tmp_path / "in.f32")
    yaw = math.radians(-40.0)
    tf = [5.0, 1.0, 1.9, 0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)]
    r1, r2 = (5.0, 1.0), (12.25, -6.5)
    res = _run("drivable", tmp_path / "in.f32", n, 16, _t(tf), _t(r1), _t(r2), tmp_path / "g.i8")
    w, h = res["width"], res["height"]
    assert (w, h, res["resolution"]) == (100, 100, 1.0)
    got = np.fromfile(tmp_path / "g.i8", np.int8).reshape(2, h, w)
    for k, (r, key) in enumerate(((r1, "origin1"), (r2, "origin2"))):
        ref, origin = oracle.drivable_area(c, tf[:3], tf[3:], r, r1)
        np.testing.assert_array_equal(res[key], origin)
        np.testing.assert_array_equal(got[k], ref)


def _oracle_frame(tmp_path, pre, oracle):
    """The oracle chain ON ITS OWN from a dumped frame's raw scans (as
    test_streaming_replay_full_chain runs it): filter x2 -> merge -> carve -> normals + cells ->
    candidates -> runOptimization's totals.  -> (totals, best index, scoring inputs)."""
    box = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])
    rt = ((8.0, -3.0, 2.0), (0.0, 0.0, 0.2588190451025208, 0.9659258262890683))
    zt = ((0.55, 0.4, 3.5), (0.0, 0.21633, 0.0, 0.97632))
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])
    filt = []
    for tag in ("rscan", "zscan"):
        scan = np.fromfile(tmp_path / (pre + tag + ".f32"), np.float32).reshape(-1, 4)
        vox, _, _, _ = oracle.voxel_grid(scan[oracle.crop_box(scan, box)], 0.2)
        filt.append(vox)
    ref = np.concatenate([oracle.transform_rgb(filt[0], rt[0], rt[1], (255, 0, 0)),
                          oracle.transform_rgb(filt[1], zt[0], zt[1], (0, 0, 255))])
    keep, surf, area, _ = oracle.excavate(ref, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    terr = np.ascontiguousarray(np.concatenate([ref[keep][:, [0, 1, 2, 4]], surf]))
    T = oracle.Cloud(terr)
    r_xyz, r_cn, bb, _ = oracle.excavation_grid(area, 0.1, 10, oracle.area_normals(area, 1.5))
    r_poses = oracle.generate_candidates(T, bb, oracle.vl_params(), zx)
    aux = np.zeros((filt[1].shape[0], 4), np.float32)
    aux[:, :3] = filt[1]
    tot, _, rep = oracle.score_poses(T, oracle.Cloud(aux), r_xyz, r_cn, r_poses, zx,
                                     oracle.vl_params(), np.zeros(r_xyz.shape[0], np.uint8))
    return tot, rep.best_idx, dict(terrain=terr, aux=aux, xyz=r_xyz, cn=r_cn, poses=r_poses, zx=zx)


def test_parity_bar_catches_drift_on_c5_frames(tmp_path, oracle, scene, cells):
    """VERDICT r5 item 5 on the C5 chain's own frames: each dumped frame's totals pass
    tests/parity.py's EXACT totals bar against the oracle chain's; then the frame's scoring inputs
    (the oracle chain's terrain, zx120 cloud, cells, normals and candidates -- the chain test
    shows the device's are bit-identical) are scored per cell by the production build, the
    `make perturb` build (every cell one ulp up) and the `make perturb8` build (every 8th cell:
    partial drift), against the oracle's per-cell values: production passes the per-cell bar,
    both perturbed builds fail it.  The production build's totals are bit-identical to the
    oracle's here (the scoring rounds acos / sin as glibc does; with ocml's, 2-20 % of a frame's
    totals differed) and pass the exact totals bar (0 differing bit patterns); the every-cell
    and the every-8th-cell drifts fail that bar too, on every frame."""
    from test_gpu_parity import PERTURB8_LIB, PERTURB_LIB, _cell_census

    from pointcloud_processor_amd import _abi

    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(cells.xyz).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals).tofile(tmp_path / "n.f32")
    res = _run("replay", tmp_path / "t.f32", scene.terrain.shape[0], tmp_path / "c.f64",
               tmp_path / "n.f32", cells.xyz.shape[0], _t(cells.grid_bbox), 2, 60032, 1, tmp_path)
    assert res["dumped"]
    params = _abi.default_vl_params()
    for d in res["dumped"]:
        pre = f"f{d['frame']}_"
        tot, best, inp = _oracle_frame(tmp_path, pre, oracle)
        got = np.fromfile(tmp_path / (pre + "tot.f64"), np.float64)
        rep = parity.totals_report(got, tot)
        print("frame", d["frame"], "totals", rep)
        parity.assert_totals_exact(got, tot)   # the chain's own totals: 0 differing bit patterns
        assert d["best_idx"] == best
        r_sm, r_sz = oracle.score_matrix(oracle.Cloud(inp["terrain"]), oracle.Cloud(inp["aux"]),
                                         inp["xyz"], inp["cn"], inp["poses"], inp["zx"],
                                         oracle.vl_params())
        for tag, path in (("prod", None), ("perturbed", str(PERTURB_LIB)),
                          ("perturbed8", str(PERTURB8_LIB))):
            with _abi.Context(0, lib_path=path) as ctx:
                ctx.set_terrain(inp["terrain"], point_step=16)
                ctx.set_aux_cloud(inp["aux"], point_step=16)
                ctx.set_cells(inp["xyz"], inp["cn"])
                sm, sz = ctx.score_matrix(inp["poses"], inp["zx"], params)
                t_lib, _, r_lib = ctx.score_poses(inp["poses"], inp["zx"], params,
                                                  np.zeros(inp["xyz"].shape[0], np.uint8))
            cen = _cell_census(sm, sz, r_sm, r_sz)
            trep = parity.totals_report(t_lib, tot)
            print("frame", d["frame"], tag, cen, parity.cell_bar(cen), "totals", trep)
            assert cen["zero_mismatch"] == 0, (tag, cen)
            assert parity.cell_bar(cen) == (tag == "prod"), (tag, cen)
            # the exact totals bar: production passes it, the every-cell drift and the
            # every-8th-cell drift (5 of 91 totals on frame 0, which the max(2, 5 %) bar let
            # through) both fail it, on every frame
            assert parity.totals_exact(t_lib, tot) == (tag == "prod"), (tag, trep)
            assert r_lib.best_idx == best


def test_replay_frame_without_tf_republishes_merged_cloud(tmp_path, scene, cells):
    """when the map -> zx120/base_link lookup fails, excavated_surface_generator
    republishes the merged cloud as the terrain (matchedCloudCallback's fallback).  With the
    composed chain's deferred front (the merged message still a header while the carve reads its
    landing) the fallback must rebuild the message from the landing, not send the header: frame
    3 of the replay runs without TF and its terrain message carries every merged point's 32-byte
    record; the chain goes on to the next frames."""
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(cells.xyz).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals).tofile(tmp_path / "n.f32")
    res = _run("replay", tmp_path / "t.f32", scene.terrain.shape[0], tmp_path / "c.f64",
               tmp_path / "n.f32", cells.xyz.shape[0], _t(cells.grid_bbox), 5, 60032, 1,
               tmp_path, env={"PCP_REPLAY_NO_TF": "3"})
    nt = res["no_tf"]
    assert nt["frame"] == 3 and nt["merged_points"] > 0
    assert nt["terrain_points"] == nt["merged_points"]
    assert nt["terrain_bytes"] == 32 * nt["merged_points"]
    assert res["frames"] == 5 and res["best_idx"] >= 0


def test_replay_knobs_give_identical_frames(tmp_path, scene, cells):
    """the A/B-only knobs of the streaming chain change how, not what.  The replay's
    dumped frames (filtered clouds, merged cloud, carved terrain, excavation area, cells and
    their normals, candidates, totals) are byte-identical with the defaults and with the
    carve's records copied by a separate pass (PCP_CARVE_FUSE_COPY=0), the host bounding boxes
    by the scalar loop (PCP_HOST_BBOX_SCALAR=1) and the index scans as three launches
    (PCP_SCAN_ONEPASS=0)."""
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(cells.xyz).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals).tofile(tmp_path / "n.f32")
    runs = {}
    for tag, env in (("default", {}), ("fuse_copy0", {"PCP_CARVE_FUSE_COPY": "0"}),
                     ("bbox_scalar", {"PCP_HOST_BBOX_SCALAR": "1"}),
                     ("scan_3pass", {"PCP_SCAN_ONEPASS": "0"})):
        out = tmp_path / tag
        out.mkdir()
        res = _run("replay", tmp_path / "t.f32", scene.terrain.shape[0], tmp_path / "c.f64",
                   tmp_path / "n.f32", cells.xyz.shape[0], _t(cells.grid_bbox), 2, 60032, 1, out,
                   env=env)
        runs[tag] = (res, {f.name: f.read_bytes() for f in sorted(out.iterdir())})
    base_res, base = runs["default"]
    assert len(base) >= 20
    for tag, (res, files) in runs.items():
        assert sorted(files) == sorted(base), tag
        for name, data in base.items():
            assert files[name] == data, (tag, name)
        assert res["best_idx"] == base_res["best_idx"]
