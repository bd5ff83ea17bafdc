"""pcp_place_coverage on the GPU: every output -- selection, gains, covered counts, the rounds'
gain rows, per-pose counts, owners -- equal to the NumPy restatement of the definition
(tests/cover_ref.py) on the ORACLE's first hits and scan_ref's resolve; all of it integers, so
equal means equal."""
import ctypes as C

import cover_ref
import mount_ref
import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu


def _call(ctx, inst, i, **kw):
    roi, sep, fixed, k = cover_ref.GRID[i]
    return ctx.place_coverage(inst["poses"], inst["fan"], k, sep, fixed, inst["rois"][roi],
                              want_round_gains=True, want_owner=True, **kw)


@pytest.fixture(scope="module")
def clutter_ctx():
    ctx = _abi.Context(0)
    ctx.set_terrain(scan_ref.clutter_cloud())
    yield ctx
    ctx.close()


@pytest.mark.parametrize("i", range(len(cover_ref.GRID)))
def test_grid_equals_the_restatement(oracle, clutter_ctx, i):
    """71 poses (past the scan mask's 64), N % 64 = 44, two word chunks and nine pose groups per
    round; ties at the maximum, an exact-equality separation, three regions, fixed sensors."""
    inst = cover_ref.instance(oracle)
    ref = cover_ref.grid_case(oracle, i)
    got = _call(clutter_ctx, inst, i)
    print(cover_ref.GRID[i], "selected", got["selected"].tolist(), "gain", got["gain"].tolist())
    cover_ref.assert_cover_equal(got, ref)
    roi = inst["rois"][cover_ref.GRID[i][0]]
    if roi is not None:   # nothing outside the region is owned
        assert (got["point_owner"][roi == 0] == _abi.OWNER_NONE).all()
    blind = (got["point_owner"] == _abi.OWNER_NONE) & (True if roi is None else roi != 0)
    assert int(blind.sum()) == got["roi_points"] - (
        int(got["covered_after"][-1]) if got["n_selected"] else got["base_covered"])


def test_fixed_owners_follow_the_list_order(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    a = clutter_ctx.place_coverage(inst["poses"], inst["fan"], 2, fixed=(10, 40), want_owner=True)
    b = clutter_ctx.place_coverage(inst["poses"], inst["fan"], 2, fixed=(40, 10), want_owner=True)
    both = np.intersect1d(inst["seen"][10], inst["seen"][40])
    assert both.size > 0
    assert (a["point_owner"][both] == 0).all() and (b["point_owner"][both] == 0).all()
    only40 = np.setdiff1d(inst["seen"][40], inst["seen"][10])
    assert (a["point_owner"][only40] == 1).all() and (b["point_owner"][only40] == 0).all()
    assert a["base_covered"] == b["base_covered"] == np.union1d(inst["seen"][10],
                                                                 inst["seen"][40]).size
    for got, fixed in ((a, (10, 40)), (b, (40, 10))):
        ref = cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], 2, 0.0, fixed)
        cover_ref.assert_cover_equal(got, ref)


def test_stops_on_zero_gain_and_on_nothing_seen(oracle, clutter_ctx):
    """ROI = the reference's seen(0) with the poses (0, far, copy of 0): one round, then the copy
    and the far pose are alive and add nothing.  The far pose alone: no round at all."""
    inst = cover_ref.instance(oracle)
    rows = [0, 4, 0]
    poses = inst["poses"][rows]
    seen = [inst["seen"][r] for r in rows]
    roi = np.zeros(inst["N"], np.uint8)
    roi[inst["seen"][0]] = 1
    got = clutter_ctx.place_coverage(poses, inst["fan"], 4, roi=roi, want_round_gains=True,
                                     want_owner=True)
    ref = cover_ref.greedy(seen, poses[:, :2], inst["N"], 4, roi=roi)
    assert ref["n_selected"] == 1 and ref["stopped"] == "gain" and ref["selected"].tolist() == [0]
    cover_ref.assert_cover_equal(got, ref)
    assert got["covered_after"].tolist() == [got["roi_points"]] == [inst["seen"][0].size]
    far = clutter_ctx.place_coverage(inst["poses"][4:5], inst["fan"], 3, want_round_gains=True,
                                     want_owner=True)
    assert far["n_selected"] == 0 and far["seen_points"].tolist() == [0]
    assert far["roi_points"] == inst["N"] and far["base_covered"] == 0
    assert (far["point_owner"] == _abi.OWNER_NONE).all()


def _ring_cloud(n_pts, nan_rows=0):
    """n_pts points on the circle of radius 0.8 m (the step table's second sample) under the
    azimuths of a 100-ray ring, then nan_rows non-finite rows in the middle."""
    a = 2.0 * np.pi * np.arange(n_pts) / 100.0
    c = np.column_stack([0.8 * np.cos(a), 0.8 * np.sin(a), 0.001 * (np.arange(n_pts) % 3),
                         np.zeros(n_pts)]).astype(np.float32)
    if nan_rows:
        bad = np.full((nan_rows, 4), np.nan, np.float32)
        bad[1::2, 0] = np.inf
        c = np.concatenate([c[:n_pts // 2], bad, c[n_pts // 2:]])
    return np.ascontiguousarray(c)


SMALL_POSES = np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [0.05, 0.02, 0.01, 0.0, 1.0],
                        [40.0, 40.0, 0.0, 0.0, 0.0], [-0.03, 0.0, 0.0, 0.0, -2.0]])


@pytest.mark.parametrize("n_pts,nan_rows", [(10, 0), (64, 0), (64, 6)])
def test_one_word_clouds_and_non_finite_rows(oracle, n_pts, nan_rows):
    """10 points (one partial word), 64 points (N % 64 == 0, the padding word beside it) and 70
    rows of which 6 are non-finite: those count in roi_points and are never owned."""
    cloud = _ring_cloud(n_pts, nan_rows)
    N = cloud.shape[0]
    fan = _abi.fan_params(n_az=100, n_el=5, el_min_deg=-10.0, el_max_deg=10.0)
    seen = cover_ref.level_seen(oracle, cloud, SMALL_POSES, fan)
    assert seen[0].size >= min(n_pts, 8) and seen[2].size == 0
    ref = cover_ref.greedy(seen, SMALL_POSES[:, :2], N, 4)
    assert ref["n_selected"] >= 1
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = ctx.place_coverage(SMALL_POSES, fan, 4, want_round_gains=True, want_owner=True)
        roi = np.ones(N, np.uint8)
        with_roi = ctx.place_coverage(SMALL_POSES, fan, 4, roi=roi, want_round_gains=True,
                                      want_owner=True)
    finally:
        ctx.close()
    for g in (got, with_roi):
        cover_ref.assert_cover_equal(g, ref)
        assert g["roi_points"] == N and g["n_points"] == N
    if nan_rows:
        bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
        assert bad.sum() == nan_rows and (got["point_owner"][bad] == _abi.OWNER_NONE).all()


def test_three_calls_give_identical_bytes(oracle):
    """A fresh context: the index's copies are built at the second query, so the resolve runs
    behind different march layouts; the answer and its bytes stay."""
    inst = cover_ref.instance(oracle)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(inst["cloud"])
        runs = [_call(ctx, inst, 3) for _ in range(3)]
        scan = ctx.simulate_scan(inst["poses"][:64], inst["fan"])
    finally:
        ctx.close()
    cover_ref.assert_cover_equal(runs[0], cover_ref.grid_case(oracle, 3))
    for r in runs[1:]:
        for k in ("selected", "gain", "covered_after", "round_gains", "seen_points", "point_owner"):
            assert r[k].tobytes() == runs[0][k].tobytes(), k
        for k in ("n_selected", "n_points", "roi_points", "base_covered"):
            assert r[k] == runs[0][k], k
    # the per-pose counts are the scan's
    np.testing.assert_array_equal(runs[0]["seen_points"][:64], scan["seen_points"])


TABLE = [-0.4, 0.1, -0.05, 0.26, -1.2]


def test_mounted_with_a_beam_table(clutter_ctx):
    """The six tilted clutter mounts with a non-uniform beam table, against the restatement on
    mount_ref's own march and resolve."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    seen = cover_ref.seen_sets(case[3], 6)
    assert sum(s.size > 0 for s in seen) >= 3
    for sep, fixed in ((0.0, ()), (3.0, (1,))):
        ref = cover_ref.greedy(seen, poses6[:, :2], cloud.shape[0], 6, sep, fixed)
        assert ref["n_selected"] >= 2
        got = clutter_ctx.place_coverage_mounted(poses6, fan, TABLE, 6, sep, fixed,
                                                 want_round_gains=True, want_owner=True)
        cover_ref.assert_cover_equal(got, ref)
    # the level twin on the same context afterwards: the direction cache holds no stale table
    lvl = clutter_ctx.place_coverage(scan_ref.CLUTTER_POSES, fan, 2)
    scan = clutter_ctx.simulate_scan(scan_ref.CLUTTER_POSES, fan)
    np.testing.assert_array_equal(lvl["seen_points"], scan["seen_points"])


def test_other_queries_are_not_disturbed(scene, cells, aux):
    """raycast_fan, simulate_scan and score_poses after the placement give the bytes they gave
    before it: the call's scratch is its own."""
    rng = np.random.default_rng(11)
    poses = np.column_stack([rng.uniform(0, 10, 8), rng.uniform(-4, 4, 8), rng.uniform(0.8, 2.0, 8),
                             np.zeros(8), rng.uniform(-3, 3, 8)])
    fan = _abi.fan_params(n_az=256, n_el=32)
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
            s = ctx.simulate_scan(poses, fan, want_dense=True)
            flags = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, p, flags)
            return [b.tobytes(), u.tobytes(), f.tobytes(), best, s["returns"].tobytes(),
                    s["offsets"].tobytes(), s["hit_point"].tobytes(), s["range"].tobytes(),
                    s["point_mask"].tobytes(), s["seen_points"].tobytes(), tot.tobytes(),
                    cov.tobytes(), flags.tobytes(), rep.best_idx, rep.green], s

        before, scan = others()
        got = ctx.place_coverage(poses, fan, 4, min_separation=1.0, fixed=(2,),
                                 want_round_gains=True, want_owner=True)
        after, _ = others()
        again = ctx.place_coverage(poses, fan, 4, min_separation=1.0, fixed=(2,),
                                   want_round_gains=True, want_owner=True)
    finally:
        ctx.close()
    assert before == after
    np.testing.assert_array_equal(got["seen_points"], scan["seen_points"])
    # the placement on the scan's own mask (eight poses fit it): the same answer
    m = scan["point_mask"]
    seen = [np.nonzero((m >> np.uint64(q)) & np.uint64(1))[0] for q in range(8)]
    ref = cover_ref.greedy(seen, poses[:, :2], m.size, 4, 1.0, (2,))
    assert ref["n_selected"] >= 1
    cover_ref.assert_cover_equal(got, ref)
    for k in ("selected", "gain", "round_gains", "point_owner"):
        assert again[k].tobytes() == got[k].tobytes(), k


def _raw(ctx, poses, n, fan, cp, roi, roi_n, owner_cap, N, mounted_table=None, null=None):
    """One raw call with sentinel-filled outputs -> (rc, True when every output kept its
    sentinel, n_points)."""
    sel = np.full(16, -7, np.int64)
    gain, cov = np.full(16, 7, np.uint64), np.full(16, 7, np.uint64)
    rg = np.full((16, max(n, 1)), -7, np.int64)
    seen = np.full(max(n, 1), 7, np.uint32)
    own = np.full(max(N, 1), -7, np.int32)
    npts, rpts, base = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    ns = C.c_int32(-7)
    args = {"poses": _abi._ptr(poses), "fan": C.byref(fan), "cp": C.byref(cp),
            "selected": _abi._ptr(sel), "gain": _abi._ptr(gain), "covered_after": _abi._ptr(cov),
            "n_points": C.byref(npts), "roi_points": C.byref(rpts), "base_covered": C.byref(base),
            "n_selected": C.byref(ns)}
    if null:
        args[null] = None
    lead = () if mounted_table is None else (_abi._ptr(mounted_table),)
    fn = ctx.lib.pcp_place_coverage if mounted_table is None else ctx.lib.pcp_place_coverage_mounted
    rc = fn(ctx.h, args["poses"], n, args["fan"], *lead, args["cp"], _abi._ptr(roi), roi_n,
            args["selected"], args["gain"], args["covered_after"], _abi._ptr(rg), _abi._ptr(seen),
            _abi._ptr(own), owner_cap, args["n_points"], args["roi_points"], args["base_covered"],
            args["n_selected"])
    clean = ((sel == -7).all() and (gain == 7).all() and (cov == 7).all() and (rg == -7).all() and
             (seen == 7).all() and (own == -7).all() and rpts.value == 7 and base.value == 7 and
             ns.value == -7)
    return rc, bool(clean), npts.value


def test_refusals_leave_the_outputs_alone(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ctx, N, fan = clutter_ctx, inst["N"], inst["fan"]
    poses = np.ascontiguousarray(inst["poses"])
    n = poses.shape[0]
    many = np.ascontiguousarray(np.resize(poses, (_abi.COVER_MAX_POSES + 1, 5)))
    roi = np.ones(N, np.uint8)

    def cp(k=4, fixed=(), reserved=0, n_fixed=None, r1=0):
        c = _abi.Context._cover_params(k, 0.0, fixed, reserved, n_fixed)
        c.reserved[1] = r1
        return c

    invalid = [
        ("fan n_az", (poses, n, _abi.fan_params(n_az=0, n_el=4), cp(), None, 0)),
        ("fan n_el", (poses, n, _abi.fan_params(n_az=64, n_el=-1), cp(), None, 0)),
        ("steps", (poses, n, _abi.fan_params(n_az=64, n_el=4, max_distance=0.5 + 0.3 * 5000),
                   cp(), None, 0)),
        ("too many poses", (many, many.shape[0], _abi.fan_params(n_az=8, n_el=2), cp(), None, 0)),
        ("too many rays", (poses, n, _abi.fan_params(n_az=8192, n_el=4096), cp(), None, 0)),
        ("k_max 0", (poses, n, fan, cp(0), None, 0)),
        ("k_max 17", (poses, n, fan, cp(17), None, 0)),
        ("n_fixed -1", (poses, n, fan, cp(n_fixed=-1), None, 0)),
        ("n_fixed 17", (poses, n, fan, cp(n_fixed=17), None, 0)),
        ("reserved[0]", (poses, n, fan, cp(reserved=1), None, 0)),
        ("reserved[1]", (poses, n, fan, cp(r1=1), None, 0)),
        ("fixed >= n", (poses, n, fan, cp(fixed=(3, n)), None, 0)),
        ("fixed < 0", (poses, n, fan, cp(fixed=(-1,)), None, 0)),
        ("fixed twice", (poses, n, fan, cp(fixed=(3, 5, 3)), None, 0)),
        ("roi_n", (poses, n, fan, cp(), roi, N - 1)),
    ]
    for name, (ps, cnt, f, c, r, rn) in invalid:
        rc, clean, npts = _raw(ctx, ps, cnt, f, c, r, rn, N, N)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, name
    for null in ("poses", "fan", "cp", "selected", "gain", "covered_after", "n_points",
                 "roi_points", "base_covered", "n_selected"):
        rc, clean, npts = _raw(ctx, poses, n, fan, cp(), None, 0, N, N, null=null)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, null
    # the mounted twin: a non-finite beam entry
    p6 = np.ascontiguousarray(mount_ref.clutter_poses6())
    f5 = _abi.fan_params(n_az=100, n_el=5)
    table = np.array([-0.4, 0.1, np.nan, 0.26, -1.2])
    rc, clean, npts = _raw(ctx, p6, 6, f5, cp(), None, 0, N, N, mounted_table=table)
    assert rc == _abi.PCP_E_INVALID and clean and npts == 7
    # a short owner array: the size is reported, nothing else is written
    rc, clean, npts = _raw(ctx, poses, n, fan, cp(), None, 0, N - 1, N)
    assert rc == _abi.PCP_E_CAPACITY and clean and npts == N
    with pytest.raises(_abi.PcpError) as ei:
        ctx.place_coverage(poses, fan, 4, want_owner=True, owner_cap=N - 1)
    assert ei.value.code == _abi.PCP_E_CAPACITY
    # and the context still answers
    cover_ref.assert_cover_equal(_call(ctx, inst, 0), cover_ref.grid_case(oracle, 0))


def test_empty_cases(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    N = inst["N"]
    roi = inst["rois"]["box"]
    got = clutter_ctx.place_coverage(np.zeros((0, 5)), inst["fan"], 3, roi=roi, want_owner=True)
    assert got["n_selected"] == 0 and got["base_covered"] == 0 and got["n_points"] == N
    assert got["roi_points"] == int(np.count_nonzero(roi))
    assert (got["point_owner"] == _abi.OWNER_NONE).all()
    ctx = _abi.Context(0)
    try:   # no terrain index: N = 0
        got = ctx.place_coverage(inst["poses"][:3], inst["fan"], 3, want_owner=True)
    finally:
        ctx.close()
    assert got["n_selected"] == 0 and got["n_points"] == 0 and got["roi_points"] == 0
    assert got["base_covered"] == 0 and got["point_owner"].size == 0


def test_burst_reports_three_phases(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ms = clutter_ctx.place_coverage_burst(inst["poses"], inst["fan"], 4, cover_ref.SEP, (10,),
                                          inst["rois"]["xpos"], reps=2)
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)
    # the timing entry commits nothing a later call could see
    cover_ref.assert_cover_equal(_call(clutter_ctx, inst, 1), cover_ref.grid_case(oracle, 1))
