"""pcp_place_coverage_aimed on the GPU: every output -- poses, aims, gains, covered counts, the
rounds' [n][n_aims] tables, per-pose and per-aim counts, owners -- equal to the NumPy restatement
of the definition (tests/cover_aim_ref.py) on the ORACLE's first hits and scan_ref's resolve; all
of it integers, so equal means equal.  The case grid and its preconditions are
tests/test_cover_aim_ref.py's."""
import ctypes as C

import cover_aim_ref as car
import cover_ref
import mount_ref
import numpy as np
import pytest
import scan_ref
from test_place_coverage import SMALL_POSES, TABLE, _ring_cloud

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu


def _call(ctx, inst, i, **kw):
    table, roi, sep, fixed, k = car.GRID[i]
    w_az, w_el, aims = car.TABLES[table]
    return ctx.place_coverage_aimed(inst["poses"], inst["fan"], w_az, w_el, aims, k, sep, fixed,
                                    inst["rois"][roi], want_round_gains=True, want_owner=True,
                                    want_aim_points=True, **kw)


@pytest.fixture(scope="module")
def clutter_ctx():
    ctx = _abi.Context(0)
    ctx.set_terrain(scan_ref.clutter_cloud())
    yield ctx
    ctx.close()


@pytest.mark.parametrize("i", range(len(car.GRID)))
def test_grid_equals_the_restatement(oracle, clutter_ctx, i):
    """71 poses, 100 x 37 fan, N % 64 = 44: 24 and 64 aims and the one full window; wrapping
    windows, bands at both ends, identical aims, three regions, a separation with its equalities,
    fixed (pose, aim) pairs, early stops."""
    inst = car.instance(oracle)
    ref = car.grid_case(oracle, i)
    got = _call(clutter_ctx, inst, i)
    print(car.GRID[i][:3], "selected", got["selected"].tolist(), "aim",
          got["selected_aim"].tolist(), "gain", got["gain"].tolist())
    car.assert_aimed_equal(got, ref)
    roi = inst["rois"][car.GRID[i][1]]
    if roi is not None:   # nothing outside the region is owned
        assert (got["point_owner"][roi == 0] == _abi.OWNER_NONE).all()
    blind = (got["point_owner"] == _abi.OWNER_NONE) & (True if roi is None else roi != 0)
    assert int(blind.sum()) == got["roi_points"] - (
        int(got["covered_after"][-1]) if got["n_selected"] else got["base_covered"])


def test_outputs_not_asked_for_do_not_change_the_rest(oracle, clutter_ctx):
    inst = car.instance(oracle)
    table, roi, sep, fixed, k = car.GRID[4]
    w_az, w_el, aims = car.TABLES[table]
    got = clutter_ctx.place_coverage_aimed(inst["poses"], inst["fan"], w_az, w_el, aims, k, sep,
                                           fixed, inst["rois"][roi])
    assert got["round_gains"] is None and got["aim_points"] is None and got["point_owner"] is None
    car.assert_aimed_equal(got, car.grid_case(oracle, 4))


@pytest.mark.parametrize("i", [6, 7])
def test_one_full_window_is_place_coverage(oracle, clutter_ctx, i):
    """n_aims = 1, w_az = n_az, w_el = n_el: byte-equal to pcp_place_coverage on the same
    arguments."""
    inst = car.instance(oracle)
    table, roi, sep, fixed, k = car.GRID[i]
    assert table == "full"
    got = _call(clutter_ctx, inst, i)
    plain = clutter_ctx.place_coverage(inst["poses"], inst["fan"], k, sep, [f for f, _ in fixed],
                                       inst["rois"][roi], want_round_gains=True, want_owner=True)
    assert plain["n_selected"] >= 2
    for key in ("selected", "gain", "covered_after", "seen_points", "point_owner"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert got["round_gains"][:, :, 0].tobytes() == plain["round_gains"].tobytes()
    for key in ("n_selected", "n_points", "roi_points", "base_covered"):
        assert got[key] == plain[key], key
    assert (got["selected_aim"] == 0).all()
    np.testing.assert_array_equal(got["aim_points"][:, 0], plain["seen_points"])


@pytest.mark.parametrize("n_pts,nan_rows", [(10, 0), (64, 0), (64, 6)])
def test_ring_clouds_a_window_sees_the_points_under_its_azimuths(oracle, n_pts, nan_rows):
    """test_place_coverage.py's 100-ray ring clouds (one partial word; N % 64 == 0 with the padding
    word beside it; 6 non-finite rows): point q lies under azimuth column q of the pose at the
    origin, so a window of w columns from az0 sees exactly the points q with (q - az0) mod 100 < w
    -- the last aim wraps from column 95 to 6."""
    cloud = _ring_cloud(n_pts, nan_rows)
    N = cloud.shape[0]
    fan = _abi.fan_params(n_az=100, n_el=5, el_min_deg=-10.0, el_max_deg=10.0)
    w_az, w_el = 12, 5
    aims = [(0, 0), (6, 0), (30, 0), (58, 0), (95, 0)]
    hits = car.level_hits(oracle, cloud, SMALL_POSES, fan)
    ref = car.greedy(hits, SMALL_POSES[:, :2], N, 100, w_az, w_el, aims, 4)
    assert ref["n_selected"] >= 1 and ref["seen_points"][2] == 0
    # the pose at the origin: each window's points are the ring's points under its columns
    fin = np.nonzero(np.isfinite(cloud[:, :3]).all(axis=1))[0]   # ring point q = row fin[q]
    ray, pt = hits[0]
    assert np.unique(pt).size == n_pts
    for a, (az0, _) in enumerate(aims):
        under = fin[(np.arange(n_pts) - az0) % 100 < w_az]
        assert ref["aim_points"][0, a] == under.size
        inside = car.in_window(ray, 100, az0, 0, w_az, w_el)
        np.testing.assert_array_equal(np.unique(pt[inside]), np.sort(under))
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = ctx.place_coverage_aimed(SMALL_POSES, fan, w_az, w_el, aims, 4,
                                       want_round_gains=True, want_owner=True,
                                       want_aim_points=True)
        with_roi = ctx.place_coverage_aimed(SMALL_POSES, fan, w_az, w_el, aims, 4,
                                            roi=np.ones(N, np.uint8), want_round_gains=True,
                                            want_owner=True, want_aim_points=True)
    finally:
        ctx.close()
    for g in (got, with_roi):
        car.assert_aimed_equal(g, ref)
        assert g["roi_points"] == N and g["n_points"] == N
    if nan_rows:
        bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
        assert bad.sum() == nan_rows and (got["point_owner"][bad] == _abi.OWNER_NONE).all()


def test_three_calls_give_identical_bytes_and_place_coverage_is_unchanged(oracle):
    """A fresh context: the index's copies are built at the second query, so the resolve and the
    mask pass run behind different march layouts; the answer and its bytes stay.  A
    pcp_place_coverage call in between gives the bytes it gives alone: the scratch is the call's
    own."""
    inst = car.instance(oracle)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(inst["cloud"])
        roi_name, sep, fixed, k = cover_ref.GRID[3]

        def plain_call():
            return ctx.place_coverage(inst["poses"], inst["fan"], k, sep, fixed,
                                      inst["rois"][roi_name], want_round_gains=True,
                                      want_owner=True)

        plain = [plain_call()]
        runs = [_call(ctx, inst, 3)]
        plain.append(plain_call())
        runs += [_call(ctx, inst, 3), _call(ctx, inst, 3)]
    finally:
        ctx.close()
    car.assert_aimed_equal(runs[0], car.grid_case(oracle, 3))
    for r in runs[1:]:
        for key in car.KEYS_ARRAY + car.KEYS_TABLE:
            assert r[key].tobytes() == runs[0][key].tobytes(), key
        for key in car.KEYS_SCALAR:
            assert r[key] == runs[0][key], key
    cover_ref.assert_cover_equal(plain[0], cover_ref.grid_case(oracle, 3))
    for key in ("selected", "gain", "covered_after", "round_gains", "seen_points", "point_owner"):
        assert plain[1][key].tobytes() == plain[0][key].tobytes(), key


def test_mounted_with_a_beam_table(clutter_ctx):
    """The six tilted clutter mounts (pitch -0.4363 among them) with an uneven beam table, against
    the restatement on mount_ref's own march and resolve: the window is in the sensor's own
    (i, j)."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    assert poses6[1, 4] == -0.4363
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    hits = car.ray_hits(case[3], 6)
    assert sum(r.size > 0 for r, _ in hits) >= 3
    w_az, w_el = 30, 3
    aims = [(az0, el0) for az0 in (0, 20, 40, 60, 80) for el0 in (0, 2)]
    for sep, fixed in ((0.0, ()), (3.0, ((1, 4),))):
        ref = car.greedy(hits, poses6[:, :2], cloud.shape[0], 100, w_az, w_el, aims, 6, sep, fixed)
        assert ref["n_selected"] >= 2
        got = clutter_ctx.place_coverage_aimed_mounted(poses6, fan, w_az, w_el, aims, TABLE, 6,
                                                       sep, fixed, want_round_gains=True,
                                                       want_owner=True, want_aim_points=True)
        car.assert_aimed_equal(got, ref)


def _raw(ctx, poses, n, fan, ap, aims, roi, roi_n, owner_cap, N, mounted_table=None, null=None):
    """One raw call with sentinel-filled outputs -> (rc, True when every output kept its
    sentinel, n_points)."""
    sel = np.full(16, -7, np.int64)
    sel_aim = np.full(16, -7, np.int32)
    gain, cov = np.full(16, 7, np.uint64), np.full(16, 7, np.uint64)
    rows = max(min(n, 1024), 1) * 64
    rg = np.full((16, rows), -7, np.int64)
    seen = np.full(max(n, 1), 7, np.uint32)
    apts = np.full(rows, 7, np.uint32)
    own = np.full(max(N, 1), -7, np.int32)
    npts, rpts, base = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    ns = C.c_int32(-7)
    args = {"poses": _abi._ptr(poses), "fan": C.byref(fan), "ap": C.byref(ap),
            "aims": _abi._ptr(aims), "selected": _abi._ptr(sel), "selected_aim": _abi._ptr(sel_aim),
            "gain": _abi._ptr(gain), "covered_after": _abi._ptr(cov), "n_points": C.byref(npts),
            "roi_points": C.byref(rpts), "base_covered": C.byref(base), "n_selected": C.byref(ns)}
    if null:
        args[null] = None
    lead = () if mounted_table is None else (_abi._ptr(mounted_table),)
    fn = (ctx.lib.pcp_place_coverage_aimed if mounted_table is None
          else ctx.lib.pcp_place_coverage_aimed_mounted)
    rc = fn(ctx.h, args["poses"], n, args["fan"], *lead, args["ap"], args["aims"], _abi._ptr(roi),
            roi_n, args["selected"], args["selected_aim"], args["gain"], args["covered_after"],
            _abi._ptr(rg), _abi._ptr(seen), _abi._ptr(apts), _abi._ptr(own), owner_cap,
            args["n_points"], args["roi_points"], args["base_covered"], args["n_selected"])
    clean = ((sel == -7).all() and (sel_aim == -7).all() and (gain == 7).all() and
             (cov == 7).all() and (rg == -7).all() and (seen == 7).all() and (apts == 7).all() and
             (own == -7).all() and rpts.value == 7 and base.value == 7 and ns.value == -7)
    return rc, bool(clean), npts.value


def test_refusals_leave_the_outputs_alone(oracle, clutter_ctx):
    inst = car.instance(oracle)
    ctx, N, fan = clutter_ctx, inst["N"], inst["fan"]
    poses = np.ascontiguousarray(inst["poses"])
    n = poses.shape[0]
    many = np.ascontiguousarray(np.resize(poses, (_abi.COVER_MAX_POSES + 1, 5)))
    roi = np.ones(N, np.uint8)
    w_az, w_el, table = car.TABLES["s24"]
    aims = np.array(table, np.int32)
    aims64 = np.array(car.TABLES["a64"][2] + [(0, 0)], np.int32)

    def ap(k=4, A=24, fixed=(), reserved=0, n_fixed=None, wa=w_az, we=w_el, r1=0, r2=0):
        a = _abi.Context._cover_aim_params(k, A, wa, we, 0.0, fixed, reserved)
        if n_fixed is not None:
            a.n_fixed = n_fixed
        a.reserved[1], a.reserved[2] = r1, r2
        return a

    def aim_at(idx, az0, el0):
        t = aims.copy()
        t[idx] = (az0, el0)
        return t

    small = _abi.fan_params(n_az=8, n_el=2)
    invalid = [
        ("fan n_az", (poses, n, _abi.fan_params(n_az=0, n_el=4), ap(wa=1, we=1), aims, None, 0)),
        ("steps", (poses, n, _abi.fan_params(n_az=100, n_el=37, max_distance=0.5 + 0.3 * 5000),
                   ap(), aims, None, 0)),
        ("too many poses", (many, many.shape[0], small, ap(A=1, wa=1, we=1), aims, None, 0)),
        ("too many rays", (poses, n, _abi.fan_params(n_az=8192, n_el=4096), ap(), aims, None, 0)),
        ("k_max 0", (poses, n, fan, ap(0), aims, None, 0)),
        ("k_max 17", (poses, n, fan, ap(17), aims, None, 0)),
        ("n_fixed -1", (poses, n, fan, ap(n_fixed=-1), aims, None, 0)),
        ("n_fixed 17", (poses, n, fan, ap(n_fixed=17), aims, None, 0)),
        ("reserved[0]", (poses, n, fan, ap(reserved=1), aims, None, 0)),
        ("reserved[1]", (poses, n, fan, ap(r1=1), aims, None, 0)),
        ("reserved[2]", (poses, n, fan, ap(r2=-1), aims, None, 0)),
        ("n_aims 0", (poses, n, fan, ap(A=0), aims, None, 0)),
        ("n_aims 65", (poses, n, fan, ap(A=65), aims64, None, 0)),
        ("w_az 0", (poses, n, fan, ap(wa=0), aims, None, 0)),
        ("w_az n_az + 1", (poses, n, fan, ap(wa=101), aims, None, 0)),
        ("w_el 0", (poses, n, fan, ap(we=0), aims, None, 0)),
        ("w_el n_el + 1", (poses, n, fan, ap(we=38), aims, None, 0)),
        ("az0 -1", (poses, n, fan, ap(), aim_at(5, -1, 0), None, 0)),
        ("az0 n_az", (poses, n, fan, ap(), aim_at(23, 100, 0), None, 0)),
        ("el0 -1", (poses, n, fan, ap(), aim_at(0, 3, -1), None, 0)),
        ("el0 past n_el - w_el", (poses, n, fan, ap(), aim_at(7, 3, 37 - w_el + 1), None, 0)),
        ("fixed pose >= n", (poses, n, fan, ap(fixed=((3, 0), (n, 0))), aims, None, 0)),
        ("fixed pose < 0", (poses, n, fan, ap(fixed=((-1, 0),)), aims, None, 0)),
        ("fixed pose twice", (poses, n, fan, ap(fixed=((3, 0), (5, 1), (3, 2))), aims, None, 0)),
        ("fixed aim outside", (poses, n, fan, ap(fixed=((3, 24),)), aims, None, 0)),
        ("fixed aim < 0", (poses, n, fan, ap(fixed=((3, -1),)), aims, None, 0)),
        ("roi_n", (poses, n, fan, ap(), aims, roi, N - 1)),
    ]
    for name, (ps, cnt, f, a, t, r, rn) in invalid:
        rc, clean, npts = _raw(ctx, ps, cnt, f, a, t, r, rn, N, N)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, name
    for null in ("poses", "fan", "ap", "aims", "selected", "selected_aim", "gain", "covered_after",
                 "n_points", "roi_points", "base_covered", "n_selected"):
        rc, clean, npts = _raw(ctx, poses, n, fan, ap(), aims, None, 0, N, N, null=null)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, null
    # the mounted twin: a non-finite beam entry
    p6 = np.ascontiguousarray(mount_ref.clutter_poses6())
    f5 = _abi.fan_params(n_az=100, n_el=5)
    beams = np.array([-0.4, 0.1, np.nan, 0.26, -1.2])
    rc, clean, npts = _raw(ctx, p6, 6, f5, ap(A=2, wa=10, we=2), aims[:2] * 0, None, 0, N, N,
                           mounted_table=beams)
    assert rc == _abi.PCP_E_INVALID and clean and npts == 7
    # a short owner array: the size is reported, nothing else is written
    rc, clean, npts = _raw(ctx, poses, n, fan, ap(), aims, None, 0, N - 1, N)
    assert rc == _abi.PCP_E_CAPACITY and clean and npts == N
    with pytest.raises(_abi.PcpError) as ei:
        ctx.place_coverage_aimed(poses, fan, w_az, w_el, aims, 4, want_owner=True,
                                 owner_cap=N - 1)
    assert ei.value.code == _abi.PCP_E_CAPACITY
    # and the context still answers
    car.assert_aimed_equal(_call(ctx, inst, 0), car.grid_case(oracle, 0))


def test_empty_cases(oracle, clutter_ctx):
    inst = car.instance(oracle)
    N = inst["N"]
    roi = inst["rois"]["box"]
    w_az, w_el, aims = car.TABLES["s24"]
    got = clutter_ctx.place_coverage_aimed(np.zeros((0, 5)), inst["fan"], w_az, w_el, aims, 3,
                                           roi=roi, want_owner=True)
    assert got["n_selected"] == 0 and got["base_covered"] == 0 and got["n_points"] == N
    assert got["roi_points"] == int(np.count_nonzero(roi))
    assert (got["point_owner"] == _abi.OWNER_NONE).all()
    # the far pose alone sees nothing: no round at all
    far = clutter_ctx.place_coverage_aimed(inst["poses"][4:5], inst["fan"], w_az, w_el, aims, 3,
                                           want_round_gains=True, want_owner=True,
                                           want_aim_points=True)
    assert far["n_selected"] == 0 and far["seen_points"].tolist() == [0]
    assert not far["aim_points"].any() and (far["point_owner"] == _abi.OWNER_NONE).all()
    ctx = _abi.Context(0)
    try:   # no terrain index: N = 0
        got = ctx.place_coverage_aimed(inst["poses"][:3], inst["fan"], w_az, w_el, aims, 3,
                                       want_owner=True, want_aim_points=True)
    finally:
        ctx.close()
    assert got["n_selected"] == 0 and got["n_points"] == 0 and got["roi_points"] == 0
    assert got["base_covered"] == 0 and got["point_owner"].size == 0
    assert got["aim_points"].shape == (3, 24) and not got["aim_points"].any()


def test_burst_reports_three_phases(oracle, clutter_ctx):
    inst = car.instance(oracle)
    w_az, w_el, aims = car.TABLES["s24"]
    ms = clutter_ctx.place_coverage_aimed_burst(inst["poses"], inst["fan"], w_az, w_el, aims, 4,
                                                car.SEP, ((10, 3),), inst["rois"]["xpos"], reps=2)
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)
    # the timing entry commits nothing a later call could see
    car.assert_aimed_equal(_call(clutter_ctx, inst, 1), car.grid_case(oracle, 1))
