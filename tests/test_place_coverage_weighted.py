"""pcp_place_coverage_weighted on the GPU: every output -- selection, weight and point gains,
covered weight, the rounds' gain rows, per-pose counts, owners, the region's points and weight --
equal to the NumPy restatement of the definition (tests/cover_weight_ref.py) on the ORACLE's first
hits and scan_ref's resolve; all of it integers, so equal means equal."""
import ctypes as C

import cover_ref
import cover_weight_ref as wr
import mount_ref
import numpy as np
import pytest
import scan_ref
from test_place_coverage import SMALL_POSES, TABLE, _ring_cloud

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

BYTES = ("selected", "gain", "gain_points", "covered_after", "round_gains", "seen_points",
         "point_owner")
SCALARS = ("n_selected", "n_points", "roi_points", "roi_weight", "base_covered", "base_points")


def _call(ctx, oracle, i, **kw):
    inst = cover_ref.instance(oracle)
    name, sep, fixed, k = wr.GRID[i]
    return ctx.place_coverage_weighted(inst["poses"], inst["fan"], wr.weights(oracle)[name], k,
                                       sep, fixed, want_round_gains=True, want_owner=True, **kw)


@pytest.fixture(scope="module")
def clutter_ctx():
    ctx = _abi.Context(0)
    ctx.set_terrain(scan_ref.clutter_cloud())
    yield ctx
    ctx.close()


@pytest.mark.parametrize("i", range(len(wr.GRID)))
def test_grid_equals_the_restatement(oracle, clutter_ctx, i):
    """71 poses, N % 64 = 44, two word chunks and nine pose groups per round; one, four and eight
    planes, weights with zeros, gains past 16 bits, ties at the maximum, fixed sensors."""
    name, _, _, _ = wr.GRID[i]
    ref = wr.grid_case(oracle, i)
    got = _call(clutter_ctx, oracle, i)
    print(wr.GRID[i], "selected", got["selected"].tolist(), "gain", got["gain"].tolist(),
          "gain_points", got["gain_points"].tolist())
    wr.assert_weighted_equal(got, ref)
    # the blind spots: R and owner == NONE, their weight what the placement leaves uncovered
    w = wr.weights(oracle)[name].astype(np.int64)
    assert (got["point_owner"][w == 0] == _abi.OWNER_NONE).all()
    blind = (got["point_owner"] == _abi.OWNER_NONE) & (w != 0)
    covered = int(got["covered_after"][-1]) if got["n_selected"] else got["base_covered"]
    assert int(w[blind].sum()) == got["roi_weight"] - covered
    assert int(blind.sum()) == got["roi_points"] - got["base_points"] - int(
        got["gain_points"].sum())


@pytest.mark.parametrize("s", range(len(wr.SETTINGS)))
def test_unit_weights_give_the_bytes_of_place_coverage(oracle, clutter_ctx, s):
    """`ones` against roi None and a 0/1 region against that roi, on the same context: every
    shared output byte for byte, gain_points == gain, roi_weight == roi_points."""
    inst = cover_ref.instance(oracle)
    sep, fixed, k = wr.SETTINGS[s]
    for region in (None, inst["rois"]["xpos"]):
        weight = np.ones(inst["N"], np.uint8) if region is None else region
        par = clutter_ctx.place_coverage(inst["poses"], inst["fan"], k, sep, fixed, region,
                                         want_round_gains=True, want_owner=True)
        got = clutter_ctx.place_coverage_weighted(inst["poses"], inst["fan"], weight, k, sep,
                                                  fixed, want_round_gains=True, want_owner=True)
        assert par["n_selected"] >= 2
        for key in ("selected", "gain", "covered_after", "round_gains", "seen_points",
                    "point_owner"):
            assert got[key].tobytes() == par[key].tobytes(), key
        for key in ("n_selected", "n_points", "roi_points", "base_covered"):
            assert got[key] == par[key], key
        assert got["gain_points"].tobytes() == got["gain"].tobytes()
        assert got["roi_weight"] == got["roi_points"]
        assert got["base_points"] == got["base_covered"]


@pytest.mark.parametrize("s", range(len(wr.SETTINGS)))
def test_one_weight_scales_the_answer(oracle, clutter_ctx, s):
    """`x128` (bit 7 alone: one plane, shifted): place_coverage's selection on xpos with 128
    times the gains."""
    inst = cover_ref.instance(oracle)
    sep, fixed, k = wr.SETTINGS[s]
    par = clutter_ctx.place_coverage(inst["poses"], inst["fan"], k, sep, fixed,
                                     inst["rois"]["xpos"], want_round_gains=True,
                                     want_owner=True)
    got = _call(clutter_ctx, oracle, wr.PATTERNS.index("x128") * len(wr.SETTINGS) + s)
    assert got["selected"].tobytes() == par["selected"].tobytes()
    assert got["point_owner"].tobytes() == par["point_owner"].tobytes()
    for key in ("gain", "covered_after"):
        np.testing.assert_array_equal(got[key], par[key] * np.uint64(128), err_msg=key)
    np.testing.assert_array_equal(got["round_gains"],
                                  np.where(par["round_gains"] < 0, -1, 128 * par["round_gains"]))
    np.testing.assert_array_equal(got["gain_points"], par["gain"])
    assert got["base_covered"] == 128 * par["base_covered"]
    assert got["base_points"] == par["base_covered"]
    assert got["roi_weight"] == 128 * par["roi_points"] and got["roi_points"] == par["roi_points"]


@pytest.mark.parametrize("n_pts,nan_rows", [(10, 0), (64, 0), (64, 6)])
def test_one_word_clouds_and_non_finite_rows(oracle, n_pts, nan_rows):
    """10 points (one partial word), 64 points (N % 64 == 0, the padding word beside it) and 70
    rows of which 6 are non-finite: those carry weight 255, count in roi_points and roi_weight
    and are never owned."""
    cloud = _ring_cloud(n_pts, nan_rows)
    N = cloud.shape[0]
    bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
    assert bad.sum() == nan_rows
    weight = (1 + np.arange(N) % 7).astype(np.uint8)
    weight[bad] = 255
    fan = _abi.fan_params(n_az=100, n_el=5, el_min_deg=-10.0, el_max_deg=10.0)
    seen = cover_ref.level_seen(oracle, cloud, SMALL_POSES, fan)
    assert seen[0].size >= min(n_pts, 8) and seen[2].size == 0
    ref = wr.greedy(seen, SMALL_POSES[:, :2], weight, 4)
    assert ref["n_selected"] >= 1
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        got = ctx.place_coverage_weighted(SMALL_POSES, fan, weight, 4, want_round_gains=True,
                                          want_owner=True)
    finally:
        ctx.close()
    wr.assert_weighted_equal(got, ref)
    assert got["roi_points"] == N == got["n_points"]
    assert got["roi_weight"] == int(weight.astype(np.int64).sum())
    if nan_rows:
        assert (got["point_owner"][bad] == _abi.OWNER_NONE).all()
        assert int(got["covered_after"][-1]) <= got["roi_weight"] - 255 * nan_rows


def test_mounted_with_a_beam_table(oracle, clutter_ctx):
    """The six tilted clutter mounts with a non-uniform beam table and box200 weights, against the
    restatement on mount_ref's own march and resolve."""
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    seen = cover_ref.seen_sets(case[3], 6)
    weight = wr.weights(oracle)["box200"]
    for sep, fixed in ((0.0, ()), (3.0, (1,))):
        ref = wr.greedy(seen, poses6[:, :2], weight, 6, sep, fixed)
        assert ref["n_selected"] >= 2
        got = clutter_ctx.place_coverage_weighted_mounted(poses6, fan, weight, TABLE, 6, sep,
                                                          fixed, want_round_gains=True,
                                                          want_owner=True)
        wr.assert_weighted_equal(got, ref)
    # the level call on the same context afterwards: the direction cache holds no stale table
    lvl = clutter_ctx.place_coverage_weighted(scan_ref.CLUTTER_POSES, fan, weight, 2)
    scan = clutter_ctx.simulate_scan(scan_ref.CLUTTER_POSES, fan)
    np.testing.assert_array_equal(lvl["seen_points"], scan["seen_points"])


def test_three_calls_give_identical_bytes(oracle):
    """A fresh context: the index's copies are built at the second query, so the resolve runs
    behind different march layouts; the answer and its bytes stay."""
    inst = cover_ref.instance(oracle)
    i = wr.GRID.index(("three", cover_ref.SEP, (10, 40), 4))
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(inst["cloud"])
        runs = [_call(ctx, oracle, i) for _ in range(3)]
    finally:
        ctx.close()
    wr.assert_weighted_equal(runs[0], wr.grid_case(oracle, i))
    for r in runs[1:]:
        for k in BYTES:
            assert r[k].tobytes() == runs[0][k].tobytes(), k
        for k in SCALARS:
            assert r[k] == runs[0][k], k


def test_other_queries_are_not_disturbed(scene, cells, aux):
    """raycast_fan, simulate_scan, score_poses and place_coverage after the weighted placement
    give the bytes they gave before it: the call's scratch is its own."""
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
        N = ctx.scan_points()
        weight = (1 + (37 * np.arange(N)) % 255).astype(np.uint8)

        def others():
            b, u, f, best = ctx.raycast_fan(poses, fan, want_first_hit=True)
            s = ctx.simulate_scan(poses, fan, want_dense=True)
            flags = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, p, flags)
            c = ctx.place_coverage(poses, fan, 4, min_separation=1.0, fixed=(2,),
                                   want_round_gains=True, want_owner=True)
            return [b.tobytes(), u.tobytes(), f.tobytes(), best, s["returns"].tobytes(),
                    s["offsets"].tobytes(), s["hit_point"].tobytes(), s["range"].tobytes(),
                    s["point_mask"].tobytes(), s["seen_points"].tobytes(), tot.tobytes(),
                    cov.tobytes(), flags.tobytes(), rep.best_idx, rep.green,
                    c["selected"].tobytes(), c["gain"].tobytes(), c["round_gains"].tobytes(),
                    c["point_owner"].tobytes(), c["roi_points"], c["base_covered"]], s

        before, scan = others()
        got = ctx.place_coverage_weighted(poses, fan, weight, 4, min_separation=1.0, fixed=(2,),
                                          want_round_gains=True, want_owner=True)
        after, _ = others()
    finally:
        ctx.close()
    assert before == after
    # the placement on the scan's own mask (eight poses fit it): the same answer
    m = scan["point_mask"]
    seen = [np.nonzero((m >> np.uint64(q)) & np.uint64(1))[0] for q in range(8)]
    ref = wr.greedy(seen, poses[:, :2], weight, 4, 1.0, (2,))
    assert ref["n_selected"] >= 1
    wr.assert_weighted_equal(got, ref)


def _raw(ctx, poses, n, fan, cp, weight, weight_n, owner_cap, N, mounted_table=None, null=None):
    """One raw call with sentinel-filled outputs -> (rc, True when every output kept its
    sentinel, n_points)."""
    sel = np.full(16, -7, np.int64)
    gain, cov, gpts = (np.full(16, 7, np.uint64) for _ in range(3))
    rg = np.full((16, max(n, 1)), -7, np.int64)
    seen = np.full(max(n, 1), 7, np.uint32)
    own = np.full(max(N, 1), -7, np.int32)
    npts, rpts, rw = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    base, bpts = C.c_uint64(7), C.c_uint64(7)
    ns = C.c_int32(-7)
    args = {"poses": _abi._ptr(poses), "fan": C.byref(fan), "cp": C.byref(cp),
            "weight": _abi._ptr(weight), "selected": _abi._ptr(sel), "gain": _abi._ptr(gain),
            "covered_after": _abi._ptr(cov), "n_points": C.byref(npts),
            "roi_points": C.byref(rpts), "roi_weight": C.byref(rw),
            "base_covered": C.byref(base), "base_points": C.byref(bpts),
            "n_selected": C.byref(ns)}
    if null:
        args[null] = None
    lead = () if mounted_table is None else (_abi._ptr(mounted_table),)
    fn = (ctx.lib.pcp_place_coverage_weighted if mounted_table is None
          else ctx.lib.pcp_place_coverage_weighted_mounted)
    rc = fn(ctx.h, args["poses"], n, args["fan"], *lead, args["cp"], args["weight"], weight_n,
            args["selected"], args["gain"], args["covered_after"], _abi._ptr(gpts), _abi._ptr(rg),
            _abi._ptr(seen), _abi._ptr(own), owner_cap, args["n_points"], args["roi_points"],
            args["roi_weight"], args["base_covered"], args["base_points"], args["n_selected"])
    clean = ((sel == -7).all() and (gain == 7).all() and (cov == 7).all() and (gpts == 7).all() and
             (rg == -7).all() and (seen == 7).all() and (own == -7).all() and rpts.value == 7 and
             rw.value == 7 and base.value == 7 and bpts.value == 7 and ns.value == -7)
    return rc, bool(clean), npts.value


def test_refusals_leave_the_outputs_alone(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ctx, N, fan = clutter_ctx, inst["N"], inst["fan"]
    poses = np.ascontiguousarray(inst["poses"])
    n = poses.shape[0]
    many = np.ascontiguousarray(np.resize(poses, (_abi.COVER_MAX_POSES + 1, 5)))
    weight = wr.weights(oracle)["ramp"]

    def cp(k=4, fixed=(), reserved=0, n_fixed=None, r1=0):
        c = _abi.Context._cover_params(k, 0.0, fixed, reserved, n_fixed)
        c.reserved[1] = r1
        return c

    invalid = [
        ("fan n_az", (poses, n, _abi.fan_params(n_az=0, n_el=4), cp(), weight, N)),
        ("fan n_el", (poses, n, _abi.fan_params(n_az=64, n_el=-1), cp(), weight, N)),
        ("steps", (poses, n, _abi.fan_params(n_az=64, n_el=4, max_distance=0.5 + 0.3 * 5000),
                   cp(), weight, N)),
        ("too many poses", (many, many.shape[0], _abi.fan_params(n_az=8, n_el=2), cp(), weight,
                            N)),
        ("too many rays", (poses, n, _abi.fan_params(n_az=8192, n_el=4096), cp(), weight, N)),
        ("k_max 0", (poses, n, fan, cp(0), weight, N)),
        ("k_max 17", (poses, n, fan, cp(17), weight, N)),
        ("n_fixed -1", (poses, n, fan, cp(n_fixed=-1), weight, N)),
        ("n_fixed 17", (poses, n, fan, cp(n_fixed=17), weight, N)),
        ("reserved[0]", (poses, n, fan, cp(reserved=1), weight, N)),
        ("reserved[1]", (poses, n, fan, cp(r1=1), weight, N)),
        ("fixed >= n", (poses, n, fan, cp(fixed=(3, n)), weight, N)),
        ("fixed < 0", (poses, n, fan, cp(fixed=(-1,)), weight, N)),
        ("fixed twice", (poses, n, fan, cp(fixed=(3, 5, 3)), weight, N)),
        ("weight null", (poses, n, fan, cp(), None, N)),
        ("weight null, 0", (poses, n, fan, cp(), None, 0)),
        ("weight_n", (poses, n, fan, cp(), weight, N - 1)),
    ]
    for name, (ps, cnt, f, c, w, wn) in invalid:
        rc, clean, npts = _raw(ctx, ps, cnt, f, c, w, wn, N, N)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, name
    for null in ("poses", "fan", "cp", "selected", "gain", "covered_after", "n_points",
                 "roi_points", "roi_weight", "base_covered", "base_points", "n_selected"):
        rc, clean, npts = _raw(ctx, poses, n, fan, cp(), weight, N, N, N, null=null)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, null
    # the mounted twin: a non-finite beam entry
    p6 = np.ascontiguousarray(mount_ref.clutter_poses6())
    f5 = _abi.fan_params(n_az=100, n_el=5)
    table = np.array([-0.4, 0.1, np.nan, 0.26, -1.2])
    rc, clean, npts = _raw(ctx, p6, 6, f5, cp(), weight, N, N, N, mounted_table=table)
    assert rc == _abi.PCP_E_INVALID and clean and npts == 7
    # a short owner array: the size is reported, nothing else is written
    rc, clean, npts = _raw(ctx, poses, n, fan, cp(), weight, N, N - 1, N)
    assert rc == _abi.PCP_E_CAPACITY and clean and npts == N
    with pytest.raises(_abi.PcpError) as ei:
        ctx.place_coverage_weighted(poses, fan, weight, 4, want_owner=True, owner_cap=N - 1)
    assert ei.value.code == _abi.PCP_E_CAPACITY
    # and the context still answers
    wr.assert_weighted_equal(_call(ctx, oracle, 0), wr.grid_case(oracle, 0))


def test_empty_cases(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    N = inst["N"]
    weight = wr.weights(oracle)["ramp0"]
    got = clutter_ctx.place_coverage_weighted(np.zeros((0, 5)), inst["fan"], weight, 3,
                                              want_owner=True)
    assert got["n_selected"] == 0 and got["n_points"] == N
    assert got["base_covered"] == 0 and got["base_points"] == 0
    assert got["roi_points"] == int(np.count_nonzero(weight))
    assert got["roi_weight"] == int(weight.astype(np.int64).sum())
    assert (got["point_owner"] == _abi.OWNER_NONE).all()
    ctx = _abi.Context(0)
    try:   # no terrain index: N = 0
        got = ctx.place_coverage_weighted(inst["poses"][:3], inst["fan"], np.zeros(0, np.uint8), 3,
                                          want_owner=True)
    finally:
        ctx.close()
    assert got["n_selected"] == 0 and got["n_points"] == 0
    assert got["roi_points"] == 0 and got["roi_weight"] == 0
    assert got["base_covered"] == 0 and got["base_points"] == 0
    assert got["point_owner"].size == 0 and got["seen_points"].tolist() == [0, 0, 0]


def test_all_zero_weights_place_nothing(oracle, clutter_ctx):
    """R empty: the build runs with one empty plane and round 0 stops on a gain of 0."""
    inst = cover_ref.instance(oracle)
    got = clutter_ctx.place_coverage_weighted(inst["poses"], inst["fan"],
                                              np.zeros(inst["N"], np.uint8), 3, want_owner=True)
    assert got["n_selected"] == 0 and got["roi_points"] == 0 and got["roi_weight"] == 0
    assert (got["point_owner"] == _abi.OWNER_NONE).all()
    np.testing.assert_array_equal(got["seen_points"],
                                  np.array([s.size for s in inst["seen"]], np.uint32))


def test_burst_reports_three_phases(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ms = clutter_ctx.place_coverage_weighted_burst(inst["poses"], inst["fan"],
                                                   wr.weights(oracle)["three"], 4, cover_ref.SEP,
                                                   (10,), reps=2)
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)
    ms = clutter_ctx.place_coverage_weighted_mounted_burst(
        mount_ref.clutter_poses6(), _abi.fan_params(n_az=100, n_el=5),
        wr.weights(oracle)["box200"], TABLE, 2, reps=2)
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)
    # the timing entry commits nothing a later call could see
    i = wr.GRID.index(("box200", cover_ref.SEP, (), 16))
    wr.assert_weighted_equal(_call(clutter_ctx, oracle, i), wr.grid_case(oracle, i))
