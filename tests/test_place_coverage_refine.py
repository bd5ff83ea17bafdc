"""pcp_place_coverage_refine on the GPU: every output -- the refined set, the moves, the
evaluations' tables, the slots' unique points, per-pose counts, owners -- equal to the NumPy
restatement of the definition (tests/cover_refine_ref.py) on the ORACLE's first hits and scan_ref's
resolve; all of it integers, so equal means equal."""
import ctypes as C

import cover_pair_ref
import cover_ref
import cover_refine_ref
import mount_ref
import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

GROUP = 8   # k_crefine_eval's pose group (kEP)


@pytest.fixture(scope="module")
def clutter_ctx():
    ctx = _abi.Context(0)
    ctx.set_terrain(scan_ref.clutter_cloud())
    yield ctx
    ctx.close()


def _call(ctx, oracle, roi, sep, start, n_locked=0, max_moves=16, **kw):
    inst = cover_ref.instance(oracle)
    return ctx.place_coverage_refine(inst["poses"], inst["fan"], start, n_locked, max_moves, sep,
                                     cover_refine_ref.rois(oracle)[roi], want_swap_covered=True,
                                     want_owner=True, **kw)


@pytest.mark.parametrize("roi", cover_refine_ref.REGIONS)
@pytest.mark.parametrize("sep", cover_refine_ref.SEPS)
def test_grid_equals_the_restatement(oracle, clutter_ctx, roi, sep):
    """71 poses (nine pose groups, the last partial), N % 64 = 44, a partial last chunk of words;
    ties (row 70 = row 35), an exact-equality separation, locked slots, moves that run out, the
    regions where greedy's two are not the best pair.  Per region and separation: k x start x
    n_locked x max_moves."""
    calls = moved = 0
    for k in cover_refine_ref.KS:
        for kind in cover_refine_ref.STARTS:
            start = cover_refine_ref.start_set(oracle, roi, sep, k, kind)
            for n_locked in cover_refine_ref.locked_counts(k):
                for mm in cover_refine_ref.MOVES:
                    ref = cover_refine_ref.grid_case(oracle, roi, sep, k, kind, n_locked, mm)
                    got = _call(clutter_ctx, oracle, roi, sep, start, n_locked, mm)
                    try:
                        cover_refine_ref.assert_refine_equal(got, ref)
                    except AssertionError:
                        print("case", roi, sep, k, kind, start, n_locked, mm)
                        raise
                    assert got["swap_covered"].shape == (got["n_moves"] + 1, k, 71)
                    assert got["selected"][:n_locked].tolist() == start[:n_locked]
                    calls += 1
                    moved += got["n_moves"]
    print(roi, sep, "calls", calls, "moves", moved)
    r = cover_refine_ref.rois(oracle)[roi]
    if r is not None:   # nothing outside the region is owned
        assert (got["point_owner"][r == 0] == _abi.OWNER_NONE).all()
    blind = (got["point_owner"] == _abi.OWNER_NONE) & (True if r is None else r != 0)
    assert int(blind.sum()) == got["roi_points"] - got["covered"]


@pytest.mark.parametrize("row", range(len(cover_refine_ref.TABLE)))
def test_the_table_rows(oracle, clutter_ctx, row):
    roi, sep, start, moves, start_covered, final = cover_refine_ref.TABLE[row]
    got = _call(clutter_ctx, oracle, roi, sep, start)
    seq = list(zip(got["move_slot"].tolist(), got["move_from"].tolist(), got["move_to"].tolist(),
                   got["move_covered"].tolist()))
    print(roi, sep, start, got["start_covered"], seq, got["selected"].tolist())
    assert got["start_covered"] == start_covered and seq == moves
    assert got["selected"].tolist() == final and got["converged"] == 1


def test_rows_are_the_greedy_route(oracle, clutter_ctx):
    """The route that existed: for each slot i one pcp_place_coverage call with the other slots
    fixed and one round.  Its base and its round gains are the evaluation's row, wherever the pose
    is alive there and is not s_i itself."""
    inst = cover_ref.instance(oracle)
    roi = cover_refine_ref.rois(oracle)["xpos"]
    for sep, start in ((0.0, [51, 49, 43]), (cover_ref.SEP, [0, 1, 2, 3])):
        got = clutter_ctx.place_coverage_refine(inst["poses"], inst["fan"], start, 0, 0, sep, roi,
                                                want_swap_covered=True)
        checked = 0
        for i, s_i in enumerate(start):
            rest = [p for p in start if p != s_i]
            slow = clutter_ctx.place_coverage(inst["poses"], inst["fan"], 1, sep, rest, roi,
                                              want_round_gains=True)
            assert slow["n_selected"] == 1
            g = slow["round_gains"][0]
            alive = g >= 0
            alive[s_i] = False
            row = got["swap_covered"][0, i]
            np.testing.assert_array_equal(row[alive], int(slow["base_covered"]) + g[alive])
            assert (row[~alive] == -1).all()
            checked += int(alive.sum())
        assert checked > 60


def test_greedys_pair_becomes_the_exact_pair(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    for name in ("box_a", "box_b"):
        roi = cover_refine_ref.rois(oracle)[name]
        g = clutter_ctx.place_coverage(inst["poses"], inst["fan"], 2, roi=roi)
        exact = clutter_ctx.place_coverage_pair(inst["poses"], inst["fan"], roi=roi)
        got = clutter_ctx.place_coverage_refine(inst["poses"], inst["fan"], g["selected"], roi=roi)
        assert got["start_covered"] == int(g["covered_after"][-1]) < exact["pair_gain"]
        assert sorted(got["selected"].tolist()) == exact["best_pair"].tolist()
        assert got["covered"] == exact["pair_gain"] and got["converged"] == 1


def test_every_pose_in_the_set_and_a_separation_that_kills_every_move(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    poses = inst["poses"][:3]
    seen = inst["seen"][:3]
    ref = cover_refine_ref.refine(seen, poses[:, :2], inst["N"], [2, 0, 1])
    got = clutter_ctx.place_coverage_refine(poses, inst["fan"], [2, 0, 1], want_swap_covered=True,
                                            want_owner=True)
    cover_refine_ref.assert_refine_equal(got, ref)
    assert got["n_moves"] == 0 and got["converged"] == 1 and (got["swap_covered"] == -1).all()
    # three lattice neighbours 1.25 m apart under 2.6 m: wherever a slot would go, the other is near
    rows = [6, 7, 8]
    poses = inst["poses"][rows]
    seen = [inst["seen"][r] for r in rows]
    ref = cover_refine_ref.refine(seen, poses[:, :2], inst["N"], [0, 1], sep=2.6)
    assert ref["converged"] == 1 and (ref["swap_covered"] == -1).all()
    got = clutter_ctx.place_coverage_refine(poses, inst["fan"], [0, 1], min_separation=2.6,
                                            want_swap_covered=True, want_owner=True)
    cover_refine_ref.assert_refine_equal(got, ref)
    # without it the third pose is tried
    assert (clutter_ctx.place_coverage_refine(poses, inst["fan"], [0, 1], want_swap_covered=True)
            ["swap_covered"][0, :, 2] >= 0).all()


@pytest.mark.parametrize("n", [GROUP, GROUP + 1, 8 * GROUP + 1])
def test_group_edges_on_repeated_rows(oracle, clutter_ctx, n):
    """Seven rows repeated to a whole pose group, one pose past it and one pose past eight groups
    (and past 64): every copy ties with its original, and the first maximum is the lowest."""
    inst = cover_ref.instance(oracle)
    rows = np.array([35, 51, 43, 49, 0, 25, 19])[np.arange(n) % 7]
    poses = np.ascontiguousarray(inst["poses"][rows])
    seen = [inst["seen"][r] for r in rows]
    roi = cover_refine_ref.rois(oracle)["box_a"]
    start = [n - 1, n - 2, n - 3]
    ref = cover_refine_ref.refine(seen, poses[:, :2], inst["N"], start, roi=roi)
    got = clutter_ctx.place_coverage_refine(poses, inst["fan"], start, roi=roi,
                                            want_swap_covered=True, want_owner=True)
    cover_refine_ref.assert_refine_equal(got, ref)
    assert (got["move_to"] < 7).all()


@pytest.mark.parametrize("n_pts,nan_rows", [(10, 0), (64, 0), (64, 6)])
def test_one_word_clouds_and_non_finite_rows(oracle, n_pts, nan_rows):
    """10 points (one partial word), 64 points (N % 64 == 0, the padding word beside it) and 70
    rows of which 6 are non-finite: those count in roi_points and are never owned."""
    cloud = cover_pair_ref.ring_cloud(n_pts, nan_rows)
    N = cloud.shape[0]
    poses = cover_pair_ref.RING_POSES
    fan = _abi.fan_params(n_az=100, n_el=5, el_min_deg=-10.0, el_max_deg=10.0)
    seen = cover_ref.level_seen(oracle, cloud, poses, fan)
    assert seen[0].size >= min(n_pts, 8) and seen[2].size == 0
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        for start in ([2], [2, 3], [3, 2, 1]):
            ref = cover_refine_ref.refine(seen, poses[:, :2], N, start)
            got = ctx.place_coverage_refine(poses, fan, start, want_swap_covered=True,
                                            want_owner=True)
            with_roi = ctx.place_coverage_refine(poses, fan, start, roi=np.ones(N, np.uint8),
                                                 want_swap_covered=True, want_owner=True)
            for g in (got, with_roi):
                cover_refine_ref.assert_refine_equal(g, ref)
                assert g["roi_points"] == N and g["n_points"] == N
            if start == [2]:   # (pose 2 sees nothing: the one slot moves)
                assert ref["n_moves"] == 1 and ref["covered"] >= seen[0].size
    finally:
        ctx.close()
    if nan_rows:
        bad = ~np.isfinite(cloud[:, :3]).all(axis=1)
        assert bad.sum() == nan_rows and (got["point_owner"][bad] == _abi.OWNER_NONE).all()


TABLE = [-0.4, 0.1, -0.05, 0.26, -1.2]


def test_mounted(oracle, clutter_ctx):
    """Zero tilt and no table: the level call's bytes.  The six tilted clutter mounts with a
    non-uniform beam table: the restatement on mount_ref's own march and resolve."""
    inst = cover_ref.instance(oracle)
    p5 = inst["poses"]
    z = np.zeros(p5.shape[0])
    p6 = np.column_stack([p5[:, :3], z, z, p5[:, 4]])
    roi = inst["rois"]["xpos"]
    level = clutter_ctx.place_coverage_refine(p5, inst["fan"], [0, 1, 2, 3], 1, 16, cover_ref.SEP,
                                              roi, want_swap_covered=True, want_owner=True)
    flat = clutter_ctx.place_coverage_refine_mounted(p6, inst["fan"], [0, 1, 2, 3], None, 1, 16,
                                                     cover_ref.SEP, roi, want_swap_covered=True,
                                                     want_owner=True)
    assert level["n_moves"] >= 2
    for k in KEYS:
        assert flat[k].tobytes() == level[k].tobytes(), k
    for k in SCALARS:
        assert flat[k] == level[k], k
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=100, n_el=5)
    poses6 = mount_ref.clutter_poses6()
    case = mount_ref.mount_case(("table", 100, 5), cloud, poses6, fan, TABLE)
    seen = cover_ref.seen_sets(case[3], 6)
    assert sum(q.size > 0 for q in seen) >= 3
    moved = 0
    for sep, start, n_locked in ((0.0, [4, 5], 0), (3.0, [5, 4, 3], 1), (0.0, [0], 0)):
        ref = cover_refine_ref.refine(seen, poses6[:, :2], cloud.shape[0], start, n_locked, 16, sep)
        got = clutter_ctx.place_coverage_refine_mounted(poses6, fan, start, TABLE, n_locked, 16,
                                                        sep, want_swap_covered=True,
                                                        want_owner=True)
        cover_refine_ref.assert_refine_equal(got, ref)
        moved += got["n_moves"]
    assert moved >= 1
    # the level twin on the same context afterwards: the direction cache holds no stale table
    lvl = clutter_ctx.place_coverage_refine(scan_ref.CLUTTER_POSES, fan, [0])
    scan = clutter_ctx.simulate_scan(scan_ref.CLUTTER_POSES, fan)
    np.testing.assert_array_equal(lvl["seen_points"], scan["seen_points"])


KEYS = ("selected", "move_slot", "move_from", "move_to", "move_covered", "swap_covered",
        "slot_unique", "seen_points", "point_owner")
SCALARS = ("covered", "start_covered", "n_moves", "converged", "n_points", "roi_points")


def test_three_calls_give_identical_bytes(oracle):
    """A fresh context: the index's copies are built at the second query, so the resolve runs
    behind different march layouts; the answer and its bytes stay."""
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cover_ref.instance(oracle)["cloud"])
        runs = [_call(ctx, oracle, "all", cover_ref.SEP, [0, 1, 2, 3]) for _ in range(3)]
    finally:
        ctx.close()
    cover_refine_ref.assert_refine_equal(
        runs[0], cover_refine_ref.grid_case(oracle, "all", cover_ref.SEP, 4, "first", 0, 16))
    assert runs[0]["n_moves"] == 6
    for r in runs[1:]:
        for k in KEYS:
            assert r[k].tobytes() == runs[0][k].tobytes(), k
        for k in SCALARS:
            assert r[k] == runs[0][k], k


def test_other_queries_are_not_disturbed(scene, cells, aux):
    """place_coverage, place_coverage_pair, simulate_scan, raycast_fan and score_poses after the
    refinement give the bytes they gave before it: the call's scratch is its own."""
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
            c = ctx.place_coverage(poses, fan, 4, min_separation=1.0, fixed=(2,),
                                   want_round_gains=True, want_owner=True)
            q = ctx.place_coverage_pair(poses, fan, 1.0, (2,), want_pair_gains=True,
                                        want_owner=True)
            flags = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, p, flags)
            return [b.tobytes(), u.tobytes(), f.tobytes(), best, s["returns"].tobytes(),
                    s["offsets"].tobytes(), s["hit_point"].tobytes(), s["range"].tobytes(),
                    s["point_mask"].tobytes(), s["seen_points"].tobytes(), c["selected"].tobytes(),
                    c["gain"].tobytes(), c["round_gains"].tobytes(), c["point_owner"].tobytes(),
                    c["seen_points"].tobytes(), c["base_covered"], q["best_pair"].tobytes(),
                    q["pair_gains"].tobytes(), q["single_gains"].tobytes(),
                    q["point_owner"].tobytes(), q["pair_gain"], q["n_selected"], tot.tobytes(),
                    cov.tobytes(), flags.tobytes(), rep.best_idx, rep.green], s

        before, scan = others()
        got = ctx.place_coverage_refine(poses, fan, [0, 1, 2], 1, 16, 1.0,
                                        want_swap_covered=True, want_owner=True)
        after, _ = others()
        again = ctx.place_coverage_refine(poses, fan, [0, 1, 2], 1, 16, 1.0,
                                          want_swap_covered=True, want_owner=True)
    finally:
        ctx.close()
    assert before == after
    np.testing.assert_array_equal(got["seen_points"], scan["seen_points"])
    # the search on the scan's own mask (eight poses fit it): the same answer
    m = scan["point_mask"]
    seen = [np.nonzero((m >> np.uint64(q)) & np.uint64(1))[0] for q in range(8)]
    ref = cover_refine_ref.refine(seen, poses[:, :2], m.size, [0, 1, 2], 1, 16, 1.0)
    cover_refine_ref.assert_refine_equal(got, ref)
    for k in KEYS:
        assert again[k].tobytes() == got[k].tobytes(), k


def _raw(ctx, poses, n, fan, rp, roi, roi_n, owner_cap, N, mounted_table=None, null=None):
    """One raw call with sentinel-filled outputs -> (rc, True when every output kept its
    sentinel, n_points)."""
    m = max(n, 1)
    sel = np.full(16, -7, np.int64)
    slot = np.full(64, -7, np.int32)
    frm, to = np.full(64, -7, np.int64), np.full(64, -7, np.int64)
    mcov = np.full(64, 7, np.uint64)
    tab = np.full((2, 16, min(m, 80)), -7, np.int64)   # (refused calls only: never written)
    uniq = np.full(16, 7, np.uint64)
    seen = np.full(m, 7, np.uint32)
    own = np.full(max(N, 1), -7, np.int32)
    cov, sc = C.c_uint64(7), C.c_uint64(7)
    npts, rpts = C.c_uint64(7), C.c_uint64(7)
    nm, cv = C.c_int32(-7), C.c_int32(-7)
    args = {"poses": _abi._ptr(poses), "fan": C.byref(fan), "rp": C.byref(rp),
            "selected": _abi._ptr(sel), "covered": C.byref(cov), "start_covered": C.byref(sc),
            "move_slot": _abi._ptr(slot), "move_from": _abi._ptr(frm), "move_to": _abi._ptr(to),
            "move_covered": _abi._ptr(mcov), "n_points": C.byref(npts),
            "roi_points": C.byref(rpts), "n_moves": C.byref(nm), "converged": C.byref(cv)}
    if null:
        args[null] = None
    lead = () if mounted_table is None else (_abi._ptr(mounted_table),)
    fn = (ctx.lib.pcp_place_coverage_refine if mounted_table is None
          else ctx.lib.pcp_place_coverage_refine_mounted)
    rc = fn(ctx.h, args["poses"], n, args["fan"], *lead, args["rp"], _abi._ptr(roi), roi_n,
            args["selected"], args["covered"], args["start_covered"], args["move_slot"],
            args["move_from"], args["move_to"], args["move_covered"], _abi._ptr(tab),
            _abi._ptr(uniq), _abi._ptr(seen), _abi._ptr(own), owner_cap, args["n_points"],
            args["roi_points"], args["n_moves"], args["converged"])
    clean = ((sel == -7).all() and (slot == -7).all() and (frm == -7).all() and (to == -7).all()
             and (mcov == 7).all() and (tab == -7).all() and (uniq == 7).all() and
             (seen == 7).all() and (own == -7).all() and cov.value == 7 and sc.value == 7 and
             rpts.value == 7 and nm.value == -7 and cv.value == -7)
    return rc, bool(clean), npts.value


def test_refusals_leave_the_outputs_alone(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ctx, N, fan = clutter_ctx, inst["N"], inst["fan"]
    poses = np.ascontiguousarray(inst["poses"])
    n = poses.shape[0]
    many = np.ascontiguousarray(np.resize(poses, (_abi.COVER_MAX_POSES + 1, 5)))
    roi = np.ones(N, np.uint8)

    def rp(start=(0, 1), n_locked=0, max_moves=1, reserved=0, k=None):
        return _abi.Context._refine_params(start, n_locked, max_moves, 0.0, reserved, k)

    invalid = [
        ("fan n_az", (poses, n, _abi.fan_params(n_az=0, n_el=4), rp(), None, 0)),
        ("fan n_el", (poses, n, _abi.fan_params(n_az=64, n_el=-1), rp(), None, 0)),
        ("steps", (poses, n, _abi.fan_params(n_az=64, n_el=4, max_distance=0.5 + 0.3 * 5000),
                   rp(), None, 0)),
        ("too many poses", (many, many.shape[0], _abi.fan_params(n_az=8, n_el=2), rp(), None, 0)),
        ("too many rays", (poses, n, _abi.fan_params(n_az=8192, n_el=4096), rp(), None, 0)),
        ("k 0", (poses, n, fan, rp(k=0), None, 0)),
        ("k 17", (poses, n, fan, rp(k=17), None, 0)),
        ("n_locked -1", (poses, n, fan, rp(n_locked=-1), None, 0)),
        ("n_locked > k", (poses, n, fan, rp(n_locked=3), None, 0)),
        ("max_moves -1", (poses, n, fan, rp(max_moves=-1), None, 0)),
        ("max_moves 65", (poses, n, fan, rp(max_moves=65), None, 0)),
        ("reserved", (poses, n, fan, rp(reserved=1), None, 0)),
        ("start >= n", (poses, n, fan, rp(start=(3, n)), None, 0)),
        ("start < 0", (poses, n, fan, rp(start=(-1,)), None, 0)),
        ("start twice", (poses, n, fan, rp(start=(3, 5, 3)), None, 0)),
        ("no poses", (poses, 0, fan, rp(), None, 0)),
        ("roi_n", (poses, n, fan, rp(), roi, N - 1)),
    ]
    for name, (ps, cnt, f, c, r, rn) in invalid:
        rc, clean, npts = _raw(ctx, ps, cnt, f, c, r, rn, N, N)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, name
    for null in ("poses", "fan", "rp", "selected", "covered", "start_covered", "move_slot",
                 "move_from", "move_to", "move_covered", "n_points", "roi_points", "n_moves",
                 "converged"):
        rc, clean, npts = _raw(ctx, poses, n, fan, rp(), None, 0, N, N, null=null)
        assert rc == _abi.PCP_E_INVALID and clean and npts == 7, null
    # the move arrays may be null when no move can be recorded
    rc, clean, npts = _raw(ctx, poses, n, fan, rp(max_moves=0), None, 0, N, N, null="move_to")
    assert rc == _abi.PCP_OK and not clean and npts == N
    # the mounted twin: a non-finite beam entry
    p6 = np.ascontiguousarray(mount_ref.clutter_poses6())
    f5 = _abi.fan_params(n_az=100, n_el=5)
    table = np.array([-0.4, 0.1, np.nan, 0.26, -1.2])
    rc, clean, npts = _raw(ctx, p6, 6, f5, rp(), None, 0, N, N, mounted_table=table)
    assert rc == _abi.PCP_E_INVALID and clean and npts == 7
    # a short owner array: the size is reported, nothing else is written
    rc, clean, npts = _raw(ctx, poses, n, fan, rp(), None, 0, N - 1, N)
    assert rc == _abi.PCP_E_CAPACITY and clean and npts == N
    with pytest.raises(_abi.PcpError) as ei:
        ctx.place_coverage_refine(poses, fan, [0, 1], want_owner=True, owner_cap=N - 1)
    assert ei.value.code == _abi.PCP_E_CAPACITY
    # and the context still answers
    cover_refine_ref.assert_refine_equal(
        _call(ctx, oracle, "box_a", 0.0, [51, 49]),
        cover_refine_ref.grid_case(oracle, "box_a", 0.0, 2, "greedy", 0, 16))


def test_without_terrain(oracle):
    inst = cover_ref.instance(oracle)
    ctx = _abi.Context(0)
    try:   # no terrain index: N = 0
        got = ctx.place_coverage_refine(inst["poses"][:5], inst["fan"], [3, 1],
                                        want_swap_covered=True, want_owner=True)
    finally:
        ctx.close()
    assert got["selected"].tolist() == [3, 1] and got["n_moves"] == 0 and got["converged"] == 1
    assert got["covered"] == got["start_covered"] == got["n_points"] == got["roi_points"] == 0
    assert got["slot_unique"].tolist() == [0, 0] and got["point_owner"].size == 0
    assert got["swap_covered"].shape[0] == 0 and (got["seen_points"] == 0).all()


def test_burst_reports_two_phases(oracle, clutter_ctx):
    inst = cover_ref.instance(oracle)
    ms = clutter_ctx.place_coverage_refine_burst(inst["poses"], inst["fan"], [0, 1, 2, 3], 1,
                                                 cover_ref.SEP, inst["rois"]["xpos"], reps=2)
    assert len(ms) == 2 and all(np.isfinite(m) and m > 0.0 for m in ms)
    p5 = scan_ref.CLUTTER_POSES
    z = np.zeros(p5.shape[0])
    ms = clutter_ctx.place_coverage_refine_mounted_burst(
        np.column_stack([p5[:, :3], z, z, p5[:, 4]]), _abi.fan_params(n_az=100, n_el=5), [0, 1],
        TABLE, reps=2)
    assert len(ms) == 2 and all(np.isfinite(m) and m > 0.0 for m in ms)
    # the timing entry commits nothing a later call could see
    cover_refine_ref.assert_refine_equal(
        _call(clutter_ctx, oracle, "all", cover_ref.SEP, [0, 1, 2, 3]),
        cover_refine_ref.grid_case(oracle, "all", cover_ref.SEP, 4, "first", 0, 16))
