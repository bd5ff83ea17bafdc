"""pcp_place_aimed (greedy placement of limited-field-of-view sensors: where to stand and which
way to look) on the GPU, against tests/aim_ref.py:
  (a) bit for bit on ctx.score_matrix's own output for the pitch-zeroed poses;
  (b) on the oracle's matrix for the device's candidates: selections, aims, counts and owners
      equal, totals under tests/parity.py's bar, every recorded round decided by more than 0.1;
  (c) its reductions to pcp_place_sensors; (d) the smallest shapes around the kernel's seams (a
      chunk is 64 cells, a wave holds 64 aims, a block one pose); (e) synthetic geometry at the
      predicate's edges; (f) the contract (refusals, empty inputs, determinism, isolation)."""
import ctypes as C
import math

import aim_ref
import numpy as np
import parity
import pytest

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
FOVS = [(90, 60), (120, 40), (70, 77)]
GAP = 0.1   # best minus runner-up of every recorded round of (b), oracle side


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _flat(poses):
    out = np.array(poses, np.float64).reshape(-1, 5)
    out[:, 3] = 0.0
    return out


def grid_aims(n):
    """n <= 64 distinct aims, pitch-major: pitches (-60, -40, -20, 0) x 16 yaw offsets."""
    return np.array([[o * DEG, p * DEG] for p in (-60.0, -40.0, -20.0, 0.0)
                     for o in np.arange(-180.0, 180.0, 22.5)], np.float64)[:n]


@pytest.fixture(scope="module")
def tick(oracle, scene, cells, aux):
    """One context with the scene loaded, the tick's 91 candidates and the oracle's matrix of the
    pitch-zeroed candidates."""
    params = _abi.default_vl_params()
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = np.ascontiguousarray(
            ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5))
        assert poses.shape == (91, 5) and cells.xyz.shape[0] == 3704
        T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
        o_S, o_Z = oracle.score_matrix(T, A, cells.xyz, cells.normals, _flat(poses),
                                       scene.zx120_pose5, oracle.vl_params())
        yield {"ctx": ctx, "poses": poses, "params": params, "S": o_S, "Z": o_Z,
               "zx": scene.zx120_pose5, "cells": cells}


def _exact(got, ref):
    """(a): everything the call returns against the restatement on the same matrix."""
    assert got["n_selected"] == ref["n_selected"]
    np.testing.assert_array_equal(got["selected"], ref["selected"])
    np.testing.assert_array_equal(got["selected_aim"], ref["selected_aim"])
    np.testing.assert_array_equal(got["covered_after"], ref["covered_after"])
    np.testing.assert_array_equal(_bits(got["total_after"]), _bits(ref["total_after"]))
    assert got["round_totals"].shape == ref["round_totals"].shape
    np.testing.assert_array_equal(np.isneginf(got["round_totals"]),
                                  np.isneginf(ref["round_totals"]))
    np.testing.assert_array_equal(_bits(got["round_totals"]), _bits(ref["round_totals"]))
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(ref["cell_score"]))
    np.testing.assert_array_equal(got["cell_owner"], ref["cell_owner"])
    assert _bits(got["base_total"])[0] == _bits(ref["base_total"])[0]
    assert got["base_covered"] == ref["base_covered"]


def _case(tick, pose_idx, Cn, aims, h, v, k_max, fixed=(), sep=0.0, set_cells=True, cidx=None):
    """place_aimed over poses[pose_idx] and cells[:Cn] (or cells[cidx]), checked (a); returns
    (device result, restatement, the poses, the view)."""
    ctx, cells = tick["ctx"], tick["cells"]
    poses = np.ascontiguousarray(tick["poses"][pose_idx])
    cidx = np.arange(Cn) if cidx is None else np.asarray(cidx)
    xyz = np.ascontiguousarray(cells.xyz[cidx])
    if set_cells:
        ctx.set_cells(xyz, np.ascontiguousarray(cells.normals[cidx]))
    got = ctx.place_aimed(poses, tick["zx"], tick["params"], aims, h, v, k_max, fixed, sep,
                          want_round_totals=True, want_cells=True)
    d_S, d_Z = ctx.score_matrix(_flat(poses), tick["zx"], tick["params"])
    assert d_S.shape == (poses.shape[0], cidx.size)
    view = aim_ref.in_view(_flat(poses), xyz, aims, h, v)
    ref = aim_ref.place_aimed(d_S, d_Z, _flat(poses), xyz, aims, h, v, k_max, fixed, sep,
                              view=view)
    _exact(got, ref)
    return got, ref, poses, view


def _oracle_side(tick, got, poses, view, aims, h, v, k_max, fixed=(), sep=0.0, gap=GAP):
    """(b): the restatement on the oracle's matrix (the full tick's poses and cells)."""
    orc = aim_ref.place_aimed(tick["S"], tick["Z"], _flat(poses), tick["cells"].xyz, aims, h, v,
                              k_max, fixed, sep, view=view)
    gaps = aim_ref.runner_up_gaps(orc)
    print(f"{h / DEG:.0f} x {v / DEG:.0f}: gaps {gaps}")
    assert gap is None or all(g > gap for g in gaps), gaps
    assert got["n_selected"] == orc["n_selected"]
    np.testing.assert_array_equal(got["selected"], orc["selected"])
    np.testing.assert_array_equal(got["selected_aim"], orc["selected_aim"])
    np.testing.assert_array_equal(got["covered_after"], orc["covered_after"])
    np.testing.assert_array_equal(got["cell_owner"], orc["cell_owner"])
    assert got["base_covered"] == orc["base_covered"]
    parity.assert_totals_exact(got["base_total"], orc["base_total"])
    for r in range(got["n_selected"]):
        a, o = got["round_totals"][r], orc["round_totals"][r]
        np.testing.assert_array_equal(np.isfinite(a), np.isfinite(o))
        print(f"round {r}:", parity.totals_report(a[np.isfinite(o)], o[np.isfinite(o)]))
        parity.assert_totals(a[np.isfinite(o)], o[np.isfinite(o)])
    parity.assert_totals(got["total_after"], orc["total_after"])
    return orc


# ---- (a) + (b): the full tick --------------------------------------------------------------

EXPECT = {(90, 60): [(32, 8), (40, 6), (33, 7)], (120, 40): [(40, 7), (48, 8), (49, 7)],
          (70, 77): [(32, 8), (56, 8), (33, 6)]}


@pytest.mark.parametrize("hv", FOVS)
def test_full_tick(tick, hv):
    """P = 91, A = 45, C = 3,704, three sensors: the answer the call was specified with."""
    h, v = hv[0] * DEG, hv[1] * DEG
    aims = aim_ref.tick_aims()
    got, ref, poses, view = _case(tick, slice(None), 3704, aims, h, v, 3)
    orc = _oracle_side(tick, got, poses, view, aims, h, v, 3)
    assert list(zip(orc["selected"].tolist(), orc["selected_aim"].tolist())) == EXPECT[hv]
    assert list(zip(got["selected"].tolist(), got["selected_aim"].tolist())) == EXPECT[hv]
    if hv == (90, 60):
        assert got["covered_after"].tolist() == [2679, 2986, 3243]
    assert np.all(np.diff(np.concatenate([[got["base_total"]], got["total_after"]])) > 0)


# ---- (c) reductions --------------------------------------------------------------------------


def test_whole_sphere_single_aim_is_place_sensors(tick):
    """h_fov = 2 pi, v_fov = pi, one aim (0, 0): pcp_place_sensors on the same poses, byte for
    byte (on this tick the pitch-zeroed matrix has the original's bits)."""
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    for sep, k in ((0.0, 8), (2.0, 16)):
        got = ctx.place_aimed(poses, zx, params, [[0.0, 0.0]], 2 * math.pi, math.pi, k,
                              min_separation=sep, want_round_totals=True, want_cells=True)
        ps = ctx.place_sensors(poses, zx, params, k, sep, want_round_totals=True,
                               want_cells=True)
        assert got["n_selected"] == ps["n_selected"] == k
        np.testing.assert_array_equal(got["selected"], ps["selected"])
        assert not got["selected_aim"].any()
        assert got["total_after"].tobytes() == ps["total_after"].tobytes()
        assert got["covered_after"].tobytes() == ps["covered_after"].tobytes()
        assert got["round_totals"][:, :, 0].tobytes() == ps["round_totals"].tobytes()
        assert got["cell_score"].tobytes() == ps["cell_score"].tobytes()
        assert got["cell_owner"].tobytes() == ps["cell_owner"].tobytes()
        assert _bits(got["base_total"])[0] == _bits(ps["zx120_total"])[0]
        assert got["base_covered"] == ps["zx120_covered"]


def test_identical_aims_select_aim_zero(tick):
    """45 copies of one aim: every row of a pose ties, the first maximum is aim 0."""
    aims = np.tile([[0.3, -25 * DEG]], (45, 1))
    got, ref, _, _ = _case(tick, slice(None), 3704, aims, 90 * DEG, 60 * DEG, 3)
    assert got["n_selected"] == 3 and not got["selected_aim"].any()
    for t in got["round_totals"]:
        assert np.all(_bits(t) == _bits(t[:, :1]))


# ---- (d) the seams ---------------------------------------------------------------------------


def seam_inputs(tick, Cn, Pn, An):
    """Poses, cells and aims at which every shape places a sensor, so that each shape's [P][A]
    table of row totals is compared: poses 32 and 40 first, the Cn cells that both of them raise
    most over zx120 (oracle side, in cell order), and as aim 0 the direction from pose 32 to those
    cells' centroid, the grid of aims behind it."""
    S, Z, xyz = tick["S"], tick["Z"], tick["cells"].xyz
    pidx = np.array(([32, 40] + [p for p in range(91) if p not in (32, 40)])[:Pn])
    gain = np.minimum(S[32], S[40]) - Z
    cidx = np.sort(np.argsort(-gain, kind="stable")[:Cn])
    q = tick["poses"][32]
    d = xyz[cidx].mean(axis=0) - q[:3]
    aim0 = [math.atan2(d[1], d[0]) - q[4], math.atan2(d[2], math.hypot(d[0], d[1]))]
    return pidx, cidx, np.concatenate([[aim0], grid_aims(63)])[:An]


@pytest.mark.parametrize("Cn", [1, 63, 64, 65, 129])
def test_shapes(tick, Cn):
    """Cells around the staged chunk (64) x aims around the walking wave (64 lanes, seven staging
    waves) x poses (a block each) from one to the tick's 91.  Every shape records at least one
    round, so its whole table of row totals, -inf pattern included, is compared bit for bit."""
    first = True
    for Pn in (1, 2, 17, 91):
        for An in (1, 2, 63, 64):
            pidx, cidx, aims = seam_inputs(tick, Cn, Pn, An)
            got, ref, _, _ = _case(tick, pidx, Cn, aims, 100 * DEG, 50 * DEG, 4, set_cells=first,
                                   cidx=cidx)
            first = False
            assert ref["n_selected"] >= 1 and got["n_selected"] >= 1, (Cn, Pn, An)
            assert got["round_totals"].shape == (got["n_selected"], Pn, An)
            assert np.isfinite(got["round_totals"][0]).all() and (got["round_totals"][0] > 0).any()


def test_fewer_alive_poses_than_rounds(tick):
    """k_max = 16 over five poses: the search ends when the poses are exhausted or add nothing."""
    got, ref, _, _ = _case(tick, [40, 32, 33, 48, 3], 3704, aim_ref.tick_aims(), 90 * DEG,
                           60 * DEG, 16)
    assert 1 <= got["n_selected"] <= 5 and len(set(got["selected"].tolist())) == got["n_selected"]


@pytest.mark.parametrize("sep", [2.0, 5.0])
def test_separation(tick, sep):
    got, ref, poses, _ = _case(tick, slice(None), 3704, aim_ref.tick_aims(), 90 * DEG, 60 * DEG,
                               8, sep=sep)
    xy = poses[got["selected"], :2]
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    assert got["n_selected"] >= 2 and np.all(d[~np.eye(len(xy), dtype=bool)] >= sep - 1e-9)
    dead = np.isneginf(got["round_totals"][-1]).all(axis=1)
    assert dead[got["selected"][:-1]].all()


@pytest.mark.parametrize("fixed", [[(32, 8)], [(40, 6), (32, 8), (33, 7)]])
def test_fixed_sensors(tick, fixed):
    """One and three aimed sensors already placed: they own what they raise, their poses (and,
    under a separation, their neighbours) are out of the search."""
    for sep in (0.0, 2.0):
        got, ref, _, _ = _case(tick, slice(None), 3704, aim_ref.tick_aims(), 90 * DEG, 60 * DEG, 3,
                               fixed=fixed, sep=sep)
        assert got["n_selected"] == 3 and got["cell_owner"].max() == len(fixed) + 2
        for p, _ in fixed:
            assert np.isneginf(got["round_totals"][:, p, :]).all()
            assert p not in got["selected"].tolist()
        assert got["base_total"] > 1715.36   # (zx120 alone totals 1715.354...)


def test_fixed_sensor_that_sees_nothing(tick):
    """A fixed sensor looking straight up (pitch 90 degrees, 10 degrees of band): it owns nothing
    and the base stays zx120's, yet its pose is out of the search."""
    aims = np.concatenate([aim_ref.tick_aims(), [[0.0, math.pi / 2]]])
    got, ref, _, view = _case(tick, slice(None), 3704, aims, 90 * DEG, 10 * DEG, 2,
                              fixed=[(40, 45)])
    assert not view[40, 45].any()
    assert abs(got["base_total"] - 1715.3544346588476) < 1e-6   # zx120 alone
    assert not (got["cell_owner"] == 0).any()
    assert np.isneginf(got["round_totals"][:, 40, :]).all()


# ---- (e) synthetic geometry ----------------------------------------------------------------


@pytest.fixture(scope="module")
def bare():
    """A fresh context without terrain or zx120 cloud: every in-range cell is visible.  One pose
    at the origin, 1 m up, looking along +x; cells on rings of 3 m at every 15 degrees and three
    heights, straight below and above, and on the sector's and the band's edges."""
    ring = []
    for k in range(24):
        a = k * 15 * DEG
        for z in (-2.0, 1.0, 4.0):     # dz = -3, 0, 3 = -hyp, 0, hyp
            ring.append([3 * math.cos(a), 3 * math.sin(a), z])
    exact = [[0.0, 0.0, 0.0], [0.0, 0.0, 2.5],             # straight below / above (hyp = 0)
             [2.0, 2.0, 1.0], [2.0, -2.0, 1.0],            # 45 degrees off the heading, exactly
             [2.0, 2.0, 3.0], [3.0, 0.0, 4.0], [3.0, 0.0, -2.0],   # dz = +-hyp (and a corner)
             [-3.0, 0.0, 1.0], [-2.0, 0.0, 0.0],           # exactly behind
             [4.0, 0.5, 0.5], [-4.0, 0.5, 0.5]]            # well inside / well outside
    xyz = np.array(ring + exact, np.float64)
    nrm = np.tile([0.0, 0.0, 1.0], (xyz.shape[0], 1)).astype(np.float32)
    poses = np.array([[0.0, 0.0, 1.0, 0.4, 0.0]])
    zx = np.array([500.0, 500.0, 1.0, 0.0, 0.0])   # out of range of every cell: Z = 0
    with _abi.Context(0) as ctx:
        ctx.set_cells(xyz, nrm)
        yield {"ctx": ctx, "xyz": xyz, "poses": poses, "zx": zx,
               "params": _abi.default_vl_params()}


def _bare_case(bare, poses, aims, h, v, k_max=1):
    ctx = bare["ctx"]
    got = ctx.place_aimed(poses, bare["zx"], bare["params"], aims, h, v, k_max,
                          want_round_totals=True, want_cells=True)
    S, Z = ctx.score_matrix(_flat(poses), bare["zx"], bare["params"])
    assert not Z.any() and (S > 0).all()   # every cell in range and visible
    view = aim_ref.in_view(_flat(poses), bare["xyz"], aims, h, v)
    ref = aim_ref.place_aimed(S, Z, _flat(poses), bare["xyz"], aims, h, v, k_max, view=view)
    _exact(got, ref)
    assert ref["n_selected"] >= 1   # a round is recorded: the row totals are compared
    return got, view


EDGE_CASES = [
    # h, v, aims: the lower bound at exactly -90 degrees and above it (the cell straight below)
    (math.pi / 2, math.pi / 2, [[0.0, -math.pi / 4]]),
    (math.pi / 2, math.pi / 2, [[0.0, -math.pi / 4 + 1e-9], [0.0, -0.5]]),
    # the band's bounds at dz = +-hyp and at dz = 0; the sector's edge at 45 degrees
    (math.pi / 2, math.pi / 2, [[0.0, 0.0], [0.0, math.pi / 4], [math.pi / 4, 0.0],
                                [-math.pi / 4, math.pi / 4], [math.pi, 0.0]]),
    # the cell exactly behind the aim, h_fov just under 2 pi and at it
    (float(np.nextafter(2 * math.pi, 0.0)), math.pi, [[0.0, 0.0], [1.0, 0.0]]),
    (6.2, 1.0, [[0.0, 0.0], [math.pi, 0.0]]),
    (2 * math.pi, math.pi, [[0.0, 0.0], [1.0, 0.3]]),
    (2 * math.pi, 1.0, [[0.0, 0.0], [1.0, -0.5], [1.0, 0.5]]),
]


@pytest.mark.parametrize("h,v,aims", EDGE_CASES)
def test_edges_bit_for_bit(bare, h, v, aims):
    _bare_case(bare, bare["poses"], np.array(aims, np.float64), h, v)


def test_edges_intent(bare):
    """Cells well inside and well outside, and the cell straight below, against intent."""
    xyz = bare["xyz"]
    n = xyz.shape[0]
    below, inside, outside = n - 11, n - 2, n - 1
    got, view = _bare_case(bare, bare["poses"], np.array([[0.0, -math.pi / 4]]), math.pi / 2,
                           math.pi / 2)
    assert got["selected"].tolist() == [0] and got["selected_aim"].tolist() == [0]
    own = got["cell_owner"]
    assert own[inside] == 0 and own[outside] == _abi.OWNER_NONE
    assert own[below] == 0                       # lo = -90 degrees: straight below is in view
    assert view[0, 0, below] and not view[0, 0, below + 1]   # straight above is not
    got, view = _bare_case(bare, bare["poses"], np.array([[0.0, -0.5]]), math.pi / 2, math.pi / 2)
    assert got["cell_owner"][below] == _abi.OWNER_NONE and got["cell_owner"][inside] == 0
    # turned round: the cells swap
    got, _ = _bare_case(bare, bare["poses"], np.array([[math.pi, 0.0]]), math.pi / 2, math.pi / 2)
    assert got["cell_owner"][inside] == _abi.OWNER_NONE and got["cell_owner"][outside] == 0
    # the whole sphere (the band of pi about pitch 0 reaches both verticals): everything
    got, _ = _bare_case(bare, bare["poses"], np.array([[0.3, 0.0]]), 2 * math.pi, math.pi)
    assert (got["cell_owner"] == 0).all() and got["covered_after"].tolist() == [n]


def test_nan_yaw_sees_nothing(bare):
    """A pose with a NaN yaw: every row of it is out of view, so it totals the base and is never
    placed; the pose beside it is."""
    poses = np.array([[0.0, 0.0, 1.0, 0.0, math.nan], [0.0, 0.0, 1.0, 0.0, 0.0]])
    aims = np.array([[0.0, 0.0], [1.0, -0.3]])
    got, view = _bare_case(bare, poses, aims, math.pi / 2, math.pi / 2, k_max=2)
    assert not view[0].any() and view[1].any()
    assert got["selected"].tolist() == [1]
    assert (got["round_totals"][0][0] == 0.0).all()


# ---- (f) the contract ------------------------------------------------------------------------


def _raw_call(ctx, poses, zx, params, ap, aims, null=()):
    """The C call with every output preset to a sentinel: (rc, outputs)."""
    P = poses.shape[0]
    out = {"sel": np.full(16, -7, np.int64), "sa": np.full(16, -7, np.int32),
           "tot": np.full(16, -7.0), "cov": np.full(16, -7, np.int32),
           "rt": np.full(16 * max(P, 1) * 64, -7.0), "cs": np.full(4096, -7.0),
           "co": np.full(4096, -7, np.int32), "bt": np.full(1, -7.0),
           "bc": np.full(1, -7, np.int32), "ns": np.full(1, -7, np.int32)}
    ptr = {k: (None if k in null else _abi._ptr(a)) for k, a in out.items()}
    rc = ctx.lib.pcp_place_aimed(
        ctx.h, None if "poses" in null else _abi._ptr(poses), P,
        None if "zx" in null else _abi._ptr(zx), None if "params" in null else C.byref(params),
        None if "ap" in null else C.byref(ap), None if "aims" in null else _abi._ptr(aims),
        ptr["sel"], ptr["sa"], ptr["tot"], ptr["cov"], ptr["rt"], ptr["cs"], ptr["co"],
        ptr["bt"], ptr["bc"], ptr["ns"])
    return rc, out


def test_refusals_write_nothing(tick):
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, params = np.ascontiguousarray(tick["poses"]), tick["params"]
    zx = np.ascontiguousarray(tick["zx"], np.float64)
    aims = np.ascontiguousarray(grid_aims(4))
    mk = _abi.Context._aim_params
    H, V = 1.5, 1.0
    bad_aims = {"nan": [[math.nan, 0.0]] * 4, "inf": [[0.0, 0.0], [math.inf, 0.0]] * 2,
                "steep": [[0.0, 0.0], [0.0, 1.5708]] * 2, "pitch_nan": [[0.0, math.nan]] * 4}
    cases = [(mk(0, 4, H, V, (), 0.0, 0), aims, poses, ()),
             (mk(_abi.PLACE_MAX + 1, 4, H, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 0, H, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, _abi.AIM_MAX + 1, H, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, (), 0.0, 0, n_fixed=-1), aims, poses, ()),
             (mk(2, 4, H, V, (), 0.0, 0, n_fixed=_abi.PLACE_MAX + 1), aims, poses, ()),
             (mk(2, 4, H, V, (), 0.0, 1), aims, poses, ()),
             (mk(2, 4, 0.0, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, -1.0, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, math.inf, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, math.nan, V, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, 0.0, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, float(np.nextafter(math.pi, 4.0)), (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, math.nan, (), 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, [(91, 0)], 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, [(-1, 0)], 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, [(5, 0), (6, 1), (5, 2)], 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, [(5, 4)], 0.0, 0), aims, poses, ()),
             (mk(2, 4, H, V, [(5, -1)], 0.0, 0), aims, poses, ()),
             (mk(2, 64, H, V, (), 0.0, 0), np.ascontiguousarray(grid_aims(64)),
              np.ascontiguousarray(np.tile(poses, (12, 1))[:1025]), ()),       # 65,600 rows
             (mk(2, 4, H, V, (), 0.0, 0), aims,
              np.ascontiguousarray(np.tile(poses, (23, 1))[:_abi.PAIR_MAX_POSES + 1]), ())]
    cases += [(mk(2, 4, H, V, (), 0.0, 0), np.array(a, np.float64), poses, ())
              for a in bad_aims.values()]
    good = mk(2, 4, H, V, (), 0.0, 0)
    cases += [(good, aims, poses, (k,)) for k in ("poses", "zx", "params", "ap", "aims", "sel",
                                                  "sa", "tot", "cov", "bt", "bc", "ns")]
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for i, (ap, am, ps, null) in enumerate(cases):
            rc, out = _raw_call(ctx, ps, zx, params, ap, np.ascontiguousarray(am), null)
            assert rc == _abi.PCP_E_INVALID, i
            for k, a in out.items():
                assert (a == -7).all(), (i, k)
        far = _abi.default_vl_params(max_distance=0.5 + 0.3 * (_abi.MAX_STEPS + 2))
        rc, out = _raw_call(ctx, poses, zx, far, good, aims)
        assert rc == _abi.PCP_E_INVALID and all((a == -7).all() for a in out.values())
        for k in ("score_cells", "pose_sum", "place_sensors"):   # nothing was launched
            assert ctx.profile_get(k)[1] == 0
        # the rounds are what PCP_K_PLACE times: one launch each
        rc, out = _raw_call(ctx, poses, zx, params, good, aims, null=("rt", "cs", "co"))
        assert rc == _abi.PCP_OK and out["ns"][0] == 2
        assert ctx.profile_get("place_sensors")[1] == 2
    finally:
        ctx.profile(False)


def test_empty_inputs(tick):
    ctx, cells = tick["ctx"], tick["cells"]
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    aims = grid_aims(3)
    # no cells: nothing to place
    ctx.set_cells(cells.xyz[:0], cells.normals[:0])
    got = ctx.place_aimed(poses, zx, params, aims, 1.5, 1.0, 4, want_round_totals=True,
                          want_cells=True)
    assert got["n_selected"] == 0 and got["selected"].size == 0
    assert got["base_total"] == 0.0 and got["base_covered"] == 0
    # no poses: the zx120 sensor alone
    ctx.set_cells(cells.xyz, cells.normals)
    got = ctx.place_aimed(poses[:0], zx, params, aims, 1.5, 1.0, 4, want_round_totals=True,
                          want_cells=True)
    assert got["n_selected"] == 0 and got["round_totals"].shape == (0, 0, 3)
    d_S, d_Z = ctx.score_matrix(poses[:1], zx, params)
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(d_Z))
    assert _bits(got["base_total"])[0] == _bits(np.cumsum(d_Z)[-1])[0]
    assert got["base_covered"] == int((d_Z > 0).sum())
    np.testing.assert_array_equal(
        got["cell_owner"], np.where(d_Z > 0, _abi.OWNER_ZX120, _abi.OWNER_NONE))


def test_determinism_and_isolation(tick):
    """Two calls give identical bytes; pcp_score_poses before and after is unchanged, the caller's
    flags are not touched, the scratch allocations settle after the first call."""
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    aims = aim_ref.tick_aims()
    f0 = np.zeros(3704, np.uint8)
    t0, c0, r0 = ctx.score_poses(poses, zx, params, f0)
    held = f0.copy()
    kw = dict(fixed=[(40, 6)], min_separation=2.0, want_round_totals=True, want_cells=True)
    first = ctx.place_aimed(poses, zx, params, aims, 90 * DEG, 60 * DEG, 8, **kw)
    np.testing.assert_array_equal(f0, held)
    settled = _abi.alloc_stats()
    again = ctx.place_aimed(poses, zx, params, aims, 90 * DEG, 60 * DEG, 8, **kw)
    assert _abi.alloc_stats() == settled
    assert first["n_selected"] >= 3
    for k in first:
        assert np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    f1 = np.zeros(3704, np.uint8)
    t1, c1, r1 = ctx.score_poses(poses, zx, params, f1)
    np.testing.assert_array_equal(_bits(t0), _bits(t1))
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(f0, f1)
    assert r0.as_dict() == r1.as_dict()
    assert _abi.alloc_stats() == settled
    # the timing entry commits nothing: the same answer after it
    ms = ctx.place_aimed_burst(poses, zx, params, aims, 90 * DEG, 60 * DEG, reps=2)
    assert ms > 0
    third = ctx.place_aimed(poses, zx, params, aims, 90 * DEG, 60 * DEG, 8, **kw)
    for k in first:
        assert np.asarray(first[k]).tobytes() == np.asarray(third[k]).tobytes(), k
