"""pcp_place_sensors (greedy multi-sensor pose selection) on the 91-candidate tick.

Every case is checked twice:
  (a) exactly, against the NumPy restatement below run on ctx.score_matrix's own output for the
      same arguments (this isolates the placement kernels: the matrix has its own oracle test);
  (b) against the same restatement run on the oracle's matrix: selections, counts and owners
      equal, round 0's totals and the zx120 total under the exact bar, the later rounds' totals
      under the loose bar (the device matrix differs from glibc's in 0.16 % of the cells by <= 4
      ulps on this tick, tests/parity.py; the smallest best-minus-runner-up margin or gain of a
      recorded round is 0.0178 at totals of about 4e3 -- asserted per case, MARGIN -- so such a
      difference cannot change a selection).
The oracle's matrix is computed once for the whole tick; cell / pose prefixes are slices of it."""
import subprocess
from pathlib import Path

import numpy as np
import parity
import pytest

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "pointcloud_processor_amd" / "_lib" / "pcp_nodes_cli"


def greedy(S, Z, xy, k_max, sep=0.0):
    """The definition of pcp_place_sensors (include/pcp_abi.h), restated: S [P, C], Z [C] as
    pcp_score_matrix returns them, xy [P, 2] the poses' x, y."""
    S = np.asarray(S, np.float64)
    Z = np.asarray(Z, np.float64)
    P, C = S.shape

    def osum(V):   # rows of V: ordered sum from +0.0 of the positive elements, and their count
        V = np.atleast_2d(V)
        pos = V > 0
        if V.shape[1] == 0:
            return np.zeros(V.shape[0]), np.zeros(V.shape[0], np.int32)
        # (adding +0.0 to a non-negative running sum leaves its bits: cumsum is sequential)
        return np.cumsum(np.where(pos, V, 0.0), axis=1)[:, -1], pos.sum(axis=1).astype(np.int32)

    base = Z.copy()
    t0, c0 = osum(base)
    T = float(t0[0])
    out = {"zx120_total": T, "zx120_covered": int(c0[0]), "selected": [], "total_after": [],
           "covered_after": [], "round_totals": []}
    owner = np.where(Z > 0, _abi.OWNER_ZX120, _abi.OWNER_NONE).astype(np.int32)
    alive = np.ones(P, bool)
    for r in range(k_max):
        if not alive.any():
            break
        t, cov = osum(np.where(base[None, :] < S, S, base[None, :]))   # std::max(base, S)
        t = np.where(alive, t, -np.inf)
        b = int(np.argmax(t))   # the first maximum
        if not t[b] > T:
            break
        out["round_totals"].append(t)
        out["selected"].append(b)
        out["total_after"].append(float(t[b]))
        out["covered_after"].append(int(cov[b]))
        T = float(t[b])
        take = base < S[b]
        owner[take] = r
        base[take] = S[b][take]
        alive[b] = False
        if sep > 0:
            dx, dy = xy[:, 0] - xy[b, 0], xy[:, 1] - xy[b, 1]
            alive &= ~(dx * dx + dy * dy < sep * sep)
    n = len(out["selected"])
    out["n_selected"] = n
    out["selected"] = np.array(out["selected"], np.int64)
    out["total_after"] = np.array(out["total_after"], np.float64)
    out["covered_after"] = np.array(out["covered_after"], np.int32)
    out["round_totals"] = np.array(out["round_totals"], np.float64).reshape(n, P)
    out["cell_score"] = base
    out["cell_owner"] = owner
    return out


MARGIN = 0.017   # best minus runner-up, and the gain, of every recorded round (oracle side)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def tick(oracle, scene, cells, aux):
    """One context with the scene loaded, the tick's 91 candidates and the oracle's matrix."""
    params = _abi.default_vl_params()
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = np.ascontiguousarray(
            ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5))
        assert poses.shape == (91, 5) and cells.xyz.shape[0] == 3704
        T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
        o_S, o_Z = oracle.score_matrix(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                                       oracle.vl_params())
        yield {"ctx": ctx, "poses": poses, "params": params, "S": o_S, "Z": o_Z,
               "zx": scene.zx120_pose5, "cells": cells}
        ctx.set_cells(cells.xyz, cells.normals)


def _case(tick, pose_idx, Cn, k_max, sep=0.0, margins=True):
    """place_sensors over poses[pose_idx] and cells[:Cn], checked (a) and (b); returns (device
    result, oracle-side restatement).  margins: every recorded round's choice and gain are
    decided by more than MARGIN on the oracle side (off where poses are exact copies)."""
    ctx, cells = tick["ctx"], tick["cells"]
    poses = np.ascontiguousarray(tick["poses"][pose_idx])
    ctx.set_cells(cells.xyz[:Cn], cells.normals[:Cn])
    got = ctx.place_sensors(poses, tick["zx"], tick["params"], k_max, sep,
                            want_round_totals=True, want_cells=True)
    d_S, d_Z = ctx.score_matrix(poses, tick["zx"], tick["params"])
    assert d_S.shape == (poses.shape[0], Cn)
    # (a) exact, on the device's own matrix
    ref = greedy(d_S, d_Z, poses[:, :2], k_max, sep)
    assert got["n_selected"] == ref["n_selected"]
    np.testing.assert_array_equal(got["selected"], ref["selected"])
    np.testing.assert_array_equal(got["covered_after"], ref["covered_after"])
    np.testing.assert_array_equal(_bits(got["total_after"]), _bits(ref["total_after"]))
    assert got["round_totals"].shape == ref["round_totals"].shape
    np.testing.assert_array_equal(_bits(got["round_totals"]), _bits(ref["round_totals"]))
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(ref["cell_score"]))
    np.testing.assert_array_equal(got["cell_owner"], ref["cell_owner"])
    assert _bits(got["zx120_total"])[0] == _bits(ref["zx120_total"])[0]
    assert got["zx120_covered"] == ref["zx120_covered"]
    # (b) the oracle's matrix
    orc = greedy(tick["S"][pose_idx][:, :Cn], tick["Z"][:Cn], poses[:, :2], k_max, sep)
    assert got["n_selected"] == orc["n_selected"]
    np.testing.assert_array_equal(got["selected"], orc["selected"])
    np.testing.assert_array_equal(got["covered_after"], orc["covered_after"])
    np.testing.assert_array_equal(got["cell_owner"], orc["cell_owner"])
    parity.assert_totals_exact(got["zx120_total"], orc["zx120_total"])
    before = orc["zx120_total"]
    for r in range(orc["n_selected"] if margins else 0):   # no choice hangs on a few ulps
        t = np.sort(orc["round_totals"][r])[::-1]
        assert min(t[0] - before, t[0] - t[1] if t.size > 1 and np.isfinite(t[1]) else np.inf) \
            > MARGIN, (r, t[:2], before)
        before = t[0]
    for r in range(got["n_selected"]):
        a = got["round_totals"][r]
        live = np.isfinite(orc["round_totals"][r])
        np.testing.assert_array_equal(np.isfinite(a), live)
        print(f"C={Cn} P={poses.shape[0]} round {r}:",
              parity.totals_report(a[live], orc["round_totals"][r][live]))
        if r == 0:
            parity.assert_totals_exact(a[live], orc["round_totals"][r][live])
        else:
            parity.assert_totals(a[live], orc["round_totals"][r][live])
    parity.assert_totals(got["total_after"], orc["total_after"])
    return got, orc


def test_full_tick(tick):
    """P = 91, C = 3,704 (the ordinary scoring kernel), eight sensors, no separation."""
    got, orc = _case(tick, slice(None), 3704, 8)
    assert orc["n_selected"] == 8 and len(set(orc["selected"].tolist())) == 8
    # round 0 is pcp_score_poses' question
    ctx = tick["ctx"]
    flags = np.zeros(3704, np.uint8)
    tot, cov, rep = ctx.score_poses(tick["poses"], tick["zx"], tick["params"], flags)
    np.testing.assert_array_equal(_bits(got["round_totals"][0]), _bits(tot))
    assert got["selected"][0] == rep.best_idx
    assert got["covered_after"][0] == cov[rep.best_idx]
    assert _bits(got["zx120_total"])[0] == _bits(rep.zx120_total_score)[0]
    assert np.all(np.diff(np.concatenate([[got["zx120_total"]], got["total_after"]])) > 0)
    assert np.all(np.diff(np.concatenate([[got["zx120_covered"]], got["covered_after"]])) >= 0)


def _expected_rounds(Cn, Pn):
    """The oracle-side outcome of the prefix cases at k_max = 4 (computed on the CPU with the
    oracle's matrix): the chunk is 384 cells, a block holds four poses."""
    if Cn == 1:
        return 1 if Pn == 91 else 0  # one cell: only pose 32 of the 91 sees it better than zx120
    if Pn == 1:
        return 0 if Cn == 191 else 1   # pose 0 adds nothing to the first 191 cells; past them it
                                       # is placed, then the poses are exhausted
    if Cn == 191 and Pn == 5:
        return 2                     # then no gain
    return 4


@pytest.mark.parametrize("Pn", [1, 5, 91])
@pytest.mark.parametrize("Cn", [1, 191, 384, 385, 1153])
def test_prefixes(tick, Cn, Pn):
    """Cell prefixes around the chunk (384) and ring (3 x 384) sizes x pose prefixes below / past
    a block's four rows.  P = 5 with these C runs the wide-lane scoring kernel ((P + 1) C <=
    32,768), P = 91 at C = 1,153 the ordinary one: both feed the rounds."""
    got, orc = _case(tick, slice(0, Pn), Cn, 4)
    assert orc["n_selected"] == _expected_rounds(Cn, Pn)


@pytest.mark.parametrize("sep,k_max,rounds", [(2.0, 16, 16), (5.0, 8, 5)])
def test_separation(tick, sep, k_max, rounds):
    got, orc = _case(tick, slice(None), 3704, k_max, sep)
    assert orc["n_selected"] == rounds
    xy = tick["poses"][got["selected"], :2]
    d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
    assert np.all(d[~np.eye(len(xy), dtype=bool)] >= sep - 1e-9)
    if sep == 5.0:   # the search ends with every pose placed or too close: pose 0 is the last
        assert orc["selected"][-1] == 0
        assert not np.isfinite(got["round_totals"][-1]).all()


def test_duplicates_and_ties(tick):
    """Three copies of the best pose and one other: the tie goes to the lowest index, the other
    copies add nothing, and the search stops on no gain with the copies still alive."""
    got, orc = _case(tick, [40, 40, 40, 3], 3704, 4, margins=False)   # (exact ties: same rows)
    assert orc["selected"].tolist() == [0, 3]
    assert got["selected"].tolist() == [0, 3]
    assert got["n_selected"] == 2


def test_ties_across_threads_and_waves(tick):
    """P = 2 x 256 + 3 poses, the tick's 91 candidates repeated: every pose has exact copies 91,
    182, .. later.  A thread of the round's last block then scans up to three poses, and the tied
    maxima sit in different threads and waves of its first-maximum reduction: every round picks
    the lowest index among the tied rows."""
    idx = np.arange(2 * 256 + 3) % 91
    got, orc = _case(tick, idx, 385, 4, margins=False)   # (exact ties: same rows)
    assert orc["n_selected"] == 4 and got["n_selected"] == 4
    assert np.all(got["selected"] < 91)
    for r in range(4):
        t = got["round_totals"][r]
        tied = np.flatnonzero(t == t.max())
        assert tied.size >= 5 and np.all(tied % 91 == tied[0])
        assert got["selected"][r] == tied[0]


def test_isolation(tick):
    """pcp_score_poses before and after a placement on one context: identical; the caller's
    flags are not touched; the scratch allocations settle after the first call."""
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    f0 = np.zeros(3704, np.uint8)
    t0, c0, r0 = ctx.score_poses(poses, zx, params, f0)
    held = f0.copy()
    first = ctx.place_sensors(poses, zx, params, 8, 2.0, want_round_totals=True, want_cells=True)
    np.testing.assert_array_equal(f0, held)
    settled = _abi.alloc_stats()
    again = ctx.place_sensors(poses, zx, params, 8, 2.0, want_round_totals=True, want_cells=True)
    assert _abi.alloc_stats() == settled
    for k in first:
        np.testing.assert_array_equal(first[k], again[k])
    f1 = np.zeros(3704, np.uint8)
    t1, c1, r1 = ctx.score_poses(poses, zx, params, f1)
    np.testing.assert_array_equal(_bits(t0), _bits(t1))
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(f0, f1)
    assert r0.as_dict() == r1.as_dict()
    assert _abi.alloc_stats() == settled


def test_refusals(tick):
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for kw in ({"k_max": 0}, {"k_max": _abi.PLACE_MAX + 1}, {"k_max": 2, "reserved": 1}):
            with pytest.raises(_abi.PcpError) as e:
                ctx.place_sensors(poses, zx, params, **kw)
            assert e.value.code == _abi.PCP_E_INVALID
        far = _abi.default_vl_params(max_distance=0.5 + 0.3 * (_abi.MAX_STEPS + 2))
        with pytest.raises(_abi.PcpError) as e:
            ctx.place_sensors(poses, zx, far, 2)
        assert e.value.code == _abi.PCP_E_INVALID
        for k in ("score_cells", "pose_sum", "place_sensors"):   # nothing was launched
            assert ctx.profile_get(k)[1] == 0
        # the rounds are what PCP_K_PLACE times: one launch each
        ctx.place_sensors(poses, zx, params, 3)
        assert ctx.profile_get("place_sensors")[1] == 3
    finally:
        ctx.profile(False)
    # no cells: nothing to place
    ctx.set_cells(cells.xyz[:0], cells.normals[:0])
    got = ctx.place_sensors(poses, zx, params, 4, want_round_totals=True, want_cells=True)
    assert got["n_selected"] == 0 and got["selected"].size == 0
    assert got["zx120_total"] == 0.0 and got["zx120_covered"] == 0
    # no poses: the zx120 sensor alone
    ctx.set_cells(cells.xyz, cells.normals)
    got = ctx.place_sensors(poses[:0], zx, params, 4, want_cells=True)
    assert got["n_selected"] == 0
    d_S, d_Z = ctx.score_matrix(poses[:1], zx, params)
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(d_Z))


def test_cli_place(tick, tmp_path, scene, cells, aux):
    """pcp_nodes_cli place (MobileLidarPlacement above the node's tick): the binding's answer."""
    import json

    assert CLI.exists(), "build first (__graft_entry__.build())"
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(aux).tofile(tmp_path / "a.f32")
    np.ascontiguousarray(cells.xyz, np.float64).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals, np.float32).tofile(tmp_path / "n.f32")
    t = lambda v: ",".join(repr(float(x)) for x in v)   # noqa: E731
    r = subprocess.run([str(CLI), "place", str(tmp_path / "t.f32"), str(scene.terrain.shape[0]),
                        str(tmp_path / "a.f32"), str(aux.shape[0]), str(tmp_path / "c.f64"),
                        str(tmp_path / "n.f32"), str(cells.xyz.shape[0]), t(cells.grid_bbox),
                        "0,0,0", "100", "15.0", "8", "2.0", str(tmp_path / "sel.i64"),
                        str(tmp_path / "tot.f64"), str(tmp_path / "rep.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    ctx = tick["ctx"]
    ctx.set_cells(cells.xyz, cells.normals)
    got = ctx.place_sensors(tick["poses"], tick["zx"], tick["params"], 8, 2.0)
    assert res["n_candidates"] == 91 and res["n_selected"] == got["n_selected"] == 8
    np.testing.assert_array_equal(np.fromfile(tmp_path / "sel.i64", np.int64), got["selected"])
    np.testing.assert_array_equal(_bits(np.fromfile(tmp_path / "tot.f64", np.float64)),
                                  _bits(got["total_after"]))
    assert _bits(res["zx120_total"])[0] == _bits(got["zx120_total"])[0]
    assert res["zx120_covered"] == got["zx120_covered"] and res["total_cells"] == 3704
    log = (tmp_path / "rep.txt").read_text()
    assert "Multi LiDAR Placement (ZX120 + 8 Mobile)" in log
    assert f"Total Score (ZX120 only): {got['zx120_total']:.2f}" in log
    for i, (s, tot) in enumerate(zip(got["selected"], got["total_after"])):
        p = tick["poses"][s]
        assert f"Mobile LiDAR {i + 1} Position: ({p[0]:.2f}, {p[1]:.2f}, {p[2]:.2f})" in log
        assert f"  Total Score: {tot:.2f} (gain " in log
