"""pcp_place_triple (the exact best triple of mobile sensors) on the 91-candidate tick.

Every case asks for the dense outputs and is checked on up to three sides:
  (a) bit for bit against tests/triple_ref.py run on ctx.score_matrix's own output for the same
      arguments: the whole triple table with its -inf pattern, first_totals / first_partners, the
      three selections, the covered counts, the base values, n_selected, cell_score's bits and
      cell_owner;
  (b) against triple_ref on the oracle's matrix: selections, covered counts and owners equal, the
      totals under parity.assert_totals.  (b) applies where nothing on the oracle side is decided
      by less than GAP (triple_ref.runner_up_gap), and the case asserts that;
  (c) for at most 17 poses, against the pair search: triple_totals[a] has the bits of the
      pair_totals of ctx.place_pair with pose a appended to the fixed sensors, for every
      admissible a -- the same search through the pair kernels alone.
The oracle's matrix is computed once for the whole tick; cell / pose subsets are slices of it."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pair_ref
import parity
import pytest
import triple_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "pointcloud_processor_amd" / "_lib" / "pcp_nodes_cli"
GAP = 0.1
T = 16        # the tile's edge in poses (kTripleTile = kPairTile; tests/test_triple_tiles_host.py
              # pins it)
CHUNK = 64    # cells per staged chunk (kWalkC of pcp_place_shared.hpp;
              # tests/test_place_shared_host.py pins it)


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
        Tc, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
        o_S, o_Z = oracle.score_matrix(Tc, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                                       oracle.vl_params())
        yield {"ctx": ctx, "poses": poses, "params": params, "S": o_S, "Z": o_Z,
               "zx": scene.zx120_pose5, "cells": cells}
        ctx.set_cells(cells.xyz, cells.normals)


def _finite_totals(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    live = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), live)
    np.testing.assert_array_equal(got[~live], ref[~live])   # -inf where the definition says so
    return got[live], ref[live]


COUNTS = ("best_single", "n_selected", "triple_covered", "pair_covered", "single_covered",
          "base_covered")
TOTALS = ("triple_total", "pair_total", "single_total", "base_total")


def _case(tick, pose_idx, Cn, fixed=(), sep=0.0, oracle_side=False, pair_side=None):
    """place_triple over poses[pose_idx] and cells[:Cn], checked (a), with oracle_side (b), and
    (c) for at most 17 poses unless pair_side says otherwise; returns (device result, device-side
    restatement)."""
    ctx, cells = tick["ctx"], tick["cells"]
    poses = np.ascontiguousarray(tick["poses"][pose_idx])
    Pn = poses.shape[0]
    fixed = list(fixed)
    ctx.set_cells(cells.xyz[:Cn], cells.normals[:Cn])
    got = ctx.place_triple(poses, tick["zx"], tick["params"], fixed, sep, want_first=True,
                           want_triple_totals=True, want_cells=True)
    d_S, d_Z = ctx.score_matrix(poses, tick["zx"], tick["params"])
    assert d_S.shape == (Pn, Cn)
    # (a) exact, on the device's own matrix
    ref = triple_ref.place_triple(d_S, d_Z, poses[:, :2], fixed, sep)
    assert got["triple_totals"].shape == (Pn, Pn, Pn) and got["first_totals"].shape == (Pn,)
    np.testing.assert_array_equal(_bits(got["triple_totals"]), _bits(ref["triple_totals"]))
    np.testing.assert_array_equal(_bits(got["first_totals"]), _bits(ref["first_totals"]))
    np.testing.assert_array_equal(got["first_partners"], ref["first_partners"])
    np.testing.assert_array_equal(got["best_triple"], ref["best_triple"])
    np.testing.assert_array_equal(got["best_pair"], ref["best_pair"])
    for k in COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in TOTALS:
        assert _bits(got[k])[0] == _bits(ref[k])[0], (k, got[k], ref[k])
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(ref["cell_score"]))
    np.testing.assert_array_equal(got["cell_owner"], ref["cell_owner"])
    # (c) the same search through the pair kernels
    if pair_side if pair_side is not None else Pn <= T + 1:
        adm = np.isfinite(ref["single_totals"])
        for a in range(Pn):
            if not adm[a]:
                assert not np.isfinite(got["triple_totals"][a]).any()
                continue
            pr = ctx.place_pair(poses, tick["zx"], tick["params"], fixed + [a], sep,
                                want_pair_totals=True)["pair_totals"]
            pr[:a + 1, :] = -np.inf   # (b > a: the pairs below a are other triples' rows)
            np.testing.assert_array_equal(_bits(got["triple_totals"][a]), _bits(pr))
    if not oracle_side:
        return got, ref
    # (b) the oracle's matrix
    orc = triple_ref.place_triple(tick["S"][pose_idx][:, :Cn], tick["Z"][:Cn], poses[:, :2], fixed,
                                  sep)
    gap = triple_ref.runner_up_gap(orc)
    assert gap > GAP, gap   # nothing hangs on ulps
    np.testing.assert_array_equal(got["best_triple"], orc["best_triple"])
    np.testing.assert_array_equal(got["best_pair"], orc["best_pair"])
    for k in COUNTS:
        assert got[k] == orc[k], (k, got[k], orc[k])
    np.testing.assert_array_equal(got["cell_owner"], orc["cell_owner"])
    tt = _finite_totals(got["triple_totals"], orc["triple_totals"])
    ft = _finite_totals(got["first_totals"], orc["first_totals"])
    print(f"C={Cn} P={Pn} fixed={fixed} sep={sep}: triples", parity.totals_report(*tt),
          "rows", parity.totals_report(*ft), "gap", gap)
    parity.assert_totals(*tt)
    parity.assert_totals(*ft)
    have = [k for k in TOTALS if np.isfinite(orc[k])]
    parity.assert_totals([got[k] for k in have], [orc[k] for k in have])
    return got, ref


# fixed, sep -> admissible triples, best triple, covered, n_selected (the oracle-side values of
# tests/test_triple_ref.py)
FULL = [
    ([], 0.0, 121485, (40, 41, 48), 3447, 3),
    ([], 2.0, 92306, (32, 41, 48), 3419, 3),
    ([], 5.0, 18009, (15, 48, 52), 3079, 3),
    ([], 8.0, 464, (23, 81, 90), 2491, 1),          # the best triple loses to pose 40 alone
    ([40], 0.0, 117480, (32, 41, 48), 3535, 3),
    ([40], 2.0, 71545, (24, 41, 56), 3503, 3),
    ([41, 48], 2.0, 54291, (24, 32, 66), 3574, 3),
    ([40, 41, 48, 3], 5.0, 5, (8, 81, 87), 3488, 3),  # beats the pair by 0.34
]


@pytest.mark.parametrize("fixed,sep,n_triples,triple,tcov,nsel", FULL)
def test_full_tick(tick, fixed, sep, n_triples, triple, tcov, nsel):
    got, ref = _case(tick, slice(None), 3704, fixed, sep, oracle_side=True)
    assert tuple(got["best_triple"]) == triple and got["n_selected"] == nsel
    assert int(np.isfinite(got["triple_totals"]).sum()) == n_triples
    assert got["triple_covered"] == tcov
    nf = len(fixed)
    if nsel == 1:   # the answer is the single: its cells carry owner n_fixed, none a later one
        assert got["best_single"] == 40
        assert got["triple_total"] < got["pair_total"] < got["single_total"]
        assert (got["cell_owner"] == nf).any() and not (got["cell_owner"] > nf).any()
    else:
        for i in range(3):
            assert (got["cell_owner"] == nf + i).any()
    # the steps 1 to 4 are the pair call's values
    pr = tick["ctx"].place_pair(tick["poses"], tick["zx"], tick["params"], fixed, sep)
    for k in ("best_single", "pair_covered", "single_covered", "base_covered"):
        assert got[k] == pr[k], k
    for k in ("pair_total", "single_total", "base_total"):
        assert _bits(got[k])[0] == _bits(pr[k])[0], k
    np.testing.assert_array_equal(got["best_pair"], pr["best_pair"])


@pytest.mark.parametrize("Cn", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
@pytest.mark.parametrize("Pn", [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1])
def test_pose_and_cell_counts(tick, Pn, Cn):
    """Pose counts around the tile edge (2T + 1 and 3T + 1 make all four kinds of tile triple
    occur: ta = tb = tc, ta = tb < tc, ta < tb = tc, ta < tb < tc) crossed with cell counts around
    the staged chunk.  Short cell prefixes leave exact ties between poses, so these are held to
    (a) and (c)."""
    got, ref = _case(tick, (np.arange(Pn) * 5) % 91, Cn)
    if Pn < 3:
        assert tuple(got["best_triple"]) == (-1, -1, -1) and got["triple_total"] == -np.inf
        assert got["triple_covered"] == 0 and got["n_selected"] <= Pn
    else:
        assert ref["n_triples"] == Pn * (Pn - 1) * (Pn - 2) // 6


@pytest.mark.parametrize("fixed", [[], [2 * T], [0, T, 2 * T, 5]])
@pytest.mark.parametrize("sep", [0.0, 2.0])
def test_fixed_sensors_across_tiles(tick, fixed, sep):
    """n_fixed = 0, 1 and 4 with the fixed sensors in every tile, the last, partial one included;
    with and without a separation that bites."""
    _case(tick, (np.arange(2 * T + 1) * 5) % 91, 3 * CHUNK + 5, fixed, sep)
    _case(tick, (np.arange(T + 1) * 5) % 91, 3704, [f for f in fixed if f <= T], sep)


def test_duplicates_and_ties(tick):
    got, _ = _case(tick, [40, 40, 41, 48, 48, 32, 32], 3704)
    # the first of the equal triples in lexicographic order
    assert tuple(got["best_triple"]) == (0, 2, 3)
    assert got["first_partners"].tolist()[:2] == [[2, 3], [2, 3]]
    np.testing.assert_array_equal(_bits(got["triple_totals"][0, 2, 3]),
                                  _bits(got["triple_totals"][1, 2, 4]))
    got, _ = _case(tick, [48, 41, 40], 3704)
    assert tuple(got["best_triple"]) == (0, 1, 2) and got["n_selected"] == 3
    # all poses the same: every triple ties, nothing is better than the single
    got, _ = _case(tick, [40] * (T + 1), CHUNK + 1)
    assert tuple(got["best_triple"]) == (0, 1, 2) and got["n_selected"] == 1


def test_separations_that_leave_no_triple_and_no_pair(tick):
    xy = tick["poses"][:, :2]
    d = np.hypot(*(xy[:, None, :] - xy[None, :, :]).transpose(2, 0, 1))
    b = int(np.argsort(d[0])[1])              # pose 0's nearest
    c = int(np.argmax(np.minimum(d[0], d[b])))   # far from both
    near, far = d[0, b], min(d[0, c], d[b, c])
    assert near < far
    idx = sorted([0, b, c])
    got, ref = _case(tick, idx, 3704, sep=0.5 * (near + far))   # pairs with c, no triple
    assert ref["n_pairs"] == 2 and ref["n_triples"] == 0
    assert tuple(got["best_triple"]) == (-1, -1, -1) and got["best_pair"][0] >= 0
    assert got["triple_total"] == -np.inf and got["triple_covered"] == 0
    got, ref = _case(tick, (np.arange(T + 1) * 5) % 91, 3704, sep=1000.0)   # no pair either
    assert ref["n_pairs"] == 0 and tuple(got["best_pair"]) == (-1, -1)
    assert tuple(got["best_triple"]) == (-1, -1, -1) and got["n_selected"] == 1
    assert not np.isfinite(got["first_totals"]).any() and (got["first_partners"] == -1).all()


def test_table_limit(tick):
    """One pose past PCP_TRIPLE_TABLE_MAX_POSES: refused with the table, searched without it."""
    ctx, cells = tick["ctx"], tick["cells"]
    Pn, Cn = _abi.TRIPLE_TABLE_MAX_POSES + 1, 256
    idx = np.arange(Pn) % 91
    poses = np.ascontiguousarray(tick["poses"][idx])
    poses[91:, 0] += 0.25   # the repeats, shifted
    ctx.set_cells(cells.xyz[:Cn], cells.normals[:Cn])
    with pytest.raises(_abi.PcpError) as e:
        ctx.place_triple(poses, tick["zx"], tick["params"], want_triple_totals=True)
    assert e.value.code == _abi.PCP_E_INVALID
    got = ctx.place_triple(poses, tick["zx"], tick["params"], min_separation=1.0,
                           want_first=True, want_cells=True)
    d_S, d_Z = ctx.score_matrix(poses, tick["zx"], tick["params"])
    ref = triple_ref.place_triple(d_S, d_Z, poses[:, :2], sep=1.0, want_table=False)
    np.testing.assert_array_equal(_bits(got["first_totals"]), _bits(ref["first_totals"]))
    np.testing.assert_array_equal(got["first_partners"], ref["first_partners"])
    np.testing.assert_array_equal(got["best_triple"], ref["best_triple"])
    assert _bits(got["triple_total"])[0] == _bits(ref["triple_total"])[0]
    for k in COUNTS:
        assert got[k] == ref[k], k
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(ref["cell_score"]))
    np.testing.assert_array_equal(got["cell_owner"], ref["cell_owner"])


def test_isolation(tick):
    """A place_pair, a score_poses and a place_refine before and after the search on one context:
    identical bytes; the caller's flags are not touched; the scratch allocations settle after the
    first call; two calls give equal bytes."""
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]

    def others():
        f = np.zeros(3704, np.uint8)
        t, c, r = ctx.score_poses(poses, zx, params, f)
        p = ctx.place_pair(poses, zx, params, [40], 2.0, want_pair_totals=True,
                           want_single_totals=True, want_cells=True)
        q = ctx.place_refine(poses, zx, params, [40, 41, 56], min_separation=2.0,
                             want_swap_totals=True, want_cells=True)
        return {"t": t, "c": c, "f": f, "r": repr(sorted(r.as_dict().items())),
                **{"p_" + k: v for k, v in p.items()}, **{"q_" + k: v for k, v in q.items()}}

    def same(x, y):
        assert x.keys() == y.keys()
        for k in x:
            a, b = np.asarray(x[k]), np.asarray(y[k])
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k

    before = others()
    kw = dict(fixed=[40], min_separation=2.0, want_first=True, want_triple_totals=True,
              want_cells=True)
    first = ctx.place_triple(poses, zx, params, **kw)
    settled = _abi.alloc_stats()
    again = ctx.place_triple(poses, zx, params, **kw)
    assert _abi.alloc_stats() == settled
    same(first, again)
    middle = others()
    same(before, middle)
    third = ctx.place_triple(poses, zx, params, **kw)
    same(first, third)
    same(before, others())
    # the optional outputs change nothing of the rest
    bare = ctx.place_triple(poses, zx, params, fixed=[40], min_separation=2.0)
    same(bare, {k: first[k] for k in bare})


def test_refusals_and_empty_inputs(tick):
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    poses, zx, params = tick["poses"], tick["zx"], tick["params"]
    ctx.profile(True)
    ctx.profile_reset()
    try:
        bad = [{"fixed": list(range(_abi.PLACE_MAX + 1))},   # n_fixed past PCP_PLACE_MAX
               {"reserved": 1},
               {"fixed": [91]}, {"fixed": [-1]},             # no pose of the call
               {"fixed": [3, 40, 3]}]                        # listed twice
        for kw in bad:
            with pytest.raises(_abi.PcpError) as e:
                ctx.place_triple(poses, zx, params, **kw)
            assert e.value.code == _abi.PCP_E_INVALID, kw
        many = np.ascontiguousarray(poses[np.arange(_abi.TRIPLE_MAX_POSES + 1) % 91])
        with pytest.raises(_abi.PcpError) as e:
            ctx.place_triple(many, zx, params)
        assert e.value.code == _abi.PCP_E_INVALID
        far = _abi.default_vl_params(max_distance=0.5 + 0.3 * (_abi.MAX_STEPS + 2))
        with pytest.raises(_abi.PcpError) as e:
            ctx.place_triple(poses, zx, far)
        assert e.value.code == _abi.PCP_E_INVALID
        # past the binding, at the C entry: every refusal leaves the outputs as they were
        C = _abi.C
        B = C.byref
        zxa = np.ascontiguousarray(zx, np.float64)
        big = np.ascontiguousarray(poses[np.arange(_abi.TRIPLE_MAX_POSES + 1) % 91])

        def raw(pp, n=91, table=False, n_sel=True, src=poses):
            bt, bp = (C.c_int64 * 3)(-7, -7, -7), (C.c_int64 * 2)(-7, -7)
            d = [C.c_double(-7.0) for _ in range(4)]
            i = [C.c_int32(-7) for _ in range(5)]
            bs = C.c_int64(-7)
            ft, fp = np.full(len(src), -7.0), np.full((len(src), 2), -7, np.int64)
            tab = np.full(8, -7.0)   # (never written: the call is refused)
            rc = ctx.lib.pcp_place_triple(
                ctx.h, _abi._ptr(src), n, _abi._ptr(zxa), B(params), B(pp), bt, B(d[0]), B(i[0]),
                bp, B(d[1]), B(i[1]), B(bs), B(d[2]), B(i[2]), B(d[3]), B(i[3]), _abi._ptr(ft),
                _abi._ptr(fp), _abi._ptr(tab) if table else None, None, None,
                B(i[4]) if n_sel else None)
            assert list(bt) == [-7] * 3 and list(bp) == [-7, -7] and bs.value == -7
            assert all(x.value == -7.0 for x in d) and all(x.value == -7 for x in i)
            assert (ft == -7.0).all() and (fp == -7).all() and (tab == -7.0).all()
            return rc

        ok = _abi.PairParams(0, 0, 0.0)
        assert raw(_abi.PairParams(-1, 0, 0.0)) == _abi.PCP_E_INVALID
        assert raw(_abi.PairParams(0, 1, 0.0)) == _abi.PCP_E_INVALID
        assert raw(ok, n_sel=False) == _abi.PCP_E_INVALID          # a null required pointer
        assert raw(ok, n=_abi.TRIPLE_MAX_POSES + 1, src=big) == _abi.PCP_E_INVALID
        assert raw(ok, n=_abi.TRIPLE_TABLE_MAX_POSES + 1, table=True, src=big) == _abi.PCP_E_INVALID
        twice = _abi.PairParams(2, 0, 0.0)
        twice.fixed[0] = twice.fixed[1] = 3
        assert raw(twice) == _abi.PCP_E_INVALID
        for k in ("score_cells", "pose_sum", "place_sensors"):   # nothing was launched
            assert ctx.profile_get(k)[1] == 0
    finally:
        ctx.profile(False)
    # no cells: nothing to cover
    ctx.set_cells(cells.xyz[:0], cells.normals[:0])
    got = ctx.place_triple(poses[:5], zx, params, want_first=True, want_triple_totals=True,
                           want_cells=True)
    assert got["n_selected"] == 0 and got["best_single"] == -1
    assert tuple(got["best_pair"]) == (-1, -1) and tuple(got["best_triple"]) == (-1, -1, -1)
    assert got["base_total"] == 0.0 and got["base_covered"] == 0
    assert got["cell_score"].size == 0 and not np.isfinite(got["triple_totals"]).any()
    assert (got["first_partners"] == -1).all() and not np.isfinite(got["first_totals"]).any()
    # no poses: the zx120 sensor alone
    ctx.set_cells(cells.xyz, cells.normals)
    got = ctx.place_triple(poses[:0], zx, params, want_first=True, want_triple_totals=True,
                           want_cells=True)
    assert got["n_selected"] == 0 and got["best_single"] == -1
    assert tuple(got["best_triple"]) == (-1, -1, -1) and got["triple_totals"].shape == (0, 0, 0)
    d_S, d_Z = ctx.score_matrix(poses[:1], zx, params)
    ref = pair_ref.place_pair(d_S[:0], d_Z, poses[:0, :2])
    np.testing.assert_array_equal(_bits(got["cell_score"]), _bits(d_Z))
    np.testing.assert_array_equal(got["cell_owner"], ref["cell_owner"])
    assert _bits(got["base_total"])[0] == _bits(ref["base_total"])[0]
    assert got["base_covered"] == ref["base_covered"]


def test_burst_times_the_triple_phase(tick):
    ctx, cells = tick["ctx"], tick["cells"]
    ctx.set_cells(cells.xyz, cells.normals)
    ms = ctx.place_triple_burst(tick["poses"], tick["zx"], tick["params"], reps=2)
    assert ms > 0.0
    for kw in ({"reps": 0}, {"fixed": [91]}):
        with pytest.raises(_abi.PcpError) as e:
            ctx.place_triple_burst(tick["poses"], tick["zx"], tick["params"], **kw)
        assert e.value.code == _abi.PCP_E_INVALID
    with pytest.raises(_abi.PcpError) as e:   # fewer than three poses: nothing to time
        ctx.place_triple_burst(tick["poses"][:2], tick["zx"], tick["params"], reps=2)
    assert e.value.code == _abi.PCP_E_INVALID


def test_cli_place_triple(tick, tmp_path, scene, cells, aux):
    """pcp_nodes_cli place_triple (MobileLidarPlacement::place_triple above the node's tick): the
    binding's answer, and a log that names the three poses, the gain over the pair and the gain
    over greedy's three."""
    assert CLI.exists(), "build first (__graft_entry__.build())"
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(aux).tofile(tmp_path / "a.f32")
    np.ascontiguousarray(cells.xyz, np.float64).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals, np.float32).tofile(tmp_path / "n.f32")
    t = lambda v: ",".join(repr(float(x)) for x in v)   # noqa: E731
    r = subprocess.run([str(CLI), "place_triple", str(tmp_path / "t.f32"),
                        str(scene.terrain.shape[0]), str(tmp_path / "a.f32"), str(aux.shape[0]),
                        str(tmp_path / "c.f64"), str(tmp_path / "n.f32"),
                        str(cells.xyz.shape[0]), t(cells.grid_bbox), "0,0,0", "100", "15.0", "3",
                        "2.0", str(tmp_path / "sel.i64"), str(tmp_path / "tot.f64"),
                        str(tmp_path / "rep.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    ctx = tick["ctx"]
    ctx.set_cells(cells.xyz, cells.normals)
    got = ctx.place_triple(tick["poses"], tick["zx"], tick["params"], min_separation=2.0)
    greedy = ctx.place_sensors(tick["poses"], tick["zx"], tick["params"], 3, 2.0)
    assert res["n_candidates"] == 91 and res["n_selected"] == got["n_selected"] == 3
    assert res["best_triple"] == got["best_triple"].tolist() == [32, 41, 48]
    assert res["best_pair"] == got["best_pair"].tolist()
    assert res["best_single"] == got["best_single"] and res["total_cells"] == 3704
    assert res["triple_covered"] == got["triple_covered"]
    np.testing.assert_array_equal(np.fromfile(tmp_path / "sel.i64", np.int64), got["best_triple"])
    np.testing.assert_array_equal(
        _bits(np.fromfile(tmp_path / "tot.f64", np.float64)),
        _bits([got["base_total"], got["single_total"], got["pair_total"], got["triple_total"]]))
    log = (tmp_path / "rep.txt").read_text()
    assert "Exact Triple Placement (ZX120 + 0 Fixed + 3 Mobile)" in log
    assert f"Total Score (ZX120 only): {got['base_total']:.2f}" in log
    for i, s in enumerate(got["best_triple"]):
        p = tick["poses"][s]
        assert (f"Best Triple LiDAR {i + 1} Position: ({p[0]:.2f}, {p[1]:.2f}, {p[2]:.2f})  "
                f"[candidate {s}]") in log
    gain = got["triple_total"] - got["pair_total"]
    assert f"  Total Score: {got['triple_total']:.2f} (gain over pair {gain:.2f})" in log
    assert greedy["selected"].tolist() == [40, 41, 56]
    over = got["triple_total"] - greedy["total_after"][2]
    assert f"(exact triple gains {over:.2f})" in log and over > 7
