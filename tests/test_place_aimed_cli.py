"""pcp_nodes_cli place_aimed (MobileLidarPlacement::place_aimed above the node's tick) against
tests/aim_ref.py on the oracle's matrix of the pitch-zeroed candidates: the selected (candidate,
aim) pairs equal, the totals under tests/parity.py's bar, every round decided by more than 0.1;
and the table it prints."""
import json
import math
import subprocess
from pathlib import Path

import aim_ref
import numpy as np
import parity
import pytest

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "pointcloud_processor_amd" / "_lib" / "pcp_nodes_cli"


@pytest.mark.parametrize("fixed,want", [
    ((), [(32, 8), (40, 6), (33, 7)]),
    # one and two aimed sensors already placed (MobileLidarPlacement::FixedAimed): the first
    # rounds' answers as the base, the later rounds' as the answer
    (((32, 8),), [(40, 6), (33, 7)]),
    (((40, 6), (32, 8)), [(33, 7)]),
])
def test_cli_place_aimed(tmp_path, oracle, scene, cells, aux, fixed, want):
    assert CLI.exists(), "build first (__graft_entry__.build())"
    h, v = math.radians(90), math.radians(60)
    aims = aim_ref.tick_aims()
    np.ascontiguousarray(scene.terrain).tofile(tmp_path / "t.f32")
    np.ascontiguousarray(aux).tofile(tmp_path / "a.f32")
    np.ascontiguousarray(cells.xyz, np.float64).tofile(tmp_path / "c.f64")
    np.ascontiguousarray(cells.normals, np.float32).tofile(tmp_path / "n.f32")
    aims.tofile(tmp_path / "aims.f64")
    t = lambda q: ",".join(repr(float(x)) for x in q)   # noqa: E731
    r = subprocess.run([str(CLI), "place_aimed", str(tmp_path / "t.f32"),
                        str(scene.terrain.shape[0]), str(tmp_path / "a.f32"), str(aux.shape[0]),
                        str(tmp_path / "c.f64"), str(tmp_path / "n.f32"), str(cells.xyz.shape[0]),
                        t(cells.grid_bbox), "0,0,0", "100", "15.0", str(len(want)), "0.0",
                        str(tmp_path / "sel.i64"), str(tmp_path / "tot.f64"),
                        str(tmp_path / "rep.txt"), repr(h), repr(v), str(tmp_path / "aims.f64")] +
                       ([",".join(str(x) for q in fixed for x in q)] if fixed else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 2)
    tot = np.fromfile(tmp_path / "tot.f64", np.float64)
    # the oracle's side, for the candidates the device generates (the node's own)
    params = _abi.default_vl_params()
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = np.ascontiguousarray(
            ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5))
    flat = poses.copy()
    flat[:, 3] = 0.0
    S, Z = oracle.score_matrix(oracle.Cloud(scene.terrain), oracle.Cloud(aux), cells.xyz,
                               cells.normals, flat, scene.zx120_pose5, oracle.vl_params())
    orc = aim_ref.place_aimed(S, Z, flat, cells.xyz, aims, h, v, len(want), fixed)
    assert all(g > 0.1 for g in aim_ref.runner_up_gaps(orc))
    assert res["n_candidates"] == 91 and res["n_aims"] == 45 and res["total_cells"] == 3704
    assert res["n_selected"] == orc["n_selected"] == len(want) and res["n_fixed"] == len(fixed)
    assert sel[:, 0].tolist() == orc["selected"].tolist() == [p for p, _ in want]
    assert sel[:, 1].tolist() == orc["selected_aim"].tolist() == [a for _, a in want]
    parity.assert_totals(tot, orc["total_after"])
    if fixed:   # (a fixed sensor's cells carry the device matrix's few-ulp differences)
        parity.assert_totals(res["base_total"], orc["base_total"])
        assert res["base_total"] > 1715.36   # (zx120 alone totals 1715.354...)
    else:
        parity.assert_totals_exact(res["base_total"], orc["base_total"])
    assert res["base_covered"] == orc["base_covered"]
    log = (tmp_path / "rep.txt").read_text()
    assert f"Aimed LiDAR Placement (ZX120 + {len(fixed)} Fixed + {len(want)} Mobile)" in log
    assert "Field of view: 90.0 x 60.0 deg" in log
    assert (f"Total Score (ZX120{' + fixed' if fixed else ' only'}): "
            f"{res['base_total']:.2f}") in log
    deg = 180.0 / math.pi
    for i, ((p, a), total) in enumerate(zip(sel.tolist(), tot)):
        q = poses[p]
        assert (f"Mobile LiDAR {i + 1} Position: ({q[0]:.2f}, {q[1]:.2f}, {q[2]:.2f})  "
                f"[candidate {p}, aim {a}]") in log
        assert (f"  Heading: yaw {(q[4] + aims[a, 0]) * deg:.1f} deg, "
                f"pitch {aims[a, 1] * deg:.1f} deg") in log
        assert f"  Total Score: {total:.2f} (gain " in log
