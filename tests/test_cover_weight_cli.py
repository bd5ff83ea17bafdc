"""`pcp_nodes_cli cover_weighted` on the GPU: the files it writes and the JSON line it prints
against the NumPy restatement (tests/cover_weight_ref.py), for weights from a byte file and from a
base weight with a box list, and the status-2 refusals of bad arguments."""
import json
import subprocess
from pathlib import Path

import cover_ref
import cover_weight_ref as wr
import numpy as np
import pytest
from test_cover_cli import _records32

from pointcloud_processor_amd import _abi

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"
BOXES = [((-1.5, 1.5, -1.5, 1.5, -0.9, 100.0), 200), ((0.0, 1.5, -1.5, 1.5, -0.9, 100.0), 10),
         ((50.0, 51.0, 50.0, 51.0, 0.0, 1.0), 77)]      # (the last holds no point)


def _run(args, timeout=120):
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=timeout)


def _box_weights(cloud, base, boxes):
    """The host rule: bounds included, the last box that holds a point decides."""
    x, y, z = (cloud[:, c].astype(np.float64) for c in range(3))
    w = np.full(cloud.shape[0], base, np.uint8)
    for (x0, x1, y0, y1, z0, z1), wt in boxes:
        w[(x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)] = wt
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["bytes", "boxes"])
def test_cli_cover_weighted_is_the_restatement(oracle, tmp_path: Path, source):
    """`three` from a byte file at 2.5 m beside two fixed candidates; a base weight of 1 with two
    overlapping boxes (the later one wins) and one that holds nothing."""
    inst = cover_ref.instance(oracle)
    if source == "bytes":
        sep, fixed, k = cover_ref.SEP, (10, 40), 4
        weight = wr.weights(oracle)["three"]
        (tmp_path / "w.u8").write_bytes(weight.tobytes())
        w_arg = tmp_path / "w.u8"
    else:
        sep, fixed, k = 0.0, (), 4
        weight = _box_weights(inst["cloud"], 1, BOXES)
        assert sorted(np.unique(weight).tolist()) == [1, 10, 200]
        w_arg = "1/" + "/".join(",".join(repr(v) for v in b) + f",{wt}" for b, wt in BOXES)
    ref = wr.greedy(inst["seen"], inst["poses"][:, :2], weight, k, sep, fixed)
    assert ref["n_selected"] >= 2
    rec = _records32(inst["cloud"])
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    (tmp_path / "poses.f64").write_bytes(np.ascontiguousarray(inst["poses"]).tobytes())
    args = ["cover_weighted", tmp_path / "terrain.f32", inst["N"], tmp_path / "poses.f64", 100, 37,
            15.0, k, sep, w_arg, tmp_path / "sel.i64", tmp_path / "owner.i32",
            tmp_path / "blind.f32"]
    if fixed:
        args.append(",".join(str(f) for f in fixed))
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 4)
    owner = np.fromfile(tmp_path / "owner.i32", np.int32)
    blind = np.fromfile(tmp_path / "blind.f32", np.float32).reshape(-1, 8)
    np.testing.assert_array_equal(sel[:, 0], ref["selected"])
    np.testing.assert_array_equal(sel[:, 1], ref["gain"].astype(np.int64))
    np.testing.assert_array_equal(sel[:, 2], ref["gain_points"].astype(np.int64))
    np.testing.assert_array_equal(sel[:, 3], ref["covered_after"].astype(np.int64))
    np.testing.assert_array_equal(owner, ref["point_owner"])
    is_blind = (weight != 0) & (ref["point_owner"] == wr.OWNER_NONE)
    want_blind = rec[is_blind]
    assert blind.tobytes() == want_blind.tobytes()
    covered = int(ref["covered_after"][-1])
    blind_weight = int(weight[is_blind].astype(np.int64).sum())
    assert out == {"n_candidates": 71, "n_selected": ref["n_selected"], "n_points": inst["N"],
                   "roi_points": ref["roi_points"], "roi_weight": ref["roi_weight"],
                   "base_covered": ref["base_covered"], "base_points": ref["base_points"],
                   "covered": covered, "n_blind": want_blind.shape[0],
                   "blind_weight": blind_weight}
    assert ref["roi_weight"] - covered == blind_weight
    # the table goes to stderr, in weight with the points beside it
    assert (f"Weighted Coverage Placement ({len(fixed)} Fixed + {ref['n_selected']} Mobile)"
            in r.stderr)
    assert f"[candidate {int(ref['selected'][0])}]" in r.stderr
    assert (f"  Weight gained: {int(ref['gain'][0])} ({int(ref['gain_points'][0])} points)"
            in r.stderr)


@pytest.mark.gpu
def test_cli_cover_weighted_refuses_bad_arguments(tmp_path: Path):
    cloud = np.zeros((4, 8), np.float32)
    cloud[:, 0] = np.arange(4)
    (tmp_path / "t.f32").write_bytes(cloud.tobytes())
    (tmp_path / "w3.u8").write_bytes(bytes([1, 1, 1]))
    outs = [tmp_path / "s", tmp_path / "o", tmp_path / "b"]
    base = ["cover_weighted", tmp_path / "t.f32", 4, "0,0,1,0,0,1,1,1,0,0", 8, 2, 5.0, 2, 0.0]
    assert _run(base + ["1"] + outs[:2]).returncode == 2                   # too few arguments
    bad_poses = list(base)
    bad_poses[3] = "0,0,1,0"
    assert _run(bad_poses + ["1"] + outs).returncode == 2                  # not 5 per candidate
    assert _run(base + [tmp_path / "w3.u8"] + outs).returncode == 2        # WEIGHTS bytes != TN
    assert _run(base + ["256"] + outs).returncode == 2                     # base weight > 255
    assert _run(base + ["1.5"] + outs).returncode == 2                     # no whole number
    assert _run(base + ["1,2"] + outs).returncode == 2                     # two base weights
    assert _run(base + ["1/0,1,0,1,0,1"] + outs).returncode == 2           # a box without a weight
    assert _run(base + ["1/0,1,0,1,0,1,300"] + outs).returncode == 2       # a box weight > 255
    assert _run(base + ["/0,1,0,1,0,1,3"] + outs).returncode == 2          # no base weight
    assert _run(base + ["1"] + outs + ["2"]).returncode == 2               # FIXED is no candidate
    assert _run(base + ["1"] + outs + ["0.5"]).returncode == 2
    for p in outs:
        assert not p.exists()
    assert _run(["cover_weighted"]).returncode == 2
