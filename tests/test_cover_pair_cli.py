"""`pcp_nodes_cli cover_pair` on the GPU -- CoveragePlacement::place_pair over the real library:
the files it writes and the JSON line it prints against the NumPy restatement
(tests/cover_pair_ref.py), the log's comparison line, and the status-2 refusals of bad arguments."""
import json
import subprocess
from pathlib import Path

import cover_pair_ref
import cover_ref
import numpy as np
import pytest

from pointcloud_processor_amd import _abi

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"


def _records32(cloud):
    """The terrain as the CLI reads it: 32-byte records, x / y / z at 0 / 4 / 8, a tag behind."""
    rec = np.zeros((cloud.shape[0], 8), np.float32)
    rec[:, :3] = cloud[:, :3]
    rec[:, 5] = np.arange(cloud.shape[0], dtype=np.float32)
    return rec


def _run(args, timeout=120):
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=timeout)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("box_a", 0.0, ()), ("all", cover_ref.SEP, (10, 40)),
                                  ("seen35", 0.0, ())])
def test_cli_cover_pair_is_the_restatement(oracle, tmp_path: Path, case):
    """The region where greedy's two are not the best pair; a separation beside two fixed
    candidates; and a region the best single covers alone (one round)."""
    i = cover_pair_ref.GRID.index(case)
    inst = cover_ref.instance(oracle)
    ref = cover_pair_ref.grid_case(oracle, i)
    roi_name, sep, fixed = case
    roi = cover_pair_ref.rois(oracle)[roi_name]
    rec = _records32(inst["cloud"])
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    (tmp_path / "poses.f64").write_bytes(np.ascontiguousarray(inst["poses"]).tobytes())
    roi_arg = "-"
    if roi is not None:
        (tmp_path / "roi.u8").write_bytes(roi.tobytes())
        roi_arg = tmp_path / "roi.u8"
    args = ["cover_pair", tmp_path / "terrain.f32", inst["N"], tmp_path / "poses.f64", 100, 37,
            15.0, sep, roi_arg, tmp_path / "sel.i64", tmp_path / "owner.i32",
            tmp_path / "blind.f32"]
    if fixed:
        args.append(",".join(str(f) for f in fixed))
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 3)
    owner = np.fromfile(tmp_path / "owner.i32", np.int32)
    blind = np.fromfile(tmp_path / "blind.f32", np.float32).reshape(-1, 8)
    # the rounds: a with its own gain, then b with the rest of the pair's; or the single alone
    base = ref["base_covered"]
    if ref["n_selected"] == 2:
        a, b = (int(v) for v in ref["best_pair"])
        ga = int(ref["single_gains"][a])
        want = [[a, ga, base + ga], [b, ref["pair_gain"] - ga, base + ref["pair_gain"]]]
    else:
        assert ref["n_selected"] == 1
        want = [[ref["best_single"], ref["single_gain"], base + ref["single_gain"]]]
    assert sel.tolist() == want
    np.testing.assert_array_equal(owner, ref["point_owner"])
    in_roi = np.ones(inst["N"], bool) if roi is None else roi != 0
    want_blind = rec[in_roi & (ref["point_owner"] == cover_pair_ref.OWNER_NONE)]
    assert blind.tobytes() == want_blind.tobytes()
    covered = want[-1][2]
    assert out == {"n_candidates": 71, "n_selected": ref["n_selected"], "n_points": inst["N"],
                   "roi_points": ref["roi_points"], "base_covered": base, "covered": covered,
                   "n_blind": want_blind.shape[0],
                   "best_pair": [int(v) for v in ref["best_pair"]],
                   "pair_gain": ref["pair_gain"], "best_single": ref["best_single"],
                   "single_gain": ref["single_gain"]}
    assert ref["roi_points"] - covered == want_blind.shape[0]
    # the table goes to stderr, with the comparison of the pair and the single
    assert f"Coverage Placement ({len(fixed)} Fixed + {ref['n_selected']} Mobile)" in r.stderr
    assert f"[candidate {want[0][0]}]" in r.stderr
    a, b = (int(v) for v in ref["best_pair"])
    verdict = "the pair adds more" if ref["n_selected"] == 2 else "the pair adds no more"
    assert (f"Best pair: candidates ({a}, {b}) gain {ref['pair_gain']} points; best single: "
            f"candidate {ref['best_single']} gains {ref['single_gain']} ({verdict})") in r.stderr


@pytest.mark.gpu
def test_cli_cover_pair_refuses_bad_arguments(tmp_path: Path):
    cloud = np.zeros((4, 8), np.float32)
    cloud[:, 0] = np.arange(4)
    (tmp_path / "t.f32").write_bytes(cloud.tobytes())
    (tmp_path / "roi3.u8").write_bytes(bytes([1, 1, 1]))
    outs = [tmp_path / "s", tmp_path / "o", tmp_path / "b"]
    base = ["cover_pair", tmp_path / "t.f32", 4, "0,0,1,0,0,1,1,1,0,0", 8, 2, 5.0, 0.0]
    assert _run(base[:8] + ["-"] + outs[:2]).returncode == 2                 # too few arguments
    bad_poses = list(base)
    bad_poses[3] = "0,0,1,0"
    assert _run(bad_poses + ["-"] + outs).returncode == 2                    # not 5 per candidate
    assert _run(base + [tmp_path / "roi3.u8"] + outs).returncode == 2        # ROI bytes != TN
    assert _run(base + ["-"] + outs + ["2"]).returncode == 2                 # FIXED is no candidate
    assert _run(base + ["-"] + outs + ["0.5"]).returncode == 2
    for p in outs:
        assert not p.exists()
    assert _run(["cover_pair"]).returncode == 2
