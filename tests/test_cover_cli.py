"""`pcp_nodes_cli cover` on the GPU: the files it writes and the JSON line it prints against the
NumPy restatement (tests/cover_ref.py), and the status-2 refusals of bad arguments."""
import json
import subprocess
from pathlib import Path

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
@pytest.mark.parametrize("i", [3, 6])
def test_cli_cover_is_the_restatement(oracle, tmp_path: Path, i):
    """(x > 0, 2.5 m) with its early stop, and (all, 2.5 m) beside two fixed candidates."""
    inst = cover_ref.instance(oracle)
    ref = cover_ref.grid_case(oracle, i)
    roi_name, sep, fixed, k = cover_ref.GRID[i]
    roi = inst["rois"][roi_name]
    rec = _records32(inst["cloud"])
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    (tmp_path / "poses.f64").write_bytes(np.ascontiguousarray(inst["poses"]).tobytes())
    roi_arg = "-"
    if roi is not None:
        (tmp_path / "roi.u8").write_bytes(roi.tobytes())
        roi_arg = tmp_path / "roi.u8"
    args = ["cover", tmp_path / "terrain.f32", inst["N"], tmp_path / "poses.f64", 100, 37, 15.0, k,
            sep, roi_arg, tmp_path / "sel.i64", tmp_path / "owner.i32", tmp_path / "blind.f32"]
    if fixed:
        args.append(",".join(str(f) for f in fixed))
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 3)
    owner = np.fromfile(tmp_path / "owner.i32", np.int32)
    blind = np.fromfile(tmp_path / "blind.f32", np.float32).reshape(-1, 8)
    np.testing.assert_array_equal(sel[:, 0], ref["selected"])
    np.testing.assert_array_equal(sel[:, 1], ref["gain"].astype(np.int64))
    np.testing.assert_array_equal(sel[:, 2], ref["covered_after"].astype(np.int64))
    np.testing.assert_array_equal(owner, ref["point_owner"])
    in_roi = np.ones(inst["N"], bool) if roi is None else roi != 0
    want_blind = rec[in_roi & (ref["point_owner"] == cover_ref.OWNER_NONE)]
    assert blind.tobytes() == want_blind.tobytes()
    covered = int(ref["covered_after"][-1]) if ref["n_selected"] else ref["base_covered"]
    assert out == {"n_candidates": 71, "n_selected": ref["n_selected"], "n_points": inst["N"],
                   "roi_points": ref["roi_points"], "base_covered": ref["base_covered"],
                   "covered": covered, "n_blind": want_blind.shape[0]}
    assert ref["roi_points"] - covered == want_blind.shape[0]
    # the table goes to stderr
    assert f"Coverage Placement ({len(fixed)} Fixed + {ref['n_selected']} Mobile)" in r.stderr
    assert f"[candidate {int(ref['selected'][0])}]" in r.stderr


@pytest.mark.gpu
def test_cli_cover_refuses_bad_arguments(tmp_path: Path):
    cloud = np.zeros((4, 8), np.float32)
    cloud[:, 0] = np.arange(4)
    (tmp_path / "t.f32").write_bytes(cloud.tobytes())
    (tmp_path / "roi3.u8").write_bytes(bytes([1, 1, 1]))
    outs = [tmp_path / "s", tmp_path / "o", tmp_path / "b"]
    base = ["cover", tmp_path / "t.f32", 4, "0,0,1,0,0,1,1,1,0,0", 8, 2, 5.0, 2, 0.0]
    assert _run(base[:9] + ["-"] + outs[:2]).returncode == 2                 # too few arguments
    bad_poses = list(base)
    bad_poses[3] = "0,0,1,0"
    assert _run(bad_poses + ["-"] + outs).returncode == 2                    # not 5 per candidate
    assert _run(base + [tmp_path / "roi3.u8"] + outs).returncode == 2        # ROI bytes != TN
    assert _run(base + ["-"] + outs + ["2"]).returncode == 2                 # FIXED is no candidate
    assert _run(base + ["-"] + outs + ["0.5"]).returncode == 2
    for p in outs:
        assert not p.exists()
    assert _run(["cover"]).returncode == 2
