"""`pcp_nodes_cli cover_aimed` on the GPU: the files it writes and the JSON line it prints against
the NumPy restatement (tests/cover_aim_ref.py), and the status-2 refusals of bad arguments."""
import json
import subprocess
from pathlib import Path

import cover_aim_ref as car
import numpy as np
import pytest
from test_cover_cli import _records32

from pointcloud_processor_amd import _abi

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"


def _run(args, timeout=120):
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=timeout)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [3, 4])
def test_cli_cover_aimed_is_the_restatement(oracle, tmp_path: Path, i):
    """64 aims over (x > 0, 2.5 m) with its early stop, and 24 aims beside two fixed (candidate,
    aim) pairs."""
    inst = car.instance(oracle)
    ref = car.grid_case(oracle, i)
    table, roi_name, sep, fixed, k = car.GRID[i]
    w_az, w_el, aims = car.TABLES[table]
    roi = inst["rois"][roi_name]
    rec = _records32(inst["cloud"])
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    (tmp_path / "poses.f64").write_bytes(np.ascontiguousarray(inst["poses"]).tobytes())
    roi_arg = "-"
    if roi is not None:
        (tmp_path / "roi.u8").write_bytes(roi.tobytes())
        roi_arg = tmp_path / "roi.u8"
    args = ["cover_aimed", tmp_path / "terrain.f32", inst["N"], tmp_path / "poses.f64", 100, 37,
            15.0, k, sep, roi_arg, w_az, w_el, ",".join(f"{a},{e}" for a, e in aims),
            tmp_path / "sel.i64", tmp_path / "owner.i32", tmp_path / "blind.f32"]
    if fixed:
        args.append(",".join(f"{p},{a}" for p, a in fixed))
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 4)
    owner = np.fromfile(tmp_path / "owner.i32", np.int32)
    blind = np.fromfile(tmp_path / "blind.f32", np.float32).reshape(-1, 8)
    np.testing.assert_array_equal(sel[:, 0], ref["selected"])
    np.testing.assert_array_equal(sel[:, 1], ref["selected_aim"])
    np.testing.assert_array_equal(sel[:, 2], ref["gain"].astype(np.int64))
    np.testing.assert_array_equal(sel[:, 3], ref["covered_after"].astype(np.int64))
    np.testing.assert_array_equal(owner, ref["point_owner"])
    in_roi = np.ones(inst["N"], bool) if roi is None else roi != 0
    want_blind = rec[in_roi & (ref["point_owner"] == car.OWNER_NONE)]
    assert blind.tobytes() == want_blind.tobytes()
    covered = int(ref["covered_after"][-1]) if ref["n_selected"] else ref["base_covered"]
    assert out == {"n_candidates": 71, "n_aims": len(aims), "n_selected": ref["n_selected"],
                   "n_points": inst["N"], "roi_points": ref["roi_points"],
                   "base_covered": ref["base_covered"], "covered": covered,
                   "n_blind": want_blind.shape[0]}
    assert ref["roi_points"] - covered == want_blind.shape[0]
    # the table goes to stderr, the aim beside the candidate
    assert (f"Aimed Coverage Placement ({len(fixed)} Fixed + {ref['n_selected']} Mobile)"
            in r.stderr)
    assert f"Window: {w_az} columns x {w_el} rings, {len(aims)} aims per candidate" in r.stderr
    a0 = int(ref["selected_aim"][0])
    assert f"[candidate {int(ref['selected'][0])}]" in r.stderr
    assert f"  Aim {a0}: columns from {aims[a0][0]}, rings from {aims[a0][1]}" in r.stderr


@pytest.mark.gpu
def test_cli_cover_aimed_refuses_bad_arguments(tmp_path: Path):
    cloud = np.zeros((4, 8), np.float32)
    cloud[:, 0] = np.arange(4)
    (tmp_path / "t.f32").write_bytes(cloud.tobytes())
    (tmp_path / "roi3.u8").write_bytes(bytes([1, 1, 1]))
    outs = [tmp_path / "s", tmp_path / "o", tmp_path / "b"]
    front = ["cover_aimed", tmp_path / "t.f32", 4, "0,0,1,0,0,1,1,1,0,0", 8, 2, 5.0, 2, 0.0]
    good = front + ["-", 3, 1, "0,0,5,1"]

    def with_(at, value):
        a = list(good)
        a[at] = value
        return a

    assert _run(good + outs[:2]).returncode == 2                         # too few arguments
    assert _run(with_(3, "0,0,1,0") + outs).returncode == 2              # not 5 per candidate
    assert _run(with_(9, tmp_path / "roi3.u8") + outs).returncode == 2   # ROI bytes != TN
    assert _run(with_(10, 0) + outs).returncode == 2                     # WAZ < 1
    assert _run(with_(10, 9) + outs).returncode == 2                     # WAZ > NAZ
    assert _run(with_(11, 3) + outs).returncode == 2                     # WEL > NEL
    assert _run(with_(12, "0,0,5") + outs).returncode == 2               # AIMS not in pairs
    assert _run(with_(12, "8,0") + outs).returncode == 2                 # az0 = NAZ
    assert _run(with_(12, "0,2") + outs).returncode == 2                 # el0 > NEL - WEL
    assert _run(with_(12, "0.5,0") + outs).returncode == 2               # no whole number
    assert _run(with_(12, ",".join(["0,0"] * 65)) + outs).returncode == 2   # 65 aims
    assert _run(good + outs + ["2,0"]).returncode == 2                   # FIXED is no candidate
    assert _run(good + outs + ["0,2"]).returncode == 2                   # FIXED aim outside AIMS
    assert _run(good + outs + ["0"]).returncode == 2                     # FIXED not in pairs
    for p in outs:
        assert not p.exists()
    assert _run(["cover_aimed"]).returncode == 2
