"""`pcp_nodes_cli scan`: pcp::VirtualScan (host/pcp_scan_node.cpp) from files -- every sensor's
scan message, the segments' offsets, the terrain's blind-spot records and the per-point mask,
against the NumPy restatement on the oracle's first hits."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"


def test_cli_scan_matches_the_restatement(oracle, tmp_path: Path):
    cloud, poses, fan, fh, blocked, ref = scan_ref.clutter_case(oracle, 100, 37, 15.0)
    rec = np.zeros((cloud.shape[0], 8), np.float32)      # 32-byte records, x / y / z at 0 / 4 / 8
    rec[:, :3] = cloud[:, :3]
    rec[:, 4] = np.arange(cloud.shape[0], dtype=np.float32)   # a payload the blind spots keep
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    out = [tmp_path / n for n in ("scans.bin", "offsets.u64", "blind.f32", "mask.u64")]
    r = subprocess.run([str(CLI), "scan", str(tmp_path / "terrain.f32"), str(cloud.shape[0]),
                        ",".join(repr(float(v)) for v in poses.ravel()), "100", "37", "15.0"]
                       + [str(o) for o in out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    scans = np.fromfile(out[0], _abi.SCAN_RETURN_DTYPE)
    assert scans.tobytes() == ref["returns"].tobytes()
    np.testing.assert_array_equal(np.fromfile(out[1], np.uint64), ref["offsets"])
    mask = np.fromfile(out[3], np.uint64)
    np.testing.assert_array_equal(mask, ref["point_mask"])
    blind = np.fromfile(out[2], np.float32).reshape(-1, 8)
    assert blind.tobytes() == rec[ref["point_mask"] == 0].tobytes()   # input order, own records
    assert info == {"n_sensors": 6, "n_returns": int(ref["offsets"][-1]),
                    "n_points": cloud.shape[0], "n_seen_any": ref["n_seen_any"],
                    "n_blind": cloud.shape[0] - ref["n_seen_any"]}


def test_cli_scan_refuses_bad_arguments(tmp_path: Path):
    (tmp_path / "t.f32").write_bytes(np.zeros((4, 8), np.float32).tobytes())
    base = [str(CLI), "scan", str(tmp_path / "t.f32"), "4"]
    tail = ["8", "2", "15.0"] + [str(tmp_path / n) for n in ("a", "b", "c", "d")]
    assert subprocess.run(base + ["1,2,3,4"] + tail, capture_output=True).returncode == 2
    assert subprocess.run(base + ["1,2,3,0,0"] + tail[:-1], capture_output=True).returncode == 2
