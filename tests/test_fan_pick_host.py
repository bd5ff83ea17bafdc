"""pcp_fan_pick.hpp (which fan kernel a query launches, on which grid) on the
CPU: the header has no HIP dependency, so tests/native/fan_pick_selftest.cpp is built with the
host compiler and run as a stand-alone program, no GPU call.  The program compares the rule with
the launch code it replaced, and prints the poses per wave and the production kernel's name,
which bench.py restates (_fan_npw, _fan_roofline's "kernel"): the two must agree."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("fan_pick") / "fan_pick_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "fan_pick_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-4000:], r.stderr)
    return r.stdout.splitlines()


def test_rule_is_the_replaced_launch_code(selftest_out):
    # the full product of the module docstring of fan_pick_selftest.cpp, three live intervals each
    m = re.fullmatch(r"(\d+) cases, (\d+) launches compared, (\d+) mismatches", selftest_out[-2])
    assert m, selftest_out[-2]
    cases, launches, mismatches = map(int, m.groups())
    assert cases == 3 * 6 * 6 * 2 * 75 * 5 * 6 * 2
    assert launches > cases and mismatches == 0


def test_poses_per_wave_is_bench_fan_npw(selftest_out, monkeypatch):
    import bench

    rows = [ln.split() for ln in selftest_out if ln.startswith("npw ")]
    assert len(rows) == 256 * 8
    assert {int(r[1]) for r in rows} == set(range(1, 257))
    for _, P, req, _, npw in rows:
        monkeypatch.setenv("PCP_FAN_NPW", req)
        assert bench._fan_npw(int(P)) == int(npw), (P, req)
    monkeypatch.delenv("PCP_FAN_NPW")   # the default request is the context's: 8
    for _, P, req, _, npw in rows:
        if req == "8":
            assert bench._fan_npw(int(P)) == int(npw), P


class _FineCtx:
    """What bench._fan_roofline reads of a context with a fine terrain copy."""

    def __init__(self, fine_tile):
        self.fine_tile = fine_tile

    def raycast_fan_stats(self, poses, fan):
        return {"samples_visited": 1000, "scanned_stencils": 100, "point_tests": 10,
                "directory_loads": 0}

    def terrain_info(self):
        return {"scan_layout": "fine", "fine_tile": self.fine_tile}


def test_production_kernel_name_is_bench_roofline_kernel(selftest_out, monkeypatch):
    import bench
    from pointcloud_processor_amd import _abi

    rows = [ln.split(None, 4) for ln in selftest_out if ln.startswith("kernel ")]
    assert len(rows) == 2 * 5 * 6
    fan = _abi.fan_params(n_az=128, n_el=32)
    seen = set()
    for _, ftile, P, req, name in rows:
        monkeypatch.setenv("PCP_FAN_NPW", req)
        r = bench._fan_roofline(_FineCtx(int(ftile)), np.zeros((int(P), 5)), fan, 1e-3, 1.0)
        assert r["kernel"] == name, (ftile, P, req)
        assert r["poses_per_wave"] == int(name.rstrip(">").rsplit(", ", 1)[1])
        seen.add(name)
    # the split terrain's production kernel at the benchmark's 256 poses and the default request
    assert "k_raycast_fan_xcd<0, 64, true, 8, 8, true, 8>" in seen
