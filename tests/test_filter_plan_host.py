"""pcp_filter_plan.hpp (which voxel chain a filter call runs, its fallback order and the chains'
sizes) on the CPU: the header has no HIP dependency, so
tests/native/filter_plan_selftest.cpp is built with the host compiler and run as a stand-alone
program, no GPU call.  The program compares filter_plan() with the decision code it replaced and
the geometries with the functions they replaced."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"


@pytest.fixture(scope="module")
def selftest_out(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("filter_plan") / "filter_plan_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "filter_plan_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-4000:], r.stderr)
    return r.stdout.splitlines()


def _counts(selftest_out):
    m = re.fullmatch(r"(\d+) plan cases, (\d+) geometry cases, (\d+) mismatches",
                     selftest_out[-2])
    assert m, selftest_out[-2]
    return tuple(map(int, m.groups()))


def test_plan_is_the_replaced_decision_code(selftest_out):
    # the full product of the module comment of filter_plan_selftest.cpp: entries x fm_fast x
    # eight yes / no inputs x clouds x certainty, bucket and fast patterns
    plan_cases, _, mismatches = _counts(selftest_out)
    assert plan_cases == 5 * 3 * 2 ** 8 * 5 * 3 * 5 * 5
    assert mismatches == 0


def test_geometries_are_the_replaced_functions(selftest_out):
    # boxes() x n {6}: the passes and the certainty test, x clouds {2} x CUs {2}: the fast
    # geometry, x bk_gt {4} x bk_pts {3}: the bucket geometry
    _, geo_cases, mismatches = _counts(selftest_out)
    boxes = 4 + 5 + 2 * 8 + 2 * 7
    assert geo_cases == boxes * 6 * (1 + 2 * 2 * (1 + 4 * 3))
    assert mismatches == 0


def test_benchmark_frames_take_the_production_geometry(selftest_out):
    # C3's and C1's box at both leaves, one and two clouds, 256 CUs: three radix passes, both
    # geometries available; the two-cloud C3 frame packs 14 crop tiles per bucket group
    rows = [ln for ln in selftest_out if ln.startswith("bench ")]
    assert len(rows) == 4
    for ln in rows:
        assert "passes 3, fast ok 1 passes 3" in ln and "bucket ok 1" in ln, ln
    assert "bucket ok 1 gt 14 ng 88" in rows[1]
