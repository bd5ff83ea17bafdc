"""pcp_place_shared.hpp (what pcp_place.hip, pcp_pairs.hip, pcp_triples.hip, pcp_refine.hip and
pcp_aim.hip share) on the CPU: its first part has no HIP dependency, so
tests/native/place_shared_selftest.cpp is built with the host compiler and run as a stand-alone
program, no GPU call."""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"


def test_first_maximum_index_list_and_layout(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "place_shared_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "place_shared_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)


def test_walk_constants_are_what_the_gpu_tests_assume():
    """tests/test_place_pair.py and tests/test_place_refine.py take their cell counts around the
    staged chunk; tools/refine_timing.py and tools/pair_timing.py state the tiles."""
    src = (CSRC / "pcp_place_shared.hpp").read_text()
    assert int(re.search(r"constexpr int kWalkC = (\d+);", src).group(1)) == 64
    assert int(re.search(r"constexpr int kWalkG = (\d+);", src).group(1)) == 4
