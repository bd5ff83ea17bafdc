"""pcp_triple_tiles.hpp (the triple search's tile arithmetic) on the CPU: the header
has no HIP dependency, so tests/native/triple_tiles_selftest.cpp is built with the host compiler
under UBSan and run as a stand-alone program, no GPU call."""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"


def test_tile_mapping_and_ownership(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "triple_tiles_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "triple_tiles_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)


def test_tile_edge_is_what_the_gpu_tests_assume():
    """tests/test_place_triple.py takes its pose counts around the tile edge T and its cell counts
    around the staged chunk."""
    src = (CSRC / "pcp_triple_tiles.hpp").read_text()
    assert re.search(r"constexpr int kTripleTile = kPairTile;", src)
    pair = (CSRC / "pcp_pair_tiles.hpp").read_text()
    assert int(re.search(r"constexpr int kPairTile = (\d+);", pair).group(1)) == 16
    shared = (CSRC / "pcp_place_shared.hpp").read_text()
    assert int(re.search(r"constexpr int kWalkC = (\d+);", shared).group(1)) == 64
    # the chains per lane divide the tile: whole A groups, one block each
    ta = int(re.search(r"#define PCP_TRIPLE_TA (\d+)", src).group(1))
    assert ta in (1, 2, 4, 8, 16)
