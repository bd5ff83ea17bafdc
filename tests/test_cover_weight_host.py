"""WeightedCoveragePlacement (csrc/host/pcp_cover_weight_node.cpp) on the CPU: what
its two methods hand to the C ABI, the box list -> bytes rule with its override order and a box
that holds no point, the rounds in weight and in points, the blind weight, the log text and the
refusal paths.  tests/native/cover_weight_host_selftest.cpp is linked from
pcp_cover_weight_node.cpp, pcp_cover_node.cpp, pcp_nodes.cpp, the shell tests' mock_pcp.cpp and its
own recording pcp_place_coverage_weighted entry points (no libpcp.so), built with ASan and UBSan
and run as a stand-alone program that checks itself.  The same methods against the real library on
the GPU: tests/test_cover_weight_cli.py."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "pointcloud_processor_amd" / "csrc" / "host"


def test_weighted_placement_marshalling_boxes_blind_weight_log_and_refusals(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "cover_weight_host_selftest"
    # -static-libasan: the runtime is part of the program, whatever else the loader brings first
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-Wextra",
                    f"-I{ROOT / 'include'}", f"-I{HOST}",
                    str(ROOT / "tests" / "native" / "cover_weight_host_selftest.cpp"),
                    str(HOST / "pcp_cover_weight_node.cpp"), str(HOST / "pcp_cover_node.cpp"),
                    str(HOST / "pcp_nodes.cpp"),
                    str(ROOT / "tests" / "ros_stub" / "mock_pcp.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, env=env, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, (r.returncode, out[-4000:], r.stderr.decode(errors="replace")[-4000:])
    assert out.strip().splitlines()[-1] == "cover_weight_host_selftest ok"


def test_the_weighted_call_stays_in_its_own_unit():
    """pcp_nodes.cpp and pcp_placement.cpp link against fixed stubs elsewhere, and a program above
    the other coverage units links without the weighted call: only pcp_cover_weight_node.cpp names
    it."""
    for name in ("pcp_nodes.cpp", "pcp_nodes.hpp", "pcp_placement.cpp", "pcp_placement.hpp",
                 "pcp_scan_node.cpp", "pcp_scan_node.hpp", "pcp_cover_node.cpp",
                 "pcp_cover_pair_node.cpp", "pcp_cover_refine_node.cpp", "pcp_cover_aim_node.cpp",
                 "pcp_cover_aim_node.hpp"):
        text = (HOST / name).read_text()
        assert "pcp_place_coverage_weighted" not in text, name
        assert '#include "pcp_cover_weight_node.hpp"' not in text, name
    for name in ("pcp_nodes.cpp", "pcp_nodes.hpp", "pcp_placement.cpp", "pcp_placement.hpp"):
        assert "pcp_cover_weight" not in (HOST / name).read_text(), name
    assert "pcp_place_coverage_weighted(" in (HOST / "pcp_cover_weight_node.cpp").read_text()
