"""MobileLidarPlacement (csrc/host/pcp_placement.cpp) on the CPU: what its five
methods hand to the C ABI, what they make of the answers, and the five logs, byte for byte.
tests/native/placement_host_selftest.cpp is linked from pcp_nodes.cpp, pcp_placement.cpp, the
shell tests' mock_pcp.cpp and its own recording pcp_place_* entry points (no libpcp.so), built
with ASan and UBSan and run as a stand-alone program.  tests/golden/placement_host.txt is that
program's output as recorded before the host layers were consolidated; it is a characterisation
and is not to be regenerated from the code it checks."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "pointcloud_processor_amd" / "csrc" / "host"


def test_placement_marshalling_results_and_logs_match_the_recording(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "placement_host_selftest"
    # -static-libasan: the runtime is part of the program, whatever else the loader brings first
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-Wextra",
                    f"-I{ROOT / 'include'}", f"-I{HOST}",
                    str(ROOT / "tests" / "native" / "placement_host_selftest.cpp"),
                    str(HOST / "pcp_nodes.cpp"), str(HOST / "pcp_placement.cpp"),
                    str(ROOT / "tests" / "ros_stub" / "mock_pcp.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r =subprocess.run([str(exe)], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-4000:])
    golden = (ROOT / "tests" / "golden" / "placement_host.txt").read_bytes()
    if r.stdout != golden:
        got, want = r.stdout.splitlines(), golden.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b),
                     min(len(got), len(want)))
        raise AssertionError(
            f"output differs from tests/golden/placement_host.txt at line {first + 1}: "
            f"got {got[first:first + 1]}, recorded {want[first:first + 1]} "
            f"({len(got)} lines against {len(want)})")
