"""pcp_walk_pair.hpp (the fan march's paired walk: two packed window entries per trip, DESIGN.md
§6b "round trips") on the CPU: the header has no HIP dependency, so
tests/native/walk_pair_selftest.cpp is built with the host compiler and run as a stand-alone
program, no GPU call.  It compares the paired walk with the one-entry walk -- answer, last entry
tested, tests -- over runs of 0..5 and more entries, odd and even starts, hits and exits in either
slot and starts on a sentinel, the last run at the end of an array of exactly nent * 12 + 16
bytes, where the program checks the bytes each walk touched itself.  (The library Makefile's asan
target builds and runs the same program under AddressSanitizer as well.)"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"


def test_paired_walk_is_the_single_walk(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "walk_pair_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "walk_pair_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)
