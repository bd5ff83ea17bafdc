"""pcp_knobs.hpp (the context's environment variables: one table of name, field and rule) on the
CPU: the header has no HIP dependency, so tests/native/knobs_selftest.cpp is built with the host
compiler and run as a stand-alone program, no GPU call.  The program checks every default and
every rule over fake environments and prints the table's variable names; here each name must be
documented in INTEGRATION.md, and the table must be the only place of the library that reads the
environment (PCP_ALLOC_TRACE apart, which is process-wide)."""
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
    exe = tmp_path_factory.mktemp("knobs") / "knobs_selftest"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "knobs_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-4000:], r.stderr)
    return r.stdout.splitlines()


def _names(lines):
    return [ln.split()[1] for ln in lines if ln.startswith("var ")]


def test_rules_and_defaults(selftest_out):
    m = re.fullmatch(r"(\d+) checks, 0 failures", selftest_out[-2])
    assert m and int(m.group(1)) > 300, selftest_out[-2]
    names = _names(selftest_out)
    assert len(names) == len(set(names)) == 37
    assert all(re.fullmatch(r"PCP_[A-Z0-9_]+", n) for n in names)


def test_every_variable_is_documented(selftest_out):
    doc = (ROOT / "INTEGRATION.md").read_text()
    missing = [n for n in _names(selftest_out) if f"`{n}`" not in doc]
    assert not missing, missing


def test_the_table_alone_reads_the_environment(selftest_out):
    # the library's sources (the CLI under csrc/host has variables of its own)
    srcs = [f for pat in ("*.hip", "*.hpp", "*.h") for f in sorted(CSRC.glob(pat))]
    assert len(srcs) > 30
    read = [(f.name, v) for f in srcs
            for v in re.findall(r'getenv\(\s*"(PCP_\w*)', f.read_text())]
    assert read == [("pcp_context.hip", "PCP_ALLOC_TRACE")], read
    # a table's name is written once in the whole library's code (comments aside)
    names = set(_names(selftest_out))
    for f in srcs:
        code = re.sub(r"//[^\n]*", "", f.read_text())
        quoted = [v for v in re.findall(r'"(PCP_\w+)"', code) if v in names]
        assert (sorted(quoted) == sorted(names)) if f.name == "pcp_knobs.hpp" else not quoted, \
            (f.name, quoted)
    # and the header reaches the environment through its `get` argument only
    assert "getenv" not in (CSRC / "pcp_knobs.hpp").read_text()
