#!/usr/bin/env python3
"""Compares the gfx950 device code of two checkouts kernel by kernel.

Every .hip source of pointcloud_processor_amd/csrc is compiled in both trees with the Makefile's
FLAGS plus --cuda-device-only -S (cross-compiles without a GPU); a kernel's body is its listing
from its label to its .Lfunc_end, comments and the source's own directory stripped.  Prints one
line per source with the kernels whose instructions differ, and for those the compiler's
resource-usage figures of both trees.

    python3 tools/device_code_diff.py PARENT_TREE [THIS_TREE] > profiles/..._device_code.txt
"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-I../../include", "-I.", "-w", "--cuda-device-only", "-S"]
PER_SOURCE = {"pcp_excav.hip": ["-fno-slp-vectorize"]}   # (the Makefile's)
FIGURES = ("NumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")


def listing(tree, src, out):
    csrc = Path(tree) / "pointcloud_processor_amd" / "csrc"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # (the Makefile's default)
    subprocess.run([hipcc] + FLAGS + PER_SOURCE.get(src, []) + [src, "-o", str(out)], cwd=csrc,
                   check=True, capture_output=True)
    kernels, name, body = {}, None, []
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            kernels[name] = {"body": body, "fig": {}}
            last, name = name, None
            continue
        code = line.split(";")[0].rstrip()
        if code.strip() and not code.strip().startswith("."):
            body.append(code)
        elif re.match(r"^\.LBB", code):
            body.append(code)
    # the resource figures follow each function as comments
    cur = None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and cur in kernels and m.group(1) in FIGURES:
            kernels[cur]["fig"].setdefault(m.group(1), int(m.group(2)))
    return kernels


def main():
    parent = sys.argv[1]
    here = sys.argv[2] if len(sys.argv) > 2 else str(Path(__file__).resolve().parents[1])
    srcs = sorted(p.name for p in (Path(here) / "pointcloud_processor_amd" / "csrc").glob("*.hip"))
    with tempfile.TemporaryDirectory() as tmp:
        for src in srcs:
            if not (Path(parent) / "pointcloud_processor_amd" / "csrc" / src).exists():
                print(f"{src}: not in the parent")
                continue
            a = listing(parent, src, Path(tmp) / "a.s")
            b = listing(here, src, Path(tmp) / "b.s")
            diff = [k for k in b if k not in a or a[k]["body"] != b[k]["body"]]
            gone = [k for k in a if k not in b]
            print(f"{src}: {len(b)} kernels, {len(b) - len(diff)} identical instruction for "
                  f"instruction, {len(diff)} differ, {len(gone)} only in the parent")
            for k in diff:
                fa = a[k]["fig"] if k in a else {}
                print(f"  differs: {k}")
                print("    " + ", ".join(f"{f} {fa.get(f, '-')} -> {b[k]['fig'].get(f, '-')}"
                                         for f in FIGURES) +
                      f", lines {len(a[k]['body']) if k in a else '-'} -> {len(b[k]['body'])}")
            for k in gone:
                print(f"  only in the parent: {k}")


if __name__ == "__main__":
    main()
