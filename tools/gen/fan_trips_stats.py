#!/usr/bin/env python3
"""Generates tests/golden/fan_trips_stats.json: pcp_raycast_fan_stats -- the march's probes, walk
starts, point tests and directory loads -- of every walk case of tests/test_fan_trips.py
(tests/fan_trips_cases.py, WALK_CASES), recorded from the build that PCP_LIB names (the parent
commit's library; default: this tree's).  Needs a GPU.

    PCP_LIB=/path/to/parent/libpcp.so python3 tools/gen/fan_trips_stats.py COMMIT [OUT]
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import fan_trips_cases as cases  # noqa: E402
from pointcloud_processor_amd import _abi  # noqa: E402


def main():
    commit = sys.argv[1]
    golden = ROOT / "tests" / "golden" / "fan_trips_stats.json"
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else golden
    os.environ["PCP_TERRAIN_BLOCKS"] = "2"
    doc = {"what": "pcp_raycast_fan_stats of the walk cases of tests/test_fan_trips.py "
                   "(tests/fan_trips_cases.py, WALK_CASES), recorded from the parent build: the "
                   "march's probes, walk starts, point tests and directory loads",
           "commit": commit,
           "terrain": "fan_trips_cases.SCENES, PCP_TERRAIN_BLOCKS=2, point_step=32; far: x, y, z "
                      "+ 3000 (float32)",
           "fan": "64 x 8, el -85 .. 85 degrees, max_distance 15.0",
           "cases": {}}
    for name in sorted(cases.WALK_CASES):
        terrain, poses, fan = cases.walk_case(name)
        scene, n, far = cases.WALK_CASES[name]
        with _abi.Context(0) as ctx:
            ctx.set_terrain(terrain, point_step=32)
            ctx.raycast_fan(poses, fan)   # (the first query builds the fine copy)
            assert ctx.terrain_info()["scan_layout"] == "fine"
            st = ctx.raycast_fan_stats(np.ascontiguousarray(poses, np.float64), fan)
        doc["cases"][name] = {"scene": scene, "poses": f"aimed_poses(points, {n}, fan)",
                              "far": far, "stats": st}
        print(name, st)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
