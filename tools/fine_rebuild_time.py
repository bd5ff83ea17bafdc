"""Build time of the terrain's fine-window copy by DESIGN.md §6b's method: one context, the C2
terrain set again and the first query after it timed, so no allocation lies inside the figure
(tools/fine_build_time.py opens a new context per run and includes them).  The index_build
profile slot around the query that triggers the build (PCP_TERRAIN_BLOCKS=2: the first query),
minus the same slot of a second query with the copy built.  Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

os.environ["PCP_TERRAIN_BLOCKS"] = "2"
from pointcloud_processor_amd import _abi, synth  # noqa: E402

sc = synth.terrain_scene()
poses = np.array([[8.0, -3.0, 1.1, -0.5, 2.6]])
fan = _abi.fan_params(n_az=64, n_el=4)
ctx = _abi.Context(0)
ctx.profile(True)
res = []
for rep in range(8):
    ctx.set_terrain(sc.terrain, point_step=32)
    ctx.profile_reset()
    ctx.raycast_fan(poses, fan)          # builds the fine copy, then marches
    ms, _ = ctx.profile_get("index_build")
    ctx.profile_reset()
    ctx.raycast_fan(poses, fan)
    ms2, _ = ctx.profile_get("index_build")
    if rep:                              # the first build allocates
        res.append(ms - ms2)
info = ctx.terrain_info()
ctx.close()
print(json.dumps({"what": "fine-window copy rebuild on one context (no allocation), C2 terrain",
                  "ms_runs": res, "ms_median": float(np.median(res)), "ms_min": min(res),
                  "scan_layout": info["scan_layout"], "fine_tile": info["fine_tile"]}))
