#!/usr/bin/env python3
"""Timing of the mounted fan and scan against their yardstick (not part of the suite).

Workload: the scan timing's (tools/scan_timing.py) -- the 1M-point synthetic terrain, the
1024 x 256 fan, 16 poses spread over the candidate lattice.  Recorded, medians of --bursts bursts
of --reps launches with their minimum and maximum:
  * the yardstick: the PARENT commit's pcp_raycast_fan_burst for those poses, on a build of the
    parent (--parent-lib, run in a child process through plain ctypes), and its own run-to-run
    spread (max - min over the bursts, relative to the median);
  * this tree's pcp_raycast_fan_burst (the level fan: meant to be the same device code);
  * pcp_raycast_fan_mounted_burst at zero tilt -- the same rays, so the ratio to the yardstick is
    the price of the rotation plus the lost ring liveness (Skip 4) -- and with every pose pitched
    -0.4363 rad (the zx120 Velodyne's mount);
  * the resolve phase both ways: pcp_simulate_scan_burst and pcp_simulate_scan_mounted_burst.

  python tools/mount_timing.py --parent-lib PATH/libpcp.so --parent-commit SHA --commit SHA
                               [--out profiles/mount_timing.json]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

N_AZ, N_EL, N_POSES = 1024, 256, 16
PITCH = -0.4363


def stat(v):
    m = float(statistics.median(v))
    return {"median_ms": m, "min_ms": float(min(v)), "max_ms": float(max(v)),
            "spread": float((max(v) - min(v)) / m) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mount_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bursts", type=int, default=7)
    a = ap.parse_args()

    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    res = {"terrain_points": int(scene.terrain.shape[0]), "fan": [N_AZ, N_EL], "poses": N_POSES,
           "reps": a.reps, "bursts": a.bursts, "pitch": PITCH, "commit": a.commit,
           "parent_commit": a.parent_commit}

    def bursts_of(fn):
        out = []
        for i in range(a.bursts + 2):   # (the second query builds the fine copy: two warm-ups)
            v = fn()
            if i >= 2:
                out.append(v)
        return out

    m = res["measured_on_commit"] = {}
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        poses = np.ascontiguousarray(cand[:: max(cand.shape[0] // N_POSES, 1)][:N_POSES])
        assert poses.shape[0] == N_POSES
        z = np.zeros(N_POSES)
        level6 = np.ascontiguousarray(np.column_stack([poses[:, :3], z, z, poses[:, 4]]))
        tilt6 = level6.copy()
        tilt6[:, 4] = PITCH
        m["raycast_fan_burst"] = stat(bursts_of(lambda: ctx.raycast_fan_burst(poses, fan, a.reps)))
        lv = bursts_of(lambda: ctx.simulate_scan_burst(poses, fan, a.reps))
        m["resolve_phase_level"] = stat([r for _, r in lv])
        # the zero-tilt mounted query is the level one (checked here at full size)
        lb, lu, _, _ = ctx.raycast_fan(poses, fan)
        mb, mu, _, _ = ctx.raycast_fan_mounted(level6, fan)
        res["zero_tilt_equals_level"] = bool(np.array_equal(lb, mb) and np.array_equal(lu, mu))
        tb, _, _, _ = ctx.raycast_fan_mounted(tilt6, fan)
        res["blocked_rays"] = {"level": int(lb.sum()), "pitched": int(tb.sum())}
        m["mounted_zero_tilt"] = stat(bursts_of(
            lambda: ctx.raycast_fan_mounted_burst(level6, fan, None, a.reps)))
        m["mounted_pitched"] = stat(bursts_of(
            lambda: ctx.raycast_fan_mounted_burst(tilt6, fan, None, a.reps)))
        z0 = bursts_of(lambda: ctx.simulate_scan_mounted_burst(level6, fan, None, a.reps))
        zp = bursts_of(lambda: ctx.simulate_scan_mounted_burst(tilt6, fan, None, a.reps))
        m["resolve_phase_mounted_zero_tilt"] = stat([r for _, r in z0])
        m["resolve_phase_mounted_pitched"] = stat([r for _, r in zp])
    if a.parent_lib:
        pf = Path(a.out).with_suffix(".poses.npy")
        np.save(pf, poses)
        try:
            out = subprocess.run([sys.executable, str(ROOT / "tools" / "scan_timing.py"),
                                  "--yardstick-child", a.parent_lib, str(pf), "--reps",
                                  str(a.reps), "--bursts", str(a.bursts)],
                                 check=True, capture_output=True, text=True).stdout
        finally:
            pf.unlink()
        y = stat(json.loads(out.strip().splitlines()[-1])["fan_ms"])
        res["measured_on_parent_commit"] = {"raycast_fan_burst": y}
        ym = y["median_ms"]
        res["ratios_to_parent_fan"] = {k: v["median_ms"] / ym for k, v in m.items()
                                       if not k.startswith("resolve")}
        res["resolve_mounted_to_level"] = {
            "zero_tilt": m["resolve_phase_mounted_zero_tilt"]["median_ms"] /
            m["resolve_phase_level"]["median_ms"],
            "pitched": m["resolve_phase_mounted_pitched"]["median_ms"] /
            m["resolve_phase_level"]["median_ms"]}
        res["yardstick_spread"] = y["spread"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
