#!/usr/bin/env python3
"""Timing of pcp_simulate_scan against its yardstick (not part of the suite).

Workload: the 1M-point synthetic terrain, the 1024 x 256 fan, 16 poses spread over the candidate
lattice.  Recorded:
  * pcp_simulate_scan_burst: the fan kernel per launch and the resolve phase (clears, wave-base
    scan, k_scan_resolve, mask counts) per repetition, medians of --bursts bursts of --reps;
  * the yardstick: the PARENT commit's fan kernel time for the same query -- pcp_raycast_fan_burst
    on a build of the parent (--parent-lib, run in a child process through plain ctypes: the
    parent has no pcp_simulate_scan).  The bar: resolve phase <= that fan time;
  * the call's wall time (records + mask, no dense images), and what a caller had to do before
    for the same returns: pcp_raycast_fan(first_hit) plus the NumPy resolve on the host
    (tests/scan_ref.py, which also checks the device's records against it at this size).

  python tools/scan_timing.py --parent-lib PATH/libpcp.so --parent-commit SHA --commit SHA
                              [--out profiles/scan_timing.json]
"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

N_AZ, N_EL, N_POSES = 1024, 256, 16


def med(v):
    return float(statistics.median(v))


def yardstick(lib_path, poses_file, reps, bursts):
    """pcp_raycast_fan_burst of another build of libpcp.so (the ABI's own structs only)."""
    from pointcloud_processor_amd import _abi, synth

    lib = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    P = C.c_void_p
    lib.pcp_create.argtypes = [C.c_int, C.POINTER(P)]
    lib.pcp_set_terrain.argtypes = [P, C.POINTER(_abi.CloudView)]
    lib.pcp_raycast_fan_burst.argtypes = [P, P, C.c_uint64, C.POINTER(_abi.FanParams), C.c_int,
                                          C.POINTER(C.c_double)]
    lib.pcp_destroy.argtypes = [P]
    lib.pcp_destroy.restype = None
    scene = synth.terrain_scene()
    poses = np.ascontiguousarray(np.load(poses_file), np.float64)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    h = P()
    assert lib.pcp_create(0, C.byref(h)) == 0
    terr = np.ascontiguousarray(scene.terrain)
    view = _abi.cloud_view(terr, point_step=32)
    assert lib.pcp_set_terrain(h, C.byref(view)) == 0
    out = []
    ms = C.c_double()
    for i in range(bursts + 2):   # (the second query builds the fine copy: two warm-up bursts)
        assert lib.pcp_raycast_fan_burst(h, poses.ctypes.data_as(P), poses.shape[0],
                                         C.byref(fan), reps, C.byref(ms)) == 0
        if i >= 2:
            out.append(ms.value)
    lib.pcp_destroy(h)
    print(json.dumps({"fan_ms": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scan_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick-child", nargs=2, metavar=("LIB", "POSES.npy"), default=None)
    a = ap.parse_args()
    if a.yardstick_child:
        yardstick(a.yardstick_child[0], a.yardstick_child[1], a.reps, a.bursts)
        return

    import pyoracle
    import scan_ref

    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    res = {"terrain_points": int(scene.terrain.shape[0]), "fan": [N_AZ, N_EL], "poses": N_POSES,
           "reps": a.reps, "bursts": a.bursts, "calls": a.calls,
           "commit": a.commit, "parent_commit": a.parent_commit}
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        poses = np.ascontiguousarray(cand[:: max(cand.shape[0] // N_POSES, 1)][:N_POSES])
        assert poses.shape[0] == N_POSES
        fan_ms, res_ms, own_fan = [], [], []
        for i in range(a.bursts + 2):
            f, r = ctx.simulate_scan_burst(poses, fan, a.reps)
            o = ctx.raycast_fan_burst(poses, fan, a.reps)
            if i >= 2:
                fan_ms.append(f)
                res_ms.append(r)
                own_fan.append(o)
        res["measured_on_commit"] = {
            "scan_burst_fan_kernel_ms": med(fan_ms),
            "scan_burst_fan_kernel_ms_min_max": [min(fan_ms), max(fan_ms)],
            "resolve_phase_ms": med(res_ms),
            "resolve_phase_ms_min_max": [min(res_ms), max(res_ms)],
            "raycast_fan_burst_ms": med(own_fan)}

        def wall_of(fn, calls=a.calls, warmup=a.warmup):
            w = []
            for i in range(warmup + calls):
                t0 = time.perf_counter()
                fn()
                if i >= warmup:
                    w.append((time.perf_counter() - t0) * 1e3)
            return med(w)

        got = ctx.simulate_scan(poses, fan)
        res["returns"] = int(got["n_returns"])
        res["seen_any"] = int(got["n_seen_any"])
        m = res["measured_on_commit"]
        m["simulate_scan_wall_ms"] = wall_of(lambda: ctx.simulate_scan(poses, fan))
        m["simulate_scan_wall_ms_no_mask"] = wall_of(
            lambda: ctx.simulate_scan(poses, fan, want_mask=False))
        m["raycast_fan_first_hit_wall_ms"] = wall_of(
            lambda: ctx.raycast_fan(poses, fan, want_first_hit=True))
        # before: the first hits to the host and the radius search redone there
        _, _, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
        t0 = time.perf_counter()
        ref = scan_ref.resolve(pyoracle, scene.terrain, poses, fan, fh)
        m["host_numpy_resolve_ms"] = (time.perf_counter() - t0) * 1e3
        m["before_total_wall_ms"] = m["raycast_fan_first_hit_wall_ms"] + m["host_numpy_resolve_ms"]
        scan_ref.assert_scan_equal(got, ref, dense=False)
        res["device_equals_host_resolve"] = True
    if a.parent_lib:
        pf = Path(a.out).with_suffix(".poses.npy")
        np.save(pf, poses)
        try:
            out = subprocess.run([sys.executable, __file__, "--yardstick-child", a.parent_lib,
                                  str(pf), "--reps", str(a.reps), "--bursts", str(a.bursts)],
                                 check=True, capture_output=True, text=True).stdout
        finally:
            pf.unlink()
        y = json.loads(out.strip().splitlines()[-1])["fan_ms"]
        res["measured_on_parent_commit"] = {"raycast_fan_burst_ms": med(y),
                                            "raycast_fan_burst_ms_min_max": [min(y), max(y)]}
        res["bar"] = "resolve_phase_ms <= the parent's raycast_fan_burst_ms"
        res["bar_met"] = bool(m["resolve_phase_ms"] <= med(y))
        res["resolve_to_parent_fan_ratio"] = m["resolve_phase_ms"] / med(y)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
