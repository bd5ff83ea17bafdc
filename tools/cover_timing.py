#!/usr/bin/env python3
"""Timing of pcp_place_coverage against its yardsticks (not part of the suite).

Workload: the 1M-point synthetic terrain, the 1024 x 256 fan, 91 and 256 candidate poses of the
candidate lattice, k_max = 8, the region of interest every point; a second run with the region =
the points inside the excavation grid's bounding box.  Recorded, medians of --bursts bursts:
  * the fan: pcp_place_coverage_burst's ms[0] against pcp_raycast_fan_burst of the same query on a
    build of the PARENT commit (--parent-lib, run in a child process through plain ctypes);
  * the resolve: ms[1] per pose against pcp_simulate_scan_burst's resolve phase per pose (64 poses,
    the scan's limit), re-measured in the same run; the ratio is stated, no bar is fixed;
  * a round: ms[2] against the bytes it must read -- alive poses x W x 8 B -- at the streaming
    rate the project measures for a read-once kernel (DESIGN.md section 6a, 4.8 TB/s); the fraction
    is stated, no bar is fixed;
  * the whole call's wall time against the route that exists without it, timed in the same run:
    ceil(n / 64) pcp_simulate_scan calls for the masks only, then the greedy in NumPy.  The two
    answers must be identical: selected, gain and the owners are asserted equal.

  python tools/cover_timing.py --parent-lib PATH/libpcp.so --parent-commit SHA --commit SHA
                               [--out profiles/cover_timing.json]
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

N_AZ, N_EL, K_MAX = 1024, 256, 8
SIZES = (91, 256)
STREAM_TBPS = 4.8   # what a read-once kernel streams here


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
    allp = np.ascontiguousarray(np.load(poses_file), np.float64)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    h = P()
    assert lib.pcp_create(0, C.byref(h)) == 0
    terr = np.ascontiguousarray(scene.terrain)
    view = _abi.cloud_view(terr, point_step=32)
    assert lib.pcp_set_terrain(h, C.byref(view)) == 0
    out = {}
    ms = C.c_double()
    for n in SIZES:
        poses = np.ascontiguousarray(allp[:n])
        v = []
        for i in range(bursts + 2):   # (the second query builds the fine copy: two warm-ups)
            assert lib.pcp_raycast_fan_burst(h, poses.ctypes.data_as(P), n, C.byref(fan), reps,
                                             C.byref(ms)) == 0
            if i >= 2:
                v.append(ms.value)
        out[str(n)] = v
    lib.pcp_destroy(h)
    print(json.dumps({"fan_ms": out}))


def numpy_greedy(masks, k_max):
    """The route that exists without the call: greedy set cover over the scans' 64-bit masks (one
    mask array per chunk of 64 poses) -> (selected, gain, owner)."""
    N = masks[0].shape[0]
    rows = []
    for m in masks:
        bits = np.unpackbits(m.view(np.uint8).reshape(N, 8), axis=1, bitorder="little")
        rows.append(bits.T.astype(bool))
    seen = np.concatenate(rows)          # [64 * chunks, N]
    need = np.ones(N, bool)
    owner = np.full(N, -2, np.int32)
    alive = np.ones(seen.shape[0], bool)
    sel, gain = [], []
    for r in range(k_max):
        g = np.where(alive, (seen & need).sum(axis=1), -1)
        b = int(np.argmax(g))
        if g[b] <= 0:
            break
        sel.append(b)
        gain.append(int(g[b]))
        hit = seen[b] & need
        owner[hit] = r
        need &= ~hit
        alive[b] = False
    return sel, gain, owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-child", nargs=2, metavar=("LIB", "POSES.npy"), default=None)
    a = ap.parse_args()
    if a.yardstick_child:
        yardstick(a.yardstick_child[0], a.yardstick_child[1], a.reps, a.bursts)
        return

    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    N = int(scene.terrain.shape[0])
    W = (N + 63) // 64
    bb = cells.grid_bbox
    xyz = np.ascontiguousarray(scene.terrain).view(np.float32).reshape(N, -1)[:, :3]
    roi_box = ((xyz[:, 0] >= bb[0]) & (xyz[:, 0] <= bb[1]) & (xyz[:, 1] >= bb[2]) &
               (xyz[:, 1] <= bb[3])).astype(np.uint8)
    res = {"terrain_points": N, "fan": [N_AZ, N_EL], "k_max": K_MAX, "words_per_pose": W,
           "reps": a.reps, "bursts": a.bursts, "calls": a.calls, "commit": a.commit,
           "parent_commit": a.parent_commit, "stream_rate_tbps": STREAM_TBPS,
           "roi_box_points": int(roi_box.sum()), "sizes": {}}

    def wall_of(fn):
        w = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                w.append((time.perf_counter() - t0) * 1e3)
        return med(w)

    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        allp = np.ascontiguousarray(np.resize(cand, (max(SIZES), 5)))
        # the scan's resolve per pose, at the scan's limit of 64 poses
        scan_res = []
        for i in range(a.bursts + 2):
            _, r = ctx.simulate_scan_burst(allp[:64], fan, a.reps)
            if i >= 2:
                scan_res.append(r)
        res["scan_resolve_ms_per_pose"] = med(scan_res) / 64
        for n in SIZES:
            poses = np.ascontiguousarray(allp[:n])
            m = {}
            for name, roi in (("all", None), ("grid_box", roi_box)):
                f, b, r = [], [], []
                for i in range(a.bursts + 2):
                    ms = ctx.place_coverage_burst(poses, fan, K_MAX, roi=roi, reps=a.reps)
                    if i >= 2:
                        f.append(ms[0])
                        b.append(ms[1])
                        r.append(ms[2])
                bytes_round = n * W * 8
                floor_ms = bytes_round / (STREAM_TBPS * 1e12) * 1e3
                m[name] = {"fan_kernel_ms": med(f), "fan_kernel_ms_min_max": [min(f), max(f)],
                           "bitset_phase_ms": med(b), "bitset_phase_ms_per_pose": med(b) / n,
                           "resolve_per_pose_ratio_to_scan":
                               med(b) / n / res["scan_resolve_ms_per_pose"],
                           "round_ms": med(r), "round_bytes": bytes_round,
                           "round_stream_floor_ms": floor_ms,
                           "round_fraction_of_stream_rate": floor_ms / med(r)}
            got = ctx.place_coverage(poses, fan, K_MAX, want_owner=True)
            m["call_wall_ms"] = wall_of(lambda: ctx.place_coverage(poses, fan, K_MAX))
            m["call_wall_ms_with_owner"] = wall_of(
                lambda: ctx.place_coverage(poses, fan, K_MAX, want_owner=True))
            m["call_wall_ms_grid_box"] = wall_of(
                lambda: ctx.place_coverage(poses, fan, K_MAX, roi=roi_box))

            # the route that exists without the call: chunks of 64 scans (masks only), NumPy greedy
            def old_route():
                masks = []
                for lo in range(0, n, 64):
                    try:
                        s = ctx.simulate_scan(poses[lo:lo + 64], fan, returns_cap=0)
                    except _abi.PcpError as e:   # (no room for records: the mask is valid)
                        s = e.partial
                    masks.append(s["point_mask"].copy())
                return numpy_greedy(masks, K_MAX)

            t0 = time.perf_counter()
            sel, gain, owner = old_route()
            m["scan_chunks_numpy_greedy_wall_ms"] = (time.perf_counter() - t0) * 1e3
            assert got["selected"].tolist() == sel, (got["selected"].tolist(), sel)
            assert got["gain"].tolist() == gain
            assert np.array_equal(got["point_owner"], owner)
            m["answers_identical"] = True
            m["selected"] = sel
            m["gain"] = gain
            m["speedup_over_scan_chunks"] = (m["scan_chunks_numpy_greedy_wall_ms"] /
                                             m["call_wall_ms_with_owner"])
            res["sizes"][str(n)] = m
    res["host_waits_per_call"] = ("one: the call's path holds a single stream synchronisation "
                                  "(stream_done) behind its last copy; a change of the fan or step "
                                  "tables adds the fan query's own upload wait, as for every fan call")
    if a.parent_lib:
        pf = Path(a.out).with_suffix(".poses.npy")
        np.save(pf, allp)
        try:
            out = subprocess.run([sys.executable, __file__, "--yardstick-child", a.parent_lib,
                                  str(pf), "--reps", str(a.reps), "--bursts", str(a.bursts)],
                                 check=True, capture_output=True, text=True).stdout
        finally:
            pf.unlink()
        y = json.loads(out.strip().splitlines()[-1])["fan_ms"]
        for n in SIZES:
            res["sizes"][str(n)]["parent_raycast_fan_burst_ms"] = med(y[str(n)])
            res["sizes"][str(n)]["parent_raycast_fan_burst_ms_min_max"] = [min(y[str(n)]),
                                                                           max(y[str(n)])]
            res["sizes"][str(n)]["fan_ratio_to_parent"] = (
                res["sizes"][str(n)]["all"]["fan_kernel_ms"] / med(y[str(n)]))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
