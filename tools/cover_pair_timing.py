#!/usr/bin/env python3
"""Timing of pcp_place_coverage_pair against its yardsticks (not part of the suite).

Workload (DESIGN.md section 6m's): the 1M-point synthetic terrain, the 1024 x 256 fan, 91, 256 and
1,024 candidate poses of the candidate lattice (the lattice's 256 repeated to 1,024), the region of
interest every point and, second, the points inside the excavation grid's bounding box.

Every GPU step is a child process of its own under `timeout`, one after the other; the first step
that fails, dies or runs out of time ends the run (nothing more is started on the GPU).  Steps:
  * --step N: pcp_place_coverage_pair_burst, medians of --bursts bursts of --reps after two warm-ups
    in one process: ms[0] = the mask pass with the singles, ms[1] = the tiles and the selection.
    Beside them: the VALU issue floor of the tiles (pairs x W2 words x 4 lane-operations at 256 CUs
    x 64 lanes per clock, 2.4 GHz) and the fraction reached; the rows' bytes (n x W2 x 8) at the
    streaming rate of DESIGN.md section 6a; the whole call's wall time with its one wait;
  * --old-route (n = 91 only): the route that existed -- 91 pcp_place_coverage calls with
    fixed = [a], k_max = 1 -- on a build of the PARENT commit (--parent-lib) through plain ctypes;
    the best of g[a] + gain over a, with its (a, b), is asserted identical to the pair call's
    answer of the same run.

  python tools/cover_pair_timing.py --parent-lib PATH/libpcp.so --parent-commit SHA --commit SHA
                                    [--out profiles/cover_pair_timing.json]
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

N_AZ, N_EL = 1024, 256
SIZES = (91, 256, 1024)
STREAM_TBPS = 4.8          # what a read-once kernel streams here
LANES_PER_CLOCK = 256 * 64  # CUs x (4 SIMDs x 16 lanes)
CLOCK_GHZ = 2.4             # the shader clock's maximum
STEP_TIMEOUT_S = 240


def med(v):
    return float(statistics.median(v))


def workload():
    """-> (scene, fan, roi of the grid's box, all candidate poses [1024, 5] via ctx)."""
    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    N = int(scene.terrain.shape[0])
    bb = cells.grid_bbox
    xyz = np.ascontiguousarray(scene.terrain).view(np.float32).reshape(N, -1)[:, :3]
    roi_box = ((xyz[:, 0] >= bb[0]) & (xyz[:, 0] <= bb[1]) & (xyz[:, 1] >= bb[2]) &
               (xyz[:, 1] <= bb[3])).astype(np.uint8)
    return scene, cells, _abi.fan_params(n_az=N_AZ, n_el=N_EL), roi_box


def step(n, a):
    """One size in one process -> a JSON line."""
    from pointcloud_processor_amd import _abi

    scene, cells, fan, roi_box = workload()
    N = int(scene.terrain.shape[0])
    W2 = ((N + 63) // 64 + 1) & ~1
    pairs = n * (n - 1) // 2
    floor_ms = pairs * W2 * 4 / (LANES_PER_CLOCK * CLOCK_GHZ * 1e9) * 1e3
    row_bytes = n * W2 * 8
    m = {"n": n, "pairs": pairs, "words_per_pose": W2, "roi_box_points": int(roi_box.sum()),
         "tiles_valu_floor_ms": floor_ms, "row_bytes": row_bytes,
         "rows_at_stream_rate_ms": row_bytes / (STREAM_TBPS * 1e12) * 1e3}
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        poses = np.ascontiguousarray(np.resize(cand, (n, 5)))
        for name, roi in (("all", None), ("grid_box", roi_box)):
            mk, tl = [], []
            for i in range(a.bursts + 2):
                ms = ctx.place_coverage_pair_burst(poses, fan, roi=roi, reps=a.reps)
                if i >= 2:
                    mk.append(ms[0])
                    tl.append(ms[1])
            w = []
            for i in range(a.warmup + a.calls):
                t0 = time.perf_counter()
                got = ctx.place_coverage_pair(poses, fan, roi=roi)
                if i >= a.warmup:
                    w.append((time.perf_counter() - t0) * 1e3)
            m[name] = {"mask_singles_ms": med(mk), "mask_singles_ms_min_max": [min(mk), max(mk)],
                       "tiles_select_ms": med(tl), "tiles_select_ms_min_max": [min(tl), max(tl)],
                       "tiles_fraction_of_valu_floor": floor_ms / med(tl),
                       "mask_fraction_of_stream_rate": m["rows_at_stream_rate_ms"] / med(mk),
                       "call_wall_ms": med(w), "call_wall_ms_min_max": [min(w), max(w)],
                       "best_pair": got["best_pair"].tolist(), "pair_gain": got["pair_gain"],
                       "best_single": got["best_single"], "single_gain": got["single_gain"],
                       "n_selected": got["n_selected"]}
        if a.poses_out:
            np.save(a.poses_out, poses)
    print(json.dumps(m))


def old_route(lib_path, poses_file, a):
    """91 greedy calls with one fixed pose each on another build of libpcp.so -> a JSON line."""
    from pointcloud_processor_amd import _abi

    scene, _, fan, _ = workload()
    lib = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    P = C.c_void_p
    lib.pcp_create.argtypes = [C.c_int, C.POINTER(P)]
    lib.pcp_set_terrain.argtypes = [P, C.POINTER(_abi.CloudView)]
    lib.pcp_place_coverage.argtypes = dict((s[0], s[2]) for s in _abi._SIGS)["pcp_place_coverage"]
    lib.pcp_destroy.argtypes = [P]
    lib.pcp_destroy.restype = None
    poses = np.ascontiguousarray(np.load(poses_file), np.float64)
    n = poses.shape[0]
    h = P()
    assert lib.pcp_create(0, C.byref(h)) == 0
    terr = np.ascontiguousarray(scene.terrain)
    view = _abi.cloud_view(terr, point_step=32)
    assert lib.pcp_set_terrain(h, C.byref(view)) == 0
    sel, gain, cov = (C.c_int64 * 16)(), (C.c_uint64 * 16)(), (C.c_uint64 * 16)()
    npts, rpts, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ns = C.c_int32()

    def route():
        best = (-1, -1, -1)
        for p in range(n):
            cp = _abi.Context._cover_params(1, 0.0, (p,), 0)
            rc = lib.pcp_place_coverage(h, poses.ctypes.data_as(P), n, C.byref(fan), C.byref(cp),
                                        None, 0, sel, gain, cov, None, None, None, 0,
                                        C.byref(npts), C.byref(rpts), C.byref(base), C.byref(ns))
            assert rc == 0, rc
            union = base.value + (gain[0] if ns.value else 0)
            if ns.value and union > best[0]:
                best = (union, p, sel[0])
        return best

    w = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        best = route()
        if i >= a.warmup:
            w.append((time.perf_counter() - t0) * 1e3)
    lib.pcp_destroy(h)
    print(json.dumps({"wall_ms": med(w), "wall_ms_min_max": [min(w), max(w)], "calls": n,
                      "pair_gain": int(best[0]), "best_pair": [int(best[1]), int(best[2])]}))


def run_child(args, what):
    """A GPU step of its own under timeout -> its last line as JSON; any other end stops the run."""
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, __file__] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"cover_pair_timing: step {what} ended with status {r.returncode}: "
                 "nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover_pair_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--poses-out", default=None)
    ap.add_argument("--old-route", nargs=2, metavar=("LIB", "POSES.npy"), default=None)
    a = ap.parse_args()
    if a.step is not None:
        step(a.step, a)
        return
    if a.old_route:
        old_route(a.old_route[0], a.old_route[1], a)
        return
    common = ["--reps", str(a.reps), "--bursts", str(a.bursts), "--calls", str(a.calls),
              "--warmup", str(a.warmup)]
    res = {"fan": [N_AZ, N_EL], "reps": a.reps, "bursts": a.bursts, "calls": a.calls,
           "commit": a.commit, "parent_commit": a.parent_commit, "stream_rate_tbps": STREAM_TBPS,
           "valu_lanes_per_clock": LANES_PER_CLOCK, "clock_ghz": CLOCK_GHZ, "sizes": {},
           "not_measured": ["PMC counters (VALU busy, LDS bank conflicts, atomics)",
                            "the mounted twin", "a separation or fixed sensors at these sizes"]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pf = Path(a.out).with_suffix(".poses.npy")
    try:
        for n in SIZES:
            extra = ["--poses-out", str(pf)] if n == SIZES[0] and a.parent_lib else []
            res["sizes"][str(n)] = run_child(["--step", str(n)] + common + extra, f"n={n}")
        if a.parent_lib:
            o = run_child(["--old-route", a.parent_lib, str(pf)] + common, "old route")
            m = res["sizes"][str(SIZES[0])]
            assert o["pair_gain"] == m["all"]["pair_gain"], (o, m["all"])
            assert o["best_pair"] == m["all"]["best_pair"], (o, m["all"])
            m["old_route"] = dict(o, answers_identical=True,
                                  speedup_of_the_pair_call=o["wall_ms"] / m["all"]["call_wall_ms"])
    finally:
        if pf.exists():
            pf.unlink()
    res["host_waits_per_call"] = "one: a single stream synchronisation behind the call's last copy"
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
