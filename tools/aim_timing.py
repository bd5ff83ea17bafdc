#!/usr/bin/env python3
"""Timing of pcp_place_aimed against its yardsticks (not part of the suite).

Workload: the synthetic tick's cells with its 91 candidates and 45 aims (the aims the call was
specified with), and with 256 candidates and 64 aims.  In one process, medians after a warm-up:
  * the device time of one round (pcp_place_aimed_burst: every (pose, aim) row's total and the
    last block's selection);
  * the condition set in advance, at (91, 45): a round takes less device time than 45
    pcp_place_sensors rounds at P = 91 (PCP_K_PLACE per launch, measured here) -- what asking the
    existing kernel once per aim would cost if it could mask at all;
  * the whole call's wall time (three sensors, one wait);
  * the route to the same answer before the call existed: pcp_score_matrix to the host plus the
    NumPy restatement (tests/aim_ref.py), predicate included;
  * two floors: the dependent f64 add (tools/mb/chain.hip, profiles/r06_chain.json) x C, a row's
    chain; and the walking wave's issue count per cell (one v_and, one v_cmp, two v_cndmask, one
    v_add_f64: 5 vector instructions of 4 cycles each for a wave alone on its SIMD) x C at an
    assumed clock of 2.4 GHz (the run does not read the clock).

  python tools/aim_timing.py [--out profiles/aim_timing.json]
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import aim_ref  # noqa: E402

from pointcloud_processor_amd import _abi  # noqa: E402
from pointcloud_processor_amd import synth  # noqa: E402
from tools.place_timing import poses_for  # noqa: E402

WALK_VALU_PER_CELL = 5    # v_and, v_cmp, 2 x v_cndmask, v_add_f64 (k_aim_round's walk)
ISSUE_CYCLES = 4          # a wave alone on its SIMD issues one vector instruction per 4 cycles
CLOCK_GHZ = 2.4          # assumed, not measured


def med(v):
    return float(statistics.median(v))


def grid_aims(n):
    return np.array([[math.radians(o), math.radians(p)] for p in (-60.0, -40.0, -20.0, 0.0)
                     for o in np.arange(-180.0, 180.0, 22.5)], np.float64)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "aim_timing.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    aux = synth.aux_cloud()
    zx = scene.zx120_pose5
    params = _abi.default_vl_params()
    C_ = int(cells.xyz.shape[0])
    add_ns = json.loads((ROOT / "profiles" / "r06_chain.json").read_text())[
        "ns_per_dependent_f64_add"]
    h, v = math.radians(90), math.radians(60)
    res = {"cells": C_, "calls": a.calls, "warmup": a.warmup, "burst_reps": a.reps,
           "h_fov_deg": 90, "v_fov_deg": 60, "dependent_f64_add_ns": add_ns,
           "floor_chain_us": add_ns * C_ * 1e-3,
           "floor_issue_us": WALK_VALU_PER_CELL * ISSUE_CYCLES / CLOCK_GHZ * C_ * 1e-3,
           "walk_valu_per_cell": WALK_VALU_PER_CELL, "assumed_clock_ghz": CLOCK_GHZ, "shapes": {}}

    def wall_of(fn, calls=None):
        w = []
        for i in range(a.warmup + (calls or a.calls)):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if i >= a.warmup:
                w.append((t1 - t0) * 1e3)
        return med(w)

    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        for P, A in ((91, 45), (256, 64)):
            poses = (np.ascontiguousarray(ctx.generate_candidates(cells.grid_bbox, params, zx))
                     if P == 91 else poses_for(ctx, cells.grid_bbox, zx, P))
            assert poses.shape[0] == P
            aims = aim_ref.tick_aims() if A == 45 else grid_aims(A)
            r = {}
            burst = [ctx.place_aimed_burst(poses, zx, params, aims, h, v, reps=a.reps) * 1e3
                     for _ in range(a.warmup + a.calls)][a.warmup:]
            r["round_us"] = med(burst)
            r["round_us_min_max"] = [min(burst), max(burst)]
            # the existing kernel's round at the same P, in this process
            ctx.profile(True)
            per = []
            for i in range(a.warmup + a.calls):
                ctx.profile_reset()
                ctx.place_sensors(poses, zx, params, 3)
                ms, n = ctx.profile_get("place_sensors")
                assert n == 3
                if i >= a.warmup:
                    per.append(ms * 1e3 / n)
            ctx.profile(False)
            r["place_sensors_round_us"] = med(per)
            r["place_sensors_rounds_x_aims_us"] = A * med(per)
            r["ratio_to_rounds_x_aims"] = r["round_us"] / r["place_sensors_rounds_x_aims_us"]
            r["ratio_to_floor_chain"] = r["round_us"] / res["floor_chain_us"]
            r["ratio_to_floor_issue"] = r["round_us"] / res["floor_issue_us"]
            # the whole call, and the host route to the same answer
            r["place_aimed_k3_wall_ms"] = wall_of(
                lambda: ctx.place_aimed(poses, zx, params, aims, h, v, 3))
            flat = poses.copy()
            flat[:, 3] = 0.0
            r["score_matrix_wall_ms"] = wall_of(lambda: ctx.score_matrix(flat, zx, params))
            S, Z = ctx.score_matrix(flat, zx, params)
            hp = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = aim_ref.place_aimed(S, Z, flat, cells.xyz, aims, h, v, 3)
                hp.append((time.perf_counter() - t0) * 1e3)
            r["host_aim_ref_ms"] = med(hp)
            r["host_route_ms"] = r["score_matrix_wall_ms"] + r["host_aim_ref_ms"]
            got = ctx.place_aimed(poses, zx, params, aims, h, v, 3)
            assert got["selected"].tolist() == ref["selected"].tolist()
            assert got["selected_aim"].tolist() == ref["selected_aim"].tolist()
            assert got["total_after"].tobytes() == ref["total_after"].tobytes()
            r["selected"] = [[int(p), int(q)] for p, q in zip(got["selected"],
                                                              got["selected_aim"])]
            r["total_after"] = [float(t) for t in got["total_after"]]
            res["shapes"][f"{P}x{A}"] = r
    s = res["shapes"]["91x45"]
    res["faster_than_rounds_x_aims"] = s["round_us"] < s["place_sensors_rounds_x_aims_us"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
