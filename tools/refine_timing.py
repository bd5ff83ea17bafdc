#!/usr/bin/env python3
"""Timing of pcp_place_refine against its yardsticks (not part of the suite).

Workload: the synthetic tick's cells with its 91 candidates and with 256 (as tools/pair_timing.py),
the start set greedy's k sensors, k = 2 / 4 / 8 / 16.  In one process, medians after a warm-up:
  * one evaluation (pcp_place_refine_burst: the preparation and the evaluation launch, the last
    block's selection included);
  * the yardstick, the device route that existed before for one evaluation: one placement round
    per unlocked slot, k x the measured PCP_K_PLACE time per launch at the same P and C;
  * the floor: the dependent f64 add (tools/mb/chain.hip, profiles/r06_chain.json) x C x the
    successive wave rounds of the evaluation launch (reported, not barred);
  * an evaluation enqueued behind the stop: the whole call with max_moves = 64 against the same
    call with max_moves = the moves it makes, per evaluation between them;
  * the whole calls' wall times, pcp_place_refine beside pcp_place_sensors at the same k.
The only condition: an evaluation is faster than the yardstick.

  python tools/refine_timing.py [--out profiles/refine_timing.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pointcloud_processor_amd import _abi  # noqa: E402
from pointcloud_processor_amd import synth  # noqa: E402
from tools.place_timing import poses_for  # noqa: E402

TILE = 16                 # kRTile: poses per block of an evaluation
CUS = 256


def med(v):
    return float(statistics.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refine_timing.json"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
    res = {"cells": C_, "calls": a.calls, "warmup": a.warmup, "burst_reps": a.reps,
           "dependent_f64_add_ns": add_ns, "poses": {}}

    def wall_of(fn):
        w = []
        for i in range(a.warmup + a.calls):
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
        for P in (91, 256):
            poses = (np.ascontiguousarray(ctx.generate_candidates(cells.grid_bbox, params, zx))
                     if P == 91 else poses_for(ctx, cells.grid_bbox, zx, P))
            assert poses.shape[0] == P
            res["poses"][str(P)] = {}
            for k in (2, 4, 8, 16):
                g = ctx.place_sensors(poses, zx, params, k)
                start = [int(x) for x in g["selected"]]
                start += [p for p in range(P) if p not in start][:k - len(start)]   # (greedy ran dry)
                r = {"start": start, "greedy_placed": int(g["n_selected"])}
                burst = [ctx.place_refine_burst(poses, zx, params, start, reps=a.reps) * 1e3
                         for _ in range(a.warmup + a.calls)][a.warmup:]
                r["evaluation_us"] = med(burst)
                r["evaluation_us_min_max"] = [min(burst), max(burst)]
                # the yardstick: PCP_K_PLACE per launch in this process, one launch per slot
                ctx.profile(True)
                per = []
                for i in range(a.warmup + a.calls):
                    ctx.profile_reset()
                    ctx.place_sensors(poses, zx, params, k)
                    ms, n = ctx.profile_get("place_sensors")
                    assert n == k
                    if i >= a.warmup:
                        per.append(ms * 1e3 / n)
                ctx.profile(False)
                r["place_round_us"] = med(per)
                r["yardstick_us"] = k * med(per)
                # the floor: the chain of one lane, every block resident at once
                blocks = (P + TILE - 1) // TILE
                rounds = -(-blocks // CUS)
                r["eval_blocks"] = blocks
                r["waves_per_block"] = 1 if k <= 4 else 2 if k <= 8 else 4
                r["wave_rounds"] = rounds
                r["floor_us"] = add_ns * C_ * rounds * 1e-3
                r["ratio_to_yardstick"] = r["evaluation_us"] / r["yardstick_us"]
                r["ratio_to_floor"] = r["evaluation_us"] / r["floor_us"]
                # the whole calls, and what the evaluations behind the stop cost
                got = ctx.place_refine(poses, zx, params, start)
                nm = int(got["n_moves"])
                assert got["converged"] == 1
                r["n_moves"] = nm
                r["selected"] = [int(x) for x in got["selected"]]
                r["start_total"] = got["start_total"]
                r["total"] = got["total"]
                full = wall_of(lambda: ctx.place_refine(poses, zx, params, start))
                tight = wall_of(lambda: ctx.place_refine(poses, zx, params, start, max_moves=nm))
                r["place_refine_wall_ms_max_moves_64"] = full
                r["place_refine_wall_ms_max_moves_exact"] = tight
                r["stopped_evaluation_us"] = (full - tight) * 1e3 / (64 - nm)
                r["place_sensors_wall_ms"] = wall_of(
                    lambda: ctx.place_sensors(poses, zx, params, k))
                res["poses"][str(P)][str(k)] = r
    res["faster_than_yardstick"] = all(v["evaluation_us"] < v["yardstick_us"]
                                       for pv in res["poses"].values() for v in pv.values())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
