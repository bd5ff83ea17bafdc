#!/usr/bin/env python3
"""Timing of pcp_place_pair against its yardsticks (not part of the suite).

Workload: the synthetic tick's cells with its 91 candidates and with 256 (num_candidates raised
until 256 survive, as tools/place_timing.py).  In one process, medians after a warm-up:
  * the pair phase per repetition (pcp_place_pair_burst: preparation + pair tiles + selection);
  * yardstick A, the device alternative that existed before for the same table: one placement
    round per choice of first sensor, (P - 1) x the measured PCP_K_PLACE time per launch;
  * yardstick B, the floor: the dependent f64 add (tools/mb/chain.hip, profiles/r06_chain.json)
    x C x the successive wave rounds the tile launch needs at its occupancy;
  * yardstick C, the host route: pcp_score_matrix plus the NumPy restatement of the search;
  * the whole calls' wall times, pcp_place_pair beside pcp_place_sensors(k_max = 2).
The only condition: the pair phase is faster than yardstick A.

  python tools/pair_timing.py [--out profiles/pair_timing.json]
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

TILE = 16                 # kPairTile: poses per tile edge, one block of four waves per tile pair
BLOCKS_PER_CU = 4         # k_pair_tiles: 33.1 KiB of LDS per block of 160 KiB (60 VGPRs allow 8)
CUS = 256


def med(v):
    return float(statistics.median(v))


def host_pairs(S, Z):
    """The definition on the host without fixed sensors or a separation (ordered sums by a
    sequential cumsum) -> (best pair, its total)."""
    osum = lambda V: np.cumsum(np.where(V > 0, V, 0.0), axis=1)[:, -1]   # noqa: E731
    M = np.where(Z[None, :] < S, S, Z[None, :])
    P = S.shape[0]
    best, bt = (-1, -1), -np.inf
    for a in range(P - 1):
        t = osum(np.where(M[a][None, :] < S[a + 1:], S[a + 1:], M[a][None, :]))
        b = int(np.argmax(t))
        if t[b] > bt:
            best, bt = (a, a + 1 + b), float(t[b])
    return best, bt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pair_timing.json"))
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
            r = {}
            burst = [ctx.place_pair_burst(poses, zx, params, reps=a.reps) * 1e3
                     for _ in range(a.warmup + a.calls)][a.warmup:]
            r["pair_phase_us"] = med(burst)
            r["pair_phase_us_min_max"] = [min(burst), max(burst)]
            # yardstick A: PCP_K_PLACE per launch in this process
            ctx.profile(True)
            per = []
            for i in range(a.warmup + a.calls):
                ctx.profile_reset()
                ctx.place_sensors(poses, zx, params, 2)
                ms, n = ctx.profile_get("place_sensors")
                assert n == 2
                if i >= a.warmup:
                    per.append(ms * 1e3 / n)
            ctx.profile(False)
            r["place_round_us"] = med(per)
            r["yardstick_a_us"] = (P - 1) * med(per)
            # yardstick B: the chain floor
            nt = (P + TILE - 1) // TILE
            blocks = nt * (nt + 1) // 2
            rounds = -(-blocks // (BLOCKS_PER_CU * CUS))
            r["tile_blocks"] = blocks
            r["wave_rounds"] = rounds
            r["yardstick_b_us"] = add_ns * C_ * rounds * 1e-3
            # yardstick C: the matrix to the host, the search there
            r["score_matrix_wall_ms"] = wall_of(lambda: ctx.score_matrix(poses, zx, params))
            S, Z = ctx.score_matrix(poses, zx, params)
            hp = []
            for _ in range(3):
                t0 = time.perf_counter()
                best, bt = host_pairs(S, Z)
                hp.append((time.perf_counter() - t0) * 1e3)
            r["host_pairs_ms"] = med(hp)
            r["yardstick_c_ms"] = r["score_matrix_wall_ms"] + r["host_pairs_ms"]
            # the whole calls
            r["place_pair_wall_ms"] = wall_of(lambda: ctx.place_pair(poses, zx, params))
            r["place_sensors_k2_wall_ms"] = wall_of(lambda: ctx.place_sensors(poses, zx, params, 2))
            r["score_poses_wall_ms"] = wall_of(lambda: ctx.score_poses(
                poses, zx, params, np.zeros(C_, np.uint8)))
            got = ctx.place_pair(poses, zx, params)
            assert tuple(got["best_pair"]) == best and got["pair_total"] == bt, (got, best, bt)
            g = ctx.place_sensors(poses, zx, params, 2)
            r["best_pair"] = [int(x) for x in got["best_pair"]]
            r["pair_total"] = got["pair_total"]
            r["greedy_pair"] = [int(x) for x in g["selected"]]
            r["greedy_total"] = float(g["total_after"][-1])
            r["ratio_to_a"] = r["pair_phase_us"] / r["yardstick_a_us"]
            r["ratio_to_b"] = r["pair_phase_us"] / r["yardstick_b_us"]
            res["poses"][str(P)] = r
    res["faster_than_a"] = all(v["pair_phase_us"] < v["yardstick_a_us"]
                               for v in res["poses"].values())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
