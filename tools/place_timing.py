#!/usr/bin/env python3
"""Timing of pcp_place_sensors against its yardstick (not part of the suite).

Workload: the synthetic tick's cells with 256 candidates (num_candidates raised until 256
survive, as bench.py does).  In one process, medians of --calls calls after --warmup:
  * PCP_K_PLACE per launch (one launch per placement round) for k_max in {1, 2, 4, 8};
  * PCP_K_POSE_SUM per launch of pcp_score_poses (k_sum_flags: the same chain length over the
    same rows) -- the yardstick; the bar for a placement round is 1.5 x that;
  * the calls' wall times, and what a caller had to do before pcp_place_sensors existed for the
    same answer: pcp_score_matrix (the whole [P][C] matrix to the host) plus the greedy on the CPU.

  python tools/place_timing.py [--out profiles/place_timing.json]
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

from pointcloud_processor_amd import _abi, synth  # noqa: E402


def poses_for(ctx, grid_bbox, zx, total):
    nc = max(total, 100)
    while True:
        p = _abi.default_vl_params(num_candidates=nc)
        poses = ctx.generate_candidates(grid_bbox, p, zx)
        if poses.shape[0] >= total:
            return np.ascontiguousarray(poses[:total])
        nc = int(nc * 1.3) + 16


def host_greedy(S, Z, k_max):
    """The definition's rounds on the host (ordered sums by a sequential cumsum)."""
    base = Z.copy()
    T = np.cumsum(np.where(base > 0, base, 0.0))[-1]
    alive = np.ones(S.shape[0], bool)
    sel = []
    for _ in range(k_max):
        M = np.where(base[None, :] < S, S, base[None, :])
        t = np.where(alive, np.cumsum(np.where(M > 0, M, 0.0), axis=1)[:, -1], -np.inf)
        b = int(np.argmax(t))
        if not t[b] > T:
            break
        sel.append(b)
        T = t[b]
        base = np.where(base < S[b], S[b], base)
        alive[b] = False
    return sel


def med(v):
    return float(statistics.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "place_timing.json"))
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.calls >= 20
    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    aux = synth.aux_cloud()
    zx = scene.zx120_pose5
    params = _abi.default_vl_params()
    res = {"poses": a.poses, "cells": int(cells.xyz.shape[0]), "calls": a.calls,
           "warmup": a.warmup, "rounds": {}}
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = poses_for(ctx, cells.grid_bbox, zx, a.poses)
        flags = np.zeros(cells.xyz.shape[0], np.uint8)
        ctx.profile(True)
        # the yardstick: k_sum_flags per launch of pcp_score_poses, and the call's wall time
        ks, wall = [], []
        for i in range(a.warmup + a.calls):
            ctx.profile_reset()
            t0 = time.perf_counter()
            ctx.score_poses(poses, zx, params, flags)
            t1 = time.perf_counter()
            ms, n = ctx.profile_get("pose_sum")
            assert n == 1
            if i >= a.warmup:
                ks.append(ms * 1e3)
                wall.append((t1 - t0) * 1e3)
        res["k_sum_flags_us"] = med(ks)
        res["k_sum_flags_us_min_max"] = [min(ks), max(ks)]
        res["score_poses_wall_ms_profiled"] = med(wall)
        for k in (1, 2, 4, 8):
            per, tot_us, wall, nsel = [], [], [], None
            for i in range(a.warmup + a.calls):
                ctx.profile_reset()
                t0 = time.perf_counter()
                got = ctx.place_sensors(poses, zx, params, k)
                t1 = time.perf_counter()
                ms, n = ctx.profile_get("place_sensors")
                assert n == k
                nsel = got["n_selected"]
                if i >= a.warmup:
                    per.append(ms * 1e3 / n)
                    tot_us.append(ms * 1e3)
                    wall.append((t1 - t0) * 1e3)
            res["rounds"][str(k)] = {"n_selected": nsel, "round_us": med(per),
                                     "round_us_min_max": [min(per), max(per)],
                                     "rounds_total_us": med(tot_us),
                                     "call_wall_ms_profiled": med(wall),
                                     "ratio_to_k_sum_flags": med(per) / res["k_sum_flags_us"]}
        ctx.profile(False)
        # wall times without the profiling events
        def wall_of(fn):
            w = []
            for i in range(a.warmup + a.calls):
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    w.append((t1 - t0) * 1e3)
            return med(w)
        res["score_poses_wall_ms"] = wall_of(lambda: ctx.score_poses(poses, zx, params, flags))
        for k in (1, 2, 4, 8):
            res["rounds"][str(k)]["call_wall_ms"] = wall_of(
                lambda: ctx.place_sensors(poses, zx, params, k))
        # before pcp_place_sensors: the matrix to the host, the greedy there
        res["score_matrix_wall_ms"] = wall_of(lambda: ctx.score_matrix(poses, zx, params))
        S, Z = ctx.score_matrix(poses, zx, params)
        res["matrix_bytes"] = int(S.nbytes + Z.nbytes)
        hg = []
        for i in range(5):
            t0 = time.perf_counter()
            sel = host_greedy(S, Z, 8)
            hg.append((time.perf_counter() - t0) * 1e3)
        res["host_greedy_k8_ms"] = med(hg)
        got = ctx.place_sensors(poses, zx, params, 8)
        assert sel == got["selected"].tolist(), (sel, got["selected"])
    res["bar_ratio"] = 1.5
    res["bar_met"] = all(v["ratio_to_k_sum_flags"] <= 1.5 for v in res["rounds"].values())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
