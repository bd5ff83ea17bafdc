#!/usr/bin/env python3
"""Timing of pcp_place_triple against its yardsticks (not part of the suite).

Workload: the synthetic tick's cells with its 91 candidates and with 256 (num_candidates raised
until 256 survive, as tools/place_timing.py).  In one process, medians of --calls after --warmup:
  * the triple phase per repetition (pcp_place_triple_burst: the pair phase it builds on, the
    triple tiles, the rows' maxima, the selection);
  * route A, the exact route that existed before: one pcp_place_pair with one fixed sensor per
    choice of first sensor, P x the per-repetition time of pcp_place_pair_burst(fixed = [0]).  It
    evaluates every triple three times, so a triple kernel that is as good per chain as
    k_pair_tiles lands at A / 3.  THE ONE CONDITION: the triple phase takes at most A / 3 at both
    sizes;
  * reported with no bar: the f64 issue floor -- 2 f64 operations (one max, one add) per evaluated
    triple-cell, the padded slots and cells included, at the device's vector f64 rate: 256 CUs x
    4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 operations/s (the data sheet's 78.6 TFLOP/s of vector
    FP64 counts a fused multiply-add as two) -- and the phase's ratio to it; the whole call's wall
    time with its one wait; route C, pcp_score_matrix plus the NumPy restatement on the host
    (tests/triple_ref.py without its table; P = 91 only: at 256 it runs for minutes);
  * --alt LABEL=LIBPCP.SO (repeatable): the same bursts through another build of the library in
    the same process (the chains-per-lane A/B: make EXTRA=-DPCP_TRIPLE_TA=4 OUTDIR=../_lib/alt4).
--trace P runs only a few calls of pcp_place_triple_burst at P poses, for
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/triple_timing.py --trace 91
and --kernel-split P=DIR/run_kernel_stats.csv (repeatable) adds that trace's per-kernel averages.

  python tools/triple_timing.py [--out profiles/triple_timing.json]
"""
import argparse
import csv
import json
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from pointcloud_processor_amd import _abi  # noqa: E402
from pointcloud_processor_amd import synth  # noqa: E402
from tools.place_timing import poses_for  # noqa: E402

TILE = 16                     # kTripleTile
CHUNK = 64                    # kWalkC: the rows are padded to whole chunks
F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9   # vector f64 adds or maxima per second (see above)


def med(v):
    return float(statistics.median(v))


def chains_per_lane(path=None):
    """kTripleA of the build at hand (the header's default, or the alt build's label)."""
    src = (ROOT / "pointcloud_processor_amd" / "csrc" / "pcp_triple_tiles.hpp").read_text()
    return int(re.search(r"#define PCP_TRIPLE_TA (\d+)", src).group(1))


def floor_us(P, C, ta):
    nt = -(-P // TILE)
    blocks = nt * (nt + 1) * (nt + 2) // 6 * (TILE // ta)
    cs = -(-C // CHUNK) * CHUNK
    slots = blocks * TILE * TILE * ta
    return {"tile_triples": blocks // (TILE // ta), "blocks": blocks, "triple_slots": slots,
            "triples": P * (P - 1) * (P - 2) // 6,
            "f64_floor_us": 2.0 * slots * cs / F64_OPS_PER_S * 1e6}


def load_scene(ctx, scene, cells, aux):
    ctx.set_terrain(scene.terrain, point_step=32)
    ctx.set_aux_cloud(aux, point_step=32)
    ctx.set_cells(cells.xyz, cells.normals)


def kernel_split(path):
    out = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"\b(k_(?:pair|triple)_\w+)\(", r["Name"])   # pcp::(anonymous namespace)::k_..(
        if m:
            out[m.group(1)] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triple_timing.json"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alt", action="append", default=[], metavar="LABEL=LIBPCP.SO")
    ap.add_argument("--kernel-split", action="append", default=[], metavar="P=STATS.CSV")
    ap.add_argument("--trace", type=int, default=0, metavar="P")
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    aux = synth.aux_cloud()
    zx = scene.zx120_pose5
    params = _abi.default_vl_params()
    C_ = int(cells.xyz.shape[0])
    ta = chains_per_lane()

    def wall_of(fn):
        w = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if i >= a.warmup:
                w.append((t1 - t0) * 1e3)
        return med(w)

    def bursts(fn):
        v = [fn() * 1e3 for _ in range(a.warmup + a.calls)][a.warmup:]
        return med(v), [min(v), max(v)]

    with _abi.Context(0) as ctx:
        load_scene(ctx, scene, cells, aux)
        pose_sets = {
            91: np.ascontiguousarray(ctx.generate_candidates(cells.grid_bbox, params, zx)),
            256: poses_for(ctx, cells.grid_bbox, zx, 256)}
        if a.trace:
            for _ in range(3):
                ctx.place_triple_burst(pose_sets[a.trace], zx, params, reps=a.reps)
            return
        res = {"cells": C_, "calls": a.calls, "warmup": a.warmup, "burst_reps": a.reps,
               "chains_per_lane": ta, "f64_ops_per_s": F64_OPS_PER_S,
               "f64_rate_source": "256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz, one f64 add or max per "
                                  "lane and clock (78.6 TFLOP/s vector FP64 on the data sheet, an "
                                  "FMA counted as two)",
               "poses": {}}
        for P, poses in pose_sets.items():
            assert poses.shape[0] == P
            r = floor_us(P, C_, ta)
            r["triple_phase_us"], r["triple_phase_us_min_max"] = bursts(
                lambda: ctx.place_triple_burst(poses, zx, params, reps=a.reps))
            r["pair_phase_one_fixed_us"], r["pair_phase_one_fixed_us_min_max"] = bursts(
                lambda: ctx.place_pair_burst(poses, zx, params, fixed=[0], reps=a.reps))
            r["pair_phase_us"], _ = bursts(
                lambda: ctx.place_pair_burst(poses, zx, params, reps=a.reps))
            r["route_a_us"] = P * r["pair_phase_one_fixed_us"]
            r["route_a_third_us"] = r["route_a_us"] / 3
            r["ratio_to_a_third"] = r["triple_phase_us"] / r["route_a_third_us"]
            r["triple_tiles_launches_us_about"] = r["triple_phase_us"] - r["pair_phase_us"]
            r["ratio_to_f64_floor"] = r["triple_phase_us"] / r["f64_floor_us"]
            r["place_triple_wall_ms"] = wall_of(lambda: ctx.place_triple(poses, zx, params))
            r["place_pair_wall_ms"] = wall_of(lambda: ctx.place_pair(poses, zx, params))
            got = ctx.place_triple(poses, zx, params)
            r["best_triple"] = [int(x) for x in got["best_triple"]]
            r["triple_total"] = got["triple_total"]
            r["n_selected"] = got["n_selected"]
            if P == 91 and not a.no_host_route:
                import triple_ref
                r["score_matrix_wall_ms"] = wall_of(lambda: ctx.score_matrix(poses, zx, params))
                S, Z = ctx.score_matrix(poses, zx, params)
                t0 = time.perf_counter()
                ref = triple_ref.place_triple(S, Z, poses[:, :2], want_table=False)
                r["host_triples_ms"] = (time.perf_counter() - t0) * 1e3
                r["route_c_ms"] = r["score_matrix_wall_ms"] + r["host_triples_ms"]
                assert tuple(ref["best_triple"]) == tuple(got["best_triple"])
                assert ref["triple_total"] == got["triple_total"]
            res["poses"][str(P)] = r
    for spec in a.alt:
        label, path = spec.split("=", 1)
        with _abi.Context(0, lib_path=path) as alt:
            load_scene(alt, scene, cells, aux)
            v = {}
            for P, poses in pose_sets.items():
                m, mm = bursts(lambda: alt.place_triple_burst(poses, zx, params, reps=a.reps))
                got = alt.place_triple(poses, zx, params)
                same = (got["triple_total"] == res["poses"][str(P)]["triple_total"] and
                        [int(x) for x in got["best_triple"]] == res["poses"][str(P)]["best_triple"])
                v[str(P)] = {"triple_phase_us": m, "min_max": mm, "same_answer": bool(same)}
            res.setdefault("chains_per_lane_ab", {})[label] = v
    if a.alt:
        res["chains_per_lane_ab"][f"{ta} (as committed)"] = {
            k: {"triple_phase_us": v["triple_phase_us"], "min_max": v["triple_phase_us_min_max"]}
            for k, v in res["poses"].items()}
    for spec in a.kernel_split:
        P, path = spec.split("=", 1)
        res["poses"][P]["kernels_us"] = kernel_split(path)
    res["at_most_a_third_of_a"] = all(v["triple_phase_us"] <= v["route_a_third_us"]
                                      for v in res["poses"].values())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
