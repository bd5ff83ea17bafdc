#!/usr/bin/env python3
"""Timing of pcp_place_coverage_weighted against its yardsticks (not part of the suite).

Workload: DESIGN.md section 6m's -- the 1M-point synthetic terrain, the 1024 x 256 fan, 91 and 256
candidate poses of the candidate lattice, k_max = 8 -- with three weightings: `ones` (one plane),
`box10` (10 inside the excavation grid's bounding box, else 1: bits 0, 1, 3, three planes) and
`ramp` (1 + 37 i mod 255: eight planes).  Recorded, medians of --bursts bursts of --reps after two
warm-up bursts, the weighted and the parent's bursts alternating in the same process:
  * the round: pcp_place_coverage_weighted_burst's ms[2] at 1, 3 and 8 planes against
    pcp_place_coverage_burst's ms[2]; the ratio, and the fraction of the streaming rate the
    project measures for a read-once kernel (DESIGN.md section 6a, 4.8 TB/s) of the bytes the
    round must read -- alive poses x W x 8 B of rows and (1 + B) x W x 8 B of need and planes
    (B = 1: need alone);
  * the build: ms[1] against the parent's ms[1] (the planes are the only addition);
  * the same two figures of every --variant build of the library (csrc/Makefile's wvariants: the
    commit keeping need & plane rows, two words per lane, four poses per block), measured in the
    same process and alternating with the production build;
  * the whole call's wall time against the route that exists without it, timed in the same run:
    ceil(n / 64) pcp_simulate_scan calls for the masks only, then the weighted greedy in NumPy.
    The two answers must be identical: selected, gain, gain_points and the owners are asserted
    equal.
--vgprs takes the compiler's register counts (a JSON object) to record beside the times.

  python tools/cover_weight_timing.py [--variant rows=PATH/libpcp.so ..] [--vgprs JSON]
                                      [--commit SHA] [--out profiles/cover_weight_timing.json]
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

N_AZ, N_EL, K_MAX = 1024, 256, 8
SIZES = (91, 256)
STREAM_TBPS = 4.8   # what a read-once kernel streams here
PLANES = {"ones": 1, "box10": 3, "ramp": 8}


def med(v):
    return float(statistics.median(v))


def numpy_weighted_greedy(masks, weight, k_max):
    """The route that exists without the call: weighted greedy over the scans' 64-bit masks (one
    mask array per chunk of 64 poses) -> (selected, gain, gain_points, owner)."""
    N = masks[0].shape[0]
    rows = []
    for m in masks:
        bits = np.unpackbits(m.view(np.uint8).reshape(N, 8), axis=1, bitorder="little")
        rows.append(bits.T.astype(bool))
    seen = np.concatenate(rows)          # [64 * chunks, N]
    w = weight.astype(np.int64)
    need = w != 0
    owner = np.full(N, -2, np.int32)
    alive = np.ones(seen.shape[0], bool)
    sel, gain, gpts = [], [], []
    for r in range(k_max):
        wn = np.where(need, w, 0)
        g = np.array([int(wn[seen[p]].sum()) if alive[p] else -1 for p in range(seen.shape[0])])
        b = int(np.argmax(g))
        if g[b] <= 0:
            break
        sel.append(b)
        gain.append(int(g[b]))
        hit = seen[b] & need
        gpts.append(int(hit.sum()))
        owner[hit] = r
        need &= ~hit
        alive[b] = False
    return sel, gain, gpts, owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover_weight_timing.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--vgprs", default=None, help="JSON object recorded as given")
    a = ap.parse_args()

    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    N = int(scene.terrain.shape[0])
    W = (N + 63) // 64
    bb = cells.grid_bbox
    xyz = np.ascontiguousarray(scene.terrain).view(np.float32).reshape(N, -1)[:, :3]
    in_box = ((xyz[:, 0] >= bb[0]) & (xyz[:, 0] <= bb[1]) & (xyz[:, 1] >= bb[2]) &
              (xyz[:, 1] <= bb[3]))
    weights = {"ones": np.ones(N, np.uint8),
               "box10": np.where(in_box, 10, 1).astype(np.uint8),
               "ramp": (1 + (37 * np.arange(N, dtype=np.int64)) % 255).astype(np.uint8)}
    for name, w in weights.items():
        assert bin(int(np.bitwise_or.reduce(w))).count("1") == PLANES[name], name
    variants = dict(v.split("=", 1) for v in a.variant)
    res = {"terrain_points": N, "fan": [N_AZ, N_EL], "k_max": K_MAX, "words_per_pose": W,
           "reps": a.reps, "bursts": a.bursts, "calls": a.calls, "commit": a.commit,
           "stream_rate_tbps": STREAM_TBPS, "box_points": int(in_box.sum()), "planes": PLANES,
           "variants": sorted(variants), "sizes": {}}
    if a.vgprs:
        res["vgprs"] = json.loads(a.vgprs)

    def wall_of(fn):
        w = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                w.append((time.perf_counter() - t0) * 1e3)
        return med(w)

    ctxs = {"production": _abi.Context(0)}
    for name, path in variants.items():
        ctxs[name] = _abi.Context(0, lib_path=path)
    try:
        for c in ctxs.values():
            c.set_terrain(scene.terrain, point_step=32)
        ctx = ctxs["production"]
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        allp = np.ascontiguousarray(np.resize(cand, (max(SIZES), 5)))
        for n in SIZES:
            poses = np.ascontiguousarray(allp[:n])
            m = {}
            # the bursts, alternating: the parent's, then every build at every weighting
            t = {("parent", "all"): []}
            for b in ctxs:
                for name in weights:
                    t[(b, name)] = []
            for i in range(a.bursts + 2):   # (the second query builds the fine copy: two warm-ups)
                for key, v in t.items():
                    if key[0] == "parent":
                        ms = ctx.place_coverage_burst(poses, fan, K_MAX, reps=a.reps)
                    else:
                        ms = ctxs[key[0]].place_coverage_weighted_burst(
                            poses, fan, weights[key[1]], K_MAX, reps=a.reps)
                    if i >= 2:
                        v.append(ms)
            par = t[("parent", "all")]
            p_build, p_round = med([x[1] for x in par]), med([x[2] for x in par])
            m["parent"] = {"build_ms": p_build, "round_ms": p_round,
                           "round_ms_min_max": [min(x[2] for x in par), max(x[2] for x in par)],
                           "build_ms_min_max": [min(x[1] for x in par), max(x[1] for x in par)]}
            for b in ctxs:
                mb = {}
                for name in weights:
                    v = t[(b, name)]
                    B = PLANES[name]
                    rnd, bld = med([x[2] for x in v]), med([x[1] for x in v])
                    # (one plane is need itself and is not read)
                    bytes_round = n * W * 8 + (1 + (B if B > 1 else 0)) * W * 8
                    floor_ms = bytes_round / (STREAM_TBPS * 1e12) * 1e3
                    mb[name] = {"planes": B, "fan_kernel_ms": med([x[0] for x in v]),
                                "build_ms": bld, "build_ratio_to_parent": bld / p_build,
                                "build_ms_min_max": [min(x[1] for x in v), max(x[1] for x in v)],
                                "round_ms": rnd, "round_ratio_to_parent": rnd / p_round,
                                "round_ms_min_max": [min(x[2] for x in v), max(x[2] for x in v)],
                                "round_bytes": bytes_round, "round_stream_floor_ms": floor_ms,
                                "round_fraction_of_stream_rate": floor_ms / rnd}
                m[b] = mb
            # the whole call against the route that exists without it
            w = weights["box10"]
            got = ctx.place_coverage_weighted(poses, fan, w, K_MAX, want_owner=True)
            m["call_wall_ms"] = wall_of(lambda: ctx.place_coverage_weighted(poses, fan, w, K_MAX))
            m["call_wall_ms_with_owner"] = wall_of(
                lambda: ctx.place_coverage_weighted(poses, fan, w, K_MAX, want_owner=True))
            m["parent_call_wall_ms"] = wall_of(lambda: ctx.place_coverage(poses, fan, K_MAX))

            def old_route():
                masks = []
                for lo in range(0, n, 64):
                    try:
                        s = ctx.simulate_scan(poses[lo:lo + 64], fan, returns_cap=0)
                    except _abi.PcpError as e:   # (no room for records: the mask is valid)
                        s = e.partial
                    masks.append(s["point_mask"].copy())
                return numpy_weighted_greedy(masks, w, K_MAX)

            t0 = time.perf_counter()
            sel, gain, gpts, owner = old_route()
            m["scan_chunks_numpy_greedy_wall_ms"] = (time.perf_counter() - t0) * 1e3
            assert got["selected"].tolist() == sel, (got["selected"].tolist(), sel)
            assert got["gain"].tolist() == gain and got["gain_points"].tolist() == gpts
            assert np.array_equal(got["point_owner"], owner)
            # every build gives the production build's bytes
            for b, c in ctxs.items():
                for name, wt in weights.items():
                    o = c.place_coverage_weighted(poses, fan, wt, K_MAX, want_owner=True,
                                                  want_round_gains=True)
                    p = ctx.place_coverage_weighted(poses, fan, wt, K_MAX, want_owner=True,
                                                    want_round_gains=True)
                    for k in ("selected", "gain", "gain_points", "round_gains", "point_owner"):
                        assert o[k].tobytes() == p[k].tobytes(), (b, name, k)
            m["answers_identical"] = True
            m["selected"] = sel
            m["gain"] = gain
            m["gain_points"] = gpts
            m["speedup_over_scan_chunks"] = (m["scan_chunks_numpy_greedy_wall_ms"] /
                                             m["call_wall_ms_with_owner"])
            res["sizes"][str(n)] = m
    finally:
        for c in ctxs.values():
            c.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
