#!/usr/bin/env python3
"""Timing of pcp_place_coverage_aimed against its yardsticks (not part of the suite).

Workload: the 1M-point synthetic terrain, the 1024 x 256 fan, 91 and 256 candidate poses of the
candidate lattice, a 90 x 30 degree sector with 45 aims (15 yaws x 3 pitches) and 64 aims (16 x 4),
k_max = 8, the region of interest every point.  Recorded, medians of --bursts bursts:
  * pcp_place_coverage_aimed_burst's ms[0] (the fan), ms[1] (the whole build with the ranks and the
    aim masks) and ms[2] (round 0 with the selection), and the whole call's wall time, one wait;
  * beside them pcp_place_coverage_burst's ms[1] / ms[2] at the same n in the same run, and the
    ratios: the aimed round does strictly more, so this states a cost, no bar;
  * the whole aimed call with A aims against A calls of pcp_place_coverage on the same poses (the
    one condition the factoring has to meet: the ratio must be below 1);
  * the route that exists without the call, timed in the same run: ceil(n / 64) pcp_simulate_scan
    calls with their hit_point images, then the windows and the greedy in NumPy.  The two answers
    must be identical: selected, selected_aim, gain and the owners are asserted equal;
  * the bytes round 0 moves -- the bitsets, the ranks, need and the gathered masks -- against the
    bytes a design with one bitset row per (pose, aim) would stream (computed, not built), and the
    round's time against the streaming time of its own bytes at the rate the project measures for
    a read-once kernel (DESIGN.md section 6a, 4.8 TB/s);
  * the mask storage in use (8 bytes per seen point) against its stated bound, n * min(rays, N)
    words.

  python tools/cover_aim_timing.py --commit SHA [--out profiles/cover_aim_timing.json]
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
DEG = np.pi / 180.0
H_FOV, V_FOV = 90.0 * DEG, 30.0 * DEG
AIM_SETS = {45: (15, (-60.0, -35.0, -10.0)), 64: (16, (-70.0, -45.0, -20.0, 5.0))}


def med(v):
    return float(statistics.median(v))


def numpy_aimed_greedy(hit_points, n_az, n_el, w_az, w_el, aims, k_max):
    """The route that exists without the call: the scans' hit_point images [n, n_el, n_az], the
    windows as 64-bit masks per (pose, seen point) and the greedy rounds, all in NumPy
    -> (selected, selected_aim, gain, owner)."""
    A = aims.shape[0]
    col = np.zeros(n_az, np.uint64)
    ring = np.zeros(n_el, np.uint64)
    for a, (az0, el0) in enumerate(aims.tolist()):
        col[(az0 + np.arange(w_az)) % n_az] |= np.uint64(1) << np.uint64(a)
        ring[el0:el0 + w_el] |= np.uint64(1) << np.uint64(a)
    ray_mask = (ring[:, None] & col[None, :]).reshape(-1)
    pts, masks = [], []
    N = 0
    for hp in hit_points:
        flat = hp.reshape(-1)
        hit = np.nonzero(flat >= 0)[0]
        p = flat[hit].astype(np.int64)
        order = np.argsort(p, kind="stable")
        p, m = p[order], ray_mask[hit][order]
        first = np.ones(p.size, bool)
        first[1:] = p[1:] != p[:-1]
        start = np.nonzero(first)[0]
        pts.append(p[start])
        masks.append(np.bitwise_or.reduceat(m, start) if p.size else np.zeros(0, np.uint64))
        N = max(N, int(p[-1]) + 1 if p.size else 0)
    return pts, masks


def greedy_rounds(pts, masks, N, A, k_max):
    need = np.ones(N, bool)
    owner = np.full(N, -2, np.int32)
    n = len(pts)
    alive = np.ones(n, bool)
    sel, sel_aim, gain = [], [], []
    for r in range(k_max):
        g = np.full((n, A), -1, np.int64)
        for p in np.nonzero(alive)[0]:
            live = np.ascontiguousarray(masks[p][need[pts[p]]])
            bits = np.unpackbits(live.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
            g[p] = bits.sum(axis=0, dtype=np.int64)[:A]
        e = int(np.argmax(g.reshape(-1)))
        b, ab = divmod(e, A)
        if g[b, ab] <= 0:
            break
        sel.append(b)
        sel_aim.append(ab)
        gain.append(int(g[b, ab]))
        inside = ((masks[b] >> np.uint64(ab)) & np.uint64(1)).astype(bool) & need[pts[b]]
        owner[pts[b][inside]] = r
        need[pts[b][inside]] = False
        alive[b] = False
    return sel, sel_aim, gain, owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover_aim_timing.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    fan = _abi.fan_params(n_az=N_AZ, n_el=N_EL)
    N = int(scene.terrain.shape[0])
    W = (N + 63) // 64
    rays = N_AZ * N_EL
    res = {"terrain_points": N, "fan": [N_AZ, N_EL], "k_max": K_MAX, "words_per_pose": W,
           "h_fov_deg": 90.0, "v_fov_deg": 30.0, "reps": a.reps, "bursts": a.bursts,
           "calls": a.calls, "commit": a.commit, "stream_rate_tbps": STREAM_TBPS, "cases": {}}

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
        for n, A in zip(SIZES, AIM_SETS):
            n_yaw, pitches = AIM_SETS[A]
            yaws = 2.0 * np.pi * np.arange(n_yaw) / n_yaw
            w_az, w_el, aims = _abi.cover_aims(fan, H_FOV, V_FOV, yaws,
                                               np.array(pitches) * DEG)
            assert aims.shape[0] == A
            poses = np.ascontiguousarray(allp[:n])
            m = {"n": n, "n_aims": A, "w_az": w_az, "w_el": w_el}
            f, b, r, pb, pr = [], [], [], [], []
            for i in range(a.bursts + 2):   # (the second query builds the fine copy: two warm-ups)
                ms = ctx.place_coverage_aimed_burst(poses, fan, w_az, w_el, aims, K_MAX,
                                                    reps=a.reps)
                pm = ctx.place_coverage_burst(poses, fan, K_MAX, reps=a.reps)
                if i >= 2:
                    f.append(ms[0])
                    b.append(ms[1])
                    r.append(ms[2])
                    pb.append(pm[1])
                    pr.append(pm[2])
            m.update({"fan_kernel_ms": med(f), "build_ms": med(b), "round_ms": med(r),
                      "round_ms_min_max": [min(r), max(r)],
                      "plain_bitset_phase_ms": med(pb), "plain_round_ms": med(pr),
                      "build_ratio_to_plain": med(b) / med(pb),
                      "round_ratio_to_plain": med(r) / med(pr)})
            got = ctx.place_coverage_aimed(poses, fan, w_az, w_el, aims, K_MAX, want_owner=True,
                                           want_aim_points=True)
            m["call_wall_ms"] = wall_of(
                lambda: ctx.place_coverage_aimed(poses, fan, w_az, w_el, aims, K_MAX))
            m["call_wall_ms_with_owner"] = wall_of(
                lambda: ctx.place_coverage_aimed(poses, fan, w_az, w_el, aims, K_MAX,
                                                 want_owner=True))
            m["plain_call_wall_ms"] = wall_of(lambda: ctx.place_coverage(poses, fan, K_MAX))
            m["aimed_call_over_A_plain_calls"] = m["call_wall_ms"] / (A * m["plain_call_wall_ms"])
            # round 0's traffic (need = every point): what it reads, what a bitset per (pose, aim)
            # would stream, and the streaming time of its own bytes
            seen_total = int(got["seen_points"].astype(np.int64).sum())
            bytes_round = n * W * 8 + n * W * 4 + W * 8 + seen_total * 8
            bytes_bitset_design = n * A * W * 8
            floor_ms = bytes_round / (STREAM_TBPS * 1e12) * 1e3
            m.update({"round_bytes": bytes_round, "round_bytes_gathered_masks": seen_total * 8,
                      "bitset_per_aim_design_bytes": bytes_bitset_design,
                      "bytes_ratio_to_bitset_design": bytes_round / bytes_bitset_design,
                      "round_stream_floor_ms": floor_ms,
                      "round_over_stream_floor": med(r) / floor_ms,
                      "mask_bytes_in_use": seen_total * 8,
                      "mask_bytes_bound": n * min(rays, N) * 8,
                      "seen_points_per_pose_mean": seen_total / n})

            # the route that exists without the call
            t0 = time.perf_counter()
            images = []
            for lo in range(0, n, 64):
                s = ctx.simulate_scan(poses[lo:lo + 64], fan, want_dense=True)
                images += [s["hit_point"][q] for q in range(s["hit_point"].shape[0])]
            t1 = time.perf_counter()
            pts, masks = numpy_aimed_greedy(images, N_AZ, N_EL, w_az, w_el, aims, K_MAX)
            sel, sel_aim, gain, owner = greedy_rounds(pts, masks, N, A, K_MAX)
            t2 = time.perf_counter()
            m["scan_chunks_ms"] = (t1 - t0) * 1e3
            m["numpy_windows_and_greedy_ms"] = (t2 - t1) * 1e3
            m["scan_chunks_numpy_wall_ms"] = (t2 - t0) * 1e3
            assert got["selected"].tolist() == sel, (got["selected"].tolist(), sel)
            assert got["selected_aim"].tolist() == sel_aim
            assert got["gain"].tolist() == gain
            assert np.array_equal(got["point_owner"], owner)
            m["answers_identical"] = True
            m["selected"] = sel
            m["selected_aim"] = sel_aim
            m["gain"] = gain
            m["speedup_over_scan_chunks"] = (m["scan_chunks_numpy_wall_ms"] /
                                             m["call_wall_ms_with_owner"])
            res["cases"][f"{n}x{A}"] = m
            print(json.dumps({f"{n}x{A}": m}), flush=True)
    res["host_waits_per_call"] = ("one: the call's path holds a single stream synchronisation "
                                  "(stream_done) behind its last copy; a change of the fan or step "
                                  "tables adds the fan query's own upload wait, as for every fan call")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
