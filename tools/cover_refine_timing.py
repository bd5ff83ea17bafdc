#!/usr/bin/env python3
"""Timing of pcp_place_coverage_refine against its yardsticks (not part of the suite).

Workload (DESIGN.md section 6m's): the 1M-point synthetic terrain, the 1024 x 256 fan, 91 and 256
candidate poses of the candidate lattice, every point in the region, k = 1, 2, 4, 8, 16 started
from pcp_place_coverage's greedy set at a separation of SEP metres (filled up with the lowest
poses greedy left out where it stops early).

Every GPU step is a child process of its own under `timeout`, one after the other; the first step
that fails, dies or runs out of time ends the run (nothing more is started on the GPU).  Steps:
  * --step N: per k, pcp_place_coverage_refine_burst, medians of --bursts bursts of --reps after
    two warm-ups: ms[0] = the start set's preparation, ms[1] = its evaluation launch with the
    selection.  In the same process pcp_place_coverage_burst's ms[2], one greedy round's gain
    launch at the same n: an evaluation by the rounds' kernel costs k of them, and the ratio
    ms[1] / (k x ms[2]) is written down for every k (condition 1: below 1 at k = 8).  Beside them
    the evaluation's bytes (n pose rows and k + 1 class rows of W2 words) at the streaming rate of
    DESIGN.md section 6a, and the whole call's wall time with its one wait;
  * --old-route (n = 91, k = 8): the route that existed -- per evaluation one pcp_place_coverage
    call per slot with fixed = s less s_i, k_max = 1 and round_gains, one wait each, and a host
    loop over the moves -- on a build of the PARENT commit (--parent-lib) through plain ctypes;
    its set, its count and its moves are asserted identical to the new call's of the same run
    (condition 2: the new call is faster).

  python tools/cover_refine_timing.py --parent-lib PATH/libpcp.so --parent-commit SHA --commit SHA
                                      [--out profiles/cover_refine_timing.json]
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
SIZES = (91, 256)
KS = (1, 2, 4, 8, 16)
SEP = 2.0
MAX_MOVES = 16
OLD_N, OLD_K = 91, 8
STREAM_TBPS = 4.8          # what a read-once kernel streams here
STEP_TIMEOUT_S = 300


def med(v):
    return float(statistics.median(v))


def workload():
    from pointcloud_processor_amd import _abi, synth

    scene = synth.terrain_scene()
    cells = synth.excavation_cells(scene.area)
    return scene, cells, _abi.fan_params(n_az=N_AZ, n_el=N_EL)


def greedy_start(ctx, poses, fan, k):
    g = ctx.place_coverage(poses, fan, k, SEP)["selected"].tolist()
    return g + [p for p in range(poses.shape[0]) if p not in g][:k - len(g)]


def step(n, a):
    """One size in one process -> a JSON line."""
    from pointcloud_processor_amd import _abi

    scene, cells, fan = workload()
    N = int(scene.terrain.shape[0])
    W2 = ((N + 63) // 64 + 1) & ~1
    m = {"n": n, "words_per_pose": W2, "separation": SEP, "k": {}}
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        cand = ctx.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=256),
                                       scene.zx120_pose5)
        poses = np.ascontiguousarray(np.resize(cand, (n, 5)))
        rd = []
        for i in range(a.bursts + 2):
            ms = ctx.place_coverage_burst(poses, fan, 1, SEP, reps=a.reps)
            if i >= 2:
                rd.append(ms[2])
        m["greedy_round_ms"] = med(rd)
        m["greedy_round_ms_min_max"] = [min(rd), max(rd)]
        for k in KS:
            start = greedy_start(ctx, poses, fan, k)
            pr, ev = [], []
            for i in range(a.bursts + 2):
                ms = ctx.place_coverage_refine_burst(poses, fan, start, 0, SEP, reps=a.reps)
                if i >= 2:
                    pr.append(ms[0])
                    ev.append(ms[1])
            w = []
            for i in range(a.warmup + a.calls):
                t0 = time.perf_counter()
                got = ctx.place_coverage_refine(poses, fan, start, 0, MAX_MOVES, SEP)
                if i >= a.warmup:
                    w.append((time.perf_counter() - t0) * 1e3)
            by = (n + k + 1) * W2 * 8
            m["k"][str(k)] = {
                "start": start, "prep_ms": med(pr), "prep_ms_min_max": [min(pr), max(pr)],
                "eval_ms": med(ev), "eval_ms_min_max": [min(ev), max(ev)],
                "eval_over_k_greedy_rounds": med(ev) / (k * med(rd)),
                "eval_bytes": by, "eval_bytes_at_stream_rate_ms": by / (STREAM_TBPS * 1e12) * 1e3,
                "eval_fraction_of_stream_rate": by / (STREAM_TBPS * 1e12) * 1e3 / med(ev),
                "call_wall_ms": med(w), "call_wall_ms_min_max": [min(w), max(w)],
                "selected": got["selected"].tolist(), "covered": got["covered"],
                "start_covered": got["start_covered"], "n_moves": got["n_moves"],
                "converged": got["converged"],
                "moves": [list(v) for v in zip(got["move_slot"].tolist(), got["move_from"].tolist(),
                                               got["move_to"].tolist(),
                                               got["move_covered"].tolist())]}
        if a.poses_out:
            np.save(a.poses_out, poses)
    print(json.dumps(m))


def old_route(lib_path, poses_file, start, a):
    """The exchanges by greedy calls with all but one slot fixed, on another build of libpcp.so
    -> a JSON line."""
    from pointcloud_processor_amd import _abi

    scene, _, fan = workload()
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
    rg = np.zeros(n, np.int64)
    npts, rpts, base = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ns = C.c_int32()

    def greedy_call(fixed, k_max, want_rg):
        cp = _abi.Context._cover_params(k_max, SEP, fixed, 0)
        rc = lib.pcp_place_coverage(h, poses.ctypes.data_as(P), n, C.byref(fan), C.byref(cp),
                                    None, 0, sel, gain, cov, rg.ctypes.data_as(P) if want_rg else None,
                                    None, None, 0, C.byref(npts), C.byref(rpts), C.byref(base),
                                    C.byref(ns))
        assert rc == 0, rc

    def route():
        s = list(start)
        greedy_call(s, 1, False)
        T = base.value            # the start set's count: every slot fixed
        moves, calls = [], 1
        while True:
            best = (-1, -1, -1)
            for i in range(len(s)):
                greedy_call(s[:i] + s[i + 1:], 1, True)
                calls += 1
                if not ns.value:          # no pose adds a point beside the others
                    continue
                u = np.where(rg >= 0, base.value + rg, -1)
                u[s[i]] = -1
                p = int(np.argmax(u))
                if u[p] > best[0]:
                    best = (int(u[p]), i, p)
            if best[0] <= T or len(moves) >= MAX_MOVES:
                return s, T, moves, int(best[0] <= T), calls
            moves.append([best[1], s[best[1]], best[2], best[0]])
            s[best[1]] = best[2]
            T = best[0]

    w = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        s, T, moves, conv, calls = route()
        if i >= a.warmup:
            w.append((time.perf_counter() - t0) * 1e3)
    lib.pcp_destroy(h)
    print(json.dumps({"wall_ms": med(w), "wall_ms_min_max": [min(w), max(w)], "calls": calls,
                      "selected": s, "covered": int(T), "moves": moves, "converged": conv}))


def run_child(args, what):
    """A GPU step of its own under timeout -> its last line as JSON; any other end stops the run."""
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, __file__] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"cover_refine_timing: step {what} ended with status {r.returncode}: "
                 "nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cover_refine_timing.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--poses-out", default=None)
    ap.add_argument("--old-route", nargs=3, metavar=("LIB", "POSES.npy", "START"), default=None)
    a = ap.parse_args()
    if a.step is not None:
        step(a.step, a)
        return
    if a.old_route:
        old_route(a.old_route[0], a.old_route[1], [int(v) for v in a.old_route[2].split(",")], a)
        return
    common = ["--reps", str(a.reps), "--bursts", str(a.bursts), "--calls", str(a.calls),
              "--warmup", str(a.warmup)]
    res = {"fan": [N_AZ, N_EL], "reps": a.reps, "bursts": a.bursts, "calls": a.calls,
           "max_moves": MAX_MOVES, "commit": a.commit, "parent_commit": a.parent_commit,
           "stream_rate_tbps": STREAM_TBPS, "sizes": {},
           "not_measured": ["PMC counters (VALU busy, atomics, L2 hit rate of the class rows)",
                            "the mounted twin", "a region of interest at these sizes",
                            "the sums through LDS per block before the atomics"]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pf = Path(a.out).with_suffix(".poses.npy")
    try:
        for n in SIZES:
            extra = ["--poses-out", str(pf)] if n == OLD_N and a.parent_lib else []
            res["sizes"][str(n)] = run_child(["--step", str(n)] + common + extra, f"n={n}")
        for n in SIZES:
            m = res["sizes"][str(n)]
            ratio = m["k"]["8"]["eval_over_k_greedy_rounds"]
            m["condition_1_eval_below_8_rounds_at_k_8"] = bool(ratio < 1.0)
        if a.parent_lib:
            m = res["sizes"][str(OLD_N)]
            new = m["k"][str(OLD_K)]
            o = run_child(["--old-route", a.parent_lib, str(pf),
                           ",".join(str(p) for p in new["start"])] + common, "old route")
            for key in ("selected", "covered", "moves", "converged"):
                assert o[key] == new[key], (key, o[key], new[key])
            m["old_route"] = dict(o, k=OLD_K, answers_identical=True,
                                  speedup_of_the_refine_call=o["wall_ms"] / new["call_wall_ms"],
                                  condition_2_the_call_is_faster=bool(
                                      new["call_wall_ms"] < o["wall_ms"]))
    finally:
        if pf.exists():
            pf.unlink()
    res["host_waits_per_call"] = "one: a single stream synchronisation behind the call's last copy"
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
