"""CPU estimate of the fan march's pivot test (DESIGN.md §5 Skip 6), with no GPU involved: with
the oracle's first hits of 8 of the 256 C2 poses (every 2nd ring, every 4th
azimuth), take each first-hit sample's fine cell, build the cell's window by the numpy rule of
tests/fine_ref.py (points within r + 1 mm of the cell's rectangle) and its pivot (the member
nearest the cell's centre in xy), and count how often the pivot is within r of the sample
(FLANN's float test) and how many entries the z-ordered walk tests up to its hit.  The same for
the samples before a ray's first hit that are candidates without being hits (a window member
within r + 2 mm of the sample in z, none within r).  Needs the oracle (make -C oracle) and numpy.
usage: python tools/fan_pivot_estimate.py > profiles/fan_pivot_estimate.log"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'oracle')
from pointcloud_processor_amd import synth  # noqa: E402
import pyoracle  # noqa: E402

sc = synth.terrain_scene()
T32 = np.ascontiguousarray(sc.terrain[:, :3].astype(np.float32))
T = T32.astype(np.float64)
r = 0.056
R = r + 1e-3
c, cf = 0.12, 0.06
r2 = np.float32(r * r)
p = sc.area[:, :3].astype(np.float64)
res = 0.1
bbox = np.array([p[:, 0].min() - res, p[:, 0].max() + res, p[:, 1].min() - res,
                 p[:, 1].max() + res, p[:, 2].min() - res, p[:, 2].max() + res])
Tc = pyoracle.Cloud(sc.terrain)
poses = pyoracle.generate_candidates(Tc, bbox, pyoracle.vl_params(num_candidates=348),
                                     sc.zx120_pose5)[:256]
sel = poses[::32]
n_az, n_el = 1024, 256
elmin, elmax = -85 * np.pi / 180, 85 * np.pi / 180
pyoracle.set_threads(min(16, os.cpu_count() or 1))
blocked, units, fh = pyoracle.raycast_fan(Tc, sel, n_az, n_el, elmin, elmax, 15.0, True)
pyoracle.set_threads(1)
print("poses", sel.shape[0], "blocked", blocked.tolist())
ca, sa, ce, se = pyoracle.fan_tables(n_az, n_el, elmin, elmax)
S = [0.5]
while S[-1] + 0.3 < 15 - 0.08:
    S.append(S[-1] + 0.3)
S = np.array(S)
K = len(S)

# the fine grid as the index lays it: one coarse padding cell below the points
ox, oy, oz = T[:, 0].min() - c, T[:, 1].min() - c, T[:, 2].min() - c
fnx = 2 * (int((T[:, 0].max() - ox) / c) + 2)
fny = 2 * (int((T[:, 1].max() - oy) / c) + 2)
cx = np.floor((T[:, 0] - ox) / cf).astype(np.int64)
cy = np.floor((T[:, 1] - oy) / cf).astype(np.int64)
cell = cy * fnx + cx
order = np.argsort(cell, kind="stable")
cnt = np.bincount(cell, minlength=fnx * fny)
M = int(cnt.max())
start = np.concatenate([[0], np.cumsum(cnt)])
slot = np.full((fnx * fny, M), -1, np.int64)        # the points of each fine cell
rank = np.arange(cell.size) - start[cell[order]]
slot[cell[order], rank] = order
print("fine grid", fnx, fny, "points per cell max", M, "mean", cnt[cnt > 0].mean())


def windows(qx, qy):
    """Members of the window of each query's fine cell: (N, 9 M) point indices (-1: none), the
    cell's centre."""
    wx = np.clip(np.floor((qx - ox) / cf).astype(np.int64), 1, fnx - 2)
    wy = np.clip(np.floor((qy - oy) / cf).astype(np.int64), 1, fny - 2)
    nb = [slot[(wy + dy) * fnx + (wx + dx)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    idx = np.concatenate(nb, 1)
    px, py = T[idx, 0], T[idx, 1]
    x0, y0 = (ox + wx * cf)[:, None], (oy + wy * cf)[:, None]
    gx = np.maximum(np.maximum(x0 - px, px - (x0 + cf)), 0.0)
    gy = np.maximum(np.maximum(y0 - py, py - (y0 + cf)), 0.0)
    mem = (idx >= 0) & (gx * gx + gy * gy <= R * R)
    return np.where(mem, idx, -1), ox + (wx + 0.5) * cf, oy + (wy + 0.5) * cf


def census(q):
    """q: (N, 3) float32 samples.  Per sample: any member within r (FLANN's float sum), the
    pivot within r, tests of the z-ordered walk from the first entry not more than r above q to
    the first member within r, or else to the first entry r below q."""
    idx, ccx, ccy = windows(q[:, 0].astype(np.float64), q[:, 1].astype(np.float64))
    ok = idx >= 0
    P = T32[np.maximum(idx, 0)]
    d0, d1, d2 = q[:, None, 0] - P[..., 0], q[:, None, 1] - P[..., 1], q[:, None, 2] - P[..., 2]
    within = ok & (((d0 * d0) + d1 * d1) + d2 * d2 < r2)
    dc = (P[..., 0].astype(np.float64) - ccx[:, None]) ** 2 + \
         (P[..., 1].astype(np.float64) - ccy[:, None]) ** 2
    piv = np.where(ok, dc, np.inf).argmin(1)
    piv_within = within[np.arange(q.shape[0]), piv]
    z = np.where(ok, P[..., 2], -np.inf)
    zo = np.argsort(-z, axis=1, kind="stable")
    zs = np.take_along_axis(z, zo, 1)
    ws = np.take_along_axis(within, zo, 1)
    live = np.take_along_axis(ok, zo, 1) & (zs - q[:, None, 2] < np.float32(r))   # not r above q
    stop = ws | (q[:, None, 2] - zs >= np.float32(r)) | ~np.take_along_axis(ok, zo, 1)
    first_stop = stop.argmax(1)                     # (the padding always stops)
    tests = (live & (np.arange(zs.shape[1])[None, :] <= first_stop[:, None])).sum(1)
    near = (ok & (np.abs(d2) < np.float32(r + 2e-3))).any(1)
    return within.any(1), piv_within, tests, near, ok.sum(1)


azs = np.arange(0, n_az, 4)
groups = [(0, 20), (20, 40), (40, 120), (120, 122), (122, 256)]
hit_q, hit_ring, miss_q = [], [], []
rng = np.random.default_rng(3)
for pi, Pz in enumerate(sel):
    px, py, pz, pitch, yaw = Pz
    cyw, syw = math.cos(yaw), math.sin(yaw)
    for j in range(0, n_el, 2):
        lx, ly = ce[j] * ca[azs], ce[j] * sa[azs]
        d = np.stack([cyw * lx - syw * ly, syw * lx + cyw * ly, np.full(azs.size, se[j])], 1)
        f = fh[pi, j, azs].astype(int)
        h = f >= 0
        if h.any():
            hit_q.append((Pz[None, :3] + d[h] * S[f[h]][:, None]).astype(np.float32))
            hit_ring.append(np.full(int(h.sum()), j))
        # the samples before the first hit (all of them for a ray that is not blocked)
        last = np.where(h, f, K)
        ks = np.arange(K)[None, :]
        m = ks < last[:, None]
        ii, kk = np.nonzero(m)
        keep = rng.random(ii.size) < 0.25            # a quarter of them is plenty
        ii, kk = ii[keep], kk[keep]
        q = (Pz[None, :3] + d[ii] * S[kk][:, None]).astype(np.float32)
        inb = ((q[:, 0] > T32[:, 0].min()) & (q[:, 0] < T32[:, 0].max()) &
               (q[:, 1] > T32[:, 1].min()) & (q[:, 1] < T32[:, 1].max()) &
               (q[:, 2] < T32[:, 2].max() + 0.06) & (q[:, 2] > T32[:, 2].min() - 0.06))
        miss_q.append(q[inb])
hit_q, hit_ring, miss_q = np.concatenate(hit_q), np.concatenate(hit_ring), np.concatenate(miss_q)

any_h, piv_h, tests_h, _, nmem = census(hit_q)
print("first-hit samples", hit_q.shape[0], "with a window member within r", int(any_h.sum()),
      "(must be all)", "members per window", nmem.mean())
print("pivot within r: share of hits %.4f" % piv_h.mean())
print("z-walk tests per hit %.3f; when the pivot fails %.3f" %
      (tests_h.mean(), tests_h[~piv_h].mean()))
for a, b in groups:
    g = (hit_ring >= a) & (hit_ring < b)
    if g.any():
        print("  rings %3d..%3d hits %7d pivot share %.4f walk tests %.3f" %
              (a, b - 1, int(g.sum()), piv_h[g].mean(), tests_h[g].mean()))
any_m, piv_m, tests_m, near_m, _ = census(miss_q)
cand = near_m & ~any_m
print("samples before the first hit (1 in 4)", miss_q.shape[0], "candidates that do not hit",
      int(cand.sum()), "pivot within r among them", int(piv_m[cand].sum()), "(must be 0)")
print("z-walk tests per such candidate %.3f" % tests_m[cand].mean())
nh, nc = hit_q.shape[0], 4.0 * cand.sum()
share = nh / (nh + nc)
print("hit share of candidates %.3f" % share)
today = 1 + (share * tests_h.mean() + (1 - share) * tests_m[cand].mean())
fail = 1 - share * piv_h.mean()
walk_fail = (share * (~piv_h).mean() * tests_h[~piv_h].mean() +
             (1 - share) * tests_m[cand].mean()) / fail
new = 1 + fail * (1 + walk_fail)
print("lane-loads per candidate: today %.2f, pivot first %.2f (pivot settles %.3f of candidates)"
      % (today, new, 1 - fail))
