"""Diagnostic: the fan kernel's wave life per elevation ring (FAN_STAMPS), and the share of the
summed wave life spent in rings that cannot reach the terrain from any pose of the call (their
clip interval is empty for every pose: DESIGN.md §5, Skip 4).  The stamps launch keeps the full
grid, so the same breakdown can be taken before and after ring culling (PCP_LIB selects the
build, PCP_FAN_CULL the per-pose early-out).
usage: python tools/fan_ring_life.py [> profiles/<name>.log]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: F401,E402  (load torch's HIP runtime first, as bench.py does)

from pointcloud_processor_amd import _abi, synth  # noqa: E402

ctx = _abi.Context(0)
sc = synth.terrain_scene()
ctx.set_terrain(sc.terrain, point_step=32)
p = sc.area[:, :3].astype(np.float64)
bb = np.array([p[:, 0].min() - .1, p[:, 0].max() + .1, p[:, 1].min() - .1, p[:, 1].max() + .1,
               p[:, 2].min() - .1, p[:, 2].max() + .1])
poses = ctx.generate_candidates(bb, _abi.default_vl_params(num_candidates=348), sc.zx120_pose5)[:256]
fan = _abi.fan_params()
for _ in range(3):
    ctx.raycast_fan(poses, fan)
st = ctx.raycast_fan_stamps(poses, fan).astype(np.int64)      # [P][waves][4]
life = st[..., 3] - st[..., 0]
march = st[..., 2] - st[..., 1]
wpr = fan.n_az // 64                                          # waves per ring
n_el = fan.n_el
ring_life = life.reshape(life.shape[0], n_el, wpr).sum(axis=(0, 2))
ring_march = march.reshape(life.shape[0], n_el, wpr).sum(axis=(0, 2))
# the rings no pose can reach the points from: every sample height above the highest point (or
# below the lowest) by more than the ray radius and the query margin
el = fan.el_min + (fan.el_max - fan.el_min) * (np.arange(n_el) + 0.5) / n_el
se = np.sin(el)
s, steps = 0.5, []
while s < fan.max_distance - 0.08:
    steps.append(s)
    s += 0.3
s0, s1 = steps[0], steps[-1]
tz = np.asarray(sc.terrain)[:, 2].astype(np.float64)
top, bot = tz.max() + 0.056 + 2e-3, tz.min() - 0.056 - 2e-3
pz = poses[:, 2]
h0, h1 = pz[:, None] + se[None, :] * s0, pz[:, None] + se[None, :] * s1
dead = ((np.minimum(h0, h1) > top) | (np.maximum(h0, h1) < bot)).all(axis=0)
print(f"poses {poses.shape[0]} fan {fan.n_az}x{n_el} K {len(steps)} pose z {pz.min():.3f}..{pz.max():.3f} "
      f"points z {tz.min():.3f}..{tz.max():.3f}")
print(f"waves {life.size}")
print(f"dead rings (all poses): {int(dead.sum())} of {n_el}"
      + (f" = rings {np.flatnonzero(dead).min()}..{np.flatnonzero(dead).max()}" if dead.any() else ""))
tot = ring_life.sum()
print(f"share of summed wave life in dead rings: {ring_life[dead].sum() / tot:.4f} "
      f"({ring_life[dead].sum()} of {tot} clk); mean life of a dead wave "
      f"{(ring_life[dead].sum() / max(dead.sum() * wpr * poses.shape[0], 1)):.0f} clk, of a live wave "
      f"{(ring_life[~dead].sum() / max((~dead).sum() * wpr * poses.shape[0], 1)):.0f} clk")
print("ring  el_deg  dead  mean_life_clk  mean_march_clk")
n = wpr * poses.shape[0]
for j in range(n_el):
    print(f"{j:4d} {np.degrees(el[j]):7.2f} {int(dead[j]):5d} {ring_life[j] / n:14.0f} {ring_march[j] / n:15.0f}")
