"""Input builders for the carve's edge-case tests (test_carve_cases.py on the CPU,
test_carve_edges.py on the GPU): clouds at the keep tiles' sizes, whole tiles carved, nearest-
point ties, many fallback queries, points exactly at the search radius, record layouts and z
sums on either side of the line where a plain double sum stops being exact.

Every builder returns a Case: the cloud as (n, 8) float32 PointXYZRGB rows (x, y, z, 1, rgb,
0, 0, 0), the zx120 transform (t, q) and the excavation parameters as keyword arguments (the
same for oracle.exc_params and _abi.excavation_params).  The pits are rectangles with few
lattice points, so the brute-force oracle (O(queries x n)) stays within seconds at n = 262,145.

geometry() restates the pose / lattice arithmetic of excavated_surface_generator.cpp in Python
floats (IEEE doubles, the same libm), so a test can name every generated height query."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name cloud t q kw")
Geometry = namedtuple("Geometry", "cx cy yaw length width slope_offset depth radius queries "
                                  "n_bottom drop area")

KEEP_BLOCK = 256          # threads of a keep tile
KEEP_MIN_TILES = 64
KEEP_MAX_ITEMS = 16
DEFAULTS = dict(depth=1.0, slope_angle_deg=75.0, offset_x=4.0, offset_y=1.0, point_density=0.05,
                terrain_search_radius=0.5, l_shape_enabled=1, width=1.2, length=1.8)
SMALL_PIT = dict(l_shape_enabled=0, length=0.6, width=0.4, point_density=0.1)
WIDE_PIT = dict(l_shape_enabled=0, length=1.2, width=0.8, point_density=0.2)
TILE_SIZES = (1, 63, 255, 256, 257, 16384, 16385, 245760, 245761, 262144, 262145)
NEAREST_COUNTS = (1, 255, 4096, 4097)
LAYOUTS = ("step12", "step16", "step20", "step32", "step32_shifted")


def keep_items(n: int) -> int:
    """Points per thread of a keep tile: clamp(ceil(n / 16384), 1, 16)."""
    per = -(-n // (KEEP_BLOCK * KEEP_MIN_TILES))
    return min(max(per, 1), KEEP_MAX_ITEMS)


def keep_tile(n: int) -> int:
    return KEEP_BLOCK * keep_items(n)


def yaw_pose(yaw_deg=20.0, t=(0.3, -0.2, 0.1)):
    yaw = math.radians(yaw_deg)
    return tuple(t), (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))


def geometry(t, q, kw) -> Geometry:
    """The excavation centre, yaw and every generated height query (centre, lattice bottoms,
    wall points: the order of the generated surface) of a rectangle-mode pit, in the
    reference's own double expressions.  drop[k]: surface record k lies at height(queries[k +
    1]) - drop[k].  area[k] = (query, rise): area record k lies at (height(queries[query]) -
    depth) + rise, or at height - depth where rise is None (the bottom points)."""
    p = dict(DEFAULTS, **kw)
    assert not p["l_shape_enabled"], "the edge cases use the rectangle mode"
    qx, qy, qz, qw = q
    d = qx * qx + qy * qy + qz * qz + qw * qw
    s = 2.0 / d
    xs, ys, zs = qx * s, qy * s, qz * s
    wx, wy, wz = qw * xs, qw * ys, qw * zs
    xx, xy, xz = qx * xs, qx * ys, qx * zs
    yy, yz, zz = qy * ys, qy * zs, qz * zs
    m = ((1.0 - (yy + zz), xy - wz, xz + wy),
         (xy + wz, 1.0 - (xx + zz), yz - wx),
         (xz - wy, yz + wx, 1.0 - (xx + yy)))
    ox, oy, oz = p["offset_x"], p["offset_y"], 0.0
    cx = (m[0][0] * ox + m[0][1] * oy + m[0][2] * oz) + t[0]
    cy = (m[1][0] * ox + m[1][1] * oy + m[1][2] * oz) + t[1]
    yaw = 0.0
    if not abs(m[2][0]) >= 1:
        pitch = -math.asin(m[2][0])
        yaw = math.atan2(m[1][0] / math.cos(pitch), m[0][0] / math.cos(pitch))
    length, width, dens, depth = p["length"], p["width"], p["point_density"], p["depth"]
    mnx, mxx, mny, mxy = -length / 2.0, length / 2.0, -width / 2.0, width / 2.0

    def inside(x, y):
        return mnx <= x <= mxx and mny <= y <= mxy

    def outer_edge(x, y):
        return inside(x, y) and not (inside(x + dens, y) and inside(x - dens, y) and
                                     inside(x, y + dens) and inside(x, y - dens))

    slope_offset = depth / math.tan(p["slope_angle_deg"] * math.pi / 180.0)
    n_x, n_y = int((mxx - mnx) / dens) + 1, int((mxy - mny) / dens) + 1
    n_slope = int(slope_offset / dens) + 1
    cyaw, syaw = math.cos(yaw), math.sin(yaw)
    n_depth = int(depth / dens)
    queries, drop, area = [(cx, cy)], [], []
    for i in range(n_x + 1):
        for j in range(n_y + 1):
            xl, yl = mnx + i * dens, mny + j * dens
            if inside(xl, yl):
                area.append((len(queries), None))
                if outer_edge(xl, yl):
                    area += [(len(queries), k * dens) for k in range(1, n_depth)]
                queries.append((cx + xl * cyaw - yl * syaw, cy + xl * syaw + yl * cyaw))
                drop.append(depth)
    n_bottom = len(queries) - 1
    for i in range(n_x + 1):
        for j in range(n_y + 1):
            xl, yl = mnx + i * dens, mny + j * dens
            if not outer_edge(xl, yl):
                continue
            for k in range(n_slope + 1):
                off = slope_offset * (k / n_slope)
                ofx = ofy = 0.0
                if not inside(xl + dens, yl):
                    ofx = off
                elif not inside(xl - dens, yl):
                    ofx = -off
                if not inside(xl, yl + dens):
                    ofy = off
                elif not inside(xl, yl - dens):
                    ofy = -off
                xs2, ys2 = xl + ofx, yl + ofy
                queries.append((cx + xs2 * cyaw - ys2 * syaw, cy + xs2 * syaw + ys2 * cyaw))
                drop.append(depth * (1.0 - k / n_slope))
    return Geometry(cx, cy, yaw, length, width, slope_offset, depth, p["terrain_search_radius"],
                    queries, n_bottom, drop, area)


def generated_z(g: Geometry, heights):
    """The generated records' z (surface, area) as float32 from one height per query."""
    surf = [np.float32(heights[k + 1] - g.drop[k]) for k in range(len(g.drop))]
    area = [np.float32(heights[q] - g.depth if rise is None else (heights[q] - g.depth) + rise)
            for q, rise in g.area]
    return np.array(surf, np.float32), np.array(area, np.float32)


def local_xy(g: Geometry, x, y):
    """Map x, y (float32 arrays) in the pit's frame, as processExcavation computes them."""
    dx, dy = x.astype(np.float64) - g.cx, y.astype(np.float64) - g.cy
    c, s = math.cos(-g.yaw), math.sin(-g.yaw)
    return dx * c - dy * s, dx * s + dy * c


def candidates(g: Geometry, cloud) -> np.ndarray:
    """Indices of the points that need a height: inside the box widened by the slope offset."""
    xl, yl = local_xy(g, cloud[:, 0], cloud[:, 1])
    with np.errstate(invalid="ignore"):
        return np.nonzero((np.abs(xl) <= g.length / 2.0 + g.slope_offset) &
                          (np.abs(yl) <= g.width / 2.0 + g.slope_offset))[0]


def flann_acc(cloud, x, y):
    """FLANN's float distance accumulator from (x, y, 0) to every point (float32 steps)."""
    qx, qy, qz = np.float32(x), np.float32(y), np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        d0, d1, d2 = qx - cloud[:, 0], qy - cloud[:, 1], qz - cloud[:, 2]
        acc = np.float32(0.0) + d0 * d0
        acc = acc + d1 * d1
        acc = acc + d2 * d2
    assert acc.dtype == np.float32
    return acc


def neighbours(cloud, x, y, radius) -> np.ndarray:
    """getTerrainHeight's valid neighbours of (x, y): finite, acc < float(r^2), 2-D distance in
    double <= r; in the radius search's (distance, index) order."""
    acc = flann_acc(cloud, x, y)
    fin = np.isfinite(cloud[:, :3]).all(axis=1)
    dx, dy = cloud[:, 0].astype(np.float64) - x, cloud[:, 1].astype(np.float64) - y
    with np.errstate(invalid="ignore"):
        ok = fin & (acc < np.float32(radius * radius)) & (np.sqrt(dx * dx + dy * dy) <= radius)
    idx = np.nonzero(ok)[0]
    return idx[np.lexsort((idx, acc[idx]))]


def rgb_of(i):
    """A distinct finite float per index (bits 0xC0000000 | i)."""
    return (np.uint32(0xC0000000) | np.asarray(i, np.uint32)).view(np.float32)


def _records(xyz, rgb=None):
    c = np.zeros((xyz.shape[0], 8), np.float32)
    c[:, :3] = xyz
    c[:, 3] = 1.0
    c[:, 4] = rgb_of(np.arange(xyz.shape[0])) if rgb is None else rgb
    return c


def _to_map(g: Geometry, xl, yl):
    c, s = math.cos(g.yaw), math.sin(g.yaw)
    return g.cx + xl * c - yl * s, g.cy + xl * s + yl * c


def _ground(g: Geometry, n, rng, skip=None):
    """n points of a 0.05 m lattice around the pit centre, nearest first (row-major among
    equals), z a multiple of 2^-10 within +-2^-7; skip(xl, yl) masks lattice points out."""
    side = int(1.13 * math.sqrt(max(n, 1))) + 9
    while True:   # grown until the n nearest lattice points lie inside the side x side window
        i = np.arange(side) - side // 2
        I, J = np.meshgrid(i, i, indexing="ij")
        I, J = I.ravel(), J.ravel()
        x, y = g.cx + I * 0.05, g.cy + J * 0.05
        if skip is not None:
            keep = ~skip(*local_xy(g, x.astype(np.float32), y.astype(np.float32)))
            I, J, x, y = I[keep], J[keep], x[keep], y[keep]
        order = np.argsort(I * I + J * J, kind="stable")[:n]
        if order.size == n and (n == 0 or (I * I + J * J)[order[-1]] <= (side // 2 - 1) ** 2):
            break
        side += max(side // 4, 8)
    z = rng.integers(-8, 9, n) * 2.0 ** -10
    return np.stack([x[order], y[order], z], 1).astype(np.float32), I[order], J[order]


@functools.lru_cache(maxsize=None)
def tile_case(n: int, seed: int = 1) -> Case:
    """C1: n points of the lattice in a random permutation of point order.  Every second point
    of the pit's box lies 0.05 m below the rest (carved); the others sit at the local mean's
    height, kept or carved by the mean's low bits.  One carved point first and one last."""
    t, q = yaw_pose()
    g = geometry(t, q, SMALL_PIT)
    rng = np.random.default_rng(seed)
    xyz, I, J = _ground(g, n, rng)
    xl, yl = local_xy(g, xyz[:, 0], xyz[:, 1])
    low = (np.abs(xl) <= g.length / 2 - 0.01) & (np.abs(yl) <= g.width / 2 - 0.01) & \
        ((I + J) % 2 == 0)
    xyz[low, 2] = -0.05
    perm = rng.permutation(n)
    low_at = np.nonzero(low[perm])[0]
    for dst, src in ((0, low_at[0]), (n - 1, low_at[-1])):
        perm[[dst, src]] = perm[[src, dst]]
    return Case(f"tile{n}", _records(xyz[perm]), t, q, SMALL_PIT)


@functools.lru_cache(maxsize=None)
def whole_tile_case(items: int) -> Case:
    """C2: tile 0, a middle tile and the last (partial) tile hold only points of a dense patch
    inside the box, 0.25 m below the ground (carved whatever the mean); the rest of the patch
    and the ground lattice fill the other tiles in random order."""
    n = {1: 5000, 2: 20000}[items]
    assert keep_items(n) == items
    t, q = yaw_pose(-35.0)
    g = geometry(t, q, WIDE_PIT)
    rng = np.random.default_rng(20 + items)
    XL, YL = np.meshgrid(np.arange(-29, 30) * 0.02, np.arange(-19, 20) * 0.02, indexing="ij")
    px, py = _to_map(g, XL.ravel(), YL.ravel())
    patch = np.stack([px, py, np.full(px.size, -0.25)], 1).astype(np.float32)
    patch = patch[rng.permutation(patch.shape[0])]
    ground, _, _ = _ground(g, n - patch.shape[0], rng)
    tile = keep_tile(n)
    slot_tile = np.arange(n) // tile
    carved = whole_tiles(n)
    in_carved = np.isin(slot_tile, carved)
    k = int(in_carved.sum())
    assert k < patch.shape[0]
    rest = np.concatenate([patch[k:], ground])
    xyz = np.empty((n, 3), np.float32)
    xyz[in_carved] = patch[:k]
    xyz[~in_carved] = rest[rng.permutation(rest.shape[0])]
    return Case(f"whole_tile{items}", _records(xyz), t, q, WIDE_PIT)


def whole_tiles(n: int):
    nt = -(-n // keep_tile(n))
    return [0, nt // 2, nt - 1]


@functools.lru_cache(maxsize=None)
def all_carved_case() -> Case:
    """C3: 300 points, all inside the box at one height: every point is carved."""
    t, q = yaw_pose()
    g = geometry(t, q, SMALL_PIT)
    XL, YL = np.meshgrid(np.linspace(-0.28, 0.28, 20), np.linspace(-0.18, 0.18, 15),
                         indexing="ij")
    px, py = _to_map(g, XL.ravel(), YL.ravel())
    xyz = np.stack([px, py, np.full(px.size, -0.25)], 1).astype(np.float32)
    return Case("all_carved", _records(xyz), t, q, SMALL_PIT)


NearestCase = namedtuple("NearestCase", "case hi lo px py n_finite")


@functools.lru_cache(maxsize=None)
def nearest_case(n_finite: int) -> NearestCase:
    """C4: no point within 2 m of the pit centre but two on its vertical, at z = +0.8 (input
    row 0) and z = -0.8 (a later row, an earlier cell of the index): every generated query and
    both points tie between them in float distance, and the lower input index wins.  Beside
    them an exact duplicate pair with different rgb, a ring of ground points to the requested
    number of finite points, and five NaN rows."""
    t, q = yaw_pose(10.0)
    g = geometry(t, q, SMALL_PIT)
    rng = np.random.default_rng(40 + n_finite)
    px, py = np.float32(g.cx), np.float32(g.cy)
    special = [[px, py, 0.8]]
    if n_finite >= 2:
        dx = np.float32(px + np.float32(0.05))
        special = [[px, py, 0.8], [dx, py, 0.9], [px, py, -0.8], [dx, py, 0.9]]
        assert n_finite >= 4
    ring, _, _ = _ground(g, n_finite - len(special), rng,
                         skip=lambda xl, yl: np.hypot(xl, yl) < 2.0)
    ring = ring[rng.permutation(ring.shape[0])]
    nan = np.full((5, 3), np.nan, np.float32)
    nan[:, 2] = 0.0
    xyz = np.concatenate([np.array(special, np.float32), nan[:2], ring[: ring.shape[0] // 2],
                          nan[2:], ring[ring.shape[0] // 2:]]).astype(np.float32)
    case = Case(f"nearest{n_finite}", _records(xyz), t, q, SMALL_PIT)
    return NearestCase(case, 0, 2 if n_finite >= 2 else None, float(px), float(py), n_finite)


@functools.lru_cache(maxsize=None)
def fallback_case() -> Case:
    """C5: a sheet of 6,825 points 0.8 m above the pit's widened box (z = 0.8 and a few
    multiples of 2^-12), nothing below it: each of its points is a candidate whose radius
    search is empty.  The ground lattice starts 0.55 m outside the widened box, so the sheet's
    rim finds the ground nearest (kept) and its middle the sheet itself (carved)."""
    t, q = yaw_pose(-15.0)
    g = geometry(t, q, SMALL_PIT)
    rng = np.random.default_rng(5)
    XL, YL = np.meshgrid(np.arange(-45, 46) * 0.0125, np.arange(-37, 38) * 0.0125, indexing="ij")
    px, py = _to_map(g, XL.ravel(), YL.ravel())
    pz = 0.8 + rng.integers(-3, 4, px.size) * 2.0 ** -12
    sheet = np.stack([px, py, pz], 1).astype(np.float32)
    hx, hy = g.length / 2 + g.slope_offset + 0.55, g.width / 2 + g.slope_offset + 0.55
    ground, _, _ = _ground(g, 3000, rng, skip=lambda xl, yl: (np.abs(xl) < hx) & (np.abs(yl) < hy))
    xyz = np.concatenate([sheet, ground])
    return Case("fallback", _records(xyz[rng.permutation(xyz.shape[0])]), t, q, SMALL_PIT)


EIGHTH_PIT = dict(l_shape_enabled=0, length=1.5, width=1.0, point_density=0.125,
                  terrain_search_radius=0.5)


@functools.lru_cache(maxsize=None)
def radius_tie_case(variant: str) -> Case:
    """C6: a 2^-3 m lattice (48 x 48) under an unrotated pit whose centre, bottom lattice and
    the cloud's minimum corner lie on it: every lattice query has four points at exactly the
    radius (acc == r2: FLANN's strict < leaves them out).
    "flat": z = 0.  "lifted": the odd points at +-2^-12 (their acc is two ulps past r2; the even
    ones' stays on it, and a count that took them in would move a non-zero mean).  "tiny": every
    point at 0 or +-2^-14, below half an ulp of r2, so acc == r2 holds with a non-zero z."""
    t, q = (1.0, -0.5, 0.25), (0.0, 0.0, 0.0, 1.0)
    g = geometry(t, q, EIGHTH_PIT)
    assert (g.cx, g.cy, g.yaw) == (5.0, 0.5, 0.0)
    i = np.arange(-24, 24)
    I, J = np.meshgrid(i, i, indexing="ij")
    I, J = I.ravel(), J.ravel()
    z = np.zeros(I.size)
    sign = np.where((I * 7 + J * 3) % 5 < 3, 1.0, -1.0)
    if variant == "lifted":
        z = np.where((I + J) % 2 != 0, sign * 2.0 ** -12, 0.0)
    elif variant == "tiny":
        z = np.where((I * 5 + J * 11) % 7 < 5, sign * 2.0 ** -14, 0.0)
    else:
        assert variant == "flat"
    xyz = np.stack([g.cx + I * 0.125, g.cy + J * 0.125, z], 1).astype(np.float32)
    rng = np.random.default_rng(6)
    return Case(f"radius_{variant}", _records(xyz[rng.permutation(xyz.shape[0])]), t, q, EIGHTH_PIT)


@functools.lru_cache(maxsize=None)
def layout_case() -> Case:
    """C7: 2,000 points of the C1 lattice, a distinct rgb float per point."""
    c = tile_case(2000, seed=7)
    return Case("layout", c.cloud, c.t, c.q, c.kw)


def pack_layout(cloud, layout):
    """The cloud's points as raw records of one layout -> (uint8 (n, step), step, (ox, oy, oz),
    expected rgb of a kept record).  Bytes that are no field hold the point's rgb bits or 0xA5:
    a reader of the wrong offset sees it."""
    n = cloud.shape[0]
    step, offs, rgb_at = {"step12": (12, (0, 4, 8), None), "step16": (16, (0, 4, 8), 12),
                          "step20": (20, (0, 4, 8), 16), "step32": (32, (0, 4, 8), 16),
                          "step32_shifted": (32, (20, 24, 28), 16)}[layout]
    raw = np.full((n, step), 0xA5, np.uint8)
    for a in range(3):
        raw[:, offs[a]:offs[a] + 4] = cloud[:, a:a + 1].copy().view(np.uint8)
    if rgb_at is not None:
        raw[:, rgb_at:rgb_at + 4] = cloud[:, 4:5].copy().view(np.uint8)
    want = cloud[:, 4].copy() if step >= 20 else np.zeros(n, np.float32)
    return np.ascontiguousarray(raw), step, offs, want


@functools.lru_cache(maxsize=None)
def sum_case(variant: str) -> Case:
    """C8: 4,000 points of the lattice under the small pit.
    "exact": every z a float of magnitude in [2^-19, 2^-5), so a multiple of 2^-42: a query's
    <= 1,024 neighbours sum below 2^5 in 47 bits, and the plain double sum is exact.
    "inexact": one point in 64 at z = 0.25, the others at +2^-55 (three in four) or -2^-55: the
    exact sum needs more than 53 bits, and the plain sum depends on its order."""
    t, q = yaw_pose(30.0)
    g = geometry(t, q, SMALL_PIT)
    rng = np.random.default_rng(8)
    xyz, I, J = _ground(g, 4000, rng)
    if variant == "exact":
        mant = 1.0 + rng.integers(0, 1 << 23, 4000) * 2.0 ** -23
        z = rng.choice([-1.0, 1.0], 4000) * mant * 2.0 ** rng.integers(-19, -5, 4000)
        xyz[:, 2] = z.astype(np.float32)
        assert np.array_equal(xyz[:, 2].astype(np.float64), z)
    else:
        assert variant == "inexact"
        tiny = np.where(rng.integers(0, 4, 4000) < 3, 1.0, -1.0) * 2.0 ** -55
        xyz[:, 2] = np.where((I % 8 == 0) & (J % 8 == 0), 0.25, tiny).astype(np.float32)
    return Case(f"sum_{variant}", _records(xyz[rng.permutation(4000)]), t, q, SMALL_PIT)


_REF = {}


def reference(oracle, case: Case):
    """oracle.excavate(case), computed once per process: (keep, surf, area, pose)."""
    if case.name not in _REF:
        _REF[case.name] = oracle.excavate(case.cloud, case.t, case.q, oracle.exc_params(**case.kw))
        for a in _REF[case.name]:
            a.flags.writeable = False
    return _REF[case.name]
