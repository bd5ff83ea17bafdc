"""The scenes of tests/test_cand_ref.py (CPU) and tests/test_candidates_gpu.py: boxes, lattices
and terrains at which generateCandidatePositions / getGroundHeight take every branch -- and the
device's kernels every path -- that the golden scene never reaches.  All tiny: terrains of at
most ~10,000 points; lattices of 0 to 4,225 points, but for gs257 (66,049 points, 4,048 of them
outside the box) and the two `land_*` cases (323^2 and 324^2: either side of the 4 MiB landing
threshold of pcp_generate_candidates).

A case is a dict: name, terrain ((N, 3) float32; N = 0: the empty cloud, no ground query), bbox
(6), search_radius, sensor_height, num_candidates, zx (5), and `sampled` (the lattice is too
large for the Python reference in full: every 97th lattice point and every 16th pose).

Everything is seeded; the searched points (boundary straddles, fused / unfused disagreements) are
found again on every run, in well under a second."""
import functools
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
NO_TERRAIN = np.zeros((0, 3), F32)
SAMPLE_LATTICE, SAMPLE_POSES = 97, 16


def _case(name, bbox, radius, nc, terrain=NO_TERRAIN, sensor_height=1.1, zx=(-50.0, -50.0),
          sampled=False):
    return {"name": name, "terrain": np.ascontiguousarray(terrain, F32).reshape(-1, 3),
            "bbox": np.array(bbox, np.float64), "search_radius": float(radius),
            "sensor_height": float(sensor_height), "num_candidates": int(nc),
            "zx": np.array([zx[0], zx[1], 0.0, 0.0, 0.0], np.float64), "sampled": sampled}


def lattice_xy(c):
    """The lattice coordinates as the reference computes them (doubles): (xs (gs,), ys (gs,))."""
    gs = int(math.ceil(math.sqrt(c["num_candidates"])))
    bb, r = c["bbox"], c["search_radius"]
    x0, x1, y0, y1 = bb[0] - r, bb[1] + r, bb[2] - r, bb[3] + r
    xs, ys = (x1 - x0) / (gs - 1), (y1 - y0) / (gs - 1)
    return (np.array([x0 + i * xs for i in range(gs)]), np.array([y0 + j * ys for j in range(gs)]))


# ---- the boxes ---------------------------------------------------------------------------------
DYADIC = dict(bbox=(0.0, 4.0, 0.0, 4.0, 0.0, 2.0), radius=2.0, nc=81, sensor_height=1.0)
ND10 = dict(bbox=(0.3, 4.1, -1.7, 2.2, -0.4, 1.3), radius=3.3, nc=100)
FAR_T = (3000.0, -2500.0)
FAR10 = dict(bbox=(ND10["bbox"][0] + FAR_T[0], ND10["bbox"][1] + FAR_T[0],
                   ND10["bbox"][2] + FAR_T[1], ND10["bbox"][3] + FAR_T[1], -0.4, 1.3),
             radius=3.3, nc=100)


def _extent(box):
    bb, r = box["bbox"], box["radius"]
    return (min(bb[0], bb[1]) - r, max(bb[0], bb[1]) + r, min(bb[2], bb[3]) - r,
            max(bb[2], bb[3]) + r)


# ---- terrains over a box's lattice -------------------------------------------------------------
def _terrain(kind, box, seed):
    g = np.random.default_rng(seed)
    x0, x1, y0, y1 = _extent(box)

    def uniform(n, z0, z1, pad=1.0):
        return np.stack([g.uniform(x0 - pad, x1 + pad, n), g.uniform(y0 - pad, y1 + pad, n),
                         g.uniform(z0, z1, n)], 1).astype(F32)
    if kind == "dense":
        return uniform(10_000, -2.5, 2.5)
    if kind == "sparse":       # ~300 points over 12 x 12 x 5 m: rows of 0 to 3 points
        return uniform(300, -2.5, 2.5)
    if kind == "sunk":         # the ground is negative wherever there is any
        return uniform(3_000, -1.9, -0.2)
    if kind == "above":        # nothing within FLANN's radius of z = 0
        return uniform(3_000, 2.1, 3.0)
    if kind == "away":         # 20 m from every lattice point: the window misses the grid
        return uniform(500, -0.5, 0.5) + np.array([x1 - x0 + 22.0, 0.0, 0.0], F32)
    if kind == "one":          # a one-point index, 0.4 m from the first lattice point
        return np.array([[x0 + 0.3, y0 + 0.25, -0.7]], F32)
    if kind == "two":
        return np.array([[x0 + 0.3, y0 + 0.25, -0.7], [x1 - 0.2, y1 + 0.3, 0.9]], F32)
    raise KeyError(kind)


TERRAINS = ("dense", "sparse", "sunk", "above", "away", "one", "two")


def _valid_lattice(c):
    """(x, y) of the lattice points outside the box, x-major."""
    xs, ys = lattice_xy(c)
    bb = c["bbox"]
    return [(i, j, x, y) for i, x in enumerate(xs) for j, y in enumerate(ys)
            if not (bb[0] <= x <= bb[1] and bb[2] <= y <= bb[3])]


def _dist(px, py, x, y):
    """getGroundHeight's 2-D distance: float points, double query, every operation rounded."""
    dx, dy = np.asarray(px, F32).astype(np.float64) - x, np.asarray(py, F32).astype(np.float64) - y
    return np.sqrt(dx * dx + dy * dy)


def straddle(x, y, g, n=16384):
    """Two float points around (x, y): the one whose double 2-D distance is the largest found
    below 1.0 and the one whose distance is the smallest found at or above 1.0, over n seeded
    directions and the five float neighbours of the circle's y on each -> ((px, py, d), (..))."""
    th = g.uniform(0.0, 2.0 * math.pi, n)
    px = (x + np.cos(th)).astype(F32)
    dx = px.astype(np.float64) - x
    py = (y + np.sqrt(np.maximum(1.0 - dx * dx, 0.0)) * np.where(np.sin(th) < 0, -1.0, 1.0))
    py = py.astype(F32)
    col, up, dn = [py], py, py
    for _ in range(2):
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
        col += [up, dn]
    PX, PY = np.tile(px, 5), np.concatenate(col)
    d = _dist(PX, PY, x, y)
    a = int(np.argmax(np.where(d < 1.0, d, -1.0)))
    b = int(np.argmin(np.where(d >= 1.0, d, 9.0)))
    assert d[a] < 1.0 <= d[b]
    return (PX[a], PY[a], float(d[a])), (PX[b], PY[b], float(d[b]))


def _spread(c, step=2):
    """Lattice points outside the box, every `step`-th in i and j: more than 2.2 m apart, so a
    point placed 1 m from one of them lies in no other's window."""
    return [(x, y) for i, j, x, y in _valid_lattice(c) if i % step == 0 and j % step == 0]


def _nd_boundaries(box, seed, edge=False):
    """For each spread lattice point two points: the nearest below 1.0 found at z = 0.5 (the
    ground) and the nearest at or above 1.0 at z = 1.0 (not the ground).  Float points a metre
    from a double query are ~1e-7 apart, so "nearest" is what the search finds, within 1e-9
    (tests/test_cand_ref.py asserts it; ~1e-11 in fact); the distances 1.0 itself and the double
    below it are reached in `fuse`, where the points lie next to the origin.  edge: every other
    lattice point instead gets a point exactly 1 m from the FLOAT query along x, on the side
    where it is closer than 1 m to the double one."""
    c = _case("tmp", box["bbox"], box["radius"], box["nc"])
    g = np.random.default_rng(seed)
    pts, dists = [], []
    for k, (x, y) in enumerate(_spread(c)):
        qx = float(F32(x))
        if edge and k % 2 and qx != x:
            pts.append((F32(qx + (1.0 if x > qx else -1.0)), F32(y), 0.75))
            continue
        lo, hi = straddle(x, y, g)
        pts += [(lo[0], lo[1], 0.5), (hi[0], hi[1], 1.0)]
        dists.append((lo[2], hi[2]))
    return np.array(pts, F32), dists


def _dyadic_boundaries():
    """Points on the boundaries of the strict tests, each the highest candidate for the ground
    of one lattice point of the dyadic lattice (offsets from a zero coordinate, so the float
    differences are exact):
      (-2, -2): a point at 2-D distance exactly 1.0, z = 1        -> not the ground (0.0)
      (-2,  2): straight below at z = -2: squared distance 4.0f   -> not a neighbour (0.0)
      (-2,  6): straight above at z = +2                          -> not a neighbour (0.0)
      ( 0, -2): z = float(sqrt 3) rounded down, dx below 1        -> a neighbour, the ground
      ( 0,  6): z = float(sqrt 3) rounded up, the same dx         -> not a neighbour (0.0)
      (-2,  0): dy = the float below 1, z = 0.25                  -> the ground
      ( 6,  0): dy = the float above 1                            -> not the ground (0.0)"""
    s3 = F32(math.sqrt(3.0))
    s3_dn = s3 if float(s3) ** 2 < 3.0 else np.nextafter(s3, F32(0))
    s3_up = np.nextafter(s3_dn, F32(2))
    # a dx below 1 whose float sum with z^2 passes for s3_dn and fails for s3_up
    dx = None
    for k in range(1, 64):
        t = F32(1.0) - F32(k) * F32(2.0 ** -24)
        acc = [F32(0) + t * t + F32(0) * F32(0) + z * z for z in (s3_dn, s3_up)]
        if acc[0] < F32(4.0) <= acc[1]:
            dx = t
            break
    assert dx is not None
    below1, above1 = np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2))
    return np.array([(-1.0, -2.0, 1.0), (-2.0, 2.0, -2.0), (-2.0, 6.0, 2.0),
                     (dx, -2.0, s3_dn), (dx, 6.0, s3_up),
                     (-2.0, below1, 0.25), (6.0, above1, 0.25)], F32)


def _rows_terrain(c):
    """Rows of exactly k = 1 .. 9 points (one y, z within one cell, x across the window), the
    highest last in x: the ground of k lattice points 2.3 m apart."""
    pts = []
    for k, (x, y) in enumerate(_spread(c)[:9], start=1):
        for i in range(k):
            pts.append((x - 0.45 + 0.1 * i, y + 0.05, 0.3 + 1e-5 * i))
    return np.array(pts, F32)


# ---- fused / unfused disagreements -------------------------------------------------------------
FUSE_R = 0.25


def _fuse_corner():
    """(x0, y0) ~ (0.28, 0.96), 1 m from the origin to a few ulps, that the lattice arithmetic
    reproduces exactly: (y0 + r) - r == y0 and (r - x0) - r == -x0."""
    x0, y0 = 0.28, 0.96
    while (-x0 + FUSE_R) - FUSE_R != -x0 or (x0 - FUSE_R) + FUSE_R != x0:
        x0 = math.nextafter(x0, 1.0)
    while (y0 + FUSE_R) - FUSE_R != y0:
        y0 = math.nextafter(y0, 1.0)
    assert abs(x0 * x0 + y0 * y0 - 1.0) < 1e-14
    return x0, y0


def _fuse_search(sx, want_unfused_in, g, tries=100_000):
    """A float point ~2^-40 m from the origin for the lattice corner (sx x0, y0): float points
    there are spaced far below a double ulp of 1, so dx and dy run through consecutive doubles.
    Its x has the corner's sign, which puts it ~1e-12 m outside the other corner's circle.
    want_unfused_in: fl(fl(dx dx) + fl(dy dy)) < 1 while the exact sum rounds to >= 1; else the
    other way round."""
    x0, y0 = _fuse_corner()
    x = sx * x0
    ax = g.uniform(0.25, 1.0, tries) * 2.0 ** -40
    px = (sx * ax).astype(F32)
    # x0^2 + y0^2 = 1: dist^2 - 1 ~ -2 x0 |px| - 2 y0 py, so py ~ -(x0 / y0) |px|
    py = (-(x0 / y0) * ax + g.uniform(-1.0, 1.0, tries) * 2.0 ** -46).astype(F32)
    dx, dy = px.astype(np.float64) - x, py.astype(np.float64) - y0
    s = dx * dx + dy * dy
    for k in np.nonzero(np.abs(s - 1.0) <= 4.0 * 2.0 ** -52)[0]:
        a, b = Fraction(float(dx[k])), Fraction(float(dy[k]))
        once = float(a * a + b * b)
        # (the unfused sum is 1.0 itself or the double below it, and so is its square root: the
        # smallest distance at or above 1.0 and the largest below it)
        if (s[k] == 1.0 - 2.0 ** -53 and once >= 1.0) if want_unfused_in else \
                (s[k] == 1.0 and once < 1.0):
            assert math.sqrt(s[k]) == s[k]
            return px[k], py[k]
    raise AssertionError("fuse search: nothing found")


def _fuse_case():
    """gs 2 over a box symmetric in x: the corners (+-x0, y0) are 1 m from the origin.
    Corner +: a point (z = 0.9) at 1.0 or beyond unfused, below 1.0 with the sum rounded once ->
    the ground is 0.0.  Corner -: a point (z = 0.7) below 1.0 unfused, at 1.0 with the sum
    rounded once -> the ground is 0.7.  (tests/test_cand_ref.py asserts the two grounds.)"""
    g = np.random.default_rng(0xF05E)
    x0, y0 = _fuse_corner()
    a = _fuse_search(+1.0, False, g)
    b = _fuse_search(-1.0, True, g)
    pts = np.array([(a[0], a[1], 0.9), (b[0], b[1], 0.7)], F32)
    bbox = (-x0 + FUSE_R, x0 - FUSE_R, y0 + FUSE_R, y0 + 2.0, 0.0, 2.0)
    return _case("fuse", bbox, FUSE_R, 4, pts)


# ---- the list ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, box, terrain=NO_TERRAIN, **kw):
        args = dict(box, **kw)
        out.append(_case(name, args.pop("bbox"), args.pop("radius"), args.pop("nc"), terrain,
                         **args))
    # dyadic: the lattice is the integers -2 .. 6; (-2, -2) and (-1, -2) are exactly 0.5 from
    # zx120 (kept), in the second case (-2, -2) is 0.25 from it (dropped)
    add("dyadic9", DYADIC, zx=(-1.5, -2.0))
    add("dyadic9_zx25", DYADIC, zx=(-2.0, -1.75))
    add("dyadic9_boundaries", DYADIC, _dyadic_boundaries())
    add("nd10", ND10, zx=(-2.9, -4.6))
    add("nd10_boundaries", ND10, _nd_boundaries(ND10, 0xB0)[0])
    add("nd10_rows", ND10, _rows_terrain(_case("tmp", ND10["bbox"], ND10["radius"], 100)))
    for k, kind in enumerate(TERRAINS):
        add("dyadic9_" + kind, DYADIC, _terrain(kind, DYADIC, 100 + k))
        add("nd10_" + kind, ND10, _terrain(kind, ND10, 200 + k))
    add("far_boundaries", FAR10, _nd_boundaries(FAR10, 0xFA, edge=True)[0])
    add("far_dense", FAR10, _terrain("dense", FAR10, 300))
    out.append(_fuse_case())
    # box [4, 0] x [4, 0]: nothing is "inside", the centre lattice point dies on hd < 0.1
    add("inverted", dict(bbox=(4.0, 0.0, 4.0, 0.0, 0.0, 2.0), radius=4.0, nc=25))
    # a small box 20 m below: elevation above 85 degrees within 1.85 m of its centre
    steep = dict(bbox=(0.0, 0.4, 0.0, 0.4, -20.5, -19.5), radius=3.0, nc=81)
    add("steep", steep)
    add("steep_sparse", steep, _terrain("sparse", steep, 400))
    # integer lattices of 1,089 and 4,225 points: 2 and 5 compaction chunks, the last partial,
    # valid only on the border ring; radius 0: every point on or inside the box
    g33 = dict(bbox=(0.0, 30.0, 0.0, 30.0, 0.0, 2.0), radius=1.0, nc=1089)
    g65 = dict(bbox=(0.0, 62.0, 0.0, 62.0, 0.0, 2.0), radius=1.0, nc=4225)
    add("gs33", g33, _terrain("sparse", g33, 500))
    add("gs65", g65, _terrain("sparse", g65, 501))
    add("gs65_r0", dict(g65, radius=0.0), _terrain("sparse", g65, 501))
    # 66,049 lattice points a quarter metre apart, 4,048 of them outside the box: past the
    # 65,535 up to which pcp_generate_and_score fuses the two stages
    add("gs257", dict(g65, nc=257 * 257), _terrain("sparse", g65, 501))
    for name, nc in (("gs1", 1), ("gs2", 2), ("nc0", 0)):
        add(name, dict(DYADIC, nc=nc))
        add(name + "_sparse", dict(DYADIC, nc=nc), _terrain("sparse", DYADIC, 600))
    # either side of the landing threshold: L 40 + 4 bytes against 4 MiB
    land = _terrain("dense", DYADIC, 700)[:2000]
    add("land_pinned", dict(DYADIC, nc=323 * 323, sensor_height=1.1), land, sampled=True)
    add("land_edge", dict(DYADIC, nc=104_900, sensor_height=1.1), land, sampled=True)
    return {c["name"]: c for c in out}


def small_cases():
    return {k: c for k, c in cases().items() if not c["sampled"]}


@functools.lru_cache(maxsize=None)
def reference(name, mut=None):
    """tests/cand_ref.py on a (not sampled) case, computed once per session ->
    (poses, reasons, undecided)."""
    import cand_ref

    c = cases()[name]
    assert not c["sampled"]
    return cand_ref.candidates(c["terrain"], c["bbox"], c, c["zx"], mut)


def oracle_poses(oracle, c):
    """The oracle's candidates of a case (an empty terrain as the reference's empty cloud)."""
    T = oracle.Cloud(c["terrain"]) if c["terrain"].shape[0] else None
    p = oracle.vl_params(search_radius=c["search_radius"], sensor_height=c["sensor_height"],
                         num_candidates=c["num_candidates"])
    return oracle.generate_candidates(T, c["bbox"], p, c["zx"], terrain_empty=T is None)
