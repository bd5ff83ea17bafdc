"""Brute-force restatement of generateCandidatePositions and getGroundHeight
(virtual_lidar.cpp:550-625) in numpy and plain Python: no grid, no tree, nothing shared with
oracle/ or the kernels.  The angles come from tests/cr_ref.py (correctly rounded, or "undecided"),
the IEEE special values where an argument is zero.

  ground_height(pts, x, y)          the maximum z of the points that pass FLANN's float predicate
                                    around (float(x), float(y), 0) and lie closer than 1.0 to
                                    (x, y) in double, over ALL points; 0.0 when there is none
  candidates(pts, bbox, params, zx) the lattice loop, x-major -> (poses, reasons, undecided)
  Lattice                           the same, one lattice point or one pose at a time

`mut` names one deliberate fault (MUTATIONS); tests/test_cand_ref.py proves that the cases of
tests/cand_cases.py tell each from the reference.  The last four are models of how the device's
grid walk, block maximum and compaction could go wrong, expressed over the brute-force point
set (GRID_CELL: the edge of the terrain index' smallest cell)."""
import math
from fractions import Fraction

import numpy as np

import cr_ref

F32 = np.float32
MIN_ELEV = -85.0 * math.pi / 180.0
MAX_ELEV = 85.0 * math.pi / 180.0
REASONS = ("zx", "inside", "hd", "elev", "valid")
GRID_CELL = 0.112
MARGIN = 1e-3
CHUNK = 1024

MUTATIONS = (
    "zx_le",            # closer than 0.5 to zx120: <= instead of <
    "flann_le",         # FLANN's squared distance: <= 4 instead of < 4
    "d2_le",            # the 2-D distance: <= 1.0 instead of < 1.0
    "box_strict",       # inside the box: strict instead of inclusive
    "d2_float_query",   # the 2-D distance from the float query instead of the double
    "d2_fused",         # dx dx + dy dy rounded once instead of three times
    "max_init0",        # the maximum starts at 0.0 instead of "none"
    "win_float",        # x / y window strictly within 1 of the float query, no margin
    "rows64",           # only the first 64 rows of the window reach the block maximum
    "tail4",            # a row's last n mod 4 points are not looked at
    "chunk_base",       # the compaction forgets the poses of the chunks before
)


def _get(params, name):
    return params[name] if isinstance(params, dict) else getattr(params, name)


def _rows(p, x, y):
    """The grid model of the row mutations: per point (row number in the window or -1, cell x)."""
    p64 = p.astype(np.float64)
    o = p64.min(0) - GRID_CELL
    n = np.floor((p64.max(0) - o) / GRID_CELL).astype(np.int64) + 2
    cell = np.floor((p64 - o) / GRID_CELL).astype(np.int64)

    def rng(lo, hi, a):
        return (max(math.floor((lo - o[a]) / GRID_CELL), 0),
                min(math.floor((hi - o[a]) / GRID_CELL), int(n[a]) - 1))
    x0, x1 = rng(x - 1.0 - MARGIN, x + 1.0 + MARGIN, 0)
    y0, y1 = rng(y - 1.0 - MARGIN, y + 1.0 + MARGIN, 1)
    z0, z1 = rng(-2.0 - MARGIN, 2.0 + MARGIN, 2)
    inside = ((cell[:, 0] >= x0) & (cell[:, 0] <= x1) & (cell[:, 1] >= y0) & (cell[:, 1] <= y1) &
              (cell[:, 2] >= z0) & (cell[:, 2] <= z1))
    row = (cell[:, 1] - y0) + (y1 - y0 + 1) * (cell[:, 2] - z0)
    return np.where(inside, row, -1), cell[:, 0]


def ground_height(pts, x, y, mut=None):
    """getGroundHeight(x, y) over all points of pts ((N, >= 3) float32, None or empty)."""
    if pts is None or len(pts) == 0:
        return 0.0
    p = np.ascontiguousarray(np.asarray(pts)[:, :3], F32)
    x, y = float(x), float(y)
    qx, qy = F32(x), F32(y)
    keep = np.ones(p.shape[0], bool)
    if mut == "win_float":
        for a, q in ((0, qx), (1, qy)):
            keep &= np.abs(p[:, a].astype(np.float64) - float(q)) < 1.0
    elif mut in ("rows64", "tail4"):
        row, cx = _rows(p, x, y)
        keep = row >= 0
        if mut == "rows64":
            keep &= row < 64
        else:
            for r in np.unique(row[keep]):
                idx = np.nonzero(row == r)[0]
                idx = idx[np.argsort(cx[idx], kind="stable")]
                if idx.size % 4:
                    keep[idx[-(idx.size % 4):]] = False
    # FLANN L2_Simple<float>, every operation rounded to float on its own
    d0, d1, d2 = qx - p[:, 0], qy - p[:, 1], F32(0.0) - p[:, 2]
    acc = F32(0.0) + d0 * d0
    acc = acc + d1 * d1
    acc = acc + d2 * d2
    keep &= (acc <= F32(4.0)) if mut == "flann_le" else (acc < F32(4.0))
    # the 2-D test in double: two products, one sum, one square root, each rounded on its own
    # (numpy's element-wise operations do not contract)
    s = p[keep].astype(np.float64)
    fq = mut == "d2_float_query"
    dx, dy = s[:, 0] - (float(qx) if fq else x), s[:, 1] - (float(qy) if fq else y)
    if mut == "d2_fused":
        sq = np.array([float(Fraction(a) * Fraction(a) + Fraction(b) * Fraction(b))
                       for a, b in zip(dx.tolist(), dy.tolist())], np.float64)
    else:
        sq = dx * dx + dy * dy
    d = np.sqrt(sq)
    z = s[:, 2][(d <= 1.0) if mut == "d2_le" else (d < 1.0)]
    if mut == "max_init0":
        z = np.append(z, 0.0)
    return float(z.max()) if z.size else 0.0


def atan2_exact(y, x):
    """(atan2(y, x) correctly rounded, undecided): the IEEE special value (libm's: +-0, +-M_PI,
    +-M_PI_2 as doubles) when an argument is zero, tests/cr_ref.py otherwise."""
    if y == 0.0 or x == 0.0:
        return math.atan2(y, x), 0
    v = cr_ref.cr_atan2(y, x)
    return (math.nan, 1) if v is None else (v, 0)


class Lattice:
    """The lattice of one call: its constants as the reference computes them (:553-567)."""

    def __init__(self, pts, bbox, params, zx, mut=None):
        self.pts = None if pts is None or len(pts) == 0 else \
            np.ascontiguousarray(np.asarray(pts)[:, :3], F32)
        bb = [float(v) for v in bbox]
        self.gminx, self.gmaxx, self.gminy, self.gmaxy = bb[:4]
        r = float(_get(params, "search_radius"))
        self.sensor_height = float(_get(params, "sensor_height"))
        self.exminx, exmaxx = self.gminx - r, self.gmaxx + r
        self.exminy, exmaxy = self.gminy - r, self.gmaxy + r
        self.cx, self.cy = (self.gminx + self.gmaxx) / 2.0, (self.gminy + self.gmaxy) / 2.0
        self.cz = (bb[4] + bb[5]) / 2.0
        nc = int(_get(params, "num_candidates"))
        self.gs = int(math.ceil(math.sqrt(float(nc)))) if nc > 0 else 0
        with np.errstate(all="ignore"):   # gs == 1: 0 / 0, a NaN lattice, as in C
            self.xs = float(np.float64(exmaxx - self.exminx) / np.float64(self.gs - 1))
            self.ys = float(np.float64(exmaxy - self.exminy) / np.float64(self.gs - 1))
        self.zx = (float(zx[0]), float(zx[1]))
        self.mut = mut

    @property
    def L(self):
        return self.gs * self.gs

    def xy(self, l):
        i, j = divmod(l, self.gs)
        return self.exminx + i * self.xs, self.exminy + j * self.ys

    def angles(self, x, y, z):
        """(elevation, yaw, undecided) of a sensor at (x, y, z) looking at the box centre."""
        dx, dy, dz = self.cx - x, self.cy - y, self.cz - z
        hd = math.sqrt(dx * dx + dy * dy)
        elev, u0 = atan2_exact(-dz, hd)
        yaw, u1 = atan2_exact(dy, dx)
        return elev, yaw, u0 + u1

    def ground(self, x, y):
        return ground_height(self.pts, x, y, self.mut)

    def point(self, l):
        """Lattice point l = i * gs + j -> (reason, pose (5,) or None, undecided)."""
        x, y = self.xy(l)
        ddx, ddy = x - self.zx[0], y - self.zx[1]
        d = math.sqrt(ddx * ddx + ddy * ddy)
        if (d <= 0.5) if self.mut == "zx_le" else (d < 0.5):
            return "zx", None, 0
        if self.mut == "box_strict":
            inside = self.gminx < x < self.gmaxx and self.gminy < y < self.gmaxy
        else:
            inside = self.gminx <= x <= self.gmaxx and self.gminy <= y <= self.gmaxy
        if inside:
            return "inside", None, 0
        z = self.ground(x, y) + self.sensor_height
        dx, dy = self.cx - x, self.cy - y
        if math.sqrt(dx * dx + dy * dy) < 0.1:
            return "hd", None, 0
        elev, yaw, und = self.angles(x, y, z)
        if elev >= MIN_ELEV and elev <= MAX_ELEV:      # (NaN: neither, as in C)
            return "valid", (x, y, z, -math.pi / 2 + elev, yaw), und
        return "elev", None, und


def candidates(pts, bbox, params, zx, mut=None):
    """-> (poses (n, 5) float64, reasons: list of L reason codes, undecided cr_atan2 calls)."""
    lat = Lattice(pts, bbox, params, zx, mut)
    poses, reasons, und = [], [], 0
    for l in range(lat.L):
        if mut == "chunk_base" and l and l % CHUNK == 0:
            poses = []                                  # the chunk writes from slot 0 again
        why, pose, u = lat.point(l)
        reasons.append(why)
        und += u
        if pose is not None:
            poses.append(pose)
    return np.array(poses, np.float64).reshape(-1, 5), reasons, und


def ulp_distance(a, b):
    """Element-wise distance in doubles between two arrays: their bit patterns as ordered
    integers (0 for equal bits; -0.0 and +0.0 are one apart)."""
    def key(v):
        u = np.ascontiguousarray(v, np.float64).view(np.int64)
        return np.where(u < 0, np.int64(-2 ** 63) - u - 1, u)   # -0.0 -> -1, below +0.0 -> 0
    return np.abs(key(a) - key(b))


def check_sampled(lat, poses, every_lattice, every_pose):
    """A pose list of a lattice too large for the reference in full: every `every_lattice`-th
    lattice point must be in the list with the reference's z, or absent when the reference
    rejects it; every `every_pose`-th pose must carry the reference's angles, bit for bit ->
    (lattice points checked, of them valid, poses checked, undecided)."""
    poses = np.ascontiguousarray(poses, np.float64)
    where = {poses[k, :2].tobytes(): k for k in range(poses.shape[0])}
    n_valid = und = 0
    picked = range(0, lat.L, every_lattice)
    for l in picked:
        why, pose, _ = lat.point(l)
        k = where.get(np.array(lat.xy(l), np.float64).tobytes())
        if pose is None:
            assert k is None, f"lattice point {l} ({why}) is in the pose list"
        else:
            assert k is not None, f"lattice point {l} is missing from the pose list"
            assert poses[k, 2].tobytes() == np.float64(pose[2]).tobytes(), (l, poses[k], pose)
            n_valid += 1
    rows = range(0, poses.shape[0], every_pose)
    for k in rows:
        x, y, z = (float(v) for v in poses[k, :3])
        elev, yaw, u = lat.angles(x, y, z)
        und += u
        want = np.array([-math.pi / 2 + elev, yaw])
        assert want.tobytes() == poses[k, 3:].tobytes(), (k, poses[k], want)
    return len(picked), n_valid, len(rows), und
