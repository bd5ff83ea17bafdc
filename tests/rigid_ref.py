"""A plain SE(3) reference and the quaternions with roll and pitch that test_rigid_ref.py (CPU)
and test_rigid_gpu.py (GPU) share.

apply() is not the Eigen matrix formula the library and the oracle restate.  It rotates by the
cross-product form

    v' = v + 2 w (u x v) + 2 u x (u x v) + t,        q = (u, w),

in float64 from the float64 q and t.  For a unit q this is the rotation q v q* exactly; for any
other q it is NOT what Eigen's toRotationMatrix() gives (Eigen does not normalise), so the bound
below is asked of unit quaternions only.

bound(): what a float result may differ from apply() by, per output component a, for unit q:

    16 * 2^-24 * (|x| + |y| + |z| + |t_a|)                                  (u = 2^-24)

derived, not measured:
  * q narrowed to float moves each component by at most u (|q_i| <= 1).  A matrix entry is a sum
    of products 2 q_i q_j, so it moves by about 4 u;
  * an entry costs at most 3 roundings in float (2 q_i, the product, the sum or 1 - (a + b)) of
    values of magnitude up to 2: about 6 u.  Together the float entry is within about 10 u of the
    exact one, and it multiplies a coordinate: 10 u |v_j| per term;
  * the three products and three sums of a row round once each (|m_ij| <= 1): the products'
    roundings are u |v_j| each, u (|x| + |y| + |z|) together, and each sum's is u of a partial
    sum no larger than |x| + |y| + |z| + |t_a|: about 4 u of that sum;
  * t narrowed to float: u |t_a|, inside the slack of the rounded-up constants.
  10 u + 4 u = 14 u, rounded up to 16 u.  The CPU oracle stays within 3.2 u of that sum over
200 random unit quaternions (t, p in [-50, 50], 2,000 points each), a fifth of the bound; a
wrong sign or a transposed entry is off by about 10^6 u.  The bound is the derived one and is
not tightened to the measured figure."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
N_CLOUD = 10_007


def apply(pts, t, q):
    """(n, 3) float64: apply(q, t) to the rows of pts (any float dtype, x y z first)."""
    v = np.asarray(pts, np.float64)[:, :3]
    u = np.asarray(q, np.float64)[:3]
    w = float(q[3])
    uv = np.cross(u, v)
    return v + 2.0 * w * uv + 2.0 * np.cross(u, uv) + np.asarray(t, np.float64)


def bound(pts, t):
    """(n, 3) float64: the tolerance of a float result against apply(), unit q."""
    v = np.abs(np.asarray(pts, np.float64)[:, :3]).sum(axis=1, keepdims=True)
    return 16.0 * U * (v + np.abs(np.asarray(t, np.float64))[None, :])


def units(got, pts, t, q):
    """max |got - apply()| in units of bound(): <= 1 passes."""
    err = np.abs(np.asarray(got, np.float64)[:, :3] - apply(pts, t, q))
    return float((err / bound(pts, t)).max())


def quat_rpy(roll_deg, pitch_deg, yaw_deg):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll) (tf2's setRPY)."""
    r, p, y = (math.radians(a) / 2.0 for a in (roll_deg, pitch_deg, yaw_deg))
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), \
        math.sin(y)
    return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
            cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)


def _axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / math.sqrt(float(a @ a))
    h = math.radians(deg) / 2.0
    return tuple(float(c) * math.sin(h) for c in a) + (math.cos(h),)


def scaled(q, s):
    return tuple(s * c for c in q)


TILT = quat_rpy(5.0, -8.0, 20.0)
TILT_YAW_ONLY = quat_rpy(0.0, 0.0, 20.0)   # the yaw part of TILT alone
QUATS = {
    "tilt": TILT,                                   # all four components non-zero
    "neg_w": scaled(TILT, -1.0),                    # the same rotation, w < 0
    "near_pi": _axis_angle((1.0, 2.0, 3.0), 179.9),
    "non_unit_small": scaled(TILT, 0.6),
    "non_unit_big": scaled(TILT, 1.7),
    "zero": (0.0, 0.0, 0.0, 0.0),
    "gimbal": (0.0, 1.0, 0.0, 1.0),                 # m[2][0] == -1 exactly in double
}
UNIT = ("tilt", "neg_w", "near_pi")
# translations no float holds exactly (a different one per use: see translation())
T_TILT = (12.3, -7.1, 1.9)


def translation(i):
    """The i-th translation: thirds, sevenths and elevenths, none a float."""
    return (12.3 + i / 3.0, -7.1 - i / 7.0, 1.9 + i / 11.0)


def colour_word(rgb):
    """PointXYZRGB's rgba word of (r, g, b): b | g << 8 | r << 16 | 255 << 24."""
    r, g, b = (int(c) for c in rgb)
    return np.uint32(b | (g << 8) | (r << 16) | (255 << 24))


def cloud(n=N_CLOUD, seed=0):
    """(n, 4) float32: x, y, z uniform in [-50, 50]^3, an intensity the transform ignores."""
    rng = np.random.default_rng(1000 + seed)
    c = np.empty((n, 4), np.float32)
    c[:, :3] = rng.uniform(-50.0, 50.0, (n, 3))
    c[:, 3] = rng.uniform(0.0, 255.0, n)
    return c


# ---- make_rigid + xform_pt restated in float32 numpy, and four wrong versions of it ------------
MUTANTS = ("twx_sign", "m12_m21_swapped", "fused_third", "assoc")
F32 = np.float32


def matrix_f32(q, mutant=None):
    """make_rigid's nine entries (row-major), every step rounded to float32."""
    qx, qy, qz, qw = (F32(c) for c in q)
    tx, ty, tz = F32(2) * qx, F32(2) * qy, F32(2) * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    if mutant == "twx_sign":
        twx = -twx
    m = [[F32(1) - (tyy + tzz), txy - twz, txz + twy],
         [txy + twz, F32(1) - (txx + tzz), tyz - twx],
         [txz - twy, tyz + twx, F32(1) - (txx + tyy)]]
    if mutant == "m12_m21_swapped":
        m[1][2], m[2][1] = m[2][1], m[1][2]
    assert all(type(e) is F32 for row in m for e in row)
    return m


def xform_f32(pts, t, q, mutant=None):
    """(n, 3) float32: xform_pt's ((m0 x + m1 y) + m2 z) + t in float32 steps.  mutant: None or
    one of MUTANTS -- a flipped sign of twx, m12 and m21 swapped, the third product fused into
    its sum (one rounding), or a + (b + c) instead of (a + b) + c."""
    assert mutant is None or mutant in MUTANTS
    m = matrix_f32(q, mutant)
    p = np.ascontiguousarray(pts, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((p.shape[0], 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a, b = m[r][0] * x, m[r][1] * y
            if mutant == "fused_third":
                # the float product is exact in double: one rounding of (a + b) + m2 * z
                s = ((a + b).astype(np.float64) +
                     np.float64(m[r][2]) * z.astype(np.float64)).astype(F32)
            elif mutant == "assoc":
                s = a + (b + m[r][2] * z)
            else:
                s = (a + b) + m[r][2] * z
            out[:, r] = s + F32(t[r])
    assert out.dtype == F32
    return out


# ---- the carve's matched cloud (test_gpu_parity._matched_cloud's generator) ---------------------
def matched_cloud(seed=3):
    """A /matched_point_cloud stand-in: a noisy 0.05 m lattice (PointXYZRGB, 32 B), a raised
    block, a hole with a few points 0.8 m up (nearest-point fallbacks), NaNs."""
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(-2.0, 9.0, 0.05), np.arange(-3.0, 6.0, 0.05)
    X, Y = np.meshgrid(xs, ys)
    P = np.stack([X.ravel(), Y.ravel(), rng.normal(0, 0.01, X.size)], 1)
    hole = np.hypot(P[:, 0] - 5.0, P[:, 1] - 0.0) < 0.8
    P = P[~hole]
    block = np.stack(np.meshgrid(np.arange(4.0, 4.6, 0.05), np.arange(1.0, 1.6, 0.05),
                                 np.array([0.3, 1.5])), -1).reshape(-1, 3)
    lifted = np.array([[5.0, 0.0, 0.8], [5.1, 0.2, 0.8], [4.8, -0.3, 0.85]])
    P = np.concatenate([P, block, lifted])
    c = np.zeros((P.shape[0], 8), np.float32)
    c[:, :3] = P
    c[:, 4] = np.frombuffer(np.full(P.shape[0], 0xFF00FF00, np.uint32).tobytes(), np.float32)
    c[rng.integers(0, P.shape[0], 20), 0] = np.nan
    return c


CARVE_T = (0.3, -0.2, 0.1)
CARVE_KW = dict(l_shape_enabled=0)   # the rectangle mode: carve_cases.geometry() restates it
_CARVE = {}


def carve_cloud():
    if "cloud" not in _CARVE:
        _CARVE["cloud"] = matched_cloud()
        _CARVE["cloud"].flags.writeable = False
    return _CARVE["cloud"]


def carve_reference(oracle, q):
    """oracle.excavate(carve_cloud(), CARVE_T, q, CARVE_KW), computed once per process and q:
    (keep, surf, area, pose), read-only."""
    key = tuple(float(c) for c in q)
    if key not in _CARVE:
        _CARVE[key] = oracle.excavate(carve_cloud(), CARVE_T, key, oracle.exc_params(**CARVE_KW))
        for a in _CARVE[key]:
            a.flags.writeable = False
    return _CARVE[key]


# ---- the drivable grid's cloud ------------------------------------------------------------------
DRIVE_KW = dict(grid_resolution=0.5, map_width=40.0, map_height=30.0, min_points_per_cell=2)
DRIVE_ROBOT, DRIVE_START = (1.0, -0.5), (2.0, 1.0)


def drive_cloud(n=20_000):
    """(n, 4) float32 over 44 m x 34 m: a smooth surface of z within +-1.5 m and 1 cm noise, so
    cells fall on both sides of the gradient limit; a few NaN rows."""
    rng = np.random.default_rng(77)
    c = np.zeros((n, 4), np.float32)
    x, y = rng.uniform(-22.0, 22.0, n), rng.uniform(-17.0, 17.0, n)
    c[:, 0], c[:, 1] = x, y
    c[:, 2] = 1.49 * np.sin(x / 3.0) * np.cos(y / 4.0) + rng.normal(0.0, 0.01, n)
    c[rng.integers(0, n, 10), 1] = np.nan
    return c


def drive_oracle(oracle, cloud, t, q):
    kw = DRIVE_KW
    return oracle.drivable_area(cloud, t, q, DRIVE_ROBOT, DRIVE_START, kw["grid_resolution"],
                                kw["map_width"], kw["map_height"], 0.3,
                                kw["min_points_per_cell"], 3.0)
