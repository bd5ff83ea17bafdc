"""NumPy restatement of pcp_raycast_fan_mounted / pcp_simulate_scan_mounted (include/pcp_abi.h):
a helper of tests/test_mount_ref.py, test_mount_abi.py and test_mount_gpu.py, not a conftest.

Nothing here comes from the device or from the oracle's march.  The direction of ray (i, j) is the
definition's: the local direction (ce_j ca_i, ce_j sa_i, se_j) -- libm's cos / sin through
math.cos / math.sin, of the uniform ring formula or of the beam table -- turned by roll, pitch and
yaw in elementwise float64 (NumPy rounds every product and sum on its own).  first_hits() marches
the whole step table of every ray: sample k is blocked iff some point has FLANN's float32
accumulator below float32(r r) at q = float32(p + d s_k), found through scan_ref.candidates' hash
grid.  resolve() turns those hits into every scan output the way scan_ref.resolve does."""
import math

import numpy as np
import scan_ref

KVIS = 0.08   # the march ends at max_distance - 0.08


def local_tables(fan, el_table=None):
    """ca, sa [n_az], ce, se [n_el] in float64 (the expressions of pcp_raycast_fan's tables)."""
    n_az, n_el = int(fan.n_az), int(fan.n_el)
    az = [2.0 * math.pi * float(i) / float(n_az) for i in range(n_az)]
    if el_table is None:
        el = [fan.el_min + (fan.el_max - fan.el_min) * (float(j) + 0.5) / float(n_el)
              for j in range(n_el)]
    else:
        el = [float(e) for e in np.asarray(el_table, np.float64).reshape(-1)]
        assert len(el) == n_el
    f = np.float64
    return (np.array([math.cos(a) for a in az], f), np.array([math.sin(a) for a in az], f),
            np.array([math.cos(e) for e in el], f), np.array([math.sin(e) for e in el], f))


def directions(poses6, fan, el_table=None):
    """-> float64 [P, n_el, n_az, 3]: the definition's (dx, dy, dz) of every ray."""
    poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
    ca, sa, ce, se = local_tables(fan, el_table)
    lx = (ce[:, None] * ca[None, :])[None]
    ly = (ce[:, None] * sa[None, :])[None]
    lz = np.broadcast_to(se[:, None], (se.size, ca.size))[None]

    def col(fn, c):
        return np.array([fn(v) for v in poses[:, c]], np.float64)[:, None, None]

    cr, sr = col(math.cos, 3), col(math.sin, 3)
    cp, sp = col(math.cos, 4), col(math.sin, 4)
    cy, sy = col(math.cos, 5), col(math.sin, 5)
    x1 = lx
    y1 = ly * cr - lz * sr
    z1 = ly * sr + lz * cr
    x2 = x1 * cp - z1 * sp
    y2 = y1
    z2 = x1 * sp + z1 * cp
    dx = cy * x2 - sy * y2
    dy = sy * x2 + cy * y2
    dz = z2
    return np.stack([dx, dy, dz], axis=-1)


def sample_points(poses6, d, s):
    """float32(p + d s) of rays d [..., 3] (leading axis: the pose) at depths s (broadcast)."""
    poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
    p = poses[:, :3].reshape((poses.shape[0],) + (1,) * (d.ndim - 2) + (3,))
    return (p + d * np.asarray(s, np.float64)[..., None]).astype(np.float32)


def first_hits(cloud, poses6, fan, el_table=None, chunk=4):
    """The whole march -> (first_hit int16 [P, n_el, n_az], blocked uint32 [P], units uint64 [P]).
    The step table is walked `chunk` samples at a time; a ray that is blocked leaves."""
    poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
    P = poses.shape[0]
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    fin = xyz[np.isfinite(xyz).all(axis=1)]
    steps = scan_ref.step_table(fan.max_distance - KVIS)
    K = steps.size
    d = directions(poses, fan, el_table).reshape(P, -1, 3)
    rays = d.shape[1]
    px = np.repeat(poses[:, :3], rays, axis=0)          # [P rays, 3]
    dd = d.reshape(-1, 3)
    fh = np.full(P * rays, -1, np.int64)
    if fin.shape[0]:
        # a sample further than 0.06 m > r outside the points' bounding box has no point within r
        lo = fin.min(axis=0).astype(np.float64) - 0.06
        hi = fin.max(axis=0).astype(np.float64) + 0.06
        alive = np.arange(P * rays)
        for k0 in range(0, K, chunk):
            if alive.size == 0:
                break
            ks = np.arange(k0, min(k0 + chunk, K))
            q = (px[alive, None, :] + dd[alive, None, :] * steps[ks][None, :, None]).astype(np.float32)
            inside = ((q >= lo) & (q <= hi)).all(axis=2)
            a_i, k_i = np.nonzero(inside)
            if a_i.size == 0:
                continue
            qid, _, _ = scan_ref.candidates(xyz, np.ascontiguousarray(q[a_i, k_i]))
            hit_q = np.unique(qid)
            first = np.full(alive.size, K, np.int64)
            np.minimum.at(first, a_i[hit_q], ks[k_i[hit_q]])
            got = first < K
            fh[alive[got]] = first[got]
            alive = alive[~got]
    fh = fh.reshape(P, rays)
    blocked = np.count_nonzero(fh >= 0, axis=1).astype(np.uint32)
    units = np.where(fh >= 0, fh + 1, K).sum(axis=1).astype(np.uint64)
    return fh.astype(np.int16).reshape(P, int(fan.n_el), int(fan.n_az)), blocked, units


def queries(poses6, fan, el_table, first_hit):
    """The blocked rays, pose-major in ascending ray id -> (pose, ray, k, q float32 [M, 3], qprev
    float32 [M, 3]: the query point of sample k - 1, meaningful where k > 0)."""
    poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
    P = poses.shape[0]
    steps = scan_ref.step_table(fan.max_distance - KVIS)
    fh = np.asarray(first_hit).reshape(P, -1)
    pp, rr = np.nonzero(fh >= 0)
    k = fh[pp, rr].astype(np.int64)
    d = directions(poses, fan, el_table).reshape(P, -1, 3)[pp, rr]
    p = poses[pp, :3]

    def at(s):
        return (p + d * s[:, None]).astype(np.float32)

    return pp, rr.astype(np.uint32), k, at(steps[k]), at(steps[np.maximum(k - 1, 0)])


def resolve(cloud, poses6, fan, el_table, first_hit):
    """Every output of pcp_simulate_scan_mounted for those first hits: scan_ref.resolve's dict."""
    poses = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
    P = poses.shape[0]
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    N = xyz.shape[0]
    pp, rr, k, q, qprev = queries(poses, fan, el_table, first_hit)
    M = pp.shape[0]
    qid, pid, acc = scan_ref.candidates(xyz, q)
    first = np.ones(qid.shape[0], bool)
    first[1:] = qid[1:] != qid[:-1]
    has = np.zeros(M, bool)
    has[qid[first]] = True
    assert has.all(), "a blocked ray without a candidate point"
    hit = np.zeros(M, np.int64)
    hit[qid[first]] = pid[first]
    hp = xyz[hit]
    e = hp.astype(np.float64) - poses[pp, :3]
    rng = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(np.float32)
    ret = np.zeros(M, scan_ref.RETURN_DTYPE)
    ret["x"], ret["y"], ret["z"] = hp[:, 0], hp[:, 1], hp[:, 2]
    ret["range"] = rng
    ret["ray"] = rr
    ret["point"] = hit
    offsets = np.zeros(P + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(pp, minlength=P))
    rays = int(fan.n_az) * int(fan.n_el)
    hit_point = np.full((P, rays), -1, np.int32)
    range_img = np.full((P, rays), -1.0, np.float32)
    hit_point[pp, rr] = hit
    range_img[pp, rr] = rng
    mask = np.zeros(N, np.uint64)
    seen = np.zeros(P, np.uint32)
    for p in range(P):
        u = np.unique(hit[pp == p])
        mask[u] |= np.uint64(1) << np.uint64(p)
        seen[p] = u.size
    shape = (P, int(fan.n_el), int(fan.n_az))
    return {"returns": ret, "offsets": offsets, "hit_point": hit_point.reshape(shape),
            "range": range_img.reshape(shape), "point_mask": mask, "seen_points": seen,
            "n_seen_any": int(np.count_nonzero(mask)), "n_points": N,
            "pose": pp, "k": k, "q": q, "qprev": qprev}


def mount_case(name, cloud, poses6, fan, el_table=None):
    """(first_hit, blocked, units, resolve's dict) of a case, computed once per process."""
    def build():
        fh, blocked, units = first_hits(cloud, poses6, fan, el_table)
        return fh, blocked, units, resolve(cloud, poses6, fan, el_table, fh)

    return scan_ref.cached(("mount",) + tuple(name), build)


# the six clutter poses (tests/scan_ref.py) with roll / pitch pairs: level, the zx120 Velodyne's
# pitch, a rolled and raised mount, one pitched so steeply that whole rings leave the clip box
CLUTTER_TILTS = [(0.0, 0.0), (0.0, -0.4363), (0.3, 0.2), (0.0, -1.5), (-0.2, -0.1245), (0.1, 0.6)]


def clutter_poses6():
    p5 = scan_ref.CLUTTER_POSES
    t = np.array(CLUTTER_TILTS)
    return np.ascontiguousarray(np.column_stack([p5[:, :3], t[:, 0], t[:, 1], p5[:, 4]]))
