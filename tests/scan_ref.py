"""NumPy restatement of pcp_simulate_scan's definition (include/pcp_abi.h): a helper of
tests/test_scan_abi.py and tests/test_simulate_scan.py, not a conftest.

The first hits come from the oracle's march (pyoracle.raycast_fan), never from the device.  For a
blocked ray the query point is float32(p + d * s_k) in float64 arithmetic (the direction tables
are the oracle's, the yaw's cosine and sine libm's, as the host pose table), the candidates are
the points with FLANN's float32 accumulator ((0 + d0 d0) + d1 d1) + d2 d2 < float32(r r), the hit
point is the candidate of smallest accumulator, ties to the lowest input index, and the range is
float32(sqrt((ex ex + ey ey) + ez ez)) in float64.  NumPy's elementwise arithmetic rounds every
operation (no contraction)."""
import math

import numpy as np

RAY_RADIUS = 0.08 * 0.7
R2 = np.float32(RAY_RADIUS * RAY_RADIUS)

RETURN_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32),
                         ("range", np.float32), ("ray", np.uint32), ("point", np.uint32)])


def step_table(end):
    s = []
    x = 0.5
    while x < end:
        s.append(x)
        x = x + 0.3
    return np.array(s, np.float64)


def queries(oracle, poses5, fan, first_hit):
    """The blocked rays, pose-major in ascending ray id -> (pose [M], ray [M], k [M], q float32
    [M, 3], qprev float32 [M, 3]: the query point of sample k - 1, meaningful where k > 0)."""
    poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 5)
    ca, sa, ce, se = oracle.fan_tables(fan.n_az, fan.n_el, fan.el_min, fan.el_max)
    steps = step_table(fan.max_distance - 0.08)
    fh = np.asarray(first_hit).reshape(poses.shape[0], -1)
    pp, rr = np.nonzero(fh >= 0)           # row-major: pose, then ray
    k = fh[pp, rr].astype(np.int64)
    j, i = rr // fan.n_az, rr % fan.n_az
    lx, ly, lz = ce[j] * ca[i], ce[j] * sa[i], se[j]
    cy = np.array([math.cos(y) for y in poses[:, 4]])[pp]
    sy = np.array([math.sin(y) for y in poses[:, 4]])[pp]
    dx = cy * lx - sy * ly
    dy = sy * lx + cy * ly
    dz = lz
    px, py, pz = poses[pp, 0], poses[pp, 1], poses[pp, 2]

    def at(s):
        return np.stack([(px + dx * s).astype(np.float32), (py + dy * s).astype(np.float32),
                         (pz + dz * s).astype(np.float32)], axis=1)

    return pp, rr.astype(np.uint32), k, at(steps[k]), at(steps[np.maximum(k - 1, 0)])


def candidates(cloud, q):
    """Every (query, point) pair with acc < R2 -> (qid, pid, acc float32), sorted by query, then
    acc, then point index.  A hash grid of cell 0.06 m > r finds a superset (the 27 cells around
    the query's), the float32 accumulator decides."""
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    fin = np.isfinite(xyz).all(axis=1)
    idx = np.nonzero(fin)[0]
    pts = xyz[idx]
    if pts.shape[0] == 0 or q.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, np.float32)
    h = 0.06
    lo = np.minimum(pts.min(axis=0).astype(np.float64), q.min(axis=0).astype(np.float64)) - 2 * h
    hi = np.maximum(pts.max(axis=0).astype(np.float64), q.max(axis=0).astype(np.float64)) + 2 * h
    dims = (np.floor((hi - lo) / h).astype(np.int64) + 2)

    def key(c):
        return (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]

    pc = np.floor((pts.astype(np.float64) - lo) / h).astype(np.int64)
    pk = key(pc)
    order = np.argsort(pk, kind="stable")
    pk_sorted = pk[order]
    qc = np.floor((q.astype(np.float64) - lo) / h).astype(np.int64)
    qid_l, pid_l = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                kk = key(qc + np.array([ox, oy, oz]))
                a = np.searchsorted(pk_sorted, kk, "left")
                b = np.searchsorted(pk_sorted, kk, "right")
                cnt = b - a
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                qi = np.repeat(np.arange(q.shape[0]), cnt)
                first = np.repeat(a - (np.cumsum(cnt) - cnt), cnt)
                qid_l.append(qi)
                pid_l.append(order[np.arange(tot) + first])
    if not qid_l:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, np.float32)
    qid = np.concatenate(qid_l)
    loc = np.concatenate(pid_l)
    d = q[qid] - pts[loc]                       # float32
    acc = np.float32(0.0) + d[:, 0] * d[:, 0]
    acc = acc + d[:, 1] * d[:, 1]
    acc = acc + d[:, 2] * d[:, 2]
    assert acc.dtype == np.float32
    keep = acc < R2
    qid, pid, acc = qid[keep], idx[loc[keep]], acc[keep]
    o = np.lexsort((pid, acc, qid))
    return qid[o], pid[o], acc[o]


def resolve(oracle, cloud, poses5, fan, first_hit):
    """Every output of pcp_simulate_scan for the oracle's first hits -> dict (returns, offsets,
    hit_point, range, point_mask, seen_points, n_seen_any, n_points) plus the intermediate
    q / cand_* / ties for the preconditions."""
    poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 5)
    P = poses.shape[0]
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    N = xyz.shape[0]
    pp, rr, k, q, qprev = queries(oracle, poses, fan, first_hit)
    M = pp.shape[0]
    qid, pid, acc = candidates(xyz, q)
    # the first pair of every query is its (acc, index) minimum
    first = np.ones(qid.shape[0], bool)
    first[1:] = qid[1:] != qid[:-1]
    has = np.zeros(M, bool)
    has[qid[first]] = True
    assert has.all(), "a blocked ray without a candidate point"
    hit = np.zeros(M, np.int64)
    hit[qid[first]] = pid[first]
    # ties: the runner-up has the same accumulator
    second = np.zeros(qid.shape[0], bool)
    second[1:] = first[:-1] & ~first[1:]
    ties = int(np.count_nonzero(second[1:] & (acc[1:] == acc[:-1])))
    hp = xyz[hit]
    e = hp.astype(np.float64) - poses[pp, :3]
    rng = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(np.float32)
    ret = np.zeros(M, RETURN_DTYPE)
    ret["x"], ret["y"], ret["z"] = hp[:, 0], hp[:, 1], hp[:, 2]
    ret["range"] = rng
    ret["ray"] = rr
    ret["point"] = hit
    offsets = np.zeros(P + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(pp, minlength=P))
    rays = fan.n_az * fan.n_el
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
    shape = (P, fan.n_el, fan.n_az)
    return {"returns": ret, "offsets": offsets, "hit_point": hit_point.reshape(shape),
            "range": range_img.reshape(shape), "point_mask": mask, "seen_points": seen,
            "n_seen_any": int(np.count_nonzero(mask)), "n_points": N,
            "pose": pp, "k": k, "q": q, "qprev": qprev, "cand_q": qid, "cand_p": pid,
            "cand_acc": acc, "ties": ties}


def assert_scan_equal(got, ref, dense=True, mask=True):
    """Bit for bit: records (as bytes), offsets, dense arrays, masks and counts."""
    assert got["n_points"] == ref["n_points"]
    np.testing.assert_array_equal(np.asarray(got["offsets"], np.uint64), ref["offsets"])
    assert got["returns"].dtype.itemsize == 24
    assert got["returns"].shape == ref["returns"].shape
    for f in ("ray", "point"):
        np.testing.assert_array_equal(got["returns"][f], ref["returns"][f], err_msg=f)
    for f in ("x", "y", "z", "range"):
        np.testing.assert_array_equal(got["returns"][f].view(np.uint32),
                                      ref["returns"][f].view(np.uint32), err_msg=f)
    assert got["returns"].tobytes() == ref["returns"].astype(got["returns"].dtype).tobytes()
    if dense:
        np.testing.assert_array_equal(got["hit_point"], ref["hit_point"])
        np.testing.assert_array_equal(got["range"].view(np.uint32), ref["range"].view(np.uint32))
    if mask:
        np.testing.assert_array_equal(got["point_mask"], ref["point_mask"])
        np.testing.assert_array_equal(got["seen_points"], ref["seen_points"])
        assert got["n_seen_any"] == ref["n_seen_any"]


# ---- the shared fixtures: computed once per process, never modified -----------------------------
_CACHE = {}

CLUTTER_POSES = np.array([[0.0, 0.0, 0.2, 0.0, 0.3], [1.5, -1.5, 1.5, 0.0, -2.0],
                          [-4.0, 2.0, 2.5, 0.0, 1.0], [0.5, 4.0, -1.5, 0.0, 0.0],
                          [40.0, 40.0, 0.0, 0.0, 0.0], [2.9, 0.0, 0.5, 0.0, 3.1]])


def clutter_cloud():
    """tests/test_gpu_parity.py's volumetric cloud plus its first 2,000 rows appended as exact
    duplicates (equal accumulators: the ties of the lowest-index rule)."""
    if "cloud" not in _CACHE:
        from test_gpu_parity import _clutter_cloud

        c = _clutter_cloud()
        c = np.ascontiguousarray(np.concatenate([c, c[:2000]]))
        c.setflags(write=False)
        _CACHE["cloud"] = c
    return _CACHE["cloud"]


def cached(name, build):
    if name not in _CACHE:
        _CACHE[name] = build()
    return _CACHE[name]


def clutter_case(oracle, n_az, n_el, max_distance=15.0):
    """(cloud, poses, fan, oracle first hits + blocked, the restatement's outputs) of the clutter
    cloud with that test's six poses."""
    from pointcloud_processor_amd import _abi

    def build():
        cloud = clutter_cloud()
        fan = _abi.fan_params(n_az=n_az, n_el=n_el, max_distance=max_distance)
        T = oracle.Cloud(cloud)
        blocked, _, fh = oracle.raycast_fan(T, CLUTTER_POSES, n_az, n_el, fan.el_min, fan.el_max,
                                            fan.max_distance)
        ref = resolve(oracle, cloud, CLUTTER_POSES, fan, fh)
        return cloud, CLUTTER_POSES, fan, fh, blocked, ref

    return cached(("clutter", n_az, n_el, max_distance), build)
