"""NumPy restatement of pcp_place_coverage_aimed's definition (include/pcp_abi.h): a helper of
tests/test_cover_aim_ref.py, test_place_coverage_aimed.py and test_cover_aim_cli.py, not a
conftest.

The rays come from the scan's restatement on the oracle's first hits (scan_ref.resolve, or
mount_ref.resolve for the mounted twin), never from the device: per pose the returns' `ray` gives
(j, i) = divmod(ray, n_az), and `point` the terrain point the ray resolved to.  A window is a
boolean over those rays; seen(p, a) is the set of points of the rays inside it.  Everything works on
index arrays and booleans -- no 64-bit mask anywhere, so no aim count is special.

`mutant` turns the restatement into one of eight wrong implementations; tests/test_cover_aim_ref.py
checks that the case grid tells every one of them from the definition."""
import cover_ref
import numpy as np
import scan_ref

OWNER_NONE = cover_ref.OWNER_NONE
MUTANTS = ("rays_not_points", "no_wrap", "ring_end_inclusive", "pose_stays", "aim_major",
           "last_max", "fixed_full_fan", "mask_lowest_ray")


def ray_hits(res, P):
    """scan_ref.resolve's / mount_ref.resolve's dict -> [P] of (ray [m], point [m]) in ascending
    ray order."""
    pp = np.asarray(res["pose"])
    ray = np.asarray(res["returns"]["ray"]).astype(np.int64)
    pt = np.asarray(res["returns"]["point"]).astype(np.int64)
    out = []
    for p in range(P):
        at = pp == p
        o = np.argsort(ray[at], kind="stable")
        out.append((ray[at][o], pt[at][o]))
    return out


def level_hits(oracle, cloud, poses5, fan):
    """ray_hits of level poses: the oracle's march, scan_ref's resolve, at most 64 poses at a
    time."""
    poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 5)
    T = oracle.Cloud(cloud)
    out = []
    for lo in range(0, poses.shape[0], 64):
        part = poses[lo:lo + 64]
        _, _, fh = oracle.raycast_fan(T, part, fan.n_az, fan.n_el, fan.el_min, fan.el_max,
                                      fan.max_distance)
        out += ray_hits(scan_ref.resolve(oracle, cloud, part, fan, fh), part.shape[0])
    return out


def in_window(ray, n_az, az0, el0, w_az, w_el, mutant=None):
    """Window(a) as a boolean over ray ids."""
    j, i = np.divmod(ray, n_az)
    if mutant == "no_wrap":
        col = (i >= az0) & (i < az0 + w_az)
    else:
        col = ((i - az0) % n_az) < w_az
    if mutant == "ring_end_inclusive":
        ring = (j >= el0) & (j <= el0 + w_el)
    else:
        ring = (j >= el0) & (j < el0 + w_el)
    return col & ring


def membership(hits, n_az, w_az, w_el, aims, mutant=None):
    """-> (pts [P] sorted unique points of each pose, cnt [P] int64 [m, A]: the rays of Window(a)
    that resolved to the point).  The definition takes cnt > 0."""
    aims = np.asarray(aims, np.int64).reshape(-1, 2)
    A = aims.shape[0]
    pts, cnt = [], []
    for ray, pt in hits:
        u, first, inv = np.unique(pt, return_index=True, return_inverse=True)
        c = np.zeros((u.size, A), np.int64)
        for a in range(A):
            if mutant == "mask_lowest_ray":   # the point's lowest ray alone says which aims hold it
                c[:, a] = in_window(ray[first], n_az, aims[a, 0], aims[a, 1], w_az, w_el)
            else:
                w = in_window(ray, n_az, aims[a, 0], aims[a, 1], w_az, w_el, mutant)
                c[:, a] = np.bincount(inv[w], minlength=u.size)
        pts.append(u)
        cnt.append(c)
    return pts, cnt


def greedy(hits, xy, N, n_az, w_az, w_el, aims, k_max, sep=0.0, fixed=(), roi=None, mutant=None):
    """The definition, step by step -> dict of every output plus `tie_rounds` (rounds whose
    maximum two alive (pose, aim) rows share), `stopped` (None, "dead" or "gain")."""
    assert mutant is None or mutant in MUTANTS
    n = len(hits)
    aims = np.asarray(aims, np.int64).reshape(-1, 2)
    A = aims.shape[0]
    pts, cnt = membership(hits, n_az, w_az, w_el, aims, mutant)
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    in_roi = np.ones(N, bool) if roi is None else np.asarray(roi).reshape(-1) != 0
    assert in_roi.shape[0] == N
    need = in_roi.copy()
    owner = np.full(N, OWNER_NONE, np.int32)
    sep2 = sep * sep if sep > 0 else 0.0

    def close(b):
        dx = xy[:, 0] - xy[b, 0]
        dy = xy[:, 1] - xy[b, 1]
        return dx * dx + dy * dy < sep2

    def gains(p, nd):
        """g[p][.] against the boolean nd over the N points"""
        live = nd[pts[p]]
        if mutant == "rays_not_points":
            return cnt[p][live].sum(axis=0)
        return np.count_nonzero(cnt[p][live] > 0, axis=0)

    def commit(b, ab, who, full=False):
        inside = np.ones(pts[b].size, bool) if full else cnt[b][:, ab] > 0
        idx = pts[b][inside & need[pts[b]]]
        owner[idx] = who
        need[idx] = False
        return idx.size

    alive = np.ones((n, A), bool)   # (rows of a pose leave together, but for `pose_stays`)
    base = 0
    for i, (f, fa) in enumerate(fixed):
        base += commit(f, fa, i, full=mutant == "fixed_full_fan")
        alive[f] = False
        if sep2 > 0:
            alive[close(f)] = False
    sel, sel_aim, gain, cov, rows = [], [], [], [], []
    ties, stopped = 0, None
    covered = base
    for r in range(k_max):
        if not alive.any():
            stopped = "dead"
            break
        g = np.full((n, A), -1, np.int64)
        for p in np.nonzero(alive.any(axis=1))[0]:
            g[p] = np.where(alive[p], gains(p, need), -1)
        top = int(g.max())
        if mutant == "aim_major":
            at = np.nonzero(g.T.reshape(-1) == top)[0]
            ab, b = divmod(int(at[0]), n)
        else:
            at = np.nonzero(g.reshape(-1) == top)[0]
            b, ab = divmod(int(at[-1] if mutant == "last_max" else at[0]), A)
        if top <= 0:
            stopped = "gain"
            break
        ties += at.size > 1
        rows.append(g)
        sel.append(b)
        sel_aim.append(ab)
        gain.append(top)
        covered += top
        cov.append(covered)
        commit(b, ab, len(fixed) + r)
        if mutant == "pose_stays":
            alive[b, ab] = False
        else:
            alive[b] = False
        if sep2 > 0:
            alive[close(b)] = False
    everything = np.ones(N, bool)
    return {"selected": np.array(sel, np.int64), "selected_aim": np.array(sel_aim, np.int32),
            "gain": np.array(gain, np.uint64), "covered_after": np.array(cov, np.uint64),
            "n_selected": len(sel), "n_points": N,
            "roi_points": int(np.count_nonzero(in_roi)), "base_covered": base,
            "seen_points": np.array([u.size for u in pts], np.uint32),
            "aim_points": np.array([gains(p, everything) for p in range(n)],
                                   np.uint32).reshape(n, A),
            "round_gains": np.array(rows, np.int64).reshape(len(rows), n, A),
            "point_owner": owner, "tie_rounds": int(ties), "stopped": stopped}


KEYS_SCALAR = ("n_selected", "n_points", "roi_points", "base_covered")
KEYS_ARRAY = ("selected", "selected_aim", "gain", "covered_after", "seen_points")
KEYS_TABLE = ("round_gains", "aim_points", "point_owner")


def assert_aimed_equal(got, ref):
    """Every output of the call against the restatement's."""
    for k in KEYS_SCALAR:
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    for k in KEYS_ARRAY:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64),
                                      np.asarray(ref[k]).astype(np.int64), err_msg=k)
    for k in KEYS_TABLE:
        if got.get(k) is not None:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


def same_answer(a, b):
    """Two restatement dicts agree on every output the device call has."""
    return (all(int(a[k]) == int(b[k]) for k in KEYS_SCALAR) and
            all(np.array_equal(a[k], b[k]) for k in KEYS_ARRAY + KEYS_TABLE))


# ---- the common instance: cover_ref's (71 poses, 100 x 37 fan, N % 64 = 44) with its rays ---------
SEP = cover_ref.SEP
N_AZ, N_EL = 100, 37


def _sectors(count, el0s):
    """`count` sectors around the circle (nearest column) times the bands el0s, sector-major."""
    return [(int(np.floor(N_AZ * k / count + 0.5)) % N_AZ, e) for k in range(count) for e in el0s]


# name -> (w_az, w_el, aims): 12 sectors x 2 bands = 24 aims of 90 deg x 20 rings, the bands at
# el0 = 0 and el0 = n_el - w_el, the sectors from column 83 on wrapping; 64 aims = 8 sectors x 4
# bands of 13 columns x 10 rings listed twice (aim a + 32 is aim a: every maximum ties, the lower
# index wins); the one full window, which is pcp_place_coverage
TABLES = {
    "s24": (25, 20, _sectors(12, (0, N_EL - 20))),
    "a64": (13, 10, _sectors(8, (0, 9, 18, N_EL - 10)) * 2),
    "full": (N_AZ, N_EL, [(0, 0)]),
}
assert len(TABLES["s24"][2]) == 24 and len(TABLES["a64"][2]) == 64

# (table, roi, separation, fixed (pose, aim) pairs, k_max)
GRID = [("s24", "all", 0.0, (), 16), ("s24", "all", SEP, (), 16), ("a64", "box", 0.0, (), 16),
        ("a64", "xpos", SEP, (), 16), ("s24", "all", 0.0, ((10, 3), (40, 17)), 4),
        ("a64", "all", SEP, ((10, 5), (40, 40)), 4), ("full", "box", 0.0, (), 16),
        ("full", "xpos", SEP, ((10, 0), (40, 0)), 4), ("s24", "top", 0.0, (), 16)]


def instance(oracle):
    """cover_ref.instance's dict plus hits [71]: every pose's (ray, point) arrays."""
    def build():
        inst = dict(cover_ref.instance(oracle))
        inst["hits"] = level_hits(oracle, inst["cloud"], inst["poses"], inst["fan"])
        # one more region: the points above the lattice's sensors, which the upper bands reach
        inst["rois"] = {**inst["rois"], "top": (inst["cloud"][:, 2] > 1.0).astype(np.uint8)}
        return inst

    return scan_ref.cached(("cover_aim", "instance"), build)


def grid_case(oracle, i, mutant=None):
    """The restatement's outputs of GRID[i] (cached)."""
    def build():
        inst = instance(oracle)
        table, roi, sep, fixed, k = GRID[i]
        w_az, w_el, aims = TABLES[table]
        return greedy(inst["hits"], inst["poses"][:, :2], inst["N"], N_AZ, w_az, w_el, aims, k,
                      sep, fixed, inst["rois"][roi], mutant)

    return scan_ref.cached(("cover_aim", "case", i, mutant), build)
