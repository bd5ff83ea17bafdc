"""NumPy restatement of pcp_place_coverage's definition (include/pcp_abi.h): a helper of
tests/test_cover_ref.py, test_place_coverage.py and test_cover_cli.py, not a conftest.

seen(p) comes from the scan's restatement on the oracle's first hits (scan_ref.resolve, or
mount_ref.resolve for the mounted twin), never from the device: per pose the sorted array of the
input indices its blocked rays resolved to.  The greedy itself works on those index arrays and on
one boolean per terrain point -- no 64-bit mask anywhere, so no pose count is special.

`mutant` turns the restatement into one of six wrong implementations; tests/test_cover_ref.py
checks that the case grid tells every one of them from the definition."""
import numpy as np
import scan_ref

OWNER_NONE = -2
MUTANTS = ("last_max", "sep_le", "roi_ignored", "fixed_alive", "need_static", "alias64")


def seen_sets(res, P):
    """scan_ref.resolve's / mount_ref.resolve's dict -> [P] sorted unique hit indices."""
    pp = np.asarray(res["pose"])
    hit = np.asarray(res["returns"]["point"]).astype(np.int64)
    return [np.unique(hit[pp == p]) for p in range(P)]


def level_seen(oracle, cloud, poses5, fan):
    """seen(p) of level poses: the oracle's march, scan_ref's resolve, at most 64 poses at a time
    (scan_ref.resolve also builds the scan's 64-bit mask)."""
    poses = np.ascontiguousarray(poses5, np.float64).reshape(-1, 5)
    T = oracle.Cloud(cloud)
    out = []
    for lo in range(0, poses.shape[0], 64):
        part = poses[lo:lo + 64]
        _, _, fh = oracle.raycast_fan(T, part, fan.n_az, fan.n_el, fan.el_min, fan.el_max,
                                      fan.max_distance)
        out += seen_sets(scan_ref.resolve(oracle, cloud, part, fan, fh), part.shape[0])
    return out


def greedy(seen, xy, N, k_max, sep=0.0, fixed=(), roi=None, mutant=None):
    """The definition, step by step -> dict of every output plus `tie_rounds` (rounds whose
    maximum two alive poses share) and `stopped` (None, "dead" or "gain")."""
    n = len(seen)
    assert mutant is None or mutant in MUTANTS
    if mutant == "alias64":   # pose p + 64 lands on p's bits
        seen = [np.unique(np.concatenate([seen[q] for q in range(p % 64, n, 64)]))
                if p < 64 else np.zeros(0, np.int64) for p in range(n)]
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    in_roi = np.ones(N, bool) if roi is None else np.asarray(roi).reshape(-1) != 0
    assert in_roi.shape[0] == N
    need = in_roi.copy() if mutant != "roi_ignored" else np.ones(N, bool)
    owner = np.full(N, OWNER_NONE, np.int32)
    sep2 = sep * sep if sep > 0 else 0.0

    def close(b):
        dx = xy[:, 0] - xy[b, 0]
        dy = xy[:, 1] - xy[b, 1]
        d2 = dx * dx + dy * dy
        return d2 <= sep2 if mutant == "sep_le" else d2 < sep2

    def commit(b, who):
        idx = seen[b][need[seen[b]]]
        owner[idx] = who
        if mutant != "need_static":
            need[idx] = False
        return idx.size

    alive = np.ones(n, bool)
    base = 0
    for i, f in enumerate(fixed):
        base += commit(f, i)
        if mutant == "fixed_alive":   # step 1's alive rule skipped: every pose starts alive
            continue
        alive[f] = False
        if sep2 > 0:
            alive &= ~close(f)
    sel, gain, cov, rows = [], [], [], []
    ties, stopped = 0, None
    covered = base
    for r in range(k_max):
        if not alive.any():
            stopped = "dead"
            break
        g = np.full(n, -1, np.int64)
        for p in np.nonzero(alive)[0]:
            g[p] = np.count_nonzero(need[seen[p]])
        top = int(g.max())
        at = np.nonzero(g == top)[0]
        b = int(at[-1] if mutant == "last_max" else at[0])
        if top <= 0:
            stopped = "gain"
            break
        ties += at.size > 1
        rows.append(g)
        sel.append(b)
        gain.append(top)
        covered += top
        cov.append(covered)
        commit(b, len(fixed) + r)
        alive[b] = False
        if sep2 > 0:
            alive &= ~close(b)
    if mutant == "roi_ignored":
        in_roi = np.ones(N, bool)
    return {"selected": np.array(sel, np.int64), "gain": np.array(gain, np.uint64),
            "covered_after": np.array(cov, np.uint64), "n_selected": len(sel), "n_points": N,
            "roi_points": int(np.count_nonzero(in_roi)), "base_covered": base,
            "seen_points": np.array([s.size for s in seen], np.uint32),
            "round_gains": np.array(rows, np.int64).reshape(len(rows), n),
            "point_owner": owner, "tie_rounds": int(ties), "stopped": stopped}


def assert_cover_equal(got, ref):
    """Every output of the call against the restatement's."""
    for k in ("n_selected", "n_points", "roi_points", "base_covered"):
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    for k in ("selected", "gain", "covered_after", "seen_points"):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64),
                                      np.asarray(ref[k]).astype(np.int64), err_msg=k)
    if got.get("round_gains") is not None:
        np.testing.assert_array_equal(got["round_gains"], ref["round_gains"])
    if got.get("point_owner") is not None:
        np.testing.assert_array_equal(got["point_owner"], ref["point_owner"])


# ---- the common instance (computed once per process, never modified) ----------------------------
SEP = 2.5
TIE_ROW = 35


def instance_poses():
    """71 rows: the six clutter poses, a lattice of 64 whose spacing 1.25 m is exact in binary (at
    a separation of 2.5 m the test dx^2 + dy^2 < sep^2 meets equality), and a copy of row 35."""
    ax = -4.375 + 1.25 * np.arange(8)
    gx, gy = np.meshgrid(ax, ax)
    j = np.arange(64)
    lat = np.column_stack([gx.ravel(), gy.ravel(), np.full(64, 0.5), np.zeros(64), 0.09375 * j])
    poses = np.concatenate([scan_ref.CLUTTER_POSES, lat])
    return np.ascontiguousarray(np.concatenate([poses, poses[TIE_ROW:TIE_ROW + 1]]))


def rois(cloud):
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    return {"all": None, "xpos": (x > 0).astype(np.uint8),
            "box": ((np.abs(x) < 1.5) & (np.abs(y) < 1.5) & (z > -0.9)).astype(np.uint8)}


# (roi, separation, fixed, k_max)
GRID = [("all", 0.0, (), 16), ("all", SEP, (), 16), ("box", 0.0, (), 16), ("xpos", SEP, (), 16),
        ("box", SEP, (), 16), ("all", 0.0, (10, 40), 4), ("all", SEP, (10, 40), 4)]


def instance(oracle):
    """-> dict: cloud, poses [71, 5], fan (100 x 37, 15 m), seen [71], rois, N."""
    from pointcloud_processor_amd import _abi

    def build():
        cloud = scan_ref.clutter_cloud()
        poses = instance_poses()
        fan = _abi.fan_params(n_az=100, n_el=37, max_distance=15.0)
        seen = level_seen(oracle, cloud, poses, fan)
        return {"cloud": cloud, "poses": poses, "fan": fan, "seen": seen, "rois": rois(cloud),
                "N": cloud.shape[0]}

    return scan_ref.cached(("cover", "instance"), build)


def grid_case(oracle, i, mutant=None):
    """The restatement's outputs of GRID[i] (cached)."""
    def build():
        inst = instance(oracle)
        roi, sep, fixed, k = GRID[i]
        return greedy(inst["seen"], inst["poses"][:, :2], inst["N"], k, sep, fixed,
                      inst["rois"][roi], mutant)

    return scan_ref.cached(("cover", "case", i, mutant), build)
