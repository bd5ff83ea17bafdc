"""NumPy restatement of pcp_place_coverage_pair's definition (include/pcp_abi.h): a helper of
tests/test_cover_pair_ref.py, test_place_coverage_pair.py, test_cover_pair_host.py and
test_cover_pair_cli.py, not a conftest.

seen(p) is cover_ref's: the scan's restatement on the oracle's first hits, per pose the sorted
array of input indices -- nothing from the device.  The pairs' intersections are counted on a 0/1
matrix over the points of need0 that any pose reaches, as a float64 product (every count is far
below 2^53: exact).

`mutant` turns the restatement into one of six wrong implementations; tests/test_cover_pair_ref.py
checks that the case grid tells every one of them from the definition."""
import cover_ref
import numpy as np
import scan_ref

OWNER_NONE = cover_ref.OWNER_NONE
MUTANTS = ("last_max", "sep_le", "lower_triangle", "need_static", "no_intersection", "nsel_ge")


def _first_max(v, ok, last=False):
    """Index of the first (last: the mutant's) maximum of v over ok, -1 without one."""
    at = np.nonzero(ok)[0]
    if at.size == 0:
        return -1
    top = at[v[at] == v[at].max()]
    return int(top[-1] if last else top[0])


def pair(seen, xy, N, sep=0.0, fixed=(), roi=None, mutant=None):
    """The definition, step by step -> dict of every output of the call."""
    n = len(seen)
    assert mutant is None or mutant in MUTANTS
    last = mutant == "last_max"
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    in_roi = np.ones(N, bool) if roi is None else np.asarray(roi).reshape(-1) != 0
    assert in_roi.shape[0] == N
    need = in_roi.copy()
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
        need[idx] = False
        return idx.size

    # 1. the base; 2. admissibility
    adm = np.ones(n, bool)
    base = 0
    for i, f in enumerate(fixed):
        base += commit(f, i)
        adm[f] = False
        if sep2 > 0:
            adm &= ~close(f)
    need0 = in_roi.copy() if mutant == "need_static" else need.copy()
    # 3. singles
    M = [s[need0[s]] for s in seen]
    g = np.array([m.size for m in M], np.int64)
    single_gains = np.where(adm, g, -1)
    bs = _first_max(g, adm, last)
    single_gain = int(g[bs]) if bs >= 0 else 0
    # 4. pairs
    cols = np.unique(np.concatenate(M + [np.zeros(0, np.int64)]))
    B = np.zeros((n, cols.size), np.float64)
    for p, m in enumerate(M):
        B[p, np.searchsorted(cols, m)] = 1.0
    x = np.rint(B @ B.T).astype(np.int64)
    u = g[:, None] + g[None, :] - (0 if mutant == "no_intersection" else x)
    ok = adm[:, None] & adm[None, :]
    idx = np.arange(n)
    ok &= (idx[:, None] != idx[None, :]) if mutant == "lower_triangle" else (idx[:, None] < idx[None, :])
    if sep2 > 0:
        for a in range(n):
            ok[a] &= ~close(a)
    pair_gains = np.where(ok, u, -1)
    partner = np.full(n, -1, np.int64)
    partner_gain = np.full(n, -1, np.int64)
    for a in range(n):
        b = _first_max(u[a], ok[a], last)
        if b >= 0:
            partner[a], partner_gain[a] = b, u[a, b]
    ba = _first_max(partner_gain, partner >= 0, last)
    best_pair = (ba, int(partner[ba])) if ba >= 0 else (-1, -1)
    pair_gain = int(partner_gain[ba]) if ba >= 0 else 0
    # 5. the answer
    beats = pair_gain >= single_gain if mutant == "nsel_ge" else pair_gain > single_gain
    if ba >= 0 and beats:
        chosen = list(best_pair)
    elif bs >= 0 and single_gain > 0:
        chosen = [bs]
    else:
        chosen = []
    for r, p in enumerate(chosen):
        commit(p, len(fixed) + r)
    return {"n_selected": len(chosen), "best_pair": np.array(best_pair, np.int64),
            "pair_gain": pair_gain, "best_single": bs, "single_gain": single_gain,
            "single_gains": single_gains.astype(np.int64), "pair_gains": pair_gains.astype(np.int64),
            "partner": partner, "partner_gain": partner_gain, "n_points": N,
            "roi_points": int(np.count_nonzero(in_roi)), "base_covered": base,
            "seen_points": np.array([s.size for s in seen], np.uint32), "point_owner": owner}


def assert_pair_equal(got, ref):
    """Every output of the call against the restatement's."""
    for k in ("n_selected", "pair_gain", "best_single", "single_gain", "n_points", "roi_points",
              "base_covered"):
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    for k in ("best_pair", "single_gains", "partner", "partner_gain", "seen_points"):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64),
                                      np.asarray(ref[k]).astype(np.int64), err_msg=k)
    if got.get("pair_gains") is not None:
        np.testing.assert_array_equal(got["pair_gains"], ref["pair_gains"])
    if got.get("point_owner") is not None:
        np.testing.assert_array_equal(got["point_owner"], ref["point_owner"])


# ---- the case grid on cover_ref's 71-pose instance ----------------------------------------------
# two regions on which greedy's two rounds are not the best pair (float32 coordinates, bounds
# included): x0, x1, y0, y1
BOXES = {"box_a": (-6.0, 4.0, -1.0, 6.0), "box_b": (-1.0, 3.0, -2.0, 3.0)}


def rois(oracle):
    """cover_ref's regions, the two boxes, seen(35) alone (a pair adds nothing to the single) and
    the points nobody reaches."""
    def build():
        inst = cover_ref.instance(oracle)
        cloud = inst["cloud"]
        out = dict(inst["rois"])
        x, y = cloud[:, 0], cloud[:, 1]
        for name, (x0, x1, y0, y1) in BOXES.items():
            out[name] = ((x >= np.float32(x0)) & (x <= np.float32(x1)) & (y >= np.float32(y0)) &
                         (y <= np.float32(y1))).astype(np.uint8)
        one = np.zeros(inst["N"], np.uint8)
        one[inst["seen"][cover_ref.TIE_ROW]] = 1
        out["seen35"] = one
        nobody = np.ones(inst["N"], np.uint8)
        nobody[np.concatenate(inst["seen"])] = 0
        out["nobody"] = nobody
        return out

    return scan_ref.cached(("cover_pair", "rois"), build)


# (roi, separation, fixed): cover_ref.GRID's seven rows, then the boxes and the two edge regions
GRID = [(roi, sep, fixed) for roi, sep, fixed, _ in cover_ref.GRID] + [
    ("box_a", 0.0, ()), ("box_b", 0.0, ()), ("seen35", 0.0, ()), ("nobody", 0.0, ())]
N_COVER_GRID = len(cover_ref.GRID)


def grid_case(oracle, i, mutant=None):
    """The restatement's outputs of GRID[i] (cached)."""
    def build():
        inst = cover_ref.instance(oracle)
        roi, sep, fixed = GRID[i]
        return pair(inst["seen"], inst["poses"][:, :2], inst["N"], sep, fixed, rois(oracle)[roi],
                    mutant)

    return scan_ref.cached(("cover_pair", "case", i, mutant), build)


def repeated(inst, n):
    """The instance's 71 rows repeated to n poses: (poses, seen) -- the seen sets repeat with them."""
    rows = np.arange(n) % inst["poses"].shape[0]
    return np.ascontiguousarray(inst["poses"][rows]), [inst["seen"][r] for r in rows]


def ring_cloud(n_pts, nan_rows=0):
    """n_pts points on the circle of radius 0.8 m (the step table's second sample) under the
    azimuths of a 100-ray ring, then nan_rows non-finite rows in the middle."""
    a = 2.0 * np.pi * np.arange(n_pts) / 100.0
    c = np.column_stack([0.8 * np.cos(a), 0.8 * np.sin(a), 0.001 * (np.arange(n_pts) % 3),
                         np.zeros(n_pts)]).astype(np.float32)
    if nan_rows:
        bad = np.full((nan_rows, 4), np.nan, np.float32)
        bad[1::2, 0] = np.inf
        c = np.concatenate([c[:n_pts // 2], bad, c[n_pts // 2:]])
    return np.ascontiguousarray(c)


RING_POSES = np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [0.05, 0.02, 0.01, 0.0, 1.0],
                       [40.0, 40.0, 0.0, 0.0, 0.0], [-0.03, 0.0, 0.0, 0.0, -2.0]])
