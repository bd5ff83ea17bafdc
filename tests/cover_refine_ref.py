"""NumPy restatement of pcp_place_coverage_refine's definition (include/pcp_abi.h): a helper of
tests/test_cover_refine_ref.py, test_place_coverage_refine.py, test_cover_refine_host.py and
test_cover_refine_cli.py, not a conftest.

seen(p) is cover_ref's: the scan's restatement on the oracle's first hits, per pose the sorted
array of input indices -- nothing from the device.  An evaluation counts, per slot i, the points of
R that the other slots leave free (reached by none of them) and every pose's share of those: a 0/1
matrix over the points of R any pose reaches times the slots' free rows, as a float64 product
(every count is far below 2^53: exact).  u[i][p] = |L_i & R| + |seen(p) & R \\ L_i|: the definition's
union, not the device's split into class rows.

`mutant` turns the restatement into one of eight wrong implementations; tests/
test_cover_refine_ref.py checks that the case grid tells every one of them from the definition."""
import cover_pair_ref
import cover_ref
import numpy as np
import scan_ref

OWNER_NONE = cover_ref.OWNER_NONE
MAX_MOVES = 64   # PCP_REFINE_MAX_MOVES
MUTANTS = ("last_max", "sep_le", "roi_ignored", "locked_moves", "sep_outgoing", "multi_lost",
           "set_static", "alias64")


def refine(seen, xy, N, start, n_locked=0, max_moves=16, sep=0.0, roi=None, mutant=None):
    """The definition, step by step -> dict of every output of the call."""
    n = len(seen)
    assert mutant is None or mutant in MUTANTS
    if mutant == "alias64":   # pose p + 64 lands on p's bits
        seen = [np.unique(np.concatenate([seen[q] for q in range(p % 64, n, 64)]))
                if p < 64 else np.zeros(0, np.int64) for p in range(n)]
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    in_roi = np.ones(N, bool) if roi is None else np.asarray(roi).reshape(-1) != 0
    assert in_roi.shape[0] == N
    roi_points = int(np.count_nonzero(in_roi))
    if mutant == "roi_ignored":
        in_roi = np.ones(N, bool)
    s = [int(p) for p in start]
    k = len(s)
    assert 1 <= k and len(set(s)) == k and 0 <= n_locked <= k and 0 <= max_moves <= MAX_MOVES
    lock = 0 if mutant == "locked_moves" else n_locked
    sep2 = sep * sep if sep > 0 else 0.0
    # the 0/1 rows over the points of R that any pose reaches
    M = [q[in_roi[q]] for q in seen]
    cols = np.unique(np.concatenate(M + [np.zeros(0, np.int64)]))
    B = np.zeros((n, cols.size), np.float64)
    for p, m in enumerate(M):
        B[p, np.searchsorted(cols, m)] = 1.0
    d2 = ((xy[:, None, 0] - xy[None, :, 0]) ** 2) + ((xy[:, None, 1] - xy[None, :, 1]) ** 2)
    close = (d2 <= sep2 if mutant == "sep_le" else d2 < sep2) if sep2 > 0 else np.zeros((n, n), bool)

    def evaluate(cur):
        """-> (T, u [k][n] with -1 at the inadmissible moves, |E_i| [k])."""
        cnt = B[cur].sum(axis=0)
        T = int(np.count_nonzero(cnt > 0))
        u = np.full((k, n), -1, np.int64)
        uniq = np.zeros(k, np.int64)
        in_s = np.zeros(n, bool)
        in_s[cur] = True
        for i in range(k):
            only = (cnt == 1) & (B[cur[i]] > 0)        # E_i
            uniq[i] = np.count_nonzero(only)
            if i < lock:
                continue
            if mutant == "multi_lost":   # every point of slot i counted as lost with it
                mine = B[cur[i]] > 0
                val = T - int(np.count_nonzero(mine)) + np.rint(B @ ((cnt == 0) | mine)).astype(np.int64)
            else:
                free = (cnt - B[cur[i]]) == 0              # R less L_i, among the reached points
                val = (T - uniq[i]) + np.rint(B @ free.astype(np.float64)).astype(np.int64)
            ok = ~in_s
            for j in range(k):
                if j != i or mutant == "sep_outgoing":
                    ok &= ~close[cur[j]]
            u[i] = np.where(ok, val, -1)
        return T, u, uniq

    moves, tables = [], []
    start_T = None
    converged = 0
    frozen = list(s)
    while True:
        T_now, u, uniq = evaluate(frozen if mutant == "set_static" else s)
        if start_T is None:
            start_T = T = T_now
        tables.append(u)
        flat = u.ravel()
        top = int(flat.max())
        at = np.nonzero(flat == top)[0]
        b = int(at[-1] if mutant == "last_max" else at[0])
        if top < 0 or top <= T:
            converged = 1
            break
        if len(moves) >= max_moves:
            break
        i, p = divmod(b, n)
        moves.append((i, s[i], p, top))
        s[i] = p
        T = top
    owner = np.full(N, OWNER_NONE, np.int32)
    for i in reversed(range(k)):   # the lowest slot that reaches the point
        idx = seen[s[i]]
        owner[idx[in_roi[idx]]] = i
    return {"selected": np.array(s, np.int64), "covered": T, "start_covered": start_T,
            "n_moves": len(moves), "converged": converged,
            "move_slot": np.array([m[0] for m in moves], np.int32),
            "move_from": np.array([m[1] for m in moves], np.int64),
            "move_to": np.array([m[2] for m in moves], np.int64),
            "move_covered": np.array([m[3] for m in moves], np.uint64),
            "swap_covered": np.array(tables, np.int64).reshape(len(tables), k, n),
            "slot_unique": uniq.astype(np.uint64), "point_owner": owner,
            "seen_points": np.array([q.size for q in seen], np.uint32), "n_points": N,
            "roi_points": roi_points}


def assert_refine_equal(got, ref):
    """Every output of the call against the restatement's."""
    for key in ("covered", "start_covered", "n_moves", "converged", "n_points", "roi_points"):
        assert int(got[key]) == int(ref[key]), (key, got[key], ref[key])
    for key in ("selected", "move_slot", "move_from", "move_to", "move_covered", "slot_unique",
                "seen_points"):
        np.testing.assert_array_equal(np.asarray(got[key]).astype(np.int64),
                                      np.asarray(ref[key]).astype(np.int64), err_msg=key)
    if got.get("swap_covered") is not None:
        np.testing.assert_array_equal(got["swap_covered"], ref["swap_covered"])
    if got.get("point_owner") is not None:
        np.testing.assert_array_equal(got["point_owner"], ref["point_owner"])


# ---- the case grid on cover_ref's 71-pose instance ----------------------------------------------
REGIONS = ("all", "box", "xpos", "box_a", "box_b")
SEPS = (0.0, cover_ref.SEP)
KS = (1, 2, 3, 4, 8, 16)
STARTS = ("greedy", "first")
MOVES = (0, 1, 16)


def rois(oracle):
    return cover_pair_ref.rois(oracle)


def start_set(oracle, roi, sep, k, kind):
    """`first`: poses 0 .. k-1.  `greedy`: pcp_place_coverage's restatement for the region and the
    separation, filled up to k with the lowest poses it left out when it stops early."""
    if kind == "first":
        return list(range(k))

    def build():
        inst = cover_ref.instance(oracle)
        g = cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], 16, sep, (),
                             rois(oracle)[roi])
        return g["selected"].tolist()

    sel = scan_ref.cached(("cover_refine", "greedy", roi, sep), build)[:k]
    return sel + [p for p in range(71) if p not in sel][:k - len(sel)]


def locked_counts(k):
    return sorted({0, min(2, k), k})


def grid_case(oracle, roi, sep, k, kind, n_locked, max_moves, mutant=None):
    """The restatement's outputs of one case of the grid (cached)."""
    def build():
        inst = cover_ref.instance(oracle)
        return refine(inst["seen"], inst["poses"][:, :2], inst["N"],
                      start_set(oracle, roi, sep, k, kind), n_locked, max_moves, sep,
                      rois(oracle)[roi], mutant)

    return scan_ref.cached(("cover_refine", "case", roi, sep, k, kind, n_locked, max_moves, mutant),
                           build)


# the rows of DESIGN.md section 6o's table: (roi, separation, start, moves (slot, from, to,
# covered), start_covered, final set)
TABLE = [
    ("box_a", 0.0, [51, 49], [(0, 51, 43, 2312), (1, 49, 50, 2330)], 2294, [43, 50]),
    ("box_a", 0.0, [51, 49, 43], [(0, 51, 0, 3399), (1, 49, 50, 3418)], 3387, [0, 50, 43]),
    ("box_a", 2.5, [51, 49], [(0, 51, 43, 2312)], 2294, [43, 49]),
    ("all", 2.5, [35, 51, 25, 49, 19, 39, 37, 23],
     [(2, 25, 33, 8721), (7, 23, 17, 8796), (6, 37, 45, 8801)], 8665,
     [35, 51, 33, 49, 19, 39, 45, 17]),
    ("all", 0.0, [0, 1, 2, 3], [(2, 2, 35, 4125), (3, 3, 43, 4613), (1, 1, 51, 4940),
                                (0, 0, 25, 4985)], 3282, [25, 51, 35, 43]),
    ("all", 2.5, [0, 1, 2, 3], [(2, 2, 51, 4030), (1, 1, 27, 4382), (3, 3, 24, 4661),
                                (0, 0, 49, 4676), (1, 27, 35, 4786), (3, 24, 25, 4890)], 3282,
     [49, 35, 51, 25]),
]
