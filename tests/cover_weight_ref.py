"""NumPy restatement of pcp_place_coverage_weighted's definition (include/pcp_abi.h): a helper of
tests/test_cover_weight_ref.py, test_place_coverage_weighted.py and test_cover_weight_cli.py, not a
conftest.

seen(p) is cover_ref's (the scan's restatement on the oracle's first hits, never the device).  The
greedy works on those index arrays, one boolean per terrain point and one int64 weight per point:
no bit plane anywhere, so a plane that is dropped, shifted or read with a sign shows.

`mutant` turns the restatement into one of the wrong implementations of MUTANTS;
tests/test_cover_weight_ref.py checks that the case grid tells every one from the definition."""
import cover_ref
import numpy as np
import scan_ref

OWNER_NONE = cover_ref.OWNER_NONE
MUTANTS = (("unweighted",) + tuple(f"drop_bit_{b}" for b in range(8)) +
           ("signed_byte", "need_static", "last_max", "points_as_weight", "zero_weight_in_R"))


def greedy(seen, xy, weight, k_max, sep=0.0, fixed=(), mutant=None):
    """The definition, step by step -> dict of every output plus `tie_rounds` (rounds whose
    maximum two alive poses share) and `stopped` (None, "dead" or "gain")."""
    n = len(seen)
    assert mutant is None or mutant in MUTANTS
    w8 = np.asarray(weight).reshape(-1)
    assert w8.min(initial=0) >= 0 and w8.max(initial=0) <= 255
    N = w8.shape[0]
    w = w8.astype(np.int64)
    in_roi = w != 0
    if mutant == "zero_weight_in_R":
        in_roi = np.ones(N, bool)
    if mutant == "unweighted":
        w = in_roi.astype(np.int64)
    elif mutant == "signed_byte":
        w = np.where(w >= 128, w - 256, w)
    elif mutant and mutant.startswith("drop_bit_"):
        w = w & ~(1 << int(mutant[-1]))
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    need = in_roi.copy()
    owner = np.full(N, OWNER_NONE, np.int32)
    sep2 = sep * sep if sep > 0 else 0.0

    def close(b):
        dx = xy[:, 0] - xy[b, 0]
        dy = xy[:, 1] - xy[b, 1]
        return dx * dx + dy * dy < sep2

    def commit(b, who):
        idx = seen[b][need[seen[b]]]
        owner[idx] = who
        if mutant != "need_static":
            need[idx] = False
        return int(w[idx].sum()), int(idx.size)

    alive = np.ones(n, bool)
    base_w = base_p = 0
    for i, f in enumerate(fixed):
        dw, dp = commit(f, i)
        base_w += dw
        base_p += dp
        alive[f] = False
        if sep2 > 0:
            alive &= ~close(f)
    sel, gain, gpts, cov, rows = [], [], [], [], []
    ties, stopped = 0, None
    covered = base_w
    for r in range(k_max):
        if not alive.any():
            stopped = "dead"
            break
        g = np.full(n, -1, np.int64)
        for p in np.nonzero(alive)[0]:
            s = seen[p]
            g[p] = int(w[s[need[s]]].sum())
        top = int(g[alive].max())
        at = np.nonzero(alive & (g == top))[0]
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
        _, dp = commit(b, len(fixed) + r)
        gpts.append(top if mutant == "points_as_weight" else dp)
        alive[b] = False
        if sep2 > 0:
            alive &= ~close(b)
    return {"selected": np.array(sel, np.int64), "gain": np.array(gain, np.uint64),
            "gain_points": np.array(gpts, np.uint64),
            "covered_after": np.array(cov, np.uint64), "n_selected": len(sel), "n_points": N,
            "roi_points": int(np.count_nonzero(in_roi)), "roi_weight": int(w[in_roi].sum()),
            "base_covered": base_w, "base_points": base_p,
            "seen_points": np.array([s.size for s in seen], np.uint32),
            "round_gains": np.array(rows, np.int64).reshape(len(rows), n),
            "point_owner": owner, "tie_rounds": int(ties), "stopped": stopped}


SHARED = ("selected", "gain", "covered_after", "seen_points")


def assert_weighted_equal(got, ref):
    """Every output of the call against the restatement's."""
    for k in ("n_selected", "n_points", "roi_points", "roi_weight", "base_covered", "base_points"):
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    for k in SHARED + ("gain_points",):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64),
                                      np.asarray(ref[k]).astype(np.int64), err_msg=k)
    if got.get("round_gains") is not None:
        np.testing.assert_array_equal(got["round_gains"], ref["round_gains"])
    if got.get("point_owner") is not None:
        np.testing.assert_array_equal(got["point_owner"], ref["point_owner"])


# ---- the weight patterns over cover_ref's instance -----------------------------------------------
PATTERNS = ("ones", "box200", "ramp", "ramp0", "x128", "three")
USED_BITS = {"ones": 0b1, "box200": 0b11001001, "ramp": 0xff, "ramp0": 0xff, "x128": 0b10000000,
             "three": 0xff}
# (separation, fixed, k_max), crossed with every pattern
SETTINGS = [(0.0, (), 16), (cover_ref.SEP, (), 16), (0.0, (10, 40), 4),
            (cover_ref.SEP, (10, 40), 4)]
GRID = [(name, *s) for name in PATTERNS for s in SETTINGS]


def patterns(rois, N):
    i = np.arange(N, dtype=np.int64)
    box, xpos = rois["box"] != 0, rois["xpos"] != 0
    out = {"ones": np.ones(N, np.int64),
           "box200": np.where(box, 200, 1),
           "ramp": 1 + (37 * i) % 255,
           "ramp0": (37 * i) % 256,
           "x128": 128 * xpos.astype(np.int64),
           "three": np.where(box, 255, np.where(xpos, 10, 1))}
    return {k: np.ascontiguousarray(v, np.uint8) for k, v in out.items()}


def weights(oracle):
    """name -> uint8 [N] on cover_ref.instance (cached, never modified)."""
    def build():
        inst = cover_ref.instance(oracle)
        return patterns(inst["rois"], inst["N"])

    return scan_ref.cached(("cover_weight", "patterns"), build)


def grid_case(oracle, i, mutant=None):
    """The restatement's outputs of GRID[i] (cached)."""
    def build():
        inst = cover_ref.instance(oracle)
        name, sep, fixed, k = GRID[i]
        return greedy(inst["seen"], inst["poses"][:, :2], weights(oracle)[name], k, sep, fixed,
                      mutant)

    return scan_ref.cached(("cover_weight", "case", i, mutant), build)


def unit_greedy(oracle, region, sep, fixed, k):
    """cover_ref.greedy on the instance with roi = `region` (bytes or None), cached."""
    def build():
        inst = cover_ref.instance(oracle)
        return cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], k, sep, fixed,
                                region)

    key = None if region is None else np.asarray(region).tobytes()
    return scan_ref.cached(("cover_weight", "unit", key, sep, fixed, k), build)
