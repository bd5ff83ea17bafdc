"""The definition of pcp_place_pair (include/pcp_abi.h), restated in NumPy: the checker of the
exact pair search.  S [P, C], Z [C] as pcp_score_matrix returns them, xy [P, 2] the poses' x, y.
Sums are sequential (cumsum) in cell order from +0.0 over the positive elements, as
tests/test_place_sensors.py::greedy."""
import numpy as np

OWNER_ZX120 = -1   # PCP_OWNER_ZX120 / PCP_OWNER_NONE (tests/test_place_abi.py pins the values)
OWNER_NONE = -2


def smax(a, b):
    """The reference's std::max(a, b): (a < b) ? b : a, elementwise."""
    return np.where(a < b, b, a)


def osum(V):
    """Rows of V: the ordered sum from +0.0 of the positive elements, and their count."""
    V = np.atleast_2d(np.asarray(V, np.float64))
    pos = V > 0
    if V.shape[1] == 0:
        return np.zeros(V.shape[0]), np.zeros(V.shape[0], np.int32)
    # (adding +0.0 to a non-negative running sum leaves its bits: cumsum is sequential)
    return np.cumsum(np.where(pos, V, 0.0), axis=1)[:, -1], pos.sum(axis=1).astype(np.int32)


def _close(xy, i, j, sep):
    dx, dy = xy[i, 0] - xy[j, 0], xy[i, 1] - xy[j, 1]
    return dx * dx + dy * dy < sep * sep


def place_pair(S, Z, xy, fixed=(), sep=0.0):
    S = np.asarray(S, np.float64)
    Z = np.asarray(Z, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    P, C = S.shape
    fixed = [int(f) for f in fixed]
    nf = len(fixed)
    # 1. the base
    base = Z.copy()
    owner = np.where(Z > 0, OWNER_ZX120, OWNER_NONE).astype(np.int32)
    for i, f in enumerate(fixed):
        take = base < S[f]
        owner[take] = i
        base = smax(base, S[f])
    t, c = osum(base)
    out = {"base_total": float(t[0]), "base_covered": int(c[0])}
    # 2. admissible poses
    adm = np.ones(P, bool)
    for f in fixed:
        adm[f] = False
        if sep > 0:
            adm &= ~_close(xy, np.arange(P), f, sep)
    # 3. singles
    M = smax(base[None, :], S)
    st, sc = osum(M) if P else (np.zeros(0), np.zeros(0, np.int32))
    st = np.where(adm, st, -np.inf)
    out["single_totals"] = st
    bs, bst = -1, -np.inf
    for p in range(P):
        if st[p] > bst:
            bs, bst = p, st[p]
    out["best_single"] = bs
    out["single_total"] = float(bst)
    out["single_covered"] = int(sc[bs]) if bs >= 0 else 0
    # 4. pairs
    T = np.full((P, P), -np.inf)
    Cv = np.zeros((P, P), np.int32)
    for a in range(P):
        if not adm[a] or a + 1 >= P:
            continue
        ok = adm[a + 1:].copy()
        if sep > 0:
            ok &= ~_close(xy, np.arange(a + 1, P), a, sep)
        if not ok.any():
            continue
        b = np.arange(a + 1, P)[ok]
        t, c = osum(smax(M[a][None, :], S[b]))
        T[a, b] = t
        Cv[a, b] = c
    out["pair_totals"] = T
    out["n_pairs"] = int(np.isfinite(T).sum())
    bp, bpt = (-1, -1), -np.inf
    if P:
        k = int(np.argmax(T))   # the first maximum in row-major order
        if T.flat[k] > -np.inf:
            bp, bpt = (k // P, k % P), T.flat[k]
    out["best_pair"] = np.array(bp, np.int64)
    out["pair_total"] = float(bpt)
    out["pair_covered"] = int(Cv[bp]) if bp[0] >= 0 else 0
    # 5. the answer
    if bp[0] >= 0 and bpt > bst:
        chosen = list(bp)
    elif bs >= 0 and bst > out["base_total"]:
        chosen = [bs]
    else:
        chosen = []
    out["n_selected"] = len(chosen)
    for i, q in enumerate(chosen):
        take = base < S[q]
        owner[take] = nf + i
        base = smax(base, S[q])
    out["cell_score"] = base
    out["cell_owner"] = owner
    return out


def runner_up_gap(ref):
    """Best minus runner-up of the pair table, of the singles, and |pair - single| (what decides
    n_selected): the smallest of those that exist."""
    gaps = []
    t = np.sort(ref["pair_totals"][np.isfinite(ref["pair_totals"])])[::-1]
    if t.size > 1:
        gaps.append(t[0] - t[1])
    s = np.sort(ref["single_totals"][np.isfinite(ref["single_totals"])])[::-1]
    if s.size > 1:
        gaps.append(s[0] - s[1])
    if t.size and s.size:
        gaps.append(abs(t[0] - s[0]))
    if s.size:
        gaps.append(s[0] - ref["base_total"])
    return min(gaps) if gaps else np.inf
