"""The definition of pcp_place_refine (include/pcp_abi.h), restated in NumPy: the checker of the
1-exchange refinement.  S [P, C], Z [C] as pcp_score_matrix returns them, xy [P, 2] the poses'
x, y.  The folds are the literal ones (fold(s without slot i) for every slot, in list order), not
the largest / second-largest shortcut of the kernels; sums as tests/pair_ref.py's."""
import numpy as np
from pair_ref import OWNER_NONE, OWNER_ZX120, osum, smax

MAX_MOVES = 64   # PCP_REFINE_MAX_MOVES


def fold(S, Z, lst):
    base = np.asarray(Z, np.float64).copy()
    for q in lst:
        base = smax(base, S[q])
    return base


def evaluate(S, Z, xy, s, n_locked, sep):
    """One evaluation of the set s: u [k, P] (-inf where the move is inadmissible), counts."""
    P = S.shape[0]
    k = len(s)
    u = np.full((k, P), -np.inf)
    cov = np.zeros((k, P), np.int32)
    inset = np.zeros(P, bool)
    inset[s] = True
    for i in range(n_locked, k):
        L = fold(S, Z, [q for j, q in enumerate(s) if j != i])
        ok = ~inset
        if sep > 0:
            for j, q in enumerate(s):
                if j != i:
                    dx, dy = xy[:, 0] - xy[q, 0], xy[:, 1] - xy[q, 1]
                    ok &= ~(dx * dx + dy * dy < sep * sep)
        t, c = osum(smax(L[None, :], S))
        u[i] = np.where(ok, t, -np.inf)
        cov[i] = c
    return u, cov


def place_refine(S, Z, xy, start, n_locked=0, max_moves=MAX_MOVES, sep=0.0):
    S = np.asarray(S, np.float64)
    Z = np.asarray(Z, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    P = S.shape[0]
    s = [int(q) for q in start]
    k = len(s)
    assert 1 <= k and len(set(s)) == k and all(0 <= q < P for q in s)
    assert 0 <= n_locked <= k and 0 <= max_moves <= MAX_MOVES
    t, c = osum(fold(S, Z, s))
    T, cov = float(t[0]), int(c[0])
    out = {"start_total": T, "start_covered": cov, "swap_totals": [], "move_slot": [],
           "move_from": [], "move_to": [], "move_total": [], "move_covered": []}
    gaps = []
    while True:
        u, uc = evaluate(S, Z, xy, s, n_locked, sep)
        out["swap_totals"].append(u)
        b = int(np.argmax(u))   # the first maximum in row-major order
        i, p = divmod(b, P)
        best = u[i, p]
        if not best > T:
            out["converged"] = 1
            gaps.append(T - best)
            break
        if len(out["move_slot"]) == max_moves:
            out["converged"] = 0
            break
        live = np.sort(u[np.isfinite(u)])[::-1]
        gaps.append(best - T)
        if live.size > 1:
            gaps.append(live[0] - live[1])
        out["move_slot"].append(i)
        out["move_from"].append(s[i])
        out["move_to"].append(p)
        out["move_total"].append(float(best))
        out["move_covered"].append(int(uc[i, p]))
        s[i] = p
        T, cov = float(best), int(uc[i, p])
    out["n_moves"] = len(out["move_slot"])
    out["selected"] = np.array(s, np.int64)
    out["total"] = T
    out["covered"] = cov
    out["swap_totals"] = np.array(out["swap_totals"], np.float64).reshape(-1, k, P)
    for key, dt in (("move_slot", np.int32), ("move_from", np.int64), ("move_to", np.int64),
                    ("move_total", np.float64), ("move_covered", np.int32)):
        out[key] = np.array(out[key], dt)
    base = Z.copy()
    owner = np.where(Z > 0, OWNER_ZX120, OWNER_NONE).astype(np.int32)
    for i, q in enumerate(s):
        take = base < S[q]
        owner[take] = i
        base = smax(base, S[q])
    out["cell_score"] = base
    out["cell_owner"] = owner
    # the smallest of every accepted gain, every accepted best-minus-runner-up and the final
    # T - best: what a perturbation of the matrix would have to overcome to change a decision
    out["decision_gap"] = float(min(gaps)) if gaps else np.inf
    return out
