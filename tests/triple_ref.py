"""The definition of pcp_place_triple (include/pcp_abi.h), restated in NumPy: the checker of the
exact triple search.  S [P, C], Z [C] as pcp_score_matrix returns them, xy [P, 2] the poses' x, y.
Steps 1 to 4 are tests/pair_ref.py's place_pair; sums are sequential (cumsum) in cell order from
+0.0 over the positive elements, as there."""
import numpy as np
from pair_ref import OWNER_NONE, OWNER_ZX120, _close, osum, place_pair, smax  # noqa: F401
import pair_ref


def place_triple(S, Z, xy, fixed=(), sep=0.0, want_table=True):
    S = np.asarray(S, np.float64)
    Z = np.asarray(Z, np.float64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    P, C = S.shape
    fixed = [int(f) for f in fixed]
    nf = len(fixed)
    # 1.-4. the pair call's values
    pr = place_pair(S, Z, xy, fixed, sep)
    out = {k: pr[k] for k in ("base_total", "base_covered", "best_single", "single_total",
                              "single_covered", "best_pair", "pair_total", "pair_covered",
                              "single_totals", "pair_totals", "n_pairs")}
    base = Z.copy()
    owner = np.where(Z > 0, OWNER_ZX120, OWNER_NONE).astype(np.int32)
    for i, f in enumerate(fixed):
        take = base < S[f]
        owner[take] = i
        base = smax(base, S[f])
    adm = np.isfinite(pr["single_totals"]) if P else np.zeros(0, bool)
    # (a single's total is a finite sum exactly where the pose is admissible)
    M = smax(base[None, :], S)
    # 5. triples: an admissible pair (a, b) is a finite entry of the pair table
    T3 = np.full((P, P, P), -np.inf) if want_table else None
    ft = np.full(P, -np.inf)
    fp = np.full((P, 2), -1, np.int64)
    fc = np.zeros(P, np.int32)
    n_triples = 0
    for a in range(P):
        if not adm[a]:
            continue
        for b in range(a + 1, P):
            if not np.isfinite(pr["pair_totals"][a, b]) or b + 1 >= P:
                continue
            ok = np.isfinite(pr["pair_totals"][a, b + 1:]) & np.isfinite(pr["pair_totals"][b, b + 1:])
            if not ok.any():
                continue
            c = np.arange(b + 1, P)[ok]
            t, cov = osum(smax(smax(M[a], S[b])[None, :], S[c]))
            n_triples += c.size
            if want_table:
                T3[a, b, c] = t
            k = int(np.argmax(t))   # the first maximum over c; rows b in ascending order
            if t[k] > ft[a]:
                ft[a], fp[a], fc[a] = t[k], (b, c[k]), cov[k]
    out["n_triples"] = n_triples
    out["first_totals"] = ft
    out["first_partners"] = fp
    if want_table:
        out["triple_totals"] = T3
    bt, btt = (-1, -1, -1), -np.inf
    for a in range(P):
        if ft[a] > btt:
            bt, btt = (a, int(fp[a, 0]), int(fp[a, 1])), ft[a]
    out["best_triple"] = np.array(bt, np.int64)
    out["triple_total"] = float(btt)
    out["triple_covered"] = int(fc[bt[0]]) if bt[0] >= 0 else 0
    # 6. the answer
    T, chosen = out["base_total"], []
    if out["best_single"] >= 0 and out["single_total"] > T:
        T, chosen = out["single_total"], [int(out["best_single"])]
    if out["best_pair"][0] >= 0 and out["pair_total"] > T:
        T, chosen = out["pair_total"], [int(q) for q in out["best_pair"]]
    if bt[0] >= 0 and btt > T:
        chosen = list(bt)
    out["n_selected"] = len(chosen)
    for i, q in enumerate(chosen):
        take = base < S[q]
        owner[take] = nf + i
        base = smax(base, S[q])
    out["cell_score"] = base
    out["cell_owner"] = owner
    return out


def triple_values(ref):
    """The finite triple totals in descending order (the reference was run with its table)."""
    t = ref["triple_totals"]
    return np.sort(t[np.isfinite(t)])[::-1]


def runner_up_gap(ref):
    """pair_ref.runner_up_gap (the pairs', the singles' and what decides between them), extended by
    best minus runner-up of the triples and by the gaps that decide step 6: the smallest of those
    that exist."""
    gaps = [pair_ref.runner_up_gap(ref)]
    t = triple_values(ref)
    if t.size > 1:
        gaps.append(t[0] - t[1])
    if t.size:
        # step 6: the triple against the best of base, single and pair
        rivals = [ref["base_total"]]
        if ref["best_single"] >= 0:
            rivals.append(ref["single_total"])
        if ref["best_pair"][0] >= 0:
            rivals.append(ref["pair_total"])
        gaps.append(abs(t[0] - max(rivals)))
    if ref["best_pair"][0] >= 0:
        gaps.append(abs(ref["pair_total"] - ref["base_total"]))
    return min(gaps) if gaps else np.inf
