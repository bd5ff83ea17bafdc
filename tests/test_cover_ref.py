"""tests/cover_ref.py, the NumPy restatement of pcp_place_coverage, without a GPU: against an
independent greedy on Python sets, and the preconditions of the common instance -- the case grid
must hold a tie at the maximum, an early stop, a pose that sees nothing and a partial last word,
and must tell six wrong implementations from the definition."""
import cover_ref
import numpy as np
import pytest


def _set_greedy(seen, xy, N, k_max, sep, fixed, roi):
    """The definition on Python sets and scalar loops."""
    n = len(seen)
    S = [set(int(i) for i in s) for s in seen]
    need = set(range(N)) if roi is None else {i for i in range(N) if roi[i]}
    R = len(need)
    owner = [cover_ref.OWNER_NONE] * N

    def near(a, b):
        dx, dy = xy[a][0] - xy[b][0], xy[a][1] - xy[b][1]
        return sep > 0 and dx * dx + dy * dy < sep * sep

    alive = [True] * n
    for i, f in enumerate(fixed):
        for pt in S[f] & need:
            owner[pt] = i
        need -= S[f]
    for p in range(n):
        if p in fixed or any(near(p, f) for f in fixed):
            alive[p] = False
    base = R - len(need)
    sel, gain, cov, rows = [], [], [], []
    covered = base
    for r in range(k_max):
        if not any(alive):
            break
        g = [len(S[p] & need) if alive[p] else -1 for p in range(n)]
        b = max(range(n), key=lambda p: (g[p], -p))
        if g[b] <= 0:
            break
        rows.append(g)
        sel.append(b)
        gain.append(g[b])
        covered += g[b]
        cov.append(covered)
        for pt in S[b] & need:
            owner[pt] = len(fixed) + r
        need -= S[b]
        for p in range(n):
            if p == b or near(p, b):
                alive[p] = False
    return sel, gain, cov, rows, owner, base, R


@pytest.mark.parametrize("seed", range(12))
def test_restatement_is_the_set_greedy(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 90))
    N = int(rng.integers(1, 200))
    seen = [np.unique(rng.integers(0, N, int(rng.integers(0, 40)))) for _ in range(n)]
    if n > 3:
        seen[n - 1] = seen[1].copy()          # a tie
    xy = rng.integers(-3, 4, (n, 2)).astype(np.float64)   # lattice points: equalities at sep 2
    sep = [0.0, 2.0, -1.0][seed % 3]
    fixed = tuple(int(f) for f in rng.choice(n, min(n, seed % 3), replace=False))
    roi = None if seed % 4 == 0 else (rng.random(N) < 0.6).astype(np.uint8)
    k_max = int(rng.integers(1, 17))
    ref = cover_ref.greedy(seen, xy, N, k_max, sep, fixed, roi)
    sel, gain, cov, rows, owner, base, R = _set_greedy(seen, xy.tolist(), N, k_max, sep, fixed, roi)
    assert ref["selected"].tolist() == sel and ref["gain"].tolist() == gain
    assert ref["covered_after"].tolist() == cov and ref["round_gains"].tolist() == rows
    assert ref["point_owner"].tolist() == owner
    assert ref["base_covered"] == base and ref["roi_points"] == R
    assert ref["n_selected"] == len(sel)
    assert ref["seen_points"].tolist() == [len(s) for s in seen]


def test_instance_preconditions(oracle):
    inst = cover_ref.instance(oracle)
    assert inst["poses"].shape == (71, 5) and inst["N"] == 120300
    assert inst["N"] % 64 != 0                                   # a partial last word
    np.testing.assert_array_equal(inst["poses"][70], inst["poses"][cover_ref.TIE_ROW])
    np.testing.assert_array_equal(inst["seen"][70], inst["seen"][cover_ref.TIE_ROW])
    assert inst["seen"][4].size == 0                             # the far pose sees nothing
    assert min(s.size for i, s in enumerate(inst["seen"]) if i != 4) > 0
    # the lattice's spacing is exact: two steps apart is exactly the separation
    xy = inst["poses"][6:70, :2]
    d2 = (xy[0, 0] - xy[2, 0]) ** 2 + (xy[0, 1] - xy[2, 1]) ** 2
    assert d2 == cover_ref.SEP * cover_ref.SEP
    cases = [cover_ref.grid_case(oracle, i) for i in range(len(cover_ref.GRID))]
    for c, (_, _, fixed, k) in zip(cases, cover_ref.GRID):
        assert c["n_selected"] >= 2                              # several rounds everywhere
        assert c["n_selected"] <= k
        assert (c["base_covered"] > 0) == bool(fixed)
    assert any(c["tie_rounds"] > 0 for c in cases)               # the first-maximum rule decides
    assert any(c["stopped"] is not None and c["n_selected"] < k  # an early stop
               for c, (_, _, _, k) in zip(cases, cover_ref.GRID))
    for name, roi in inst["rois"].items():
        if roi is not None:
            assert 0 < np.count_nonzero(roi) < inst["N"], name


@pytest.mark.parametrize("mutant", cover_ref.MUTANTS)
def test_grid_rejects_the_mutant(oracle, mutant):
    """Each wrong implementation changes `selected` on at least one case of the grid."""
    differs = []
    for i in range(len(cover_ref.GRID)):
        ref = cover_ref.grid_case(oracle, i)
        bad = cover_ref.grid_case(oracle, i, mutant)
        differs.append(ref["selected"].tolist() != bad["selected"].tolist())
    assert any(differs), mutant
