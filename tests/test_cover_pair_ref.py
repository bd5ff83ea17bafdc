"""tests/cover_pair_ref.py, the NumPy restatement of pcp_place_coverage_pair, without a GPU: against
an independent search on Python sets, the preconditions of its case grid -- two regions on which
greedy's two rounds are not the best pair, one of them with the best single pose outside the best
pair -- and the grid's power to tell six wrong implementations from the definition."""
import cover_pair_ref
import cover_ref
import numpy as np
import pytest


def _set_pair(seen, xy, N, sep, fixed, roi):
    """The definition on Python sets and scalar loops."""
    n = len(seen)
    S = [set(int(i) for i in s) for s in seen]
    need = set(range(N)) if roi is None else {i for i in range(N) if roi[i]}
    R = len(need)
    owner = [cover_ref.OWNER_NONE] * N

    def near(a, b):
        dx, dy = xy[a][0] - xy[b][0], xy[a][1] - xy[b][1]
        return sep > 0 and dx * dx + dy * dy < sep * sep

    for i, f in enumerate(fixed):
        for pt in S[f] & need:
            owner[pt] = i
        need -= S[f]
    base = R - len(need)
    adm = [p not in fixed and not any(near(p, f) for f in fixed) for p in range(n)]
    g = [len(S[p] & need) for p in range(n)]
    bs, sg = -1, 0
    for p in range(n):
        if adm[p] and (bs < 0 or g[p] > sg):
            bs, sg = p, g[p]
    bp, pg = (-1, -1), 0
    table = [[-1] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            if adm[a] and adm[b] and not near(a, b):
                table[a][b] = len((S[a] | S[b]) & need)
                if bp[0] < 0 or table[a][b] > pg:
                    bp, pg = (a, b), table[a][b]
    chosen = list(bp) if bp[0] >= 0 and pg > sg else ([bs] if bs >= 0 and sg > 0 else [])
    for r, p in enumerate(chosen):
        for pt in S[p] & need:
            owner[pt] = len(fixed) + r
        need -= S[p]
    return {"chosen": chosen, "bp": bp, "pg": pg, "bs": bs, "sg": sg, "table": table,
            "owner": owner, "base": base, "R": R,
            "singles": [g[p] if adm[p] else -1 for p in range(n)]}


@pytest.mark.parametrize("seed", range(12))
def test_restatement_is_the_set_search(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 40))
    N = int(rng.integers(1, 200))
    seen = [np.unique(rng.integers(0, N, int(rng.integers(0, 40)))) for _ in range(n)]
    if n > 3:
        seen[n - 1] = seen[1].copy()          # a tie
    xy = rng.integers(-3, 4, (n, 2)).astype(np.float64)   # lattice points: equalities at sep 2
    sep = [0.0, 2.0, -1.0][seed % 3]
    fixed = tuple(int(f) for f in rng.choice(n, min(n, seed % 3), replace=False))
    roi = None if seed % 4 == 0 else (rng.random(N) < 0.6).astype(np.uint8)
    ref = cover_pair_ref.pair(seen, xy, N, sep, fixed, roi)
    want = _set_pair(seen, xy.tolist(), N, sep, fixed, roi)
    assert ref["best_pair"].tolist() == list(want["bp"]) and ref["pair_gain"] == want["pg"]
    assert ref["best_single"] == want["bs"] and ref["single_gain"] == want["sg"]
    assert ref["n_selected"] == len(want["chosen"])
    assert ref["pair_gains"].tolist() == want["table"]
    assert ref["single_gains"].tolist() == want["singles"]
    assert ref["point_owner"].tolist() == want["owner"]
    assert ref["base_covered"] == want["base"] and ref["roi_points"] == want["R"]
    for a in range(n):   # the rows' partners: the first maximum of the table's row
        row = want["table"][a]
        top = max(row)
        assert ref["partner_gain"][a] == top
        assert ref["partner"][a] == (row.index(top) if top >= 0 else -1)


def _greedy2(oracle, i):
    inst = cover_ref.instance(oracle)
    roi, sep, fixed = cover_pair_ref.GRID[i]
    return cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], 2, sep, fixed,
                            cover_pair_ref.rois(oracle)[roi])


def test_the_boxes_separate_the_exact_pair_from_greedy(oracle):
    """The two regions the case grid adds: greedy's two rounds reach fewer points than the best
    pair, and on the first the best single pose is no member of the best pair."""
    a = cover_pair_ref.grid_case(oracle, cover_pair_ref.N_COVER_GRID)
    ga = _greedy2(oracle, cover_pair_ref.N_COVER_GRID)
    print("box_a", a["best_pair"], a["pair_gain"], ga["selected"], ga["gain"], a["best_single"])
    assert a["best_pair"].tolist() == [43, 50] and a["pair_gain"] == 2330
    assert ga["selected"].tolist() == [51, 49] and int(ga["covered_after"][-1]) == 2294
    assert a["best_single"] == 51 == ga["selected"][0] and 51 not in a["best_pair"].tolist()
    assert a["n_selected"] == 2 and a["pair_gain"] > int(ga["covered_after"][-1])
    b = cover_pair_ref.grid_case(oracle, cover_pair_ref.N_COVER_GRID + 1)
    gb = _greedy2(oracle, cover_pair_ref.N_COVER_GRID + 1)
    print("box_b", b["best_pair"], b["pair_gain"], gb["selected"], gb["gain"], b["best_single"])
    assert b["best_pair"].tolist() == [34, 42] and b["pair_gain"] == 2132
    assert gb["selected"].tolist() == [0, 34] and int(gb["covered_after"][-1]) == 2105
    assert b["n_selected"] == 2 and b["pair_gain"] > int(gb["covered_after"][-1])


def test_grid_preconditions(oracle):
    inst = cover_ref.instance(oracle)
    cases = [cover_pair_ref.grid_case(oracle, i) for i in range(len(cover_pair_ref.GRID))]
    for i, c in enumerate(cases):
        g = _greedy2(oracle, i)
        # the exact pair is at least greedy's two, whenever greedy places two
        if g["n_selected"] == 2:
            assert c["pair_gain"] >= int(g["gain"][0]) + int(g["gain"][1]), i
        assert c["base_covered"] == g["base_covered"] and c["roi_points"] == g["roi_points"]
        # the first round of greedy is the best single
        if g["n_selected"] >= 1:
            assert c["best_single"] == g["selected"][0] and c["single_gain"] == g["gain"][0]
    # on cover_ref's own rows greedy's first two are the exact pair: the boxes are needed
    for i in range(cover_pair_ref.N_COVER_GRID):
        g = _greedy2(oracle, i)
        assert sorted(g["selected"].tolist()) == cases[i]["best_pair"].tolist(), i
    # row 70 duplicates row 35: the first maximum is the lower copy, and a pair of the two copies
    # adds nothing to either
    one = cases[cover_pair_ref.GRID.index(("seen35", 0.0, ()))]
    assert one["best_single"] == cover_ref.TIE_ROW and one["n_selected"] == 1
    assert one["pair_gain"] == one["single_gain"] == inst["seen"][cover_ref.TIE_ROW].size
    none = cases[cover_pair_ref.GRID.index(("nobody", 0.0, ()))]
    assert none["n_selected"] == 0 and none["roi_points"] > 0 and none["best_pair"].tolist() == [0, 1]
    assert none["pair_gain"] == 0 and none["best_single"] == 0
    assert (none["point_owner"] == cover_ref.OWNER_NONE).all()
    # a separation that removes pairs, fixed sensors that remove poses
    assert any((c["single_gains"] < 0).any() for c in cases)
    sep_case = cases[1]
    assert ((sep_case["pair_gains"] < 0) & np.triu(np.ones((71, 71), bool), 1)).any()


@pytest.mark.parametrize("mutant", cover_pair_ref.MUTANTS)
def test_grid_rejects_the_mutant(oracle, mutant):
    """Each wrong implementation changes an output on at least one case of the grid."""
    differs = []
    for i in range(len(cover_pair_ref.GRID)):
        ref = cover_pair_ref.grid_case(oracle, i)
        bad = cover_pair_ref.grid_case(oracle, i, mutant)
        try:
            cover_pair_ref.assert_pair_equal(bad, ref)
            differs.append(False)
        except AssertionError:
            differs.append(True)
    print(mutant, differs)
    assert any(differs), mutant
