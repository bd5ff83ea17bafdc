"""tests/cover_refine_ref.py, the NumPy restatement of pcp_place_coverage_refine, without a GPU:
against an independent search on Python sets, the rows of DESIGN.md section 6o's table (start, each
move, each covered count, the final set), the edges of the definition, and the case grid's power to
tell eight wrong implementations from the definition."""
import cover_pair_ref
import cover_ref
import cover_refine_ref
import numpy as np
import pytest


def _set_refine(seen, xy, N, start, n_locked, max_moves, sep, roi):
    """The definition on Python sets and scalar loops."""
    n = len(seen)
    S = [set(int(i) for i in q) for q in seen]
    R = set(range(N)) if roi is None else {i for i in range(N) if roi[i]}
    s = list(start)
    k = len(s)

    def near(a, b):
        dx, dy = xy[a][0] - xy[b][0], xy[a][1] - xy[b][1]
        return sep > 0 and dx * dx + dy * dy < sep * sep

    def cover(poses):
        got = set()
        for p in poses:
            got |= S[p]
        return len(got & R)

    T = start_T = cover(s)
    moves, tables = [], []
    converged = 0
    while True:
        table = [[-1] * n for _ in range(k)]
        best, bi, bp = -1, -1, -1
        for i in range(n_locked, k):
            rest = s[:i] + s[i + 1:]
            for p in range(n):
                if p in s or any(near(p, q) for q in rest):
                    continue
                table[i][p] = cover(rest + [p])
                if table[i][p] > best:
                    best, bi, bp = table[i][p], i, p
        tables.append(table)
        if bi < 0 or best <= T:
            converged = 1
            break
        if len(moves) >= max_moves:
            break
        moves.append((bi, s[bi], bp, best))
        s[bi] = bp
        T = best
    uniq = []
    for i in range(k):
        others = set()
        for j in range(k):
            if j != i:
                others |= S[s[j]]
        uniq.append(len((S[s[i]] - others) & R))
    owner = [cover_ref.OWNER_NONE] * N
    for pt in R:
        for i in range(k):
            if pt in S[s[i]]:
                owner[pt] = i
                break
    return {"s": s, "T": T, "start_T": start_T, "moves": moves, "tables": tables,
            "converged": converged, "uniq": uniq, "owner": owner, "R": len(R)}


@pytest.mark.parametrize("seed", range(12))
def test_restatement_is_the_set_search(seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(3, 30))
    N = int(rng.integers(1, 160))
    seen = [np.unique(rng.integers(0, N, int(rng.integers(0, 30)))) for _ in range(n)]
    seen[n - 1] = seen[1].copy()          # a tie
    xy = rng.integers(-3, 4, (n, 2)).astype(np.float64)   # lattice points: equalities at sep 2
    sep = [0.0, 2.0, -1.0][seed % 3]
    k = int(rng.integers(1, min(n, 6) + 1))
    start = [int(p) for p in rng.choice(n, k, replace=False)]
    n_locked = [0, min(1, k), min(2, k), k][seed % 4]
    max_moves = [16, 16, 1, 0, 3, 16][seed % 6]
    roi = None if seed % 4 == 1 else (rng.random(N) < 0.6).astype(np.uint8)
    ref = cover_refine_ref.refine(seen, xy, N, start, n_locked, max_moves, sep, roi)
    want = _set_refine(seen, xy.tolist(), N, start, n_locked, max_moves, sep, roi)
    assert ref["selected"].tolist() == want["s"]
    assert ref["covered"] == want["T"] and ref["start_covered"] == want["start_T"]
    assert ref["n_moves"] == len(want["moves"]) and ref["converged"] == want["converged"]
    got_moves = list(zip(ref["move_slot"].tolist(), ref["move_from"].tolist(),
                         ref["move_to"].tolist(), ref["move_covered"].tolist()))
    assert got_moves == want["moves"]
    assert ref["swap_covered"].tolist() == want["tables"]
    assert ref["slot_unique"].tolist() == want["uniq"]
    assert ref["point_owner"].tolist() == want["owner"]
    assert ref["roi_points"] == want["R"] and ref["n_points"] == N
    assert ref["selected"][:n_locked].tolist() == start[:n_locked]


def _run(oracle, roi, sep, start, n_locked=0, max_moves=16, mutant=None):
    inst = cover_ref.instance(oracle)
    return cover_refine_ref.refine(inst["seen"], inst["poses"][:, :2], inst["N"], start, n_locked,
                                   max_moves, sep, cover_refine_ref.rois(oracle)[roi], mutant)


@pytest.mark.parametrize("row", range(len(cover_refine_ref.TABLE)))
def test_the_table_rows(oracle, row):
    """Start, each move, each covered count and the final set of every row of the table."""
    roi, sep, start, moves, start_covered, final = cover_refine_ref.TABLE[row]
    r = _run(oracle, roi, sep, start)
    got = list(zip(r["move_slot"].tolist(), r["move_from"].tolist(), r["move_to"].tolist(),
                   r["move_covered"].tolist()))
    print(roi, sep, start, r["start_covered"], got, r["selected"].tolist(), r["covered"])
    assert r["start_covered"] == start_covered and got == moves
    assert r["selected"].tolist() == final and r["converged"] == 1
    assert r["covered"] == (moves[-1][3] if moves else start_covered)
    assert r["swap_covered"].shape == (len(moves) + 1, len(start), 71)
    # the starts the table calls greedy's are greedy's
    if start[0] != 0:
        inst = cover_ref.instance(oracle)
        g = cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], len(start), sep, (),
                             cover_refine_ref.rois(oracle)[roi])
        assert g["selected"].tolist() == start and int(g["covered_after"][-1]) == start_covered
        assert cover_refine_ref.start_set(oracle, roi, sep, len(start), "greedy") == start


def test_greedys_pair_becomes_the_exact_pair(oracle):
    for i, roi in ((cover_pair_ref.N_COVER_GRID, "box_a"), (cover_pair_ref.N_COVER_GRID + 1, "box_b")):
        exact = cover_pair_ref.grid_case(oracle, i)
        r = _run(oracle, roi, 0.0, cover_refine_ref.start_set(oracle, roi, 0.0, 2, "greedy"))
        assert sorted(r["selected"].tolist()) == exact["best_pair"].tolist()
        assert r["covered"] == exact["pair_gain"] and r["converged"] == 1


def test_edges_of_the_definition(oracle):
    # the moves run out first: one move of the first row, not converged
    r = _run(oracle, "box_a", 0.0, [51, 49], max_moves=1)
    assert r["selected"].tolist() == [43, 49] and r["covered"] == 2312
    assert r["converged"] == 0 and r["n_moves"] == 1 and r["swap_covered"].shape[0] == 2
    r = _run(oracle, "box_a", 0.0, [51, 49], max_moves=0)
    assert r["selected"].tolist() == [51, 49] and r["converged"] == 0 and r["n_moves"] == 0
    assert r["covered"] == r["start_covered"] == 2294 and r["swap_covered"].shape[0] == 1
    # k = 1 ends at the best single pose of the pair call's restatement
    for i, (roi, sep, fixed) in enumerate(cover_pair_ref.GRID):
        if fixed or roi == "nobody":
            continue
        exact = cover_pair_ref.grid_case(oracle, i)
        r = _run(oracle, roi, sep, [70])
        assert r["covered"] == exact["single_gain"], roi
        # (row 70 copies row 35: where that row is the best, the start ties with it and stays)
        want = 70 if exact["best_single"] == cover_ref.TIE_ROW else exact["best_single"]
        assert r["selected"].tolist() == [want], roi
    # a locked slot never moves
    free = _run(oracle, "all", 0.0, [0, 1, 2, 3])
    lock = _run(oracle, "all", 0.0, [0, 1, 2, 3], n_locked=2)
    assert set(free["move_slot"].tolist()) == {0, 1, 2, 3}
    assert lock["selected"][:2].tolist() == [0, 1] and set(lock["move_slot"].tolist()) <= {2, 3}
    assert (lock["swap_covered"][:, :2] == -1).all() and lock["covered"] < free["covered"]
    full = _run(oracle, "all", 0.0, [0, 1, 2, 3], n_locked=4)
    assert full["n_moves"] == 0 and full["converged"] == 1 and (full["swap_covered"] == -1).all()
    # a slot that has moved moves again
    again = _run(oracle, "all", 2.5, [0, 1, 2, 3])
    assert again["move_slot"].tolist().count(1) == 2 and again["move_slot"].tolist().count(3) == 2
    # the unique points and the owners describe the final set
    inst = cover_ref.instance(oracle)
    own = free["point_owner"]
    for i, p in enumerate(free["selected"]):
        assert np.count_nonzero(own == i) >= free["slot_unique"][i]
        assert np.isin(np.nonzero(own == i)[0], inst["seen"][p]).all()
    assert np.count_nonzero(own != cover_ref.OWNER_NONE) == free["covered"]


# the cases the mutants are tried on: the table's rows, then locked slots and a cut-off
MUTANT_CASES = [(roi, sep, start, 0, 16) for roi, sep, start, _, _, _ in cover_refine_ref.TABLE] + [
    ("all", 0.0, [0, 1, 2, 3], 2, 16), ("box", 2.5, [0, 1, 2, 3, 4, 5, 6, 7], 2, 16),
    ("xpos", 0.0, [3, 2, 1], 1, 1)]


@pytest.mark.parametrize("mutant", cover_refine_ref.MUTANTS)
def test_cases_reject_the_mutant(oracle, mutant):
    """Each wrong implementation changes an output on at least one case."""
    differs = []
    for roi, sep, start, n_locked, max_moves in MUTANT_CASES:
        ref = _run(oracle, roi, sep, start, n_locked, max_moves)
        bad = _run(oracle, roi, sep, start, n_locked, max_moves, mutant)
        try:
            cover_refine_ref.assert_refine_equal(bad, ref)
            differs.append(False)
        except AssertionError:
            differs.append(True)
    print(mutant, differs)
    assert any(differs), mutant
