"""tests/cover_weight_ref.py, the NumPy restatement of pcp_place_coverage_weighted, without a GPU:
the two identities against cover_ref.greedy, the facts of the case grid the device test leans on
(so the cases cannot go soft), an independent greedy on Python dicts, and every mutant of the
restatement told from the definition by at least one grid case."""
import cover_ref
import cover_weight_ref as wr
import numpy as np
import pytest

OUTPUTS = ("selected", "gain", "gain_points", "covered_after", "round_gains", "point_owner")
SCALARS = ("n_selected", "roi_points", "roi_weight", "base_covered", "base_points")


def _case(oracle, name, sep, fixed):
    i = next(j for j, g in enumerate(wr.GRID) if g[0] == name and g[1] == sep and g[2] == fixed)
    return i, wr.grid_case(oracle, i)


def _unit(oracle, i):
    name, sep, fixed, k = wr.GRID[i]
    region = (wr.weights(oracle)[name] != 0).astype(np.uint8)
    return wr.unit_greedy(oracle, region, sep, fixed, k)


def test_patterns_use_the_stated_bits(oracle):
    W = wr.weights(oracle)
    assert tuple(W) == wr.PATTERNS and len(wr.GRID) == 24
    for name, w in W.items():
        assert w.dtype == np.uint8 and w.shape == (cover_ref.instance(oracle)["N"],)
        assert int(np.bitwise_or.reduce(w)) == wr.USED_BITS[name], name
    assert (W["ramp"] != 0).all() and (W["ramp0"] == 0).any() and (W["x128"] == 0).any()
    assert bin(wr.USED_BITS["box200"]).count("1") == 4
    assert sorted(np.unique(W["three"]).tolist()) == [1, 10, 255]


@pytest.mark.parametrize("name,c", [("ones", 1), ("x128", 128)])
@pytest.mark.parametrize("s", range(len(wr.SETTINGS)))
def test_identities_against_the_unit_greedy(oracle, name, c, s):
    """Weights in {0, c}: cover_ref.greedy's selection on the same region, every weight-valued
    output c times it, and the points gained are its gains."""
    i = wr.PATTERNS.index(name) * len(wr.SETTINGS) + s
    got, unit = wr.grid_case(oracle, i), _unit(oracle, i)
    assert got["selected"].tolist() == unit["selected"].tolist()
    for k in ("gain", "covered_after", "round_gains"):
        u = np.asarray(unit[k]).astype(np.int64)
        want = np.where(u < 0, u, c * u)     # (-1, not alive, stays)
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), want, err_msg=k)
    np.testing.assert_array_equal(got["gain_points"], unit["gain"])
    np.testing.assert_array_equal(got["point_owner"], unit["point_owner"])
    np.testing.assert_array_equal(got["seen_points"], unit["seen_points"])
    assert got["roi_points"] == unit["roi_points"] and got["roi_weight"] == c * unit["roi_points"]
    assert got["base_covered"] == c * unit["base_covered"]
    assert got["base_points"] == unit["base_covered"]


# (pattern, sep, fixed) -> (first four selected, differs from the 0/1 greedy on R, tie rounds)
FACTS = [("ones", 0.0, (), [35, 43, 51, 25], False, 1),
         ("box200", 0.0, (), [33, 42, 34, 41], True, 1),
         ("box200", cover_ref.SEP, (), [33, 35, 50, 48], True, 1),
         ("box200", 0.0, (10, 40), [0, 33, 42, 34], True, 0),
         ("box200", cover_ref.SEP, (10, 40), [34, 50, 24, 36], True, 0),
         ("ramp", 0.0, (), [35, 43, 27, 51], True, 1),
         ("ramp0", cover_ref.SEP, (), [35, 51, 25, 49], True, 1),
         ("x128", 0.0, (), [35, 43, 51, 27], False, 2)]


@pytest.mark.parametrize("name,sep,fixed,first,differs,ties", FACTS)
def test_facts_of_the_grid(oracle, name, sep, fixed, first, differs, ties):
    i, c = _case(oracle, name, sep, fixed)
    assert c["selected"][:4].tolist() == first
    assert (c["selected"].tolist() != _unit(oracle, i)["selected"].tolist()) == differs
    assert c["tie_rounds"] == ties
    if name == "box200":   # four planes, and gains past 16 bits in round 0
        assert int(c["gain"][0]) > 213000
    if name == "ramp0":    # 15 rounds, then no pose alive or no gain
        assert c["n_selected"] == 15 and c["stopped"] in ("dead", "gain")


def test_grid_preconditions(oracle):
    cases = [wr.grid_case(oracle, i) for i in range(len(wr.GRID))]
    for c, (name, _, fixed, k) in zip(cases, wr.GRID):
        assert 2 <= c["n_selected"] <= k
        assert (c["base_covered"] > 0) == bool(fixed) == (c["base_points"] > 0)
        assert int(c["covered_after"][-1]) <= c["roi_weight"] <= 255 * c["roi_points"]
        w = wr.weights(oracle)[name].astype(np.int64)
        blind = (c["point_owner"] == wr.OWNER_NONE) & (w != 0)
        assert int(w[blind].sum()) == c["roi_weight"] - int(c["covered_after"][-1])
    # the weighted question has another answer than the 0/1 question somewhere, and not everywhere
    diff = [cases[i]["selected"].tolist() != _unit(oracle, i)["selected"].tolist()
            for i in range(len(wr.GRID))]
    assert any(diff) and not all(diff)


def _dict_greedy(seen, xy, weight, k_max, sep, fixed):
    """The definition on Python sets and a weight per point, scalar loops."""
    n, N = len(seen), len(weight)
    S = [set(int(i) for i in s) for s in seen]
    need = {i for i in range(N) if weight[i]}
    owner = [wr.OWNER_NONE] * N

    def near(a, b):
        dx, dy = xy[a][0] - xy[b][0], xy[a][1] - xy[b][1]
        return sep > 0 and dx * dx + dy * dy < sep * sep

    alive = [not (p in fixed or any(near(p, f) for f in fixed)) for p in range(n)]
    base_w = base_p = 0
    for i, f in enumerate(fixed):
        for pt in S[f] & need:
            owner[pt] = i
            base_w += int(weight[pt])
            base_p += 1
        need -= S[f]
    sel, gain, gpts, rows = [], [], [], []
    for r in range(k_max):
        if not any(alive):
            break
        g = [sum(int(weight[pt]) for pt in S[p] & need) if alive[p] else -1 for p in range(n)]
        b = max(range(n), key=lambda p: (g[p], -p))
        if g[b] <= 0:
            break
        rows.append(g)
        sel.append(b)
        gain.append(g[b])
        gpts.append(len(S[b] & need))
        for pt in S[b] & need:
            owner[pt] = len(fixed) + r
        need -= S[b]
        for p in range(n):
            if p == b or near(p, b):
                alive[p] = False
    return sel, gain, gpts, rows, owner, base_w, base_p


@pytest.mark.parametrize("seed", range(12))
def test_restatement_is_the_dict_greedy(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 90))
    N = int(rng.integers(1, 200))
    seen = [np.unique(rng.integers(0, N, int(rng.integers(0, 40)))) for _ in range(n)]
    if n > 3:
        seen[n - 1] = seen[1].copy()          # a tie
    xy = rng.integers(-3, 4, (n, 2)).astype(np.float64)
    sep = [0.0, 2.0, -1.0][seed % 3]
    fixed = tuple(int(f) for f in rng.choice(n, min(n, seed % 3), replace=False))
    weight = rng.integers(0, 256, N).astype(np.uint8)
    weight[rng.random(N) < 0.3] = 0
    if seed % 4 == 0:
        weight[:] = np.where(weight != 0, 255, 0)
    k_max = int(rng.integers(1, 17))
    ref = wr.greedy(seen, xy, weight, k_max, sep, fixed)
    sel, gain, gpts, rows, owner, base_w, base_p = _dict_greedy(seen, xy.tolist(), weight, k_max,
                                                                sep, fixed)
    assert ref["selected"].tolist() == sel and ref["gain"].tolist() == gain
    assert ref["gain_points"].tolist() == gpts and ref["round_gains"].tolist() == rows
    assert ref["covered_after"].tolist() == (base_w + np.cumsum(gain)).tolist()
    assert ref["point_owner"].tolist() == owner
    assert ref["base_covered"] == base_w and ref["base_points"] == base_p
    assert ref["roi_points"] == int(np.count_nonzero(weight))
    assert ref["roi_weight"] == int(weight.astype(np.int64).sum())


@pytest.mark.parametrize("mutant", wr.MUTANTS)
def test_grid_rejects_the_mutant(oracle, mutant):
    """Each wrong implementation changes an output the device test compares on at least one case
    of the grid."""
    differs = []
    for i in range(len(wr.GRID)):
        ref, bad = wr.grid_case(oracle, i), wr.grid_case(oracle, i, mutant)
        differs.append(any(not np.array_equal(ref[k], bad[k]) for k in OUTPUTS) or
                       any(ref[k] != bad[k] for k in SCALARS))
    assert any(differs), mutant
    if mutant.startswith("drop_bit_"):   # a dropped plane shows on a pattern that uses the bit
        b = int(mutant[-1])
        hit = {wr.GRID[i][0] for i, d in enumerate(differs) if d}
        assert hit and all((wr.USED_BITS[name] >> b) & 1 for name in hit)
