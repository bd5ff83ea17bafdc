"""tests/pair_ref.py (the NumPy restatement of pcp_place_pair's definition, the checker of the GPU
tests) on the CPU: against a plain Python triple loop on small random matrices, and on the
oracle's matrix of the 91-candidate tick against the values the exact search was specified with."""
import math

import numpy as np
import pair_ref
import pytest
from test_place_sensors import greedy


def loops(S, Z, xy, fixed, sep):
    """include/pcp_abi.h's definition of pcp_place_pair, one scalar at a time."""
    P, C = len(S), len(Z)
    ninf = -math.inf

    def smax(a, b):
        return b if a < b else a

    def osum(v):
        t, n = 0.0, 0
        for x in v:
            if x > 0:
                t += x
                n += 1
        return t, n

    def close(i, j):
        dx, dy = xy[i][0] - xy[j][0], xy[i][1] - xy[j][1]
        return dx * dx + dy * dy < sep * sep

    base = [float(z) for z in Z]
    owner = [pair_ref.OWNER_ZX120 if z > 0 else pair_ref.OWNER_NONE for z in Z]
    for i, f in enumerate(fixed):
        for c in range(C):
            if base[c] < S[f][c]:
                base[c] = float(S[f][c])
                owner[c] = i
    out = {}
    out["base_total"], out["base_covered"] = osum(base)
    adm = [p not in fixed and not (sep > 0 and any(close(p, f) for f in fixed)) for p in range(P)]
    st = [ninf] * P
    sc = [0] * P
    for p in range(P):
        if adm[p]:
            st[p], sc[p] = osum([smax(base[c], S[p][c]) for c in range(C)])
    bs, bst = -1, ninf
    for p in range(P):
        if st[p] > bst:
            bs, bst = p, st[p]
    out.update(single_totals=st, best_single=bs, single_total=bst,
               single_covered=sc[bs] if bs >= 0 else 0)
    T = [[ninf] * P for _ in range(P)]
    bp, bpt, bpc = (-1, -1), ninf, 0
    for a in range(P):
        for b in range(a + 1, P):
            if not (adm[a] and adm[b]) or (sep > 0 and close(a, b)):
                continue
            T[a][b], cov = osum([smax(smax(base[c], S[a][c]), S[b][c]) for c in range(C)])
            if T[a][b] > bpt:
                bp, bpt, bpc = (a, b), T[a][b], cov
    out.update(pair_totals=T, best_pair=bp, pair_total=bpt, pair_covered=bpc)
    if bp[0] >= 0 and bpt > bst:
        chosen = list(bp)
    elif bs >= 0 and bst > out["base_total"]:
        chosen = [bs]
    else:
        chosen = []
    for i, q in enumerate(chosen):
        for c in range(C):
            if base[c] < S[q][c]:
                base[c] = float(S[q][c])
                owner[c] = len(fixed) + i
    out.update(n_selected=len(chosen), cell_score=base, cell_owner=owner)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(ref, lo):
    for k in ("base_covered", "best_single", "single_covered", "pair_covered", "n_selected"):
        assert ref[k] == lo[k], k
    assert tuple(ref["best_pair"]) == tuple(lo["best_pair"])
    for k in ("base_total", "single_total", "pair_total", "single_totals", "pair_totals",
              "cell_score"):
        np.testing.assert_array_equal(_bits(ref[k]), _bits(np.array(lo[k], np.float64)), err_msg=k)
    np.testing.assert_array_equal(ref["cell_owner"], np.array(lo["cell_owner"], np.int32))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("nf", [0, 1, 2, 3])
def test_restatement_against_loops(seed, nf):
    """Random small matrices with zero and negative scores and exact duplicate rows, every fixed
    length 0..3, with and without a separation that bites."""
    rng = np.random.default_rng(100 * nf + seed)
    P, C = int(rng.integers(nf + 1, 9)), int(rng.integers(1, 12))
    S = rng.normal(0.3, 1.0, (P, C))
    S[rng.random((P, C)) < 0.25] = 0.0
    Z = rng.normal(0.0, 1.0, C)
    Z[rng.random(C) < 0.3] = 0.0
    if P > 2:
        S[P - 1] = S[0]          # exact duplicate rows: ties are decided by index
    if seed % 2:
        S = np.round(S * 2) / 2  # coarse values: many exact ties between different rows
    xy = rng.uniform(0, 4, (P, 2))
    fixed = [int(f) for f in rng.permutation(P)[:nf]]
    for sep in (0.0, -1.0, 1.5, 3.0):
        _same(pair_ref.place_pair(S, Z, xy, fixed, sep), loops(S, Z, xy, fixed, sep))


def test_restatement_edges():
    xy = np.zeros((1, 2))
    r = pair_ref.place_pair(np.array([[1.0, -1.0]]), np.array([0.5, 0.0]), xy)
    assert tuple(r["best_pair"]) == (-1, -1) and r["pair_total"] == -np.inf
    assert r["best_single"] == 0 and r["n_selected"] == 1 and r["single_total"] == 1.0
    assert r["cell_owner"].tolist() == [0, pair_ref.OWNER_NONE]
    r = pair_ref.place_pair(np.zeros((0, 2)), np.array([0.5, 0.0]), np.zeros((0, 2)))
    assert r["best_single"] == -1 and r["n_selected"] == 0 and r["base_total"] == 0.5
    # a pose that adds nothing: no single is selected, and the pair does not beat it
    r = pair_ref.place_pair(np.array([[0.25, 0.0], [0.5, 0.0]]), np.array([0.5, 0.0]),
                            np.zeros((2, 2)))
    assert r["n_selected"] == 0 and tuple(r["best_pair"]) == (0, 1) and r["best_single"] == 0


@pytest.fixture(scope="module")
def tick(oracle, scene, cells, aux):
    """The oracle's matrix of the 91-candidate tick (as tests/test_place_sensors.py's)."""
    T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
    poses = oracle.generate_candidates(T, cells.grid_bbox, oracle.vl_params(), scene.zx120_pose5)
    assert poses.shape == (91, 5) and cells.xyz.shape[0] == 3704
    S, Z = oracle.score_matrix(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                               oracle.vl_params())
    return S, Z, poses[:, :2]


def _rel(a, b):
    assert abs(a - b) <= 1e-9 * abs(b), (a, b)


# fixed, sep -> n_pairs, best pair, its total, its covered, best single, its total, n_selected
TICK = [
    ([], 0.0, 91 * 90 // 2, (41, 48), 3946.7926559254142, 3260, 40, 3273.1249820026733, 2),
    ([], 2.0, 3744, (41, 48), 3946.7926559254142, 3260, 40, 3273.1249820026733, 2),
    ([], 5.0, 2301, (15, 48), 3355.2996155682104, 3015, 40, 3273.1249820026733, 2),
    ([], 8.0, 697, (32, 90), 2835.4766599533955, None, 40, 3273.1249820026733, 1),
    ([40], 0.0, 90 * 89 // 2, (41, 48), 4371.431464867334, 3447, 41, 3930.4967484026056, 2),
    ([40], 2.0, 3175, (41, 56), 4228.499431666214, 3414, None, None, 2),
    ([41, 48], 2.0, None, (24, 32), 4331.011080135697, 3504, 32, 4236.486666692474, 2),
    ([40, 41, 48, 3], 5.0, 11, (8, 87), 4392.965922154437, 3487, 87, 4392.4229090758745, 2),
]


@pytest.mark.parametrize("fixed,sep,n_pairs,pair,ptot,pcov,single,stot,nsel", TICK)
def test_tick_values(tick, fixed, sep, n_pairs, pair, ptot, pcov, single, stot, nsel):
    S, Z, xy = tick
    r = pair_ref.place_pair(S, Z, xy, fixed, sep)
    if not fixed:
        assert 1715.354 <= r["base_total"] < 1715.355   # zx120 alone totals 1715.354...
    assert tuple(r["best_pair"]) == pair
    _rel(r["pair_total"], ptot)
    assert r["n_selected"] == nsel
    if n_pairs is not None:
        assert r["n_pairs"] == n_pairs
    if pcov is not None:
        assert r["pair_covered"] == pcov
    if single is not None:
        assert r["best_single"] == single
        _rel(r["single_total"], stot)
    # the runner-up pair is lower by the margins the search was specified with
    t = np.sort(r["pair_totals"][np.isfinite(r["pair_totals"])])[::-1]
    assert t[0] - t[1] > 0.1


def test_tick_exact_beats_greedy(tick):
    """Greedy's two sensors on the same matrix: (40, 41) at 3930.4967484026056, more than 10
    below the exact pair; under a separation of 5 m (40, 77) at 3342.1655135797490; at 8 m pose
    40 alone, and nothing adds."""
    S, Z, xy = tick
    g = greedy(S, Z, xy, 2)
    assert g["selected"].tolist() == [40, 41]
    _rel(g["total_after"][1], 3930.4967484026056)
    r = pair_ref.place_pair(S, Z, xy)
    assert r["pair_total"] - g["total_after"][1] > 10
    assert 40 not in r["best_pair"].tolist()   # no greedy start reaches it
    g5 = greedy(S, Z, xy, 2, 5.0)
    assert g5["selected"].tolist() == [40, 77]
    _rel(g5["total_after"][1], 3342.1655135797490)
    g8 = greedy(S, Z, xy, 2, 8.0)
    assert g8["selected"].tolist() == [40]
    _rel(g8["total_after"][0], 3273.1249820026733)
    # the singles are greedy's round 0, and the row of greedy's first pose is its round 1
    np.testing.assert_array_equal(_bits(r["single_totals"]), _bits(g["round_totals"][0]))
    row = np.array([r["pair_totals"][min(40, p), max(40, p)] for p in range(91) if p != 40])
    np.testing.assert_array_equal(_bits(row), _bits(np.delete(g["round_totals"][1], 40)))
