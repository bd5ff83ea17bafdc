"""tests/triple_ref.py (the NumPy restatement of pcp_place_triple's definition, the checker of the
GPU tests) on the CPU: against a plain Python loop of the header's text on small random matrices,
against pair_ref with the first sensor fixed, and on the oracle's matrix of the 91-candidate tick
against the values the exact triple search was specified with."""
import math

import numpy as np
import pair_ref
import pytest
import refine_ref
import triple_ref
from test_pair_ref import loops as pair_loops
from test_place_sensors import greedy


def loops(S, Z, xy, fixed, sep):
    """include/pcp_abi.h's definition of pcp_place_triple, one scalar at a time (steps 1 to 4:
    test_pair_ref.loops, pcp_place_pair's definition)."""
    P, C = len(S), len(Z)
    ninf = -math.inf
    pr = pair_loops(S, Z, xy, fixed, sep)

    def smax(a, b):
        return b if a < b else a

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
    adm = [p not in fixed and not (sep > 0 and any(close(p, f) for f in fixed)) for p in range(P)]
    out = {k: pr[k] for k in ("base_total", "base_covered", "best_single", "single_total",
                              "single_covered", "best_pair", "pair_total", "pair_covered")}
    T3 = [[[ninf] * P for _ in range(P)] for _ in range(P)]
    ft, fp = [ninf] * P, [[-1, -1] for _ in range(P)]
    bt, btt, btc = (-1, -1, -1), ninf, 0
    for a in range(P):
        for b in range(a + 1, P):
            for c in range(b + 1, P):
                if not (adm[a] and adm[b] and adm[c]):
                    continue
                if sep > 0 and (close(a, b) or close(a, c) or close(b, c)):
                    continue
                t, n = 0.0, 0
                for k in range(C):
                    x = smax(smax(smax(base[k], S[a][k]), S[b][k]), S[c][k])
                    if x > 0:
                        t += x
                        n += 1
                T3[a][b][c] = t
                if t > ft[a]:
                    ft[a], fp[a] = t, [b, c]
                if t > btt:
                    bt, btt, btc = (a, b, c), t, n
    out.update(triple_totals=T3, first_totals=ft, first_partners=fp, best_triple=bt,
               triple_total=btt, triple_covered=btc)
    T, chosen = out["base_total"], []
    if out["best_single"] >= 0 and out["single_total"] > T:
        T, chosen = out["single_total"], [out["best_single"]]
    if out["best_pair"][0] >= 0 and out["pair_total"] > T:
        T, chosen = out["pair_total"], list(out["best_pair"])
    if bt[0] >= 0 and btt > T:
        chosen = list(bt)
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
    for k in ("base_covered", "best_single", "single_covered", "pair_covered", "triple_covered",
              "n_selected"):
        assert ref[k] == lo[k], k
    assert tuple(ref["best_pair"]) == tuple(lo["best_pair"])
    assert tuple(ref["best_triple"]) == tuple(lo["best_triple"])
    for k in ("base_total", "single_total", "pair_total", "triple_total", "first_totals",
              "triple_totals", "cell_score"):
        want = np.array(lo[k], np.float64).reshape(np.shape(ref[k]))   # (P = 0: empty lists)
        np.testing.assert_array_equal(_bits(ref[k]), _bits(want), err_msg=k)
    np.testing.assert_array_equal(ref["first_partners"],
                                  np.array(lo["first_partners"], np.int64).reshape(-1, 2))
    np.testing.assert_array_equal(ref["cell_owner"], np.array(lo["cell_owner"], np.int32))


def _random(seed, nf):
    rng = np.random.default_rng(100 * nf + seed)
    P, C = int(rng.integers(nf + 1, 10)), int(rng.integers(1, 12))
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
    return S, Z, xy, fixed


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("nf", [0, 1, 2, 3])
def test_restatement_against_loops(seed, nf):
    """Random small matrices (P <= 9, C <= 11) with zero and negative scores, exact duplicate rows
    and coarse half-integer values, every fixed length 0..3, with and without a separation that
    bites."""
    S, Z, xy, fixed = _random(seed, nf)
    for sep in (0.0, -1.0, 1.5, 3.0):
        _same(triple_ref.place_triple(S, Z, xy, fixed, sep), loops(S, Z, xy, fixed, sep))


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("nf", [0, 2])
def test_first_sensor_fixed_is_the_pair_search(seed, nf):
    """t[a][b][c] is, bit for bit, the pair total of (b, c) with pose a appended to the fixed
    sensors: the same fold in the same order."""
    S, Z, xy, fixed = _random(seed, nf)
    P = S.shape[0]
    for sep in (0.0, 1.5):
        r = triple_ref.place_triple(S, Z, xy, fixed, sep)
        adm = np.isfinite(r["single_totals"])
        for a in range(P):
            if not adm[a]:
                assert not np.isfinite(r["triple_totals"][a]).any()
                continue
            pr = pair_ref.place_pair(S, Z, xy, fixed + [a], sep)
            # (with a fixed, its partners below a are admissible pairs there; the triples' are
            # only those above a)
            want = pr["pair_totals"].copy()
            want[:a + 1, :] = -np.inf
            np.testing.assert_array_equal(_bits(r["triple_totals"][a]), _bits(want))


def test_restatement_edges():
    Z = np.array([0.5, 0.0])
    for n in (0, 1, 2):
        S = np.array([[1.0, -1.0], [0.25, 2.0]])[:n].reshape(n, 2)
        r = triple_ref.place_triple(S, Z, np.zeros((n, 2)))
        assert tuple(r["best_triple"]) == (-1, -1, -1) and r["triple_total"] == -np.inf
        assert r["triple_covered"] == 0 and r["n_selected"] == n and r["n_triples"] == 0
        assert r["triple_totals"].shape == (n, n, n) and not np.isfinite(r["triple_totals"]).any()
        assert (r["first_partners"] == -1).all() and not np.isfinite(r["first_totals"]).any()
        _same(r, loops(S.tolist(), Z.tolist(), np.zeros((n, 2)).tolist(), [], 0.0))
    S = np.array([[1.0, -1.0], [0.25, 2.0], [0.0, 3.0]])
    r = triple_ref.place_triple(S, Z, np.zeros((3, 2)))
    assert tuple(r["best_triple"]) == (0, 1, 2) and r["triple_total"] == 4.0
    assert r["n_triples"] == 1 and r["triple_covered"] == 2
    # the pair (0, 2) reaches 4.0 as well: the triple does not beat it, the answer is the pair
    assert tuple(r["best_pair"]) == (0, 2) and r["n_selected"] == 2
    assert r["first_partners"].tolist() == [[1, 2], [-1, -1], [-1, -1]]
    # a separation that leaves pairs and no triple
    xy = np.array([[0.0, 0.0], [3.0, 0.0], [0.5, 0.0]])
    r = triple_ref.place_triple(S, Z, xy, sep=1.0)
    assert tuple(r["best_triple"]) == (-1, -1, -1) and r["n_pairs"] == 2


@pytest.fixture(scope="module")
def tick(oracle, scene, cells, aux):
    """The oracle's matrix of the 91-candidate tick (as tests/test_pair_ref.py's)."""
    T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
    poses = oracle.generate_candidates(T, cells.grid_bbox, oracle.vl_params(), scene.zx120_pose5)
    assert poses.shape == (91, 5) and cells.xyz.shape[0] == 3704
    S, Z = oracle.score_matrix(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                               oracle.vl_params())
    return S, Z, poses[:, :2]


def _rel(a, b):
    assert abs(a - b) <= 1e-9 * abs(b), (a, b)


# fixed, sep -> triples, best triple, its total, its covered, more than this above the runner-up,
# n_selected
TICK = [
    ([], 0.0, 121485, (40, 41, 48), 4371.431464867334, 3447, 128.8, 3),
    ([], 2.0, 92306, (32, 41, 48), 4236.486666692474, 3419, 7.9, 3),
    ([], 5.0, 18009, (15, 48, 52), 3388.9776728675897, 3079, 7.2, 3),
    ([], 8.0, 464, (23, 81, 90), 2349.824310488472, 2491, 6.4, 1),
    ([40], 0.0, 117480, (32, 41, 48), 4511.981947299196, 3535, 15.3, 3),
    ([40], 2.0, 71545, (24, 41, 56), 4328.50963844578, 3503, 4.3, 3),
    ([41, 48], 2.0, 54291, (24, 32, 66), 4396.861797066253, 3574, 3.0, 3),
    ([40, 41, 48, 3], 5.0, 5, (8, 81, 87), 4393.310044155941, 3488, 6.6, 3),
]


@pytest.fixture(scope="module")
def tick_refs(tick):
    """The restatement on the tick, once per row of TICK."""
    S, Z, xy = tick
    return {(tuple(f), s): triple_ref.place_triple(S, Z, xy, f, s) for f, s, *_ in TICK}


@pytest.mark.parametrize("fixed,sep,n_triples,triple,ttot,tcov,gap,nsel", TICK)
def test_tick_values(tick_refs, fixed, sep, n_triples, triple, ttot, tcov, gap, nsel):
    r = tick_refs[(tuple(fixed), sep)]
    assert r["n_triples"] == n_triples
    assert tuple(r["best_triple"]) == triple
    _rel(r["triple_total"], ttot)
    assert r["triple_covered"] == tcov and r["n_selected"] == nsel
    t = triple_ref.triple_values(r)
    assert t[0] == r["triple_total"] and t[0] - t[1] > gap
    assert triple_ref.runner_up_gap(r) > 0.1   # nothing is decided by ulps
    if nsel == 1:   # at 8 m the best triple loses to pose 40 alone
        assert r["best_single"] == 40
        _rel(r["single_total"], 3273.1249820026733)
        assert r["triple_total"] < r["pair_total"] < r["single_total"]
    if len(fixed) == 4:   # the triple beats the pair's 4392.9659 by 0.34
        _rel(r["pair_total"], 4392.965922154437)
        assert 0.3 < r["triple_total"] - r["pair_total"] < 0.4


@pytest.mark.parametrize("sep,three,gtot,gain", [(2.0, [40, 41, 56], 4228.4994, 7.0),
                                                 (5.0, [40, 77, 27], 3381.6737, 7.0)])
def test_tick_greedy_is_exchange_optimal_and_not_best(tick, tick_refs, sep, three, gtot, gain):
    """With a separation greedy's three sensors admit no single move (pcp_place_refine's
    definition) and the exact triple is still more than 7 better: two sensors move together."""
    S, Z, xy = tick
    g = greedy(S, Z, xy, 3, sep)
    assert g["selected"].tolist() == three
    assert abs(g["total_after"][2] - gtot) < 1e-3
    f = refine_ref.place_refine(S, Z, xy, three, sep=sep)
    assert f["n_moves"] == 0 and f["selected"].tolist() == three
    r = tick_refs[((), sep)]
    assert r["triple_total"] - g["total_after"][2] > gain
    assert len(set(three) & set(r["best_triple"].tolist())) <= 1


def test_tick_without_separation_greedy_is_the_best_triple(tick, tick_refs):
    S, Z, xy = tick
    g = greedy(S, Z, xy, 3)
    r = tick_refs[((), 0.0)]
    assert sorted(g["selected"].tolist()) == r["best_triple"].tolist() == [40, 41, 48]
    assert _bits(g["total_after"][2])[0] == _bits(r["triple_total"])[0]
