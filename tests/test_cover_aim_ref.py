"""tests/cover_aim_ref.py, the NumPy restatement of pcp_place_coverage_aimed, without a GPU:
against an independent greedy on Python sets, the preconditions of the case grid that the GPU
tests rely on (chosen here, on the CPU) -- every wrong implementation told from the definition, a
point hit from two disjoint windows, a point hit twice inside one window, a selected window that
wraps, bands at both ends of the fan, identical aims that tie -- and the rounding rule of
_abi.cover_aims."""
import cover_aim_ref as car
import cover_ref
import numpy as np
import pytest

from pointcloud_processor_amd import _abi


def _set_greedy(hits, xy, N, n_az, w_az, w_el, aims, k_max, sep, fixed, roi):
    """The definition on Python sets and scalar loops."""
    n, A = len(hits), len(aims)
    S = [[set() for _ in range(A)] for _ in range(n)]
    for p, (ray, pt) in enumerate(hits):
        for rid, point in zip(ray.tolist(), pt.tolist()):
            j, i = divmod(rid, n_az)
            for a, (az0, el0) in enumerate(aims):
                if (i - az0) % n_az < w_az and el0 <= j < el0 + w_el:
                    S[p][a].add(point)
    need = set(range(N)) if roi is None else {i for i in range(N) if roi[i]}
    R = len(need)
    owner = [car.OWNER_NONE] * N

    def near(a, b):
        dx, dy = xy[a][0] - xy[b][0], xy[a][1] - xy[b][1]
        return sep > 0 and dx * dx + dy * dy < sep * sep

    alive = [True] * n
    for i, (f, fa) in enumerate(fixed):
        for pt in S[f][fa] & need:
            owner[pt] = i
        need -= S[f][fa]
    for p in range(n):
        if any(p == f or near(p, f) for f, _ in fixed):
            alive[p] = False
    base = R - len(need)
    sel, sel_aim, gain, cov, rows = [], [], [], [], []
    covered = base
    for r in range(k_max):
        if not any(alive):
            break
        g = [[len(S[p][a] & need) if alive[p] else -1 for a in range(A)] for p in range(n)]
        b, ab = max(((p, a) for p in range(n) for a in range(A)),
                    key=lambda e: (g[e[0]][e[1]], -e[0], -e[1]))
        if g[b][ab] <= 0:
            break
        rows.append(g)
        sel.append(b)
        sel_aim.append(ab)
        gain.append(g[b][ab])
        covered += g[b][ab]
        cov.append(covered)
        for pt in S[b][ab] & need:
            owner[pt] = len(fixed) + r
        need -= S[b][ab]
        for p in range(n):
            if p == b or near(p, b):
                alive[p] = False
    aim_points = [[len(S[p][a]) for a in range(A)] for p in range(n)]
    return sel, sel_aim, gain, cov, rows, owner, base, R, aim_points


@pytest.mark.parametrize("seed", range(10))
def test_restatement_is_the_set_greedy(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 30))
    N = int(rng.integers(1, 150))
    n_az, n_el = int(rng.integers(3, 12)), int(rng.integers(2, 6))
    w_az, w_el = int(rng.integers(1, n_az + 1)), int(rng.integers(1, n_el + 1))
    A = int(rng.integers(1, 9))
    aims = [(int(rng.integers(0, n_az)), int(rng.integers(0, n_el - w_el + 1))) for _ in range(A)]
    if A > 2:
        aims[A - 1] = aims[0]                     # identical aims: a tie
    hits = []
    for _ in range(n):
        ray = np.sort(rng.choice(n_az * n_el, int(rng.integers(0, n_az * n_el + 1)), replace=False))
        hits.append((ray.astype(np.int64), rng.integers(0, N, ray.size).astype(np.int64)))
    xy = rng.integers(-3, 4, (n, 2)).astype(np.float64)   # lattice points: equalities at sep 2
    sep = [0.0, 2.0, -1.0][seed % 3]
    fixed = tuple((int(f), int(rng.integers(0, A)))
                  for f in rng.choice(n, min(n, seed % 3), replace=False))
    roi = None if seed % 4 == 0 else (rng.random(N) < 0.6).astype(np.uint8)
    k_max = int(rng.integers(1, 17))
    ref = car.greedy(hits, xy, N, n_az, w_az, w_el, aims, k_max, sep, fixed, roi)
    sel, sel_aim, gain, cov, rows, owner, base, R, apts = _set_greedy(
        hits, xy.tolist(), N, n_az, w_az, w_el, aims, k_max, sep, fixed, roi)
    assert ref["selected"].tolist() == sel and ref["selected_aim"].tolist() == sel_aim
    assert ref["gain"].tolist() == gain and ref["covered_after"].tolist() == cov
    assert ref["round_gains"].tolist() == rows
    assert ref["point_owner"].tolist() == owner
    assert ref["base_covered"] == base and ref["roi_points"] == R
    assert ref["n_selected"] == len(sel)
    assert ref["aim_points"].tolist() == apts
    assert ref["seen_points"].tolist() == [len(set(pt.tolist())) for _, pt in hits]


def test_the_rays_are_the_instance_of_cover_ref(oracle):
    inst = car.instance(oracle)
    assert inst["poses"].shape == (71, 5) and inst["N"] % 64 == 44
    assert (inst["fan"].n_az, inst["fan"].n_el) == (car.N_AZ, car.N_EL)
    for (ray, pt), seen in zip(inst["hits"], inst["seen"]):
        np.testing.assert_array_equal(np.unique(pt), seen)
        assert (np.diff(ray) > 0).all()


def test_tables_are_valid_and_reach_both_ends():
    sizes = sorted(len(t[2]) for t in car.TABLES.values())
    assert sizes == [1, 24, 64] and _abi.COVER_AIM_MAX == 64
    for w_az, w_el, aims in car.TABLES.values():
        assert 1 <= w_az <= car.N_AZ and 1 <= w_el <= car.N_EL
        for az0, el0 in aims:
            assert 0 <= az0 < car.N_AZ and 0 <= el0 <= car.N_EL - w_el
    for name in ("s24", "a64"):
        w_az, w_el, aims = car.TABLES[name]
        el0s = {e for _, e in aims}
        assert 0 in el0s and car.N_EL - w_el in el0s          # windows at both ends of the fan
        assert any(az0 + w_az > car.N_AZ for az0, _ in aims)   # windows past column n_az - 1
    aims = car.TABLES["a64"][2]
    assert aims[:32] == aims[32:] and len(set(aims[:32])) == 32


def test_grid_preconditions(oracle):
    inst = car.instance(oracle)
    cases = [car.grid_case(oracle, i) for i in range(len(car.GRID))]
    for c, (_, _, _, fixed, k) in zip(cases, car.GRID):
        assert 2 <= c["n_selected"] <= k                          # several rounds everywhere
        assert (c["base_covered"] > 0) == bool(fixed)
    assert any(c["stopped"] is not None and c["n_selected"] < k   # an early stop
               for c, (_, _, _, _, k) in zip(cases, car.GRID))
    # a selected window wraps past column n_az - 1
    wraps = 0
    for c, (table, *_) in zip(cases, car.GRID):
        w_az, _, aims = car.TABLES[table]
        wraps += sum(1 for a in c["selected_aim"] if 0 < aims[a][0] and aims[a][0] + w_az > car.N_AZ)
    assert wraps > 0
    # selected windows at el0 = 0 and at el0 = n_el - w_el both occur
    ends = set()
    for c, (table, *_) in zip(cases, car.GRID):
        _, w_el, aims = car.TABLES[table]
        if table != "full":
            ends |= {"lo" if aims[a][1] == 0 else "hi" if aims[a][1] == car.N_EL - w_el else "mid"
                     for a in c["selected_aim"]}
    assert {"lo", "hi"} <= ends
    # two identical aims tie and the lower index wins: in the doubled table every round ties,
    # and no round picks the copy
    for c, (table, *_) in zip(cases, car.GRID):
        if table == "a64":
            assert c["tie_rounds"] == c["n_selected"] and (c["selected_aim"] < 32).all()
            np.testing.assert_array_equal(c["round_gains"][:, :, :32], c["round_gains"][:, :, 32:])
    # some (pose, point) is hit from two disjoint windows, and some point by two rays of one
    w_az, w_el, aims = car.TABLES["s24"]
    _, cnt = car.membership(inst["hits"], car.N_AZ, w_az, w_el, aims)
    a, b = 0, 6   # (columns 0 .. 24 and 25 .. 49 of the lower band)
    assert aims[a][1] == aims[b][1] and aims[a][0] + w_az <= aims[b][0]
    assert any(((c[:, a] > 0) & (c[:, b] > 0)).any() for c in cnt)
    assert any((c > 1).any() for c in cnt)
    # and a point hit by rays inside and outside a window
    ray, pt = inst["hits"][0]
    inside = car.in_window(ray, car.N_AZ, aims[a][0], aims[a][1], w_az, w_el)
    assert np.intersect1d(pt[inside], pt[~inside]).size > 0


def test_one_full_window_is_the_coverage_greedy(oracle):
    """n_aims = 1, w_az = n_az, w_el = n_el: the restatement equals cover_ref.greedy."""
    inst = car.instance(oracle)
    for i, (table, roi, sep, fixed, k) in enumerate(car.GRID):
        if table != "full":
            continue
        got = car.grid_case(oracle, i)
        ref = cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], k, sep,
                               [f for f, _ in fixed], inst["rois"][roi])
        cover_ref.assert_cover_equal({**got, "round_gains": got["round_gains"][:, :, 0]}, ref)
        assert (got["selected_aim"] == 0).all()
        np.testing.assert_array_equal(got["aim_points"][:, 0], ref["seen_points"])
    # a full window may start anywhere: the wrap covers the circle
    full = car.greedy(inst["hits"][:8], inst["poses"][:8, :2], inst["N"], car.N_AZ, car.N_AZ,
                      car.N_EL, [(0, 0), (37, 0)], 3)
    np.testing.assert_array_equal(full["round_gains"][:, :, 0], full["round_gains"][:, :, 1])


@pytest.mark.parametrize("mutant", car.MUTANTS)
def test_grid_rejects_the_mutant(oracle, mutant):
    """Each wrong implementation changes an output on at least one case of the grid."""
    assert any(not car.same_answer(car.grid_case(oracle, i), car.grid_case(oracle, i, mutant))
               for i in range(len(car.GRID))), mutant


# ---- _abi.cover_aims: angles -> (w_az, w_el, aims) ------------------------------------------------

def test_cover_aims_rounds_to_the_nearest_column_and_ring():
    fan = _abi.fan_params(n_az=100, n_el=37)   # da = 3.6 deg, de = 170 / 37 = 4.59.. deg
    deg = np.pi / 180.0
    w_az, w_el, aims = _abi.cover_aims(fan, 90 * deg, 30 * deg, [0.0, np.pi / 2, -np.pi / 2],
                                       [0.0, -80 * deg, 80 * deg])
    assert (w_az, w_el) == (25, 7)             # 90 / 3.6 = 25; 30 / 4.59 = 6.53 -> 7
    assert aims.dtype == np.int32 and aims.shape == (9, 2)
    # yaw 0: columns -12 .. 12 -> az0 = 88 (wraps); yaw 90 deg = column 25 -> 13; -90 deg -> 63
    assert aims[:, 0].tolist() == [88] * 3 + [13] * 3 + [63] * 3
    # pitch 0 lies at ring 18 (el_min + 18.5 de = 0): rings 15 .. 21; the steep pitches are held
    # inside the fan
    assert aims[:3, 1].tolist() == [15, 0, 37 - 7]
    # yaw-major order
    assert (aims[0::3, 1] == 15).all()


def test_cover_aims_windows_are_at_least_one_by_one_and_at_most_the_fan():
    fan = _abi.fan_params(n_az=64, n_el=8)
    w_az, w_el, aims = _abi.cover_aims(fan, 1e-6, 1e-6, [0.1], [0.05])
    assert (w_az, w_el) == (1, 1)
    assert aims.tolist() == [[1, 4]]           # 0.1 rad = 1.02 columns; 0.05 rad lies in ring 4
    w_az, w_el, aims = _abi.cover_aims(fan, 7.0, 4.0, [3.0], [0.3])
    assert (w_az, w_el) == (64, 8) and aims[0, 1] == 0 and 0 <= aims[0, 0] < 64
    da = 2 * np.pi / 64
    assert [_abi.cover_aims(fan, c * da, 1.0, [0.0], [0.0])[0] for c in (2.4, 2.6, 3.4)] == [2, 3, 3]
