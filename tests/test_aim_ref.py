"""tests/aim_ref.py (the NumPy restatement of pcp_place_aimed's definition, the checker of the GPU
tests) on the CPU: against a plain Python scalar loop on small random inputs, on the oracle's
matrix of the 91-candidate tick against the values the call was specified with, and three mutants
of the restatement that these checks must catch."""
import math

import aim_ref
import numpy as np
import pair_ref
import pytest
from test_place_sensors import greedy


def loops(S, Z, poses5, cells, aims, h_fov, v_fov, k_max, fixed, sep):
    """include/pcp_abi.h's definition of pcp_place_aimed, one scalar at a time."""
    P, C, A = len(S), len(Z), len(aims)
    ninf = -math.inf

    def fcos(x):
        return math.cos(x) if math.isfinite(x) else math.nan

    def fsin(x):
        return math.sin(x) if math.isfinite(x) else math.nan

    ch = math.cos(h_fov * 0.5)
    tab = []
    for off, pitch in aims:
        lo, hi = pitch - v_fov * 0.5, pitch + v_fov * 0.5
        tab.append((math.cos(off), math.sin(off), ninf if lo <= -math.pi / 2 else math.tan(lo),
                    math.inf if hi >= math.pi / 2 else math.tan(hi)))

    def mul(a, b):   # inf * 0 = NaN, as the hardware's product
        return math.nan if (math.isinf(a) and b == 0) or (math.isinf(b) and a == 0) else a * b

    def w(p, a, c):
        px, py, pz, _, yaw = (float(v) for v in poses5[p])
        dx, dy, dz = float(cells[c][0]) - px, float(cells[c][1]) - py, float(cells[c][2]) - pz
        hyp = math.sqrt(dx * dx + dy * dy)
        cyp, syp = fcos(yaw), fsin(yaw)
        ca, sa, tlo, thi = tab[a]
        Cy = cyp * ca - syp * sa
        Sy = syp * ca + cyp * sa
        fwd = dx * Cy + dy * Sy
        H = h_fov >= 2 * math.pi or fwd >= ch * hyp
        V = (not dz < mul(tlo, hyp)) and (not dz > mul(thi, hyp))
        return float(S[p][c]) if H and V else 0.0

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
        dx, dy = poses5[i][0] - poses5[j][0], poses5[i][1] - poses5[j][1]
        return dx * dx + dy * dy < sep * sep

    base = [float(z) for z in Z]
    owner = [pair_ref.OWNER_ZX120 if z > 0 else pair_ref.OWNER_NONE for z in Z]
    for i, (p, a) in enumerate(fixed):
        for c in range(C):
            v = w(p, a, c)
            if base[c] < v:
                base[c], owner[c] = v, i
    T, bc = osum(base)
    out = {"base_total": T, "base_covered": bc}
    fp = [p for p, _ in fixed]
    alive = [p not in fp and not (sep > 0 and any(close(p, f) for f in fp)) for p in range(P)]
    sel, sela, tot, cov, tabs = [], [], [], [], []
    for r in range(k_max):
        if not any(alive):
            break
        t = [[ninf] * A for _ in range(P)]
        best, bt, bcv = (-1, -1), ninf, 0
        for p in range(P):
            for a in range(A):
                if not alive[p]:
                    continue
                t[p][a], n = osum([smax(base[c], w(p, a, c)) for c in range(C)])
                if t[p][a] > bt:
                    best, bt, bcv = (p, a), t[p][a], n
        if best[0] < 0 or not bt > T:
            break
        tabs.append(t)
        sel.append(best[0])
        sela.append(best[1])
        tot.append(bt)
        cov.append(bcv)
        T = bt
        for c in range(C):
            v = w(best[0], best[1], c)
            if base[c] < v:
                base[c], owner[c] = v, len(fixed) + r
        b = best[0]
        alive = [alive[p] and p != b and not (sep > 0 and close(p, b)) for p in range(P)]
    out.update(n_selected=len(sel), selected=sel, selected_aim=sela, total_after=tot,
               covered_after=cov, round_totals=tabs, cell_score=base, cell_owner=owner)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(ref, lo):
    assert ref["n_selected"] == lo["n_selected"] and ref["base_covered"] == lo["base_covered"]
    assert ref["selected"].tolist() == lo["selected"]
    assert ref["selected_aim"].tolist() == lo["selected_aim"]
    assert ref["covered_after"].tolist() == lo["covered_after"]
    for k in ("base_total", "total_after", "cell_score"):
        np.testing.assert_array_equal(_bits(ref[k]), _bits(np.array(lo[k], np.float64)), err_msg=k)
    n = ref["n_selected"]
    np.testing.assert_array_equal(
        _bits(ref["round_totals"]),
        _bits(np.array(lo["round_totals"], np.float64).reshape(ref["round_totals"].shape)))
    assert n == len(lo["round_totals"])
    np.testing.assert_array_equal(ref["cell_owner"], np.array(lo["cell_owner"], np.int32))


def _random_case(seed, nf):
    rng = np.random.default_rng(1000 * nf + seed)
    P, C, A = int(rng.integers(nf + 1, 7)), int(rng.integers(1, 14)), int(rng.integers(1, 6))
    S = np.abs(rng.normal(0.3, 1.0, (P, C)))
    S[rng.random((P, C)) < 0.25] = 0.0
    Z = np.abs(rng.normal(0.0, 0.6, C))
    Z[rng.random(C) < 0.3] = 0.0
    if seed % 2:
        S = np.round(S * 2) / 2   # coarse values: many exact ties between rows
    poses = np.zeros((P, 5))
    poses[:, :2] = rng.uniform(0, 4, (P, 2))
    poses[:, 2] = rng.uniform(0.5, 2.0, P)
    poses[:, 4] = rng.uniform(-4, 4, P)
    if P > 2:
        poses[P - 1] = poses[0]    # an exact duplicate pose: ties are decided by index
        S[P - 1] = S[0]
    cells = np.concatenate([rng.uniform(-1, 5, (C, 2)), rng.uniform(-1.5, 2.5, (C, 1))], axis=1)
    cells[0, :2] = poses[0, :2]    # a cell straight below / above pose 0
    aims = np.stack([rng.uniform(-3, 3, A), rng.uniform(-1.2, 0.6, A)], axis=1)
    if A > 2:
        aims[A - 1] = aims[0]      # an exact duplicate aim
    fixed = [(int(f), int(rng.integers(0, A))) for f in rng.permutation(P)[:nf]]
    return S, Z, poses, cells, aims, fixed


FOVS = [(math.radians(90), math.radians(60)), (math.radians(200), math.pi / 2),
        (2 * math.pi, math.pi), (math.radians(30), math.radians(170))]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("nf", [0, 1, 3])
def test_restatement_against_loops(seed, nf):
    S, Z, poses, cells, aims, fixed = _random_case(seed, nf)
    h, v = FOVS[seed % len(FOVS)]
    for sep in (0.0, 1.5):
        _same(aim_ref.place_aimed(S, Z, poses, cells, aims, h, v, 4, fixed, sep),
              loops(S, Z, poses, cells, aims, h, v, 4, fixed, sep))


def test_restatement_edges():
    """One pose at the origin looking along +x, 90 x 90 degrees about pitch -45 and 0."""
    poses = np.array([[0.0, 0.0, 1.0, 0.0, 0.0]])
    cells = np.array([[0.0, 0.0, 0.0],     # straight below
                      [2.0, 0.0, 1.0],     # ahead, level
                      [-2.0, 0.0, 1.0],    # behind
                      [1.0, 0.0, 0.0],     # ahead, 45 degrees down
                      [0.0, 2.0, 1.0]])    # to the left
    S = np.array([[1.0, 2.0, 4.0, 8.0, 16.0]])
    Z = np.zeros(5)
    aims = np.array([[0.0, -math.pi / 4], [0.0, 0.0], [math.pi / 2, 0.0]])
    view = aim_ref.in_view(poses, cells, aims, math.pi / 2, math.pi / 2)
    assert view[0].tolist() == [[True, True, False, True, False],     # lo = -90: the cell below
                                # dz = -hyp lies on the lower bound, and tan(-pi / 4) rounds to
                                # -0.9999999999999999: the definition puts the cell outside
                                [False, True, False, False, False],
                                [False, False, False, False, True]]
    r = aim_ref.place_aimed(S, Z, poses, cells, aims, math.pi / 2, math.pi / 2, 2)
    assert r["selected"].tolist() == [0] and r["selected_aim"].tolist() == [2]
    assert r["total_after"].tolist() == [16.0] and r["cell_owner"].tolist() == [-2, -2, -2, -2, 0]
    full = aim_ref.in_view(poses, cells, aims, 2 * math.pi, math.pi)
    assert full.all()
    nan = poses.copy()
    nan[0, 4] = math.nan
    assert not aim_ref.in_view(nan, cells, aims, math.pi / 2, math.pi).any()
    # no poses: the base alone
    r = aim_ref.place_aimed(np.zeros((0, 5)), np.array([0.5, 0, 0, 0, 0]), np.zeros((0, 5)), cells,
                            aims, 1.0, 1.0, 3)
    assert r["n_selected"] == 0 and r["base_total"] == 0.5 and r["base_covered"] == 1


@pytest.fixture(scope="module")
def tick(oracle, scene, cells, aux):
    """The oracle's matrix of the 91-candidate tick, oracle candidates, every pitch zeroed."""
    T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
    poses = oracle.generate_candidates(T, cells.grid_bbox, oracle.vl_params(), scene.zx120_pose5)
    assert poses.shape == (91, 5) and cells.xyz.shape[0] == 3704
    flat = poses.copy()
    flat[:, 3] = 0.0
    S, Z = oracle.score_matrix(T, A, cells.xyz, cells.normals, flat, scene.zx120_pose5,
                               oracle.vl_params())
    S1, _ = oracle.score_matrix(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                                oracle.vl_params())
    # on this tick the reference's own field-of-view test rejects nothing
    np.testing.assert_array_equal(_bits(S), _bits(S1))
    return S, Z, flat, cells.xyz


# h, v (degrees) -> per round ((pose, aim), runner-up gap, covered or None)
TICK = [
    (90, 60, [((32, 8), 121.5, 2679), ((40, 6), 32.7, 2986), ((33, 7), 14.6, 3243)]),
    (120, 40, [((40, 7), 24.6, None), ((48, 8), 36.9, None), ((49, 7), 18.6, None)]),
    (70, 77, [((32, 8), 2.06, None), ((56, 8), 4.92, None), ((33, 6), 13.4, None)]),
]


def _tick_checks(tick, ref=aim_ref):
    """Everything the tick pins, as one function: the mutants run it too."""
    S, Z, poses, cxyz = tick
    aims = ref.tick_aims()
    assert aims.shape == (45, 2)
    for h, v, rounds in TICK:
        view, edge = ref.in_view(poses, cxyz, aims, math.radians(h), math.radians(v),
                                 want_edge=True)
        # no membership hangs on a last-bit difference between two sets of candidate yaws
        assert edge > 1e-9, (h, v, edge)
        r = ref.place_aimed(S, Z, poses, cxyz, aims, math.radians(h), math.radians(v), 3,
                            view=view)
        assert _bits(r["base_total"])[0] == _bits(1715.3544346588476)[0]
        assert r["n_selected"] == 3
        gaps = ref.runner_up_gaps(r)
        for i, ((p, a), gap, cov) in enumerate(rounds):
            assert (int(r["selected"][i]), int(r["selected_aim"][i])) == (p, a), (h, v, i)
            assert abs(gaps[i] - gap) <= 0.05 * gap + 0.05, (h, v, i, gaps[i])   # (as quoted)
            if cov is not None:
                assert r["covered_after"][i] == cov
        if (h, v) == (90, 60):
            assert abs(r["total_after"][0] - 2766.21) < 0.005
            assert 6.0e-7 < edge < 6.5e-7


def test_tick_values(tick):
    _tick_checks(tick)


def test_tick_whole_sphere_is_greedy(tick):
    """360 x 180 degrees: every aim sees everything, all aims tie, and the rounds are
    pcp_place_sensors' -- 40, 41, 48, each with aim 0, the same totals bit for bit."""
    S, Z, poses, cxyz = tick
    aims = aim_ref.tick_aims()
    r = aim_ref.place_aimed(S, Z, poses, cxyz, aims, 2 * math.pi, math.pi, 3)
    g = greedy(S, Z, poses[:, :2], 3)
    assert r["selected"].tolist() == g["selected"].tolist() == [40, 41, 48]
    assert r["selected_aim"].tolist() == [0, 0, 0]
    np.testing.assert_array_equal(_bits(r["total_after"]), _bits(g["total_after"]))
    np.testing.assert_array_equal(r["covered_after"], g["covered_after"])
    np.testing.assert_array_equal(r["cell_owner"], g["cell_owner"])
    for i in range(3):
        np.testing.assert_array_equal(_bits(r["round_totals"][i]),
                                      _bits(np.repeat(g["round_totals"][i][:, None], 45, axis=1)))


# ---- the mutants ---------------------------------------------------------------------------


def _select_drops_base(view, s_row):
    # an out-of-view cell is marked -inf; the mutant's max turns the mark into +0.0, so the cell
    # counts for nothing instead of for the base
    return np.where(view, s_row, -np.inf)


def _last_max(t):
    if not t.size or not np.max(t) > -np.inf:
        return -1, -1
    k = t.size - 1 - int(np.argmax(t.ravel()[::-1]))
    return k // t.shape[1], k % t.shape[1]


MUTANTS = ["rotate", "drops_base", "last_max"]


@pytest.fixture
def mutant(request, monkeypatch):
    """aim_ref with one mistake built in."""
    kind = request.param
    if kind == "rotate":
        turn = aim_ref.rotate   # the aim rotated the wrong way: Sy negated
        monkeypatch.setattr(aim_ref, "rotate", lambda *q: (turn(*q)[0], -turn(*q)[1]))
    elif kind == "drops_base":
        monkeypatch.setattr(aim_ref, "select", _select_drops_base)
        saved = aim_ref.smax
        monkeypatch.setattr(aim_ref, "smax",
                            lambda a, b: np.where(np.isneginf(b), 0.0, saved(a, b)))
    else:
        monkeypatch.setattr(aim_ref, "first_max", _last_max)
    return kind


@pytest.mark.parametrize("mutant", MUTANTS, indirect=True)
def test_mutants_fail_against_the_loops(mutant):
    """Each mutant disagrees with the scalar loop on at least one of the random cases."""
    caught = 0
    for nf in (0, 1, 3):
        for seed in range(6):
            S, Z, poses, cells, aims, fixed = _random_case(seed, nf)
            h, v = FOVS[seed % len(FOVS)]
            try:
                _same(aim_ref.place_aimed(S, Z, poses, cells, aims, h, v, 4, fixed, 0.0),
                      loops(S, Z, poses, cells, aims, h, v, 4, fixed, 0.0))
            except AssertionError:
                caught += 1
    assert caught > 0, mutant


@pytest.mark.parametrize("mutant", MUTANTS, indirect=True)
def test_mutants_fail_on_the_tick(tick, mutant):
    """The rotation's sense and the kept base change the tick's pinned answer; the last maximum
    shows where all aims tie (360 x 180 degrees: aim 44 instead of aim 0)."""
    if mutant == "last_max":
        S, Z, poses, cxyz = tick
        r = aim_ref.place_aimed(S, Z, poses, cxyz, aim_ref.tick_aims(), 2 * math.pi, math.pi, 1)
        assert r["selected"].tolist() == [40] and r["selected_aim"].tolist() != [0]
        return
    with pytest.raises(AssertionError):
        _tick_checks(tick)
