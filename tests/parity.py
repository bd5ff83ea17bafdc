"""The parity bars of the scoring, at what the kernels achieve.  Shared by the GPU
parity tests and the node tests.

Totals, two bars:
  * exact (assert_totals_exact / totals_exact): 0 of the per-pose totals differ in their bits.
    Since round 6 the device rounds acos / sin correctly (pcp_crmath.h), as glibc does but for its
    rare near ties, and sums in the oracle's order: 0 of 91 totals differ on the 91-candidate
    tick and on every C5 frame, so those cases -- and the long-range cases of
    test_gpu_parity.py -- are held to it.  It fails a one-ulp error of every cell score
    (make perturb: 61 of 91 totals) and of every 8th cell's (make perturb8: 10 of 91 on the
    tick, 5 of 91 on C5 frame 0).
  * loose (assert_totals / totals_match): at most max(2, 5 %) of the totals differ, by at most
    2 ulps each.  Kept only for cases whose recorded census shows glibc near ties reaching a total
    (profiles/r04_ulp_census.log: 5 of 32 on test_excavation_area_node's small tick) and for the
    small synthetic scenes that were never censused; a case moves here from the exact bar only
    with its printed report as the reason, named below.
      (none of the exact cases has had to move)

Angles: candidate pitch / yaw bit-identical but for glibc's own near-tie misroundings, 2 of 7,090.
Cells: see CELL_DIFFER_FRAC below."""
import math

import numpy as np

TOTAL_MAX_ULPS = 2          # per total (the loose bar)
TOTAL_DIFFER_FRAC = 0.05
TOTAL_DIFFER_FLOOR = 2


def ulps(a, b) -> np.ndarray:
    """Distance in units in the last place between float64 arrays (0 = same bits; +0 / -0 equal)."""
    def key(x):
        u = np.asarray(x, np.float64).view(np.int64)
        return np.where(u < 0, np.int64(-2**63) - u, u)   # monotone in the value
    a, b = np.broadcast_arrays(np.atleast_1d(np.asarray(a, np.float64)),
                               np.atleast_1d(np.asarray(b, np.float64)))
    return np.abs(key(a).astype(object) - key(b).astype(object)).astype(np.float64)


def totals_report(got, ref) -> dict:
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = ulps(got, ref) if got.size else np.zeros(0)
    return {"n": int(got.size), "max_ulps": float(d.max()) if d.size else 0.0,
            "differ": int((d != 0).sum()),
            "allowed_differ": max(TOTAL_DIFFER_FLOOR, math.ceil(TOTAL_DIFFER_FRAC * got.size))}


def totals_match(got, ref) -> bool:
    r = totals_report(got, ref)
    return r["max_ulps"] <= TOTAL_MAX_ULPS and r["differ"] <= r["allowed_differ"]


def assert_totals(got, ref):
    r = totals_report(got, ref)
    assert r["max_ulps"] <= TOTAL_MAX_ULPS and r["differ"] <= r["allowed_differ"], r


def totals_exact(got, ref) -> bool:
    """The exact bar: every total has the oracle's bit pattern (+0 / -0 alike, no NaN)."""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return got.shape == ref.shape and totals_report(got, ref)["differ"] == 0


def assert_totals_exact(got, ref):
    r = totals_report(got, ref)
    assert r["differ"] == 0, r


ANGLE_DIFFER_MAX = 2        # candidate pitch / yaw values not bit-identical to glibc's


def assert_angles(got, ref):
    """Candidate pitch / yaw: at most ANGLE_DIFFER_MAX values differ, each by one ulp."""
    d = ulps(got, ref)
    assert d.max(initial=0) <= 1 and int((d != 0).sum()) <= ANGLE_DIFFER_MAX, \
        (int((d != 0).sum()), d.max(initial=0))


# per-cell bar (evaluateCellScore values, test_parity_bar_per_cell / the C5 frames / the
# long-range cases): glibc's near-tie misroundings leave 0.16-0.17 % of the positive cell scores
# off by 1-4 ulps (round 6, both ways, 2:1 downward; profiles/r04_ulp_census.log and the round-6
# logs); at most 0.4 % (at least 5) may differ, by at most 8 ulps each.  make perturb8 moves
# 12.5 % of the cells, make perturb all of them.
# Observed production maximum over the suite's censused cases (MI355X): 0.35 % -- 7 of 1,996
# positive cells, one ulp each, on the long-range scene at max_distance 110 with 5 poses
# (0.23 % there with 60 poses: 47 of 20,436, the largest 8 ulps); 0.16 % on the 91-candidate
# tick (106 of 66,036, <= 4 ulps) and 0.17-0.18 % on the C5 frames (<= 4 ulps).  Recomputed
# with 200-bit arithmetic, the device's value is the correctly rounded chain's in each of the
# long-range cells looked at and glibc's is the one off: the 8-ulp cell is glibc's acos one ulp
# (2^-52, acos in [1, 2)) from the correctly rounded value under a score in [0.125, 0.25), whose
# ulp is 2^-55.  The same misrounding under a score below 0.125 would show as 16 ulps: none
# occurs in the suite's scenes, and CELL_MAX_ULPS stays where it is.
CELL_MAX_ULPS = 8
CELL_DIFFER_FRAC = 0.004


def cell_bar(census: dict) -> bool:
    return (census["max_ulps"] <= CELL_MAX_ULPS
            and census["differ"] <= max(5, CELL_DIFFER_FRAC * census["positive"]))
