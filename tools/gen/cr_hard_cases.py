#!/usr/bin/env python3
"""Generates tests/golden/cr_hard_cases.npz: the arguments whose acos, scoring composite
sin(M_PI / 2 - acos(d)) and atan2 lie closest to a rounding midpoint of double -- where a
correctly rounded result is hardest to get and a wrong decision most likely to show.

A long-double screen (numpy.longdouble, the x87's 64-bit significand: 11 bits past double) over
2^24 arguments per function keeps the 2^14 whose long-double value lies nearest a midpoint; the
exact reference (tests/cr_ref.py) then measures each candidate's true distance, and the closest
2,048 per function are written with their exact results (and that distance in ulps):

    acos_d, acos_exact, acos_dist            d uniform in (0, 1)
    spa_d, spa_exact, spa_dist               the composite's sin, same d
    atan2_y, atan2_x, atan2_exact, atan2_dist   metre-scale pairs in +-60

CPU only, about two minutes.    python3 tools/gen/cr_hard_cases.py
"""
import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))

import cr_ref  # noqa: E402

N_SCREEN = 1 << 24
CHUNK = 1 << 21
N_CAND = 1 << 14
N_KEEP = 2048
LD = np.longdouble


def midpoint_dist_ld(v):
    """Distance of long-double values from the nearest double rounding midpoint, in ulps."""
    r = v.astype(np.float64)
    ulp = np.spacing(np.abs(r)).astype(LD)
    return np.abs(np.abs(v - r.astype(LD)) - ulp / 2) / ulp


def midpoint_dist_exact(v: int, prec: int) -> float:
    """The same from a fixed-point value of cr_ref (its error is ~2^-247 ulp: no matter)."""
    x = Fraction(v, 1 << prec)
    r = float(x)
    ulp = Fraction(math.ulp(r))
    return float(abs(abs(x - Fraction(r)) - ulp / 2) / ulp)


def screen(draw, value_ld):
    """The N_CAND argument tuples of N_SCREEN drawn whose long-double value is nearest a
    midpoint."""
    best_args, best_dist = None, None
    for c in range(N_SCREEN // CHUNK):
        args = draw(c)
        dist = midpoint_dist_ld(value_ld(*args))
        if best_args is not None:
            args = tuple(np.concatenate([b, a]) for b, a in zip(best_args, args))
            dist = np.concatenate([best_dist, dist])
        keep = np.argpartition(dist, N_CAND)[:N_CAND]
        best_args, best_dist = tuple(a[keep] for a in args), dist[keep]
    return best_args


def confirm(args, fixed, exact):
    """Exact distances of the candidates; the N_KEEP closest with their exact results."""
    dist = np.array([midpoint_dist_exact(*fixed(*map(float, t))) for t in zip(*args)])
    order = np.argsort(dist, kind="stable")[:N_KEEP]
    args = tuple(a[order] for a in args)
    res = [exact(*map(float, t)) for t in zip(*args)]
    assert all(v is not None for v in res), "undecided at 320 bits"
    return args, np.array(res, np.float64), dist[order]


def main():
    def draw_d(c):
        d = np.random.default_rng([20260301, c]).uniform(0.0, 1.0, CHUNK)
        return (d[(d > 2.0 ** -20) & (d < 1.0)],)

    def draw_yx(c):
        g = np.random.default_rng([20260302, c])
        return g.uniform(-60.0, 60.0, CHUNK), g.uniform(-60.0, 60.0, CHUNK)

    def spa_ld(d):
        # the double angle of the composite from the long-double acos (the exact pass redoes it)
        a = cr_ref.M_PI_2 - np.arccos(d.astype(LD)).astype(np.float64)
        return np.sin(a.astype(LD))

    def spa_fixed(d):
        return cr_ref.sin_fixed(cr_ref.M_PI_2 - cr_ref.cr_acos(d))

    out = {}
    (d,), ex, dist = confirm(screen(draw_d, lambda d: np.arccos(d.astype(LD))),
                             cr_ref.acos_fixed, cr_ref.cr_acos)
    out.update(acos_d=d, acos_exact=ex, acos_dist=dist)
    (d,), ex, dist = confirm(screen(draw_d, spa_ld), spa_fixed, cr_ref.cr_score_sin_part)
    out.update(spa_d=d, spa_exact=ex, spa_dist=dist)
    (y, x), ex, dist = confirm(screen(draw_yx, lambda y, x: np.arctan2(y.astype(LD), x.astype(LD))),
                               cr_ref.atan2_fixed, cr_ref.cr_atan2)
    out.update(atan2_y=y, atan2_x=x, atan2_exact=ex, atan2_dist=dist)
    path = ROOT / "tests" / "golden" / "cr_hard_cases.npz"
    np.savez_compressed(path, **out)
    for k in ("acos", "spa", "atan2"):
        print(k, "closest", out[k + "_dist"][0], "farthest kept", out[k + "_dist"][-1])
    print(path.name, path.stat().st_size)


if __name__ == "__main__":
    main()
