"""tests/cr_ref.py -- the exact reference of the device-math census -- is right, and bites.
CPU only.  Right: it agrees with the x87 long double (numpy.longdouble: 64-bit significand)
rounded to double wherever that value lies more than 2^-8 of a double ulp from a rounding
midpoint -- 8 long-double ulps, glibc documents at most 2 for acosl / sinl / atan2l on x86-64 --
and it holds the identities that are exact in double.  Bites: a value one ulp off is a mismatch,
and a precision too low to decide gives "undecided", never another double."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cr_ref
import devmath

LD = np.longdouble
N = 1 << 12
PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")


def _ld_rounded(v):
    """(long-double values rounded to double, mask: farther than 2^-8 ulp from a midpoint)"""
    r = v.astype(np.float64)
    ulp = np.spacing(np.abs(r)).astype(LD)
    dist = np.abs(np.abs(v - r.astype(LD)) - ulp / 2) / ulp
    return r, dist > 2.0 ** -8


def _check(name, exact, und, v_ld):
    r, clear = _ld_rounded(v_ld)
    assert und == 0, f"{name}: {und} undecided"
    assert clear.mean() > 0.98          # (2^-7 of the values lie that near a midpoint)
    bad = ~devmath.bit_equal(exact, r) & clear
    assert not bad.any(), f"{name}: {bad.sum()} of {clear.sum()} differ from the long double"


@pytest.mark.skipif(np.finfo(LD).nmant < 63, reason="no 64-bit long double on this host")
def test_acos_sin_atan2_agree_with_long_double():
    g = np.random.default_rng(7)
    d = np.concatenate([g.uniform(0.0, 1.0, N), g.uniform(0.99, 1.0, N), g.uniform(-1.0, 0.0, N),
                        g.uniform(2.0 ** -20, 0.01, N)])
    d = d[(np.abs(d) < 1.0) & (d != 0.0)]
    _check("acos", *devmath.exact_acos(d), np.arccos(d.astype(LD)))
    a = np.concatenate([g.uniform(2.0 ** -20, math.pi / 2, N), g.uniform(-4.0, 4.0, N),
                        g.uniform(0.0, 2.0 ** -8, N)])
    _check("sin", *devmath.exact_sin(a), np.sin(a.astype(LD)))
    for name, (y, x) in devmath.atan2_families(N).items():
        with np.errstate(all="ignore"):
            v = np.arctan2(y.astype(LD), x.astype(LD))
        _check("atan2 " + name, *devmath.exact_atan2(y, x), v)
    # a level sensor's |dz| << hd and the four quadrants of it
    y = g.uniform(-1e-6, 1e-6, N)
    x = g.uniform(0.1, 60.0, N) * g.choice([-1.0, 1.0], N)
    _check("atan2 level", *devmath.exact_atan2(y, x), np.arctan2(y.astype(LD), x.astype(LD)))


def test_composite_is_sin_of_the_double_difference():
    """cr_score_sin_part(d) = cr_sin(M_PI / 2 - cr_acos(d)), the subtraction in double; d = 0 and
    d = 1 included (acos exact there: 0 -> sin 0 = 0, M_PI / 2 -> 1)."""
    assert cr_ref.cr_score_sin_part(1.0) == 1.0
    assert cr_ref.cr_score_sin_part(0.0) == 0.0
    assert cr_ref.cr_acos(1.0) == 0.0 and cr_ref.cr_acos(0.0) == math.pi / 2
    g = np.random.default_rng(8)
    for d in g.uniform(0.0, 1.0, 256):
        th = cr_ref.cr_acos(float(d))
        assert cr_ref.cr_score_sin_part(float(d)) == cr_ref.cr_sin(math.pi / 2 - th)
    # a subnormal d: acos rounds to M_PI / 2, the difference is 0
    assert cr_ref.cr_score_sin_part(5e-324) == 0.0


def test_exact_identities():
    def rounded(q):
        return float(q)                             # Fraction -> double: one exact rounding
    assert rounded(PI) == math.pi and rounded(PI / 2) == math.pi / 2
    assert cr_ref.cr_atan2(1.0, 1.0) == math.pi / 4
    assert cr_ref.cr_atan2(1.0, -1.0) == rounded(3 * PI / 4)
    assert cr_ref.cr_atan2(5.0, 0.0) == math.pi / 2 and cr_ref.cr_atan2(-5.0, 0.0) == -math.pi / 2
    assert cr_ref.cr_atan2(0.0, -1.0) == math.pi and cr_ref.cr_atan2(-0.0, -1.0) == -math.pi
    z = cr_ref.cr_atan2(-0.0, 2.0)
    assert z == 0.0 and math.copysign(1.0, z) < 0
    assert cr_ref.cr_acos(0.5) == rounded(PI / 3)
    assert cr_ref.cr_acos(-0.5) == rounded(2 * PI / 3)
    assert cr_ref.cr_acos(-1.0) == math.pi
    assert cr_ref.cr_sin(0.0) == 0.0 and cr_ref.cr_sin(2.0 ** -40) == 2.0 ** -40
    # sin(pi / 6 rounded) against the series evaluated independently in rationals
    a = rounded(PI / 6)
    q, term, k = Fraction(0), Fraction(a), 0
    while abs(term) > Fraction(1, 1 << 200):
        q += term
        k += 1
        term = -term * Fraction(a) ** 2 / ((2 * k) * (2 * k + 1))
    assert cr_ref.cr_sin(a) == rounded(q)
    # odd in y / in a; atan2 over a huge exponent gap keeps its relative precision
    g = np.random.default_rng(9)
    for y, x in zip(g.uniform(-60, 60, 128), g.uniform(-60, 60, 128)):
        assert cr_ref.cr_atan2(-y, x) == -cr_ref.cr_atan2(y, x)
        assert cr_ref.cr_sin(-y / 20) == -cr_ref.cr_sin(y / 20)
    assert cr_ref.cr_atan2(1e-300, 1.0) == 1e-300
    assert cr_ref.cr_atan2(3.0 * 2.0 ** -1000, 2.0 ** 20) == 3.0 * 2.0 ** -1020
    assert cr_ref.cr_atan2(1.0, 1e-300) == math.pi / 2


def test_a_value_one_ulp_off_is_a_mismatch():
    d = devmath.spa_families(N)["uniform"]
    exact, und = devmath.exact_score_sin_part(d)
    assert und == 0
    for k in (-1, 1):
        assert not devmath.bit_equal(devmath.moved(exact, k), exact).any()
    # and the rounding is to nearest: the exact value lies within half an ulp of the result
    for dv, e in zip(d[:256], exact[:256]):
        v, prec = cr_ref.sin_fixed(math.pi / 2 - cr_ref.cr_acos(float(dv)))
        assert abs(Fraction(v, 1 << prec) - Fraction(float(e))) <= Fraction(math.ulp(float(e))) / 2


def test_too_little_precision_is_undecided_not_wrong(monkeypatch):
    """At 80 bits (an error interval of ~2^-7 ulp) the hard cases, which lie within 2^-14 ulp of
    a midpoint, are undecided; whatever is decided equals the 320-bit result."""
    h = devmath.hard_cases()
    full = [cr_ref.cr_acos(float(d)) for d in h["acos_d"][:256]]
    assert None not in full
    monkeypatch.setattr(cr_ref, "P", 80)
    low = [cr_ref.cr_acos(float(d)) for d in h["acos_d"][:256]]
    assert all(v is None for v in low)
    assert all(v is None or v == f for v, f in zip(low, full))
    g = np.random.default_rng(10)
    for d in g.uniform(0.0, 1.0, 256):
        v = cr_ref.cr_acos(float(d))
        monkeypatch.setattr(cr_ref, "P", 320)
        assert v is None or v == cr_ref.cr_acos(float(d))
        monkeypatch.setattr(cr_ref, "P", 80)
