"""Exact reference for the double-precision acos / sin / atan2 this library promises bit for bit:
integer fixed point (320 fractional bits, more where an argument is tiny), every rounding to
double one exact float(Fraction).  Plain Python; no dependency beyond the standard library.

  atan    argument halving t -> t / (1 + sqrt(1 + t^2)) (math.isqrt) eight times, then the
          Taylor series; atan2 the quadrant rules over atan of the smaller ratio
  acos    atan2(sqrt(1 - d^2), d)
  sin     the Taylor series (|a| <= 8)
  pi      Machin: 16 atan(1/5) - 4 atan(1/239)

Every value carries a bound on its error (ERR_ULPS fixed-point units, a generous multiple of
what the floors of these few dozen integer operations can add up to: each floor is below one
unit, a halving step maps an error e to below 0.75 e + 1.25, the series' <= 70 terms add below
4 units each, and undoing eight halvings multiplies by 2^8 -- under 2^17 in all).  A result is
returned only when both ends of that interval round to the same double; otherwise None
("undecided"), never a wrong answer.  At 320 bits the interval is ~2^-300 of the value, so an
undecided double would have to lie within 2^-247 ulp of a rounding boundary."""
import math
from fractions import Fraction

P = 320                 # fractional bits (the least used)
ERR_ULPS = 1 << 20      # error bound of every fixed-point value, in units of 2^-prec
HALVINGS = 8
M_PI_2 = math.pi / 2    # the double M_PI / 2 of the scoring's subtraction

_pi_cache = {}


def _atan_series(t: int, prec: int) -> int:
    """atan(t / 2^prec) * 2^prec for small t (the series converges for |t| < 2^prec)."""
    t2 = (t * t) >> prec
    term, total, k = t, 0, 0
    while term:
        q = term // (2 * k + 1)
        total += -q if k & 1 else q
        term = (term * t2) >> prec
        k += 1
    return total


def _atan_fixed(num: int, den: int, prec: int) -> int:
    """atan(num / den) * 2^prec for integers 0 <= num <= den, den > 0."""
    one = 1 << prec
    t = (num << prec) // den
    for _ in range(HALVINGS):
        t = (t << prec) // (one + math.isqrt((one << prec) + t * t))
    return _atan_series(t, prec) << HALVINGS


def _pi_fixed(prec: int) -> int:
    if prec not in _pi_cache:
        g = prec + 16
        v = 16 * _atan_series((1 << g) // 5, g) - 4 * _atan_series((1 << g) // 239, g)
        _pi_cache[prec] = v >> 16
    return _pi_cache[prec]


def _half_pi_fixed(prec: int) -> int:
    return _pi_fixed(prec + 1) >> 2


def _round(v: int, prec: int):
    """The double nearest v / 2^prec if the error interval decides it, else None."""
    lo = float(Fraction(v - ERR_ULPS, 1 << prec))
    hi = float(Fraction(v + ERR_ULPS, 1 << prec))
    return lo if lo == hi else None


def _exp(x: float) -> int:
    return math.frexp(x)[1]


def _atan2_fixed(yn: int, yd: int, xn: int, xd: int):
    """atan2(yn / yd, xn / xd) for yn > 0, xn != 0 (positive denominators) -> (value, prec)."""
    num_y, num_x = yn * xd, abs(xn) * yd          # |y| / |x| = num_y / num_x
    if num_y <= num_x:
        # a small ratio makes a small angle: keep P bits below its leading one
        prec = P + max(0, num_x.bit_length() - num_y.bit_length() + 1) if xn > 0 else P
        a = _atan_fixed(num_y, num_x, prec)
        return (a if xn > 0 else _pi_fixed(prec) - a), prec
    a = _atan_fixed(num_x, num_y, P)
    return (_half_pi_fixed(P) - a if xn > 0 else _half_pi_fixed(P) + a), P


def atan2_fixed(y: float, x: float):
    """(v, prec): atan2(y, x) = (v +- ERR_ULPS) / 2^prec, for finite non-zero y and x."""
    yn, yd = abs(y).as_integer_ratio()
    xn, xd = x.as_integer_ratio()
    v, prec = _atan2_fixed(yn, yd, xn, xd)
    return (-v if y < 0 else v), prec


def cr_atan2(y: float, x: float):
    """atan2(y, x) correctly rounded (IEEE / C99 values for zeros); None when undecided."""
    if math.isnan(y) or math.isnan(x) or math.isinf(y) or math.isinf(x):
        return math.atan2(y, x)                   # (no rounding question: not this module's)
    if y == 0.0:
        if math.copysign(1.0, x) > 0:
            return y
        return math.copysign(_round(_pi_fixed(P), P), y)
    if x == 0.0:
        return math.copysign(_round(_half_pi_fixed(P), P), y)
    return _round(*atan2_fixed(y, x))


def acos_fixed(d: float):
    """(v, prec): acos(d) = (v +- ERR_ULPS) / 2^prec, for 0 < |d| < 1."""
    # d and sqrt(1 - d^2) at 2 P bits: near |d| = 1 the root is small (>= 2^-27) and must keep
    # its relative precision.  d is exact there unless |d| < 2^-587, where the floor moves acos
    # (~pi / 2) by less than one unit
    W = 2 * P
    dn, dd = abs(d).as_integer_ratio()
    D = (dn << W) // dd
    if D == 0:
        return _half_pi_fixed(P), P
    s = math.isqrt((1 << (2 * W)) - D * D)
    return _atan2_fixed(s, 1, D if d > 0 else -D, 1)


def cr_acos(d: float):
    """acos(d) correctly rounded; None when undecided."""
    if math.isnan(d) or abs(d) > 1.0:
        return math.nan
    if d == 1.0:
        return 0.0
    if d == -1.0:
        return _round(_pi_fixed(P), P)
    if d == 0.0:
        return _round(_half_pi_fixed(P), P)
    return _round(*acos_fixed(d))


def sin_fixed(a: float):
    """(v, prec): sin(a) = (v +- ERR_ULPS) / 2^prec, for 2^-30 <= |a| <= 8."""
    prec = P + max(0, 1 - _exp(a))                # a is a multiple of 2^-prec: exact below
    an, ad = abs(a).as_integer_ratio()
    t = (an << prec) // ad
    t2 = (t * t) >> prec
    term, total, k = t, 0, 0
    while term:
        total += -term if k & 1 else term
        k += 1
        term = ((term * t2) >> prec) // ((2 * k) * (2 * k + 1))
    return (-total if a < 0 else total), prec


def cr_sin(a: float):
    """sin(a) correctly rounded for |a| <= 8; None when undecided."""
    if math.isnan(a) or abs(a) > 8.0:
        raise ValueError("cr_sin: |a| <= 8")
    if abs(a) < 2.0 ** -30:
        # sin a = a (1 - a^2 / 6 + ..): the correction is below 2^-61 of a, far inside the
        # quarter-ulp (2^-54) that separates a from its nearest rounding boundary
        return a
    return _round(*sin_fixed(a))


def cr_score_sin_part(d: float):
    """evaluateCellScore's sin(M_PI / 2 - acos(d)) with both functions correctly rounded and the
    subtraction in double, as the reference computes it; None when either is undecided."""
    th = cr_acos(d)
    if th is None:
        return None
    return cr_sin(M_PI_2 - th)


def as_interval(v: int, prec: int):
    """The error interval of a fixed-point value as two Fractions."""
    return Fraction(v - ERR_ULPS, 1 << prec), Fraction(v + ERR_ULPS, 1 << prec)


def brackets(raw: float, v: int, prec: int) -> bool:
    """Whether the true value (v +- ERR_ULPS) / 2^prec lies between raw's two neighbours: the
    precondition of pcp_crmath.h's fixes ("a faithful first result")."""
    lo, hi = as_interval(v, prec)
    return (Fraction(math.nextafter(raw, -math.inf)) <= lo and
            hi <= Fraction(math.nextafter(raw, math.inf)))


def ulps_off(raw: float, v: int, prec: int) -> float:
    """|raw - true| in units of the correctly rounded value's ulp."""
    mid = Fraction(v, 1 << prec)
    return float(abs(Fraction(raw) - mid) / Fraction(math.ulp(float(mid))))
