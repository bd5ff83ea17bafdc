"""Shared by tests/test_crmath_exact.py (CPU) and tests/test_device_math_gpu.py: the host (gcc)
build of pcp_crmath.h / pcp_libm.h as array functions (tests/libm/devmath_host.c), the argument
families of tests/libm/crmath_check.c, the hard-case fixture, and the exact values of
tests/cr_ref.py, computed once per argument set and cached for the session."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np

import cr_ref

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"
HARD = ROOT / "tests" / "golden" / "cr_hard_cases.npz"
N = 1 << 15             # arguments per function and family

_P = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_P)


class HostMath:
    """The gcc build of the two headers (gcc -O2 -ffp-contract=off, as tests/test_crmath.py
    builds its checker).  include_first: a directory searched before csrc (a mutated header)."""

    def __init__(self, out_dir: Path, include_first: Path | None = None, name="devmath_host"):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            import pytest
            pytest.skip("no C compiler")
        so = Path(out_dir) / f"{name}.so"
        inc = ([f"-I{include_first}"] if include_first else []) + [f"-I{CSRC}"]
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", *inc,
                        str(ROOT / "tests" / "libm" / "devmath_host.c"), "-o", str(so), "-lm"],
                       check=True)
        self.lib = C.CDLL(str(so))

    @staticmethod
    def _f64(*arrs):
        return [np.ascontiguousarray(a, np.float64) for a in arrs]

    @staticmethod
    def _f32(*arrs):
        return [np.ascontiguousarray(a, np.float32) for a in arrs]

    def score_sin_part(self, d, r0):
        d, r0 = self._f64(d, r0)
        out, ph = np.empty_like(d), np.empty(d.size, np.int32)
        self.lib.dm_score_sin_part(_p(d), _p(r0), C.c_int64(d.size), _p(out), _p(ph))
        return out, ph

    def acos_fix(self, d, r0):
        d, r0 = self._f64(d, r0)
        out = np.empty_like(d)
        self.lib.dm_acos_fix(_p(d), _p(r0), C.c_int64(d.size), _p(out))
        return out

    def cr_sin(self, a):
        a, = self._f64(a)
        out = np.empty_like(a)
        self.lib.dm_cr_sin(_p(a), C.c_int64(a.size), _p(out))
        return out

    def atan2_fix(self, y, x, r0):
        y, x, r0 = self._f64(y, x, r0)
        out = np.empty_like(y)
        self.lib.dm_atan2_fix(_p(y), _p(x), _p(r0), C.c_int64(y.size), _p(out))
        return out

    def _f32_op(self, fn, a, b=None):
        a, = self._f32(a)
        out = np.empty_like(a)
        if b is None:
            getattr(self.lib, fn)(_p(a), C.c_int64(a.size), _p(out))
        else:
            b, = self._f32(b)
            getattr(self.lib, fn)(_p(a), _p(b), C.c_int64(a.size), _p(out))
        return out

    def atan2f(self, y, x):
        return self._f32_op("dm_atan2f", y, x)

    def sinf(self, a):
        return self._f32_op("dm_sinf", a)

    def cosf(self, a):
        return self._f32_op("dm_cosf", a)

    def divf(self, a, b):
        return self._f32_op("dm_divf", a, b)

    def sqrtf(self, a):
        return self._f32_op("dm_sqrtf", a)


# ---- argument families (tests/libm/crmath_check.c's, as numpy draws) ---------------------------
def spa_families(n=N):
    """The composite's d: uniform (0, 1), (2^-20, 0.01) and (0.99, 1)."""
    g = np.random.default_rng(0xC0FFEE)
    fam = {"uniform": g.uniform(0.0, 1.0, n), "small": g.uniform(2.0 ** -20, 0.01, n),
           "near_one": g.uniform(0.99, 1.0, n)}
    return {k: v[(v > 0.0) & (v < 1.0)] for k, v in fam.items()}


def acos_family(n=N):
    g = np.random.default_rng(0xAC05)
    v = g.uniform(0.0, 1.0, n)
    return v[(v > 0.0) & (v < 1.0)]


def sin_family(n=N):
    return np.random.default_rng(0x51).uniform(2.0 ** -20, math.pi / 2, n)


def atan2_families(n=N):
    """(y, x): metre-scale pairs in +-60, ratios 2^+-40, arbitrary finite bit patterns (those
    whose angle is below 2^-900 lie outside the fix's domain and are left out), none with a zero
    argument; and `axes`, every pair with one."""
    g = np.random.default_rng(0xA7A2)
    fam = {"metres": (g.uniform(-60.0, 60.0, n), g.uniform(-60.0, 60.0, n)),
           "ratios": (g.uniform(-1.0, 1.0, n) * np.exp2(g.integers(-40, 40, n)),
                      g.uniform(-1.0, 1.0, n) * np.exp2(g.integers(-40, 40, n)))}
    bits = g.integers(0, 1 << 64, 4 * n, dtype=np.uint64).view(np.float64)
    bits = bits[np.isfinite(bits) & (bits != 0.0)]
    y, x = bits[:n], bits[n:2 * n]
    with np.errstate(all="ignore"):
        keep = np.abs(np.arctan2(y, x)) >= 2.0 ** -890
    fam["bits"] = (y[keep], x[keep])
    fam = {k: (y[(y != 0) & (x != 0)], x[(y != 0) & (x != 0)]) for k, (y, x) in fam.items()}
    # the axes: y or x = +-0 with the other finite and non-zero, in both signs (an odd candidate
    # lattice over a symmetric box produces them); the exact value is the IEEE special value
    m = min(n, 256)
    a = np.concatenate([g.uniform(-60.0, 60.0, m), g.uniform(-1.0, 1.0, m) *
                        np.exp2(g.integers(-1000, 1000, m))])
    a = a[a != 0.0]
    z = np.where(g.integers(0, 2, a.size) == 0, 0.0, -0.0)
    fam["axes"] = (np.concatenate([z, a]), np.concatenate([a, z]))
    return fam


def hard_cases():
    """tests/golden/cr_hard_cases.npz (tools/gen/cr_hard_cases.py): the arguments whose acos /
    composite / atan2 lie closest to a rounding midpoint, with their exact results."""
    return dict(np.load(HARD))


# ---- exact values, cached per argument array ---------------------------------------------------
_cache = {}


def _cached(tag, fn, *arrs):
    key = (tag,) + tuple(a.tobytes() for a in arrs)
    if key not in _cache:
        out = [fn(*map(float, t)) for t in zip(*arrs)]
        und = sum(v is None for v in out)
        _cache[key] = (np.array([math.nan if v is None else v for v in out], np.float64), und)
    return _cache[key]


def exact_acos(d):
    """(values, undecided count)"""
    return _cached("acos", cr_ref.cr_acos, np.asarray(d, np.float64))


def exact_sin(a):
    return _cached("sin", cr_ref.cr_sin, np.asarray(a, np.float64))


def exact_score_sin_part(d):
    """cr_ref.cr_score_sin_part element by element, through the two caches: cr_sin of the double
    M_PI / 2 - cr_acos(d)."""
    th, und_a = exact_acos(d)
    s, und_s = exact_sin(cr_ref.M_PI_2 - np.where(np.isnan(th), 0.0, th))
    return np.where(np.isnan(th), math.nan, s), und_a + und_s


def exact_atan2(y, x):
    return _cached("atan2", cr_ref.cr_atan2, np.asarray(y, np.float64), np.asarray(x, np.float64))


def bit_equal(a, b):
    """Element-wise equality of the bit patterns (so -0.0 != 0.0 and NaN == the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.view(u) == b.view(u)


def moved(v, k):
    """v moved by k ulps (k in -2 .. 2)."""
    out = np.array(v, np.float64)
    for _ in range(abs(k)):
        out = np.nextafter(out, math.inf if k > 0 else -math.inf)
    return out
