"""pcp_crmath.h (the gcc build, as tests/test_crmath.py builds it) against the exact reference
tests/cr_ref.py: pcp_score_sin_part, pcp_cr_acos_fix, pcp_cr_sin and pcp_cr_atan2_fix return the
correctly rounded double for every argument, from first results at -1, 0 and +1 ulp of the
exact value.  No allowance: glibc's own near-tie misroundings, which tests/test_crmath.py has to
tolerate, are counted and printed here instead.  CPU only.

Arguments: the families of tests/libm/crmath_check.c, 2^15 per function and family, and the
hard cases of tests/golden/cr_hard_cases.npz (tools/gen/cr_hard_cases.py).

Measured (printed by each run): the host build's exact phase (phase 2) handles 3 of 32,768
uniform d from the exact first result (9 of 98,304 over the three first results, 9.2e-5), 7 and
9 of 32,768 in (2^-20, 0.01) and (0.99, 1), and 2,092 of the 4,096 composite hard cases; glibc
2.35 differs from the exact value on 89 of 32,768 uniform composites (acos and sin together),
39 of 32,768 acos and 39 of 32,768 sin arguments, 33 / 3 / 0 of the metre-scale / ratio /
bit-pattern atan2 pairs, 0 of the 1,024 axis pairs (one argument +-0: pcp_cr_atan2_fix returns the
IEEE special value whatever the first result).  The census found pcp_cr_atan2_fix wrong for 9 of 90,309 bit-pattern
pairs (a y next to the subnormal range: the products' low words underflowed), since fixed by
scaling both arguments by a common power of two.

The census bites (each mutant must produce mismatches):
  * first results two ulps off -- outside the fix's precondition -- make the composite wrong
    for 77 % of the arguments;
  * test_mutant_table_low_words: a copy of pcp_crmath.h whose k pi / 512 table is read without
    its low words (kPcpSinCos512[k][1] and [k][3] replaced by 0.0), which leaves phase 1's
    sin / cos good to ~2^-54 while its margins assume 2^-84: 31 % wrong."""
import math
import shutil

import numpy as np
import pytest

import devmath

FIRST = (-1, 0, 1)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return devmath.HostMath(tmp_path_factory.mktemp("devmath"))


def _census(name, fn, exact, und, first_from=None, steps=FIRST):
    """fn(first result) over first results moved by each of `steps` ulps -> mismatches."""
    assert und == 0, f"{name}: {und} undecided"
    first_from = exact if first_from is None else first_from
    bad = 0
    for k in steps:
        bad += int((~devmath.bit_equal(fn(devmath.moved(first_from, k)), exact)).sum())
    return bad


def _glibc(name, fn, exact, *args):
    """The running libm through Python's math module, one call per element (numpy's array
    functions are its own SIMD kernels, not libm)."""
    g = np.array([fn(*map(float, t)) for t in zip(*args)], np.float64)
    n_bad = int((~devmath.bit_equal(g, exact)).sum())
    print(f"glibc {name}: {n_bad} of {exact.size} differ from the exact value")
    assert n_bad < 3e-3 * exact.size          # (what tests/test_crmath.py allows; not ours)


def test_score_sin_part_exact(host):
    h = devmath.hard_cases()
    fams = dict(devmath.spa_families(), hard=np.concatenate([h["acos_d"], h["spa_d"]]))
    for name, d in fams.items():
        exact, und = devmath.exact_score_sin_part(d)
        th, und_a = devmath.exact_acos(d)
        assert und_a == 0
        bad = _census(name, lambda r0: host.score_sin_part(d, r0)[0], exact, und, first_from=th)
        assert bad == 0, f"{name}: {bad} mismatches of {3 * d.size}"
        _, ph = host.score_sin_part(d, th)
        print(f"host phase 2, {name}: {int((ph == 2).sum())} of {d.size}")
        if name != "hard":
            _glibc("sin(M_PI / 2 - acos(d)) " + name,
                   lambda v: math.sin(math.pi / 2 - math.acos(v)), exact, d)
    assert np.array_equal(np.concatenate([h["acos_exact"]]), devmath.exact_acos(h["acos_d"])[0])
    assert np.array_equal(h["spa_exact"], devmath.exact_score_sin_part(h["spa_d"])[0])
    # the edges: 0, 1, 2^-20 (phase 1's lower limit) and its neighbours, 1's lower neighbour,
    # a subnormal
    e = np.array([0.0, 1.0, 2.0 ** -20, np.nextafter(2.0 ** -20, 0), np.nextafter(2.0 ** -20, 1),
                  np.nextafter(1.0, 0), 5e-324, 2.0 ** -1030])
    exact, und = devmath.exact_score_sin_part(e)
    th, _ = devmath.exact_acos(e)
    assert und == 0 and devmath.bit_equal(host.score_sin_part(e, th)[0], exact).all()


def test_acos_fix_and_sin_exact(host):
    h = devmath.hard_cases()
    for name, d in (("uniform", devmath.acos_family()), ("hard", h["acos_d"])):
        exact, und = devmath.exact_acos(d)
        bad = _census(name, lambda r0: host.acos_fix(d, r0), exact, und)
        assert bad == 0, f"acos {name}: {bad} mismatches of {3 * d.size}"
    d = devmath.acos_family()
    _glibc("acos", math.acos, devmath.exact_acos(d)[0], d)
    a = devmath.sin_family()
    exact, und = devmath.exact_sin(a)
    assert und == 0
    bad = int((~devmath.bit_equal(host.cr_sin(a), exact)).sum())
    assert bad == 0, f"sin: {bad} mismatches of {a.size}"
    _glibc("sin", math.sin, exact, a)
    # the composite hard cases' own angles
    a = math.pi / 2 - devmath.exact_acos(h["spa_d"])[0]
    assert devmath.bit_equal(host.cr_sin(a), h["spa_exact"]).all()


def test_atan2_fix_exact(host):
    h = devmath.hard_cases()
    fams = dict(devmath.atan2_families(), hard=(h["atan2_y"], h["atan2_x"]))
    for name, (y, x) in fams.items():
        exact, und = devmath.exact_atan2(y, x)
        bad = _census(name, lambda r0: host.atan2_fix(y, x, r0), exact, und)
        assert bad == 0, f"atan2 {name}: {bad} mismatches of {3 * y.size}"
        if name != "hard":
            _glibc("atan2 " + name, math.atan2, exact, y, x)
    assert np.array_equal(h["atan2_exact"], devmath.exact_atan2(h["atan2_y"], h["atan2_x"])[0])


def test_atan2_fix_follows_first_results_four_ulps_off(host):
    """pcp_cr_atan2_fix repeats its midpoint tests from the neighbour they point to (ocml's
    atan2 is up to 1.06 ulps from the true angle, tests/test_device_math_gpu.py): first results
    2, 3 and 4 ulps off either way still give the exact value."""
    h = devmath.hard_cases()
    fams = dict(devmath.atan2_families(1 << 13), hard=(h["atan2_y"], h["atan2_x"]))
    for name, (y, x) in fams.items():
        exact, und = devmath.exact_atan2(y, x)
        bad = _census(name, lambda r0: host.atan2_fix(y, x, r0), exact, und,
                      steps=(-4, -3, -2, 2, 3, 4))
        assert bad == 0, f"atan2 {name}: {bad} mismatches of {6 * y.size}"


def test_mutant_first_result_two_ulps_off(host):
    """A first result outside the fix's precondition must show: the census is not blind to the
    first result's quality."""
    d = devmath.spa_families()["uniform"]
    exact, und = devmath.exact_score_sin_part(d)
    th, _ = devmath.exact_acos(d)
    bad = _census("two ulps", lambda r0: host.score_sin_part(d, r0)[0], exact, und,
                  first_from=th, steps=(-2, 2))
    print(f"first result +-2 ulps: {bad} of {2 * d.size} wrong")
    assert bad > 0.5 * 2 * d.size


def test_mutant_table_low_words(tmp_path):
    """The k pi / 512 table without its low words (a mutated copy of the header, searched
    first): the census must report mismatches."""
    src = (devmath.CSRC / "pcp_crmath.h").read_text()
    mut = src.replace("kPcpSinCos512[k][1]", "0.0").replace("kPcpSinCos512[k][3]", "0.0")
    assert mut != src and mut.count("kPcpSinCos512[k]") == 2
    (tmp_path / "pcp_crmath.h").write_text(mut)
    shutil.copy(devmath.CSRC / "pcp_crmath_tab.h", tmp_path)
    mutant = devmath.HostMath(tmp_path, include_first=tmp_path, name="devmath_mutant")
    d = devmath.spa_families()["uniform"]
    exact, und = devmath.exact_score_sin_part(d)
    th, _ = devmath.exact_acos(d)
    bad = _census("mutant", lambda r0: mutant.score_sin_part(d, r0)[0], exact, und, first_from=th)
    print(f"table low words zeroed: {bad} of {3 * d.size} wrong")
    assert bad > 0
