"""pcp_place_coverage_weighted at the C ABI boundary, without a GPU: the header declares the four
functions, the binding mirrors them, the library exports them, the ABI version and the kernel ids
are unchanged, and a call without a context is refused with nothing written."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("pcp_place_coverage_weighted", "pcp_place_coverage_weighted_mounted",
         "pcp_place_coverage_weighted_burst", "pcp_place_coverage_weighted_mounted_burst")


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", HEADER, flags=re.M)
    assert m, name
    return int(m.group(1))


def _prototype_args(name):
    m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", CODE, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _arg_names(args):
    return [re.search(r"(\w+)\s*(?:\[\d*\])?$", a).group(1) for a in args]


def test_header_declares_place_coverage_weighted():
    tail = ["cp", "weight", "weight_n", "selected", "gain", "covered_after", "gain_points",
            "round_gains", "seen_points", "point_owner", "owner_cap", "n_points", "roi_points",
            "roi_weight", "base_covered", "base_points", "n_selected"]
    level = _prototype_args("pcp_place_coverage_weighted")
    assert level[0].replace(" ", "") == "pcp_ctx*ctx" and len(level) == 21
    assert _arg_names(level) == ["ctx", "poses5", "n", "fan"] + tail
    assert "const pcp_cover_params *cp" in level[4] and "const uint8_t *weight" in level[5]
    assert "uint64_t *gain_points" in level[10] and "int64_t *round_gains" in level[11]
    mounted = _prototype_args("pcp_place_coverage_weighted_mounted")
    assert _arg_names(mounted) == ["ctx", "poses6", "n", "fan", "el_table"] + tail
    burst = _prototype_args("pcp_place_coverage_weighted_burst")
    assert _arg_names(burst) == ["ctx", "poses5", "n", "fan", "cp", "weight", "weight_n", "reps",
                                 "ms"]
    assert burst[-1] == "double ms[3]"
    mburst = _prototype_args("pcp_place_coverage_weighted_mounted_burst")
    assert _arg_names(mburst) == ["ctx", "poses6", "n", "fan", "el_table", "cp", "weight",
                                  "weight_n", "reps", "ms"]
    # additive: the version stays, and the rounds have no kernel id of their own
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15
    # the comment states both bounds and both identities
    doc = HEADER[HEADER.index("pcp_place_coverage with a weight per terrain point"):
                 HEADER.index("int pcp_place_coverage_weighted(")]
    for phrase in ("255 N < 2^40", "< 2^53", "{0, 1}", "{0, c}"):
        assert phrase in doc, phrase


def test_binding_and_library_hold_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s(pcp_\w+)", out))
    sigs = {s[0]: s for s in _abi._SIGS}
    lib = _abi.load_library()
    for name in NAMES:
        assert name in exported and name in _abi.ABI_SYMBOLS, name
        assert len(sigs[name][2]) == len(_prototype_args(name)), name
        assert sigs[name][1] is C.c_int
        cp_at = 5 if "mounted" in name else 4
        assert sigs[name][2][cp_at]._type_ is _abi.CoverParams
        assert sigs[name][2][3]._type_ is _abi.FanParams
        assert sigs[name][2][cp_at + 2] is C.c_uint64        # weight_n
        assert len(getattr(lib, name).argtypes) == len(_prototype_args(name))
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    p = inspect.signature(_abi.Context.place_coverage_weighted).parameters
    for k in ("poses5", "fan", "weight", "k_max", "min_separation", "fixed", "want_round_gains",
              "want_owner", "reserved"):
        assert k in p, k
    p = inspect.signature(_abi.Context.place_coverage_weighted_mounted).parameters
    assert "poses6" in p and "el_table" in p and "weight" in p
    assert "reps" in inspect.signature(_abi.Context.place_coverage_weighted_burst).parameters
    assert "reps" in inspect.signature(
        _abi.Context.place_coverage_weighted_mounted_burst).parameters


def test_null_context_is_refused():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    weight = (C.c_uint8 * 4)(1, 2, 3, 4)
    for n in (0, 3, _abi.COVER_MAX_POSES + 1):
        cp = _abi.CoverParams(2, 0, (C.c_int32 * 2)(0, 0), 0.0)
        sel = (C.c_int64 * 16)(*[-7] * 16)
        gain, cov = (C.c_uint64 * 16)(*[7] * 16), (C.c_uint64 * 16)(*[7] * 16)
        gpts = (C.c_uint64 * 16)(*[7] * 16)
        npts, rpts, rw = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        base, bpts = C.c_uint64(7), C.c_uint64(7)
        ns = C.c_int32(-7)
        tail = (C.byref(cp), weight, 4, sel, gain, cov, gpts, None, None, None, 0,
                C.byref(npts), C.byref(rpts), C.byref(rw), C.byref(base), C.byref(bpts),
                C.byref(ns))
        assert lib.pcp_place_coverage_weighted(None, None, n, C.byref(fan),
                                               *tail) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_weighted_mounted(None, None, n, C.byref(fan), None,
                                                       *tail) == _abi.PCP_E_INVALID
        for a in (gain, cov, gpts):
            assert list(a) == [7] * 16
        assert list(sel) == [-7] * 16 and ns.value == -7
        assert npts.value == rpts.value == rw.value == base.value == bpts.value == 7
        ms = (C.c_double * 3)(-7.0, -7.0, -7.0)
        assert lib.pcp_place_coverage_weighted_burst(None, None, n, C.byref(fan), C.byref(cp),
                                                     weight, 4, 3, ms) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_weighted_mounted_burst(
            None, None, n, C.byref(fan), None, C.byref(cp), weight, 4, 3,
            ms) == _abi.PCP_E_INVALID
        assert list(ms) == [-7.0] * 3


def test_weights_are_bytes():
    """The binding refuses what a byte does not hold instead of wrapping it."""
    import numpy as np
    import pytest
    w8, n = _abi.Context._weight(np.array([0, 1, 255]))
    assert w8.dtype == np.uint8 and n == 3 and w8.tolist() == [0, 1, 255]
    for bad in ([256], [-1], [0.5]):
        with pytest.raises(ValueError):
            _abi.Context._weight(np.array(bad))
    assert _abi.Context._weight(None) == (None, 0)
    w8, n = _abi.Context._weight(np.zeros(0, np.uint8))
    assert n == 0 and w8 is not None
