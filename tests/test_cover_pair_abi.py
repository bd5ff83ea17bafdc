"""pcp_place_coverage_pair at the C ABI boundary, without a GPU: the header declares the four
functions on pcp_place_pair's struct, the binding mirrors them, the library exports them, the ABI
version and the kernel ids are unchanged, and a call without a context is refused with nothing
written."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("pcp_place_coverage_pair", "pcp_place_coverage_pair_mounted",
         "pcp_place_coverage_pair_burst", "pcp_place_coverage_pair_mounted_burst")
TAIL = ["pp", "roi", "roi_n", "best_pair", "pair_gain", "best_single", "single_gain",
        "single_gains", "pair_gains", "partner", "partner_gain", "seen_points", "point_owner",
        "owner_cap", "n_points", "roi_points", "base_covered", "n_selected"]


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


def test_header_declares_place_coverage_pair():
    level = _prototype_args("pcp_place_coverage_pair")
    assert level[0].replace(" ", "") == "pcp_ctx*ctx" and len(level) == 22
    assert _arg_names(level) == ["ctx", "poses5", "n", "fan"] + TAIL
    assert "const pcp_pair_params *pp" in level[4] and "const uint8_t *roi" in level[5]
    assert level[7] == "int64_t best_pair[2]" and level[8] == "uint64_t *pair_gain"
    mounted = _prototype_args("pcp_place_coverage_pair_mounted")
    assert _arg_names(mounted) == ["ctx", "poses6", "n", "fan", "el_table"] + TAIL
    burst = _prototype_args("pcp_place_coverage_pair_burst")
    assert _arg_names(burst) == ["ctx", "poses5", "n", "fan", "pp", "roi", "roi_n", "reps", "ms"]
    assert burst[-1] == "double ms[2]"
    mburst = _prototype_args("pcp_place_coverage_pair_mounted_burst")
    assert _arg_names(mburst) == ["ctx", "poses6", "n", "fan", "el_table", "pp", "roi", "roi_n",
                                  "reps", "ms"]
    # the limit is pcp_place_coverage's, the struct pcp_place_pair's: neither is new
    assert _define("PCP_COVER_MAX_POSES") == 1024 == _abi.COVER_MAX_POSES
    assert len(re.findall(r"typedef struct pcp_pair_params\b", CODE)) == 1
    assert C.sizeof(_abi.PairParams) == 16 + 8 * _define("PCP_PLACE_MAX")
    # additive: the version stays, and the pair phase has no kernel id of its own
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15


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
        pp_at = 5 if "mounted" in name else 4
        assert sigs[name][2][pp_at]._type_ is _abi.PairParams
        assert sigs[name][2][3]._type_ is _abi.FanParams
        assert len(getattr(lib, name).argtypes) == len(_prototype_args(name))
    # owner_cap is the one integer among the outputs
    assert sigs["pcp_place_coverage_pair"][2][17] is C.c_uint64
    assert sigs["pcp_place_coverage_pair_mounted"][2][18] is C.c_uint64
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    p = inspect.signature(_abi.Context.place_coverage_pair).parameters
    for k in ("poses5", "fan", "min_separation", "fixed", "roi", "want_pair_gains", "want_owner",
              "reserved"):
        assert k in p, k
    assert "k_max" not in p
    p = inspect.signature(_abi.Context.place_coverage_pair_mounted).parameters
    assert "poses6" in p and "el_table" in p
    assert "reps" in inspect.signature(_abi.Context.place_coverage_pair_burst).parameters
    assert "reps" in inspect.signature(_abi.Context.place_coverage_pair_mounted_burst).parameters


def test_null_context_is_refused():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    for n in (0, 3, _abi.COVER_MAX_POSES + 1):
        pp = _abi.PairParams(0, 0, 0.0)
        bp = (C.c_int64 * 2)(-7, -7)
        pg, sg = C.c_uint64(7), C.c_uint64(7)
        bs = C.c_int64(-7)
        npts, rpts, base = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        ns = C.c_int32(-7)
        tail = (C.byref(pp), None, 0, bp, C.byref(pg), C.byref(bs), C.byref(sg), None, None, None,
                None, None, None, 0, C.byref(npts), C.byref(rpts), C.byref(base), C.byref(ns))
        assert lib.pcp_place_coverage_pair(None, None, n, C.byref(fan),
                                           *tail) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_pair_mounted(None, None, n, C.byref(fan), None,
                                                   *tail) == _abi.PCP_E_INVALID
        assert list(bp) == [-7, -7] and pg.value == sg.value == 7 and bs.value == -7
        assert npts.value == rpts.value == base.value == 7 and ns.value == -7
        ms = (C.c_double * 2)(-7.0, -7.0)
        assert lib.pcp_place_coverage_pair_burst(None, None, n, C.byref(fan), C.byref(pp), None,
                                                 0, 3, ms) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_pair_mounted_burst(None, None, n, C.byref(fan), None,
                                                         C.byref(pp), None, 0, 3,
                                                         ms) == _abi.PCP_E_INVALID
        assert list(ms) == [-7.0] * 2
