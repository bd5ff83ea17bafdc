"""pcp_place_coverage at the C ABI boundary, without a GPU: the header declares the four functions,
the limit and the struct, the binding mirrors them (size and offsets included), the library
exports them, the ABI version and the kernel ids are unchanged, and a call without a context is
refused with nothing written."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("pcp_place_coverage", "pcp_place_coverage_mounted", "pcp_place_coverage_burst",
         "pcp_place_coverage_mounted_burst")


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


def test_header_declares_place_coverage():
    tail = ["cp", "roi", "roi_n", "selected", "gain", "covered_after", "round_gains",
            "seen_points", "point_owner", "owner_cap", "n_points", "roi_points", "base_covered",
            "n_selected"]
    level = _prototype_args("pcp_place_coverage")
    assert level[0].replace(" ", "") == "pcp_ctx*ctx" and len(level) == 18
    assert _arg_names(level) == ["ctx", "poses5", "n", "fan"] + tail
    assert "const pcp_cover_params *cp" in level[4] and "const uint8_t *roi" in level[5]
    mounted = _prototype_args("pcp_place_coverage_mounted")
    assert _arg_names(mounted) == ["ctx", "poses6", "n", "fan", "el_table"] + tail
    burst = _prototype_args("pcp_place_coverage_burst")
    assert _arg_names(burst) == ["ctx", "poses5", "n", "fan", "cp", "roi", "roi_n", "reps", "ms"]
    assert burst[-1] == "double ms[3]"
    mburst = _prototype_args("pcp_place_coverage_mounted_burst")
    assert _arg_names(mburst) == ["ctx", "poses6", "n", "fan", "el_table", "cp", "roi", "roi_n",
                                  "reps", "ms"]
    assert _define("PCP_COVER_MAX_POSES") == 1024 == _abi.COVER_MAX_POSES
    # additive: the version stays, and the rounds have no kernel id of their own
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15


def test_struct_layout():
    """pcp_cover_params as the header lays it out: four int32 (two of them reserved), a double,
    sixteen int64 -- 152 bytes, no padding."""
    body = re.search(r"typedef struct pcp_cover_params\s*\{(.*?)\}\s*pcp_cover_params;", CODE,
                     flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", body)
    names = [re.match(r"\s*(\w+)", decl).group(1) for _, decl in fields]
    assert names == [f[0] for f in _abi.CoverParams._fields_] == [
        "k_max", "n_fixed", "reserved", "min_separation", "fixed"]
    assert _define("PCP_PLACE_MAX") == _abi.PLACE_MAX == 16
    assert C.sizeof(_abi.CoverParams) == 152
    off = {k: getattr(_abi.CoverParams, k).offset for k in names}
    assert off == {"k_max": 0, "n_fixed": 4, "reserved": 8, "min_separation": 16, "fixed": 24}
    assert _abi.CoverParams.reserved.size == 8 and "reserved[2]" in body
    assert _abi.OWNER_NONE == _define("PCP_OWNER_NONE") == -2


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
        assert len(getattr(lib, name).argtypes) == len(_prototype_args(name))
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    p = inspect.signature(_abi.Context.place_coverage).parameters
    for k in ("poses5", "fan", "k_max", "min_separation", "fixed", "roi", "want_round_gains",
              "want_owner", "reserved"):
        assert k in p, k
    p = inspect.signature(_abi.Context.place_coverage_mounted).parameters
    assert "poses6" in p and "el_table" in p
    assert "reps" in inspect.signature(_abi.Context.place_coverage_burst).parameters
    assert "reps" in inspect.signature(_abi.Context.place_coverage_mounted_burst).parameters


def test_null_context_is_refused():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    for n in (0, 3, _abi.COVER_MAX_POSES + 1):
        cp = _abi.CoverParams(2, 0, (C.c_int32 * 2)(0, 0), 0.0)
        sel = (C.c_int64 * 16)(*[-7] * 16)
        gain, cov = (C.c_uint64 * 16)(*[7] * 16), (C.c_uint64 * 16)(*[7] * 16)
        npts, rpts, base = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        ns = C.c_int32(-7)
        tail = (C.byref(cp), None, 0, sel, gain, cov, None, None, None, 0, C.byref(npts),
                C.byref(rpts), C.byref(base), C.byref(ns))
        assert lib.pcp_place_coverage(None, None, n, C.byref(fan), *tail) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_mounted(None, None, n, C.byref(fan), None,
                                              *tail) == _abi.PCP_E_INVALID
        assert list(sel) == [-7] * 16 and list(gain) == [7] * 16 and list(cov) == [7] * 16
        assert npts.value == rpts.value == base.value == 7 and ns.value == -7
        ms = (C.c_double * 3)(-7.0, -7.0, -7.0)
        assert lib.pcp_place_coverage_burst(None, None, n, C.byref(fan), C.byref(cp), None, 0, 3,
                                            ms) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_mounted_burst(None, None, n, C.byref(fan), None,
                                                    C.byref(cp), None, 0, 3,
                                                    ms) == _abi.PCP_E_INVALID
        assert list(ms) == [-7.0] * 3
