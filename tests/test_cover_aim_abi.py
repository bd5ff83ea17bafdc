"""pcp_place_coverage_aimed at the C ABI boundary, without a GPU: the header declares the four
functions, the limit and the struct, the binding mirrors them (size and offsets included), the
library exports them, the ABI version and the kernel ids are unchanged, and every refusal that
needs no context's state -- the call without a context first of all -- comes back before any
launch with nothing written."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("pcp_place_coverage_aimed", "pcp_place_coverage_aimed_mounted",
         "pcp_place_coverage_aimed_burst", "pcp_place_coverage_aimed_mounted_burst")


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


def test_header_declares_place_coverage_aimed():
    tail = ["ap", "aims", "roi", "roi_n", "selected", "selected_aim", "gain", "covered_after",
            "round_gains", "seen_points", "aim_points", "point_owner", "owner_cap", "n_points",
            "roi_points", "base_covered", "n_selected"]
    level = _prototype_args("pcp_place_coverage_aimed")
    assert level[0].replace(" ", "") == "pcp_ctx*ctx" and len(level) == 21
    assert _arg_names(level) == ["ctx", "poses5", "n", "fan"] + tail
    assert "const pcp_cover_aim_params *ap" in level[4] and "const int32_t *aims" in level[5]
    assert "int32_t *selected_aim" in level[9] and "uint32_t *aim_points" in level[14]
    mounted = _prototype_args("pcp_place_coverage_aimed_mounted")
    assert _arg_names(mounted) == ["ctx", "poses6", "n", "fan", "el_table"] + tail
    burst = _prototype_args("pcp_place_coverage_aimed_burst")
    assert _arg_names(burst) == ["ctx", "poses5", "n", "fan", "ap", "aims", "roi", "roi_n", "reps",
                                 "ms"]
    assert burst[-1] == "double ms[3]"
    mburst = _prototype_args("pcp_place_coverage_aimed_mounted_burst")
    assert _arg_names(mburst) == ["ctx", "poses6", "n", "fan", "el_table", "ap", "aims", "roi",
                                  "roi_n", "reps", "ms"]
    assert _define("PCP_COVER_AIM_MAX") == 64 == _abi.COVER_AIM_MAX
    assert _define("PCP_AIM_MAX_ROWS") == 65536 == _abi.AIM_MAX_ROWS
    assert _abi.COVER_MAX_POSES * _abi.COVER_AIM_MAX <= _abi.AIM_MAX_ROWS
    # additive: the version stays, and the rounds have no kernel id of their own
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15


def test_struct_layout():
    """pcp_cover_aim_params as the header lays it out: eight int32 (three of them reserved), a
    double, sixteen int64, sixteen int32 -- 232 bytes, no padding."""
    body = re.search(r"typedef struct pcp_cover_aim_params\s*\{(.*?)\}\s*pcp_cover_aim_params;",
                     CODE, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", body)
    names = [re.match(r"\s*(\w+)", decl).group(1) for _, decl in fields]
    assert names == [f[0] for f in _abi.CoverAimParams._fields_] == [
        "k_max", "n_aims", "n_fixed", "w_az", "w_el", "reserved", "min_separation", "fixed_pose",
        "fixed_aim"]
    assert _define("PCP_PLACE_MAX") == _abi.PLACE_MAX == 16
    assert C.sizeof(_abi.CoverAimParams) == 232
    off = {k: getattr(_abi.CoverAimParams, k).offset for k in names}
    assert off == {"k_max": 0, "n_aims": 4, "n_fixed": 8, "w_az": 12, "w_el": 16, "reserved": 20,
                   "min_separation": 32, "fixed_pose": 40, "fixed_aim": 168}
    assert _abi.CoverAimParams.reserved.size == 12 and "reserved[3]" in body
    assert "fixed_pose[PCP_PLACE_MAX]" in body and "fixed_aim[PCP_PLACE_MAX]" in body


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
        ap_at = 5 if "mounted" in name else 4
        assert sigs[name][2][ap_at]._type_ is _abi.CoverAimParams
        assert sigs[name][2][3]._type_ is _abi.FanParams
        assert len(getattr(lib, name).argtypes) == len(_prototype_args(name))
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    p = inspect.signature(_abi.Context.place_coverage_aimed).parameters
    for k in ("poses5", "fan", "w_az", "w_el", "aims", "k_max", "min_separation", "fixed", "roi",
              "want_round_gains", "want_owner", "want_aim_points", "reserved"):
        assert k in p, k
    p = inspect.signature(_abi.Context.place_coverage_aimed_mounted).parameters
    assert "poses6" in p and "el_table" in p
    assert "reps" in inspect.signature(_abi.Context.place_coverage_aimed_burst).parameters
    assert "reps" in inspect.signature(_abi.Context.place_coverage_aimed_mounted_burst).parameters
    assert callable(_abi.cover_aims)


def test_null_context_is_refused_with_nothing_written():
    """Whatever else the arguments hold -- good ones, or any of the refusals of the definition --
    a call without a context returns PCP_E_INVALID and leaves every output as it was."""
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    aims = (C.c_int32 * 4)(0, 0, 5, 1)
    variants = [dict(), dict(k_max=0), dict(n_aims=0), dict(n_aims=65), dict(w_az=0), dict(w_az=9),
                dict(w_el=3), dict(reserved=1), dict(n_fixed=17)]
    for n in (0, 3, _abi.COVER_MAX_POSES + 1):
        for v in variants:
            f = dict(k_max=2, n_aims=2, n_fixed=0, w_az=4, w_el=1, reserved=0)
            f.update(v)
            ap = _abi.CoverAimParams(f["k_max"], f["n_aims"], f["n_fixed"], f["w_az"], f["w_el"],
                                     (C.c_int32 * 3)(f["reserved"], 0, 0), 0.0)
            sel = (C.c_int64 * 16)(*[-7] * 16)
            sel_aim = (C.c_int32 * 16)(*[-7] * 16)
            gain, cov = (C.c_uint64 * 16)(*[7] * 16), (C.c_uint64 * 16)(*[7] * 16)
            npts, rpts, base = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
            ns = C.c_int32(-7)
            tail = (C.byref(ap), aims, None, 0, sel, sel_aim, gain, cov, None, None, None, None, 0,
                    C.byref(npts), C.byref(rpts), C.byref(base), C.byref(ns))
            assert lib.pcp_place_coverage_aimed(None, None, n, C.byref(fan),
                                                *tail) == _abi.PCP_E_INVALID
            assert lib.pcp_place_coverage_aimed_mounted(None, None, n, C.byref(fan), None,
                                                        *tail) == _abi.PCP_E_INVALID
            assert list(sel) == [-7] * 16 and list(sel_aim) == [-7] * 16
            assert list(gain) == [7] * 16 and list(cov) == [7] * 16
            assert npts.value == rpts.value == base.value == 7 and ns.value == -7
            ms = (C.c_double * 3)(-7.0, -7.0, -7.0)
            assert lib.pcp_place_coverage_aimed_burst(None, None, n, C.byref(fan), C.byref(ap),
                                                      aims, None, 0, 3, ms) == _abi.PCP_E_INVALID
            assert lib.pcp_place_coverage_aimed_mounted_burst(
                None, None, n, C.byref(fan), None, C.byref(ap), aims, None, 0, 3,
                ms) == _abi.PCP_E_INVALID
            assert list(ms) == [-7.0] * 3
