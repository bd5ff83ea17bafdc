"""pcp_place_coverage_refine at the C ABI boundary, without a GPU: the header declares the four
functions on pcp_place_refine's struct, the binding mirrors them, the library exports them, the ABI
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
NAMES = ("pcp_place_coverage_refine", "pcp_place_coverage_refine_mounted",
         "pcp_place_coverage_refine_burst", "pcp_place_coverage_refine_mounted_burst")
TAIL = ["rp", "roi", "roi_n", "selected", "covered", "start_covered", "move_slot", "move_from",
        "move_to", "move_covered", "swap_covered", "slot_unique", "seen_points", "point_owner",
        "owner_cap", "n_points", "roi_points", "n_moves", "converged"]


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


def test_header_declares_place_coverage_refine():
    level = _prototype_args("pcp_place_coverage_refine")
    assert level[0].replace(" ", "") == "pcp_ctx*ctx" and len(level) == 23
    assert _arg_names(level) == ["ctx", "poses5", "n", "fan"] + TAIL
    assert "const pcp_refine_params *rp" in level[4] and "const uint8_t *roi" in level[5]
    assert level[7] == "int64_t *selected" and level[8] == "uint64_t *covered"
    assert level[10] == "int32_t *move_slot" and level[13] == "uint64_t *move_covered"
    assert level[14] == "int64_t *swap_covered" and level[15] == "uint64_t *slot_unique"
    assert level[18] == "uint64_t owner_cap" and level[22] == "int32_t *converged"
    mounted = _prototype_args("pcp_place_coverage_refine_mounted")
    assert _arg_names(mounted) == ["ctx", "poses6", "n", "fan", "el_table"] + TAIL
    burst = _prototype_args("pcp_place_coverage_refine_burst")
    assert _arg_names(burst) == ["ctx", "poses5", "n", "fan", "rp", "roi", "roi_n", "reps", "ms"]
    assert burst[-1] == "double ms[2]"
    mburst = _prototype_args("pcp_place_coverage_refine_mounted_burst")
    assert _arg_names(mburst) == ["ctx", "poses6", "n", "fan", "el_table", "rp", "roi", "roi_n",
                                  "reps", "ms"]
    # the limits are pcp_place_coverage's and pcp_place_refine's, the struct the latter's: none new
    assert _define("PCP_COVER_MAX_POSES") == 1024 == _abi.COVER_MAX_POSES
    assert _define("PCP_REFINE_MAX_MOVES") == 64 == _abi.REFINE_MAX_MOVES
    assert len(re.findall(r"typedef struct pcp_refine_params\b", CODE)) == 1
    assert len(re.findall(r"\bstruct\s+pcp_\w*cover\w*refine\w*", CODE)) == 0
    assert C.sizeof(_abi.RefineParams) == 24 + 8 * _define("PCP_PLACE_MAX")
    # additive: the version stays, and the refinement has no kernel id of its own
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
        rp_at = 5 if "mounted" in name else 4
        assert sigs[name][2][rp_at]._type_ is _abi.RefineParams
        assert sigs[name][2][3]._type_ is _abi.FanParams
        assert len(getattr(lib, name).argtypes) == len(_prototype_args(name))
    # owner_cap is the one integer among the outputs
    assert sigs["pcp_place_coverage_refine"][2][18] is C.c_uint64
    assert sigs["pcp_place_coverage_refine_mounted"][2][19] is C.c_uint64
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    p = inspect.signature(_abi.Context.place_coverage_refine).parameters
    for k in ("poses5", "fan", "start", "n_locked", "max_moves", "min_separation", "roi",
              "want_swap_covered", "want_owner", "reserved"):
        assert k in p, k
    assert p["max_moves"].default == 16 and "k_max" not in p and "fixed" not in p
    p = inspect.signature(_abi.Context.place_coverage_refine_mounted).parameters
    assert "poses6" in p and "el_table" in p and p["max_moves"].default == 16
    assert "reps" in inspect.signature(_abi.Context.place_coverage_refine_burst).parameters
    assert "reps" in inspect.signature(_abi.Context.place_coverage_refine_mounted_burst).parameters


def test_null_context_is_refused():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    for n in (0, 3, _abi.COVER_MAX_POSES + 1):
        rp = _abi.Context._refine_params([0, 1], 0, 4, 0.0, 0)
        sel = (C.c_int64 * 2)(-7, -7)
        cov, sc = C.c_uint64(7), C.c_uint64(7)
        slot = (C.c_int32 * 4)(*[-7] * 4)
        frm, to = (C.c_int64 * 4)(*[-7] * 4), (C.c_int64 * 4)(*[-7] * 4)
        mcov = (C.c_uint64 * 4)(*[7] * 4)
        uniq = (C.c_uint64 * 2)(7, 7)
        npts, rpts = C.c_uint64(7), C.c_uint64(7)
        nm, cv = C.c_int32(-7), C.c_int32(-7)
        tail = (C.byref(rp), None, 0, sel, C.byref(cov), C.byref(sc), slot, frm, to, mcov, None,
                uniq, None, None, 0, C.byref(npts), C.byref(rpts), C.byref(nm), C.byref(cv))
        assert lib.pcp_place_coverage_refine(None, None, n, C.byref(fan),
                                             *tail) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_refine_mounted(None, None, n, C.byref(fan), None,
                                                     *tail) == _abi.PCP_E_INVALID
        assert list(sel) == [-7, -7] and cov.value == sc.value == 7 and list(uniq) == [7, 7]
        assert list(slot) == list(frm) == list(to) == [-7] * 4 and list(mcov) == [7] * 4
        assert npts.value == rpts.value == 7 and nm.value == cv.value == -7
        ms = (C.c_double * 2)(-7.0, -7.0)
        assert lib.pcp_place_coverage_refine_burst(None, None, n, C.byref(fan), C.byref(rp), None,
                                                   0, 3, ms) == _abi.PCP_E_INVALID
        assert lib.pcp_place_coverage_refine_mounted_burst(None, None, n, C.byref(fan), None,
                                                           C.byref(rp), None, 0, 3,
                                                           ms) == _abi.PCP_E_INVALID
        assert list(ms) == [-7.0] * 2
