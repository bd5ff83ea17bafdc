"""pcp_place_aimed at the C ABI boundary, without a GPU: the header declares both functions, the
two limits and the struct, the binding mirrors them (size and offsets included), the ABI version
and the kernel ids are unchanged, and a call without a context is refused with nothing written."""
import ctypes as C
import inspect
import re
from pathlib import Path

import aim_ref

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", HEADER, flags=re.M)
    assert m, name
    return int(m.group(1))


def _prototype_args(name):
    m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", CODE, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_place_aimed():
    args = _prototype_args("pcp_place_aimed")
    assert args[0].replace(" ", "") == "pcp_ctx*ctx" and len(args) == 17
    assert [re.search(r"(\w+)\s*(?:\[\d*\])?$", a).group(1) for a in args[5:]] == [
        "ap", "aims", "selected", "selected_aim", "total_after", "covered_after", "round_totals",
        "cell_score", "cell_owner", "base_total", "base_covered", "n_selected"]
    assert "const pcp_aim_params *ap" in args[5]
    burst = _prototype_args("pcp_place_aimed_burst")
    assert len(burst) == 9 and burst[-2] == "int reps" and burst[-1] == "double *ms_per_round"
    assert _define("PCP_AIM_MAX") == 64 == aim_ref.AIM_MAX
    assert _define("PCP_AIM_MAX_ROWS") == 65536 == aim_ref.AIM_MAX_ROWS
    # additive: the version stays, and the rounds have no kernel id of their own
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15


def test_struct_layout():
    """pcp_aim_params as the header lays it out: four int32, three doubles, sixteen int64, sixteen
    int32 -- 232 bytes, no padding."""
    body = re.search(r"typedef struct pcp_aim_params\s*\{(.*?)\}\s*pcp_aim_params;", CODE,
                     flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", body)
    names = []
    for _, decl in fields:
        names += [re.match(r"\s*(\w+)", d).group(1) for d in decl.split(",")]
    assert names == [f[0] for f in _abi.AimParams._fields_] == [
        "k_max", "n_aims", "n_fixed", "reserved", "h_fov", "v_fov", "min_separation",
        "fixed_pose", "fixed_aim"]
    assert _define("PCP_PLACE_MAX") == _abi.PLACE_MAX == 16
    assert C.sizeof(_abi.AimParams) == 232
    off = {k: getattr(_abi.AimParams, k).offset for k in names}
    assert off == {"k_max": 0, "n_aims": 4, "n_fixed": 8, "reserved": 12, "h_fov": 16, "v_fov": 24,
                   "min_separation": 32, "fixed_pose": 40, "fixed_aim": 168}


def test_binding_mirrors_the_prototypes():
    assert _abi.AIM_MAX == _define("PCP_AIM_MAX") and _abi.AIM_MAX_ROWS == _define("PCP_AIM_MAX_ROWS")
    assert "pcp_place_aimed" in _abi.ABI_SYMBOLS and "pcp_place_aimed_burst" in _abi.ABI_SYMBOLS
    sigs = {s[0]: s for s in _abi._SIGS}
    for name in ("pcp_place_aimed", "pcp_place_aimed_burst"):
        assert len(sigs[name][2]) == len(_prototype_args(name)), name
        assert sigs[name][1] is C.c_int
        assert sigs[name][2][5]._type_ is _abi.AimParams
    lib = _abi.load_library()
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    assert len(lib.pcp_place_aimed.argtypes) == 17 and len(lib.pcp_place_aimed_burst.argtypes) == 9
    p = inspect.signature(_abi.Context.place_aimed).parameters
    for k in ("aims", "h_fov", "v_fov", "k_max", "fixed", "min_separation", "want_round_totals",
              "want_cells"):
        assert k in p, k
    assert "reps" in inspect.signature(_abi.Context.place_aimed_burst).parameters


def test_null_context_is_refused():
    lib = _abi.load_library()
    p = _abi.default_vl_params()
    zx = (C.c_double * 5)()
    aims = (C.c_double * 2)(0.0, 0.0)
    for ap in (_abi.AimParams(1, 1, 0, 0, 1.5, 1.0, 0.0), _abi.AimParams(0, 1, 0, 0, 1.5, 1.0, 0.0),
               _abi.AimParams(1, 1, 0, 1, 1.5, 1.0, 2.0)):
        for n in (0, 3, _abi.PAIR_MAX_POSES + 1):
            sel, sa = (C.c_int64 * 16)(*[-7] * 16), (C.c_int32 * 16)(*[-7] * 16)
            tot, cov = (C.c_double * 16)(*[-7.0] * 16), (C.c_int32 * 16)(*[-7] * 16)
            bt, bc, ns = C.c_double(-7.0), C.c_int32(-7), C.c_int32(-7)
            rc = lib.pcp_place_aimed(None, None, n, zx, C.byref(p), C.byref(ap), aims, sel, sa, tot,
                                     cov, None, None, None, C.byref(bt), C.byref(bc), C.byref(ns))
            assert rc == _abi.PCP_E_INVALID
            assert list(sel) == [-7] * 16 and list(sa) == [-7] * 16 and list(cov) == [-7] * 16
            assert list(tot) == [-7.0] * 16 and bt.value == -7.0 and bc.value == ns.value == -7
            ms = C.c_double(-7.0)
            rc = lib.pcp_place_aimed_burst(None, None, n, zx, C.byref(p), C.byref(ap), aims, 3,
                                           C.byref(ms))
            assert rc == _abi.PCP_E_INVALID and ms.value == -7.0
