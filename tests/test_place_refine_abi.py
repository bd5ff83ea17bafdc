"""pcp_place_refine at the C ABI boundary, without a GPU: the header declares both functions and
the parameter struct, the binding mirrors them, the ABI version and the kernel ids are unchanged,
and a null context is refused with nothing written."""
import ctypes as C
import re
from pathlib import Path

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", HEADER, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_declares_place_refine():
    assert re.search(r"\bint\s+pcp_place_refine\s*\(\s*pcp_ctx\s*\*", CODE)
    assert re.search(r"\bint\s+pcp_place_refine_burst\s*\(\s*pcp_ctx\s*\*", CODE)
    m = re.search(r"typedef\s+struct\s+pcp_refine_params\s*\{(.*?)\}\s*pcp_refine_params\s*;", CODE,
                  flags=re.S)
    assert m
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*(\[\w+\])?\s*;", m.group(1))
    assert fields == [("int32_t", "k", ""), ("int32_t", "n_locked", ""),
                      ("int32_t", "max_moves", ""), ("int32_t", "reserved", ""),
                      ("double", "min_separation", ""), ("int64_t", "start", "[PCP_PLACE_MAX]")]
    assert _define("PCP_REFINE_MAX_MOVES") == 64
    # the arguments of the entry, in order
    args = re.search(r"\bint\s+pcp_place_refine\s*\((.*?)\)\s*;", CODE, flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*(?:\[\d*\])?\s*$", a.strip()).group(1) for a in args.split(",")]
    assert names == ["ctx", "poses5", "n", "zx120_pose5", "p", "rp", "selected", "total", "covered",
                     "start_total", "start_covered", "move_slot", "move_from", "move_to",
                     "move_total", "move_covered", "swap_totals", "cell_score", "cell_owner",
                     "n_moves", "converged"]
    # additive: the version stays, and the refinement has no kernel id (PCP_K_PLACE is still last)
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15
    assert _abi.KERNELS[-1] == "place_sensors"


def test_binding_mirrors_the_struct():
    assert _abi.REFINE_MAX_MOVES == _define("PCP_REFINE_MAX_MOVES")
    assert [f[0] for f in _abi.RefineParams._fields_] == ["k", "n_locked", "max_moves", "reserved",
                                                          "min_separation", "start"]
    assert C.sizeof(_abi.RefineParams) == 152
    R = _abi.RefineParams
    assert [R.k.offset, R.n_locked.offset, R.max_moves.offset, R.reserved.offset,
            R.min_separation.offset, R.start.offset] == [0, 4, 8, 12, 16, 24]
    assert C.sizeof(R().start) == 8 * _abi.PLACE_MAX == 8 * _define("PCP_PLACE_MAX")
    assert "pcp_place_refine" in _abi.ABI_SYMBOLS and "pcp_place_refine_burst" in _abi.ABI_SYMBOLS
    sigs = {s[0]: s for s in _abi._SIGS}
    assert len(sigs["pcp_place_refine"][2]) == 21 and len(sigs["pcp_place_refine_burst"][2]) == 8
    assert _abi.ABI_VERSION == 2 == _abi.load_library().pcp_abi_version()


def test_null_context_is_refused():
    lib = _abi.load_library()
    p = _abi.default_vl_params()
    rp = _abi.RefineParams(1, 0, 4, 0, 0.0)
    zx = (C.c_double * 5)()
    poses = (C.c_double * 5)()
    sel = (C.c_int64 * 1)(-7)
    d = [C.c_double(-7.0) for _ in range(2)]
    i = [C.c_int32(-7) for _ in range(4)]
    ms, mc = (C.c_int32 * 4)(-7, -7, -7, -7), (C.c_int32 * 4)(-7, -7, -7, -7)
    mf, mt = (C.c_int64 * 4)(-7, -7, -7, -7), (C.c_int64 * 4)(-7, -7, -7, -7)
    mtot = (C.c_double * 4)(-7.0, -7.0, -7.0, -7.0)
    rc = lib.pcp_place_refine(None, poses, 1, zx, C.byref(p), C.byref(rp), sel, C.byref(d[0]),
                              C.byref(i[0]), C.byref(d[1]), C.byref(i[1]), ms, mf, mt, mtot, mc,
                              None, None, None, C.byref(i[2]), C.byref(i[3]))
    assert rc == _abi.PCP_E_INVALID
    assert list(sel) == [-7]   # nothing written
    assert all(x.value == -7.0 for x in d) and all(x.value == -7 for x in i)
    for a in (ms, mc, mf, mt, mtot):
        assert all(x == -7 for x in a)
    t = C.c_double(-7.0)
    rc = lib.pcp_place_refine_burst(None, poses, 1, zx, C.byref(p), C.byref(rp), 3, C.byref(t))
    assert rc == _abi.PCP_E_INVALID and t.value == -7.0
