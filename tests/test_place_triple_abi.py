"""pcp_place_triple at the C ABI boundary, without a GPU: the header declares both functions and
the two limits, the binding mirrors them argument for argument, the ABI version and the kernel ids
are unchanged, and a call that cannot be served (no context) is refused with nothing written."""
import ctypes as C
import inspect
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


def _prototype_args(name):
    m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", CODE, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_place_triple():
    args = _prototype_args("pcp_place_triple")
    assert args[0].replace(" ", "") == "pcp_ctx*ctx" and len(args) == 23
    assert [re.search(r"(\w+)\s*(?:\[\d*\])?$", a).group(1) for a in args[5:]] == [
        "pp", "best_triple", "triple_total", "triple_covered", "best_pair", "pair_total",
        "pair_covered", "best_single", "single_total", "single_covered", "base_total",
        "base_covered", "first_totals", "first_partners", "triple_totals", "cell_score",
        "cell_owner", "n_selected"]
    assert "const pcp_pair_params *pp" in args[5]   # the pair call's struct, no new one
    burst = _prototype_args("pcp_place_triple_burst")
    assert len(burst) == 8 and burst[-2] == "int reps" and burst[-1] == "double *ms_per_rep"
    assert _define("PCP_TRIPLE_MAX_POSES") == 512
    assert _define("PCP_TRIPLE_TABLE_MAX_POSES") == 128
    assert _define("PCP_TRIPLE_MAX_POSES") <= _define("PCP_PAIR_MAX_POSES")
    # additive: the version stays, and the search has no kernel id (PCP_K_PLACE is still the last)
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15


def test_binding_mirrors_the_prototypes():
    assert _abi.TRIPLE_MAX_POSES == _define("PCP_TRIPLE_MAX_POSES")
    assert _abi.TRIPLE_TABLE_MAX_POSES == _define("PCP_TRIPLE_TABLE_MAX_POSES")
    assert "pcp_place_triple" in _abi.ABI_SYMBOLS and "pcp_place_triple_burst" in _abi.ABI_SYMBOLS
    sigs = {s[0]: s for s in _abi._SIGS}
    for name in ("pcp_place_triple", "pcp_place_triple_burst"):
        assert len(sigs[name][2]) == len(_prototype_args(name)), name
        assert sigs[name][1] is C.c_int
        assert sigs[name][2][5]._type_ is _abi.PairParams
    lib = _abi.load_library()
    assert _abi.ABI_VERSION == 2 == lib.pcp_abi_version()
    assert len(lib.pcp_place_triple.argtypes) == 23 and len(lib.pcp_place_triple_burst.argtypes) == 8
    p = inspect.signature(_abi.Context.place_triple).parameters
    for k in ("fixed", "min_separation", "want_first", "want_triple_totals", "want_cells"):
        assert k in p, k
    assert "reps" in inspect.signature(_abi.Context.place_triple_burst).parameters


def test_null_context_is_refused():
    """Without a device there is no context to reach the argument checks with; what the entry
    refuses first is refused with every output as the caller left it."""
    lib = _abi.load_library()
    p = _abi.default_vl_params()
    zx = (C.c_double * 5)()
    cases = [_abi.PairParams(0, 0, 0.0), _abi.PairParams(-1, 0, 0.0), _abi.PairParams(0, 1, 0.0),
             _abi.PairParams(_abi.PLACE_MAX + 1, 0, 2.0)]
    for pp in cases:
        for n in (0, 3, _abi.TRIPLE_TABLE_MAX_POSES + 1, _abi.TRIPLE_MAX_POSES + 1):
            bt = (C.c_int64 * 3)(-7, -7, -7)
            bp = (C.c_int64 * 2)(-7, -7)
            d = [C.c_double(-7.0) for _ in range(4)]
            i = [C.c_int32(-7) for _ in range(5)]
            bs = C.c_int64(-7)
            ft, fp, tab = (C.c_double * 2)(-7.0, -7.0), (C.c_int64 * 2)(-7, -7), C.c_double(-7.0)
            rc = lib.pcp_place_triple(None, None, n, zx, C.byref(p), C.byref(pp), bt, C.byref(d[0]),
                                      C.byref(i[0]), bp, C.byref(d[1]), C.byref(i[1]), C.byref(bs),
                                      C.byref(d[2]), C.byref(i[2]), C.byref(d[3]), C.byref(i[3]),
                                      ft, fp, C.byref(tab), None, None, C.byref(i[4]))
            assert rc == _abi.PCP_E_INVALID
            assert list(bt) == [-7] * 3 and list(bp) == [-7, -7] and bs.value == -7
            assert all(x.value == -7.0 for x in d) and all(x.value == -7 for x in i)
            assert list(ft) == [-7.0, -7.0] and list(fp) == [-7, -7] and tab.value == -7.0
            ms = C.c_double(-7.0)
            rc = lib.pcp_place_triple_burst(None, None, n, zx, C.byref(p), C.byref(pp), 3,
                                            C.byref(ms))
            assert rc == _abi.PCP_E_INVALID and ms.value == -7.0
