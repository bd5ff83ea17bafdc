"""pcp_place_pair at the C ABI boundary, without a GPU: the header declares both functions and the
parameter struct, the binding mirrors them, the ABI version and the kernel ids are unchanged, and
a null context is refused with nothing written."""
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


def test_header_declares_place_pair():
    assert re.search(r"\bint\s+pcp_place_pair\s*\(\s*pcp_ctx\s*\*", CODE)
    assert re.search(r"\bint\s+pcp_place_pair_burst\s*\(\s*pcp_ctx\s*\*", CODE)
    m = re.search(r"typedef\s+struct\s+pcp_pair_params\s*\{(.*?)\}\s*pcp_pair_params\s*;", CODE,
                  flags=re.S)
    assert m
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*(\[\w+\])?\s*;", m.group(1))
    assert fields == [("int32_t", "n_fixed", ""), ("int32_t", "reserved", ""),
                      ("double", "min_separation", ""), ("int64_t", "fixed", "[PCP_PLACE_MAX]")]
    assert _define("PCP_PAIR_MAX_POSES") == 2048
    # additive: the version stays, and the search has no kernel id (PCP_K_PLACE is still the last)
    assert _define("PCP_ABI_VERSION") == 2
    ids = re.search(r"enum\s+pcp_kernel_id\s*\{(.*?)\}", CODE, flags=re.S).group(1)
    names = re.findall(r"\b(PCP_K_\w+)", ids)
    assert names[-2:] == ["PCP_K_PLACE", "PCP_K_COUNT"]
    assert len(_abi.KERNELS) == names.index("PCP_K_COUNT") == 15
    assert _abi.KERNELS[-1] == "place_sensors"


def test_binding_mirrors_the_struct():
    assert _abi.PAIR_MAX_POSES == _define("PCP_PAIR_MAX_POSES")
    assert [f[0] for f in _abi.PairParams._fields_] == ["n_fixed", "reserved", "min_separation",
                                                        "fixed"]
    assert C.sizeof(_abi.PairParams) == 144
    assert _abi.PairParams.reserved.offset == 4
    assert _abi.PairParams.min_separation.offset == 8
    assert _abi.PairParams.fixed.offset == 16
    assert C.sizeof(_abi.PairParams().fixed) == 8 * _abi.PLACE_MAX == 8 * _define("PCP_PLACE_MAX")
    assert "pcp_place_pair" in _abi.ABI_SYMBOLS and "pcp_place_pair_burst" in _abi.ABI_SYMBOLS
    assert _abi.ABI_VERSION == 2 == _abi.load_library().pcp_abi_version()


def test_null_context_is_refused():
    lib = _abi.load_library()
    p = _abi.default_vl_params()
    pp = _abi.PairParams(0, 0, 0.0)
    zx = (C.c_double * 5)()
    bp = (C.c_int64 * 2)(-7, -7)
    d = [C.c_double(-7.0) for _ in range(3)]
    i = [C.c_int32(-7) for _ in range(4)]
    bs = C.c_int64(-7)
    rc = lib.pcp_place_pair(None, None, 0, zx, C.byref(p), C.byref(pp), bp, C.byref(d[0]),
                            C.byref(i[0]), C.byref(bs), C.byref(d[1]), C.byref(i[1]),
                            C.byref(d[2]), C.byref(i[2]), None, None, None, None, C.byref(i[3]))
    assert rc == _abi.PCP_E_INVALID
    assert list(bp) == [-7, -7] and bs.value == -7   # nothing written
    assert all(x.value == -7.0 for x in d) and all(x.value == -7 for x in i)
    ms = C.c_double(-7.0)
    rc = lib.pcp_place_pair_burst(None, None, 0, zx, C.byref(p), C.byref(pp), 3, C.byref(ms))
    assert rc == _abi.PCP_E_INVALID and ms.value == -7.0
