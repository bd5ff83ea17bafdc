"""pcp_raycast_fan_mounted / pcp_simulate_scan_mounted / pcp_raycast_fan_mounted_burst at the C
ABI boundary, without a GPU: the header declares the three calls, the binding mirrors them, a
null context is refused with nothing written, and the ABI version and the kernel ids are what
they were."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
CALLS = ["pcp_raycast_fan_mounted", "pcp_simulate_scan_mounted", "pcp_raycast_fan_mounted_burst"]


def _decl(name):
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", CODE, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_three_calls():
    for name in CALLS:
        args = _decl(name)
        assert args[0] == "pcp_ctx *ctx"
        assert args[1] == "const double *poses6" and args[2] == "uint64_t n"
        assert args[3] == "const pcp_fan_params *fan" and args[4] == "const double *el_table"
    assert _decl("pcp_raycast_fan_mounted")[5:] == _decl("pcp_raycast_fan")[4:]
    assert _decl("pcp_simulate_scan_mounted")[5:] == _decl("pcp_simulate_scan")[4:]
    assert _decl("pcp_raycast_fan_mounted_burst")[5:] == _decl("pcp_raycast_fan_burst")[4:]
    m = re.search(r"^#define\s+PCP_ABI_VERSION\s+(\d+)", HEADER, flags=re.M)
    assert m and int(m.group(1)) == 2 == _abi.ABI_VERSION
    assert len(_abi.KERNELS) == 15
    m = re.search(r"\benum\s+pcp_kernel_id\s*\{([^}]*)PCP_K_COUNT", CODE, flags=re.S)
    assert m and len(re.findall(r"\bPCP_K_\w+", m.group(1))) == 15
    # the contract: the pose layout, the sign of pitch and the rotation order are written down
    assert "poses6" in HEADER and "pitch = -pitch_tf" in HEADER
    assert "x2 = x1*cp - z1*sp" in HEADER


def test_binding_mirrors_them():
    lib = _abi.load_library()
    sigs = {s[0]: s for s in _abi._SIGS}
    for name in CALLS:
        assert name in _abi.ABI_SYMBOLS and hasattr(lib, name)
        assert len(sigs[name][2]) == len(_decl(name)), name
        assert sigs[name][1] is C.c_int
    for meth in ("raycast_fan_mounted", "simulate_scan_mounted", "raycast_fan_mounted_burst"):
        assert callable(getattr(_abi.Context, meth))
    # the level twins' argument lists with the table inserted after the fan
    for a, b in (("pcp_raycast_fan_mounted", "pcp_raycast_fan"),
                 ("pcp_simulate_scan_mounted", "pcp_simulate_scan"),
                 ("pcp_raycast_fan_mounted_burst", "pcp_raycast_fan_burst")):
        la, lb = list(sigs[a][2]), list(sigs[b][2])
        assert la[:4] == lb[:4] and la[4] is C.c_void_p and la[5:] == lb[4:], a


def test_null_context_is_refused_with_nothing_written():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    poses = np.zeros((1, 6))
    tab = np.zeros(2)
    blocked = np.full(1, 0xABABABAB, np.uint32)
    units = np.full(1, 77, np.uint64)
    fh = np.full(16, -7, np.int16)
    best = C.c_int64(123)
    rc = lib.pcp_raycast_fan_mounted(None, _abi._ptr(poses), 1, C.byref(fan), _abi._ptr(tab),
                                     _abi._ptr(blocked), _abi._ptr(units), _abi._ptr(fh),
                                     C.byref(best))
    assert rc == _abi.PCP_E_INVALID
    assert blocked[0] == 0xABABABAB and units[0] == 77 and (fh == -7).all() and best.value == 123
    nret = C.c_uint64(7)
    off = (C.c_uint64 * 2)(9, 9)
    rc = lib.pcp_simulate_scan_mounted(None, _abi._ptr(poses), 1, C.byref(fan), _abi._ptr(tab), None,
                                       0, C.byref(nret), off, None, None, None, None, 0, None, None,
                                       None)
    assert rc == _abi.PCP_E_INVALID
    assert nret.value == 7 and list(off) == [9, 9]
    ms = C.c_double(5.0)
    rc = lib.pcp_raycast_fan_mounted_burst(None, _abi._ptr(poses), 1, C.byref(fan), None, 3,
                                           C.byref(ms))
    assert rc == _abi.PCP_E_INVALID and ms.value == 5.0


def test_binding_checks_the_table_length():
    import pytest

    with pytest.raises(ValueError):
        _abi.Context._el_table(_abi.fan_params(n_az=8, n_el=3), [0.0, 0.1])
    assert _abi.Context._el_table(_abi.fan_params(n_az=8, n_el=3), None) is None
