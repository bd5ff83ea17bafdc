"""pcp_simulate_scan at the C ABI boundary, without a GPU: the header declares both entry points,
the record and the pose bound, the binding mirrors them -- and the NumPy restatement of the
definition (tests/scan_ref.py) stands on the oracle: on the fixtures of the GPU tests every
blocked ray's query point has a point within r, the sample before it has none, the restated
KdTreeFLANN returns exactly the restatement's candidate set, ties exist and a pose has no return."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "pcp_abi.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_declares_simulate_scan():
    assert re.search(r"\bint\s+pcp_simulate_scan\s*\(\s*pcp_ctx\s*\*", CODE)
    assert re.search(r"\bint\s+pcp_simulate_scan_burst\s*\(\s*pcp_ctx\s*\*", CODE)
    m = re.search(r"typedef\s+struct\s+pcp_scan_return\s*\{(.*?)\}\s*pcp_scan_return\s*;", CODE,
                  flags=re.S)
    assert m
    body = m.group(1)
    assert re.search(r"\bfloat\s+x\s*,\s*y\s*,\s*z\s*;", body)
    rest = re.findall(r"\b(float|uint32_t)\s+(\w+)\s*;", body)
    assert rest == [("float", "range"), ("uint32_t", "ray"), ("uint32_t", "point")]
    m = re.search(r"^#define\s+PCP_ABI_VERSION\s+(\d+)", HEADER, flags=re.M)
    assert m and int(m.group(1)) == 2


def test_binding_mirrors_the_record_and_the_bound():
    m = re.search(r"^#define\s+PCP_SCAN_MAX_POSES\s+(\d+)\s*$", HEADER, flags=re.M)
    assert m and int(m.group(1)) == _abi.SCAN_MAX_POSES == 64
    R = _abi.ScanReturn
    assert C.sizeof(R) == 24
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("x", 0), ("y", 4), ("z", 8), ("range", 12), ("ray", 16), ("point", 20)]
    assert [t for _, t in R._fields_] == [C.c_float] * 4 + [C.c_uint32] * 2
    d = _abi.SCAN_RETURN_DTYPE
    assert d.itemsize == 24 and d == scan_ref.RETURN_DTYPE
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 16, 20]
    assert "pcp_simulate_scan" in _abi.ABI_SYMBOLS
    assert "pcp_simulate_scan_burst" in _abi.ABI_SYMBOLS
    lib = _abi.load_library()
    assert hasattr(lib, "pcp_simulate_scan") and hasattr(lib, "pcp_simulate_scan_burst")
    assert hasattr(_abi.Context, "simulate_scan")


def test_null_context_is_refused():
    lib = _abi.load_library()
    fan = _abi.fan_params(n_az=8, n_el=2)
    nret = C.c_uint64(7)
    off = (C.c_uint64 * 1)(9)
    rc = lib.pcp_simulate_scan(None, None, 0, C.byref(fan), None, 0, C.byref(nret), off, None,
                               None, None, None, 0, None, None, None)
    assert rc == _abi.PCP_E_INVALID
    assert nret.value == 7 and off[0] == 9   # nothing written
    ms = (C.c_double * 2)()
    assert lib.pcp_simulate_scan_burst(None, None, 0, C.byref(fan), 1, ms) == _abi.PCP_E_INVALID


@pytest.mark.parametrize("n_az,n_el,dmax", [(100, 37, 15.0), (64, 3, 110.0)])
def test_restatement_preconditions(oracle, n_az, n_el, dmax):
    cloud, poses, fan, fh, blocked, ref = scan_ref.clutter_case(oracle, n_az, n_el, dmax)
    if dmax > 100.0:   # a step table past the fan kernels' LDS copy (256 entries)
        assert scan_ref.step_table(dmax - 0.08).size > 256
    T = oracle.Cloud(cloud)
    q, qprev, k = ref["q"], ref["qprev"], ref["k"]
    M = q.shape[0]
    assert M == int(blocked.sum()) > 0
    r = scan_ref.RAY_RADIUS
    # the blocking set is never empty, and the sample before the first hit has none
    for m in range(M):
        assert T.count_within(q[m], r) > 0, m
        if k[m] > 0:
            assert T.count_within(qprev[m], r) == 0, m
    # the candidate sets are the reference's own radius search (KdTreeFLANN restated)
    kd = oracle.KdTree(cloud)
    qid, pid = ref["cand_q"], ref["cand_p"]
    starts = np.searchsorted(qid, np.arange(M + 1))
    for m in range(0, M, 7):
        n, idx = kd.radius_search(q[m], r, want_idx=True)
        mine = np.sort(pid[starts[m]:starts[m + 1]])
        assert n == mine.size and np.array_equal(idx, mine), m
    assert ref["ties"] >= 1
    seg = np.diff(ref["offsets"].astype(np.int64))
    assert np.array_equal(seg, blocked.astype(np.int64))
    if dmax < 40.0:   # pose 4 stands ~48 m outside the cloud: an empty segment (at 110 m its
        assert seg[4] == 0 and (seg == 0).any()   # beams reach the cloud)
    # the ties resolve to the lowest index: no return names an appended duplicate whose
    # original is its equal
    n0 = cloud.shape[0] - 2000
    assert not (ref["returns"]["point"] >= n0).any()
