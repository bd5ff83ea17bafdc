"""pcp_excavate against the CPU oracle on the carve's own edges (the cases of carve_cases.py,
shown decisive by test_carve_cases.py): every keep-tile size and remainder, whole tiles and
whole clouds carved, nearest-point ties, more fallback queries than blocks, points exactly at
the radius, every record layout, both output paths with exact-size and short buffers, and z
sums on both sides of the line where the reference's plain double sum is exact.  Kept points
(order, x / y / z / rgb bits), generated surface and area records, counts and pose: bit-exact."""
import ctypes as C
import math

import numpy as np
import pytest

import carve_cases as cc
from pointcloud_processor_amd import _abi

pytestmark = pytest.mark.gpu

COLS = [0, 1, 2, 4]   # x, y, z, rgb of a PointXYZRGB record


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_format(rec):
    """The constant fields of PointXYZRGB records: (x, y, z, 1, rgb, 0, 0, 0)."""
    assert np.all(_bits(rec[:, 3]) == _bits(np.float32(1.0)))
    assert not _bits(rec[:, 5:]).any()


def _compare(terr, area, pose, cloud, ref, rgb=None, heights_exact=True):
    """The outputs of one call against the oracle's (keep, surf, area, pose)."""
    keep, surf, r_area, r_pose = ref
    nk = int(keep.sum())
    assert terr.shape[0] == nk + surf.shape[0] and area.shape[0] == r_area.shape[0]
    assert surf.shape[0] > 0 and r_area.shape[0] > 0
    kept = cloud[keep]
    rgb = cloud[:, 4] if rgb is None else rgb
    np.testing.assert_array_equal(_bits(terr[:nk, :3]), _bits(kept[:, :3]))
    np.testing.assert_array_equal(_bits(terr[:nk, 4]), _bits(rgb[keep]))
    # record columns x, y, z, rgb against the oracle's rows (x, y, z, rgb); z and the pose's
    # height left to the caller when the case's heights are not the reference's bits
    cols, r_cols = (COLS, [0, 1, 2, 3]) if heights_exact else ([0, 1, 4], [0, 1, 3])
    np.testing.assert_array_equal(_bits(terr[nk:, cols]), _bits(surf[:, r_cols]))
    np.testing.assert_array_equal(_bits(area[:, cols]), _bits(r_area[:, r_cols]))
    which = [0, 1, 2, 3] if heights_exact else [0, 1, 3]
    np.testing.assert_array_equal(pose[which].view(np.uint64), r_pose[which].view(np.uint64))
    _check_format(terr)
    _check_format(area)


def _run(ctx, oracle, case, mixed=True):
    ref = cc.reference(oracle, case)
    if mixed:
        assert 0 < ref[0].sum() < ref[0].size
    terr, area, pose = ctx.excavate(case.cloud, (case.t, case.q), _abi.excavation_params(**case.kw))
    _compare(terr, area, pose, case.cloud, ref)


@pytest.mark.parametrize("n", cc.TILE_SIZES)
def test_keep_tile_sizes(gpu, oracle, n):
    """C1: 1, 2, 15 and 16 points per thread, exact multiples of the tile, a last tile of one
    point, fewer points than a wave; carved points in most tiles, in random point order."""
    _run(gpu, oracle, cc.tile_case(n), mixed=n >= 2)   # (one point is carved or kept)


@pytest.mark.parametrize("items", [1, 2])
def test_whole_tiles_carved(gpu, oracle, items):
    """C2: the first, a middle and the last tile keep nothing: their counts reach 0."""
    _run(gpu, oracle, cc.whole_tile_case(items))


def test_all_points_carved(gpu, oracle):
    """C3: nothing kept: the generated surface starts at record 0."""
    case = cc.all_carved_case()
    assert cc.reference(oracle, case)[0].sum() == 0
    _run(gpu, oracle, case, mixed=False)


@pytest.mark.parametrize("n_finite", cc.NEAREST_COUNTS)
def test_nearest_point_ties(gpu, oracle, n_finite):
    """C4: equal float distance goes to the lowest input index, whatever the index's cell
    order, at 1, 255, 4,096 and 4,097 indexed points (the unrolled sweep's step and one past)."""
    _run(gpu, oracle, cc.nearest_case(n_finite).case)


def test_more_fallbacks_than_blocks(gpu, oracle):
    """C5: more than 4,096 nearest-point queries: the blocks stride over the list."""
    _run(gpu, oracle, cc.fallback_case())


@pytest.mark.parametrize("variant", ["flat", "lifted", "tiny"])
def test_points_at_the_radius(gpu, oracle, variant):
    """C6: points at exactly the radius (acc == r2) stay out of the mean; queries on the r
    lattice of the cloud's minimum corner."""
    _run(gpu, oracle, cc.radius_tie_case(variant))


@pytest.mark.parametrize("layout", cc.LAYOUTS)
def test_record_layouts(gpu, oracle, layout):
    """C7: 12-, 16-, 20- and 32-byte records, x / y / z at other offsets; rgb is the float at
    byte 16 of records of 20 bytes and more, else 0."""
    case = cc.layout_case()
    ref = cc.reference(oracle, case)
    assert 0 < ref[0].sum() < ref[0].size
    raw, step, offs, want = cc.pack_layout(case.cloud, layout)
    terr, area, pose = gpu.excavate(raw, (case.t, case.q), _abi.excavation_params(**case.kw),
                                    point_step=step, offs=offs)
    _compare(terr, area, pose, case.cloud, ref, rgb=want)


class _Call:
    """One pcp_excavate call with caller-chosen capacities (the binding's excavate() always
    passes pcp_excavate_bounds).  The arrays themselves hold the bounds: the records past the
    capacity handed to the call are guards, which it must leave alone."""
    GUARD = 0x7B

    def __init__(self, ctx, case, terr_rows, area_rows, terr_cap=None, area_cap=None,
                 terr_null=False):
        v = _abi.cloud_view(case.cloud)
        p = _abi.excavation_params(**case.kw)
        tf = _abi.Rigid((C.c_double * 3)(*case.t), (C.c_double * 4)(*case.q))
        nt, na = C.c_uint64(), C.c_uint64()
        assert ctx.lib.pcp_excavate_bounds(C.byref(p), v.n, C.byref(nt), C.byref(na)) == 0
        assert nt.value > terr_rows and na.value > area_rows
        self.terr = np.empty((nt.value, 8), np.float32)
        self.area = np.empty((na.value, 8), np.float32)
        self.terr.view(np.uint8)[:] = self.GUARD
        self.area.view(np.uint8)[:] = self.GUARD
        self.pose = np.zeros(4, np.float64)
        self.rc = ctx.lib.pcp_excavate(
            ctx.h, C.byref(v), C.byref(p), C.byref(tf),
            None if terr_null else self.terr.ctypes.data_as(C.c_void_p),
            terr_rows if terr_cap is None else terr_cap, C.byref(nt),
            self.area.ctypes.data_as(C.c_void_p),
            area_rows if area_cap is None else area_cap, C.byref(na),
            self.pose.ctypes.data_as(C.c_void_p))
        self.nt, self.na = nt.value, na.value

    def guards_intact(self, terr_rows, area_rows):
        return bool(np.all(self.terr[terr_rows:].view(np.uint8) == self.GUARD) and
                    np.all(self.area[area_rows:].view(np.uint8) == self.GUARD))


@pytest.mark.parametrize("zc_in", [None, "0"])
def test_output_paths(oracle, monkeypatch, zc_in):
    """The pinned landing (default) and the device buffer with the area records behind the
    queries (PCP_ZC_IN=0), each with: buffers of pcp_excavate_bounds (one trip), buffers of
    exactly the record counts (the copy after the counts), a terrain and then an area buffer one
    record short (PCP_E_CAPACITY with both counts, nothing written), a null terrain buffer
    (PCP_E_INVALID) -- and a correct, bit-exact call after each refusal."""
    if zc_in is not None:
        monkeypatch.setenv("PCP_ZC_IN", zc_in)
    else:
        monkeypatch.delenv("PCP_ZC_IN", raising=False)
    case = cc.whole_tile_case(2)
    ref = cc.reference(oracle, case)
    keep, surf, r_area, _ = ref
    assert case.cloud.shape[0] == 20000 and 0 < keep.sum() < keep.size
    nt, na = int(keep.sum()) + surf.shape[0], r_area.shape[0]
    assert nt > 1 and na > 1
    ctx = _abi.Context(0)
    try:
        _run(ctx, oracle, case)                                   # (i) the bounds
        c = _Call(ctx, case, nt, na)                              # (ii) exactly the counts
        assert (c.rc, c.nt, c.na) == (_abi.PCP_OK, nt, na)
        _compare(c.terr[:nt], c.area[:na], c.pose, case.cloud, ref)
        assert c.guards_intact(nt, na)
        for short in ({"terr_cap": nt - 1}, {"area_cap": na - 1}):   # (iii) one record short
            c = _Call(ctx, case, nt, na, **short)
            assert (c.rc, c.nt, c.na) == (_abi.PCP_E_CAPACITY, nt, na)
            assert c.guards_intact(0, 0)
            _run(ctx, oracle, case)
        c = _Call(ctx, case, nt, na, terr_null=True)              # the null-output refusal
        assert c.rc == _abi.PCP_E_INVALID and c.guards_intact(0, 0)
        c = _Call(ctx, case, nt, na)
        assert (c.rc, c.nt, c.na) == (_abi.PCP_OK, nt, na)
        _compare(c.terr[:nt], c.area[:na], c.pose, case.cloud, ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("zc_in", [None, "0"])
def test_tile_sizes_in_sequence(oracle, monkeypatch, zc_in):
    """One context through n = 262,145 -> 255 -> 16,385 -> 262,144 under one pose: the scratch
    buffers and the two counter sets reused across tile sizes, the cached lattice reused for
    every cloud after the first; on both output paths."""
    if zc_in is not None:
        monkeypatch.setenv("PCP_ZC_IN", zc_in)
    else:
        monkeypatch.delenv("PCP_ZC_IN", raising=False)
    ctx = _abi.Context(0)
    try:
        for n in (262145, 255, 16385, 262144):
            _run(ctx, oracle, cc.tile_case(n))
    finally:
        ctx.close()


def test_sum_exact(gpu, oracle):
    """C8 (a): every z a multiple of 2^-42 (the sufficient condition pcp_abi.h states): the
    reference's plain double sum is exact, and the mean is its bits."""
    _run(gpu, oracle, cc.sum_case("exact"))


def test_sum_inexact(gpu, oracle):
    """C8 (b): z = 0.25 among +-2^-55, where the reference's sequential sum depends on its
    order (test_carve_cases.py: its mean differs from the exact one at the centre and at most
    queries).  The library promises the exactly rounded sum over the count, to one ulp of the
    mean (the double-double's final rounding): every height-dependent output is derived from
    fsum(z) / m within that ulp -- the pose height as a double, the generated z as floats --
    and everything that depends on no height is the oracle's bits.  (The kept set does depend
    on heights, by margins above 1e-3 m against a mean that moves by 1e-17.)"""
    case = cc.sum_case("inexact")
    ref = cc.reference(oracle, case)
    keep, surf, r_area, r_pose = ref
    assert 0 < keep.sum() < keep.size
    terr, area, pose = gpu.excavate(case.cloud, (case.t, case.q),
                                    _abi.excavation_params(**case.kw))
    _compare(terr, area, pose, case.cloud, ref, heights_exact=False)
    g = cc.geometry(case.t, case.q, case.kw)
    z64 = case.cloud[:, 2].astype(np.float64)
    mean = []
    for x, y in g.queries:
        nb = cc.neighbours(case.cloud, x, y, g.radius)
        mean.append(math.fsum(z64[nb]) / nb.size)
    mean = np.array(mean)
    assert mean[0] != r_pose[2]   # the reference is past its exactness here
    near = [np.nextafter(mean, -np.inf), mean, np.nextafter(mean, np.inf)]
    print(f"pose z {pose[2]!r}: exact mean {mean[0]!r}, reference {r_pose[2]!r}")
    assert pose[2] in (near[0][0], near[1][0], near[2][0])
    nk = int(keep.sum())
    allowed = [cc.generated_z(g, h) for h in near]
    got_s, got_a = terr[nk:, 2], area[:, 2]
    assert np.all(np.any([_bits(got_s) == _bits(s) for s, _ in allowed], axis=0))
    assert np.all(np.any([_bits(got_a) == _bits(a) for _, a in allowed], axis=0))
