"""The carve's edge cases (carve_cases.py) are decisive: from the CPU oracle and numpy alone,
each case puts on the line what test_carve_edges.py compares on the GPU -- carved points in
the tiles that count them, whole tiles carved, float-distance ties, more fallback queries than
the nearest-point launch has blocks, points exactly at the radius, z sums on both sides of
exactness.  A GPU comparison over a case that fails here would pass vacuously."""
import math

import numpy as np
import pytest

import carve_cases as cc


def _tile_hits(keep, n):
    """Per keep tile: the number of carved points."""
    tile = cc.keep_tile(n)
    return np.add.reduceat((~keep).astype(np.int64), np.arange(0, n, tile))


def test_tile_sizes_cover_the_keep_arithmetic():
    """C1: the sizes reach 1, 2, 15 and 16 points per thread, a cloud that is an exact multiple
    of its tile and a last tile of one point (keep_items restated from its formula)."""
    items = {n: min(max(math.ceil(n / 16384), 1), 16) for n in cc.TILE_SIZES}
    assert {n: cc.keep_items(n) for n in cc.TILE_SIZES} == items
    assert {1, 2, 15, 16} <= set(items.values())
    assert items[16384] == 1 and items[16385] == 2 and items[245760] == 15 and items[245761] == 16
    multiples = [n for n in cc.TILE_SIZES if n % (256 * items[n]) == 0]
    one_left = [n for n in cc.TILE_SIZES if n > 256 and n % (256 * items[n]) == 1]
    assert {256, 16384, 245760, 262144} <= set(multiples)
    assert {257, 16385, 245761, 262145} <= set(one_left)
    assert any(n < 64 for n in cc.TILE_SIZES)


@pytest.mark.parametrize("n", cc.TILE_SIZES)
def test_tile_case_carves_across_tiles(oracle, n):
    """C1: the oracle carves in the first tile, in the last tile and in at least half of all
    tiles (n >= 257); the mask is mixed wherever n allows it."""
    case = cc.tile_case(n)
    assert case.cloud.shape == (n, 8)
    keep, surf, area, _ = cc.reference(oracle, case)
    assert surf.shape[0] > 0 and area.shape[0] > 0
    if n >= 2:
        assert 0 < keep.sum() < n
    if n >= 257:
        hits = _tile_hits(keep, n)
        assert hits.size == math.ceil(n / cc.keep_tile(n))
        assert hits[0] >= 1 and hits[-1] >= 1
        assert (hits > 0).sum() * 2 >= hits.size
        if n % cc.keep_tile(n) == 1:
            assert not keep[-1]   # the last tile's only point: its count reaches 0


@pytest.mark.parametrize("items", [1, 2])
def test_whole_tiles_carved(oracle, items):
    """C2: the mask is all-false on exactly tile 0, the middle tile and the last tile."""
    case = cc.whole_tile_case(items)
    n = case.cloud.shape[0]
    assert cc.keep_items(n) == items and n % cc.keep_tile(n) != 0
    keep, surf, area, _ = cc.reference(oracle, case)
    tile = cc.keep_tile(n)
    sizes = np.minimum(tile, n - np.arange(0, n, tile))
    empty = np.nonzero(_tile_hits(keep, n) == sizes)[0].tolist()
    assert empty == cc.whole_tiles(n) and len(set(empty)) == 3
    assert surf.shape[0] > 0 and area.shape[0] > 0


def test_all_carved(oracle):
    """C3: nothing is kept, and the surface is still generated."""
    case = cc.all_carved_case()
    keep, surf, area, _ = cc.reference(oracle, case)
    assert 256 < keep.size <= 320 and keep.sum() == 0
    assert surf.shape[0] > 0 and area.shape[0] > 0


@pytest.mark.parametrize("n_finite", cc.NEAREST_COUNTS)
def test_nearest_tie_goes_to_the_lower_index(oracle, n_finite):
    """C4: the pit centre's column has no point within the radius; the nearest-point answer is
    the +0.8 m point's while it has the lower input index, and the -0.8 m point's after the two
    rows are swapped.  Every generated query falls back the same way."""
    nc = cc.nearest_case(n_finite)
    c = nc.case.cloud
    assert int(np.isfinite(c[:, :3]).all(axis=1).sum()) == n_finite and c.shape[0] == n_finite + 5
    g = cc.geometry(nc.case.t, nc.case.q, nc.case.kw)
    for x, y in g.queries:
        assert cc.neighbours(c, x, y, g.radius).size == 0
    assert oracle.terrain_height(c, nc.px, nc.py) == np.float32(0.8)
    keep, surf, area, pose = cc.reference(oracle, nc.case)
    assert surf.shape[0] > 0 and area.shape[0] > 0 and 0 < keep.sum() < c.shape[0]
    if n_finite == 1:
        return
    assert nc.hi < nc.lo and c[nc.hi, 2] == np.float32(0.8) and c[nc.lo, 2] == np.float32(-0.8)
    assert np.array_equal(c[nc.hi, :2], c[nc.lo, :2])
    acc = cc.flann_acc(c, nc.px, nc.py)
    assert acc[nc.hi] == acc[nc.lo] == np.nanmin(acc)
    sw = c.copy()
    sw[[nc.hi, nc.lo]] = sw[[nc.lo, nc.hi]]
    assert oracle.terrain_height(sw, nc.px, nc.py) == np.float32(-0.8)
    # the tie decides the mask: the +0.8 m point is carved (it is its own height), the other kept
    assert not keep[nc.hi] and keep[nc.lo]
    # every generated query ties too, and the lower z sorts into the earlier cell of any grid
    for x, y in g.queries:
        a = cc.flann_acc(c, x, y)
        assert a[nc.hi] == a[nc.lo] == np.nanmin(a)
    assert np.all(surf[:g.n_bottom, 2] == np.float32(np.float64(np.float32(0.8)) - g.depth))
    # the exact duplicate pair: same coordinates, different rgb, both kept
    assert np.array_equal(c[1, :3], c[3, :3]) and c[1, 4].view(np.uint32) != c[3, 4].view(np.uint32)
    assert keep[1] and keep[3]


def test_more_fallbacks_than_nearest_blocks(oracle):
    """C5: more than 4,096 queries (generated + candidate points) have no neighbour that passes
    both predicates, so the nearest-point kernel's blocks take more than one query each."""
    case = cc.fallback_case()
    c = case.cloud
    g = cc.geometry(case.t, case.q, case.kw)
    assert int((c[:, 2] > 0.7).sum()) >= 5000
    cand = cc.candidates(g, c)
    empty = sum(cc.neighbours(c, float(c[i, 0]), float(c[i, 1]), g.radius).size == 0
                for i in cand)
    empty += sum(cc.neighbours(c, x, y, g.radius).size == 0 for x, y in g.queries)
    assert empty > 4096
    keep, surf, area, _ = cc.reference(oracle, case)
    sheet = c[:, 2] > 0.7
    assert 0 < keep[sheet].sum() < sheet.sum()   # rim kept (ground nearest), middle carved
    assert surf.shape[0] > 0 and area.shape[0] > 0


@pytest.mark.parametrize("variant", ["flat", "lifted", "tiny"])
def test_points_exactly_at_the_radius(oracle, variant):
    """C6: at least 100 (query, point) pairs have acc == r2 in float, at least 100 queries lie
    on a multiple of r from the cloud's minimum corner; "lifted" also has acc two ulps past r2,
    and "lifted" / "tiny" have heights that change if an at-radius point is counted."""
    case = cc.radius_tie_case(variant)
    c = case.cloud
    g = cc.geometry(case.t, case.q, case.kw)
    assert g.radius == 0.5
    assert np.all(c[:, :2] * 8 == np.round(c[:, :2] * 8))
    r2 = np.float32(g.radius * g.radius)
    cand = cc.candidates(g, c)
    queries = [(float(c[i, 0]), float(c[i, 1])) for i in cand] + list(g.queries)
    mn = c[:, :2].min(axis=0).astype(np.float64)
    on, past, aligned, moved = 0, 0, 0, 0
    for x, y in queries:
        acc = cc.flann_acc(c, x, y)
        tie = acc == r2
        on += int(tie.sum())
        past += int((acc == r2 + np.float32(2.0 ** -24)).sum())   # 0.25 + (2^-12)^2: two ulps up
        aligned += ((x - mn[0]) / g.radius).is_integer() or ((y - mn[1]) / g.radius).is_integer()
        nb = cc.neighbours(c, x, y, g.radius)
        if tie.any() and nb.size:
            z, zt = c[nb, 2].astype(np.float64), c[tie, 2].astype(np.float64)
            moved += math.fsum(z) / z.size != math.fsum(np.concatenate([z, zt])) / (z.size + zt.size)
    assert on >= 100 and aligned >= 100
    if variant == "lifted":
        assert past >= 100
    if variant != "flat":
        assert moved >= 100
    keep, surf, area, _ = cc.reference(oracle, case)
    assert 0 < keep.sum() < keep.size and surf.shape[0] > 0 and area.shape[0] > 0


def test_layouts_hold_the_same_points():
    """C7: every layout holds the case's x, y, z at its offsets, the rgb values are distinct, and
    the expected rgb is the float at byte 16 for records of 20 bytes and more, else 0."""
    c = cc.layout_case().cloud
    assert np.unique(c[:, 4].view(np.uint32)).size == c.shape[0]
    assert np.isfinite(c[:, 4]).all()
    for layout in cc.LAYOUTS:
        raw, step, offs, want = cc.pack_layout(c, layout)
        assert raw.shape == (c.shape[0], step) and raw.dtype == np.uint8
        for a in range(3):
            got = raw[:, offs[a]:offs[a] + 4].copy().view(np.uint32)[:, 0]
            assert np.array_equal(got, c[:, a].view(np.uint32))
        if step >= 20:
            at16 = raw[:, 16:20].copy().view(np.uint32)[:, 0]
            assert np.array_equal(at16, want.view(np.uint32))
            assert np.array_equal(want.view(np.uint32), c[:, 4].view(np.uint32))
        else:
            assert not want.any()


def _seq_sum(z):
    s = 0.0
    for v in z:
        s += v
    return s


def test_sum_exact_case(oracle):
    """C8 (a): every z is a multiple of 2^-42 below 2^-5, no query has more than 1,024
    neighbours, and the exactly rounded sum equals the plain double sum in the reference's
    order for every generated query: the reference's mean is the exact sum's."""
    case = cc.sum_case("exact")
    c = case.cloud
    g = cc.geometry(case.t, case.q, case.kw)
    z64 = c[:, 2].astype(np.float64)
    assert np.all(z64 * 2.0 ** 42 == np.round(z64 * 2.0 ** 42)) and np.abs(z64).max() < 2.0 ** -5
    heights = []
    for x, y in g.queries:
        nb = cc.neighbours(c, x, y, g.radius)
        assert 0 < nb.size <= 1024
        assert math.fsum(z64[nb]) == _seq_sum(z64[nb])
        heights.append(math.fsum(z64[nb]) / nb.size)
        assert oracle.terrain_height(c, x, y, g.radius) == heights[-1]
    keep, surf, area, _ = cc.reference(oracle, case)
    # the restated recipes (geometry().drop / .area) give the oracle's generated records
    sz, az = cc.generated_z(g, heights)
    assert np.array_equal(sz.view(np.uint32), surf[:, 2].view(np.uint32))
    assert np.array_equal(az.view(np.uint32), area[:, 2].view(np.uint32))
    assert 0 < keep.sum() < keep.size and surf.shape[0] > 0 and area.shape[0] > 0


def test_sum_inexact_case(oracle):
    """C8 (b): the reference's sequential sum drops what the exact sum keeps: its mean differs
    from fsum(z) / m at the pit centre (the published pose height) and at 10 or more generated
    queries.  Both means are the same float, so every float output still agrees."""
    case = cc.sum_case("inexact")
    c = case.cloud
    g = cc.geometry(case.t, case.q, case.kw)
    z64 = c[:, 2].astype(np.float64)
    differ = []
    for x, y in g.queries:
        nb = cc.neighbours(c, x, y, g.radius)
        assert nb.size > 0
        ref = oracle.terrain_height(c, x, y, g.radius)
        assert ref == _seq_sum(z64[nb]) / nb.size   # the restated neighbour set and order
        differ.append(ref != math.fsum(z64[nb]) / nb.size)
    assert differ[0] and sum(differ) >= 10
    keep, surf, area, pose = cc.reference(oracle, case)
    assert pose[2] == oracle.terrain_height(c, g.cx, g.cy, g.radius)
    assert 0 < keep.sum() < keep.size and surf.shape[0] > 0 and area.shape[0] > 0
