"""tests/band_ref.py on the CPU: the checker of the thresholds' tight twin (DESIGN.md §5 Skip 7)
accepts a twin built from the rule with Python loops beside fine_ref's loop-built copy, and
reports every named mutation of it under the name of what the mutation breaks."""
import numpy as np
import pytest

import band_ref
import fine_ref


@pytest.fixture(scope="module")
def ref():
    pts, geo, dump = fine_ref.build_reference_copy(fine_ref.small_terrain())
    twin = band_ref.build_reference_twin(pts, geo, dump["frec"])
    twin.flags.writeable = False
    return pts, geo, dump["frec"], twin


def _records(geo, frec, twin):
    """(idx, spec, twin) words per (iz, wy, wx)."""
    idx, _ = fine_ref.record_index(geo)
    return idx, band_ref.spec_words(geo, frec)[idx].astype(np.int64), twin[idx].astype(np.int64)


def test_reference_twin_is_correct(ref):
    pts, geo, frec, twin = ref
    assert band_ref.check_band(pts, geo, frec, twin) == []
    idx, s, t = _records(geo, frec, twin)
    live = (s & 255) != 255
    # the terrain exercises the rule: records tighter than the specified copy on either side,
    # records the copy already bounds as tightly, unbounded ones, empty ones, padding
    assert ((t >> 8) < (s >> 8))[live].sum() > 50 and ((t & 255) > (s & 255))[live].sum() > 50
    assert ((t >> 8) == (s >> 8))[live].any() and ((t >> 8) == 255)[live].any()
    assert ((t & 255) == 0)[live].any() and (~live).any() and twin.size > idx.size
    assert (t[~live] == s[~live]).all()


def _first_where(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


# name of the mutation -> (what it does to the twin, the violation it must raise)
def _hi_lowered(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((t >> 8) < (s >> 8)) & ((t >> 8) > 1))
    twin[idx[k]] -= 1 << 8


def _lo_raised(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((t & 255) > (s & 255)) & ((t & 255) < 253))
    twin[idx[k]] += 1


def _hi_left_specified(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((t >> 8) + 1 < (s >> 8)))
    twin[idx[k]] = (t[k] & 255) | (s[k] & 0xFF00)


def _lo_left_specified(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((t & 255) > (s & 255) + 1))
    twin[idx[k]] = (s[k] & 255) | (t[k] & 0xFF00)


def _hi_looser_than_specified(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((s >> 8) < 255))
    twin[idx[k]] = (t[k] & 255) | (((s[k] >> 8) + 1) << 8)


def _lo_looser_than_specified(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) != 255) & ((s & 255) > 0))
    twin[idx[k]] = ((s[k] & 255) - 1) | (t[k] & 0xFF00)


def _clearance_code_dropped(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    k = _first_where(((s & 255) == 255) & ((s >> 8) > 0))
    twin[idx[k]] = 0x00FF


def _empty_record_coded(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    twin[idx[_first_where((s & 255) == 255)]] = 254


def _record_marked_empty(geo, frec, twin):
    idx, s, t = _records(geo, frec, twin)
    twin[idx[_first_where((s & 255) != 255)]] = 0x00FF


def _padding_touched(geo, frec, twin):
    idx, _ = fine_ref.record_index(geo)
    pad = np.ones(twin.size, bool)
    pad[idx.ravel()] = False
    twin[np.nonzero(pad)[0][0]] = 0x1000


def _full_reach_for_all(geo, frec, twin):
    # the specified rule under the twin's name: every entry reaches rho whatever its distance
    twin[:] = band_ref.spec_words(geo, frec)


def _truncated(geo, frec, twin):
    return twin[:-1]


MUTATIONS = {
    "hi_lowered": (_hi_lowered, "hi.sound"),
    "lo_raised": (_lo_raised, "lo.sound"),
    "hi_left_specified": (_hi_left_specified, "hi.tight"),
    "lo_left_specified": (_lo_left_specified, "lo.tight"),
    "hi_looser_than_specified": (_hi_looser_than_specified, "looser.hi"),
    "lo_looser_than_specified": (_lo_looser_than_specified, "looser.lo"),
    "clearance_code_dropped": (_clearance_code_dropped, "empty"),
    "empty_record_coded": (_empty_record_coded, "empty"),
    "record_marked_empty": (_record_marked_empty, "empty.flag"),
    "padding_touched": (_padding_touched, "padding"),
    "full_reach_for_all": (_full_reach_for_all, "hi.tight"),
    "truncated": (_truncated, "size"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_reported(ref, name):
    pts, geo, frec, twin = ref
    mutate, want = MUTATIONS[name]
    t = twin.copy()
    r = mutate(geo, frec, t)
    t = t if r is None else r
    out = band_ref.check_band(pts, geo, frec, t)
    names = [v.split(":")[0] for v in out]
    assert want in names, (name, out)
    if name.endswith("looser_than_specified"):       # (looser than the copy is not tight either)
        assert set(names) == {want, want.split(".")[1] + ".tight"}, (name, out)
    elif name not in ("full_reach_for_all", "truncated"):
        assert len(out) == 1, (name, out)            # one record wrong, one violation


def test_bounds_against_brute_force(ref):
    """real_bounds against the definition, one sampled record at a time: the highest and lowest
    height at which a query over the cell, or within m of it, can have an entry of the record
    within rho, scanned on a lattice of query positions.  No lattice query may pass the bound,
    and the bound lies within MISS steps of the lattice's extreme: a lattice point misses the
    position nearest an entry by at most half the lattice's diagonal, 0.7 mm, and the reach
    changes by g / reach <= 0.056 / 0.015 of that, 2.7 steps."""
    MISS = 3.0
    pts, geo, frec, twin = ref
    bhi, blo, part, has = band_ref.real_bounds(pts, geo)
    p = pts[:, :3].astype(np.float64)
    cz = np.clip(np.floor((p[:, 2] - geo["oz"]) * geo["inv_c"]), 0, geo["nz"] - 1)
    rho, cf, step = geo["r_q"] + band_ref.MU, geo["cf"], geo["zq"] * geo["c"]
    rng = np.random.default_rng(5)
    cand = np.argwhere(part)
    u = np.linspace(-band_ref.MARGIN_M, cf + band_ref.MARGIN_M, 65)
    for iz, wy, wx in cand[rng.choice(cand.shape[0], 40, replace=False)]:
        x0, y0 = geo["ox"] + wx * cf, geo["oy"] + wy * cf
        qx, qy = (a.ravel() for a in np.meshgrid(x0 + u, y0 + u))
        gx, gy = fine_ref._rect_gap(x0, cf, 0.0, qx), fine_ref._rect_gap(y0, cf, 0.0, qy)
        keep = gx * gx + gy * gy <= band_ref.MARGIN_M ** 2
        qx, qy = qx[keep], qy[keep]
        dx, dy = fine_ref._rect_gap(x0, cf, 0.0, p[:, 0]), fine_ref._rect_gap(y0, cf, 0.0, p[:, 1])
        mem = p[(cz >= iz) & (cz <= iz + 1) & (dx * dx + dy * dy <= geo["R2"])]
        h2 = (qx[:, None] - mem[:, 0]) ** 2 + (qy[:, None] - mem[:, 1]) ** 2
        reach = np.sqrt(np.maximum(rho * rho - h2, 0.0))
        near = h2 < rho * rho
        zb = geo["oz"] + iz * geo["c"]
        top = (np.where(near, mem[:, 2] + reach, -np.inf).max() - zb) / step + 1.0
        bot = (np.where(near, mem[:, 2] - reach, np.inf).min() - zb) / step - 1.0
        assert bhi[iz, wy, wx] - MISS <= top <= bhi[iz, wy, wx] + band_ref.EPS
        assert blo[iz, wy, wx] + MISS >= bot >= blo[iz, wy, wx] - band_ref.EPS
