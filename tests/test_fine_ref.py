"""The fine copy's checker (tests/fine_ref.py) checked itself, without a GPU: it accepts a correct
dump of a 24 x 20 fine-cell terrain in every layout, and reports each single fault below under
the name of the field that is wrong -- the proof that tests/test_fine_copy_gpu.py can fail."""
import numpy as np
import pytest

import fine_ref
from fine_ref import build_reference_copy, check_fine_copy, decode_records, record_index


@pytest.fixture(scope="module")
def good():
    """The default layout's dump (split records in 8 x 8 tiles, two skips, packed entries) and
    its decoded records; never modified."""
    pts, geo, dump = build_reference_copy(fine_ref.small_terrain())
    assert (geo["fnx"], geo["fny"]) == (24, 20) and geo["rz"] >= 4
    for a in dump.values():
        a.setflags(write=False)
    return pts, geo, dump, decode_records(geo, dump["frec"])


def _fields(violations):
    return sorted({v.split(":")[0] for v in violations})


def _mutated(good, band=None, start=None, at=None, slot=None):
    """A copy of the dump with record `at` = (iz, wy, wx) given a new threshold word and / or
    start word (functions of the old word); `slot`: the record slot written instead of at's."""
    pts, geo, dump, _ = good
    frec = dump["frec"].copy()
    idx, nrec = record_index(geo)
    k = int(idx[at]) if slot is None else slot
    bw = frec[:2 * nrec].view(np.uint16)
    sw = frec[geo["start_off"]:].view(np.uint32)
    if band is not None:
        bw[k] = band(int(bw[int(idx[at])]))
    if start is not None:
        sw[k] = start(int(sw[int(idx[at])]))
    return check_fine_copy(pts, geo, {"frec": frec, "wpts": dump["wpts"]})


def _pick(mask):
    assert mask.any()
    return tuple(int(v) for v in np.argwhere(mask)[mask.sum() // 2])


def _entries(good):
    pts, geo, dump, _ = good
    return dump["wpts"].copy().view(np.float32).reshape(-1, 3)


def _check_entries(good, ent):
    pts, geo, dump, _ = good
    return check_fine_copy(pts, geo, {"frec": dump["frec"], "wpts": ent.view(np.uint8).ravel()})


def _long_run(good):
    """(first entry, length) of the longest run (the wall's: many heights, and ties too)."""
    ent = _entries(good)
    sent = np.nonzero(np.isnan(ent[:, 0]))[0]
    begin = np.concatenate([[0], sent[:-1] + 1])
    k = int(np.argmax(sent - begin))
    assert sent[k] - begin[k] >= 3
    return int(begin[k]), int(sent[k] - begin[k])


def test_accepts_the_correct_dump(good):
    pts, geo, dump, _ = good
    assert check_fine_copy(pts, geo, dump) == []


@pytest.mark.parametrize("kw", [dict(tile=0), dict(tile=1), dict(skip=1), dict(packed=False),
                                dict(F=3), dict(F=4, tile=1, packed=False)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_accepts_every_layout(kw):
    pts, geo, dump = build_reference_copy(fine_ref.small_terrain(), **kw)
    assert check_fine_copy(pts, geo, dump) == []


def test_the_small_terrain_exercises_every_feature(good):
    """The non-vacuity conditions of the GPU tests, on the builder's dump."""
    _, geo, dump, _ = good
    f = fine_ref.features(geo, dump["frec"])
    assert f["empty"] > 0 and f["nonempty"] > 0
    assert f["hi_saturated"] > 0 and f["lo_zero"] > 0 and f["hi_bounded"] > 0 and f["lo_bounded"] > 0
    assert all(v > 0 for v in f["skip_below_cap"]) and all(v > 0 for v in f["skip_at_cap"])
    assert f["code_ge2"] > 0


def test_the_wall_terrain_exercises_every_feature():
    """The GPU suite's wall scene (without its edge points), from the builder: both skip caps
    are reached, and every other kind of record occurs."""
    pts, geo, dump = build_reference_copy(fine_ref.wall_terrain())
    assert check_fine_copy(pts, geo, dump) == []
    f = fine_ref.features(geo, dump["frec"])
    assert f["empty"] > 0 and f["nonempty"] > 0 and f["hi_saturated"] > 0 and f["lo_zero"] > 0
    assert all(v > 0 for v in f["skip_below_cap"]) and all(v > 0 for v in f["skip_at_cap"])
    assert f["code_ge2"] > 0


@pytest.mark.parametrize("delta", [+1, -1])
def test_reports_a_clearance_code_off_by_one(good, delta):
    _, geo, _, rec = good
    inner = (rec["lo"] == 255) & ~fine_ref.border_mask(geo)
    at = _pick(inner & (rec["hi"] >= 2) & (rec["hi"] < 250))
    v = _mutated(good, band=lambda b: b + (delta << 8), at=at)
    # (the point-list sample allows one cell either way, so it may or may not object as well)
    assert "clear.code" in _fields(v) and set(_fields(v)) <= {
        "clear.code", "clear.sample.hard" if delta > 0 else "clear.sample.tight"}, v


def test_the_point_list_rejects_a_code_two_too_large(good):
    _, geo, _, rec = good
    inner = (rec["lo"] == 255) & ~fine_ref.border_mask(geo)
    at = _pick(inner & (rec["hi"] >= 2) & (rec["hi"] < 250))
    v = _mutated(good, band=lambda b: b + (2 << 8), at=at)
    assert {"clear.code", "clear.sample.hard"} <= set(_fields(v)), v
    v = _mutated(good, band=lambda b: b - (2 << 8), at=at)
    assert {"clear.code", "clear.sample.tight"} <= set(_fields(v)), v


def test_reports_a_border_code(good):
    _, geo, _, rec = good
    at = _pick((rec["lo"] == 255) & fine_ref.border_mask(geo))
    assert _fields(_mutated(good, band=lambda b: b | (1 << 8), at=at)) == ["clear.border"]


@pytest.mark.parametrize("delta", [+1, -1])
@pytest.mark.parametrize("which", [0, 1])
def test_reports_a_skip_count_off_by_one(good, delta, which):
    _, _, _, rec = good
    s, cap, shift = rec["skips"][which], (15, 7)[which], (25, 29)[which]
    at = _pick((s > 0) & (s < cap))
    v = _mutated(good, start=lambda w: w + (delta << shift), at=at)
    assert _fields(v) == [f"skip.{(1.375, 1.6875)[which]}"], v


@pytest.mark.parametrize("delta", [+1, -1])
def test_reports_a_walk_start_off_by_one(good, delta):
    _, _, _, rec = good
    at = _pick(rec["start"] > 0)
    assert _fields(_mutated(good, start=lambda w: w + delta, at=at)) == ["start"]


def test_reports_a_high_threshold_one_too_low(good):
    _, _, _, rec = good
    at = _pick((rec["lo"] != 255) & (rec["hi"] < 255))
    assert _fields(_mutated(good, band=lambda b: b - (1 << 8), at=at)) == ["band.hi.sound"]


def test_reports_a_low_threshold_one_too_high(good):
    _, _, _, rec = good
    at = _pick((rec["lo"] != 255) & (rec["lo"] > 0))
    assert _fields(_mutated(good, band=lambda b: b + 1, at=at)) == ["band.lo.sound"]


def test_reports_thresholds_wider_than_three_steps(good):
    _, _, _, rec = good
    at = _pick((rec["lo"] != 255) & (rec["lo"] > 8) & (rec["hi"] < 240))
    assert _fields(_mutated(good, band=lambda b: b + (4 << 8), at=at)) == ["band.hi.tight"]
    assert _fields(_mutated(good, band=lambda b: b - 4, at=at)) == ["band.lo.tight"]
    assert _fields(_mutated(good, band=lambda b: b | 0xFF00, at=at)) == ["band.hi.tight"]
    assert _fields(_mutated(good, band=lambda b: b & 0xFF00, at=at)) == ["band.lo.tight"]


def test_reports_an_empty_record_marked_non_empty(good):
    _, _, _, rec = good
    at = _pick(rec["lo"] == 255)
    assert "empty" in _fields(_mutated(good, band=lambda b: 0xFF00, at=at))
    at = _pick(rec["lo"] != 255)
    assert "empty" in _fields(_mutated(good, band=lambda b: 0x00FF, at=at))


def test_reports_two_swapped_entries(good):
    ent = _entries(good)
    b, n = _long_run(good)
    ent[[b, b + 1]] = ent[[b + 1, b]]
    assert _fields(_check_entries(good, ent)) == ["wpts.order"]


def test_reports_a_dropped_entry(good):
    """The rest of the run moves up and its sentinel comes one entry early."""
    ent = _entries(good)
    b, n = _long_run(good)
    ent[b + 1:b + n] = ent[b + 2:b + n + 1].copy()
    assert _fields(_check_entries(good, ent)) == ["wpts.members"]
    # and an entry missing from the buffer altogether
    v = _check_entries(good, np.delete(_entries(good), b + 1, axis=0))
    assert _fields(v) == ["wpts.count"]


def test_reports_an_overwritten_sentinel(good):
    ent = _entries(good)
    b, n = _long_run(good)
    ent[b + n] = ent[b + n - 1]
    assert _fields(_check_entries(good, ent)) == ["wpts.sentinel"]
    ent = _entries(good)
    ent[b + n, 2] = np.float32(-1e30)    # finite z alone
    assert _fields(_check_entries(good, ent)) == ["wpts.sentinel"]


def test_reports_a_record_at_its_x_fastest_position(good):
    """A record of the tiled dump written where the x-fastest layout would put it lands in
    another record's slot: that record's fields are reported."""
    _, geo, _, rec = good
    idx, _ = record_index(geo)
    nw = geo["fnx"] * geo["fny"]
    iz, wy, wx = at = _pick((rec["lo"] != 255) & (rec["start"] > 0))
    slot = iz * nw + wy * geo["fnx"] + wx
    assert slot != idx[at]
    hit = np.argwhere(idx == slot)
    v = _mutated(good, band=lambda b: b, start=lambda w: w, at=at, slot=slot)
    if hit.size:    # another window's record was overwritten
        z2, y2, x2 = (int(a) for a in hit[0])
        assert rec["start"][z2, y2, x2] != rec["start"][at]
        assert any(s.startswith("start:") and f"({x2}, {y2}, {z2})" in s for s in v), v
    else:
        assert _fields(v) == ["frec.padding"], v


def test_reports_a_padding_record(good):
    pts, geo, dump, _ = good
    idx, nrec = record_index(geo)
    pad = np.ones(nrec, bool)
    pad[idx.ravel()] = False
    assert pad.sum() == (24 * 24 - 24 * 20) * geo["rz"]
    frec = dump["frec"].copy()
    frec[:2 * nrec].view(np.uint16)[np.nonzero(pad)[0][7]] = 0x01FF
    assert _fields(check_fine_copy(pts, geo, {"frec": frec, "wpts": dump["wpts"]})) == \
        ["frec.padding"]


def test_reports_a_point_missing_from_the_index(good):
    """The runs are checked against the point list: with one more point in it, the windows
    around that point lack a member."""
    pts, geo, dump, _ = good
    more = np.concatenate([pts, pts[:1] + np.float32([0.01, 0.01, 0.0, 0.0])], 0)
    g2 = dict(geo, n_points=geo["n_points"] + 1)
    assert "wpts.count" in _fields(check_fine_copy(more, g2, dump))


def test_reports_wrong_geometry(good):
    pts, geo, dump, _ = good
    assert _fields(check_fine_copy(pts, dict(geo, tsteps=geo["tsteps"] - 1), dump)) == \
        ["geo.tsteps"]
    assert "geo.R2" in _fields(check_fine_copy(pts, dict(geo, R2=geo["r_q"] ** 2), dump))
