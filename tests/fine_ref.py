"""The fine-window copy of the terrain index (pcp_fine.hip) checked against its
specification in plain numpy, float64, from the index's own points.

check_fine_copy(points, geo, dump) takes what Context.debug_fine_copy() returns -- the index's
float4 points, the geometry the build kernels received, and the raw bytes of the record and
entry buffers -- and returns a list of violations, one string per field that is wrong, each
beginning with the field's name.  Every expectation is derived from the meaning of the field:
the membership of a window, the order of its run, what a walk start, a threshold, a skip count
and a clearance code promise to the march.  The layout (tiles, split arrays, padding, packing)
is decoded here from its description, so it is checked as well.

build_reference_copy() makes a correct dump from the same specification with Python loops, one
window and one record at a time (small terrains only): the CPU tests mutate it to prove that
the checker reports each kind of fault, and read the features a terrain exercises from it.

No GPU and no ctypes here."""
import math

import numpy as np

MARGIN_R = 1e-3      # the windows' margin: R = r_q + 1 mm
MARGIN_T = 2e-3      # the thresholds' margin: r_q + 2 mm
CLEAR_MAX = 255      # the clearance code saturates: "at least 255 cells"
SKIP_H = {2: ((1.375, 15), (1.6875, 7)), 1: ((1.5, 15),)}   # skip mode: (height in cells, cap)


# ---- layout ---------------------------------------------------------------------------------

def record_index(geo):
    """Index of record (iz, wy, wx) in the record arrays, as an (rz, fny, fnx) array, and the
    number of records with the tiles' padding: x-fastest (tile 0), or T x T xy tiles of
    consecutive records, T = 4 (tile 1) or 8 (tile 2), tile rows x-fastest, one plane per iz."""
    fnx, fny, rz, tile = geo["fnx"], geo["fny"], geo["rz"], geo["tile"]
    wx = np.arange(fnx, dtype=np.int64)[None, :]
    wy = np.arange(fny, dtype=np.int64)[:, None]
    if tile == 0:
        base, plane = wy * fnx + wx, fnx * fny
    else:
        T = 8 if tile == 2 else 4
        tx, ty = -(-fnx // T), -(-fny // T)
        base = ((wy // T) * tx + wx // T) * (T * T) + (wy % T) * T + wx % T
        plane = tx * ty * T * T
    return np.arange(rz, dtype=np.int64)[:, None, None] * plane + base[None], plane * rz


def record_sizes(geo):
    """(start_off, frec_bytes) of the record buffer: split arrays (tile 2: uint16 thresholds,
    padded to 256 bytes, then uint32 walk starts) or 8-byte records."""
    _, nrec = record_index(geo)
    if geo["tile"] == 2:
        off = (nrec * 2 + 255) & ~255
        return off, off + nrec * 4
    return 0, nrec * 8


def raw_records(geo, frec):
    """The record buffer as (start words, threshold words), one per record slot."""
    _, nrec = record_index(geo)
    off, _ = record_sizes(geo)
    if geo["tile"] == 2:
        return (frec[off:off + 4 * nrec].view(np.uint32),
                frec[:2 * nrec].view(np.uint16).astype(np.uint32))
    rec = frec[:8 * nrec].view(np.uint32).reshape(nrec, 2)
    return rec[:, 0], rec[:, 1]


def decode_records(geo, frec):
    """The fields of every record as (rz, fny, fnx) arrays: start, lo, hi, band (the whole
    threshold word), skips (one array per skip height), and pad_start / pad_band, the words of
    the slots that belong to no window."""
    idx, nrec = record_index(geo)
    sw_all, bw_all = raw_records(geo, frec)
    sw, bw = sw_all[idx].astype(np.int64), bw_all[idx].astype(np.int64)
    out = {"band": bw, "lo": bw & 255, "hi": (bw >> 8) & 255, "skips": []}
    if geo["tile"] == 2:
        bits = 25 if geo["skip"] == 2 else 28
        out["start"] = sw & ((1 << bits) - 1)
        if geo["skip"] == 2:
            out["skips"] = [(sw >> 25) & 15, (sw >> 29) & 7]
        else:
            out["skips"] = [(sw >> 28) & 15]
    else:
        out["start"] = sw
    pad = np.ones(nrec, bool)
    pad[idx.ravel()] = False
    out["pad_start"], out["pad_band"] = sw_all[pad], bw_all[pad]
    return out


def border_mask(geo):
    """fan_clear_border: the grid's outermost cells and levels, (rz, fny, fnx)."""
    fnx, fny, rz = geo["fnx"], geo["fny"], geo["rz"]
    m = np.zeros((rz, fny, fnx), bool)
    m[[0, rz - 1]] = True
    m[:, [0, fny - 1]] = True
    m[:, :, [0, fnx - 1]] = True
    return m


def features(geo, frec):
    """What a dump exercises (the GPU tests' non-vacuity conditions), from the records alone."""
    r = decode_records(geo, frec)
    empty = r["lo"] == 255
    f = {"empty": int(empty.sum()), "nonempty": int((~empty).sum()),
         "hi_saturated": int((~empty & (r["hi"] == 255)).sum()),
         "lo_zero": int((~empty & (r["lo"] == 0)).sum()),
         "hi_bounded": int((~empty & (r["hi"] < 255)).sum()),
         "lo_bounded": int((~empty & (r["lo"] > 0)).sum())}
    if geo["tile"] == 2:
        caps = [cap for _, cap in SKIP_H[geo["skip"]]]
        f["skip_below_cap"] = [int(((s > 0) & (s < cap)).sum()) for s, cap in zip(r["skips"], caps)]
        f["skip_at_cap"] = [int((s == cap).sum()) for s, cap in zip(r["skips"], caps)]
        inner = empty & ~border_mask(geo)
        f["empty_interior"] = int(inner.sum())
        f["codes"] = np.bincount(r["hi"][inner], minlength=256)
        f["code_ge1"] = int(f["codes"][1:].sum())
        f["code_ge2"] = int(f["codes"][2:].sum())
    return f


# ---- the specification, vectorised --------------------------------------------------------------

def _rect_gap(o, cf, w, p):
    """Distance along one axis from coordinate p to fine cell w's interval [o + w cf, + cf]."""
    x0 = o + w * cf
    return np.maximum(np.maximum(x0 - p, p - (x0 + cf)), 0.0)


def _window_pairs(geo, x, y):
    """(window, point) for every point whose xy distance to the window's rectangle is <= R.
    Every window within reach + 1 cells of the point's own cell is tried (one more ring than
    the build tries, so a reach that is too small shows as a missing member)."""
    fnx, fny, cf = geo["fnx"], geo["fny"], geo["cf"]
    cx = np.clip(np.floor((x - geo["ox"]) * geo["inv_cf"]), 0, fnx - 1).astype(np.int64)
    cy = np.clip(np.floor((y - geo["oy"]) * geo["inv_cf"]), 0, fny - 1).astype(np.int64)
    rr = int(math.ceil(math.sqrt(geo["R2"]) / cf)) + 1
    ws, ps = [], []
    for oy in range(-rr, rr + 1):
        for ox in range(-rr, rr + 1):
            wx, wy = cx + ox, cy + oy
            dx = _rect_gap(geo["ox"], cf, wx.astype(np.float64), x)
            dy = _rect_gap(geo["oy"], cf, wy.astype(np.float64), y)
            inw = ((wx >= 0) & (wx < fnx) & (wy >= 0) & (wy < fny) & (dx * dx + dy * dy <= geo["R2"]))
            p = np.nonzero(inw)[0]
            ws.append((wy * fnx + wx)[p])
            ps.append(p)
    return np.concatenate(ws), np.concatenate(ps), cx, cy


def _chebyshev(occ, cap):
    """Cells (Chebyshev) from every cell to the nearest True cell of `occ`, cap + 1 when none
    lies within cap: the smallest d whose (2 d + 1)^2 box holds one, found by bisection over
    box sums of an integral image."""
    ny, nx = occ.shape
    S = np.zeros((ny + 1, nx + 1), np.int64)
    S[1:, 1:] = occ.astype(np.int64).cumsum(0).cumsum(1)
    Y, X = np.mgrid[0:ny, 0:nx]
    lo, hi = np.zeros(occ.shape, np.int64), np.full(occ.shape, cap + 1, np.int64)
    while (lo < hi).any():
        mid = (lo + hi) // 2
        y0, y1 = np.maximum(Y - mid, 0), np.minimum(Y + mid + 1, ny)
        x0, x1 = np.maximum(X - mid, 0), np.minimum(X + mid + 1, nx)
        any_ = (S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]) > 0
        found = any_ & (mid <= cap)
        hi = np.where(found, mid, hi)
        lo = np.where(found, lo, np.minimum(mid + 1, hi))
    return lo


def _first(mask):
    """(iz, wy, wx) of the first True of an (rz, fny, fnx) mask."""
    return tuple(int(v) for v in np.argwhere(mask)[0])


def _geo_violations(geo):
    out = []
    R = geo["r_q"] + MARGIN_R
    zabs = max(abs(geo["oz"]), abs(geo["oz"] + float(geo["nz"]) * geo["c"]))
    want = {"inv_c": 1.0 / geo["c"], "cf": geo["c"] / geo["F"], "inv_cf": geo["F"] * geo["inv_c"],
            "R2": R * R, "reach": math.ceil(R / geo["cf"]), "fnx": geo["F"] * geo["nx"],
            "fny": geo["F"] * geo["ny"], "rz": geo["nz"] - 1,
            "zq": float(np.float32(2.0) / np.float32(250.0)),
            "tsteps": math.ceil((geo["r_q"] + MARGIN_T) / geo["c"] / geo["zq"]),
            "clear_c": geo["c"],
            "clear_zt0": geo["oz"] + geo["c"] + 2.0 * R + zabs * (1.0 / 1048576.0)}
    for k, v in want.items():
        if geo[k] != v:
            out.append(f"geo.{k}: got {geo[k]!r}, expected {v!r}")
    return out


def check_fine_copy(points, geo, dump, sample=2000, seed=0, edge_ulps=4.0):
    """Violations of the fine copy's specification in `dump` = {"frec": uint8
    bytes, "wpts": uint8 bytes}, for the index's `points` ((n, 4) float32, original index bits
    in column 3) and the geometry `geo`.  [] when the copy is correct.  sample, seed: the
    records whose clearance code is checked against the point list; edge_ulps: the rounding of
    a cell edge that check allows (see there)."""
    out = _geo_violations(geo)
    fnx, fny, rz, nz, tile = geo["fnx"], geo["fny"], geo["rz"], geo["nz"], geo["tile"]
    nw = fnx * fny
    pts = np.ascontiguousarray(points, np.float32)
    if pts.shape != (geo["n_points"], 4):
        return out + [f"geo.n_points: {geo['n_points']} against points of shape {pts.shape}"]
    orig = pts[:, 3].copy().view(np.uint32).astype(np.int64)
    x, y, z = (pts[:, a].astype(np.float64) for a in range(3))

    # ---- runs: members, order, sentinels, placement ----------------------------------------
    wk, pk, cx, cy = _window_pairs(geo, x, y)
    order = np.lexsort((orig[pk], -z[pk], wk))        # window, descending z, original index
    wk, pk = wk[order], pk[order]
    cnt = np.bincount(wk, minlength=nw)
    cstart = np.concatenate([[0], np.cumsum(cnt)])
    begin = cstart[:-1] + np.arange(nw)               # run w begins at cstart[w] + w
    sent = cstart[1:] + np.arange(nw)                 # and its sentinel follows its last entry
    pos = np.arange(wk.size) + wk
    nent = wk.size + nw
    esz = 12 if geo["packed"] else 16
    wbytes = dump["wpts"]
    if geo["n_entries"] != nent or wbytes.size != nent * esz:
        return out + [f"wpts.count: {geo['n_entries']} entries in {wbytes.size} bytes, expected "
                      f"{nent} entries of {esz} bytes"]
    ent = wbytes.view(np.float32).reshape(nent, esz // 4)
    exp = np.empty((nent, 3), np.float32)
    exp[pos] = pts[pk, :3]
    exp[sent] = (np.nan, np.nan, -np.inf)
    ewin = np.empty(nent, np.int64)
    ewin[pos], ewin[sent] = wk, np.arange(nw)
    s = ent[sent]
    bad = ~(np.isnan(s[:, 0]) & np.isnan(s[:, 1]) & (s[:, 2] == -np.inf))
    if bad.any():
        w = int(np.nonzero(bad)[0][0])
        out.append(f"wpts.sentinel: {int(bad.sum())} windows, first ({w % fnx}, {w // fnx}) at "
                   f"entry {int(sent[w])}: got {s[w, :3].tolist()}")
    diff = (ent[pos, :3] != exp[pos]).any(1)
    if diff.any():
        # the same entries in another order, or other entries
        gb = np.ascontiguousarray(ent[pos, :3]).view(np.uint32).astype(np.int64)
        eb = np.ascontiguousarray(exp[pos]).view(np.uint32).astype(np.int64)
        gs = gb[np.lexsort((gb[:, 2], gb[:, 1], gb[:, 0], wk))]
        es = eb[np.lexsort((eb[:, 2], eb[:, 1], eb[:, 0], wk))]
        wrong_set = np.zeros(nw, bool)
        wrong_set[wk[(gs != es).any(1)]] = True
        for name, sel in (("members", wrong_set[wk] & diff), ("order", ~wrong_set[wk] & diff)):
            if sel.any():
                k = int(np.nonzero(sel)[0][0])
                out.append(f"wpts.{name}: {int(sel.sum())} entries, first in window "
                           f"({int(wk[k]) % fnx}, {int(wk[k]) // fnx}) at entry {int(pos[k])}: got "
                           f"{ent[pos[k], :3].tolist()}, expected {exp[pos[k]].tolist()}")
    if not geo["packed"]:
        gi = np.ascontiguousarray(ent[pos, 3]).view(np.uint32).astype(np.int64)
        bad = gi != orig[pk]
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            out.append(f"wpts.index: {int(bad.sum())} entries, first at entry {int(pos[k])}: got "
                       f"{int(gi[k])}, expected {int(orig[pk[k]])}")

    # ---- records -------------------------------------------------------------------------
    _, nrec = record_index(geo)
    start_off, frec_bytes = record_sizes(geo)
    if (geo["n_records"] != nrec or geo["start_off"] != start_off or
            geo["frec_bytes"] != frec_bytes or dump["frec"].size != frec_bytes):
        return out + [f"frec.size: {geo['n_records']} records, start_off {geo['start_off']}, "
                      f"{dump['frec'].size} bytes; expected {nrec}, {start_off}, {frec_bytes}"]
    if nent >= 1 << (32 if tile != 2 else 25 if geo["skip"] == 2 else 28):
        out.append(f"start.width: {nent} entries do not fit the walk start's bits")
    rec = decode_records(geo, dump["frec"])
    bad = (rec["pad_start"] != 0) | (rec["pad_band"] != 0x00FF)
    if bad.any():
        out.append(f"frec.padding: {int(bad.sum())} padding records are not {{0, 0x00FF}}")

    def report(field, mask, got=None, want=None, extra=""):
        if not mask.any():
            return
        iz, wy, wx = _first(mask)
        txt = f"{field}: {int(mask.sum())} records, first (wx, wy, iz) = ({wx}, {wy}, {iz})"
        if got is not None:
            txt += f": got {got[iz, wy, wx]}"
        if want is not None:
            txt += f", expected {want[iz, wy, wx]}"
        out.append(txt + extra)

    shape = (rz, fny, fnx)
    zk = z[pk]
    czk = np.clip(np.floor((zk - geo["oz"]) * geo["inv_c"]), 0, nz - 1).astype(np.int64)
    above = np.empty((rz, nw), np.int64)    # entries of the run in coarse z cells > iz + 1
    inband = np.empty((rz, nw), np.int64)   # entries in coarse z cells iz, iz + 1
    nskip = [np.empty((rz, nw), np.int64) for _ in rec["skips"]]
    for iz in range(rz):                    # (a loop over levels, never over records)
        above[iz] = np.bincount(wk, weights=czk > iz + 1, minlength=nw)
        walk = czk <= iz + 1                # the entries from the walk start on
        inband[iz] = np.bincount(wk, weights=walk & (czk >= iz), minlength=nw)
        for a, (h, cap) in zip(nskip, SKIP_H[geo["skip"]] if tile == 2 else ()):
            thr = geo["oz"] + (float(iz) + h) * geo["c"]
            a[iz] = np.minimum(np.bincount(wk, weights=walk & (zk >= thr), minlength=nw), cap)
    want_start = (begin[None, :] + above).reshape(shape)
    report("start", rec["start"] != want_start, rec["start"], want_start)
    has = inband.reshape(shape) > 0
    flagged = rec["lo"] == 255
    report("empty", flagged != ~has, rec["lo"], None,
           " (the low threshold byte is 255 if and only if the record is empty)")
    if tile != 2:
        report("empty.hi", flagged & ~has & (rec["band"] != 0x00FF), rec["band"])
        report("band.word", rec["band"] >= 1 << 16, rec["band"])
    for sgot, swant, (h, _) in zip(rec["skips"], nskip, SKIP_H[geo["skip"]] if tile == 2 else ()):
        swant = swant.reshape(shape)
        report(f"skip.{h}", sgot != swant, sgot, swant)

    # thresholds of the non-empty records
    zexp = exp[:, 2].astype(np.float64)
    live = has & ~flagged
    first = np.where(has, want_start, 0)
    zmax = zexp[first]
    zmin = zexp[np.where(has, want_start + inband.reshape(shape) - 1, 0)]
    zb = geo["oz"] + np.arange(rz, dtype=np.float64)[:, None, None] * geo["c"]
    step = geo["zq"] * geo["c"]
    lo, hi = rec["lo"].astype(np.float64), rec["hi"].astype(np.float64)
    top = zmax + geo["r_q"] + MARGIN_T
    bot = zmin - geo["r_q"] - MARGIN_T
    report("band.hi.sound", live & (rec["hi"] != 255) & ~(zb + hi * step >= top), rec["hi"])
    report("band.lo.sound", live & (rec["lo"] != 0) & ~(zb + lo * step <= bot), rec["lo"])
    report("band.hi.tight", live & ~(hi - (top - zb) / step <= 3.0), rec["hi"],
           np.ceil((top - zb) / step))
    report("band.lo.tight", live & ~((bot - zb) / step - lo <= 3.0), rec["lo"],
           np.floor((bot - zb) / step))
    report("band.order", live & (rec["lo"] > rec["hi"]), rec["band"])
    if tile != 2:
        return out

    # ---- clearance codes of the empty split records ------------------------------------------
    zt = geo["clear_zt0"] + np.arange(rz, dtype=np.float64) * geo["clear_c"]     # Zt(iz)
    plev = (z[:, None] > zt[None, :]).sum(1)          # lowest level at which the point counts
    lev = np.full(nw, rz, np.int64)
    np.minimum.at(lev, cy * fnx + cx, plev)           # a cell's level: that of its lowest point
    want_code = np.empty(shape, np.int64)
    for iz in range(rz):
        D = _chebyshev((lev <= iz).reshape(fny, fnx), CLEAR_MAX + 1)
        want_code[iz] = np.where(D == 0, 0, np.minimum(D - 1, CLEAR_MAX))
    border = border_mask(geo)
    empty = flagged & ~has
    report("clear.border", empty & border & (rec["hi"] != 0), rec["hi"])
    inner = empty & ~border
    report("clear.code", inner & (rec["hi"] != want_code), rec["hi"], want_code)
    # a sample against the point list itself: the largest e <= 255 such that no point with
    # z <= Zt(iz) lies closer than e cf (Chebyshev) to the rectangle
    # ("no closer" in real numbers: a point that lies on a cell edge belongs to the cell above
    # it and is exactly D cf from a rectangle D cells below, but the rectangle's double edges
    # (ox + w cf) + cf and the point's cell floor((p - ox) / cf) each round by an ulp of the
    # coordinate, so the double distance can come out an ulp short of D cf.  eps = 4 ulps of
    # the grid's largest coordinate, 1e-15 m near the origin and 3e-12 m at 3 km, is that
    # rounding; the march keeps r + 1 mm in hand, rb of pcp_fan_clear.hpp.)
    eps = edge_ulps * 2.0 ** -52 * max(abs(geo["ox"]), abs(geo["ox"] + fnx * geo["cf"]),
                           abs(geo["oy"]), abs(geo["oy"] + fny * geo["cf"]))
    cand = np.argwhere(inner)
    if cand.size:
        rng = np.random.default_rng(seed)
        pick = cand[rng.choice(cand.shape[0], min(sample, cand.shape[0]), replace=False)]
        e = np.empty(pick.shape[0], np.int64)
        for a in range(0, pick.shape[0], 64):
            iz, wy, wx = (pick[a:a + 64, k] for k in range(3))
            dx = _rect_gap(geo["ox"], geo["cf"], wx.astype(np.float64)[:, None], x[None, :])
            dy = _rect_gap(geo["oy"], geo["cf"], wy.astype(np.float64)[:, None], y[None, :])
            d = np.where(z[None, :] <= zt[iz][:, None], np.maximum(dx, dy), np.inf).min(1)
            e[a:a + 64] = np.minimum(np.floor((d + eps) / geo["cf"]), CLEAR_MAX)
        code = rec["hi"][pick[:, 0], pick[:, 1], pick[:, 2]]
        for name, bad in (("clear.sample.hard", code > e), ("clear.sample.tight", code < e - 1)):
            if bad.any():
                k = int(np.nonzero(bad)[0][0])
                iz, wy, wx = (int(v) for v in pick[k])
                out.append(f"{name}: {int(bad.sum())} of {pick.shape[0]} sampled records, first "
                           f"(wx, wy, iz) = ({wx}, {wy}, {iz}): code {int(code[k])}, the point "
                           f"list allows {int(e[k])}")
    return out


# ---- terrains the CPU and GPU tests share ---------------------------------------------------------

def sheet(x0, x1, y0, y1, z, d=0.05):
    """A flat lattice of points, spacing d, over [x0, x1) x [y0, y1) at height z: (n, 3)."""
    X, Y = np.meshgrid(np.arange(x0, x1 - 1e-9, d), np.arange(y0, y1 - 1e-9, d))
    return np.stack([X.ravel(), Y.ravel(), np.full(X.size, float(z))], 1)


def wall(x, y0, y1, z0, height, per_step=60, d=0.05):
    """A vertical wall in the plane x = const: per_step points per d of length, spread evenly
    over `height` above z0."""
    Y, Z = np.meshgrid(np.arange(y0, y1 - 1e-9, d), z0 + height * np.arange(per_step) / per_step)
    return np.stack([np.full(Y.size, float(x)), Y.ravel(), Z.ravel()], 1)


def small_terrain():
    """24 x 20 fine cells at F = 2 (12 x 10 coarse cells with the padding: no multiple of 8): a
    sheet at z = 0, a second one 0.6 m below half of it, and a wall of 0.36 m across it."""
    return np.concatenate([sheet(0.0, 1.15, 0.0, 0.9, 0.0), sheet(0.0, 0.55, 0.0, 0.9, -0.6),
                           wall(0.8, 0.2, 0.7, 0.0, 0.36)], 0).astype(np.float32)


def wall_terrain(size=3.0):
    """The GPU suite's wall scene: a size x size sheet, a second sheet 0.6 m below half of it,
    and a wall of 60 points per 0.05 m spread over 0.36 m of height, so single windows hold far
    more than 15 entries above every skip height."""
    h = size / 2
    return np.concatenate([sheet(0.0, size, 0.0, size, 0.0), sheet(0.0, h, 0.0, size, -0.6),
                           wall(h + 0.52, 0.5, size - 0.5, 0.0, 0.36)], 0).astype(np.float32)


# ---- a correct dump, one window and one record at a time --------------------------------------------

def build_reference_copy(xyz, c=0.12, r_q=0.056, F=2, tile=2, skip=2, packed=True, seed=1):
    """A correct fine copy of the points `xyz` ((n, 3)), written from the specification with
    Python loops: (points (n, 4) float32, geo, {"frec", "wpts"}) as Context.debug_fine_copy()
    returns them.  The grid has one padding cell around the points' bounding box.  Thresholds
    are the tightest sound ones (the build's may be up to 3 steps wider), so lowering a high one
    or raising a low one by a step is a fault."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    orig = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    pts = np.concatenate([xyz, orig.view(np.float32)[:, None]], 1)
    p64 = xyz.astype(np.float64)
    bmin, bmax = p64.min(0), p64.max(0)
    o = bmin - c
    dims = [int(math.floor((bmax[a] - bmin[a]) / c)) + 3 for a in range(3)]
    R = r_q + MARGIN_R
    zq = float(np.float32(2.0) / np.float32(250.0))
    geo = {"built": 1, "tile": tile, "skip": skip if tile == 2 else 1, "packed": int(packed),
           "nx": dims[0], "ny": dims[1], "nz": dims[2], "F": F, "fnx": F * dims[0],
           "fny": F * dims[1], "rz": dims[2] - 1, "n_points": n,
           "ox": float(o[0]), "oy": float(o[1]), "oz": float(o[2]), "c": c, "inv_c": 1.0 / c,
           "r_q": r_q, "cf": c / F, "inv_cf": F * (1.0 / c), "R2": R * R, "zq": zq,
           "reach": math.ceil(R / (c / F)), "tsteps": math.ceil((r_q + MARGIN_T) / c / zq),
           "clear_c": c}
    zabs = max(abs(geo["oz"]), abs(geo["oz"] + float(dims[2]) * c))
    geo["clear_zt0"] = geo["oz"] + c + 2.0 * R + zabs * (1.0 / 1048576.0)
    fnx, fny, rz, cf = geo["fnx"], geo["fny"], geo["rz"], geo["cf"]
    step = zq * c
    idx, nrec = record_index(geo)
    start_w = np.zeros(nrec, np.uint32)
    band_w = np.full(nrec, 0x00FF, np.uint32)       # padding records stay {0, 0x00FF}
    entries, empty = [], np.zeros((rz, fny, fnx), bool)
    cellz = np.clip(np.floor((p64[:, 2] - geo["oz"]) * geo["inv_c"]), 0, dims[2] - 1).astype(int)
    for wy in range(fny):
        for wx in range(fnx):
            x0, y0 = geo["ox"] + wx * cf, geo["oy"] + wy * cf
            dx = np.maximum(np.maximum(x0 - p64[:, 0], p64[:, 0] - (x0 + cf)), 0.0)
            dy = np.maximum(np.maximum(y0 - p64[:, 1], p64[:, 1] - (y0 + cf)), 0.0)
            run = sorted(np.nonzero(dx * dx + dy * dy <= geo["R2"])[0],
                         key=lambda i: (-p64[i, 2], orig[i]))
            begin = len(entries)
            entries += [pts[i] for i in run]
            entries.append(np.array([np.nan, np.nan, -np.inf, np.nan], np.float32))
            for iz in range(rz):
                j = 0
                while j < len(run) and cellz[run[j]] > iz + 1:
                    j += 1
                inb = [i for i in run[j:] if cellz[i] >= iz]
                word, band = begin + j, 0x00FF
                if inb:
                    zb = geo["oz"] + iz * c
                    hi = math.ceil((p64[inb[0], 2] + r_q + MARGIN_T - zb) / step)
                    lo = math.floor((p64[inb[-1], 2] - r_q - MARGIN_T - zb) / step)
                    band = max(lo, 0) | ((hi if hi <= 254 else 255) << 8)
                else:
                    empty[iz, wy, wx] = True
                if tile == 2:
                    for (h, cap), sh in zip(SKIP_H[geo["skip"]], (25, 29) if skip == 2 else (28,)):
                        k = 0
                        while j + k < len(run) and p64[run[j + k], 2] >= geo["oz"] + (iz + h) * c:
                            k += 1
                        word |= min(k, cap) << sh
                start_w[idx[iz, wy, wx]] = word
                band_w[idx[iz, wy, wx]] = band
    if tile == 2:
        # clearance codes: the cell distance to the nearest cell whose lowest point counts at iz
        pcx = np.clip(np.floor((p64[:, 0] - geo["ox"]) * geo["inv_cf"]), 0, fnx - 1).astype(int)
        pcy = np.clip(np.floor((p64[:, 1] - geo["oy"]) * geo["inv_cf"]), 0, fny - 1).astype(int)
        zlow = np.full((fny, fnx), np.inf)
        np.minimum.at(zlow, (pcy, pcx), p64[:, 2])
        Y, X = np.mgrid[0:fny, 0:fnx]
        for iz in range(1, rz - 1):
            occ = zlow <= geo["clear_zt0"] + iz * c
            for wy in range(1, fny - 1):
                for wx in range(1, fnx - 1):
                    if empty[iz, wy, wx] and occ.any():
                        D = int(np.maximum(abs(Y - wy), abs(X - wx))[occ].min())
                        band_w[idx[iz, wy, wx]] |= min(max(D - 1, 0), CLEAR_MAX) << 8
                    elif empty[iz, wy, wx]:
                        band_w[idx[iz, wy, wx]] |= CLEAR_MAX << 8
    ent = np.stack(entries)
    ent[:, 3].view(np.uint32)[np.isnan(ent[:, 0])] = 0xFFFFFFFF
    geo["n_entries"], geo["n_records"] = ent.shape[0], nrec
    geo["start_off"], geo["frec_bytes"] = record_sizes(geo)
    wp = np.ascontiguousarray(ent[:, :3] if packed else ent)
    geo["wpts_bytes"], geo["pts_bytes"] = wp.nbytes, pts.nbytes
    if tile == 2:
        frec = np.zeros(geo["frec_bytes"], np.uint8)
        frec[:2 * nrec] = band_w.astype(np.uint16).view(np.uint8)
        frec[geo["start_off"]:] = start_w.view(np.uint8)
    else:
        frec = np.ascontiguousarray(np.stack([start_w, band_w], 1)).view(np.uint8).ravel()
    return pts, geo, {"frec": frec, "wpts": wp.view(np.uint8).ravel().copy()}
