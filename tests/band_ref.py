"""The tight twin of the split records' probe thresholds (DESIGN.md §5 Skip 7, pcp_fan_band.hpp)
checked against its rule in plain numpy, float64.

Record (W, iz) holds window W's entries in coarse z cells iz, iz + 1 (tests/fine_ref.py's
membership).  Each entry p, at xy distance d_p from W's rectangle, takes part when
g_p = max(d_p - m, 0) < rho = r + mu and reaches sqrt(rho^2 - g_p^2) above and below its height:

    top = max_p (z_p + reach_p)        bottom = min_p (z_p - reach_p)

and the march needs, in steps of zq c above the block floor zb = oz + iz c,

    hi >= (top - zb) / step + 1        lo <= (bottom - zb) / step - 1

(the real-number bounds: the whole step beside top and bottom is part of the probe's error budget,
pcp_fan_band.hpp (4), (5)).  zband_code's rounding -- a ceil, a floor -- puts each threshold less
than TIGHT_STEPS = 1 step beyond its bound, unless the specified threshold is tighter still, which
then stands.  hi 255 and lo 0 are "unbounded"; lo is at most 254.

check_band(points, geo, frec, twin) returns a list of violations, each beginning with the name
of what is wrong; build_reference_twin() makes a correct twin with Python loops, one record at a
time, for the CPU tests to mutate.  No GPU and no ctypes here."""
import math

import numpy as np

import fine_ref

MARGIN_M = 1e-3      # m: the query margin, the allowance for the float probe cell
MU = 2e-3            # mu: the thresholds' margin beside r
TIGHT_STEPS = 1.0    # a threshold lies less than this beyond its real-number bound
EPS = 1e-6           # steps: the double roundings of either side's arithmetic


def real_bounds(points, geo, mu=MU):
    """(bound_hi, bound_lo, takes_part, has) as (rz, fny, fnx) arrays: the real-number bounds of
    the thresholds in steps above each record's floor (-inf / +inf where no entry takes part),
    whether any entry takes part, whether the record holds entries at all."""
    fnx, fny, rz, nz = geo["fnx"], geo["fny"], geo["rz"], geo["nz"]
    nw = fnx * fny
    pts = np.asarray(points, np.float32)
    x, y, z = (pts[:, a].astype(np.float64) for a in range(3))
    wk, pk, _, _ = fine_ref._window_pairs(geo, x, y)
    dx = fine_ref._rect_gap(geo["ox"], geo["cf"], (wk % fnx).astype(np.float64), x[pk])
    dy = fine_ref._rect_gap(geo["oy"], geo["cf"], (wk // fnx).astype(np.float64), y[pk])
    g = np.maximum(np.sqrt(dx * dx + dy * dy) - MARGIN_M, 0.0)
    rho = geo["r_q"] + mu
    part = g < rho
    reach = np.sqrt(np.maximum(rho * rho - g * g, 0.0))
    zk = z[pk]
    czk = np.clip(np.floor((zk - geo["oz"]) * geo["inv_c"]), 0, nz - 1).astype(np.int64)
    step = geo["zq"] * geo["c"]
    bhi = np.full((rz, nw), -np.inf)
    blo = np.full((rz, nw), np.inf)
    has = np.zeros((rz, nw), bool)
    for iz in range(rz):                    # (a loop over levels, never over records)
        inb = (czk >= iz) & (czk <= iz + 1)
        has[iz, wk[inb]] = True
        sel = inb & part
        zb = geo["oz"] + iz * geo["c"]
        np.maximum.at(bhi[iz], wk[sel], (zk[sel] + reach[sel] - zb) / step + 1.0)
        np.minimum.at(blo[iz], wk[sel], (zk[sel] - reach[sel] - zb) / step - 1.0)
    shape = (rz, fny, fnx)
    return bhi.reshape(shape), blo.reshape(shape), np.isfinite(bhi).reshape(shape), has.reshape(shape)


def spec_words(geo, frec):
    """The specified threshold array: one uint16 word per record slot."""
    _, nrec = fine_ref.record_index(geo)
    return frec[:2 * nrec].view(np.uint16)


def check_band(points, geo, frec, twin, mu=MU):
    """Violations of the twin's rule in `twin` (uint16 per record slot) beside the specified
    copy `frec` (pcp_debug_fine_copy's bytes) of the index's `points`.  [] when it is correct."""
    out = []
    if geo["tile"] != 2:
        return ["layout: the twin goes with the split records (tile 2)"]
    idx, nrec = fine_ref.record_index(geo)
    spec = spec_words(geo, frec)
    twin = np.asarray(twin)
    if twin.dtype != np.uint16 or twin.shape != (nrec,):
        return [f"size: {twin.dtype} {twin.shape}, expected uint16 ({nrec},)"]
    pad = np.ones(nrec, bool)
    pad[idx.ravel()] = False
    if (twin[pad] != spec[pad]).any():
        out.append(f"padding: {int((twin[pad] != spec[pad]).sum()) } padding records differ from "
                   "the specified copy's")
    s, t = spec[idx].astype(np.int64), twin[idx].astype(np.int64)
    slo, shi, lo, hi = s & 255, s >> 8, t & 255, t >> 8
    bhi, blo, part, has = real_bounds(points, geo, mu)

    def report(name, mask, got=None, want=None):
        if not mask.any():
            return
        iz, wy, wx = fine_ref._first(mask)
        txt = f"{name}: {int(mask.sum())} records, first (wx, wy, iz) = ({wx}, {wy}, {iz})"
        if got is not None:
            txt += f": got {got[iz, wy, wx]}"
        if want is not None:
            txt += f", bound {want[iz, wy, wx]}"
        out.append(txt)

    empty = slo == 255
    report("empty", empty & (t != s), t, s)          # with their clearance codes
    live = ~empty
    report("empty.flag", live & (lo == 255), t)
    report("members", live & ~has, t)                # (the specified copy's own fault)
    dead = live & has & ~part
    report("dead", dead & ~((hi == 0) | (lo >= hi)), t)
    ok = live & part & (lo != 255)
    report("looser.hi", ok & (hi > shi), hi, shi)
    report("looser.lo", ok & (lo < slo), lo, slo)
    # soundness: at or beyond the bound, or the specified threshold (sound by its own rule)
    report("hi.sound", ok & (hi != 255) & (hi < bhi - EPS) & (hi != shi), hi, bhi)
    report("lo.sound", ok & (lo != 0) & (lo > blo + EPS) & (lo != slo), lo, blo)
    # tightness: less than a step beyond the bound (255 / 0 only where the bound is out of range)
    want_hi = np.minimum(np.where(bhi + TIGHT_STEPS > 255.0, 255.0, bhi + TIGHT_STEPS), shi)
    report("hi.tight", ok & ~(hi < want_hi + EPS) & ~((hi == 255) & (want_hi >= 255.0)), hi, bhi)
    want_lo = np.maximum(np.where(blo - TIGHT_STEPS <= 0.0, 0.0, np.minimum(blo - TIGHT_STEPS, 254.0)),
                         slo)
    report("lo.tight", ok & ~(lo > want_lo - EPS) & ~((lo == 254) & (want_lo >= 254.0 - EPS)) &
           ~((lo == 0) & (want_lo <= EPS)), lo, blo)
    return out


def build_reference_twin(points, geo, frec, mu=MU):
    """A correct twin, written from the rule one window and one record at a time with Python
    loops (small terrains only): the tightest coded thresholds, never looser than `frec`'s."""
    idx, nrec = fine_ref.record_index(geo)
    twin = spec_words(geo, frec).copy()
    p64 = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    fnx, fny, rz, cf, c = geo["fnx"], geo["fny"], geo["rz"], geo["cf"], geo["c"]
    step, rho = geo["zq"] * c, geo["r_q"] + mu
    cellz = np.clip(np.floor((p64[:, 2] - geo["oz"]) * geo["inv_c"]), 0, geo["nz"] - 1).astype(int)
    for wy in range(fny):
        for wx in range(fnx):
            x0, y0 = geo["ox"] + wx * cf, geo["oy"] + wy * cf
            dx = np.maximum(np.maximum(x0 - p64[:, 0], p64[:, 0] - (x0 + cf)), 0.0)
            dy = np.maximum(np.maximum(y0 - p64[:, 1], p64[:, 1] - (y0 + cf)), 0.0)
            mem = np.nonzero(dx * dx + dy * dy <= geo["R2"])[0]
            for iz in range(rz):
                spec = int(twin[idx[iz, wy, wx]])
                if spec & 255 == 255:
                    continue
                top, bot = -math.inf, math.inf
                for i in mem:
                    if iz <= cellz[i] <= iz + 1:
                        g = max(math.hypot(dx[i], dy[i]) - MARGIN_M, 0.0)
                        if g < rho:
                            reach = math.sqrt(rho * rho - g * g)
                            top, bot = max(top, p64[i, 2] + reach), min(bot, p64[i, 2] - reach)
                if top == -math.inf:
                    twin[idx[iz, wy, wx]] = 254
                    continue
                zb = geo["oz"] + iz * c
                h = math.ceil((top - zb) / step) + 1
                lw = math.floor((bot - zb) / step) - 1
                hi = 255 if h >= 255 else max(h, 1)
                lo = 0 if lw <= 0 else min(lw, 254)
                twin[idx[iz, wy, wx]] = max(lo, spec & 255) | (min(hi, spec >> 8) << 8)
    return twin
