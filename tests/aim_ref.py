"""The definition of pcp_place_aimed (include/pcp_abi.h), restated in NumPy: the checker of the
aimed placement.  S [P, C], Z [C] as pcp_score_matrix returns them for the poses with every pitch
set to 0.0, poses5 [P, 5] (x, y, z, pitch, yaw), cells [C, 3], aims [A, 2] (yaw offset, pitch).
The tables are math.cos / math.sin / math.tan (the host C library's), every product, sum and sqrt
is rounded on its own (one NumPy operation each), sums are sequential in cell order from +0.0
(pair_ref.osum)."""
import math

import numpy as np
from pair_ref import OWNER_NONE, OWNER_ZX120, osum, smax

AIM_MAX = 64          # PCP_AIM_MAX / PCP_AIM_MAX_ROWS (tests/test_place_aimed_abi.py pins them)
AIM_MAX_ROWS = 65536


def pose_table(poses5):
    """(cos, sin) of every pose's yaw."""
    return [(math.cos(float(q[4])), math.sin(float(q[4]))) if math.isfinite(float(q[4]))
            else (math.nan, math.nan) for q in np.asarray(poses5, np.float64).reshape(-1, 5)]


def aim_table(aims, h_fov, v_fov):
    """Per aim (ca, sa, tlo, thi), and ch."""
    rows = []
    for off, pitch in np.asarray(aims, np.float64).reshape(-1, 2):
        lo = float(pitch) - v_fov * 0.5
        hi = float(pitch) + v_fov * 0.5
        tlo = -math.inf if lo <= -math.pi / 2 else math.tan(lo)
        thi = math.inf if hi >= math.pi / 2 else math.tan(hi)
        rows.append((math.cos(float(off)), math.sin(float(off)), tlo, thi))
    return rows, math.cos(h_fov * 0.5)


def rotate(cyp, syp, ca, sa):
    """The aimed heading's (cos, sin): the pose's yaw plus the aim's offset."""
    return cyp * ca - syp * sa, syp * ca + cyp * sa


def select(view, s_row):
    """W of a row: the pose's score where the cell is in view, +0.0 elsewhere."""
    return np.where(view, s_row, 0.0)


def first_max(t):
    """The first maximum of a [P, A] table in row-major order (strict '>' from -inf): (p, a), or
    (-1, -1) when every entry is -inf."""
    k = int(np.argmax(t)) if t.size else 0
    if not t.size or not t.flat[k] > -np.inf:
        return -1, -1
    return k // t.shape[1], k % t.shape[1]


def geometry(pose, cells):
    """dx, dy, dz, hyp of one pose against every cell."""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    dx, dy, dz = cells[:, 0] - pose[0], cells[:, 1] - pose[1], cells[:, 2] - pose[2]
    return dx, dy, dz, np.sqrt(dx * dx + dy * dy)


def in_view(poses5, cells, aims, h_fov, v_fov, want_edge=False):
    """view [P, A, C]: H && V of the definition.  want_edge: also the smallest |fwd - ch * hyp|
    over every (pose, aim, cell)."""
    poses5 = np.asarray(poses5, np.float64).reshape(-1, 5)
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    rows, ch = aim_table(aims, h_fov, v_fov)
    pt = pose_table(poses5)
    view = np.zeros((poses5.shape[0], len(rows), cells.shape[0]), bool)
    edge = np.inf
    no_h = h_fov >= 2.0 * math.pi
    with np.errstate(invalid="ignore"):
        for p, (cyp, syp) in enumerate(pt):
            dx, dy, dz, hyp = geometry(poses5[p], cells)
            chh = ch * hyp
            head = [rotate(cyp, syp, ca, sa) for ca, sa, _, _ in rows]
            Cy = np.array([q[0] for q in head], np.float64)[:, None]
            Sy = np.array([q[1] for q in head], np.float64)[:, None]
            tlo = np.array([q[2] for q in rows], np.float64)[:, None]
            thi = np.array([q[3] for q in rows], np.float64)[:, None]
            fwd = dx[None, :] * Cy + dy[None, :] * Sy      # [A, C], each operation rounded
            H = np.ones_like(fwd, bool) if no_h else fwd >= chh[None, :]
            V = ~(dz[None, :] < tlo * hyp[None, :]) & ~(dz[None, :] > thi * hyp[None, :])
            view[p] = H & V
            if want_edge and fwd.size and not np.isnan(fwd).all():
                edge = min(edge, float(np.nanmin(np.abs(fwd - chh[None, :]))))
    return (view, edge) if want_edge else view


def place_aimed(S, Z, poses5, cells, aims, h_fov, v_fov, k_max, fixed=(), sep=0.0, view=None):
    """fixed: (pose, aim) pairs already placed.  -> dict as Context.place_aimed's, with the whole
    round_totals [n_selected + (1 if the search stopped on no gain) .., P, A] under "tables" and
    the recorded ones under "round_totals"."""
    S = np.asarray(S, np.float64)
    Z = np.asarray(Z, np.float64)
    poses5 = np.asarray(poses5, np.float64).reshape(-1, 5)
    aims = np.asarray(aims, np.float64).reshape(-1, 2)
    P, C = S.shape
    A = aims.shape[0]
    if view is None:
        view = in_view(poses5, cells, aims, h_fov, v_fov)
    xy = poses5[:, :2]
    fixed = [(int(p), int(a)) for p, a in fixed]
    nf = len(fixed)
    # 1. the base
    base = Z.copy()
    owner = np.where(Z > 0, OWNER_ZX120, OWNER_NONE).astype(np.int32)
    for i, (p, a) in enumerate(fixed):
        w = select(view[p, a], S[p])
        owner[base < w] = i
        base = smax(base, w)
    t0, c0 = osum(base)
    T = float(t0[0])
    out = {"base_total": T, "base_covered": int(c0[0]), "selected": [], "selected_aim": [],
           "total_after": [], "covered_after": [], "round_totals": [], "tables": []}
    # 2. the poses in the search

    def close(b):
        dx, dy = xy[:, 0] - xy[b, 0], xy[:, 1] - xy[b, 1]
        return dx * dx + dy * dy < sep * sep

    alive = np.ones(P, bool)
    for p, _ in fixed:
        alive[p] = False
        if sep > 0:
            alive &= ~close(p)
    for r in range(k_max):
        if not alive.any():
            break
        t = np.full((P, A), -np.inf)
        cov = np.zeros((P, A), np.int32)
        for p in np.flatnonzero(alive):
            t[p], cov[p] = osum(smax(base[None, :], select(view[p], S[p][None, :])))
        out["tables"].append(t)
        b, ab = first_max(t)
        if b < 0 or not t[b, ab] > T:
            break
        out["round_totals"].append(t)
        out["selected"].append(b)
        out["selected_aim"].append(ab)
        out["total_after"].append(float(t[b, ab]))
        out["covered_after"].append(int(cov[b, ab]))
        T = float(t[b, ab])
        w = select(view[b, ab], S[b])
        owner[base < w] = nf + r
        base = smax(base, w)
        alive[b] = False
        if sep > 0:
            alive &= ~close(b)
    n = len(out["selected"])
    out["n_selected"] = n
    out["selected"] = np.array(out["selected"], np.int64)
    out["selected_aim"] = np.array(out["selected_aim"], np.int32)
    out["total_after"] = np.array(out["total_after"], np.float64)
    out["covered_after"] = np.array(out["covered_after"], np.int32)
    out["round_totals"] = np.array(out["round_totals"], np.float64).reshape(n, P, A)
    out["cell_score"] = base
    out["cell_owner"] = owner
    return out


def runner_up_gaps(ref):
    """Best minus runner-up of every recorded round's table."""
    gaps = []
    for t in ref["round_totals"]:
        v = np.sort(t[np.isfinite(t)])[::-1]
        gaps.append(float(v[0] - v[1]) if v.size > 1 else np.inf)
    return gaps


def tick_aims():
    """The aims the call was specified with, pitch-major: pitches (-45, -25, -5) degrees x yaw
    offsets -90 .. 78 degrees in steps of 12, A = 45."""
    return np.array([[math.radians(o), math.radians(p)] for p in (-45.0, -25.0, -5.0)
                     for o in range(-90, 79, 12)], np.float64)
