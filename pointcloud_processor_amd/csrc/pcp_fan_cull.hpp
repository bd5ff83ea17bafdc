// Ring liveness of the dense ray fan ("Skip 4"): which (pose, elevation ring)
// pairs can reach the terrain's clip box at all.  Plain host C++ (no HIP dependency):
// fan_enqueue sizes the launch with it and hands every pose its live ring interval, and
// tests/native/fan_cull_selftest.cpp checks it stand-alone.
//
// A ray of ring j from a pose at height pz has the sample heights pz + se[j] s_k: the yaw
// rotation leaves the z component of the direction alone and the pose's pitch is not used
// (fan_body).  The step table ascends, so every height lies between h_0 = pz + se[j] s_0 and
// h_1 = pz + se[j] s_{K-1}.  The pair is dead iff that interval lies wholly above the box top or
// wholly below the box bottom.  A sample outside the clip box has no point within r (Skip 3:
// the box is the points' bounding box inflated by r + m + 1e-6 |coord|), so a dead pair's rays
// are "not blocked, K samples" -- what the march computes for them.
//
// Margin.  The test compares against the float box (GridView.fb) the kernel clips against,
// which is the double box rounded once: off by at most 2^-24 |fb|.  h_0 and h_1 are evaluated
// in double with one product and one sum: off by at most 2^-52 (|pz| + 2 |se s|), |se| <= 1.
// fan_cull_margin() bounds both generously -- 2^-22 of the larger box bound plus 2^-48 of
// (|pz| + s_{K-1}) -- and a pair is dead only when it clears the box by more than that.  The
// margin only ever turns dead pairs into live ones, which is always allowed; at the terrain's
// scale it is ~1e-7 m, four orders of magnitude below the 1 mm query margin m in the box.
//
// Monotony.  min(h_0, h_1) and max(h_0, h_1) do not decrease when se grows (products and sums
// round monotonically), so "dead above" holds on an upper range of se and "dead below" on a
// lower one: over a sorted se table a pose's live rings are one interval, found by bisection
// (or confirmed from the previous pose's interval in four tests).
#pragma once

#include <cmath>
#include <cstdint>

namespace pcp {

inline double fan_cull_margin(double zlo, double zhi, double pz, double s_last) {
    const double b = std::fmax(std::fabs(zlo), std::fabs(zhi));
    return b * (1.0 / 4194304.0) + (std::fabs(pz) + std::fabs(s_last)) * (1.0 / 281474976710656.0);
}

// every sample height of the pair above zhi + mg / below zlo - mg (false on any NaN)
inline bool fan_dead_above(double zhi, double mg, double pz, double se, double s_first,
                           double s_last) {
    const double h0 = pz + se * s_first, h1 = pz + se * s_last;
    return (h0 < h1 ? h0 : h1) > zhi + mg && h0 == h0 && h1 == h1;
}
inline bool fan_dead_below(double zlo, double mg, double pz, double se, double s_first,
                           double s_last) {
    const double h0 = pz + se * s_first, h1 = pz + se * s_last;
    return (h0 > h1 ? h0 : h1) < zlo - mg && h0 == h0 && h1 == h1;
}

// true: no sample of a ray with z component se from height pz lies inside [zlo, zhi].
// s_first, s_last: the first and last step-table entries (0 <= s_first <= s_last).
inline bool fan_pair_dead(double zlo, double zhi, double pz, double se, double s_first,
                          double s_last) {
    const double mg = fan_cull_margin(zlo, zhi, pz, s_last);
    return fan_dead_above(zhi, mg, pz, se, s_first, s_last) ||
           fan_dead_below(zlo, mg, pz, se, s_first, s_last);
}

// +1: se never decreases with j, -1: never increases, 0: neither (an elevation range past
// +-90 degrees)
inline int fan_se_order(const double *se, int n_el) {
    bool up = true, down = true;
    for (int j = 1; j < n_el; ++j) {
        if (!(se[j] >= se[j - 1])) up = false;
        if (!(se[j] <= se[j - 1])) down = false;
    }
    return up ? 1 : down ? -1 : 0;
}

struct FanLive {
    int j0, j1;   // live rings [j0, j1); j0 == j1: none
};

// One pose's live rings: the smallest interval holding every ring that is not dead (over a
// sorted table: exactly the live rings).  order: fan_se_order(se, n_el); hint: a guess that is
// confirmed in four tests when right (the previous pose's answer), any value allowed.
inline FanLive fan_pose_live(double zlo, double zhi, double pz, const double *se, int n_el,
                             int order, double s_first, double s_last,
                             FanLive hint = FanLive{0, 0}) {
    if (!(zlo <= zhi) || !std::isfinite(pz) || n_el <= 0) return FanLive{0, n_el > 0 ? n_el : 0};
    const double mg = fan_cull_margin(zlo, zhi, pz, s_last);
    if (order == 0) {
        int j0 = n_el, j1 = 0;
        for (int j = 0; j < n_el; ++j) {
            if (fan_dead_above(zhi, mg, pz, se[j], s_first, s_last) ||
                fan_dead_below(zlo, mg, pz, se[j], s_first, s_last))
                continue;
            if (j < j0) j0 = j;
            j1 = j + 1;
        }
        return j0 < j1 ? FanLive{j0, j1} : FanLive{0, 0};
    }
    // i: the rings in ascending se order; below(i) holds on [0, ib), above(i) on [ia, n_el)
    auto at = [&](int i) { return order > 0 ? se[i] : se[n_el - 1 - i]; };
    auto above = [&](int i) { return fan_dead_above(zhi, mg, pz, at(i), s_first, s_last); };
    auto below = [&](int i) { return fan_dead_below(zlo, mg, pz, at(i), s_first, s_last); };
    int hb = order > 0 ? hint.j0 : n_el - hint.j1, ha = order > 0 ? hint.j1 : n_el - hint.j0;
    int ib, ia;
    if (hb >= 0 && hb <= n_el && (hb == n_el || !below(hb)) && (hb == 0 || below(hb - 1))) {
        ib = hb;
    } else {
        int lo = 0, hi = n_el;   // first i that is not dead below
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (below(mid)) lo = mid + 1;
            else hi = mid;
        }
        ib = lo;
    }
    if (ha >= 0 && ha <= n_el && (ha == n_el || above(ha)) && (ha == 0 || !above(ha - 1))) {
        ia = ha;
    } else {
        int lo = 0, hi = n_el;   // first i that is dead above
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (above(mid)) hi = mid;
            else lo = mid + 1;
        }
        ia = lo;
    }
    if (ib >= ia) return FanLive{0, 0};
    return order > 0 ? FanLive{ib, ia} : FanLive{n_el - ia, n_el - ib};
}

// The interval of rings spanning every live (pose, ring) pair of a call.  pose_z: the poses'
// heights, `stride` doubles apart.  per_pose (nullable): each pose's own interval as two
// uint32 {j0, j1}, `pp_stride` uint32 apart.
inline FanLive fan_live_rings(double zlo, double zhi, const double *pose_z, uint64_t n_pose,
                              uint64_t stride, const double *se, int n_el, double s_first,
                              double s_last, uint32_t *per_pose = nullptr,
                              uint64_t pp_stride = 2) {
    const int order = fan_se_order(se, n_el);
    int j0 = n_el, j1 = 0;
    FanLive prev{0, 0};
    for (uint64_t k = 0; k < n_pose; ++k) {
        const FanLive l = fan_pose_live(zlo, zhi, pose_z[k * stride], se, n_el, order, s_first,
                                        s_last, prev);
        prev = l;
        if (per_pose) {
            per_pose[k * pp_stride] = (uint32_t)l.j0;
            per_pose[k * pp_stride + 1] = (uint32_t)l.j1;
        }
        if (l.j0 < l.j1) {
            if (l.j0 < j0) j0 = l.j0;
            if (l.j1 > j1) j1 = l.j1;
        }
    }
    return j0 < j1 ? FanLive{j0, j1} : FanLive{0, 0};
}

// The waves (64 consecutive rays, ring-major: ray = j n_az + i) that hold a ray of a live ring:
// [w0, w1) of ceil(n_az n_el / 64).  Culling is in whole waves: a wave that straddles a live
// and a dead ring stays.
struct FanWaves {
    uint32_t w0, w1;
};
inline FanWaves fan_live_waves(FanLive L, int n_az, int n_el) {
    const uint64_t rays = (uint64_t)n_az * (uint64_t)n_el;
    const uint32_t waves = (uint32_t)((rays + 63) / 64);
    if (L.j0 >= L.j1) return FanWaves{0u, 0u};
    const uint64_t r0 = (uint64_t)L.j0 * (uint64_t)n_az, r1 = (uint64_t)L.j1 * (uint64_t)n_az;
    FanWaves w{(uint32_t)(r0 / 64), (uint32_t)((r1 + 63) / 64)};
    if (w.w1 > waves) w.w1 = waves;
    return w;
}

}  // namespace pcp
