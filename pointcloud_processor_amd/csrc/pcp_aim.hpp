// The front of the aimed placement (pcp_place_aimed, pcp_aim.hip): the argument
// check, the host tables of the field-of-view predicate and the plan of the call's blocks.  Plain
// C++ (no HIP dependency): tests/native/aim_selftest.cpp builds it with the host compiler.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "pcp_abi.h"
#include "pcp_place_shared.hpp"

namespace pcp {

// one aim's row of the predicate's table: cos / sin of the yaw offset and the tangents of the
// elevation bounds (-inf / +inf where a bound reaches the vertical)
struct AimRow {
    double ca, sa, tlo, thi;
};
static_assert(sizeof(AimRow) == 32, "four doubles");

constexpr double kAimPi = 3.14159265358979323846;       // M_PI
constexpr double kAimPi2 = 1.57079632679489661923;      // M_PI_2

// the aims' rows; *ch = cos(h_fov / 2); -> 1 when there is no horizontal test (h_fov >= 2 pi).
// Every cos, sin and tan is the host C library's double function.
inline int aim_rows(const double *aims, int n_aims, double h_fov, double v_fov, AimRow *rows,
                    double *ch) {
    for (int a = 0; a < n_aims; ++a) {
        const double lo = aims[2 * a + 1] - v_fov * 0.5, hi = aims[2 * a + 1] + v_fov * 0.5;
        rows[a].ca = std::cos(aims[2 * a]);
        rows[a].sa = std::sin(aims[2 * a]);
        rows[a].tlo = lo <= -kAimPi2 ? -INFINITY : std::tan(lo);
        rows[a].thi = hi >= kAimPi2 ? INFINITY : std::tan(hi);
    }
    *ch = std::cos(h_fov * 0.5);
    return h_fov >= 2.0 * kAimPi ? 1 : 0;
}

// (cos, sin) of every pose's yaw, [n][2]
inline void aim_pose_rows(const double *poses5, uint64_t n, double *cs) {
    for (uint64_t p = 0; p < n; ++p) {
        cs[2 * p] = std::cos(poses5[5 * p + 4]);
        cs[2 * p + 1] = std::sin(poses5[5 * p + 4]);
    }
}

// the predicate of one (pose, aim, cell), every operation rounded on its own (the build has
// -ffp-contract=off): the definition in include/pcp_abi.h, shared by the kernels and the host
struct AimGeo {
    double dx, dy, dz, hyp, chh;
};
PCP_PS_HD inline AimGeo aim_geo(double cx, double cy, double cz, double px, double py, double pz,
                                double ch) {
    AimGeo g;
    g.dx = cx - px;
    g.dy = cy - py;
    g.dz = cz - pz;
    g.hyp = sqrt(g.dx * g.dx + g.dy * g.dy);
    g.chh = ch * g.hyp;
    return g;
}
PCP_PS_HD inline void aim_heading(double cyp, double syp, double ca, double sa, double &Cy,
                                  double &Sy) {
    Cy = cyp * ca - syp * sa;
    Sy = syp * ca + cyp * sa;
}
PCP_PS_HD inline bool aim_sees(const AimGeo &g, double Cy, double Sy, double tlo, double thi,
                               bool no_h) {
    const double fwd = g.dx * Cy + g.dy * Sy;
    const bool H = no_h || fwd >= g.chh;
    // (negated: -inf * 0 = NaN counts as inside)
    const bool V = !(g.dz < tlo * g.hyp) && !(g.dz > thi * g.hyp);
    return H && V;
}

// what is wrong with a call's parameters: 0, or the first of these
enum {
    kAimOk = 0,
    kAimKmax,       // k_max outside 1 .. PCP_PLACE_MAX
    kAimCount,      // n_aims outside 1 .. PCP_AIM_MAX
    kAimFixedCount, // n_fixed outside 0 .. PCP_PLACE_MAX
    kAimReserved,   // reserved != 0
    kAimHfov,       // h_fov not finite or <= 0
    kAimVfov,       // v_fov outside (0, pi]
    kAimAim,        // a non-finite aim or a pitch outside [-pi / 2, pi / 2]: *bad = the aim
    kAimPoses,      // n > PCP_PAIR_MAX_POSES
    kAimRows,       // n * n_aims > PCP_AIM_MAX_ROWS
    kAimFixedPose,  // a fixed pose >= n: *bad = the entry
    kAimFixedTwice, // a fixed pose listed twice: *bad = the entry
    kAimFixedAim    // a fixed aim outside the table: *bad = the entry
};
inline int aim_check(const pcp_aim_params *ap, const double *aims, uint64_t n, int *bad) {
    *bad = 0;
    if (ap->k_max < 1 || ap->k_max > PCP_PLACE_MAX) return kAimKmax;
    if (ap->n_aims < 1 || ap->n_aims > PCP_AIM_MAX) return kAimCount;
    if (ap->n_fixed < 0 || ap->n_fixed > PCP_PLACE_MAX) return kAimFixedCount;
    if (ap->reserved != 0) return kAimReserved;
    if (!std::isfinite(ap->h_fov) || !(ap->h_fov > 0)) return kAimHfov;
    if (!(ap->v_fov > 0 && ap->v_fov <= kAimPi)) return kAimVfov;
    for (int a = 0; a < ap->n_aims; ++a) {
        *bad = a;
        if (!std::isfinite(aims[2 * a]) || !std::isfinite(aims[2 * a + 1]) ||
            aims[2 * a + 1] < -kAimPi2 || aims[2 * a + 1] > kAimPi2)
            return kAimAim;
    }
    *bad = 0;
    if (n > PCP_PAIR_MAX_POSES) return kAimPoses;
    if (n * (uint64_t)ap->n_aims > PCP_AIM_MAX_ROWS) return kAimRows;
    const int l = check_index_list(ap->fixed_pose, ap->n_fixed, n, bad);
    if (l == kListRange) return kAimFixedPose;
    if (l == kListTwice) return kAimFixedTwice;
    for (int i = 0; i < ap->n_fixed; ++i) {
        *bad = i;
        if (ap->fixed_aim[i] < 0 || ap->fixed_aim[i] >= ap->n_aims) return kAimFixedAim;
    }
    *bad = 0;
    return kAimOk;
}

// the fixed sensors as the kernels take them
struct AimFixed {
    int32_t n;
    int32_t pose[PCP_PLACE_MAX], aim[PCP_PLACE_MAX];
};

// The call's blocks.  Device and pinned alike: [state | base f64 C | owner i32 C | round totals
// f64 K x P x A | round covered i32 K x P x A | alive u32 P]; the download is a prefix of it.  The
// tables, uploaded in one copy: [pose (cos, sin) f64 P x 2 | aim rows A].
struct AimPlan {
    int C, P, A, K;
    CellBlock cb;
    size_t rt_off, rc_off, al_off, bytes;   // the block
    size_t tp_off, ta_off, tab_bytes;       // the tables
    size_t rows() const { return (size_t)P * (size_t)A; }
    // the span a caller's outputs need
    size_t down(bool round_totals, bool cells) const {
        return round_totals ? rc_off : cells ? rt_off : cb.score_off;
    }
};
inline AimPlan aim_plan(size_t state_bytes, int C, int P, int A, int K) {
    AimPlan s;
    s.C = C;
    s.P = P;
    s.A = A;
    s.K = K;
    s.cb = cell_block(state_bytes, C);
    s.rt_off = s.cb.rest_off;
    s.rc_off = a16(s.rt_off + (size_t)K * s.rows() * sizeof(double));
    s.al_off = a16(s.rc_off + (size_t)K * s.rows() * sizeof(int32_t));
    s.bytes = a16(s.al_off + (size_t)P * sizeof(uint32_t));
    s.tp_off = 0;
    s.ta_off = a16((size_t)P * 2 * sizeof(double));
    s.tab_bytes = s.ta_off + (size_t)A * sizeof(AimRow);
    return s;
}

}  // namespace pcp
