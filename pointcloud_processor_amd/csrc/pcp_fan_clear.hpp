// Clearance codes of the fine copy's empty probe records and the march's jump over them
// ("Skip 5").  Plain C++ with no HIP dependency: pcp_fine.hip builds the codes and
// pcp_march.hpp's march reads them through these functions, and
// tests/native/fan_clear_selftest.cpp checks the rule stand-alone.
//
// The record of (fine cell w, coarse corner iz) is empty (0x00FF: low byte 255, no sample passes
// the probe) when w's window holds no point in the coarse z cells iz, iz + 1.  Its free high
// byte carries a code e, 0 = no information:
//
//   no terrain point with z <= Zt(iz) lies closer than e c_f, horizontally, to w's rectangle.
//
// Zt.  The probe maps sample k to the corner fz = (q_z - oz - (r + m)) / c and reads record
// iz = floor(fz) (march, FN 8), so a sample that reads record iz unclamped has
// q_z < oz + (iz + 1) c + (r + m), up to the float probe's error.  A point within r of that
// sample, or of any lower one, has z <= q_z + r.  So
//
//   Zt(iz) = oz + (iz + 1) c + 2 (r + m) + 2^-20 max|z of the grid|:
//
// the second m absorbs the probe's error (~1e-5 m, DESIGN.md §5 "Float probes") and the last
// term the float rounding of a far-away terrain's coordinates (3e-3 m at 3 km).
//
// Metric.  The distance to the rectangle is Chebyshev, max(dx, dy), which never exceeds Euclid:
// a point no closer than e c_f in it is no closer in the plane.  255 means "at least 255 cells".
//
// The jump.  A descending ray (dz < 0) whose sample k reads an unclamped empty record with code
// e (the grid's border records carry 0, fan_clear_border) skips its next
// n = floor((e c_f - rb) / hs) samples, hs = 0.3 sqrt(dx^2 + dy^2) the
// horizontal sample spacing and rb = r + m + 1e-6 max|coord| (the clip box's inflation):
//  * every skipped sample is lower than q_k, so a point within r of it has z <= Zt(iz);
//  * every skipped sample lies horizontally within n hs <= e c_f - rb of q_k, which lies in w's
//    rectangle up to the probe's error (inside m): a point within r of it would be closer than
//    e c_f to the rectangle;
//  * no such point exists, so no skipped sample is blocked -- what the march finds for them.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PCP_CLR_HD __host__ __device__ inline
#else
#define PCP_CLR_HD inline
#endif

namespace pcp {

constexpr int kClearMax = 255;        // the code saturates: "at least 255 cells"

// the levels' geometry: Zt(iz) = zt0 + iz c
struct ClearGeo {
    double zt0, c;
};
PCP_CLR_HD ClearGeo fan_clear_geo(double oz, double c, double rm, double zabs_max) {
    return ClearGeo{oz + c + 2.0 * rm + zabs_max * (1.0 / 1048576.0), c};
}
PCP_CLR_HD double fan_clear_ztop(const ClearGeo &g, int iz) { return g.zt0 + (double)iz * g.c; }

// the lowest level at which a point of height z counts: the smallest iz >= 0 with
// z <= Zt(iz), at most `cap`
PCP_CLR_HD int fan_clear_level(const ClearGeo &g, double z, int cap) {
    double t = ceil((z - g.zt0) / g.c);
    int l = t <= 0.0 ? 0 : t >= (double)cap ? cap : (int)t;
    while (l < cap && z > fan_clear_ztop(g, l)) ++l;
    while (l > 0 && z <= fan_clear_ztop(g, l - 1)) --l;
    return l;
}

// code of a cell whose nearest occupied cell is D cells away (Chebyshev, in cell indices;
// D = 0: the cell itself): a point of that cell is no closer than (D - 1) c_f to the rectangle
PCP_CLR_HD uint32_t fan_clear_code(uint32_t D) {
    return D == 0u ? 0u : (D - 1u > (uint32_t)kClearMax ? (uint32_t)kClearMax : D - 1u);
}

// The jump's two per-ray constants: n = floor(e a - b) with a = c_f / hs, b = rb / hs, 1 / hs
// biased downward by 2^-16 (far above the float rounding of a, b and the product).  a = b = 0
// turns the jump off (a ray that does not descend, the knob); a vertical ray's 1 / hs is capped,
// so its jump is large and finite.
struct ClearRay {
    float a, b;
};
PCP_CLR_HD ClearRay fan_clear_ray(float dx, float dy, float dz, float step, float cf, float rb,
                                  bool on) {
    if (!on || !(dz < 0.0f)) return ClearRay{0.0f, 0.0f};
    // (the device's approximate reciprocal square root is within 1 ulp, 6e-8: inside the bias;
    // this runs once per ray and pose, where an IEEE division and root cost as much as a probe)
#if defined(__HIP_DEVICE_COMPILE__)
    const float rs = __builtin_amdgcn_rsqf(dx * dx + dy * dy);
#else
    const float rs = 1.0f / sqrtf(dx * dx + dy * dy);
#endif
    float inv = rs * ((1.0f - 1.0f / 65536.0f) / step);
    inv = inv < 1e6f ? inv : 1e6f;
    return ClearRay{cf * inv, rb * inv};
}

// samples to skip after one that read an empty record with code e (at most 255 * 0.06e6: no
// overflow of the sample index); e = 0 gives 0
PCP_CLR_HD int fan_clear_skip(float e, const ClearRay &r) {
    return (int)fmaxf(fmaf(e, r.a, -r.b), 0.0f);   // (one rounding, host and device alike)
}

// The grid's outermost cells and levels carry no code.  The probe clamps its cell coordinates
// to the grid, so a sample outside it (or a NaN) reads one of those records, which belongs to
// another place: it must not jump, and with 0 there it does not.
PCP_CLR_HD bool fan_clear_border(uint32_t wx, uint32_t wy, uint32_t iz, uint32_t fnx, uint32_t fny,
                                 uint32_t rz) {
    return wx == 0u || wx + 1u == fnx || wy == 0u || wy + 1u == fny || iz == 0u || iz + 1u == rz;
}

// ---- host references --------------------------------------------------------------------

// The code's meaning, for one record, from a point list (x, y, z triples): the largest e <= 255
// such that no point with z <= Zt(iz) is closer than e c_f (Chebyshev) to the rectangle of
// fine cell (wx, wy) of a grid with origin (ox, oy).
inline uint32_t fan_clear_ref(const double *xyz, size_t n, double ox, double oy, double cf,
                              int wx, int wy, const ClearGeo &g, int iz) {
    const double x0 = ox + (double)wx * cf, y0 = oy + (double)wy * cf, zt = fan_clear_ztop(g, iz);
    double dmin = 1e300;
    for (size_t i = 0; i < n; ++i) {
        if (!(xyz[3 * i + 2] <= zt)) continue;
        const double dx = std::fmax(std::fmax(x0 - xyz[3 * i], xyz[3 * i] - (x0 + cf)), 0.0);
        const double dy = std::fmax(std::fmax(y0 - xyz[3 * i + 1], xyz[3 * i + 1] - (y0 + cf)), 0.0);
        dmin = std::fmin(dmin, std::fmax(dx, dy));
    }
    const double e = std::floor(dmin / cf);
    return e >= (double)kClearMax ? (uint32_t)kClearMax : (uint32_t)e;
}

// The build's passes (pcp_fine.hip runs them one thread per record): lev[w] = the cell's
// lowest level (fan_clear_level of its lowest point; >= rz: none).  Per level, h = the distance
// along y to the nearest occupied cell of the column, then D = min over dx of max(h(x + dx), |dx|)
// -- the Chebyshev distance -- both capped.  out[iz * fnx * fny + w] = fan_clear_code(D), 0 on
// the border.
inline void fan_clear_grid(const std::vector<uint32_t> &lev, int fnx, int fny, int rz,
                           std::vector<uint8_t> &out) {
    const int cap = kClearMax + 1;
    std::vector<int> h((size_t)fnx * fny);
    out.assign((size_t)fnx * fny * rz, 0);
    for (int iz = 0; iz < rz; ++iz) {
        for (int y = 0; y < fny; ++y)
            for (int x = 0; x < fnx; ++x) {
                int d = 0;
                for (; d < cap; ++d)
                    if ((y - d >= 0 && lev[(size_t)(y - d) * fnx + x] <= (uint32_t)iz) ||
                        (y + d < fny && lev[(size_t)(y + d) * fnx + x] <= (uint32_t)iz))
                        break;
                h[(size_t)y * fnx + x] = d;
            }
        for (int y = 0; y < fny; ++y)
            for (int x = 0; x < fnx; ++x) {
                int D = cap;
                for (int d = 0; d < D; ++d) {
                    if (x - d >= 0) D = std::min(D, std::max(h[(size_t)y * fnx + x - d], d));
                    if (x + d < fnx) D = std::min(D, std::max(h[(size_t)y * fnx + x + d], d));
                }
                if (!fan_clear_border((uint32_t)x, (uint32_t)y, (uint32_t)iz, (uint32_t)fnx,
                                      (uint32_t)fny, (uint32_t)rz))
                    out[((size_t)iz * fny + y) * fnx + x] = (uint8_t)fan_clear_code((uint32_t)D);
            }
    }
}

}  // namespace pcp
