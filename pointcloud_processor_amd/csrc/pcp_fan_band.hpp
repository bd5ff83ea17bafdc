// The tight probe bands of the split records ("Skip 7"): a twin of the records'
// threshold array in which every point of the window widens the band only by its own reach over
// the cell.  Plain C++ with no HIP dependency: pcp_fine.hip's k_band_tight builds the twin through
// these functions, tests/native/fan_band_selftest.cpp checks the rule stand-alone.
//
// The rule.  Record (W, iz) holds window W's entries in coarse z cells iz, iz + 1, and the probe
// calls a sample a candidate when its height above the block floor zb = oz + iz c, in steps of
// kZq c, lies strictly between the record's two thresholds.  The specified thresholds are the z
// range of those entries widened by r + 2 mm (pcp_fine.hip, k_frec).  Here, with d_p the xy
// distance from entry p to W's rectangle (0 inside it), m the 1 mm query margin and rho = r + mu:
//
//   g_p = max(d_p - m, 0)          reach_p = sqrt(rho^2 - g_p^2)        (g_p < rho, else no part)
//   top = max_p (z_p + reach_p)    bottom = min_p (z_p - reach_p)
//
// coded as zband_code codes a z range, hi = ceil((top - zb) / step) + 1 and
// lo = floor((bottom - zb) / step) - 1 (hi >= 255: 255, unbounded; lo <= 0: 0, unbounded; lo at
// most 254, 255 in the low byte marks an empty record), and each then replaced by the specified
// threshold where that one is tighter: the twin is never looser than the copy it stands in for.
// A record none of whose entries takes part gets lo 254, hi 0, which no sample satisfies.
//
// Soundness.  Let a sample k of a ray probe (W, iz), let q = q_k be its exact float position, and
// let an entry p of the terrain pass FLANN's predicate fl(fl(dx^2 + dy^2) + dz^2) < r2 with
// dx = fl(q_x - p_x) etc.  Then the probe's float `us` lies strictly inside the twin's thresholds:
//
//  (1) the predicate: each difference and square carries a relative u = 2^-24 and the sums
//      another, so in real numbers |q - p| < r' = r (1 + 4 u): 1.4e-8 m more than r.
//  (2) the probe cell: the probe's float cell W is that of a point within e_xy of q in xy, with
//      e_xy inside m however far from the origin the terrain lies -- the allowance the window's
//      own membership (xy distance <= r + m from W's rectangle) already rests on (pcp_fine.hip,
//      march).  So q's xy distance to W's rectangle is at most m, p's xy distance to q at least
//      g_p, p is an entry of W, and |q_z - p_z| < sqrt(r'^2 - g_p^2) (with g_p < r' < rho, so p
//      takes part).  In z, q's stencil corner is iz up to the same error, and the entries within
//      r of q lie in coarse cells iz, iz + 1 (c >= 2 r + 2 m): p belongs to the record.
//  (3) sqrt(rho^2 - g^2) - sqrt(r'^2 - g^2) >= rho - r' for 0 <= g < r' (the difference grows
//      with g), so q_z < z_p + reach_p - (mu - 4 u r) <= top - (mu - 4 u r), and likewise
//      q_z > bottom + (mu - 4 u r).
//  (4) the code rounding: hi >= (top - zb) / step + 1 and lo <= (bottom - zb) / step - 1 up to
//      the double roundings of the build (1e-12 steps), so with U = (q_z - zb) / step
//          hi - U > 1 + (mu - 4 u r) / step        U - lo > 1 + (mu - 4 u r) / step.
//  (5) the error of us.  us = fma(fz - iz, 1 / kZq, fus_off), fz = fma(Dz, k, Az) in cells,
//      Az = fl(fl(fl(p_z) - fl(lo_z)) fl(1 / c)) + fl(fl(d_z) h).  In metres, with Z the largest
//      |z| among the pose and the grid, H the grid's height and S the ray's length (at most
//      1229 m, PCP_MAX_STEPS samples): the two conversions u Z each, the subtraction and the two
//      factors 3 u (H + S), the direction terms 4 u S, the fma's result u H, the second fma
//      2 u c (fz - iz is exact, below one cell); in all
//          E <= u (2 Z + 4 H + 7 S + 1),
//      5.2e-4 m for the longest ray near the origin, 7e-6 m at the benchmark's 15 m, and
//      another 1.2e-4 m per kilometre of height.  The probe's iz may be the exact corner's
//      neighbour when fz lies within E of an integer; us is then the height above that record's
//      floor, and (2) holds for it with the same allowance.
//      So us < hi and us > lo whenever E < step + mu - 4 u r, which with mu = kBandMu = 2 mm and
//      step = 0.96 mm is 2.96 mm: every terrain with 2 Z + 4 H + 7 S < 49 km.  These are the
//      margin and the rounding of the specified thresholds (theirs is this argument at g = 0):
//      the twin needs nothing the copy does not.
//  (6) a smaller mu was derived and not taken: E itself, as 1e-4 + 2^-23 (2 Z + 4 H + 7 * 1229 +
//      1), is 1.3 mm at the origin, 0.7 mm less than 2 mm of a band some 100 mm wide; the
//      estimate (profiles/fan_band_estimate.log) puts that below what a run can show.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCP_BAND_HD __host__ __device__ inline
#else
#define PCP_BAND_HD inline
#endif

namespace pcp {

constexpr double kBandMu = 2e-3;   // mu: the thresholds' margin beside r, as the specified copy's

// what the entries of a record contribute, folded one at a time
struct BandAcc {
    double top, bottom;
    bool any;
};

PCP_BAND_HD BandAcc fan_band_begin() { return BandAcc{-INFINITY, INFINITY, false}; }

// xy distance from (px, py) to fine cell (wx, wy)'s rectangle, the window rule's arithmetic
PCP_BAND_HD double fan_band_dist(double ox, double oy, double cf, int wx, int wy, double px,
                                 double py) {
    const double x0 = ox + (double)wx * cf, y0 = oy + (double)wy * cf;
    const double dx = fmax(fmax(x0 - px, px - (x0 + cf)), 0.0);
    const double dy = fmax(fmax(y0 - py, py - (y0 + cf)), 0.0);
    return sqrt(dx * dx + dy * dy);
}

// one entry at height z, xy distance d from the rectangle: rho = r + mu, m the query margin
PCP_BAND_HD void fan_band_add(BandAcc &a, double z, double d, double m, double rho) {
    const double g = fmax(d - m, 0.0);
    if (!(g < rho)) return;
    const double reach = sqrt(rho * rho - g * g);
    a.top = fmax(a.top, z + reach);
    a.bottom = fmin(a.bottom, z - reach);
    a.any = true;
}

// The record's threshold word lo | hi << 8 above the block floor zb in steps of `step`,
// never looser than `spec`, the specified word of the same record (not an empty one).
PCP_BAND_HD uint32_t fan_band_word(const BandAcc &a, double zb, double step, uint32_t spec) {
    if (!a.any) return 254u;   // lo 254, hi 0: never satisfied
    const double h = ceil((a.top - zb) / step) + 1.0;
    const double l = floor((a.bottom - zb) / step) - 1.0;
    const uint32_t hi = h >= 255.0 ? 255u : (uint32_t)fmax(h, 1.0);
    const uint32_t lo = l <= 0.0 ? 0u : (uint32_t)fmin(l, 254.0);
    const uint32_t slo = spec & 255u, shi = (spec >> 8) & 255u;
    return (lo > slo ? lo : slo) | ((hi < shi ? hi : shi) << 8);
}

}  // namespace pcp
