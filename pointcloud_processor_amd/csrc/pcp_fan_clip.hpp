// The march's clip interval ("Skip 3"): the samples k of a ray p + d s_k,
// s_k = 0.5 + 0.3 k, that can lie inside the terrain's clip box.  Plain C++ with no HIP
// dependency: pcp_march.hpp's clip_kf calls fan_clip with the device's approximate reciprocals,
// tests/native/fan_clip_selftest.cpp checks the rule stand-alone with exact and perturbed ones.
//
// The rule.  Slab times in float, t0 = max over the axes of the entry time (and 0), t1 = min of
// the exit times, then
//
//   klo = ceil ((t0 - 0.5) / 0.3 - e)          khi = floor((t1 - 0.5) / 0.3 + e),
//
// clamped to [0, K] and [-1, K - 1].  e is a slack in samples (GridView.fclip_e).  e = 1 is the
// rule as it was before the slack became a value -- ceil(x) - 1 and floor(y) + 1, a whole sample
// each side -- and kClipSlack = 2^-6 is the default.  khi is computed as
// floor(y - (1 - e)) + 1: at e = 1 that subtracts 0 and is the old expression to the bit.  klo's
// x - 1 is exact for x >= 0.5 (Sterbenz, and a float >= 2 is a multiple of its own ulp); for
// x < 0.5 both forms are <= 0 and clamp to 0.  So e = 1 gives the old bounds bit for bit.
//
// What a dropped sample is outside of.  Take k < klo (k > khi is the mirror image).  k is an
// integer below ceil(z), so k < z = fl(x~ - e).  With u = 2^-24:
//
//  (1) the scaled value: x~ = fl(fl(t0 - 0.5) fl(1 / 0.3)) and z carry four roundings, each
//      relative u, of values up to K <= PCP_MAX_STEPS = 4096 samples (t <= S = s_(K-1) < 1229 m;
//      if t0 > S every sample is dropped and (3) applies), so 0.3 z <= t0 - 0.5 - 0.3 e + 4.1 u S:
//      3.0e-4 m.  The table's s_k deviates from 0.5 + 0.3 k by the roundings of its k additions,
//      k ulp(S) / 2 < 5e-10 m.  Both vanish in 0.3 e = 4.7e-3 m (15 times over), so s_k < t0.
//  (2) t0 itself: it is the entry time of one axis a, fl(fl(f - fl(p_a)) inv), f the float face
//      fb, inv the reciprocal of fl(d_a) to within 2.5 ulp (the device's v_rcp_f32: 1 ulp).
//      That is ((f - p_a) + pi) (1 + eps) / d_a with |pi| = |p_a - fl(p_a)| <= u |p_a| and
//      |eps| <= kClipRelErr = 8 u (subtraction, fl(d_a), product: u each; reciprocal: 5 u).  From
//      s_k < t0, along axis a (say d_a > 0, entry through the low face):
//          q_a - f = d_a s_k - (f - p_a) < (f - p_a) eps + pi (1 + eps).
//  (3) f - p_a is at most d_a t0 <= S where t0 <= S (1 + 2 eps); where t0 is larger, s_k <= S
//      gives q_a - f < pi directly.  And a pose further than 2 S + 1 from the box's coordinates
//      cannot reach the face at all.  So with A = max |fb|
//          q_a - f < delta = 1.001 (S kClipRelErr + u (A + 2 S + 1)):
//      the sample lies outside the clip box shrunk by delta.  Its part that does not grow with
//      the coordinates, 1.001 S (8 u + 2 u) = 7.4e-4 m at K = 4096 (8.9e-6 m at the default
//      15 m, K = 49), is below the 1 mm query margin m; the part u A, with another u A for
//      fb = fl(double face), is inside the 1e-6 A the box is inflated by beside r + m
//      (GridIndex::view).  The clip box is the points' bounding box inflated by r + m + 1e-6 A, so
//      a sample outside the box shrunk by delta is further than r from every point: its
//      radiusSearch finds nothing, which is what the march assumes of it.
//  (4) a zero direction component (inv = +-inf; a flushed denormal likewise): the slab's times
//      are -+inf for a start strictly inside it, and for a start on or outside a face t0 = inf or
//      t1 = -inf (0 inf = NaN is dropped by fmin / fmax): every sample is dropped, and every
//      sample has q_a = p_a, on or outside the face up to pi.
//
// A sample exactly on a face stays: x = k gives ceil(k - e) = k, y = k gives floor(k + e) = k,
// and the roundings of (1) are far smaller than e.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define PCP_CLIP_HD __host__ __device__ inline
#else
#define PCP_CLIP_HD inline
#endif

namespace pcp {

constexpr float kClipSlack = 1.0f / 64.0f;      // the default e, in samples
constexpr float kClipSlackWhole = 1.0f;         // PCP_FAN_CLIP=0: a whole sample, the rule as it was
constexpr double kClipRelErr = 8.0 / 16777216.0;   // (2): relative error of a slab time

// (3): how far inside the clip box (faces fb, largest magnitude fb_abs_max) a dropped sample of a
// K-sample ray can lie, metres
PCP_CLIP_HD double fan_clip_delta(int K, double fb_abs_max) {
    const double S = 0.5 + 0.3 * (double)(K > 1 ? K - 1 : 1);
    return 1.001 * (S * kClipRelErr + (fb_abs_max + 2.0 * S + 1.0) / 16777216.0);
}

// The slab times of the ray p + d t against the box fb = {x0, x1, y0, y1, z0, z1}; inv[a] ~
// 1 / d[a] comes from the caller.  False: the ray misses the box.
// (rel: the six face differences fb[i] - p[i / 2], formed by the caller -- the fan's pose rows
// carry them ready, pcp_fan_row.hpp)
PCP_CLIP_HD bool fan_clip_slabs_rel(const float rel[6], const float inv[3], float &t0, float &t1) {
    // branch-free slabs: a zero (or flushed denormal) direction component gives +-inf slab
    // times, so a start strictly inside the slab leaves [t0, t1] as it is and one outside
    // empties it; a start exactly on a slab face (0 * inf = NaN, dropped by fmin/fmax, the
    // other time +-inf) also empties it -- exact, since the face lies r + m + 1e-6 |coord| from
    // every point and a ray parallel to it never comes closer
    t0 = 0.0f;
    t1 = FLT_MAX;
    for (int a = 0; a < 3; ++a) {
        const float ta = rel[2 * a] * inv[a], tb = rel[2 * a + 1] * inv[a];
        t0 = fmaxf(t0, fminf(ta, tb));
        t1 = fminf(t1, fmaxf(ta, tb));
    }
    return t0 <= t1;
}
PCP_CLIP_HD bool fan_clip_slabs(const float fb[6], const float p[3], const float inv[3], float &t0,
                                float &t1) {
    const float rel[6] = {fb[0] - p[0], fb[1] - p[0], fb[2] - p[1],
                          fb[3] - p[1], fb[4] - p[2], fb[5] - p[2]};
    return fan_clip_slabs_rel(rel, inv, t0, t1);
}

// [t0, t1] to sample bounds with e samples of slack each side, inv_step = fl(1 / 0.3)
PCP_CLIP_HD void fan_clip_bounds(float t0, float t1, float inv_step, float e, int K, int &klo,
                                 int &khi) {
    // (0.5 / 0.3 + (1 - e) is uniform: computed once per thread, not per ray)
    const float kl = ceilf((t0 - 0.5f) * inv_step - e);
    const float kh = floorf(fminf(t1, 1e30f) * inv_step - (0.5f * inv_step + (1.0f - e))) + 1.0f;
    klo = (int)fminf(fmaxf(kl, 0.0f), (float)K);
    khi = (int)fminf(fmaxf(kh, -1.0f), (float)(K - 1));
}

// Sample bounds [klo, khi] of a K-sample ray; klo > khi (0, -1): no sample can be inside
PCP_CLIP_HD void fan_clip(const float fb[6], const float p[3], const float inv[3], float inv_step,
                          float e, int K, int &klo, int &khi) {
    float t0, t1;
    if (!fan_clip_slabs(fb, p, inv, t0, t1)) {
        klo = 0;
        khi = -1;
        return;
    }
    fan_clip_bounds(t0, t1, inv_step, e, K, klo, khi);
}
// the same from the six face differences
PCP_CLIP_HD void fan_clip_rel(const float rel[6], const float inv[3], float inv_step, float e,
                              int K, int &klo, int &khi) {
    float t0, t1;
    if (!fan_clip_slabs_rel(rel, inv, t0, t1)) {
        klo = 0;
        khi = -1;
        return;
    }
    fan_clip_bounds(t0, t1, inv_step, e, K, klo, khi);
}

}  // namespace pcp
