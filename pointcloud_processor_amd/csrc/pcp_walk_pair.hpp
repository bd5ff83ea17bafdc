// The paired walk of a fine window's packed run ("round trips"): two 12-byte
// entries per trip instead of one.  Plain C++ with no HIP dependency: pcp_march.hpp's
// scan_window3 walks through these functions and tests/native/walk_pair_selftest.cpp checks them
// stand-alone against the one-entry walk.
//
// A run is z-descending and ends at its window's sentinel (NaN, NaN, -inf): never within r,
// always r below.  The one-entry walk tests entry k, stops when it is within r of q or lies
// rexit below q, else goes on to k + 1: every trip is a dependent round trip through vector
// memory, although consecutive entries are 12 bytes apart.  The paired walk loads entries k and
// k + 1 (24 contiguous bytes) together, tests k with the same predicate and tests k + 1 only
// where k did not stop.  So the answer, the last entry tested and the number of tests are the
// one-entry walk's; only the loads differ: a trip that stops at its first entry has loaded one
// entry it does not look at.
//
// Bounds: a walk that starts on (or reaches in its first slot) a window's sentinel loads the
// entry behind it.  For the last window of the array that is the 12 bytes behind the array: the
// allocation keeps kWalkPairSlack bytes there (build_fine, pcp_fine.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PCP_WP_HD __host__ __device__ __forceinline__
#else
#define PCP_WP_HD inline
#endif

namespace pcp {

constexpr size_t kWalkEntryBytes = 12;   // one packed entry: x, y, z
// entries a trip loads behind the one it must test, and the bytes the array keeps behind its
// last entry for them: slack >= kWalkEntryBytes per extra entry loaded
constexpr int kWalkPairExtra = 1;
constexpr size_t kWalkPairSlack = 16;
static_assert(kWalkPairSlack >= kWalkPairExtra * kWalkEntryBytes, "an extra entry per trip");

// FLANN's L2_Simple<float> against r2 (pcp_stencil.hpp's flann_within, restated on scalars) and
// the walk's exit: the entry lies rexit or more below q.  Returns stop; within: the answer.
PCP_WP_HD bool walk_test(float px, float py, float pz, float qx, float qy, float qz, float r2,
                         float rexit, bool &within) {
    const float d0 = qx - px, d1 = qy - py, d2 = qz - pz;
    float acc = 0.0f;
    acc = acc + d0 * d0;
    acc = acc + d1 * d1;
    acc = acc + d2 * d2;
    within = acc < r2;
    return within | (qz - pz >= rexit);
}

// one trip over entries a (k) and b (k + 1), both already loaded: b is tested only where a did
// not stop.  tests: the entries tested, 1 or 2.
PCP_WP_HD bool walk_pair_step(float ax, float ay, float az, float bx, float by, float bz,
                              float qx, float qy, float qz, float r2, float rexit, bool &within,
                              uint32_t &tests) {
    tests = 1;
    if (walk_test(ax, ay, az, qx, qy, qz, r2, rexit, within)) return true;
    tests = 2;
    return walk_test(bx, by, bz, qx, qy, qz, r2, rexit, within);
}

// the entry at index k of a packed run (32-bit byte offset, as the march addresses it)
PCP_WP_HD const float *walk_entry(const float *pts, uint32_t k) {
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(pts) +
                                           ((k << 3) + (k << 2)));
}

struct WalkResult {
    bool within;      // an entry within r of q
    uint32_t last;    // index of the last entry tested
    uint32_t tests;   // entries tested
};

// the one-entry walk from k (scan_window3 as it was)
PCP_WP_HD WalkResult walk_single(const float *pts, uint32_t k, float qx, float qy, float qz,
                                 float r2, float rexit) {
    WalkResult w{false, k, 0};
    bool stop;
    do {
        const float *f = walk_entry(pts, k);
        w.last = k++;
        w.tests += 1;
        stop = walk_test(f[0], f[1], f[2], qx, qy, qz, r2, rexit, w.within);
    } while (!stop);
    return w;
}

// the paired walk from k: each trip reads the six floats of entries k, k + 1
PCP_WP_HD WalkResult walk_paired(const float *pts, uint32_t k, float qx, float qy, float qz,
                                 float r2, float rexit) {
    WalkResult w{false, k, 0};
    bool stop;
    do {
        const float *f = walk_entry(pts, k);
        const float ax = f[0], ay = f[1], az = f[2], bx = f[3], by = f[4], bz = f[5];
        uint32_t t;
        stop = walk_pair_step(ax, ay, az, bx, by, bz, qx, qy, qz, r2, rexit, w.within, t);
        w.last = k + t - 1;
        w.tests += t;
        k += 2;
    } while (!stop);
    return w;
}

}  // namespace pcp
