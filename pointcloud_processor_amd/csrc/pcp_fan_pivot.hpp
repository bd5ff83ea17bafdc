// The pivot of a fine window ("Skip 6"): the one point of the window the fan
// march tests before it walks the window's run.  Plain C++ with no HIP dependency: pcp_fine.hip
// picks the pivots through these functions and tests/native/fan_pivot_selftest.cpp checks the
// rule stand-alone.
//
// The window of fine cell (wx, wy) is a z-descending run, random in xy on level ground, and a
// candidate sample q lies in the cell's rectangle (up to the probe's error).  The member most
// likely within r of q is the one nearest the rectangle's centre in xy:
//
//   pivot = the member with the smallest squared xy distance, in double, to
//           (ox + (wx + 0.5) c_f, oy + (wy + 0.5) c_f);
//           ties: the higher z, then the lower original index.
//
// The march tests the pivot with the walk's own predicate; a pivot within r blocks the sample
// (radiusSearch(q, r) > 0 asks for any point, and the pivot is a terrain point), any other
// pivot leaves the candidate to the walk.  So the choice rule bears on speed alone, never on a
// result: any member of the window would be exact.
//
// The table: one 12-byte (x, y, z) record per fine cell in 8 x 8 xy tiles of 64 records,
// tile rows x-fastest -- the band records' addressing without the iz term -- over the padded
// tile plane, so the march's clamped (ix, iy) always indexes inside it.  A window without a
// point and every padding cell hold the sentinel (NaN, NaN, -inf): never within r.  (Packed as
// the window entries are: 16-byte records measured 1.5-2 % slower)
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PCP_PIV_HD __host__ __device__ inline
#else
#define PCP_PIV_HD inline
#endif

namespace pcp {

// a window member as the choice sees it: d2 from pivot_d2, z, original index
struct PivotKey {
    double d2;
    float z;
    uint32_t idx;
};

// squared xy distance of (px, py) to the centre of fine cell (wx, wy)
PCP_PIV_HD double pivot_d2(double ox, double oy, double cf, uint32_t wx, uint32_t wy, float px,
                           float py) {
    const double dx = (double)px - (ox + ((double)wx + 0.5) * cf);
    const double dy = (double)py - (oy + ((double)wy + 0.5) * cf);
    return dx * dx + dy * dy;
}

// a is chosen over b
PCP_PIV_HD bool pivot_better(const PivotKey &a, const PivotKey &b) {
    if (a.d2 != b.d2) return a.d2 < b.d2;
    if (a.z != b.z) return a.z > b.z;
    return a.idx < b.idx;
}

constexpr size_t kPivotBytes = 12;   // one record: x, y, z

// tiles per axis and the record of cell (wx, wy)
PCP_PIV_HD uint32_t pivot_tiles(uint32_t fn) { return (fn + 7u) >> 3; }
PCP_PIV_HD size_t pivot_index(uint32_t tx, uint32_t wx, uint32_t wy) {
    return (((size_t)(wy >> 3) * tx + (wx >> 3)) << 6) | ((wy & 7u) << 3) | (wx & 7u);
}

}  // namespace pcp
