// The direction of a mounted sensor's ray (include/pcp_abi.h): the fan's local
// direction l = (ce_j ca_i, ce_j sa_i, se_j) turned by the mount's roll, pitch and yaw.  Plain
// C++ with no HIP dependency, usable from host and device: the mounted march (fan_body, MT) and
// k_scan_resolve<true> both call fan_dir(), so that the resolve's query point is the march's
// bit for bit, and tests/native/fan_dir_selftest.cpp prints its bits for tests/mount_ref.py.
//
// Three plane rotations in double, every product and sum rounded on its own (the build's
// -ffp-contract=off; no fused multiply-add may be formed here):
//
//   x1 = lx                 y1 = ly cr - lz sr      z1 = ly sr + lz cr    roll about the boresight
//   x2 = x1 cp - z1 sp      y2 = y1                 z2 = x1 sp + z1 cp    pitch: (1,0,0) -> (cp,0,sp)
//   dx = cy x2 - sy y2      dy = sy x2 + cy y2      dz = z2               yaw, as the level fan
//
// pitch is the elevation of the boresight (negative looks down).  With roll = pitch = 0 (cr = cp
// = 1, sr = sp = 0) every product with 1 is exact and every product with 0 is a zero, so the
// direction equals the level fan's (cy lx - sy ly, sy lx + cy ly, lz) as a value; a component
// can differ in the sign of a zero only.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PCP_DIR_HD __host__ __device__ inline
#else
#define PCP_DIR_HD inline
#endif

namespace pcp {

// The pose row of a mounted query, kFanDirRow doubles per sensor: x, y, z, cos / sin of roll,
// of pitch, of yaw (the host C library's), padded to a multiple of 32 bytes.
constexpr int kFanDirRow = 12;
enum { FD_X = 0, FD_Y, FD_Z, FD_CR, FD_SR, FD_CP, FD_SP, FD_CY, FD_SY };

// poses6 row (x, y, z, roll, pitch, yaw) -> pose row; host only.  cos and sin are libm's two
// double functions (the definition's): a build that merges the pair of one argument into sincos
// gets results that differ from theirs in rare last bits (hipcc does not; g++: -fno-builtin)
inline void fan_dir_row(const double *pose6, double *row) {
    row[FD_X] = pose6[0];
    row[FD_Y] = pose6[1];
    row[FD_Z] = pose6[2];
    row[FD_CR] = std::cos(pose6[3]);
    row[FD_SR] = std::sin(pose6[3]);
    row[FD_CP] = std::cos(pose6[4]);
    row[FD_SP] = std::sin(pose6[4]);
    row[FD_CY] = std::cos(pose6[5]);
    row[FD_SY] = std::sin(pose6[5]);
    for (int q = FD_SY + 1; q < kFanDirRow; ++q) row[q] = 0.0;
}

struct FanDir {
    double x, y, z;
};

// row: a pose row (only the six cosines and sines are read); (lx, ly, lz): the local direction
PCP_DIR_HD FanDir fan_dir(const double *row, double lx, double ly, double lz) {
    const double cr = row[FD_CR], sr = row[FD_SR], cp = row[FD_CP], sp = row[FD_SP];
    const double cy = row[FD_CY], sy = row[FD_SY];
    const double y1 = ly * cr - lz * sr;
    const double z1 = ly * sr + lz * cr;
    const double x2 = lx * cp - z1 * sp;
    const double z2 = lx * sp + z1 * cp;
    FanDir d;
    d.x = cy * x2 - sy * y1;
    d.y = sy * x2 + cy * y1;
    d.z = z2;
    return d;
}

}  // namespace pcp
