// The pose row of a level fan query (DESIGN.md §6b "VALU diet 2"): what fan_enqueue stages per
// pose and fan_body / k_scan_resolve read back.  Plain C++ with no HIP dependency, usable from
// host and device: tests/native/fan_row_selftest.cpp checks the layout and every float stand-alone.
//
// Beside the pose itself the row carries the float terms of the march's preamble whose operands
// are the pose and the terrain's GridView alone -- the same value in all 64 lanes of a wave, which
// the kernel used to derive per lane and pose:
//
//   the clip's six differences    fb[i] - (float)p[i / 2]                   (clip_kf, Skip 3)
//   the probe origin's three      ((float)p[a] - flo[a]) * finv_c           (march, A = base + d h)
//
// ((float)p itself is not carried: with those nine no kernel needs it.)
//
// They are formed here in float with the kernel's former expressions, operation by operation.
// IEEE single arithmetic without contraction and without excess precision (the build's
// -ffp-contract=off; x86-64 SSE and the device's v_sub_f32 / v_mul_f32 both round to nearest
// even) gives the same bits on the host as on the device: that equality is the
// contract, and the selftest restates it.  The row depends on the terrain's view, so it is built
// per query; nothing is kept across calls.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCP_ROW_HD __host__ __device__ inline
#else
#define PCP_ROW_HD inline
#endif

namespace pcp {

// doubles per level pose row (128 bytes: a row never straddles a cache line, and its float block
// is 16-byte aligned for the kernel's LDS reads).  The one stride of fan_enqueue's staging,
// fan_body's LDS rows and k_scan_resolve.
constexpr int kFanRow = 16;
// slots, in doubles
enum { FR_X = 0, FR_Y, FR_Z, FR_PITCH, FR_YAW, FR_CY, FR_SY,
       FR_LIVE,        // two uint32: the pose's live rings [j0, j1) (pcp_fan_cull.hpp)
       FR_F32 };       // the float block: kFanRowFloats floats, then zero padding
// the float block, in floats from FR_F32
enum { FRF_CLIP = 0,   // 6: fb[i] - (float)p[i / 2], i = x0, x1, y0, y1, z0, z1
       FRF_BASE = 6,   // 3: ((float)p[a] - flo[a]) * finv_c
       kFanRowFloats = 9 };
static_assert(FR_F32 % 2 == 0, "the float block starts on 16 bytes");
static_assert(FR_F32 * 2 + kFanRowFloats <= kFanRow * 2, "the float block fits the row");
// uint32 index of the live-ring pair inside a row, and between two rows' pairs
constexpr int kFanRowLiveU32 = FR_LIVE * 2;
constexpr int kFanRowStrideU32 = kFanRow * 2;

// the part of a GridView the row depends on (GridView itself needs the HIP vector types)
struct FanRowGrid {
    float fb[6];              // GridView.fb
    float flo[3];             // GridView.flo_x, flo_y, flo_z
    float finv_c;             // GridView.finv_c
};

PCP_ROW_HD const float *fan_row_floats(const double *row) {
    return reinterpret_cast<const float *>(row + FR_F32);
}

// pose5 (x, y, z, pitch, yaw) -> its row; host only (libm's cos and sin, as the oracle's).  The
// live-ring pair is left 0, 0 for the caller (fan_live_rings writes it in place).
inline void fan_row_fill(const double *pose5, const FanRowGrid &g, double *row) {
    for (int q = 0; q < 5; ++q) row[q] = pose5[q];
    row[FR_CY] = std::cos(pose5[4]);
    row[FR_SY] = std::sin(pose5[4]);
    uint32_t *live = reinterpret_cast<uint32_t *>(row + FR_LIVE);
    live[0] = 0u;
    live[1] = 0u;
    float *f = reinterpret_cast<float *>(row + FR_F32);
    for (int a = 0; a < 3; ++a) {
        const float p = (float)pose5[a];
        f[FRF_CLIP + 2 * a] = g.fb[2 * a] - p;
        f[FRF_CLIP + 2 * a + 1] = g.fb[2 * a + 1] - p;
        const float rel = p - g.flo[a];
        f[FRF_BASE + a] = rel * g.finv_c;
    }
    for (int q = FR_F32 * 2 + kFanRowFloats; q < kFanRow * 2; ++q)
        reinterpret_cast<float *>(row)[q] = 0.0f;
}

}  // namespace pcp
