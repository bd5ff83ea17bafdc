// Stand-alone check of pcp_fan_row.hpp (no GPU, no HIP): the level fan's pose row.
//  * the layout: the stride is the one constant the device code uses (kFanRow; fan_body's LDS
//    rows, fan_enqueue's staging and k_scan_resolve all take it from the header), the float block
//    is 16-byte aligned and inside the row, the live-ring pair sits in its slot;
//  * every float of the row equals the kernel's former per-lane expression restated here in
//    float, bit for bit: fb[i] - (float)p for the clip, ((float)p - flo) * finv_c for the probe
//    origin -- and the clip's slab times from the row's differences are those of
//    fan_clip_slabs from the box and the pose (pcp_fan_clip.hpp);
//  * poses at the origin, at +-3 km in x / y / z, with negative coordinates, and with yaws whose
//    cosine or sine is exactly 0.
// Build: c++ -std=c++17 -ffp-contract=off -I pointcloud_processor_amd/csrc
//        tests/native/fan_row_selftest.cpp   (also with -fsanitize=address,undefined)
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcp_fan_clip.hpp"
#include "pcp_fan_row.hpp"

using namespace pcp;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}
static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}
// the kernel's former expressions, each operation on its own (volatile: no value is kept in a
// wider register or folded with its neighbour, whatever the flags)
static float sub_f(float a, float b) {
    volatile float r = a - b;
    return r;
}
static float mul_f(float a, float b) {
    volatile float r = a * b;
    return r;
}

int main() {
    static_assert(kFanRow == 16, "a level pose row is 16 doubles (128 bytes)");
    static_assert(FR_LIVE == 7, "the live-ring pair keeps the eighth double's place");
    static_assert(kFanRowLiveU32 == 14 && kFanRowStrideU32 == 32, "the pair's uint32 indices");
    static_assert((FR_F32 * sizeof(double)) % 16 == 0, "the float block is 16-byte aligned");
    static_assert(FR_F32 * sizeof(double) + kFanRowFloats * sizeof(float) <=
                      kFanRow * sizeof(double),
                  "the float block lies inside the row");
    static_assert(FRF_CLIP == 0 && FRF_BASE == 6 && kFanRowFloats == 9,
                  "the float block's slots");

    // two views: a terrain near the origin and one 3 km out (float spacing 2.4e-4 m there)
    const FanRowGrid grids[] = {
        {{-2.0571f, 8.0571f, -4.0571f, 6.0571f, -1.5571f, 0.3571f},
         {-2.25f, -4.25f, -1.75f},
         1.0f / 0.112f},
        {{2997.9429f, 3008.0571f, 2995.9429f, 3006.0571f, 2998.4429f, 3000.3571f},
         {2997.75f, 2995.75f, 2998.25f},
         1.0f / 0.112f},
        {{-3008.06f, -2997.94f, -3006.06f, -2995.94f, -3000.36f, -2998.44f},
         {-3008.25f, -3006.25f, -3000.5f},
         8.928571f},
    };
    const double kPi = 3.14159265358979323846;
    const double poses[][5] = {
        {0.0, 0.0, 0.0, 0.0, 0.0},                       // the origin; sin(yaw) = 0 exactly
        {3000.0, 0.0, 0.0, -0.4, 1.0},                   // +-3 km, one axis at a time
        {-3000.0, 0.0, 0.0, -0.4, 1.0},
        {0.0, 3000.0, 0.0, 0.1, -2.0},
        {0.0, -3000.0, 0.0, 0.1, -2.0},
        {0.0, 0.0, 3000.0, 0.0, 0.5},
        {0.0, 0.0, -3000.0, 0.0, 0.5},
        {3000.123456789, 3001.987654321, 2999.555555555, -0.3, 0.7},
        {-3000.123456789, -3001.987654321, -2999.555555555, -0.3, 0.7},
        {-1.1, -3.3, -0.5, -0.2, -0.0},                  // negative coordinates, yaw -0
        {1.0000001, 2.0000002, 1.1, 0.0, 0.0},           // not floats: (float)p rounds
        {7.25, -3.75, 1.1, 0.0, std::acos(0.0)},         // libm's pi / 2: cos = 6.1e-17, not 0
        {0.3, 0.4, 1.1, 0.0, kPi},
    };
    const int n_pose = (int)(sizeof poses / sizeof poses[0]);
    // yaws whose cosine or sine is exactly 0: sin(0) = 0, sin(-0) = -0; cos is exactly 0 for
    // no double, so the exact zeros a row can hold are the sines'
    CHECK(std::sin(poses[0][4]) == 0.0 && std::cos(poses[0][4]) == 1.0);
    CHECK(std::sin(poses[9][4]) == 0.0 && std::signbit(std::sin(poses[9][4])));

    for (const FanRowGrid &g : grids) {
        // rows side by side, as fan_enqueue stages them, with guard values around
        std::vector<double> buf((size_t)kFanRow * n_pose + 2, -7.0);
        double *rows = buf.data() + 1;
        for (int k = 0; k < n_pose; ++k) fan_row_fill(poses[k], g, rows + (size_t)kFanRow * k);
        CHECK(buf.front() == -7.0 && buf.back() == -7.0);
        // the live rings, written in place the way fan_live_rings does
        uint32_t *lr = reinterpret_cast<uint32_t *>(rows) + kFanRowLiveU32;
        for (int k = 0; k < n_pose; ++k) {
            CHECK(lr[(size_t)kFanRowStrideU32 * k] == 0u && lr[(size_t)kFanRowStrideU32 * k + 1] == 0u);
            lr[(size_t)kFanRowStrideU32 * k] = 3u + (uint32_t)k;
            lr[(size_t)kFanRowStrideU32 * k + 1] = 100u + (uint32_t)k;
        }
        for (int k = 0; k < n_pose; ++k) {
            const double *row = rows + (size_t)kFanRow * k;
            const double *p = poses[k];
            for (int q = 0; q < 5; ++q) CHECK(bits(row[q]) == bits(p[q]));
            CHECK(bits(row[FR_CY]) == bits(std::cos(p[4])));
            CHECK(bits(row[FR_SY]) == bits(std::sin(p[4])));
            uint32_t pair[2];
            std::memcpy(pair, row + FR_LIVE, sizeof pair);
            CHECK(pair[0] == 3u + (uint32_t)k && pair[1] == 100u + (uint32_t)k);
            const float *f = fan_row_floats(row);
            CHECK((const void *)f == (const void *)(row + 8));
            float pf[3];
            for (int a = 0; a < 3; ++a) {
                pf[a] = (float)p[a];
                CHECK(bits(f[FRF_CLIP + 2 * a]) == bits(sub_f(g.fb[2 * a], pf[a])));
                CHECK(bits(f[FRF_CLIP + 2 * a + 1]) == bits(sub_f(g.fb[2 * a + 1], pf[a])));
                CHECK(bits(f[FRF_BASE + a]) == bits(mul_f(sub_f(pf[a], g.flo[a]), g.finv_c)));
            }
            for (int q = kFanRowFloats; q < (kFanRow - FR_F32) * 2; ++q) CHECK(bits(f[q]) == 0u);
            // the clip from the row's differences is the clip from the box and the pose, for
            // directions with zero components (infinite reciprocals) among them
            const float dirs[][3] = {{0.6f, -0.64f, -0.48f}, {1.0f, 0.0f, 0.0f}, {0.0f, -1.0f, 0.0f},
                                     {0.0f, 0.0f, -1.0f},    {0.8f, 0.0f, 0.6f}, {6.1e-17f, 1.0f, 0.0f}};
            for (const auto &d : dirs) {
                const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
                float a0, a1, b0, b1;
                const bool ha = fan_clip_slabs(g.fb, pf, inv, a0, a1);
                const bool hb = fan_clip_slabs_rel(f + FRF_CLIP, inv, b0, b1);
                CHECK(ha == hb && bits(a0) == bits(b0) && bits(a1) == bits(b1));
            }
        }
    }
    if (fails) {
        std::printf("%d failures\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
