// Stand-alone check of pcp_fan_cull.hpp (no GPU, no HIP): random boxes, pose heights,
// elevation tables (ascending, descending, unsorted) and step tables.
//  * every (pose, ring) the rule calls dead has all K sample heights, recomputed in long double,
//    outside the box;
//  * a pose's interval and the call's interval contain every ring that is not dead, and over a
//    sorted table a pose's interval holds live rings only;
//  * the bisection (with and without a hint) agrees with the plain walk over the rings;
//  * the live waves cover every ray of a live ring.
// Build: c++ -std=c++17 -I pointcloud_processor_amd/csrc tests/native/fan_cull_selftest.cpp
// (add -fsanitize=address,undefined for a sanitizer run of the host logic).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pcp_fan_cull.hpp"

using namespace pcp;

static int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (++fails < 20) {                        \
                std::printf("FAIL %s: ", #c);          \
                std::printf(__VA_ARGS__);              \
                std::printf("\n");                     \
            }                                          \
        }                                              \
    } while (0)

int main() {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    long dead_pairs = 0, live_pairs = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        // box: a terrain-like slab, sometimes far from the origin or very thin
        const double scale = trial % 7 == 0 ? 3000.0 : trial % 5 == 0 ? 0.01 : 3.0;
        const double zc = (u01(rng) - 0.5) * 2.0 * scale;
        const double half = u01(rng) * 1.5 + 1e-3;
        const double zlo_d = zc - half, zhi_d = zc + half;
        const double zlo = (double)(float)zlo_d, zhi = (double)(float)zhi_d;   // GridView.fb
        // steps: 0.5, 0.8, ... by repeated addition, as step_table()
        const double end = 0.6 + u01(rng) * (trial % 3 == 0 ? 120.0 : 15.0);
        std::vector<double> steps;
        for (double s = 0.5; s < end; s += 0.3) steps.push_back(s);
        const int K = (int)steps.size();
        // elevation table
        const int n_el = 1 + (int)(u01(rng) * 70.0);
        const int kind = trial % 4;   // 0, 1: ascending, 2: descending, 3: unsorted
        double e0 = -1.55 + u01(rng) * 1.5, e1 = e0 + u01(rng) * (1.55 - e0);
        if (kind == 2) std::swap(e0, e1);
        if (kind == 3) e1 = e0 + 1.0 + u01(rng) * 5.0;   // past the zenith
        std::vector<double> se(n_el);
        for (int j = 0; j < n_el; ++j) se[j] = std::sin(e0 + (e1 - e0) * (j + 0.5) / n_el);
        const int order = fan_se_order(se.data(), n_el);
        if (kind < 2) CHECK(order == 1 || n_el == 1, "ascending table, order %d", order);
        if (kind == 2) CHECK(order != 0, "descending table, order %d", order);
        // poses: around the box, on the rule's edge, far away
        const int P = 1 + (int)(u01(rng) * 12.0);
        std::vector<double> pose(8 * (size_t)P, 0.0);
        for (int k = 0; k < P; ++k) {
            double pz;
            const int how = (int)(u01(rng) * 6.0);
            const int j = (int)(u01(rng) * n_el);
            if (how == 0) pz = zc + (u01(rng) - 0.5) * 2.0 * half;                  // inside
            else if (how == 1) pz = zhi + u01(rng) * 20.0;                          // above
            else if (how == 2) pz = zlo - u01(rng) * 20.0;                          // below
            else if (how == 3) pz = zhi - se[j] * steps.back() + (u01(rng) - 0.5) * 4e-6;
            else if (how == 4) pz = zlo - se[j] * steps.front() + (u01(rng) - 0.5) * 4e-6;
            else pz = zc + (u01(rng) - 0.5) * 400.0;                                // far
            pose[8 * (size_t)k + 2] = pz;
        }
        std::vector<uint32_t> pp(2 * (size_t)P);
        const FanLive call = fan_live_rings(zlo, zhi, pose.data() + 2, (uint64_t)P, 8, se.data(),
                                            n_el, steps.front(), steps.back(), pp.data(), 2);
        CHECK(call.j0 >= 0 && call.j0 <= call.j1 && call.j1 <= n_el, "call [%d, %d)", call.j0,
              call.j1);
        for (int k = 0; k < P; ++k) {
            const double pz = pose[8 * (size_t)k + 2];
            const int pj0 = (int)pp[2 * k], pj1 = (int)pp[2 * k + 1];
            CHECK(pj0 >= 0 && pj0 <= pj1 && pj1 <= n_el, "pose [%d, %d)", pj0, pj1);
            const FanLive nohint = fan_pose_live(zlo, zhi, pz, se.data(), n_el, order,
                                                 steps.front(), steps.back());
            const FanLive walk = fan_pose_live(zlo, zhi, pz, se.data(), n_el, 0, steps.front(),
                                               steps.back());
            CHECK(nohint.j0 == pj0 && nohint.j1 == pj1, "hint changes the answer");
            CHECK(walk.j0 == pj0 && walk.j1 == pj1, "bisection [%d, %d) vs walk [%d, %d)", pj0,
                  pj1, walk.j0, walk.j1);
            for (int j = 0; j < n_el; ++j) {
                const bool dead = fan_pair_dead(zlo, zhi, pz, se[j], steps.front(), steps.back());
                if (dead) {
                    ++dead_pairs;
                    // all K heights outside the box the kernel clips against (and, by the
                    // margin, outside the double box it was rounded from)
                    for (int q = 0; q < K; ++q) {
                        const long double h = (long double)pz + (long double)se[j] * steps[q];
                        CHECK(h > (long double)zhi || h < (long double)zlo,
                              "dead pair with a sample inside: pz %.17g se %.17g s %.17g", pz,
                              se[j], steps[q]);
                        CHECK(h > (long double)zhi_d || h < (long double)zlo_d,
                              "dead pair inside the unrounded box");
                    }
                    if (order != 0) CHECK(j < pj0 || j >= pj1, "dead ring %d in [%d, %d)", j, pj0, pj1);
                } else {
                    ++live_pairs;
                    CHECK(j >= pj0 && j < pj1, "live ring %d outside the pose's [%d, %d)", j, pj0,
                          pj1);
                    CHECK(j >= call.j0 && j < call.j1, "live ring %d outside the call's [%d, %d)",
                          j, call.j0, call.j1);
                }
            }
        }
        // waves
        const int n_az = trial % 2 ? 64 * (1 + (int)(u01(rng) * 4.0)) : 1 + (int)(u01(rng) * 200.0);
        const FanWaves W = fan_live_waves(call, n_az, n_el);
        const uint64_t rays = (uint64_t)n_az * n_el;
        CHECK(W.w0 <= W.w1 && (uint64_t)W.w1 * 64 < rays + 64, "waves [%u, %u)", W.w0, W.w1);
        for (int j = call.j0; j < call.j1; ++j) {
            const uint64_t a = (uint64_t)j * n_az, b = a + n_az - 1;
            CHECK(a / 64 >= W.w0 && b / 64 < W.w1, "ring %d outside waves [%u, %u)", j, W.w0, W.w1);
        }
    }
    // non-finite input is live
    const double se1[1] = {-0.5};
    const FanLive nanp = fan_pose_live(-1.0, 0.1, std::nan(""), se1, 1, 1, 0.5, 14.9);
    CHECK(nanp.j0 == 0 && nanp.j1 == 1, "NaN pose height");
    CHECK(!fan_pair_dead(-1.0, 0.1, 1.0, std::nan(""), 0.5, 14.9), "NaN direction");
    CHECK(dead_pairs > 10000 && live_pairs > 10000, "coverage: %ld dead, %ld live", dead_pairs,
          live_pairs);
    std::printf("pairs: %ld dead, %ld live\n", dead_pairs, live_pairs);
    std::printf(fails ? "FAILED\n" : "ok\n");
    return fails ? 1 : 0;
}
