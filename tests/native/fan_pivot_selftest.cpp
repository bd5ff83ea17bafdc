// Stand-alone check of pcp_fan_pivot.hpp (DESIGN.md §5 Skip 6) with the host compiler: the
// choice rule, applied in run order as the build kernel applies it, against brute force over
// all members of a few hundred random windows, and the table's addressing.  No GPU call.
// Prints "ok" on success.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "pcp_fan_pivot.hpp"

using namespace pcp;

namespace {

int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++fails < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

struct Pt {
    float x, y, z;
    uint32_t idx;
};

}  // namespace

int main() {
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double CF = 0.06, R = 0.057;
    long ties = 0, windows = 0;
    for (int trial = 0; trial < 400; ++trial) {
        // a window far from or near the origin, its members within R of the cell's rectangle
        const double ox = (trial & 1) ? 2999.7 : -1.3, oy = (trial & 2) ? -2000.2 : 0.4;
        const uint32_t wx = (uint32_t)(U(rng) * 200.0), wy = (uint32_t)(U(rng) * 200.0);
        const int n = 1 + (int)(U(rng) * 24.0);
        std::vector<Pt> run;
        for (int i = 0; i < n; ++i) {
            Pt p;
            p.x = (float)(ox + wx * CF - R + (CF + 2.0 * R) * U(rng));
            p.y = (float)(oy + wy * CF - R + (CF + 2.0 * R) * U(rng));
            p.z = (float)(0.4 * U(rng));
            p.idx = (uint32_t)(U(rng) * 1e6);
            run.push_back(p);
            // exact ties: the same xy at another height or index, and the mirror image
            if (U(rng) < 0.3) {
                Pt q = p;
                q.z = U(rng) < 0.5 ? p.z : (float)(0.4 * U(rng));
                q.idx = p.idx + 1u + (uint32_t)(U(rng) * 10.0);
                run.push_back(q);
            }
        }
        // the run's order: descending z, ties by ascending original index
        std::sort(run.begin(), run.end(), [](const Pt &a, const Pt &b) {
            return a.z != b.z ? a.z > b.z : a.idx < b.idx;
        });
        // the build's pass: keep the better of (kept, next) along the run
        size_t kept = 0;
        PivotKey kb{pivot_d2(ox, oy, CF, wx, wy, run[0].x, run[0].y), run[0].z, run[0].idx};
        for (size_t j = 1; j < run.size(); ++j) {
            const PivotKey k{pivot_d2(ox, oy, CF, wx, wy, run[j].x, run[j].y), run[j].z, run[j].idx};
            if (pivot_better(k, kb)) {
                kb = k;
                kept = j;
            }
        }
        // brute force: the stated rule over all members, from the centre as stated
        const double cx = ox + ((double)wx + 0.5) * CF, cy = oy + ((double)wy + 0.5) * CF;
        double dmin = INFINITY;
        for (const Pt &p : run) {
            const double dx = (double)p.x - cx, dy = (double)p.y - cy;
            dmin = std::fmin(dmin, dx * dx + dy * dy);
        }
        int at_min = 0;
        float zbest = -INFINITY;
        uint32_t ibest = 0xFFFFFFFFu;
        for (const Pt &p : run) {
            const double dx = (double)p.x - cx, dy = (double)p.y - cy;
            if (dx * dx + dy * dy != dmin) continue;
            ++at_min;
            if (p.z > zbest || (p.z == zbest && p.idx < ibest)) {
                zbest = p.z;
                ibest = p.idx;
            }
        }
        CHECK(kb.d2 == dmin);                                   // no member is strictly nearer
        CHECK(run[kept].z == zbest && run[kept].idx == ibest);  // ties: higher z, lower index
        if (at_min > 1) ++ties;
        ++windows;
        // a total order: irreflexive, and exactly one of two different keys wins
        for (size_t a = 0; a < run.size(); ++a)
            for (size_t b = 0; b < run.size(); ++b) {
                const PivotKey ka{pivot_d2(ox, oy, CF, wx, wy, run[a].x, run[a].y), run[a].z, run[a].idx};
                const PivotKey kc{pivot_d2(ox, oy, CF, wx, wy, run[b].x, run[b].y), run[b].z, run[b].idx};
                const bool same = ka.d2 == kc.d2 && ka.z == kc.z && ka.idx == kc.idx;
                CHECK(same ? !pivot_better(ka, kc) : pivot_better(ka, kc) != pivot_better(kc, ka));
            }
    }
    CHECK(windows == 400 && ties > 50);

    // the table's addressing: a bijection of the padded plane, tile rows x-fastest
    for (uint32_t fnx : {1u, 8u, 9u, 71u}) {
        const uint32_t fny = fnx == 71u ? 54u : fnx + 3u;
        const uint32_t tx = pivot_tiles(fnx), ty = pivot_tiles(fny);
        CHECK(tx * 8u >= fnx && (tx - 1u) * 8u < fnx);
        std::vector<int> seen((size_t)tx * ty * 64, 0);
        for (uint32_t y = 0; y < ty * 8u; ++y)
            for (uint32_t x = 0; x < tx * 8u; ++x) {
                const size_t r = pivot_index(tx, x, y);
                CHECK(r < seen.size());
                if (r < seen.size()) ++seen[r];
                CHECK(r / 64 == (size_t)(y / 8) * tx + x / 8 && r % 64 == (y % 8) * 8 + x % 8);
            }
        for (int s : seen) CHECK(s == 1);
    }

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("windows %ld with ties %ld\nok\n", windows, ties);
    return 0;
}
