// Stand-alone check of pcp_walk_pair.hpp ("round trips") with the host compiler:
// the paired walk (two packed entries per trip) against the one-entry walk over random
// z-descending runs ended by the sentinel (NaN, NaN, -inf) -- the answer, the index of the last
// entry tested and the number of tests must agree.  The entry array is a heap block of exactly
// nent * 12 + kWalkPairSlack bytes, as build_fine allocates it, with the last run at its end: built
// with -fsanitize=address a read past the slack fails.  No GPU call.  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "pcp_walk_pair.hpp"

using namespace pcp;

namespace {

int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++fails < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

// what the cases must have covered, by the slot (0: entry k, 1: entry k + 1) of the last test
struct Cover {
    long hit[2] = {0, 0}, exit_[2] = {0, 0}, sentinel[2] = {0, 0};
    long start_parity[2] = {0, 0}, start_on_sentinel = 0, tail_run = 0, walks = 0;
    long by_len[7] = {0, 0, 0, 0, 0, 0, 0};   // runs of 0..5 entries, [6]: longer
} cov;

struct Run {
    uint32_t first, n;   // entries [first, first + n), the sentinel at first + n
};

size_t g_bytes = 0;   // the array's allocation

void one_walk(const float *pts, const Run &run, uint32_t start, float qx, float qy, float qz,
              float r2, float rexit) {
    const WalkResult a = walk_single(pts, start, qx, qy, qz, r2, rexit);
    const WalkResult b = walk_paired(pts, start, qx, qy, qz, r2, rexit);
    CHECK(a.within == b.within);
    CHECK(a.last == b.last);
    CHECK(a.tests == b.tests);
    CHECK(a.last <= run.first + run.n);   // never past the run's sentinel
    CHECK(a.tests == a.last - start + 1);
    // the bytes the paired walk touched: whole trips from start
    const uint32_t trips = (b.tests + 1) / 2;
    CHECK(((size_t)start + 2 * (size_t)trips) * kWalkEntryBytes <= g_bytes);
    const int slot = (int)((a.last - start) & 1u);
    const bool at_sentinel = a.last == run.first + run.n;
    if (a.within) cov.hit[slot] += 1;
    else if (at_sentinel) cov.sentinel[slot] += 1;
    else cov.exit_[slot] += 1;
    cov.start_parity[start & 1u] += 1;
    if (start == run.first + run.n) cov.start_on_sentinel += 1;
    cov.walks += 1;
}

}  // namespace

int main() {
    std::mt19937 rng(20261021u);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const float r = 0.05f, r2 = r * r;
    // the walk's exit distance: the least float whose square is >= r2
    float rexit = std::sqrt(r2);
    while (rexit * rexit >= r2) rexit = std::nextafter(rexit, 0.0f);
    while (rexit * rexit < r2) rexit = std::nextafter(rexit, 1.0f);
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int trial = 0; trial < 60; ++trial) {
        // the runs of one array: every length 0..5 and two long ones, in random order, a run of
        // the trial's own length last (so every length is the array's tail in some trial)
        std::vector<uint32_t> lens = {0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 17, 64};
        for (size_t i = lens.size(); i > 1; --i) std::swap(lens[i - 1], lens[rng() % i]);
        lens.push_back((uint32_t)(trial % 8 == 7 ? 33 : trial % 8 == 6 ? 0 : trial % 8));
        if (trial & 8) lens.insert(lens.begin(), 1u);   // shifts every later run's parity
        std::vector<Run> runs;
        size_t nent = 0;
        for (uint32_t n : lens) {
            runs.push_back(Run{(uint32_t)nent, n});
            nent += (size_t)n + 1;
        }
        g_bytes = nent * kWalkEntryBytes + kWalkPairSlack;
        float *pts = static_cast<float *>(std::malloc(g_bytes));
        CHECK(pts != nullptr);
        if (!pts) return 1;
        std::memset(pts, 0xA5, g_bytes);
        const float base = (trial % 3 == 2) ? 3000.0f : 0.0f;   // near and 3 km out
        for (const Run &run : runs) {
            float z = base + 1.0f + U(rng);
            for (uint32_t e = 0; e < run.n; ++e) {
                float *f = pts + 3 * (size_t)(run.first + e);
                f[0] = base + 0.2f * U(rng);
                f[1] = base + 0.2f * U(rng);
                f[2] = z;
                // gaps from 0 (equal heights) to beyond r
                const float u = U(rng);
                z -= u < 0.2f ? 0.0f : u < 0.8f ? 0.03f * U(rng) : 0.12f * U(rng);
            }
            float *s = pts + 3 * (size_t)(run.first + run.n);
            s[0] = nan;
            s[1] = nan;
            s[2] = -inf;
        }
        for (size_t ri = 0; ri < runs.size(); ++ri) {
            const Run &run = runs[ri];
            cov.by_len[run.n < 6 ? run.n : 6] += 1;
            if (ri + 1 == runs.size()) cov.tail_run += 1;
            for (uint32_t st = 0; st <= run.n; ++st) {   // every start, the sentinel's included
                const uint32_t start = run.first + st;
                // above everything, far to the side: no hit, every entry tested to the sentinel
                one_walk(pts, run, start, base + 5.0f, base + 5.0f, base + 9.0f, r2, rexit);
                // below everything: the exit at the first test
                one_walk(pts, run, start, base + 0.1f, base + 0.1f, base - 9.0f, r2, rexit);
                for (uint32_t e = st; e < run.n; ++e) {
                    const float *f = pts + 3 * (size_t)(run.first + e);
                    // on entry e (a hit there unless an earlier entry is within r or r below)
                    one_walk(pts, run, start, f[0] + 0.01f * U(rng), f[1], f[2] + 0.01f, r2,
                             rexit);
                    // at its edge: within r or not by the last bits
                    one_walk(pts, run, start, f[0] + r * 0.7071f, f[1] + r * 0.7071f, f[2], r2,
                             rexit);
                    // far to the side at heights about rexit above e: the exit at or near e
                    one_walk(pts, run, start, f[0] + 0.5f, f[1], f[2] + rexit, r2, rexit);
                    one_walk(pts, run, start, f[0] + 0.5f, f[1],
                             std::nextafter(f[2] + rexit, -inf), r2, rexit);
                    one_walk(pts, run, start, f[0] + 0.5f, f[1], f[2] + 1.5f * rexit, r2, rexit);
                }
                for (int q = 0; q < 4; ++q)   // anywhere
                    one_walk(pts, run, start, base + 0.3f * U(rng) - 0.05f,
                             base + 0.3f * U(rng) - 0.05f, base + 2.2f * U(rng) - 0.1f, r2, rexit);
            }
        }
        std::free(pts);
    }
    CHECK(cov.hit[0] > 0 && cov.hit[1] > 0);
    CHECK(cov.exit_[0] > 0 && cov.exit_[1] > 0);
    CHECK(cov.sentinel[0] > 0 && cov.sentinel[1] > 0);
    CHECK(cov.start_parity[0] > 0 && cov.start_parity[1] > 0);
    CHECK(cov.start_on_sentinel > 0 && cov.tail_run == 60);
    for (int l = 0; l < 7; ++l) CHECK(cov.by_len[l] > 0);
    std::printf("%ld walks: hits %ld / %ld, exits %ld / %ld, sentinel %ld / %ld by slot; "
                "%ld started on a sentinel\n",
                cov.walks, cov.hit[0], cov.hit[1], cov.exit_[0], cov.exit_[1], cov.sentinel[0],
                cov.sentinel[1], cov.start_on_sentinel);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
