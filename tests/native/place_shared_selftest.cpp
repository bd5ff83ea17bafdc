// The plain C++ part of pcp_place_shared.hpp on the host: the first-maximum order, the index
// list check and the front of the placement calls' blocks.  Stand-alone: prints "ok" and returns
// 0, or says what failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/pcp_abi.h"
#include "pcp_place_shared.hpp"

using namespace pcp;

static int fails = 0;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            ++fails;                  \
        }                             \
    } while (0)

// folding best_ahead over any order of the candidates gives the first maximum in row-major order
static void check_best_ahead() {
    const double inf = INFINITY;
    // equal totals, -inf totals and empty candidates (a < 0), one of them with the largest total
    const std::vector<RowBest> cand = {{3.5, 2, 7},  {3.5, 2, 4},   {3.5, 1, 9}, {-inf, 0, 0},
                                       {inf, -1, -1}, {-inf, -1, 3}, {1.25, 0, 1}};
    auto brute = [](const std::vector<RowBest> &v) {
        RowBest w{-INFINITY, -1, -1};
        for (const RowBest &c : v) {
            if (c.a < 0) continue;
            const bool first = w.a < 0;
            const bool earlier = c.a < w.a || (c.a == w.a && c.b < w.b);
            if (first || c.t > w.t || (c.t == w.t && earlier)) w = c;
        }
        return w;
    };
    // every subset (the empty ones alone, a real -inf against the empty +inf, ..), every order
    for (unsigned mask = 1; mask < (1u << cand.size()); ++mask) {
        std::vector<RowBest> v;
        std::vector<int> order;
        for (size_t i = 0; i < cand.size(); ++i)
            if (mask >> i & 1u) {
                order.push_back((int)v.size());
                v.push_back(cand[i]);
            }
        const RowBest want = brute(v);
        do {
            RowBest w = v[(size_t)order[0]];
            for (size_t i = 1; i < order.size(); ++i) {
                const RowBest &c = v[(size_t)order[i]];
                if (best_ahead(c.t, c.a, c.b, w.t, w.a, w.b)) w = c;
            }
            if (want.a < 0)
                CHECK(w.a < 0, "mask %u: an empty candidate list gave (%d, %d)", mask, w.a, w.b);
            else
                CHECK(w.a == want.a && w.b == want.b && w.t == want.t,
                      "mask %u: (%g, %d, %d), first maximum (%g, %d, %d)", mask, w.t, w.a, w.b,
                      want.t, want.a, want.b);
        } while (std::next_permutation(order.begin(), order.end()));
    }
    CHECK(!best_ahead(inf, -1, 0, -inf, 5, 5), "an empty candidate beat a real one at -inf");
    CHECK(best_ahead(-inf, 5, 5, inf, -1, 0), "a real candidate at -inf lost to an empty one");
    CHECK(!best_ahead(1.0, 3, 3, 1.0, 3, 3), "a candidate is ahead of itself");
}

static void check_index_lists() {
    int bad = -1;
    const int64_t good[] = {4, 0, 9, 2};
    CHECK(check_index_list(good, 4, 10, &bad) == kListOk, "a valid list refused");
    CHECK(check_index_list(good, 0, 10, &bad) == kListOk, "an empty list refused");
    CHECK(check_index_list(nullptr, 0, 0, &bad) == kListOk, "no list of no poses refused");
    const int64_t neg[] = {4, -1, 4};
    CHECK(check_index_list(neg, 3, 10, &bad) == kListRange && bad == 1, "negative: entry %d", bad);
    const int64_t edge[] = {4, 0, 10};
    CHECK(check_index_list(edge, 3, 10, &bad) == kListRange && bad == 2, "index == n: entry %d", bad);
    CHECK(check_index_list(edge, 3, 11, &bad) == kListOk, "index == n - 1 refused");
    const int64_t dup[] = {4, 0, 9, 0, 4};
    CHECK(check_index_list(dup, 5, 10, &bad) == kListTwice && bad == 3, "duplicate: entry %d", bad);
    CHECK(check_index_list(dup, 3, 10, &bad) == kListOk, "the list before its duplicate refused");
}

// the states' sizes as pcp_pairs.hip (64), pcp_place.hip and pcp_refine.hip declare them
struct PlaceStateSize {
    int32_t n_sel, done;
    uint32_t ticket;
    int32_t zx_cov;
    double T, zx_total;
    int64_t sel[PCP_PLACE_MAX];
    double total_after[PCP_PLACE_MAX];
    int32_t cov_after[PCP_PLACE_MAX];
};
struct RefineStateSize {
    int32_t n_moves, done, converged, start_cov;
    uint32_t ticket;
    int32_t pad[3];
    double T, start_total;
    int32_t set[PCP_PLACE_MAX];
    int32_t move_slot[PCP_REFINE_MAX_MOVES], move_from[PCP_REFINE_MAX_MOVES];
    int32_t move_to[PCP_REFINE_MAX_MOVES], move_cov[PCP_REFINE_MAX_MOVES];
    double move_total[PCP_REFINE_MAX_MOVES];
};

static void check_layout() {
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t states[] = {64, sizeof(PlaceStateSize), sizeof(RefineStateSize)};
    for (size_t st : states)
        for (int C : {1, 63, 64, 65}) {
            const CellBlock b = cell_block(st, C);
            CHECK(st % 16 == 0, "state of %zu bytes", st);
            CHECK(b.score_off % 16 == 0 && b.owner_off % 16 == 0 && b.rest_off % 16 == 0,
                  "state %zu C %d: alignment", st, C);
            CHECK(b.score_off >= st && b.owner_off >= b.score_off + (size_t)C * sizeof(double) &&
                      b.rest_off >= b.owner_off + (size_t)C * sizeof(int32_t),
                  "state %zu C %d: the parts overlap", st, C);
            // the plans of the three calls before they shared this: base_off / own_off / rt_off,
            // cs_off / own_off / sg_off, cs_off / own_off / tab_off -- one formula
            const size_t cs_off = st;
            const size_t own_off = up(cs_off + (size_t)C * sizeof(double));
            const size_t next_off = up(own_off + (size_t)C * sizeof(int32_t));
            CHECK(b.score_off == cs_off && b.owner_off == own_off && b.rest_off == next_off,
                  "state %zu C %d: (%zu, %zu, %zu), the plans' (%zu, %zu, %zu)", st, C, b.score_off,
                  b.owner_off, b.rest_off, cs_off, own_off, next_off);
        }
    CHECK(a16(0) == 0 && a16(1) == 16 && a16(16) == 16 && a16(17) == 32, "a16");
    CHECK(sep2_of(0.0) == 0.0 && sep2_of(-2.0) == 0.0 && sep2_of(1.5) == 2.25, "sep2_of");
}

int main() {
    check_best_ahead();
    check_index_lists();
    check_layout();
    if (fails)
        std::printf("FAILED (%d)\n", fails);
    else
        std::printf("ok\n");
    return fails ? 1 : 0;
}
