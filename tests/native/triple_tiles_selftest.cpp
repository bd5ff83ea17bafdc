// pcp_triple_tiles.hpp on the host: the index <-> tile triple mapping is a bijection onto
// ta <= tb <= tc with every ta's tile triples one contiguous range in tile-pair order, and every
// triple a < b < c < n has exactly one (block, lane, slot), nothing else any.  Stand-alone: prints
// "ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../../include/pcp_abi.h"
#include "pcp_triple_tiles.hpp"

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

static void check_mapping(int nt) {
    const int nb = triple_tile_count(nt);
    long want = 0;
    for (int a = 0; a < nt; ++a)
        for (int b = a; b < nt; ++b) want += nt - b;
    CHECK(nb == want, "nt %d: %d tile triples, %ld expected", nt, nb, want);
    CHECK(triple_blocks(nt) == nb * kTripleSub, "nt %d: blocks", nt);
    std::vector<int> seen((size_t)nt * nt * nt, 0);
    TripleTile prev{0, 0, -1};
    for (int k = 0; k < nb; ++k) {
        const TripleTile t = triple_tile_of(nt, k);
        const bool in = t.ta >= 0 && t.ta <= t.tb && t.tb <= t.tc && t.tc < nt;
        CHECK(in, "nt %d index %d -> (%d, %d, %d)", nt, k, t.ta, t.tb, t.tc);
        if (!in) return;
        CHECK(triple_index_of(nt, t.ta, t.tb, t.tc) == k, "nt %d index %d: not its own inverse", nt,
              k);
        // lexicographic order: a ta's range is contiguous, and k_triple_rows walks it
        const bool after = t.ta > prev.ta || (t.ta == prev.ta && t.tb > prev.tb) ||
                           (t.ta == prev.ta && t.tb == prev.tb && t.tc > prev.tc);
        CHECK(after, "nt %d index %d: order", nt, k);
        CHECK(k >= triple_row_start(nt, t.ta) &&
                  k < triple_row_start(nt, t.ta) + triple_row_count(nt, t.ta),
              "nt %d index %d: outside its ta's range", nt, k);
        prev = t;
        ++seen[((size_t)t.ta * nt + t.tb) * nt + t.tc];
    }
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b)
            for (int c = 0; c < nt; ++c)
                CHECK(seen[((size_t)a * nt + b) * nt + c] == (a <= b && b <= c ? 1 : 0),
                      "nt %d tile (%d, %d, %d): %d times", nt, a, b, c,
                      seen[((size_t)a * nt + b) * nt + c]);
    int total = 0;
    for (int a = 0; a < nt; ++a) {
        CHECK(triple_row_start(nt, a) == total, "nt %d: ta %d starts at %d, not %d", nt, a,
              triple_row_start(nt, a), total);
        total += triple_row_count(nt, a);
    }
    CHECK(total == nb, "nt %d: the ranges sum to %d", nt, total);
}

static void check_ownership(int n) {
    const int nt = triple_tiles(n), nb = triple_blocks(nt);
    CHECK(nt * kTripleTile >= n && (nt - 1) * kTripleTile < n, "n %d: %d tiles", n, nt);
    std::vector<unsigned char> owned((size_t)n * n * n, 0);
    long count = 0;
    for (int k = 0; k < nb; ++k) {
        const TripleTile t = triple_tile_of(nt, k / kTripleSub);
        const int sub = k % kTripleSub;
        for (int lane = 0; lane < kTripleLanes; ++lane)
            for (int slot = 0; slot < kTripleA; ++slot) {
                const TripleSlot s = triple_slot(t, sub, lane, slot);
                const int pad = nt * kTripleTile;
                CHECK(s.a >= 0 && s.b >= 0 && s.c >= 0 && s.a < pad && s.b < pad && s.c < pad,
                      "n %d: slot out of the padded range", n);
                // the row of k_triple_rows that reads this block's slot
                CHECK(s.a / kTripleTile == t.ta && s.a % kTripleTile / kTripleA == sub &&
                          s.a % kTripleA == slot,
                      "n %d: pose %d is not slot %d of block %d", n, s.a, slot, k);
                if (!triple_is_triple(s, n)) continue;
                CHECK(s.a < s.b && s.b < s.c && s.c < n, "n %d: (%d, %d, %d) owned", n, s.a, s.b,
                      s.c);
                if (!(s.a < s.b && s.b < s.c && s.c < n)) continue;
                unsigned char &o = owned[((size_t)s.a * n + s.b) * n + s.c];
                CHECK(o == 0, "n %d: (%d, %d, %d) owned twice", n, s.a, s.b, s.c);
                o = 1;
                ++count;
            }
    }
    CHECK(count == (long)n * (n - 1) * (n - 2) / 6, "n %d: %ld triples owned", n, count);
}

int main() {
    static_assert(kTripleTile == kPairTile && kTripleLanes == kTripleTile * kTripleTile &&
                      kTripleSub * kTripleA == kTripleTile,
                  "the lanes cover the B x C tile, the blocks' groups the A tile");
    for (int nt = 1; nt <= 32; ++nt) check_mapping(nt);
    CHECK(triple_tiles(PCP_TRIPLE_MAX_POSES) == 32 &&
              triple_tiles(PCP_TRIPLE_MAX_POSES) * kTripleTile == PCP_TRIPLE_MAX_POSES,
          "the cap is 32 whole tiles");
    CHECK(PCP_TRIPLE_TABLE_MAX_POSES <= PCP_TRIPLE_MAX_POSES && PCP_TRIPLE_MAX_POSES <= PCP_PAIR_MAX_POSES,
          "the limits nest");
    const int T = kTripleTile;
    const int ns[] = {1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1, 91, PCP_TRIPLE_MAX_POSES};
    for (int n : ns) check_ownership(n);
    CHECK(triple_tiles(0) == 0 && triple_blocks(0) == 0, "no poses, no blocks");
    if (fails)
        std::printf("FAILED (%d)\n", fails);
    else
        std::printf("ok\n");
    return fails ? 1 : 0;
}
