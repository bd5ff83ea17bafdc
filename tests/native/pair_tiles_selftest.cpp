// pcp_pair_tiles.hpp on the host: the block <-> tile mapping is a bijection onto the upper
// triangle, and every pair a < b < n has exactly one (block, lane, slot), every single one, and
// nothing past n any.  Stand-alone: prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../../include/pcp_abi.h"
#include "pcp_pair_tiles.hpp"

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
    const int nb = pair_blocks(nt);
    CHECK(nb == nt * (nt + 1) / 2, "nt %d: %d blocks", nt, nb);
    std::vector<int> seen((size_t)nt * nt, 0);
    int prev_a = 0, prev_b = -1;
    for (int k = 0; k < nb; ++k) {
        const PairTile t = pair_tile_of(nt, k);
        CHECK(t.ta >= 0 && t.ta <= t.tb && t.tb < nt, "nt %d block %d -> (%d, %d)", nt, k, t.ta,
              t.tb);
        if (!(t.ta >= 0 && t.ta <= t.tb && t.tb < nt)) return;
        CHECK(pair_block_of(nt, t.ta, t.tb) == k, "nt %d block %d: not its own inverse", nt, k);
        // row-major order: the blocks' bests combine with ties to the smaller (a, b)
        CHECK(t.ta > prev_a || (t.ta == prev_a && t.tb > prev_b), "nt %d block %d: order", nt, k);
        prev_a = t.ta;
        prev_b = t.tb;
        ++seen[(size_t)t.ta * nt + t.tb];
    }
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b)
            CHECK(seen[(size_t)a * nt + b] == (a <= b ? 1 : 0), "nt %d tile (%d, %d): %d blocks", nt,
                  a, b, seen[(size_t)a * nt + b]);
}

static void check_ownership(int n) {
    const int nt = pair_tiles(n), nb = pair_blocks(nt);
    CHECK(nt * kPairTile >= n && (nt - 1) * kPairTile < n, "n %d: %d tiles", n, nt);
    std::vector<int> pairs((size_t)n * n, 0), singles((size_t)n, 0);
    for (int k = 0; k < nb; ++k) {
        const PairTile t = pair_tile_of(nt, k);
        for (int lane = 0; lane < kPairLanes; ++lane)
            for (int slot = 0; slot < kPairSlots; ++slot) {
                const PairSlot s = pair_slot(t.ta, t.tb, lane, slot);
                CHECK(s.a >= 0 && s.b >= 0 && s.a < nt * kPairTile && s.b < nt * kPairTile,
                      "n %d: slot out of the padded range", n);
                const bool p = pair_is_pair(s, n), g = pair_is_single(s, n);
                CHECK(!(p && g), "n %d: (%d, %d) both", n, s.a, s.b);
                if (p || g) CHECK(s.a < n && s.b < n, "n %d: (%d, %d) past n owned", n, s.a, s.b);
                if (p) ++pairs[(size_t)s.a * n + s.b];
                if (g) {
                    CHECK(t.ta == t.tb, "n %d: single %d off the diagonal tiles", n, s.a);
                    ++singles[(size_t)s.a];
                }
            }
    }
    for (int a = 0; a < n; ++a) {
        CHECK(singles[(size_t)a] == 1, "n %d: single %d owned %d times", n, a, singles[(size_t)a]);
        for (int b = 0; b < n; ++b)
            CHECK(pairs[(size_t)a * n + b] == (a < b ? 1 : 0), "n %d: pair (%d, %d) owned %d times",
                  n, a, b, pairs[(size_t)a * n + b]);
    }
}

int main() {
    static_assert(kPairLanes == kPairSide * kPairSide && kPairSub * kPairSide == kPairTile &&
                      kPairSlots == kPairSub * kPairSub,
                  "the lanes' register tiles cover the tile pair");
    for (int nt = 1; nt <= 64; ++nt) check_mapping(nt);
    check_mapping(pair_tiles(PCP_PAIR_MAX_POSES));
    CHECK(pair_tiles(PCP_PAIR_MAX_POSES) * kPairTile == PCP_PAIR_MAX_POSES, "the cap is whole tiles");
    for (int n = 1; n <= 3 * kPairTile + 1; ++n) check_ownership(n);
    CHECK(pair_tiles(0) == 0 && pair_blocks(0) == 0, "no poses, no blocks");
    if (fails)
        std::printf("FAILED (%d)\n", fails);
    else
        std::printf("ok\n");
    return fails ? 1 : 0;
}
