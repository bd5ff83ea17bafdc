// The pair search's tile arithmetic (pcp_place_pair, pcp_pairs.hip).  Plain C++
// (no HIP dependency): the kernels and tests/native/pair_tiles_selftest.cpp share it.
//
// The poses are cut into tiles of kPairTile; a block owns one tile pair (ta <= tb) of the upper
// triangle, numbered row-major: (0,0), (0,1) .. (0,nt-1), (1,1), (1,2) ..  Lane l of the block
// holds the kPairSub x kPairSub register tile of pairs (a, b) with
//   a = ta kPairTile + kPairSub (l / kPairSide) + u,   b = tb kPairTile + kPairSub (l % kPairSide) + v,
// slot = u kPairSub + v.  A slot is a pair of the search when a < b < n; the slots with a == b of
// a diagonal tile are the singles.  (kPairSub = 1: one pair, one f64 chain per lane, the tile
// pair's 256 chains on the four SIMDs of its CU: 2 x 2 pairs per lane on one wave per tile pair
// ran the tick's tiles in 132 us, this runs them in 50 us)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCP_PT_HD __host__ __device__
#else
#define PCP_PT_HD
#endif

namespace pcp {

constexpr int kPairTile = 16;                     // poses per tile edge
constexpr int kPairSub = 1;                       // a lane's register tile is kPairSub x kPairSub
constexpr int kPairSide = kPairTile / kPairSub;   // lanes per tile edge
constexpr int kPairLanes = kPairSide * kPairSide; // threads per block: four waves
constexpr int kPairSlots = kPairSub * kPairSub;
static_assert(kPairLanes % 64 == 0 && kPairLanes <= 1024, "a tile pair is whole waves of a block");

PCP_PT_HD inline int pair_tiles(int n) { return (n + kPairTile - 1) / kPairTile; }
PCP_PT_HD inline int pair_blocks(int nt) { return nt * (nt + 1) / 2; }
// the first block of tile row ta
PCP_PT_HD inline int pair_row_start(int nt, int ta) { return ta * nt - ta * (ta - 1) / 2; }
PCP_PT_HD inline int pair_block_of(int nt, int ta, int tb) {
    return pair_row_start(nt, ta) + (tb - ta);
}

struct PairTile { int ta, tb; };
// the inverse of pair_block_of: an estimate of the row, then exact integer steps
PCP_PT_HD inline PairTile pair_tile_of(int nt, int block) {
    // rows are nt, nt - 1, .. long: ta = the largest row whose start is <= block
    int ta = (int)((double)block / (double)(nt > 0 ? nt : 1));
    if (ta > nt - 1) ta = nt - 1;
    if (ta < 0) ta = 0;
    while (ta + 1 < nt && pair_row_start(nt, ta + 1) <= block) ++ta;
    while (ta > 0 && pair_row_start(nt, ta) > block) --ta;
    return PairTile{ta, ta + (block - pair_row_start(nt, ta))};
}

struct PairSlot { int a, b; };
PCP_PT_HD inline PairSlot pair_slot(int ta, int tb, int lane, int slot) {
    return PairSlot{ta * kPairTile + kPairSub * (lane / kPairSide) + slot / kPairSub,
                    tb * kPairTile + kPairSub * (lane % kPairSide) + slot % kPairSub};
}
PCP_PT_HD inline bool pair_is_pair(PairSlot s, int n) { return s.a < s.b && s.b < n; }
PCP_PT_HD inline bool pair_is_single(PairSlot s, int n) { return s.a == s.b && s.a < n; }

}  // namespace pcp
