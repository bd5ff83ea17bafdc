// The triple search's tile arithmetic (pcp_place_triple, pcp_triples.hip).  Plain
// C++ (no HIP dependency): the kernels and tests/native/triple_tiles_selftest.cpp share it.
//
// The poses are cut into the pair search's tiles (kTripleTile = kPairTile).  A tile triple
// ta <= tb <= tc is numbered ta-major, and within one ta as the tile pair (tb - ta, tc - ta) of the
// nt - ta tiles from ta on (pcp_pair_tiles.hpp's row-major numbering), so the tile triples of one
// ta are one contiguous range.  A tile triple is split over kTripleSub blocks, block =
// index kTripleSub + sub: block sub runs the kTripleA poses a = ta kTripleTile + sub kTripleA + slot
// of the A tile, one f64 chain per slot in every lane, and lane l owns
//   b = tb kTripleTile + l / kTripleTile,   c = tc kTripleTile + l % kTripleTile.
// (slot, lane) is a triple of the search when a < b < c < n.  (kTripleA = 4: four blocks per tile
// triple fill the device at the tick's 91 poses, where 8 and 16 chains per lane leave CUs idle;
// DESIGN.md §6k has the measurement against 2, 8 and 16.)
#pragma once

#include <cstdint>

#include "pcp_pair_tiles.hpp"

namespace pcp {

#ifndef PCP_TRIPLE_TA
#define PCP_TRIPLE_TA 4
#endif

constexpr int kTripleTile = kPairTile;                      // poses per tile edge
constexpr int kTripleA = PCP_TRIPLE_TA;                     // chains per lane: poses a of a block
constexpr int kTripleSub = kTripleTile / kTripleA;          // blocks per tile triple
constexpr int kTripleLanes = kTripleTile * kTripleTile;     // threads per block: four waves
static_assert(kTripleA >= 1 && kTripleSub * kTripleA == kTripleTile, "whole A groups per tile");
static_assert(kTripleLanes % 64 == 0 && kTripleLanes <= 1024, "whole waves of a block");

PCP_PT_HD inline int triple_tiles(int n) { return pair_tiles(n); }
// tile triples ta <= tb <= tc of nt tiles
PCP_PT_HD inline int triple_tile_count(int nt) { return nt * (nt + 1) * (nt + 2) / 6; }
PCP_PT_HD inline int triple_blocks(int nt) { return triple_tile_count(nt) * kTripleSub; }
// the first tile triple of ta: those before it are all but the ones within the tiles ta ..
PCP_PT_HD inline int triple_row_start(int nt, int ta) {
    return triple_tile_count(nt) - triple_tile_count(nt - ta);
}
// the tile triples of one ta: the tile pairs of the nt - ta tiles from ta on
PCP_PT_HD inline int triple_row_count(int nt, int ta) { return pair_blocks(nt - ta); }
PCP_PT_HD inline int triple_index_of(int nt, int ta, int tb, int tc) {
    return triple_row_start(nt, ta) + pair_block_of(nt - ta, tb - ta, tc - ta);
}

struct TripleTile { int ta, tb, tc; };
// the inverse of triple_index_of: the last ta whose range starts at or before index (at most 32
// exact integer steps), then the tile pair within it
PCP_PT_HD inline TripleTile triple_tile_of(int nt, int index) {
    int ta = 0;
    while (ta + 1 < nt && triple_row_start(nt, ta + 1) <= index) ++ta;
    const PairTile p = pair_tile_of(nt - ta, index - triple_row_start(nt, ta));
    return TripleTile{ta, ta + p.ta, ta + p.tb};
}

struct TripleSlot { int a, b, c; };
PCP_PT_HD inline TripleSlot triple_slot(TripleTile t, int sub, int lane, int slot) {
    return TripleSlot{t.ta * kTripleTile + sub * kTripleA + slot,
                      t.tb * kTripleTile + lane / kTripleTile,
                      t.tc * kTripleTile + lane % kTripleTile};
}
PCP_PT_HD inline bool triple_is_triple(TripleSlot s, int n) {
    return s.a < s.b && s.b < s.c && s.c < n;
}

}  // namespace pcp
