// The context's runtime knobs: every environment variable pcp_create reads, once, in one table.
// Plain host C++ (no HIP dependency): pcp_create calls knobs_from_env() over the process
// environment, tests/native/knobs_selftest.cpp checks every rule over a fake one, and
// INTEGRATION.md ("Runtime variables") lists the same names with their meaning.
// A row is a name, a field and a rule.  Most rules are a flag (atoi(v) != 0), an inverted flag
// (atoi(v) == 0) or a plain atoi, so a value that is set but empty parses as 0; the odd rows carry
// a setter of their own, and one of them (PCP_SCORE_WIDE_G) can refuse a value.  An unset
// variable leaves the field's initializer, the default.  knobs_from_env walks the rows in table
// order and stops at the first refused value: the rows before it hold their parsed values, the
// refused row and the rows after it their defaults.
// Not here: PCP_ALLOC_TRACE (process-wide: note_realloc has no context), the CLI's own variables
// (host/pcp_nodes_cli.cpp) and every -D build knob.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "pcp_fan_clip.hpp"

namespace pcp {

struct Knobs {
    // fan query (pcp_fan.hip, pcp_march.hpp)
    int fan_batch = 0;               // fan kernel variant, A/B only (fan_pick())
    int fan_npw = 8;                 // poses per wave of the production fan kernel
    bool fan_cull = true;            // only the rings that can reach the terrain are launched
    bool fan_clear = true;           // the march jumps by the empty records' clearance codes
    bool fan_pivot = true;           // the fan march tests a window's pivot before its walk
    bool fan_band = true;            // the march's probe reads the thresholds' tight twin
    float fan_clip_e = kClipSlack;   // the clip interval's slack each side, in samples
    bool fan_horizon_first = true;   // the live rings nearest the horizon first (0: ring order)
    bool fan_host_out = true;        // k_fan_reduce stores into the pinned landing block
    // cell scoring (pcp_score.hip)
    bool score_wide = true;          // k_score_cells_wide for few-ray launches
    int64_t score_wide_rays = -1;    // rays up to which it runs (-1: the built-in bound)
    int score_wide_g = 0;            // its lanes per ray, 2 / 4 / 8 / 16 (0: the built-in choice)
    // excavation area (pcp_excav.hip)
    bool normals_exact = true;       // the reference's summation order (0: order-free, A/B only)
    bool cells_all_ordered = false;  // every cell through the sorted lists
    int nb_blocks = 0;               // k_nb_lists grid (0: kNbBlocks)
    bool nb_small = true;            // 16-bit list keys below 2^16 points (0: 32-bit there too)
    int nb_region_pct = 75;          // list words in the blocks' regions (rest: spill pool)
    uint64_t nb_guess_max = 64ull << 20;   // cap of a first list buffer, words
    bool area_side = true;           // the async setup's normals + lattice on a side stream
    bool index_pair = true;          // the area's two grids from one pass (0: two builds)
    // scans, copies and staging (pcp_context.hip, pcp_hostcopy.hip, pcp_index.hip)
    bool scan_onepass = true;        // exclusive_scan_u32's one-pass look-back form
    bool scan_pair = true;           // a grid pair's two one-tile scans in one launch
    bool copy_kernel = true;         // pinned <-> device copies by a copy kernel (0: DMA)
    bool zc_in = true;               // message-sized inputs read in place from pinned memory
    int copy_threads = 3;            // helper threads of a large host copy (0: plain memcpy)
    bool host_bbox_scalar = false;   // the host bounding box by the scalar loop (A/B)
    // filter chain (pcp_filter.hip, filter_plan())
    int fm_fast = 2;                 // the voxel chain: 2 bucket, 1 LSD fast, 0 the general one
    bool fm_host_out = true;         // filter_merge's result sizes stored into pinned memory
    int bk_gt = 0;                   // crop tiles per k_bk_group group (0: one round of blocks)
    int bk_pts = 512;                // input points per bucket at least (0: by voxel count only)
    bool use_graphs = true;          // the device-resident filter_merge replayed as a graph
    // carve (pcp_carve.hip) and terrain copies (pcp_index.hip, pcp_fine.hip)
    bool carve_fuse_copy = true;     // the composed carve's records copied by its index's build
    int terrain_blocks = 1;          // the terrain copy: 0 never, 1 at the second query, 2 first
    int terrain_fine = 2;            // its fine-window layout, cells of c / F (0: the 2x2x2 blocks)
    int fine_tile = 2;               // fine records: 0 x-fastest, 1 4 x 4 tiles, 2 split, 8 x 8
    int fine_skip = 2;               // the split records' skip thresholds: 1 or 2
    bool fine_pack = true;           // fine-window entries as 12 bytes
};

// A row's rule.  Flag / NotFlag set the bool field, Int the int field, Odd calls its setter; a
// Strict setter may refuse the value: it returns null, or what is wrong with it ("is not ...").
struct KnobRow {
    enum Kind { Flag, NotFlag, Int, Odd, Strict };
    const char *name;
    Kind kind;
    bool Knobs::*b = nullptr;
    int Knobs::*i = nullptr;
    void (*odd)(Knobs &, const char *) = nullptr;
    const char *(*strict)(Knobs &, const char *) = nullptr;
};

inline const std::vector<KnobRow> &knob_rows() {   // the table
    using K = Knobs;
    using R = KnobRow;
    constexpr auto flag = [](const char *s, bool K::*f) { return R{s, R::Flag, f}; };
    constexpr auto inv = [](const char *s, bool K::*f) { return R{s, R::NotFlag, f}; };
    constexpr auto num = [](const char *s, int K::*f) { return R{s, R::Int, nullptr, f}; };
    constexpr auto odd = [](const char *s, void (*f)(K &, const char *)) {
        return R{s, R::Odd, nullptr, nullptr, f};
    };
    static const std::vector<KnobRow> rows = {
        num("PCP_FAN_BATCH", &K::fan_batch),
        odd("PCP_FAN_NPW", [](K &k, const char *v) {   // the instantiated widths, else 1
            const int w = std::atoi(v);
            k.fan_npw = (w == 2 || w == 4 || w == 8 || w == 16 || w == 32) ? w : 1;
        }),
        flag("PCP_FAN_CULL", &K::fan_cull),
        flag("PCP_FAN_CLEAR", &K::fan_clear),
        flag("PCP_FAN_PIVOT", &K::fan_pivot),
        flag("PCP_FAN_BAND", &K::fan_band),
        odd("PCP_FAN_CLIP", [](K &k, const char *v) {
            k.fan_clip_e = std::atoi(v) != 0 ? kClipSlack : kClipSlackWhole;
        }),
        flag("PCP_FAN_ORDER", &K::fan_horizon_first),
        flag("PCP_FAN_HOST_OUT", &K::fan_host_out),
        flag("PCP_NORMALS_EXACT", &K::normals_exact),
        flag("PCP_SCORE_WIDE", &K::score_wide),
        odd("PCP_SCORE_WIDE_RAYS", [](K &k, const char *v) { k.score_wide_rays = std::atoll(v); }),
        // the instantiated widths only, the whole string: no silent fall-back to the default
        R{"PCP_SCORE_WIDE_G", R::Strict, nullptr, nullptr, nullptr,
          [](K &k, const char *v) -> const char * {
              char *end = nullptr;
              const long g = std::strtol(v, &end, 10);
              if (end == v || *end != '\0' || !(g == 2 || g == 4 || g == 8 || g == 16))
                  return "is not one of 2, 4, 8, 16";
              k.score_wide_g = (int)g;
              return nullptr;
          }},
        inv("PCP_CELLS_ORDER_FREE", &K::cells_all_ordered),
        num("PCP_NB_BLOCKS", &K::nb_blocks),
        flag("PCP_SCAN_ONEPASS", &K::scan_onepass),
        flag("PCP_INDEX_PAIR", &K::index_pair),
        flag("PCP_AREA_STREAM", &K::area_side),
        flag("PCP_NB_SMALL", &K::nb_small),
        odd("PCP_NB_REGION_PCT", [](K &k, const char *v) {
            k.nb_region_pct = std::min(100, std::max(1, std::atoi(v)));
        }),
        odd("PCP_NB_GUESS_WORDS", [](K &k, const char *v) {
            k.nb_guess_max = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
        }),
        num("PCP_COPY_THREADS", &K::copy_threads),
        flag("PCP_FM_HOST_OUT", &K::fm_host_out),
        odd("PCP_FM_FAST", [](K &k, const char *v) {   // an unknown value is the default
            const int f = std::atoi(v);
            k.fm_fast = (f == 0 || f == 1) ? f : 2;
        }),
        num("PCP_BK_GT", &K::bk_gt),
        flag("PCP_SCAN_PAIR", &K::scan_pair),
        flag("PCP_CARVE_FUSE_COPY", &K::carve_fuse_copy),
        num("PCP_BK_PTS", &K::bk_pts),
        flag("PCP_ZC_IN", &K::zc_in),
        flag("PCP_COPY_KERNEL", &K::copy_kernel),
        num("PCP_TERRAIN_BLOCKS", &K::terrain_blocks),
        num("PCP_TERRAIN_FINE", &K::terrain_fine),
        num("PCP_FINE_TILE", &K::fine_tile),
        odd("PCP_FINE_SKIP", [](K &k, const char *v) { k.fine_skip = std::atoi(v) == 2 ? 2 : 1; }),
        flag("PCP_FINE_PACK", &K::fine_pack),
        inv("PCP_NO_GRAPHS", &K::use_graphs),
        // presence alone
        odd("PCP_HOST_BBOX_SCALAR", [](K &k, const char *) { k.host_bbox_scalar = true; }),
    };
    return rows;
}

// Fill k from the environment `get` answers for (null: the variable is unset).
// 0, or -1 with *err = `NAME="value" is not ...` (see the top comment for what k then holds).
inline int knobs_from_env(Knobs &k, const char *(*get)(const char *), std::string *err) {
    for (const KnobRow &r : knob_rows()) {
        const char *v = get(r.name);
        if (!v) continue;
        const char *bad = nullptr;
        switch (r.kind) {
        case KnobRow::Flag: k.*r.b = std::atoi(v) != 0; break;
        case KnobRow::NotFlag: k.*r.b = std::atoi(v) == 0; break;
        case KnobRow::Int: k.*r.i = std::atoi(v); break;
        case KnobRow::Odd: r.odd(k, v); break;
        case KnobRow::Strict: bad = r.strict(k, v); break;
        }
        if (bad) {
            if (err) *err = std::string(r.name) + "=\"" + v + "\" " + bad;
            return -1;
        }
    }
    return 0;
}

}  // namespace pcp
