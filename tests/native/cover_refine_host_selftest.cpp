// cover_refine_host_selftest.cpp -- what CoveragePlacement::refine / refine_mounted
// (pcp_cover_node.hpp) hand to the C ABI and make of its answers, on the CPU.  Linked from
// pcp_cover_node.cpp, pcp_cover_refine_node.cpp, pcp_nodes.cpp, the shell tests' mock_pcp.cpp and
// the two pcp_place_coverage_refine entry points below, which record what they were given and
// return the answers a case has set.  The program checks the marshalling, the rounds made of the
// slots, the moves, the blind-spot records, the log text and the refusal paths itself and ends with
// status 0 and "cover_refine_host_selftest ok" only if every check held.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcp_cover_node.hpp"

using namespace pcp;
using Opt = SimplifiedDualLidarOptimizer;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

// ---- the canned answer and the call record ---------------------------------------------------
struct CannedMove {
    int32_t slot;
    int64_t from, to;
    uint64_t covered;
};
struct Canned {
    int rc = PCP_OK;
    std::vector<int64_t> selected;
    uint64_t covered = 0, start_covered = 0, n_points = 0, roi_points = 0;
    std::vector<CannedMove> moves;
    int32_t converged = 1;
    std::vector<uint64_t> uniq;
    std::vector<int32_t> owner;
    std::vector<uint32_t> seen;
};
struct Seen {
    int calls = 0;
    bool mounted = false, ctx_ok = false;
    std::vector<double> poses, el_table;
    bool el_null = true, roi_null = true, tab_null = true, uniq_null = true, seen_null = true,
         owner_null = true, moves_null = true;
    uint64_t n = 0, roi_n = 0, owner_cap = 0;
    pcp_fan_params fan{};
    pcp_refine_params rp{};
    std::vector<uint8_t> roi;
};
static Canned g;
static Seen s;
static pcp_ctx *g_ctx = nullptr;

static int record(bool mounted, pcp_ctx *ctx, const double *poses, uint64_t n,
                  const pcp_fan_params *fan, const double *el_table, const pcp_refine_params *rp,
                  const uint8_t *roi, uint64_t roi_n, int64_t *selected, uint64_t *covered,
                  uint64_t *start_covered, int32_t *move_slot, int64_t *move_from,
                  int64_t *move_to, uint64_t *move_covered, int64_t *swap_covered,
                  uint64_t *slot_unique, uint32_t *seen_points, int32_t *point_owner,
                  uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points, int32_t *n_moves,
                  int32_t *converged) {
    ++s.calls;
    s.mounted = mounted;
    s.ctx_ok = ctx == g_ctx;
    s.n = n;
    s.poses.assign(poses, poses + (mounted ? 6 : 5) * n);
    s.fan = *fan;
    s.el_null = el_table == nullptr;
    if (el_table) s.el_table.assign(el_table, el_table + fan->n_el);
    s.rp = *rp;
    s.roi_null = roi == nullptr;
    s.roi_n = roi_n;
    if (roi) s.roi.assign(roi, roi + roi_n);
    s.tab_null = swap_covered == nullptr;
    s.uniq_null = slot_unique == nullptr;
    s.seen_null = seen_points == nullptr;
    s.owner_null = point_owner == nullptr;
    s.moves_null = !move_slot || !move_from || !move_to || !move_covered;
    s.owner_cap = owner_cap;
    if (g.rc != PCP_OK) {   // (an error is left in the context by a call that always fails)
        pcp_crop_voxel(ctx, nullptr, nullptr, 0.f, nullptr, 0, nullptr, nullptr);
        return g.rc;
    }
    for (size_t i = 0; i < g.selected.size(); ++i) selected[i] = g.selected[i];
    *covered = g.covered;
    *start_covered = g.start_covered;
    for (size_t m = 0; m < g.moves.size() && (int)m < rp->max_moves; ++m) {
        move_slot[m] = g.moves[m].slot;
        move_from[m] = g.moves[m].from;
        move_to[m] = g.moves[m].to;
        move_covered[m] = g.moves[m].covered;
    }
    for (size_t i = 0; i < g.uniq.size() && slot_unique; ++i) slot_unique[i] = g.uniq[i];
    for (size_t i = 0; i < g.seen.size() && seen_points; ++i) seen_points[i] = g.seen[i];
    for (size_t i = 0; i < g.owner.size() && point_owner && i < owner_cap; ++i)
        point_owner[i] = g.owner[i];
    *n_points = g.n_points;
    *roi_points = g.roi_points;
    *n_moves = (int32_t)g.moves.size();
    *converged = g.converged;
    return PCP_OK;
}

extern "C" {
int pcp_place_coverage_refine(pcp_ctx *ctx, const double *poses5, uint64_t n,
                              const pcp_fan_params *fan, const pcp_refine_params *rp,
                              const uint8_t *roi, uint64_t roi_n, int64_t *selected,
                              uint64_t *covered, uint64_t *start_covered, int32_t *move_slot,
                              int64_t *move_from, int64_t *move_to, uint64_t *move_covered,
                              int64_t *swap_covered, uint64_t *slot_unique, uint32_t *seen_points,
                              int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                              uint64_t *roi_points, int32_t *n_moves, int32_t *converged) {
    return record(false, ctx, poses5, n, fan, nullptr, rp, roi, roi_n, selected, covered,
                  start_covered, move_slot, move_from, move_to, move_covered, swap_covered,
                  slot_unique, seen_points, point_owner, owner_cap, n_points, roi_points, n_moves,
                  converged);
}
int pcp_place_coverage_refine_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                      const pcp_fan_params *fan, const double *el_table,
                                      const pcp_refine_params *rp, const uint8_t *roi,
                                      uint64_t roi_n, int64_t *selected, uint64_t *covered,
                                      uint64_t *start_covered, int32_t *move_slot,
                                      int64_t *move_from, int64_t *move_to, uint64_t *move_covered,
                                      int64_t *swap_covered, uint64_t *slot_unique,
                                      uint32_t *seen_points, int32_t *point_owner,
                                      uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                                      int32_t *n_moves, int32_t *converged) {
    return record(true, ctx, poses6, n, fan, el_table, rp, roi, roi_n, selected, covered,
                  start_covered, move_slot, move_from, move_to, move_covered, swap_covered,
                  slot_unique, seen_points, point_owner, owner_cap, n_points, roi_points, n_moves,
                  converged);
}
// pcp_cover_node.cpp's greedy methods reference these; nothing here calls them
int pcp_place_coverage(pcp_ctx *, const double *, uint64_t, const pcp_fan_params *,
                       const pcp_cover_params *, const uint8_t *, uint64_t, int64_t *, uint64_t *,
                       uint64_t *, int64_t *, uint32_t *, int32_t *, uint64_t, uint64_t *,
                       uint64_t *, uint64_t *, int32_t *) {
    ++g_fail;
    return PCP_E_INVALID;
}
int pcp_place_coverage_mounted(pcp_ctx *, const double *, uint64_t, const pcp_fan_params *,
                               const double *, const pcp_cover_params *, const uint8_t *, uint64_t,
                               int64_t *, uint64_t *, uint64_t *, int64_t *, uint32_t *, int32_t *,
                               uint64_t, uint64_t *, uint64_t *, uint64_t *, int32_t *) {
    ++g_fail;
    return PCP_E_INVALID;
}
}

// six terrain records of 20 bytes: x, y, z and a tag (the blind spots carry the records whole);
// point 4 is not finite
static PointCloud2 terrain6() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float xyz[6][3] = {{0.f, 0.f, 0.f},  {1.f, 0.5f, 0.25f}, {2.f, 2.f, -1.f},
                             {1.f, -1.f, 0.f}, {nan, 0.f, 0.f},    {1.5f, 0.5f, 0.5f}};
    PointCloud2 m;
    m.frame_id = "map";
    m.stamp = 7.25;
    m.width = 6;
    m.point_step = 20;
    m.row_step = 120;
    m.fields = {{"x", 0, PointField::FLOAT32, 1}, {"y", 4, PointField::FLOAT32, 1},
                {"z", 8, PointField::FLOAT32, 1}, {"tag", 16, PointField::UINT32, 1}};
    m.data.assign(120, 0);
    for (uint32_t i = 0; i < 6; ++i) {
        std::memcpy(m.data.data() + 20 * i, xyz[i], 12);
        const uint32_t tag = 100 + i;
        std::memcpy(m.data.data() + 20 * i + 16, &tag, 4);
    }
    return m;
}

static uint32_t tag_of(const PointCloud2 &m, size_t i) {
    uint32_t t = 0;
    std::memcpy(&t, m.data.data() + m.point_step * i + 16, 4);
    return t;
}

int main() {
    Device dev(0);
    g_ctx = dev.ctx();
    const PointCloud2 terrain = terrain6();
    std::vector<Opt::LidarPosition> cand(4);
    for (int i = 0; i < 4; ++i) {
        cand[i].x = 1.5 * i;
        cand[i].y = i ? -0.25 * i : 0.0;   // (no negative zero in the log)
        cand[i].z = 1.125;
        cand[i].pitch = -0.5;
        cand[i].yaw = 0.75 * i;
    }
    VirtualScan::Params fan;
    fan.n_az = 64;
    fan.n_el = 4;
    fan.max_distance = 12.0;

    // ---- a level call with a locked slot and a box region: two moves, converged -----------------
    {
        CoveragePlacement::Params p;
        p.num_mobile_lidars = 7;   // (not used by the refinement)
        p.min_separation = 2.5;
        CoveragePlacement cpl(p);
        g = Canned{};
        g.selected = {1, 3, 0};
        g.start_covered = 2;
        g.covered = 4;
        g.moves = {{2, 2, 0, 3}, {1, 0, 3, 4}};
        g.uniq = {1, 2, 0};
        g.n_points = 6;
        g.roi_points = 5;
        g.owner = {0, 0, 1, PCP_OWNER_NONE, PCP_OWNER_NONE, 1};
        g.seen = {5, 0, 9, 4};
        s = Seen{};
        const auto r = cpl.refine(dev, terrain, cand, fan, {1, 0, 2}, 1, 9,
                                  CoveragePlacement::Roi(CoveragePlacement::Box{
                                      0.0, 2.0, -1.0, 2.0, -1.0, 0.5}));
        CHECK(r.ran && cpl.lastError().empty());
        CHECK(s.calls == 1 && !s.mounted && s.ctx_ok && s.n == 4);
        const double want[10] = {0.0, 0.0, 1.125, -0.5, 0.0, 1.5, -0.25, 1.125, -0.5, 0.75};
        CHECK(s.poses.size() == 20 && std::vector<double>(s.poses.begin(), s.poses.begin() + 10) ==
                                          std::vector<double>(want, want + 10));
        CHECK(s.fan.n_az == 64 && s.fan.n_el == 4 && s.fan.max_distance == 12.0);
        CHECK(s.fan.el_min == fan.el_min && s.fan.el_max == fan.el_max);
        CHECK(s.rp.k == 3 && s.rp.n_locked == 1 && s.rp.max_moves == 9 && s.rp.reserved == 0);
        CHECK(s.rp.min_separation == 2.5);
        CHECK(s.rp.start[0] == 1 && s.rp.start[1] == 0 && s.rp.start[2] == 2);
        for (int i = 3; i < PCP_PLACE_MAX; ++i) CHECK(s.rp.start[i] == 0);
        CHECK(!s.roi_null && s.roi_n == 6 && s.roi == (std::vector<uint8_t>{1, 1, 1, 1, 0, 1}));
        CHECK(s.tab_null && !s.uniq_null && !s.moves_null);
        CHECK(!s.seen_null && !s.owner_null && s.owner_cap == 6);
        // the answer: the slots in order, each with the points it owns
        CHECK(r.refined && !r.pair_searched && r.converged && r.start_covered == 2);
        CHECK(r.n_locked == 1 && r.slot_unique == (std::vector<uint64_t>{1, 2, 0}));
        CHECK(r.moves.size() == 2 && r.moves[0].slot == 2 && r.moves[0].from == 2);
        CHECK(r.moves[0].to == 0 && r.moves[0].covered == 3 && r.moves[1].slot == 1);
        CHECK(r.moves[1].from == 0 && r.moves[1].to == 3 && r.moves[1].covered == 4);
        CHECK(r.rounds.size() == 3 && r.placed.size() == 3 && r.placed_mounts.empty());
        CHECK(r.rounds[0].candidate == 1 && r.rounds[0].gain == 2 && r.rounds[0].covered == 2);
        CHECK(r.rounds[0].coverage_ratio == 0.4);
        CHECK(r.rounds[1].candidate == 3 && r.rounds[1].gain == 2 && r.rounds[1].covered == 4);
        CHECK(r.rounds[2].candidate == 0 && r.rounds[2].gain == 0 && r.rounds[2].covered == 4);
        CHECK(r.rounds[2].coverage_ratio == 0.8);
        CHECK(r.placed[0].x == 1.5 && r.placed[1].x == 4.5 && r.placed[1].total_score == 4.0);
        CHECK(r.n_fixed == 0 && r.n_points == 6 && r.roi_points == 5 && r.base_covered == 0);
        CHECK(r.seen_points == (std::vector<uint32_t>{5, 0, 9, 4}) && r.point_owner == g.owner);
        // the blind spots: region and no owner -- point 3 (4 lies outside), the record whole
        const PointCloud2 &b = r.blind_spots;
        CHECK(b.width == 1 && b.point_step == 20 && b.row_step == 20 && b.data.size() == 20);
        CHECK(b.frame_id == "map" && b.stamp == 7.25 && b.fields.size() == 4);
        CHECK(tag_of(b, 0) == 103);
        CHECK(std::memcmp(b.data.data(), terrain.data.data() + 60, 20) == 0);
        const std::string want_log =
            "========================================\n"
            "Coverage Placement (0 Fixed + 3 Mobile)\n"
            "========================================\n"
            "Terrain points in region: 5 of 6\n"
            "  Covered by fixed sensors: 0 (0.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 1 Position: (1.50, -0.25, 1.12)  [candidate 1]\n"
            "  Points gained: 2\n"
            "  Covered points: 2 of 5 (40.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 2 Position: (4.50, -0.75, 1.12)  [candidate 3]\n"
            "  Points gained: 2\n"
            "  Covered points: 4 of 5 (80.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 3 Position: (0.00, 0.00, 1.12)  [candidate 0]\n"
            "  Points gained: 0\n"
            "  Covered points: 4 of 5 (80.0%)\n"
            "----------------------------------------\n"
            "Exchange refinement (1 locked): start 2 points (40.0%)\n"
            "  Move 1: slot 2, candidate 2 -> 0, covered 3 (60.0%)\n"
            "  Move 2: slot 1, candidate 0 -> 3, covered 4 (80.0%)\n"
            "  No single move adds a point after 2 moves\n"
            "----------------------------------------\n"
            "Blind spots: 1 of 5 (20.0%)\n"
            "========================================\n";
        if (r.log != want_log) std::printf("log:\n%s", r.log.c_str());
        CHECK(r.log == want_log && coverage_log(r) == want_log);
    }

    // ---- mounted, a beam table, every point: the moves run out ----------------------------------
    {
        CoveragePlacement cpl;
        std::vector<VirtualScan::SensorPose> mounts(2);
        mounts[0].x = 1.0;
        mounts[0].roll = 0.25;
        mounts[1].y = -2.0;
        mounts[1].z = 0.5;
        mounts[1].pitch = -0.125;
        mounts[1].yaw = 3.0;
        VirtualScan::Params mf = fan;
        mf.el_table = {-0.5, -0.25, 0.0, 0.125};
        g = Canned{};
        g.selected = {1};
        g.start_covered = 3;
        g.covered = 4;
        g.moves = {{0, 0, 1, 4}};
        g.converged = 0;
        g.uniq = {4};
        g.n_points = 6;
        g.roi_points = 6;
        g.owner = {0, 0, 0, 0, PCP_OWNER_NONE, PCP_OWNER_NONE};
        g.seen = {3, 4};
        s = Seen{};
        const auto r = cpl.refine_mounted(dev, terrain, mounts, mf, {0}, 0, 1);
        CHECK(r.ran && s.calls == 1 && s.mounted && s.n == 2 && s.roi_null);
        const double want[12] = {1.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, -2.0, 0.5, 0.0, -0.125, 3.0};
        CHECK(s.poses == std::vector<double>(want, want + 12));
        CHECK(!s.el_null && s.el_table == mf.el_table);
        CHECK(s.rp.k == 1 && s.rp.n_locked == 0 && s.rp.max_moves == 1);
        CHECK(s.rp.min_separation == 0.0);
        CHECK(r.rounds.size() == 1 && r.rounds[0].candidate == 1 && r.rounds[0].gain == 4);
        CHECK(r.rounds[0].covered == 4 && r.placed.empty() && r.placed_mounts.size() == 1);
        CHECK(r.placed_mounts[0].yaw == 3.0 && !r.converged && r.moves.size() == 1);
        CHECK(r.blind_spots.width == 2 && tag_of(r.blind_spots, 0) == 104);
        CHECK(r.log.find("Coverage Placement (0 Fixed + 1 Mobile)") != std::string::npos);
        CHECK(r.log.find("  Moves ran out after 1 move\n") != std::string::npos);
        CHECK(r.log.find("Blind spots: 2 of 6 (33.3%)") != std::string::npos);
        // without a table the call gets none; without moves the arrays are still the caller's
        s = Seen{};
        mf.el_table.clear();
        g.moves.clear();
        g.covered = 4;
        CHECK(cpl.refine_mounted(dev, terrain, mounts, mf, {1}, 1, 0).ran && s.el_null);
        CHECK(s.rp.max_moves == 0 && s.rp.n_locked == 1);
    }

    // ---- refusals -------------------------------------------------------------------------------
    {
        CoveragePlacement cpl;
        s = Seen{};
        VirtualScan::Params bad = fan;
        bad.n_az = 0;
        CHECK(!cpl.refine(dev, terrain, cand, bad, {0}).ran && !cpl.lastError().empty());
        CHECK(!cpl.refine(dev, terrain, cand, fan, {}).ran && !cpl.lastError().empty());
        std::vector<int64_t> many(PCP_PLACE_MAX + 1, 0);
        CHECK(!cpl.refine(dev, terrain, cand, fan, many).ran && !cpl.lastError().empty());
        CHECK(!cpl.refine(dev, terrain, cand, fan, {0}, 0, -1).ran);
        CHECK(!cpl.refine(dev, terrain, cand, fan, {0}, 0, PCP_REFINE_MAX_MOVES + 1).ran);
        CHECK(!cpl.refine(dev, terrain, cand, fan, {0}, 0, 16,
                          CoveragePlacement::Roi(std::vector<uint8_t>(5, 1))).ran);
        std::vector<VirtualScan::SensorPose> mounts(1);
        bad = fan;
        bad.el_table = {0.0, 0.1};
        CHECK(!cpl.refine_mounted(dev, terrain, mounts, bad, {0}).ran);
        CHECK(s.calls == 0);
        // the library refuses: its message is passed on
        g = Canned{};
        g.rc = PCP_E_INVALID;
        const auto r = cpl.refine(dev, terrain, cand, fan, {0, 0});
        CHECK(!r.ran && s.calls == 1 && !cpl.lastError().empty() && r.rounds.empty());
        // a terrain message that is not the index's cloud
        g = Canned{};
        g.selected = {0};
        g.n_points = 7;
        CHECK(!cpl.refine(dev, terrain, cand, fan, {0}).ran && !cpl.lastError().empty());
        // owners that do not add up to the count
        g.n_points = 6;
        g.covered = 2;
        g.owner = {0, PCP_OWNER_NONE, PCP_OWNER_NONE, PCP_OWNER_NONE, PCP_OWNER_NONE, PCP_OWNER_NONE};
        CHECK(!cpl.refine(dev, terrain, cand, fan, {0}).ran && !cpl.lastError().empty());
        // and a good call clears the error
        g.covered = 1;
        CHECK(cpl.refine(dev, terrain, cand, fan, {0}).ran && cpl.lastError().empty());
    }

    if (g_fail) {
        std::printf("cover_refine_host_selftest: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("cover_refine_host_selftest ok\n");
    return 0;
}
