// cover_host_selftest.cpp -- what CoveragePlacement (pcp_cover_node.hpp) hands to the C ABI and
// makes of its answers, on the CPU.  Linked from pcp_cover_node.cpp, pcp_nodes.cpp, the shell
// tests' mock_pcp.cpp and the two pcp_place_coverage entry points below, which record what they
// were given and return the answers a case has set.  The program checks the marshalling, the box
// region's bytes, the blind-spot records, the log text and the refusal paths itself and ends with
// status 0 and "cover_host_selftest ok" only if every check held.  Only the public surface of
// pcp_cover_node.hpp is used.
#include <cmath>
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
struct Canned {
    int rc = PCP_OK;
    int32_t ns = 0;
    int64_t sel[PCP_PLACE_MAX] = {};
    uint64_t gain[PCP_PLACE_MAX] = {}, cov[PCP_PLACE_MAX] = {};
    uint64_t n_points = 0, roi_points = 0, base_covered = 0;
    std::vector<int32_t> owner;
    std::vector<uint32_t> seen;
};
struct Seen {
    int calls = 0;
    bool mounted = false, ctx_ok = false;
    std::vector<double> poses, el_table;
    bool el_null = true, roi_null = true, rg_null = true, seen_null = true, owner_null = true;
    uint64_t n = 0, roi_n = 0, owner_cap = 0;
    pcp_fan_params fan{};
    pcp_cover_params cp{};
    std::vector<uint8_t> roi;
};
static Canned g;
static Seen s;
static pcp_ctx *g_ctx = nullptr;

static int record(bool mounted, pcp_ctx *ctx, const double *poses, uint64_t n,
                  const pcp_fan_params *fan, const double *el_table, const pcp_cover_params *cp,
                  const uint8_t *roi, uint64_t roi_n, int64_t *selected, uint64_t *gain,
                  uint64_t *covered_after, int64_t *round_gains, uint32_t *seen_points,
                  int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                  uint64_t *roi_points, uint64_t *base_covered, int32_t *n_selected) {
    ++s.calls;
    s.mounted = mounted;
    s.ctx_ok = ctx == g_ctx;
    s.n = n;
    s.poses.assign(poses, poses + (mounted ? 6 : 5) * n);
    s.fan = *fan;
    s.el_null = el_table == nullptr;
    if (el_table) s.el_table.assign(el_table, el_table + fan->n_el);
    s.cp = *cp;
    s.roi_null = roi == nullptr;
    s.roi_n = roi_n;
    if (roi) s.roi.assign(roi, roi + roi_n);
    s.rg_null = round_gains == nullptr;
    s.seen_null = seen_points == nullptr;
    s.owner_null = point_owner == nullptr;
    s.owner_cap = owner_cap;
    if (g.rc != PCP_OK) {   // (an error is left in the context by a call that always fails)
        pcp_crop_voxel(ctx, nullptr, nullptr, 0.f, nullptr, 0, nullptr, nullptr);
        return g.rc;
    }
    for (int32_t i = 0; i < g.ns; ++i) {
        selected[i] = g.sel[i];
        gain[i] = g.gain[i];
        covered_after[i] = g.cov[i];
    }
    for (size_t i = 0; i < g.seen.size() && seen_points; ++i) seen_points[i] = g.seen[i];
    for (size_t i = 0; i < g.owner.size() && point_owner && i < owner_cap; ++i)
        point_owner[i] = g.owner[i];
    *n_points = g.n_points;
    *roi_points = g.roi_points;
    *base_covered = g.base_covered;
    *n_selected = g.ns;
    return PCP_OK;
}

extern "C" {
int pcp_place_coverage(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                       const pcp_cover_params *cp, const uint8_t *roi, uint64_t roi_n,
                       int64_t *selected, uint64_t *gain, uint64_t *covered_after,
                       int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                       uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                       uint64_t *base_covered, int32_t *n_selected) {
    return record(false, ctx, poses5, n, fan, nullptr, cp, roi, roi_n, selected, gain,
                  covered_after, round_gains, seen_points, point_owner, owner_cap, n_points,
                  roi_points, base_covered, n_selected);
}
int pcp_place_coverage_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                               const pcp_fan_params *fan, const double *el_table,
                               const pcp_cover_params *cp, const uint8_t *roi, uint64_t roi_n,
                               int64_t *selected, uint64_t *gain, uint64_t *covered_after,
                               int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                               uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                               uint64_t *base_covered, int32_t *n_selected) {
    return record(true, ctx, poses6, n, fan, el_table, cp, roi, roi_n, selected, gain,
                  covered_after, round_gains, seen_points, point_owner, owner_cap, n_points,
                  roi_points, base_covered, n_selected);
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
    std::vector<Opt::LidarPosition> cand(3);
    for (int i = 0; i < 3; ++i) {
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

    // ---- the box region as bytes: bounds included, the non-finite point outside ---------------
    {
        std::vector<uint8_t> roi;
        CoveragePlacement::Box box{1.0, 2.0, 0.0, 2.0, -1.0, 0.5};
        CHECK(coverage_roi_bytes(terrain, box, roi));
        CHECK(roi == (std::vector<uint8_t>{0, 1, 1, 0, 0, 1}));
        PointCloud2 nofields = terrain;
        nofields.fields.clear();
        std::string why;
        CHECK(!coverage_roi_bytes(nofields, box, roi, &why) && !why.empty());
    }

    // ---- a level call with fixed candidates and a box region ----------------------------------
    {
        CoveragePlacement::Params p;
        p.num_mobile_lidars = 3;
        p.min_separation = 2.5;
        CoveragePlacement cpl(p);
        g = Canned{};
        g.ns = 2;
        g.sel[0] = 2;
        g.sel[1] = 0;
        g.gain[0] = 2;
        g.gain[1] = 0;   // (whatever the library says is passed on)
        g.cov[0] = 3;
        g.cov[1] = 3;
        g.n_points = 6;
        g.roi_points = 4;
        g.base_covered = 1;
        g.owner = {PCP_OWNER_NONE, 0, 1, PCP_OWNER_NONE, PCP_OWNER_NONE, PCP_OWNER_NONE};
        g.seen = {5, 0, 9};
        s = Seen{};
        const auto r = cpl.place(dev, terrain, cand, fan, {1},
                                 CoveragePlacement::Roi(CoveragePlacement::Box{0.0, 2.0, 0.0, 2.0,
                                                                                -1.0, 0.5}));
        CHECK(r.ran && cpl.lastError().empty());
        CHECK(s.calls == 1 && !s.mounted && s.ctx_ok && s.n == 3);
        const double want[15] = {0.0, 0.0, 1.125, -0.5, 0.0,  1.5, -0.25, 1.125, -0.5, 0.75,
                                 3.0, -0.5, 1.125, -0.5, 1.5};
        CHECK(s.poses == std::vector<double>(want, want + 15));
        CHECK(s.fan.n_az == 64 && s.fan.n_el == 4 && s.fan.max_distance == 12.0);
        CHECK(s.fan.el_min == fan.el_min && s.fan.el_max == fan.el_max);
        CHECK(s.cp.k_max == 3 && s.cp.n_fixed == 1 && s.cp.min_separation == 2.5);
        CHECK(s.cp.reserved[0] == 0 && s.cp.reserved[1] == 0 && s.cp.fixed[0] == 1);
        for (int i = 1; i < PCP_PLACE_MAX; ++i) CHECK(s.cp.fixed[i] == 0);
        CHECK(!s.roi_null && s.roi_n == 6 && s.roi == (std::vector<uint8_t>{1, 1, 1, 0, 0, 1}));
        CHECK(s.rg_null && !s.seen_null && !s.owner_null && s.owner_cap == 6);
        // the answer
        CHECK(r.rounds.size() == 2 && r.placed.size() == 2 && r.placed_mounts.empty());
        CHECK(r.rounds[0].candidate == 2 && r.rounds[0].gain == 2 && r.rounds[0].covered == 3);
        CHECK(r.rounds[0].coverage_ratio == 0.75 && r.rounds[1].candidate == 0);
        CHECK(r.placed[0].x == 3.0 && r.placed[0].yaw == 1.5 && r.placed[0].total_score == 3.0);
        CHECK(r.placed[1].x == 0.0 && r.n_fixed == 1);
        CHECK(r.n_points == 6 && r.roi_points == 4 && r.base_covered == 1);
        CHECK(r.seen_points == (std::vector<uint32_t>{5, 0, 9}) && r.point_owner == g.owner);
        // the blind spots: region and no owner -- points 0 and 5 (3 and 4 lie outside), whole
        // records in input order, the message's layout
        const PointCloud2 &b = r.blind_spots;
        CHECK(b.width == 2 && b.point_step == 20 && b.row_step == 40 && b.data.size() == 40);
        CHECK(b.frame_id == "map" && b.stamp == 7.25 && b.fields.size() == 4);
        CHECK(tag_of(b, 0) == 100 && tag_of(b, 1) == 105);
        CHECK(std::memcmp(b.data.data() + 20, terrain.data.data() + 100, 20) == 0);
        const std::string want_log =
            "========================================\n"
            "Coverage Placement (1 Fixed + 2 Mobile)\n"
            "========================================\n"
            "Terrain points in region: 4 of 6\n"
            "  Covered by fixed sensors: 1 (25.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 1 Position: (3.00, -0.50, 1.12)  [candidate 2]\n"
            "  Points gained: 2\n"
            "  Covered points: 3 of 4 (75.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 2 Position: (0.00, 0.00, 1.12)  [candidate 0]\n"
            "  Points gained: 0\n"
            "  Covered points: 3 of 4 (75.0%)\n"
            "----------------------------------------\n"
            "Blind spots: 1 of 4 (25.0%)\n"
            "========================================\n";
        if (r.log != want_log) std::printf("log:\n%s", r.log.c_str());
        CHECK(r.log == want_log && coverage_log(r) == want_log);
    }

    // ---- region bytes, every point, no fixed ---------------------------------------------------
    {
        CoveragePlacement cpl;
        g = Canned{};
        g.n_points = 6;
        g.roi_points = 2;
        g.owner.assign(6, PCP_OWNER_NONE);
        s = Seen{};
        auto r = cpl.place(dev, terrain, cand, fan, {},
                           CoveragePlacement::Roi(std::vector<uint8_t>{0, 0, 7, 0, 1, 0}));
        CHECK(r.ran && !s.roi_null && s.roi == (std::vector<uint8_t>{0, 0, 7, 0, 1, 0}));
        CHECK(s.cp.k_max == 2 && s.cp.n_fixed == 0 && s.cp.min_separation == 0.0);
        CHECK(r.rounds.empty() && r.blind_spots.width == 2 && tag_of(r.blind_spots, 0) == 102 &&
              tag_of(r.blind_spots, 1) == 104);
        CHECK(r.log.find("Coverage Placement (0 Fixed + 0 Mobile)") != std::string::npos);
        CHECK(r.log.find("Blind spots: 2 of 2 (100.0%)") != std::string::npos);
        s = Seen{};
        g.roi_points = 6;
        r = cpl.place(dev, terrain, cand, fan);
        CHECK(r.ran && s.roi_null && s.roi_n == 6 && r.blind_spots.width == 6);
    }

    // ---- the mounted twin with a beam table ----------------------------------------------------
    {
        std::vector<VirtualScan::SensorPose> mounts(2);
        mounts[0] = VirtualScan::SensorPose{1.0, 2.0, 3.0, 0.1, -0.4363, 0.5};
        mounts[1] = VirtualScan::SensorPose{-1.0, 0.0, 2.0, 0.0, 0.0, -1.0};
        VirtualScan::Params mf = fan;
        mf.el_table = {-0.3, 0.1, -0.1, 0.2};
        CoveragePlacement cpl;
        g = Canned{};
        g.ns = 1;
        g.sel[0] = 1;
        g.gain[0] = 6;
        g.cov[0] = 6;
        g.n_points = 6;
        g.roi_points = 6;
        g.owner.assign(6, 1);
        s = Seen{};
        auto r = cpl.place_mounted(dev, terrain, mounts, mf, {0});
        CHECK(r.ran && s.mounted && s.n == 2 && !s.el_null && s.el_table == mf.el_table);
        const double want[12] = {1.0, 2.0, 3.0, 0.1, -0.4363, 0.5, -1.0, 0.0, 2.0, 0.0, 0.0, -1.0};
        CHECK(s.poses == std::vector<double>(want, want + 12));
        CHECK(r.placed.empty() && r.placed_mounts.size() == 1 && r.placed_mounts[0].x == -1.0);
        CHECK(r.blind_spots.width == 0 && r.blind_spots.data.empty());
        CHECK(r.log.find("Mobile LiDAR 1 Position: (-1.00, 0.00, 2.00)  [candidate 1]") !=
              std::string::npos);
        mf.el_table.clear();   // no table: the uniform rings
        s = Seen{};
        r = cpl.place_mounted(dev, terrain, mounts, mf);
        CHECK(r.ran && s.mounted && s.el_null);
    }

    // ---- refusals: nothing reaches the library, or its error is passed on ----------------------
    {
        CoveragePlacement cpl;
        g = Canned{};
        g.n_points = 6;
        s = Seen{};
        VirtualScan::Params bad = fan;
        bad.n_az = 0;
        CHECK(!cpl.place(dev, terrain, cand, bad).ran && !cpl.lastError().empty() && s.calls == 0);
        std::vector<Opt::LidarPosition> many(PCP_COVER_MAX_POSES + 1);
        CHECK(!cpl.place(dev, terrain, many, fan).ran && s.calls == 0);
        CHECK(!cpl.place(dev, terrain, cand, fan, std::vector<int64_t>(PCP_PLACE_MAX + 1, 0)).ran &&
              s.calls == 0);
        CHECK(!cpl.place(dev, terrain, cand, fan, {},
                         CoveragePlacement::Roi(std::vector<uint8_t>{1, 1})).ran && s.calls == 0);
        CHECK(cpl.lastError().find("one byte per terrain point") != std::string::npos);
        PointCloud2 nofields = terrain;
        nofields.fields.clear();
        CHECK(!cpl.place(dev, nofields, cand, fan, {},
                         CoveragePlacement::Roi(CoveragePlacement::Box{})).ran && s.calls == 0);
        VirtualScan::Params mf = fan;
        mf.el_table = {0.1, 0.2};
        CHECK(!cpl.place_mounted(dev, terrain, {VirtualScan::SensorPose{}}, mf).ran && s.calls == 0);
        // the library refuses: its error text is the layer's
        g.rc = PCP_E_INVALID;
        auto r = cpl.place(dev, terrain, cand, fan);
        CHECK(!r.ran && s.calls == 1 && r.rounds.empty() && r.log.empty());
        CHECK(cpl.lastError().find("mock libpcp") != std::string::npos);
        // another cloud's index: the point counts differ
        g.rc = PCP_OK;
        g.n_points = 5;
        r = cpl.place(dev, terrain, cand, fan);
        CHECK(!r.ran && cpl.lastError().find("not the cloud") != std::string::npos);
        // and a good call clears the error
        g.n_points = 6;
        g.owner.assign(6, PCP_OWNER_NONE);
        r = cpl.place(dev, terrain, cand, fan);
        CHECK(r.ran && cpl.lastError().empty());
    }

    if (g_fail) {
        std::printf("cover_host_selftest: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("cover_host_selftest ok\n");
    return 0;
}
