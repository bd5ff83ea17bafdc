// cover_aim_host_selftest.cpp -- what AimedCoveragePlacement::place / place_mounted
// (pcp_cover_aim_node.hpp) hand to the C ABI and make of its answers, on the CPU.  Linked from
// pcp_cover_aim_node.cpp, pcp_cover_node.cpp, pcp_nodes.cpp, the shell tests' mock_pcp.cpp and the
// two pcp_place_coverage_aimed entry points below, which record what they were given and return
// the answers a case has set.  The program checks the marshalling, the rounds with their aims, the
// blind-spot records, the log text and the refusal paths itself and ends with status 0 and
// "cover_aim_host_selftest ok" only if every check held.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcp_cover_aim_node.hpp"

using namespace pcp;
using Opt = SimplifiedDualLidarOptimizer;
using Aimed = AimedCoveragePlacement;

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
    std::vector<int64_t> sel;
    std::vector<int32_t> sel_aim;
    std::vector<uint64_t> gain, cov;
    uint64_t n_points = 0, roi_points = 0, base_covered = 0;
    std::vector<int32_t> owner;
    std::vector<uint32_t> seen, aim_points;
};
struct Seen {
    int calls = 0;
    bool mounted = false, ctx_ok = false;
    std::vector<double> poses, el_table;
    bool el_null = true, roi_null = true, rg_null = true, seen_null = true, ap_null = true,
         owner_null = true;
    uint64_t n = 0, roi_n = 0, owner_cap = 0;
    pcp_fan_params fan{};
    pcp_cover_aim_params ap{};
    std::vector<int32_t> aims;
    std::vector<uint8_t> roi;
};
static Canned g;
static Seen s;
static pcp_ctx *g_ctx = nullptr;

static int record(bool mounted, pcp_ctx *ctx, const double *poses, uint64_t n,
                  const pcp_fan_params *fan, const double *el_table,
                  const pcp_cover_aim_params *ap, const int32_t *aims, const uint8_t *roi,
                  uint64_t roi_n, int64_t *selected, int32_t *selected_aim, uint64_t *gain,
                  uint64_t *covered_after, int64_t *round_gains, uint32_t *seen_points,
                  uint32_t *aim_points, int32_t *point_owner, uint64_t owner_cap,
                  uint64_t *n_points, uint64_t *roi_points, uint64_t *base_covered,
                  int32_t *n_selected) {
    ++s.calls;
    s.mounted = mounted;
    s.ctx_ok = ctx == g_ctx;
    s.n = n;
    s.poses.assign(poses, poses + (mounted ? 6 : 5) * n);
    s.fan = *fan;
    s.el_null = el_table == nullptr;
    if (el_table) s.el_table.assign(el_table, el_table + fan->n_el);
    s.ap = *ap;
    s.aims.assign(aims, aims + 2 * (size_t)ap->n_aims);
    s.roi_null = roi == nullptr;
    s.roi_n = roi_n;
    if (roi) s.roi.assign(roi, roi + roi_n);
    s.rg_null = round_gains == nullptr;
    s.seen_null = seen_points == nullptr;
    s.ap_null = aim_points == nullptr;
    s.owner_null = point_owner == nullptr;
    s.owner_cap = owner_cap;
    if (g.rc != PCP_OK) {   // (an error is left in the context by a call that always fails)
        pcp_crop_voxel(ctx, nullptr, nullptr, 0.f, nullptr, 0, nullptr, nullptr);
        return g.rc;
    }
    for (int32_t i = 0; i < g.ns; ++i) {
        selected[i] = g.sel[(size_t)i];
        selected_aim[i] = g.sel_aim[(size_t)i];
        gain[i] = g.gain[(size_t)i];
        covered_after[i] = g.cov[(size_t)i];
    }
    for (size_t i = 0; i < g.seen.size() && seen_points; ++i) seen_points[i] = g.seen[i];
    for (size_t i = 0; i < g.aim_points.size() && aim_points; ++i) aim_points[i] = g.aim_points[i];
    for (size_t i = 0; i < g.owner.size() && point_owner && i < owner_cap; ++i)
        point_owner[i] = g.owner[i];
    *n_points = g.n_points;
    *roi_points = g.roi_points;
    *base_covered = g.base_covered;
    *n_selected = g.ns;
    return PCP_OK;
}

extern "C" {
int pcp_place_coverage_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n,
                             const pcp_fan_params *fan, const pcp_cover_aim_params *ap,
                             const int32_t *aims, const uint8_t *roi, uint64_t roi_n,
                             int64_t *selected, int32_t *selected_aim, uint64_t *gain,
                             uint64_t *covered_after, int64_t *round_gains, uint32_t *seen_points,
                             uint32_t *aim_points, int32_t *point_owner, uint64_t owner_cap,
                             uint64_t *n_points, uint64_t *roi_points, uint64_t *base_covered,
                             int32_t *n_selected) {
    return record(false, ctx, poses5, n, fan, nullptr, ap, aims, roi, roi_n, selected,
                  selected_aim, gain, covered_after, round_gains, seen_points, aim_points,
                  point_owner, owner_cap, n_points, roi_points, base_covered, n_selected);
}
int pcp_place_coverage_aimed_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                     const pcp_fan_params *fan, const double *el_table,
                                     const pcp_cover_aim_params *ap, const int32_t *aims,
                                     const uint8_t *roi, uint64_t roi_n, int64_t *selected,
                                     int32_t *selected_aim, uint64_t *gain,
                                     uint64_t *covered_after, int64_t *round_gains,
                                     uint32_t *seen_points, uint32_t *aim_points,
                                     int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                                     uint64_t *roi_points, uint64_t *base_covered,
                                     int32_t *n_selected) {
    return record(true, ctx, poses6, n, fan, el_table, ap, aims, roi, roi_n, selected, selected_aim,
                  gain, covered_after, round_gains, seen_points, aim_points, point_owner, owner_cap,
                  n_points, roi_points, base_covered, n_selected);
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

static Aimed::Aim aim(int32_t az0, int32_t el0) {
    Aimed::Aim a;
    a.az0 = az0;
    a.el0 = el0;
    return a;
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
    Aimed::Params base;
    base.num_mobile_lidars = 3;
    base.min_separation = 2.5;
    base.w_az = 16;
    base.w_el = 2;
    base.aims = {aim(0, 0), aim(56, 2), aim(24, 1)};

    // ---- a level call with a fixed (candidate, aim) and a box region ---------------------------
    {
        Aimed apl(base);
        g = Canned{};
        g.ns = 2;
        g.sel = {3, 0};
        g.sel_aim = {1, 2};
        g.gain = {2, 1};
        g.cov = {3, 4};
        g.n_points = 6;
        g.roi_points = 5;
        g.base_covered = 1;
        g.owner = {2, 0, 1, PCP_OWNER_NONE, PCP_OWNER_NONE, 1};
        g.seen = {5, 0, 9, 4};
        g.aim_points = {1, 2, 3, 0, 0, 0, 4, 5, 6, 7, 8, 9};
        s = Seen{};
        Aimed::Fixed f;
        f.candidate = 1;
        f.aim = 2;
        const auto r = apl.place(dev, terrain, cand, fan, {f},
                                 Aimed::Roi(CoverageBox{0.0, 2.0, -1.0, 2.0, -1.0, 0.5}));
        CHECK(r.ran && apl.lastError().empty());
        CHECK(s.calls == 1 && !s.mounted && s.ctx_ok && s.n == 4);
        const double want[10] = {0.0, 0.0, 1.125, -0.5, 0.0, 1.5, -0.25, 1.125, -0.5, 0.75};
        CHECK(s.poses.size() == 20 && std::vector<double>(s.poses.begin(), s.poses.begin() + 10) ==
                                          std::vector<double>(want, want + 10));
        CHECK(s.fan.n_az == 64 && s.fan.n_el == 4 && s.fan.max_distance == 12.0);
        CHECK(s.fan.el_min == fan.el_min && s.fan.el_max == fan.el_max);
        CHECK(s.ap.k_max == 3 && s.ap.n_aims == 3 && s.ap.n_fixed == 1 && s.ap.w_az == 16 &&
              s.ap.w_el == 2 && s.ap.min_separation == 2.5);
        CHECK(s.ap.reserved[0] == 0 && s.ap.reserved[1] == 0 && s.ap.reserved[2] == 0);
        CHECK(s.ap.fixed_pose[0] == 1 && s.ap.fixed_aim[0] == 2);
        for (int i = 1; i < PCP_PLACE_MAX; ++i)
            CHECK(s.ap.fixed_pose[i] == 0 && s.ap.fixed_aim[i] == 0);
        CHECK(s.aims == (std::vector<int32_t>{0, 0, 56, 2, 24, 1}));
        CHECK(!s.roi_null && s.roi_n == 6 && s.roi == (std::vector<uint8_t>{1, 1, 1, 1, 0, 1}));
        CHECK(s.rg_null && !s.seen_null && !s.ap_null && !s.owner_null && s.owner_cap == 6);
        // the answer: rounds with their aims
        CHECK(r.rounds.size() == 2 && r.aim == (std::vector<int32_t>{1, 2}));
        CHECK(r.placed.size() == 2 && r.placed_mounts.empty());
        CHECK(r.rounds[0].candidate == 3 && r.rounds[0].gain == 2 && r.rounds[0].covered == 3);
        CHECK(r.rounds[0].coverage_ratio == 0.6);
        CHECK(r.rounds[1].candidate == 0 && r.rounds[1].gain == 1 && r.rounds[1].covered == 4);
        CHECK(r.placed[0].x == 4.5 && r.placed[0].total_score == 3.0 && r.placed[1].x == 0.0);
        CHECK(r.n_fixed == 1 && r.n_points == 6 && r.roi_points == 5 && r.base_covered == 1);
        CHECK(r.w_az == 16 && r.w_el == 2 && r.aims.size() == 3 && r.aims[1].az0 == 56);
        CHECK(r.seen_points == (std::vector<uint32_t>{5, 0, 9, 4}) && r.point_owner == g.owner);
        CHECK(r.aim_points == g.aim_points);
        // the blind spots: region and no owner -- point 3 (4 lies outside), the record whole
        const PointCloud2 &b = r.blind_spots;
        CHECK(b.width == 1 && b.point_step == 20 && b.row_step == 20 && b.data.size() == 20);
        CHECK(b.frame_id == "map" && b.stamp == 7.25 && b.fields.size() == 4);
        CHECK(tag_of(b, 0) == 103);
        CHECK(std::memcmp(b.data.data(), terrain.data.data() + 60, 20) == 0);
        const std::string want_log =
            "========================================\n"
            "Aimed Coverage Placement (1 Fixed + 2 Mobile)\n"
            "========================================\n"
            "Window: 16 columns x 2 rings, 3 aims per candidate\n"
            "Terrain points in region: 5 of 6\n"
            "  Covered by fixed sensors: 1 (20.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 1 Position: (4.50, -0.75, 1.12)  [candidate 3]\n"
            "  Aim 1: columns from 56, rings from 2\n"
            "  Points gained: 2\n"
            "  Covered points: 3 of 5 (60.0%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 2 Position: (0.00, 0.00, 1.12)  [candidate 0]\n"
            "  Aim 2: columns from 24, rings from 1\n"
            "  Points gained: 1\n"
            "  Covered points: 4 of 5 (80.0%)\n"
            "----------------------------------------\n"
            "Blind spots: 1 of 5 (20.0%)\n"
            "========================================\n";
        if (r.log != want_log) std::printf("log:\n%s", r.log.c_str());
        CHECK(r.log == want_log && aimed_coverage_log(r) == want_log);
    }

    // ---- mounted, a beam table, every point ----------------------------------------------------
    {
        Aimed::Params p = base;
        p.min_separation = 0.0;
        p.num_mobile_lidars = 1;
        Aimed apl(p);
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
        g.ns = 1;
        g.sel = {1};
        g.sel_aim = {0};
        g.gain = {4};
        g.cov = {4};
        g.n_points = 6;
        g.roi_points = 6;
        g.owner = {0, 0, 0, 0, PCP_OWNER_NONE, PCP_OWNER_NONE};
        g.seen = {3, 4};
        s = Seen{};
        const auto r = apl.place_mounted(dev, terrain, mounts, mf);
        CHECK(r.ran && s.calls == 1 && s.mounted && s.n == 2 && s.roi_null);
        const double want[12] = {1.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, -2.0, 0.5, 0.0, -0.125, 3.0};
        CHECK(s.poses == std::vector<double>(want, want + 12));
        CHECK(!s.el_null && s.el_table == mf.el_table);
        CHECK(s.ap.k_max == 1 && s.ap.n_fixed == 0 && s.ap.min_separation == 0.0);
        CHECK(r.rounds.size() == 1 && r.rounds[0].candidate == 1 && r.aim[0] == 0);
        CHECK(r.placed.empty() && r.placed_mounts.size() == 1 && r.placed_mounts[0].yaw == 3.0);
        CHECK(r.blind_spots.width == 2 && tag_of(r.blind_spots, 0) == 104);
        CHECK(r.log.find("Aimed Coverage Placement (0 Fixed + 1 Mobile)") != std::string::npos);
        CHECK(r.log.find("  Aim 0: columns from 0, rings from 0\n") != std::string::npos);
        CHECK(r.log.find("Blind spots: 2 of 6 (33.3%)") != std::string::npos);
        // without a table the call gets none
        s = Seen{};
        mf.el_table.clear();
        CHECK(apl.place_mounted(dev, terrain, mounts, mf).ran && s.el_null);
    }

    // ---- nothing adds anything: no rounds, every point of the region blind; no candidates ------
    {
        Aimed apl(base);
        g = Canned{};
        g.n_points = 6;
        g.roi_points = 6;
        g.owner.assign(6, PCP_OWNER_NONE);
        s = Seen{};
        const auto r = apl.place(dev, terrain, cand, fan);
        CHECK(r.ran && r.rounds.empty() && r.aim.empty() && r.blind_spots.width == 6);
        CHECK(r.aim_points.size() == 12);
        const auto e = apl.place(dev, terrain, {}, fan);
        CHECK(e.ran && e.seen_points.empty() && e.aim_points.empty() && s.n == 0);
    }

    // ---- refusals -------------------------------------------------------------------------------
    {
        Aimed apl(base);
        s = Seen{};
        VirtualScan::Params bad = fan;
        bad.n_az = 0;
        CHECK(!apl.place(dev, terrain, cand, bad).ran && !apl.lastError().empty());
        std::vector<Aimed::Fixed> many(PCP_PLACE_MAX + 1);
        CHECK(!apl.place(dev, terrain, cand, fan, many).ran && !apl.lastError().empty());
        CHECK(!apl.place(dev, terrain, cand, fan, {}, Aimed::Roi(std::vector<uint8_t>(5, 1))).ran);
        std::vector<VirtualScan::SensorPose> mounts(1);
        bad = fan;
        bad.el_table = {0.0, 0.1};
        CHECK(!apl.place_mounted(dev, terrain, mounts, bad).ran);
        Aimed none(base);
        none.params().aims.clear();
        CHECK(!none.place(dev, terrain, cand, fan).ran && !none.lastError().empty());
        none.params().aims.assign(PCP_COVER_AIM_MAX + 1, aim(0, 0));
        CHECK(!none.place(dev, terrain, cand, fan).ran && !none.lastError().empty());
        CHECK(s.calls == 0);
        // the library refuses: its message is passed on
        g = Canned{};
        g.rc = PCP_E_INVALID;
        const auto r = apl.place(dev, terrain, cand, fan);
        CHECK(!r.ran && s.calls == 1 && !apl.lastError().empty() && r.rounds.empty());
        // a terrain message that is not the index's cloud
        g = Canned{};
        g.n_points = 7;
        CHECK(!apl.place(dev, terrain, cand, fan).ran && !apl.lastError().empty());
        // and a good call clears the error
        g.n_points = 6;
        g.owner.assign(6, PCP_OWNER_NONE);
        CHECK(apl.place(dev, terrain, cand, fan).ran && apl.lastError().empty());
    }

    if (g_fail) {
        std::printf("cover_aim_host_selftest: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("cover_aim_host_selftest ok\n");
    return 0;
}
