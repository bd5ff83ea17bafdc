// cover_weight_host_selftest.cpp -- what WeightedCoveragePlacement::place / place_mounted
// (pcp_cover_weight_node.hpp) hand to the C ABI and make of its answers, on the CPU.  Linked from
// pcp_cover_weight_node.cpp, pcp_cover_node.cpp, pcp_nodes.cpp, the shell tests' mock_pcp.cpp and
// the two pcp_place_coverage_weighted entry points below, which record what they were given and
// return the answers a case has set.  The program checks the marshalling, the box list -> bytes
// rule with its override order, the rounds in weight and in points, the blind weight, the log text
// and the refusal paths itself and ends with status 0 and "cover_weight_host_selftest ok" only if
// every check held.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcp_cover_weight_node.hpp"

using namespace pcp;
using Opt = SimplifiedDualLidarOptimizer;
using Weighted = WeightedCoveragePlacement;

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
    std::vector<uint64_t> gain, cov, gpts;
    uint64_t n_points = 0, roi_points = 0, roi_weight = 0, base_covered = 0, base_points = 0;
    std::vector<int32_t> owner;
    std::vector<uint32_t> seen;
};
struct Seen {
    int calls = 0;
    bool mounted = false, ctx_ok = false;
    std::vector<double> poses, el_table;
    bool el_null = true, weight_null = true, rg_null = true, seen_null = true, gp_null = true,
         owner_null = true;
    uint64_t n = 0, weight_n = 0, owner_cap = 0;
    pcp_fan_params fan{};
    pcp_cover_params cp{};
    std::vector<uint8_t> weight;
};
static Canned g;
static Seen s;
static pcp_ctx *g_ctx = nullptr;

static int record(bool mounted, pcp_ctx *ctx, const double *poses, uint64_t n,
                  const pcp_fan_params *fan, const double *el_table, const pcp_cover_params *cp,
                  const uint8_t *weight, uint64_t weight_n, int64_t *selected, uint64_t *gain,
                  uint64_t *covered_after, uint64_t *gain_points, int64_t *round_gains,
                  uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap,
                  uint64_t *n_points, uint64_t *roi_points, uint64_t *roi_weight,
                  uint64_t *base_covered, uint64_t *base_points, int32_t *n_selected) {
    ++s.calls;
    s.mounted = mounted;
    s.ctx_ok = ctx == g_ctx;
    s.n = n;
    if (n) s.poses.assign(poses, poses + (mounted ? 6 : 5) * n);
    s.fan = *fan;
    s.el_null = el_table == nullptr;
    if (el_table) s.el_table.assign(el_table, el_table + fan->n_el);
    s.cp = *cp;
    s.weight_null = weight == nullptr;
    s.weight_n = weight_n;
    if (weight) s.weight.assign(weight, weight + weight_n);
    s.rg_null = round_gains == nullptr;
    s.seen_null = seen_points == nullptr;
    s.gp_null = gain_points == nullptr;
    s.owner_null = point_owner == nullptr;
    s.owner_cap = owner_cap;
    if (g.rc != PCP_OK) {   // (an error is left in the context by a call that always fails)
        pcp_crop_voxel(ctx, nullptr, nullptr, 0.f, nullptr, 0, nullptr, nullptr);
        return g.rc;
    }
    for (int32_t i = 0; i < g.ns; ++i) {
        selected[i] = g.sel[(size_t)i];
        gain[i] = g.gain[(size_t)i];
        covered_after[i] = g.cov[(size_t)i];
        if (gain_points) gain_points[i] = g.gpts[(size_t)i];
    }
    for (size_t i = 0; i < g.seen.size() && seen_points; ++i) seen_points[i] = g.seen[i];
    for (size_t i = 0; i < g.owner.size() && point_owner && i < owner_cap; ++i)
        point_owner[i] = g.owner[i];
    *n_points = g.n_points;
    *roi_points = g.roi_points;
    *roi_weight = g.roi_weight;
    *base_covered = g.base_covered;
    *base_points = g.base_points;
    *n_selected = g.ns;
    return PCP_OK;
}

extern "C" {
int pcp_place_coverage_weighted(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                const pcp_fan_params *fan, const pcp_cover_params *cp,
                                const uint8_t *weight, uint64_t weight_n, int64_t *selected,
                                uint64_t *gain, uint64_t *covered_after, uint64_t *gain_points,
                                int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                                uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                                uint64_t *roi_weight, uint64_t *base_covered,
                                uint64_t *base_points, int32_t *n_selected) {
    return record(false, ctx, poses5, n, fan, nullptr, cp, weight, weight_n, selected, gain,
                  covered_after, gain_points, round_gains, seen_points, point_owner, owner_cap,
                  n_points, roi_points, roi_weight, base_covered, base_points, n_selected);
}
int pcp_place_coverage_weighted_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                        const pcp_fan_params *fan, const double *el_table,
                                        const pcp_cover_params *cp, const uint8_t *weight,
                                        uint64_t weight_n, int64_t *selected, uint64_t *gain,
                                        uint64_t *covered_after, uint64_t *gain_points,
                                        int64_t *round_gains, uint32_t *seen_points,
                                        int32_t *point_owner, uint64_t owner_cap,
                                        uint64_t *n_points, uint64_t *roi_points,
                                        uint64_t *roi_weight, uint64_t *base_covered,
                                        uint64_t *base_points, int32_t *n_selected) {
    return record(true, ctx, poses6, n, fan, el_table, cp, weight, weight_n, selected, gain,
                  covered_after, gain_points, round_gains, seen_points, point_owner, owner_cap,
                  n_points, roi_points, roi_weight, base_covered, base_points, n_selected);
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

static CoverageWeightBox wbox(double x0, double x1, double y0, double y1, double z0, double z1,
                              uint8_t w) {
    CoverageWeightBox b;
    b.box = CoverageBox{x0, x1, y0, y1, z0, z1};
    b.weight = w;
    return b;
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
    Weighted::Params base;
    base.num_mobile_lidars = 3;
    base.min_separation = 2.5;

    // ---- the box list -> bytes rule -------------------------------------------------------------
    {
        std::vector<uint8_t> w;
        std::string why;
        // no box: the base weight everywhere, the non-finite point included
        CHECK(coverage_weight_bytes(terrain, 3, {}, w, &why));
        CHECK(w == (std::vector<uint8_t>{3, 3, 3, 3, 3, 3}));
        // a box holds points 0, 1, 3, 5 (bounds included: x = 0 and y = -1 lie on them); a later
        // box overrides it on points 1 and 5; a box that holds no point changes nothing
        const std::vector<CoverageWeightBox> list = {
            wbox(0.0, 1.5, -1.0, 0.5, 0.0, 0.5, 200), wbox(0.9, 1.6, 0.4, 0.6, 0.2, 0.6, 7),
            wbox(10.0, 11.0, 10.0, 11.0, 0.0, 1.0, 99)};
        CHECK(coverage_weight_bytes(terrain, 1, list, w, &why));
        CHECK(w == (std::vector<uint8_t>{200, 7, 1, 200, 1, 7}));
        // the order decides: the same two boxes the other way round
        CHECK(coverage_weight_bytes(terrain, 1, {list[1], list[0]}, w, &why));
        CHECK(w == (std::vector<uint8_t>{200, 200, 1, 200, 1, 200}));
        // a box of weight 0 takes its points out of the region; base 0 leaves the boxes alone
        CHECK(coverage_weight_bytes(terrain, 0, {list[0], wbox(0.9, 1.1, -1.1, -0.9, -0.1, 0.1, 0)},
                                    w, &why));
        CHECK(w == (std::vector<uint8_t>{200, 200, 0, 0, 0, 200}));
        // a message without x, y, z
        PointCloud2 bad = terrain;
        bad.fields.erase(bad.fields.begin());
        CHECK(!coverage_weight_bytes(bad, 1, {}, w, &why) && !why.empty());
    }

    // ---- a level call with a fixed candidate and a box list -------------------------------------
    {
        Weighted wpl(base);
        g = Canned{};
        g.ns = 2;
        g.sel = {3, 0};
        g.gain = {14, 200};
        g.gpts = {2, 1};
        g.cov = {214, 414};
        g.n_points = 6;
        g.roi_points = 6;
        g.roi_weight = 416;
        g.base_covered = 200;
        g.base_points = 1;
        g.owner = {2, 1, PCP_OWNER_NONE, 0, PCP_OWNER_NONE, 1};
        g.seen = {5, 0, 9, 4};
        s = Seen{};
        const Weighted::Weights weights(
            1, {wbox(0.0, 1.5, -1.0, 0.5, 0.0, 0.5, 200), wbox(0.9, 1.6, 0.4, 0.6, 0.2, 0.6, 7)});
        const auto r = wpl.place(dev, terrain, cand, fan, weights, {1});
        CHECK(r.ran && wpl.lastError().empty());
        CHECK(s.calls == 1 && !s.mounted && s.ctx_ok && s.n == 4);
        const double want[10] = {0.0, 0.0, 1.125, -0.5, 0.0, 1.5, -0.25, 1.125, -0.5, 0.75};
        CHECK(s.poses.size() == 20 && std::vector<double>(s.poses.begin(), s.poses.begin() + 10) ==
                                          std::vector<double>(want, want + 10));
        CHECK(s.fan.n_az == 64 && s.fan.n_el == 4 && s.fan.max_distance == 12.0);
        CHECK(s.fan.el_min == fan.el_min && s.fan.el_max == fan.el_max);
        CHECK(s.cp.k_max == 3 && s.cp.n_fixed == 1 && s.cp.min_separation == 2.5);
        CHECK(s.cp.reserved[0] == 0 && s.cp.reserved[1] == 0 && s.cp.fixed[0] == 1);
        for (int i = 1; i < PCP_PLACE_MAX; ++i) CHECK(s.cp.fixed[i] == 0);
        CHECK(!s.weight_null && s.weight_n == 6 &&
              s.weight == (std::vector<uint8_t>{200, 7, 1, 200, 1, 7}));
        CHECK(s.rg_null && !s.seen_null && !s.gp_null && !s.owner_null && s.owner_cap == 6);
        // the answer: rounds in weight, the points beside them
        CHECK(r.rounds.size() == 2 && r.gain_points == (std::vector<uint64_t>{2, 1}));
        CHECK(r.placed.size() == 2 && r.placed_mounts.empty());
        CHECK(r.rounds[0].candidate == 3 && r.rounds[0].gain == 14 && r.rounds[0].covered == 214);
        CHECK(r.rounds[0].coverage_ratio == 214.0 / 416.0);
        CHECK(r.rounds[1].candidate == 0 && r.rounds[1].gain == 200 && r.rounds[1].covered == 414);
        CHECK(r.placed[0].x == 4.5 && r.placed[0].total_score == 214.0 && r.placed[1].x == 0.0);
        CHECK(r.n_fixed == 1 && r.n_points == 6 && r.roi_points == 6 && r.roi_weight == 416);
        CHECK(r.base_covered == 200 && r.base_points == 1);
        CHECK(r.seen_points == (std::vector<uint32_t>{5, 0, 9, 4}) && r.point_owner == g.owner);
        CHECK(r.weight == s.weight);
        // the blind spots: a weight and no owner -- points 2 and 4 (the non-finite one has the
        // base weight), the records whole; their weight from the bytes
        const PointCloud2 &b = r.blind_spots;
        CHECK(b.width == 2 && b.point_step == 20 && b.row_step == 40 && b.data.size() == 40);
        CHECK(b.frame_id == "map" && b.stamp == 7.25 && b.fields.size() == 4);
        CHECK(tag_of(b, 0) == 102 && tag_of(b, 1) == 104);
        CHECK(std::memcmp(b.data.data(), terrain.data.data() + 40, 20) == 0);
        CHECK(r.blind_points == 2 && r.blind_weight == 2);
        const std::string want_log =
            "========================================\n"
            "Weighted Coverage Placement (1 Fixed + 2 Mobile)\n"
            "========================================\n"
            "Terrain points in region: 6 of 6, weight 416\n"
            "  Covered by fixed sensors: weight 200 (48.1%), 1 points\n"
            "----------------------------------------\n"
            "Mobile LiDAR 1 Position: (4.50, -0.75, 1.12)  [candidate 3]\n"
            "  Weight gained: 14 (2 points)\n"
            "  Covered weight: 214 of 416 (51.4%)\n"
            "----------------------------------------\n"
            "Mobile LiDAR 2 Position: (0.00, 0.00, 1.12)  [candidate 0]\n"
            "  Weight gained: 200 (1 points)\n"
            "  Covered weight: 414 of 416 (99.5%)\n"
            "----------------------------------------\n"
            "Blind spots: 2 of 6 points, weight 2 of 416 (0.5%)\n"
            "========================================\n";
        if (r.log != want_log) std::printf("log:\n%s", r.log.c_str());
        CHECK(r.log == want_log && weighted_coverage_log(r) == want_log);
    }

    // ---- mounted, a beam table, bytes with zeros -------------------------------------------------
    {
        Weighted::Params p = base;
        p.min_separation = 0.0;
        p.num_mobile_lidars = 1;
        Weighted wpl(p);
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
        g.gain = {300};
        g.gpts = {3};
        g.cov = {300};
        g.n_points = 6;
        g.roi_points = 4;
        g.roi_weight = 555;
        g.owner = {0, 0, PCP_OWNER_NONE, 0, PCP_OWNER_NONE, PCP_OWNER_NONE};
        g.seen = {3, 4};
        s = Seen{};
        const std::vector<uint8_t> bytes = {100, 100, 0, 100, 0, 255};
        const auto r = wpl.place_mounted(dev, terrain, mounts, mf, Weighted::Weights(bytes));
        CHECK(r.ran && s.calls == 1 && s.mounted && s.n == 2 && s.weight == bytes);
        const double want[12] = {1.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, -2.0, 0.5, 0.0, -0.125, 3.0};
        CHECK(s.poses == std::vector<double>(want, want + 12));
        CHECK(!s.el_null && s.el_table == mf.el_table);
        CHECK(s.cp.k_max == 1 && s.cp.n_fixed == 0 && s.cp.min_separation == 0.0);
        CHECK(r.rounds.size() == 1 && r.rounds[0].candidate == 1 && r.gain_points[0] == 3);
        CHECK(r.placed.empty() && r.placed_mounts.size() == 1 && r.placed_mounts[0].yaw == 3.0);
        // points 2 and 4 weigh nothing: not blind; point 5 is
        CHECK(r.blind_spots.width == 1 && tag_of(r.blind_spots, 0) == 105);
        CHECK(r.blind_points == 1 && r.blind_weight == 255);
        CHECK(r.log.find("Weighted Coverage Placement (0 Fixed + 1 Mobile)") != std::string::npos);
        CHECK(r.log.find("Terrain points in region: 4 of 6, weight 555\n") != std::string::npos);
        CHECK(r.log.find("Blind spots: 1 of 4 points, weight 255 of 555 (45.9%)") !=
              std::string::npos);
        // without a table the call gets none
        s = Seen{};
        mf.el_table.clear();
        CHECK(wpl.place_mounted(dev, terrain, mounts, mf, Weighted::Weights(bytes)).ran &&
              s.el_null);
    }

    // ---- the default weights: every point 1; nothing adds anything; no candidates ---------------
    {
        Weighted wpl(base);
        g = Canned{};
        g.n_points = 6;
        g.roi_points = 6;
        g.roi_weight = 6;
        g.owner.assign(6, PCP_OWNER_NONE);
        s = Seen{};
        const auto r = wpl.place(dev, terrain, cand, fan);
        CHECK(r.ran && r.rounds.empty() && r.gain_points.empty() && r.blind_spots.width == 6);
        CHECK(s.weight == std::vector<uint8_t>(6, 1) && r.blind_weight == 6);
        const auto e = wpl.place(dev, terrain, {}, fan);
        CHECK(e.ran && e.seen_points.empty() && s.n == 0 && !s.weight_null);
        // no terrain points: the call still gets an address
        PointCloud2 empty = terrain;
        empty.width = 0;
        empty.row_step = 0;
        empty.data.clear();
        g = Canned{};
        s = Seen{};
        const auto z = wpl.place(dev, empty, cand, fan);
        CHECK(z.ran && s.calls == 1 && !s.weight_null && s.weight_n == 0 && z.point_owner.empty());
        CHECK(z.blind_points == 0 && z.blind_weight == 0);
    }

    // ---- refusals -------------------------------------------------------------------------------
    {
        Weighted wpl(base);
        s = Seen{};
        VirtualScan::Params bad = fan;
        bad.n_az = 0;
        CHECK(!wpl.place(dev, terrain, cand, bad).ran && !wpl.lastError().empty());
        std::vector<int64_t> many(PCP_PLACE_MAX + 1, 0);
        CHECK(!wpl.place(dev, terrain, cand, fan, Weighted::Weights(), many).ran &&
              !wpl.lastError().empty());
        CHECK(!wpl.place(dev, terrain, cand, fan, Weighted::Weights(std::vector<uint8_t>(5, 1))).ran);
        CHECK(wpl.lastError().find("one byte per terrain point") != std::string::npos);
        std::vector<VirtualScan::SensorPose> mounts(1);
        bad = fan;
        bad.el_table = {0.0, 0.1};
        CHECK(!wpl.place_mounted(dev, terrain, mounts, bad).ran);
        PointCloud2 nox = terrain;
        nox.fields.erase(nox.fields.begin());
        CHECK(!wpl.place(dev, nox, cand, fan).ran && !wpl.lastError().empty());
        CHECK(s.calls == 0);
        // the library refuses: its message is passed on
        g = Canned{};
        g.rc = PCP_E_INVALID;
        const auto r = wpl.place(dev, terrain, cand, fan);
        CHECK(!r.ran && s.calls == 1 && !wpl.lastError().empty() && r.rounds.empty());
        // a terrain message that is not the index's cloud
        g = Canned{};
        g.n_points = 7;
        CHECK(!wpl.place(dev, terrain, cand, fan).ran && !wpl.lastError().empty());
        // and a good call clears the error
        g.n_points = 6;
        g.owner.assign(6, PCP_OWNER_NONE);
        CHECK(wpl.place(dev, terrain, cand, fan).ran && wpl.lastError().empty());
    }

    if (g_fail) {
        std::printf("cover_weight_host_selftest: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("cover_weight_host_selftest ok\n");
    return 0;
}
