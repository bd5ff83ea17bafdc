// pcp_placement.cpp -- MobileLidarPlacement: see pcp_placement.hpp
#include "pcp_placement.hpp"

#include <cstdarg>
#include <cstdio>

namespace pcp {

static void appendf(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void appendf(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
    s += '\n';
}

std::string placement_log(const MobileLidarPlacement::Result &r) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Multi LiDAR Placement (ZX120 + %zu Mobile)", r.placed.size());
    appendf(log, "%s", rule);
    appendf(log, "Total Score (ZX120 only): %.2f", r.zx120_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.zx120_covered, tc, pct(r.zx120_covered));
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const auto &p = r.placed[i];
        appendf(log, "%s", thin);
        appendf(log, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, p.x,
                p.y, p.z, (long long)q.candidate);
        appendf(log, "  Total Score: %.2f (gain %.2f)", q.total, q.gain);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", q.covered, tc, pct(q.covered));
    }
    appendf(log, "%s", rule);
    return log;
}

MobileLidarPlacement::Result MobileLidarPlacement::place(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl) {
    Result r;
    err_.clear();
    if (!tick.ran) return r;
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
    const pcp_place_params pp{p_.num_mobile_lidars, 0, p_.min_separation};
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    int64_t sel[PCP_PLACE_MAX];
    double tot[PCP_PLACE_MAX];
    int32_t cov[PCP_PLACE_MAX], ns = 0;
    if (pcp_place_sensors(dev.ctx(), poses.data(), n, zx, &p, &pp, sel, tot, cov, nullptr, nullptr,
                          nullptr, &r.zx120_total, &r.zx120_covered, &ns) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.total_cells = tick.report.total_cells;
    double before = r.zx120_total;
    for (int32_t i = 0; i < ns; ++i) {
        Round q;
        q.candidate = sel[i];
        q.total = tot[i];
        q.gain = tot[i] - before;
        q.covered = cov[i];
        q.coverage_ratio = r.total_cells > 0 ? (double)cov[i] / r.total_cells : 0.0;
        before = tot[i];
        r.rounds.push_back(q);
        r.placed.push_back(tick.candidates[(size_t)sel[i]]);
        r.placed.back().total_score = tot[i];
    }
    r.log = placement_log(r);
    return r;
}

}  // namespace pcp
