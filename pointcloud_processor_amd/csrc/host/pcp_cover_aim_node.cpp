// pcp_cover_aim_node.cpp -- AimedCoveragePlacement: see pcp_cover_aim_node.hpp.  The only unit
// above the C ABI that references pcp_place_coverage_aimed.
#include "pcp_cover_aim_node.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace pcp {

namespace {
__attribute__((format(printf, 2, 3))) void line(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
    s += '\n';
}
double pct(uint64_t a, uint64_t b) { return b ? (double)a / (double)b * 100.0 : 0.0; }
}  // namespace

std::string aimed_coverage_log(const AimedCoveragePlacement::Result &r) {
    static const char *rule = "========================================";
    static const char *thin = "----------------------------------------";
    std::string s;
    line(s, "%s", rule);
    line(s, "Aimed Coverage Placement (%d Fixed + %zu Mobile)", r.n_fixed, r.rounds.size());
    line(s, "%s", rule);
    line(s, "Window: %d columns x %d rings, %zu aims per candidate", r.w_az, r.w_el, r.aims.size());
    line(s, "Terrain points in region: %llu of %llu", (unsigned long long)r.roi_points,
         (unsigned long long)r.n_points);
    line(s, "  Covered by fixed sensors: %llu (%.1f%%)", (unsigned long long)r.base_covered,
         pct(r.base_covered, r.roi_points));
    const bool mounted = !r.placed_mounts.empty();
    uint64_t covered = r.base_covered;
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const double x = mounted ? r.placed_mounts[i].x : r.placed[i].x;
        const double y = mounted ? r.placed_mounts[i].y : r.placed[i].y;
        const double z = mounted ? r.placed_mounts[i].z : r.placed[i].z;
        const AimedCoveragePlacement::Aim a = r.aims[(size_t)r.aim[i]];
        line(s, "%s", thin);
        line(s, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, x, y, z,
             (long long)q.candidate);
        line(s, "  Aim %d: columns from %d, rings from %d", r.aim[i], a.az0, a.el0);
        line(s, "  Points gained: %llu", (unsigned long long)q.gain);
        line(s, "  Covered points: %llu of %llu (%.1f%%)", (unsigned long long)q.covered,
             (unsigned long long)r.roi_points, q.coverage_ratio * 100.0);
        covered = q.covered;
    }
    line(s, "%s", thin);
    line(s, "Blind spots: %llu of %llu (%.1f%%)", (unsigned long long)(r.roi_points - covered),
         (unsigned long long)r.roi_points, pct(r.roi_points - covered, r.roi_points));
    line(s, "%s", rule);
    return s;
}

AimedCoveragePlacement::Result AimedCoveragePlacement::place(
    Device &dev, const PointCloud2 &terrain,
    const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
    const VirtualScan::Params &fan, const std::vector<Fixed> &fixed, const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = candidates[i];
        const double row[5] = {c.x, c.y, c.z, c.pitch, c.yaw};
        std::memcpy(poses.data() + 5 * i, row, sizeof row);
    }
    Result r = run(dev, terrain, poses, n, false, fan, fixed, roi);
    for (const CoveragePlacement::Round &q : r.rounds) {
        auto p = candidates[(size_t)q.candidate];
        p.total_score = (double)q.covered;
        r.placed.push_back(p);
    }
    if (r.ran) r.log = aimed_coverage_log(r);
    return r;
}

AimedCoveragePlacement::Result AimedCoveragePlacement::place_mounted(
    Device &dev, const PointCloud2 &terrain, const std::vector<VirtualScan::SensorPose> &candidates,
    const VirtualScan::Params &fan, const std::vector<Fixed> &fixed, const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const VirtualScan::SensorPose &c = candidates[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    Result r = run(dev, terrain, poses, n, true, fan, fixed, roi);
    for (const CoveragePlacement::Round &q : r.rounds)
        r.placed_mounts.push_back(candidates[(size_t)q.candidate]);
    if (r.ran) r.log = aimed_coverage_log(r);
    return r;
}

AimedCoveragePlacement::Result AimedCoveragePlacement::run(
    Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
    bool mounted, const VirtualScan::Params &fp, const std::vector<Fixed> &fixed, const Roi &roi) {
    Result r;
    // the fan, the candidates' count, the fixed list's length, the beam table and the region:
    // CoveragePlacement's own checks and bytes
    CoveragePlacement base;
    std::vector<int64_t> fixed_idx;
    for (const Fixed &f : fixed) fixed_idx.push_back(f.candidate);
    std::vector<uint8_t> box_bytes;
    const std::vector<uint8_t> *bytes = nullptr;
    if (!base.region(terrain, n, mounted, fp, fixed_idx, roi, box_bytes, bytes)) {
        err_ = base.lastError();
        return r;
    }
    err_.clear();
    if (p_.aims.empty() || p_.aims.size() > PCP_COVER_AIM_MAX) {
        err_ = "AimedCoveragePlacement: the aim table holds 1 .. PCP_COVER_AIM_MAX aims";
        return r;
    }
    const bool table = mounted && !fp.el_table.empty();
    const size_t np = terrain.size();
    const size_t A = p_.aims.size();
    const pcp_fan_params fan{fp.n_az, fp.n_el, fp.el_min, fp.el_max, fp.max_distance};
    pcp_cover_aim_params ap{};
    ap.k_max = p_.num_mobile_lidars;
    ap.n_aims = (int32_t)A;
    ap.n_fixed = (int32_t)fixed.size();
    ap.w_az = p_.w_az;
    ap.w_el = p_.w_el;
    ap.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) {
        ap.fixed_pose[i] = fixed[i].candidate;
        ap.fixed_aim[i] = fixed[i].aim;
    }
    std::vector<int32_t> aims(2 * A);
    for (size_t a = 0; a < A; ++a) {
        aims[2 * a] = p_.aims[a].az0;
        aims[2 * a + 1] = p_.aims[a].el0;
    }
    int64_t sel[PCP_PLACE_MAX];
    int32_t sel_aim[PCP_PLACE_MAX];
    uint64_t gain[PCP_PLACE_MAX], cov[PCP_PLACE_MAX];
    int32_t ns = 0;
    r.seen_points.assign(n ? n : 1, 0);
    r.aim_points.assign(n ? n * A : 1, 0);
    r.point_owner.assign(np ? np : 1, PCP_OWNER_NONE);
    const uint8_t *roi_p = bytes ? bytes->data() : nullptr;
    const int rc =
        mounted ? pcp_place_coverage_aimed_mounted(
                      dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                      table ? fp.el_table.data() : nullptr, &ap, aims.data(), roi_p, np, sel,
                      sel_aim, gain, cov, nullptr, r.seen_points.data(), r.aim_points.data(),
                      r.point_owner.data(), np, &r.n_points, &r.roi_points, &r.base_covered, &ns)
                : pcp_place_coverage_aimed(dev.ctx(), n ? poses.data() : nullptr, n, &fan, &ap,
                                           aims.data(), roi_p, np, sel, sel_aim, gain, cov, nullptr,
                                           r.seen_points.data(), r.aim_points.data(),
                                           r.point_owner.data(), np, &r.n_points, &r.roi_points,
                                           &r.base_covered, &ns);
    if (rc != PCP_OK) {
        err_ = dev.error();
        if (err_.empty()) err_ = "AimedCoveragePlacement: pcp_place_coverage_aimed failed";
        return r;
    }
    if (r.n_points != np) {
        err_ = "AimedCoveragePlacement: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.seen_points.resize(n);
    r.aim_points.resize(n * A);
    r.point_owner.resize(np);
    r.n_fixed = ap.n_fixed;
    r.aims = p_.aims;
    r.w_az = p_.w_az;
    r.w_el = p_.w_el;
    for (int32_t i = 0; i < ns; ++i) {
        CoveragePlacement::Round q;
        q.candidate = sel[i];
        q.gain = gain[i];
        q.covered = cov[i];
        q.coverage_ratio = r.roi_points ? (double)cov[i] / (double)r.roi_points : 0.0;
        r.rounds.push_back(q);
        r.aim.push_back(sel_aim[i]);
    }
    CoveragePlacement::blind_spots(r, terrain, bytes);
    r.ran = true;
    return r;
}

}  // namespace pcp
