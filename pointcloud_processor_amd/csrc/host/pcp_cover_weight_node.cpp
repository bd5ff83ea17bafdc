// pcp_cover_weight_node.cpp -- WeightedCoveragePlacement: see pcp_cover_weight_node.hpp.  The only
// unit above the C ABI that references pcp_place_coverage_weighted.
#include "pcp_cover_weight_node.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace pcp {

bool coverage_weight_bytes(const PointCloud2 &terrain, uint8_t base,
                           const std::vector<CoverageWeightBox> &boxes,
                           std::vector<uint8_t> &weight, std::string *why) {
    pcp_cloud_view v{};
    if (!cloud_view(terrain, v, why)) return false;
    weight.assign(v.n, base);
    const uint8_t *data = static_cast<const uint8_t *>(v.data);
    for (uint64_t i = 0; i < v.n; ++i) {
        float p[3];
        const uint8_t *rec = data + i * v.point_step;
        std::memcpy(&p[0], rec + v.off_x, 4);
        std::memcpy(&p[1], rec + v.off_y, 4);
        std::memcpy(&p[2], rec + v.off_z, 4);
        // in list order, so the last box that holds the point decides (a NaN fails every
        // comparison, an infinity lies outside every finite box: the base weight stays)
        for (const CoverageWeightBox &b : boxes)
            if ((double)p[0] >= b.box.x0 && (double)p[0] <= b.box.x1 && (double)p[1] >= b.box.y0 &&
                (double)p[1] <= b.box.y1 && (double)p[2] >= b.box.z0 && (double)p[2] <= b.box.z1)
                weight[i] = b.weight;
    }
    return true;
}

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

std::string weighted_coverage_log(const WeightedCoveragePlacement::Result &r) {
    static const char *rule = "========================================";
    static const char *thin = "----------------------------------------";
    std::string s;
    line(s, "%s", rule);
    line(s, "Weighted Coverage Placement (%d Fixed + %zu Mobile)", r.n_fixed, r.rounds.size());
    line(s, "%s", rule);
    line(s, "Terrain points in region: %llu of %llu, weight %llu", (unsigned long long)r.roi_points,
         (unsigned long long)r.n_points, (unsigned long long)r.roi_weight);
    line(s, "  Covered by fixed sensors: weight %llu (%.1f%%), %llu points",
         (unsigned long long)r.base_covered, pct(r.base_covered, r.roi_weight),
         (unsigned long long)r.base_points);
    const bool mounted = !r.placed_mounts.empty();
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const double x = mounted ? r.placed_mounts[i].x : r.placed[i].x;
        const double y = mounted ? r.placed_mounts[i].y : r.placed[i].y;
        const double z = mounted ? r.placed_mounts[i].z : r.placed[i].z;
        line(s, "%s", thin);
        line(s, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, x, y, z,
             (long long)q.candidate);
        line(s, "  Weight gained: %llu (%llu points)", (unsigned long long)q.gain,
             (unsigned long long)r.gain_points[i]);
        line(s, "  Covered weight: %llu of %llu (%.1f%%)", (unsigned long long)q.covered,
             (unsigned long long)r.roi_weight, q.coverage_ratio * 100.0);
    }
    line(s, "%s", thin);
    line(s, "Blind spots: %llu of %llu points, weight %llu of %llu (%.1f%%)",
         (unsigned long long)r.blind_points, (unsigned long long)r.roi_points,
         (unsigned long long)r.blind_weight, (unsigned long long)r.roi_weight,
         pct(r.blind_weight, r.roi_weight));
    line(s, "%s", rule);
    return s;
}

WeightedCoveragePlacement::Result WeightedCoveragePlacement::place(
    Device &dev, const PointCloud2 &terrain,
    const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
    const VirtualScan::Params &fan, const Weights &weights, const std::vector<int64_t> &fixed) {
    const size_t n = candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = candidates[i];
        const double row[5] = {c.x, c.y, c.z, c.pitch, c.yaw};
        std::memcpy(poses.data() + 5 * i, row, sizeof row);
    }
    Result r = run(dev, terrain, poses, n, false, fan, weights, fixed);
    for (const CoveragePlacement::Round &q : r.rounds) {
        auto p = candidates[(size_t)q.candidate];
        p.total_score = (double)q.covered;
        r.placed.push_back(p);
    }
    if (r.ran) r.log = weighted_coverage_log(r);
    return r;
}

WeightedCoveragePlacement::Result WeightedCoveragePlacement::place_mounted(
    Device &dev, const PointCloud2 &terrain, const std::vector<VirtualScan::SensorPose> &candidates,
    const VirtualScan::Params &fan, const Weights &weights, const std::vector<int64_t> &fixed) {
    const size_t n = candidates.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const VirtualScan::SensorPose &c = candidates[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    Result r = run(dev, terrain, poses, n, true, fan, weights, fixed);
    for (const CoveragePlacement::Round &q : r.rounds)
        r.placed_mounts.push_back(candidates[(size_t)q.candidate]);
    if (r.ran) r.log = weighted_coverage_log(r);
    return r;
}

WeightedCoveragePlacement::Result WeightedCoveragePlacement::run(
    Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
    bool mounted, const VirtualScan::Params &fp, const Weights &weights,
    const std::vector<int64_t> &fixed) {
    Result r;
    // the fan, the candidates' count, the fixed list's length and the beam table:
    // CoveragePlacement's own checks (the region is the weights', below)
    CoveragePlacement base;
    std::vector<uint8_t> unused;
    const std::vector<uint8_t> *all = nullptr;
    if (!base.region(terrain, n, mounted, fp, fixed, CoverageRoi(), unused, all)) {
        err_ = base.lastError();
        return r;
    }
    err_.clear();
    const size_t np = terrain.size();
    if (weights.kind == Weights::Bytes) {
        r.weight = weights.bytes;
    } else {
        std::string why;
        if (!coverage_weight_bytes(terrain, weights.base, weights.boxes, r.weight, &why)) {
            err_ = "WeightedCoveragePlacement: " + why;
            return r;
        }
    }
    if (r.weight.size() != np) {
        err_ = "WeightedCoveragePlacement: the weights do not hold one byte per terrain point";
        r.weight.clear();
        return r;
    }
    const bool table = mounted && !fp.el_table.empty();
    const pcp_fan_params fan{fp.n_az, fp.n_el, fp.el_min, fp.el_max, fp.max_distance};
    pcp_cover_params cp{};
    cp.k_max = p_.num_mobile_lidars;
    cp.n_fixed = (int32_t)fixed.size();
    cp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) cp.fixed[i] = fixed[i];
    int64_t sel[PCP_PLACE_MAX];
    uint64_t gain[PCP_PLACE_MAX], cov[PCP_PLACE_MAX], gpts[PCP_PLACE_MAX];
    int32_t ns = 0;
    r.seen_points.assign(n ? n : 1, 0);
    r.point_owner.assign(np ? np : 1, PCP_OWNER_NONE);
    // (the call wants an address even for no points)
    const uint8_t none = 0;
    const uint8_t *w_p = np ? r.weight.data() : &none;
    const int rc =
        mounted ? pcp_place_coverage_weighted_mounted(
                      dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                      table ? fp.el_table.data() : nullptr, &cp, w_p, np, sel, gain, cov, gpts,
                      nullptr, r.seen_points.data(), r.point_owner.data(), np, &r.n_points,
                      &r.roi_points, &r.roi_weight, &r.base_covered, &r.base_points, &ns)
                : pcp_place_coverage_weighted(dev.ctx(), n ? poses.data() : nullptr, n, &fan, &cp,
                                              w_p, np, sel, gain, cov, gpts, nullptr,
                                              r.seen_points.data(), r.point_owner.data(), np,
                                              &r.n_points, &r.roi_points, &r.roi_weight,
                                              &r.base_covered, &r.base_points, &ns);
    if (rc != PCP_OK) {
        err_ = dev.error();
        if (err_.empty()) err_ = "WeightedCoveragePlacement: pcp_place_coverage_weighted failed";
        return r;
    }
    if (r.n_points != np) {
        err_ = "WeightedCoveragePlacement: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.seen_points.resize(n);
    r.point_owner.resize(np);
    r.n_fixed = cp.n_fixed;
    for (int32_t i = 0; i < ns; ++i) {
        CoveragePlacement::Round q;
        q.candidate = sel[i];
        q.gain = gain[i];
        q.covered = cov[i];
        q.coverage_ratio = r.roi_weight ? (double)cov[i] / (double)r.roi_weight : 0.0;
        r.rounds.push_back(q);
        r.gain_points.push_back(gpts[i]);
    }
    // the blind spots: a weight and no owner; their weight from the bytes, not from the counts
    CoveragePlacement::blind_spots(r, terrain, &r.weight);
    r.blind_points = r.blind_spots.width;
    for (size_t i = 0; i < np; ++i)
        if (r.point_owner[i] == PCP_OWNER_NONE) r.blind_weight += r.weight[i];
    r.ran = true;
    return r;
}

}  // namespace pcp
