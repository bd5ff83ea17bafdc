// pcp_cover_pair_node.cpp -- CoveragePlacement::place_pair / place_pair_mounted: see
// pcp_cover_node.hpp.  The only unit above the C ABI that references pcp_place_coverage_pair.
#include <cstring>

#include "pcp_cover_node.hpp"

namespace pcp {

CoveragePlacement::Result CoveragePlacement::place_pair(
    Device &dev, const PointCloud2 &terrain,
    const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
    const VirtualScan::Params &fan, const std::vector<int64_t> &fixed, const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = candidates[i];
        const double row[5] = {c.x, c.y, c.z, c.pitch, c.yaw};
        std::memcpy(poses.data() + 5 * i, row, sizeof row);
    }
    Result r = run_pair(dev, terrain, poses, n, false, fan, fixed, roi);
    for (const Round &q : r.rounds) {
        auto p = candidates[(size_t)q.candidate];
        p.total_score = (double)q.covered;
        r.placed.push_back(p);
    }
    if (r.ran) r.log = coverage_log(r);
    return r;
}

CoveragePlacement::Result CoveragePlacement::place_pair_mounted(
    Device &dev, const PointCloud2 &terrain, const std::vector<VirtualScan::SensorPose> &candidates,
    const VirtualScan::Params &fan, const std::vector<int64_t> &fixed, const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const VirtualScan::SensorPose &c = candidates[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    Result r = run_pair(dev, terrain, poses, n, true, fan, fixed, roi);
    for (const Round &q : r.rounds) r.placed_mounts.push_back(candidates[(size_t)q.candidate]);
    if (r.ran) r.log = coverage_log(r);
    return r;
}

CoveragePlacement::Result CoveragePlacement::run_pair(Device &dev, const PointCloud2 &terrain,
                                                      const std::vector<double> &poses, size_t n,
                                                      bool mounted, const VirtualScan::Params &fp,
                                                      const std::vector<int64_t> &fixed,
                                                      const Roi &roi) {
    Result r;
    std::vector<uint8_t> box_bytes;
    const std::vector<uint8_t> *bytes = nullptr;
    if (!region(terrain, n, mounted, fp, fixed, roi, box_bytes, bytes)) return r;
    const bool table = mounted && !fp.el_table.empty();
    const size_t np = terrain.size();
    const pcp_fan_params fan{fp.n_az, fp.n_el, fp.el_min, fp.el_max, fp.max_distance};
    pcp_pair_params pp{};
    pp.n_fixed = (int32_t)fixed.size();
    pp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) pp.fixed[i] = fixed[i];
    int32_t ns = 0;
    r.seen_points.assign(n ? n : 1, 0);
    r.point_owner.assign(np ? np : 1, PCP_OWNER_NONE);
    std::vector<int64_t> singles(n ? n : 1, -1);
    const uint8_t *roi_p = bytes ? bytes->data() : nullptr;
    const int rc =
        mounted ? pcp_place_coverage_pair_mounted(
                      dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                      table ? fp.el_table.data() : nullptr, &pp, roi_p, np, r.best_pair,
                      &r.pair_gain, &r.best_single, &r.single_gain, singles.data(), nullptr,
                      nullptr, nullptr, r.seen_points.data(), r.point_owner.data(), np,
                      &r.n_points, &r.roi_points, &r.base_covered, &ns)
                : pcp_place_coverage_pair(dev.ctx(), n ? poses.data() : nullptr, n, &fan, &pp,
                                          roi_p, np, r.best_pair, &r.pair_gain, &r.best_single,
                                          &r.single_gain, singles.data(), nullptr, nullptr,
                                          nullptr, r.seen_points.data(), r.point_owner.data(), np,
                                          &r.n_points, &r.roi_points, &r.base_covered, &ns);
    if (rc != PCP_OK) {
        err_ = dev.error();
        if (err_.empty()) err_ = "CoveragePlacement: pcp_place_coverage_pair failed";
        return r;
    }
    if (r.n_points != np) {
        err_ = "CoveragePlacement: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.seen_points.resize(n);
    r.point_owner.resize(np);
    r.n_fixed = pp.n_fixed;
    r.pair_searched = true;
    // the rounds of the answer: a alone gains g[a], then b the rest of the pair's gain; or the
    // best single candidate alone
    uint64_t covered = r.base_covered;
    auto round = [&](int64_t cand, uint64_t gain) {
        Round q;
        q.candidate = cand;
        q.gain = gain;
        covered += gain;
        q.covered = covered;
        q.coverage_ratio = r.roi_points ? (double)covered / (double)r.roi_points : 0.0;
        r.rounds.push_back(q);
    };
    if (ns == 2) {
        const uint64_t ga = (uint64_t)singles[(size_t)r.best_pair[0]];
        round(r.best_pair[0], ga);
        round(r.best_pair[1], r.pair_gain - ga);
    } else if (ns == 1) {
        round(r.best_single, r.single_gain);
    }
    blind_spots(r, terrain, bytes);
    r.ran = true;
    return r;
}

}  // namespace pcp
