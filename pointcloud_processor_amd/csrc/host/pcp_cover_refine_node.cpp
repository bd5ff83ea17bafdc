// pcp_cover_refine_node.cpp -- CoveragePlacement::refine / refine_mounted: see pcp_cover_node.hpp.
// The only unit above the C ABI that references pcp_place_coverage_refine.
#include <cstring>

#include "pcp_cover_node.hpp"

namespace pcp {

CoveragePlacement::Result CoveragePlacement::refine(
    Device &dev, const PointCloud2 &terrain,
    const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
    const VirtualScan::Params &fan, const std::vector<int64_t> &start, int n_locked, int max_moves,
    const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = candidates[i];
        const double row[5] = {c.x, c.y, c.z, c.pitch, c.yaw};
        std::memcpy(poses.data() + 5 * i, row, sizeof row);
    }
    Result r = run_refine(dev, terrain, poses, n, false, fan, start, n_locked, max_moves, roi);
    for (const Round &q : r.rounds) {
        auto p = candidates[(size_t)q.candidate];
        p.total_score = (double)q.covered;
        r.placed.push_back(p);
    }
    if (r.ran) r.log = coverage_log(r);
    return r;
}

CoveragePlacement::Result CoveragePlacement::refine_mounted(
    Device &dev, const PointCloud2 &terrain, const std::vector<VirtualScan::SensorPose> &candidates,
    const VirtualScan::Params &fan, const std::vector<int64_t> &start, int n_locked, int max_moves,
    const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const VirtualScan::SensorPose &c = candidates[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    Result r = run_refine(dev, terrain, poses, n, true, fan, start, n_locked, max_moves, roi);
    for (const Round &q : r.rounds) r.placed_mounts.push_back(candidates[(size_t)q.candidate]);
    if (r.ran) r.log = coverage_log(r);
    return r;
}

CoveragePlacement::Result CoveragePlacement::run_refine(
    Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
    bool mounted, const VirtualScan::Params &fp, const std::vector<int64_t> &start, int n_locked,
    int max_moves, const Roi &roi) {
    Result r;
    std::vector<uint8_t> box_bytes;
    const std::vector<uint8_t> *bytes = nullptr;
    if (!region(terrain, n, mounted, fp, {}, roi, box_bytes, bytes)) return r;
    if (start.empty() || start.size() > PCP_PLACE_MAX || max_moves < 0 ||
        max_moves > PCP_REFINE_MAX_MOVES) {
        err_ = "CoveragePlacement: a start set of 1 .. PCP_PLACE_MAX candidates and 0 .. "
               "PCP_REFINE_MAX_MOVES moves";
        return r;
    }
    const bool table = mounted && !fp.el_table.empty();
    const size_t np = terrain.size();
    const size_t k = start.size();
    const pcp_fan_params fan{fp.n_az, fp.n_el, fp.el_min, fp.el_max, fp.max_distance};
    pcp_refine_params rp{};
    rp.k = (int32_t)k;
    rp.n_locked = n_locked;
    rp.max_moves = max_moves;
    rp.min_separation = p_.min_separation;
    for (size_t i = 0; i < k; ++i) rp.start[i] = start[i];
    int64_t sel[PCP_PLACE_MAX], from[PCP_REFINE_MAX_MOVES], to[PCP_REFINE_MAX_MOVES];
    int32_t slot[PCP_REFINE_MAX_MOVES], nm = 0, conv = 0;
    uint64_t mcov[PCP_REFINE_MAX_MOVES], covered = 0;
    r.seen_points.assign(n ? n : 1, 0);
    r.point_owner.assign(np ? np : 1, PCP_OWNER_NONE);
    r.slot_unique.assign(k, 0);
    const uint8_t *roi_p = bytes ? bytes->data() : nullptr;
    const int rc =
        mounted ? pcp_place_coverage_refine_mounted(
                      dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                      table ? fp.el_table.data() : nullptr, &rp, roi_p, np, sel, &covered,
                      &r.start_covered, slot, from, to, mcov, nullptr, r.slot_unique.data(),
                      r.seen_points.data(), r.point_owner.data(), np, &r.n_points, &r.roi_points,
                      &nm, &conv)
                : pcp_place_coverage_refine(dev.ctx(), n ? poses.data() : nullptr, n, &fan, &rp,
                                            roi_p, np, sel, &covered, &r.start_covered, slot, from,
                                            to, mcov, nullptr, r.slot_unique.data(),
                                            r.seen_points.data(), r.point_owner.data(), np,
                                            &r.n_points, &r.roi_points, &nm, &conv);
    if (rc != PCP_OK) {
        err_ = dev.error();
        if (err_.empty()) err_ = "CoveragePlacement: pcp_place_coverage_refine failed";
        return r;
    }
    if (r.n_points != np) {
        err_ = "CoveragePlacement: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.seen_points.resize(n);
    r.point_owner.resize(np);
    r.refined = true;
    r.converged = conv != 0;
    r.n_locked = rp.n_locked;
    for (int32_t m = 0; m < nm; ++m) {
        Move mv;
        mv.slot = slot[m];
        mv.from = from[m];
        mv.to = to[m];
        mv.covered = mcov[m];
        r.moves.push_back(mv);
    }
    // the rounds of the answer: the slots in order, each with the points it owns (the ones no
    // lower slot reaches); their sum is the set's count
    std::vector<uint64_t> own(k, 0);
    for (size_t i = 0; i < np; ++i) {
        const int32_t o = r.point_owner[i];
        if (o >= 0 && (size_t)o < k) ++own[(size_t)o];
    }
    uint64_t sum = 0;
    for (size_t i = 0; i < k; ++i) {
        Round q;
        q.candidate = sel[i];
        q.gain = own[i];
        sum += own[i];
        q.covered = sum;
        q.coverage_ratio = r.roi_points ? (double)sum / (double)r.roi_points : 0.0;
        r.rounds.push_back(q);
    }
    if (sum != covered) {
        err_ = "CoveragePlacement: the owners do not add up to the covered count";
        r.rounds.clear();
        return r;
    }
    blind_spots(r, terrain, bytes);
    r.ran = true;
    return r;
}

}  // namespace pcp
