// pcp_cover_node.cpp -- CoveragePlacement: see pcp_cover_node.hpp
#include "pcp_cover_node.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace pcp {

bool coverage_roi_bytes(const PointCloud2 &terrain, const CoveragePlacement::Box &box,
                        std::vector<uint8_t> &roi, std::string *why) {
    pcp_cloud_view v{};
    if (!cloud_view(terrain, v, why)) return false;
    roi.assign(v.n, 0);
    const uint8_t *base = static_cast<const uint8_t *>(v.data);
    for (uint64_t i = 0; i < v.n; ++i) {
        float p[3];
        const uint8_t *rec = base + i * v.point_step;
        std::memcpy(&p[0], rec + v.off_x, 4);
        std::memcpy(&p[1], rec + v.off_y, 4);
        std::memcpy(&p[2], rec + v.off_z, 4);
        // (a NaN fails every comparison, an infinity lies outside every finite box)
        roi[i] = (double)p[0] >= box.x0 && (double)p[0] <= box.x1 && (double)p[1] >= box.y0 &&
                 (double)p[1] <= box.y1 && (double)p[2] >= box.z0 && (double)p[2] <= box.z1;
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

std::string coverage_log(const CoveragePlacement::Result &r) {
    static const char *rule = "========================================";
    static const char *thin = "----------------------------------------";
    std::string s;
    line(s, "%s", rule);
    line(s, "Coverage Placement (%d Fixed + %zu Mobile)", r.n_fixed, r.rounds.size());
    line(s, "%s", rule);
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
        line(s, "%s", thin);
        line(s, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, x, y, z,
             (long long)q.candidate);
        line(s, "  Points gained: %llu", (unsigned long long)q.gain);
        line(s, "  Covered points: %llu of %llu (%.1f%%)", (unsigned long long)q.covered,
             (unsigned long long)r.roi_points, q.coverage_ratio * 100.0);
        covered = q.covered;
    }
    if (r.pair_searched) {   // the exact search: the best pair beside the best single candidate
        line(s, "%s", thin);
        if (r.best_pair[0] >= 0)
            line(s, "Best pair: candidates (%lld, %lld) gain %llu points; best single: candidate "
                 "%lld gains %llu (%s)", (long long)r.best_pair[0], (long long)r.best_pair[1],
                 (unsigned long long)r.pair_gain, (long long)r.best_single,
                 (unsigned long long)r.single_gain,
                 r.pair_gain > r.single_gain ? "the pair adds more" : "the pair adds no more");
        else
            line(s, "Best pair: none admissible; best single: candidate %lld gains %llu",
                 (long long)r.best_single, (unsigned long long)r.single_gain);
    }
    if (r.refined) {   // the exchanges: where the set started, a line per move, how it ended
        line(s, "%s", thin);
        line(s, "Exchange refinement (%d locked): start %llu points (%.1f%%)", r.n_locked,
             (unsigned long long)r.start_covered, pct(r.start_covered, r.roi_points));
        for (size_t m = 0; m < r.moves.size(); ++m)
            line(s, "  Move %zu: slot %d, candidate %lld -> %lld, covered %llu (%.1f%%)", m + 1,
                 r.moves[m].slot, (long long)r.moves[m].from, (long long)r.moves[m].to,
                 (unsigned long long)r.moves[m].covered, pct(r.moves[m].covered, r.roi_points));
        line(s, "  %s after %zu move%s", r.converged ? "No single move adds a point" : "Moves ran out",
             r.moves.size(), r.moves.size() == 1 ? "" : "s");
    }
    line(s, "%s", thin);
    line(s, "Blind spots: %llu of %llu (%.1f%%)", (unsigned long long)(r.roi_points - covered),
         (unsigned long long)r.roi_points, pct(r.roi_points - covered, r.roi_points));
    line(s, "%s", rule);
    return s;
}

CoveragePlacement::Result CoveragePlacement::place(
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
    Result r = run(dev, terrain, poses, n, false, fan, fixed, roi);
    for (const Round &q : r.rounds) {
        auto p = candidates[(size_t)q.candidate];
        p.total_score = (double)q.covered;
        r.placed.push_back(p);
    }
    if (r.ran) r.log = coverage_log(r);
    return r;
}

CoveragePlacement::Result CoveragePlacement::place_mounted(
    Device &dev, const PointCloud2 &terrain, const std::vector<VirtualScan::SensorPose> &candidates,
    const VirtualScan::Params &fan, const std::vector<int64_t> &fixed, const Roi &roi) {
    const size_t n = candidates.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const VirtualScan::SensorPose &c = candidates[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    Result r = run(dev, terrain, poses, n, true, fan, fixed, roi);
    for (const Round &q : r.rounds) r.placed_mounts.push_back(candidates[(size_t)q.candidate]);
    if (r.ran) r.log = coverage_log(r);
    return r;
}

bool CoveragePlacement::region(const PointCloud2 &terrain, size_t n, bool mounted,
                               const VirtualScan::Params &fp, const std::vector<int64_t> &fixed,
                               const Roi &roi, std::vector<uint8_t> &box_bytes,
                               const std::vector<uint8_t> *&bytes) {
    err_.clear();
    bytes = nullptr;
    if (fp.n_az <= 0 || fp.n_el <= 0 || n > PCP_COVER_MAX_POSES) {
        err_ = "CoveragePlacement: bad fan size or more than PCP_COVER_MAX_POSES candidates";
        return false;
    }
    if (fixed.size() > PCP_PLACE_MAX) {
        err_ = "CoveragePlacement: more than PCP_PLACE_MAX fixed candidates";
        return false;
    }
    const bool table = mounted && !fp.el_table.empty();
    if (table && fp.el_table.size() != (size_t)fp.n_el) {
        err_ = "CoveragePlacement: el_table does not hold n_el entries";
        return false;
    }
    if (roi.kind == Roi::Bytes) {
        bytes = &roi.bytes;
    } else if (roi.kind == Roi::InBox) {
        std::string why;
        if (!coverage_roi_bytes(terrain, roi.box, box_bytes, &why)) {
            err_ = "CoveragePlacement: " + why;
            return false;
        }
        bytes = &box_bytes;
    }
    if (bytes && bytes->size() != terrain.size()) {
        err_ = "CoveragePlacement: the region does not hold one byte per terrain point";
        return false;
    }
    return true;
}

// the blind spots: the message's own records of the region with no owner, input order
void CoveragePlacement::blind_spots(Result &r, const PointCloud2 &terrain,
                                    const std::vector<uint8_t> *bytes) {
    const size_t np = terrain.size();
    PointCloud2 &b = r.blind_spots;
    b.frame_id = terrain.frame_id;
    b.stamp = terrain.stamp;
    b.fields = terrain.fields;
    b.is_bigendian = terrain.is_bigendian;
    b.point_step = terrain.point_step;
    b.is_dense = terrain.is_dense;
    const size_t step = terrain.point_step;
    size_t w = 0;
    for (size_t i = 0; i < np; ++i) {
        const bool blind = r.point_owner[i] == PCP_OWNER_NONE && (!bytes || (*bytes)[i] != 0);
        if (!blind || (i + 1) * step > terrain.data.size()) continue;
        b.data.insert(b.data.end(), terrain.data.begin() + i * step,
                      terrain.data.begin() + (i + 1) * step);
        ++w;
    }
    b.width = (uint32_t)w;
    b.row_step = (uint32_t)(w * step);
}

CoveragePlacement::Result CoveragePlacement::run(Device &dev, const PointCloud2 &terrain,
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
    pcp_cover_params cp{};
    cp.k_max = p_.num_mobile_lidars;
    cp.n_fixed = (int32_t)fixed.size();
    cp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) cp.fixed[i] = fixed[i];
    int64_t sel[PCP_PLACE_MAX];
    uint64_t gain[PCP_PLACE_MAX], cov[PCP_PLACE_MAX];
    int32_t ns = 0;
    r.seen_points.assign(n ? n : 1, 0);
    r.point_owner.assign(np ? np : 1, PCP_OWNER_NONE);
    const uint8_t *roi_p = bytes ? bytes->data() : nullptr;
    const int rc =
        mounted ? pcp_place_coverage_mounted(dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                                             table ? fp.el_table.data() : nullptr, &cp, roi_p, np,
                                             sel, gain, cov, nullptr, r.seen_points.data(),
                                             r.point_owner.data(), np, &r.n_points, &r.roi_points,
                                             &r.base_covered, &ns)
                : pcp_place_coverage(dev.ctx(), n ? poses.data() : nullptr, n, &fan, &cp, roi_p, np,
                                     sel, gain, cov, nullptr, r.seen_points.data(),
                                     r.point_owner.data(), np, &r.n_points, &r.roi_points,
                                     &r.base_covered, &ns);
    if (rc != PCP_OK) {
        err_ = dev.error();
        if (err_.empty()) err_ = "CoveragePlacement: pcp_place_coverage failed";
        return r;
    }
    if (r.n_points != np) {
        err_ = "CoveragePlacement: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.seen_points.resize(n);
    r.point_owner.resize(np);
    r.n_fixed = cp.n_fixed;
    for (int32_t i = 0; i < ns; ++i) {
        Round q;
        q.candidate = sel[i];
        q.gain = gain[i];
        q.covered = cov[i];
        q.coverage_ratio = r.roi_points ? (double)cov[i] / (double)r.roi_points : 0.0;
        r.rounds.push_back(q);
    }
    blind_spots(r, terrain, bytes);
    r.ran = true;
    return r;
}

}  // namespace pcp
