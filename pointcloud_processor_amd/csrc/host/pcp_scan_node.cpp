// pcp_scan_node.cpp -- VirtualScan: see pcp_scan_node.hpp
#include "pcp_scan_node.hpp"

#include <cstring>

namespace pcp {

PointCloud2 make_scan_cloud(const pcp_scan_return *rec, size_t n, const std::string &frame) {
    static_assert(sizeof(pcp_scan_return) == 24, "pcp_scan_return is the message's record");
    PointCloud2 m;
    m.frame_id = frame;
    m.width = (uint32_t)n;
    m.point_step = sizeof(pcp_scan_return);
    m.row_step = m.point_step * (uint32_t)n;
    m.fields = {{"x", 0, PointField::FLOAT32, 1},     {"y", 4, PointField::FLOAT32, 1},
                {"z", 8, PointField::FLOAT32, 1},     {"range", 12, PointField::FLOAT32, 1},
                {"ray", 16, PointField::UINT32, 1},   {"point", 20, PointField::UINT32, 1}};
    m.data.resize(n * sizeof(pcp_scan_return));
    if (n) std::memcpy(m.data.data(), rec, m.data.size());
    return m;
}

VirtualScan::Result VirtualScan::scan(
    Device &dev, const PointCloud2 &terrain,
    const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &sensors,
    const std::string &frame) {
    Result r;
    err_.clear();
    const size_t n = sensors.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = sensors[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    return run(dev, terrain, poses, n, false, frame);
}

VirtualScan::Result VirtualScan::scan_mounted(Device &dev, const PointCloud2 &terrain,
                                              const std::vector<SensorPose> &sensors,
                                              const std::string &frame) {
    const size_t n = sensors.size();
    std::vector<double> poses(6 * n);
    for (size_t i = 0; i < n; ++i) {
        const SensorPose &c = sensors[i];
        const double row[6] = {c.x, c.y, c.z, c.roll, c.pitch, c.yaw};
        std::memcpy(poses.data() + 6 * i, row, sizeof row);
    }
    return run(dev, terrain, poses, n, true, frame);
}

VirtualScan::Result VirtualScan::run(Device &dev, const PointCloud2 &terrain,
                                     const std::vector<double> &poses, size_t n, bool mounted,
                                     const std::string &frame) {
    Result r;
    err_.clear();
    const pcp_fan_params fan{p_.n_az, p_.n_el, p_.el_min, p_.el_max, p_.max_distance};
    if (p_.n_az <= 0 || p_.n_el <= 0 || n > PCP_SCAN_MAX_POSES) {
        err_ = "VirtualScan: bad fan size or more than PCP_SCAN_MAX_POSES sensors";
        return r;
    }
    const bool table = mounted && !p_.el_table.empty();
    if (table && p_.el_table.size() != (size_t)p_.n_el) {
        err_ = "VirtualScan: el_table does not hold n_el entries";
        return r;
    }
    const size_t np = terrain.size();
    const uint64_t cap = (uint64_t)n * (uint64_t)p_.n_az * (uint64_t)p_.n_el;
    std::vector<pcp_scan_return> rec(cap ? cap : 1);
    std::vector<uint64_t> off(n + 1, 0);
    r.point_mask.assign(np ? np : 1, 0);
    r.seen_points.assign(n ? n : 1, 0);
    uint64_t total = 0;
    const int rc =
        mounted ? pcp_simulate_scan_mounted(dev.ctx(), n ? poses.data() : nullptr, n, &fan,
                                            table ? p_.el_table.data() : nullptr, rec.data(), cap,
                                            &total, off.data(), nullptr, nullptr, nullptr,
                                            r.point_mask.data(), np, &r.n_points,
                                            r.seen_points.data(), &r.n_seen_any)
                : pcp_simulate_scan(dev.ctx(), n ? poses.data() : nullptr, n, &fan, rec.data(), cap,
                                    &total, off.data(), nullptr, nullptr, nullptr,
                                    r.point_mask.data(), np, &r.n_points, r.seen_points.data(),
                                    &r.n_seen_any);
    if (rc != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    if (r.n_points != np) {
        err_ = "VirtualScan: the terrain message is not the cloud the terrain index was built from";
        return r;
    }
    r.point_mask.resize(np);
    r.seen_points.resize(n);
    for (size_t s = 0; s < n; ++s)
        r.scans.push_back(make_scan_cloud(rec.data() + off[s], (size_t)(off[s + 1] - off[s]), frame));
    // the blind spots: the message's own records, input order
    PointCloud2 &b = r.blind_spots;
    b.frame_id = terrain.frame_id;
    b.stamp = terrain.stamp;
    b.fields = terrain.fields;
    b.is_bigendian = terrain.is_bigendian;
    b.point_step = terrain.point_step;
    b.is_dense = terrain.is_dense;
    const size_t step = terrain.point_step;
    size_t nb = 0;
    for (size_t i = 0; i < np; ++i) nb += r.point_mask[i] == 0;
    b.data.resize(nb * step);
    size_t w = 0;
    for (size_t i = 0; i < np; ++i)
        if (r.point_mask[i] == 0 && (i + 1) * step <= terrain.data.size()) {
            std::memcpy(b.data.data() + w * step, terrain.data.data() + i * step, step);
            ++w;
        }
    b.data.resize(w * step);
    b.width = (uint32_t)w;
    b.row_step = (uint32_t)(w * step);
    r.ran = true;
    return r;
}

}  // namespace pcp
