// pcp_scan_node.hpp -- the simulated scans of placed LiDARs above pcp_simulate_scan: one
// PointCloud2 per sensor (the terrain points its beams hit) and the terrain's blind-spot cloud
// (the points no sensor's beam reaches).  A translation unit of its own: pcp_nodes.cpp (the
// drop-in surface of the reference's nodes) does not reference it.
#pragma once

#include <string>
#include <vector>

#include "pcp_nodes.hpp"

namespace pcp {

class VirtualScan {
   public:
    struct Params {   // the beam fan (pcp_fan_params)
        int n_az = 1024, n_el = 256;
        double el_min = -85.0 * 3.14159265358979323846 / 180.0;
        double el_max = 85.0 * 3.14159265358979323846 / 180.0;
        double max_distance = 15.0;
        // scan_mounted only: the rings' elevations in radians, n_el entries in any order
        // (pcp_simulate_scan_mounted's el_table); empty: the uniform rings el_min .. el_max
        std::vector<double> el_table;
    };
    // a mounted sensor (pcp_simulate_scan_mounted's poses6 row): pitch is the elevation of the
    // boresight, negative looks down -- a tf static transform "x y z yaw pitch_tf roll" is
    // pitch = -pitch_tf
    struct SensorPose {
        double x = 0.0, y = 0.0, z = 0.0, roll = 0.0, pitch = 0.0, yaw = 0.0;
    };
    struct Result {
        bool ran = false;                  // false: the call failed (lastError)
        // one message per sensor, in the sensors' order: point_step 24, fields x, y, z, range
        // (FLOAT32) and ray, point (UINT32), in ascending ray id (ray = j * n_az + i)
        std::vector<PointCloud2> scans;
        // the terrain message's records whose mask is zero, in input order (its layout)
        PointCloud2 blind_spots;
        std::vector<uint64_t> point_mask;  // per terrain point: bit s = sensor s reaches it
        std::vector<uint32_t> seen_points; // per sensor: terrain points it reaches
        uint64_t n_seen_any = 0;           // terrain points some sensor reaches
        uint64_t n_points = 0;             // terrain points
    };
    VirtualScan() = default;
    explicit VirtualScan(const Params &p) : p_(p) {}
    Params &params() { return p_; }
    const Params &params() const { return p_; }
    // the sensors' scans against the context's terrain index; terrain = the message that index
    // was built from (terrainCallback's), the source of the blind-spot records.  At most
    // PCP_SCAN_MAX_POSES sensors
    Result scan(Device &dev, const PointCloud2 &terrain,
                const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &sensors,
                const std::string &frame = "map");
    // the same from tilted mounts, with Params::el_table's beam model: the same Result
    Result scan_mounted(Device &dev, const PointCloud2 &terrain,
                        const std::vector<SensorPose> &sensors, const std::string &frame = "map");
    const std::string &lastError() const { return err_; }

   private:
    // poses: 5 (level) or 6 (mounted) doubles per sensor
    Result run(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
               bool mounted, const std::string &frame);
    Params p_;
    std::string err_;
};

// a sensor's returns as a PointCloud2 (host only)
PointCloud2 make_scan_cloud(const pcp_scan_return *rec, size_t n, const std::string &frame);

}  // namespace pcp
