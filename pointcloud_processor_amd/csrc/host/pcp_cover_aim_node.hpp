// pcp_cover_aim_node.hpp -- mobile LiDARs with a limited field of view placed by the terrain
// their scans reach, above pcp_place_coverage_aimed: where to stand and which way to look, over
// CoveragePlacement's regions, with its blind spots and its log table plus the aim column.  A
// translation unit of its own (pcp_cover_aim_node.cpp), the only one above the C ABI that
// references the aimed calls: pcp_nodes.cpp, pcp_placement.cpp and pcp_cover_node.cpp do not.
#pragma once

#include <string>
#include <vector>

#include "pcp_cover_node.hpp"

namespace pcp {

class AimedCoveragePlacement {
   public:
    struct Aim {
        int32_t az0 = 0;   // first column of the window, 0 .. n_az - 1 (the window wraps)
        int32_t el0 = 0;   // first ring of the window, 0 .. n_el - w_el
    };
    struct Params {
        int num_mobile_lidars = 2;     // sensors to place, 1 .. PCP_PLACE_MAX
        double min_separation = 0.0;   // metres in XY between sensors; <= 0: none
        int w_az = 1, w_el = 1;        // the window: columns by rings of the fan
        std::vector<Aim> aims;         // 1 .. PCP_COVER_AIM_MAX, searched at every candidate
    };
    struct Fixed {                     // a sensor already placed: candidate and aim indices
        int64_t candidate = -1;
        int32_t aim = -1;
    };
    using Roi = CoverageRoi;
    // CoveragePlacement's result (rounds, owners, blind spots, counts), and per round its aim
    struct Result : CoveragePlacement::Result {
        std::vector<int32_t> aim;            // per round: index into the aims
        std::vector<Aim> aims;               // the table searched
        int32_t w_az = 0, w_el = 0;
        std::vector<uint32_t> aim_points;    // [candidates][aims]: terrain points each window reaches
    };
    AimedCoveragePlacement() = default;
    explicit AimedCoveragePlacement(const Params &p) : p_(p) {}
    Params &params() { return p_; }
    const Params &params() const { return p_; }
    // the candidates and their aims placed greedily against the context's terrain index; the
    // arguments are CoveragePlacement::place's, fixed = (candidate, aim) pairs already placed
    Result place(Device &dev, const PointCloud2 &terrain,
                 const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
                 const VirtualScan::Params &fan, const std::vector<Fixed> &fixed = {},
                 const Roi &roi = Roi());
    // the same over tilted mounts with fan.el_table's beam model: an aim turns the head about its
    // own spin axis
    Result place_mounted(Device &dev, const PointCloud2 &terrain,
                         const std::vector<VirtualScan::SensorPose> &candidates,
                         const VirtualScan::Params &fan, const std::vector<Fixed> &fixed = {},
                         const Roi &roi = Roi());
    const std::string &lastError() const { return err_; }

   private:
    Result run(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
               bool mounted, const VirtualScan::Params &fan, const std::vector<Fixed> &fixed,
               const Roi &roi);
    Params p_;
    std::string err_;
};

// coverage_log's table with each sensor's aim beside its candidate: host arithmetic only
std::string aimed_coverage_log(const AimedCoveragePlacement::Result &r);

}  // namespace pcp
