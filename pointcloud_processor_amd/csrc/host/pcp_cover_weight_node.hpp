// pcp_cover_weight_node.hpp -- mobile LiDARs placed by the WEIGHT of the terrain their scans reach,
// above pcp_place_coverage_weighted: CoveragePlacement's inputs with a weight of 0 .. 255 per
// terrain point in the region's place -- a point of the pit's working face may count 200 where a
// point of the apron counts 1 -- its blind spots and its log table in weight and in points.  A
// translation unit of its own (pcp_cover_weight_node.cpp), the only one above the C ABI that
// references the weighted calls: pcp_nodes.cpp, pcp_placement.cpp and the other coverage units
// do not.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "pcp_cover_node.hpp"

namespace pcp {

// the weights: a byte per terrain point, or a base weight and an ordered list of (axis-aligned box
// in map coordinates, bounds included; weight) turned into the bytes on the host -- a point takes
// the weight of the LAST box of the list that holds it, the base weight when none does.  Weight 0
// puts a point outside the region
struct CoverageWeightBox {
    CoverageBox box;
    uint8_t weight = 1;
};
struct CoverageWeights {
    enum Kind { Bytes, Boxes } kind = Boxes;
    std::vector<uint8_t> bytes;             // Bytes: one per terrain point
    uint8_t base = 1;                       // Boxes: the weight outside every box
    std::vector<CoverageWeightBox> boxes;   // Boxes: a later box overrides an earlier one
    CoverageWeights() = default;            // every point weighs 1
    explicit CoverageWeights(std::vector<uint8_t> b) : kind(Bytes), bytes(std::move(b)) {}
    CoverageWeights(uint8_t base_weight, std::vector<CoverageWeightBox> list)
        : kind(Boxes), base(base_weight), boxes(std::move(list)) {}
};

class WeightedCoveragePlacement {
   public:
    using Params = CoveragePlacement::Params;
    using Weights = CoverageWeights;
    // CoveragePlacement's result with the rounds in WEIGHT -- a round's gain = the weight its
    // sensor reaches first, covered = the weight reached with sensors 0 .. r placed,
    // coverage_ratio = covered / roi_weight; base_covered = the weight the fixed candidates
    // reach; roi_points stays the region's point count -- and beside them the same in points
    struct Result : CoveragePlacement::Result {
        std::vector<uint64_t> gain_points;   // per round: points its sensor reaches first
        uint64_t roi_weight = 0;             // the region's weight
        uint64_t base_points = 0;            // points of the region the fixed candidates reach
        uint64_t blind_weight = 0;           // weight of the blind spots
        uint64_t blind_points = 0;           // their count (blind_spots.width)
        std::vector<uint8_t> weight;         // the bytes the call was given
    };
    WeightedCoveragePlacement() = default;
    explicit WeightedCoveragePlacement(const Params &p) : p_(p) {}
    Params &params() { return p_; }
    const Params &params() const { return p_; }
    // CoveragePlacement::place's arguments with the weights in the region's place
    Result place(Device &dev, const PointCloud2 &terrain,
                 const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
                 const VirtualScan::Params &fan, const Weights &weights = Weights(),
                 const std::vector<int64_t> &fixed = {});
    // the same over tilted mounts with fan.el_table's beam model
    Result place_mounted(Device &dev, const PointCloud2 &terrain,
                         const std::vector<VirtualScan::SensorPose> &candidates,
                         const VirtualScan::Params &fan, const Weights &weights = Weights(),
                         const std::vector<int64_t> &fixed = {});
    const std::string &lastError() const { return err_; }

   private:
    Result run(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
               bool mounted, const VirtualScan::Params &fan, const Weights &weights,
               const std::vector<int64_t> &fixed);
    Params p_;
    std::string err_;
};

// the base weight and the box list as bytes over the message's points (x, y, z FLOAT32 by name; a
// non-finite point lies in no box and takes the base weight); false: the message has no such
// fields (*why says so)
bool coverage_weight_bytes(const PointCloud2 &terrain, uint8_t base,
                           const std::vector<CoverageWeightBox> &boxes,
                           std::vector<uint8_t> &weight, std::string *why = nullptr);
// coverage_log's table in weight, the points beside it: host arithmetic only
std::string weighted_coverage_log(const WeightedCoveragePlacement::Result &r);

}  // namespace pcp
