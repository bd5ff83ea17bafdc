// pcp_cover_node.hpp -- mobile LiDARs placed by the terrain their scans reach, above
// pcp_place_coverage: the greedy maximum coverage of a region of the terrain message over the
// simulated scans of the candidates, and the blind spots the answer leaves; above
// pcp_place_coverage_pair the exact best pair (pcp_cover_pair_node.cpp, a unit of its own so that
// a program using only the greedy placement links without the pair call); and above
// pcp_place_coverage_refine a standing set improved by single-sensor exchanges
// (pcp_cover_refine_node.cpp, a unit of its own for the same reason).  Translation units of
// their own: pcp_nodes.cpp and pcp_placement.cpp do not reference them.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "pcp_scan_node.hpp"

namespace pcp {

// the region of interest: every terrain point, a byte per terrain point (non-zero counts), or an
// axis-aligned box in map coordinates (bounds included), turned into the bytes on the host
struct CoverageBox {
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
};
struct CoverageRoi {
    enum Kind { All, Bytes, InBox } kind = All;
    std::vector<uint8_t> bytes;    // Bytes: one per terrain point
    CoverageBox box;               // InBox
    CoverageRoi() = default;
    explicit CoverageRoi(std::vector<uint8_t> b) : kind(Bytes), bytes(std::move(b)) {}
    explicit CoverageRoi(const CoverageBox &b) : kind(InBox), box(b) {}
};

class CoveragePlacement {
   public:
    struct Params {
        int num_mobile_lidars = 2;     // sensors to place, 1 .. PCP_PLACE_MAX
        double min_separation = 0.0;   // metres in XY between sensors; <= 0: none
    };
    using Box = CoverageBox;
    using Roi = CoverageRoi;
    struct Round {
        int64_t candidate = -1;        // index into the candidates
        uint64_t gain = 0;             // points of the region this sensor reaches first
        uint64_t covered = 0;          // points of the region reached with sensors 0 .. r placed
        double coverage_ratio = 0;     // covered / points of the region
    };
    struct Move {                      // one exchange of refine(): slot `slot` went from -> to
        int32_t slot = -1;
        int64_t from = -1, to = -1;    // indices into the candidates
        uint64_t covered = 0;          // points of the region reached after the move
    };
    struct Result {
        bool ran = false;              // false: the call failed (lastError)
        // the placed sensors in placement order: `placed` after place(), `placed_mounts` after
        // place_mounted(); total_score = the points covered with that sensor placed
        std::vector<SimplifiedDualLidarOptimizer::LidarPosition> placed;
        std::vector<VirtualScan::SensorPose> placed_mounts;
        std::vector<Round> rounds;     // one per placed sensor
        uint64_t n_points = 0;         // terrain points
        uint64_t roi_points = 0;       // of them in the region
        uint64_t base_covered = 0;     // of those reached by the fixed candidates
        int32_t n_fixed = 0;
        std::vector<uint32_t> seen_points;   // per candidate: terrain points its scan reaches
        std::vector<int32_t> point_owner;    // per terrain point: fixed index, n_fixed + round, or
                                             // PCP_OWNER_NONE
        // the terrain message's records of the region that nobody reaches, in input order (the
        // message's layout, as VirtualScan's blind spots)
        PointCloud2 blind_spots;
        std::string log;               // a table in the style of placement_log
        // place_pair() / place_pair_mounted() only (pair_searched set): the exact search's figures
        bool pair_searched = false;
        int64_t best_pair[2] = {-1, -1};   // the best admissible pair, (-1, -1) without one
        uint64_t pair_gain = 0;            // points of the region the pair adds to the fixed ones'
        int64_t best_single = -1;          // the best admissible single candidate, -1 without one
        uint64_t single_gain = 0;          // points of the region it adds
        // refine() / refine_mounted() only (refined set): the exchanges' record
        bool refined = false;
        std::vector<Move> moves;           // in the order they were taken
        bool converged = false;            // no single move adds a point (false: the moves ran out)
        uint64_t start_covered = 0;        // points of the region the start set reaches
        int32_t n_locked = 0;
        std::vector<uint64_t> slot_unique; // per slot: points of the region only it reaches
    };
    CoveragePlacement() = default;
    explicit CoveragePlacement(const Params &p) : p_(p) {}
    Params &params() { return p_; }
    const Params &params() const { return p_; }
    // the candidates placed greedily against the context's terrain index; terrain = the message
    // that index was built from (terrainCallback's); fixed = candidates already placed, in order.
    // At most PCP_COVER_MAX_POSES candidates
    Result place(Device &dev, const PointCloud2 &terrain,
                 const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
                 const VirtualScan::Params &fan, const std::vector<int64_t> &fixed = {},
                 const Roi &roi = Roi());
    // the same over tilted mounts with fan.el_table's beam model (pcp_place_coverage_mounted):
    // the excavator's own LiDAR counts as a fixed row of such a call
    Result place_mounted(Device &dev, const PointCloud2 &terrain,
                         const std::vector<VirtualScan::SensorPose> &candidates,
                         const VirtualScan::Params &fan, const std::vector<int64_t> &fixed = {},
                         const Roi &roi = Roi());
    // The exact best pair instead of the greedy rounds (pcp_place_coverage_pair; the parameters'
    // sensor count is not used): every admissible pair of the candidates evaluated on the device.
    // The same Result: the rounds are a, then b (or the best single candidate alone where no pair
    // adds more than it), with the best single and the pair's gain beside them and a log line
    // comparing the two.  Defined in pcp_cover_pair_node.cpp
    Result place_pair(Device &dev, const PointCloud2 &terrain,
                      const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
                      const VirtualScan::Params &fan, const std::vector<int64_t> &fixed = {},
                      const Roi &roi = Roi());
    Result place_pair_mounted(Device &dev, const PointCloud2 &terrain,
                              const std::vector<VirtualScan::SensorPose> &candidates,
                              const VirtualScan::Params &fan,
                              const std::vector<int64_t> &fixed = {}, const Roi &roi = Roi());
    // A standing set improved by single-sensor exchanges (pcp_place_coverage_refine; the
    // parameters' sensor count is not used): start = the set as candidate indices, whose first
    // n_locked slots never move (the part of fixed sensors).  The same Result with the slots in
    // order as the rounds -- a round's gain = the points its slot reaches first -- the moves, the
    // blind spots of the refined set and a log line per move.  Defined in
    // pcp_cover_refine_node.cpp
    Result refine(Device &dev, const PointCloud2 &terrain,
                  const std::vector<SimplifiedDualLidarOptimizer::LidarPosition> &candidates,
                  const VirtualScan::Params &fan, const std::vector<int64_t> &start,
                  int n_locked = 0, int max_moves = 16, const Roi &roi = Roi());
    Result refine_mounted(Device &dev, const PointCloud2 &terrain,
                          const std::vector<VirtualScan::SensorPose> &candidates,
                          const VirtualScan::Params &fan, const std::vector<int64_t> &start,
                          int n_locked = 0, int max_moves = 16, const Roi &roi = Roi());
    const std::string &lastError() const { return err_; }

   private:
    // (pcp_cover_aim_node.hpp's and pcp_cover_weight_node.hpp's classes share region() and
    // blind_spots())
    friend class AimedCoveragePlacement;
    friend class WeightedCoveragePlacement;
    // poses: 5 (level) or 6 (mounted) doubles per candidate
    Result run(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses, size_t n,
               bool mounted, const VirtualScan::Params &fan, const std::vector<int64_t> &fixed,
               const Roi &roi);
    Result run_pair(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses,
                    size_t n, bool mounted, const VirtualScan::Params &fan,
                    const std::vector<int64_t> &fixed, const Roi &roi);
    Result run_refine(Device &dev, const PointCloud2 &terrain, const std::vector<double> &poses,
                      size_t n, bool mounted, const VirtualScan::Params &fan,
                      const std::vector<int64_t> &start, int n_locked, int max_moves,
                      const Roi &roi);
    // what every search refuses before the call (false: err_ says why), and the region as bytes
    // (bytes null: every point; box_bytes holds a box's)
    bool region(const PointCloud2 &terrain, size_t n, bool mounted, const VirtualScan::Params &fan,
                const std::vector<int64_t> &fixed, const Roi &roi, std::vector<uint8_t> &box_bytes,
                const std::vector<uint8_t> *&bytes);
    // r.blind_spots from r.point_owner
    static void blind_spots(Result &r, const PointCloud2 &terrain,
                            const std::vector<uint8_t> *bytes);
    Params p_;
    std::string err_;
};

// the box as bytes over the message's points (x, y, z FLOAT32 by name; a non-finite point is
// outside); false: the message has no such fields (*why says so)
bool coverage_roi_bytes(const PointCloud2 &terrain, const CoveragePlacement::Box &box,
                        std::vector<uint8_t> &roi, std::string *why = nullptr);
// the placement's table: host arithmetic only (after a pair search, with the comparison of the
// pair and the best single candidate; after a refinement, with a line per move)
std::string coverage_log(const CoveragePlacement::Result &r);

}  // namespace pcp
