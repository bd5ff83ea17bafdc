// pcp_placement.hpp -- several mobile LiDARs: the greedy placement above pcp_place_sensors, for
// the candidates and the zx120 pose of a SimplifiedDualLidarOptimizer tick.  A translation unit
// of its own: pcp_nodes.cpp (the drop-in surface of the reference's nodes) does not reference it.
#pragma once

#include <string>
#include <vector>

#include "pcp_nodes.hpp"

namespace pcp {

class MobileLidarPlacement {
   public:
    struct Params {
        int num_mobile_lidars = 2;     // sensors to place, 1 .. PCP_PLACE_MAX
        double min_separation = 0.0;   // metres in XY between placed sensors; <= 0: none
    };
    struct Round {
        int64_t candidate = -1;        // index into the tick's candidates
        double total = 0;              // total with sensors 0 .. r placed
        double gain = 0;               // total - the total before this sensor
        int32_t covered = 0;           // cells with a positive combined score
        double coverage_ratio = 0;     // covered / total cells
    };
    struct Result {
        bool ran = false;              // false: the tick did not run, or the call failed
        std::vector<SimplifiedDualLidarOptimizer::LidarPosition> placed;   // in placement order,
                                                                            // total_score = Round::total
        std::vector<Round> rounds;     // one per placed sensor
        double zx120_total = 0;        // the total of the zx120 sensor alone
        int32_t zx120_covered = 0;
        int32_t total_cells = 0;
        std::string log;               // a table in the style of optimization_log
    };
    MobileLidarPlacement() = default;
    explicit MobileLidarPlacement(const Params &p) : p_(p) {}
    Params &params() { return p_; }
    const Params &params() const { return p_; }
    // the tick's candidates placed greedily against the context's terrain, zx120 cloud and cells
    // (the state the tick ran on); vl = the tick's parameters.  The optimizer's GridCell flags
    // are not touched
    Result place(Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
                 const SimplifiedDualLidarOptimizer::Params &vl);

    // The exact best pair (pcp_place_pair): every pair of the tick's candidates evaluated beside
    // zx120 and the `fixed` candidates (sensors already placed), not greedy rounds.
    struct PairResult {
        bool ran = false;              // false: the tick did not run, or the call failed
        int32_t n_selected = 0;        // 2: the pair beats the best single; 1: only the single
                                       // adds to the base; 0: nothing does
        int64_t pair[2] = {-1, -1};    // candidate indices, a < b; -1: no admissible pair
        double pair_total = 0;
        int32_t pair_covered = 0;
        int64_t single = -1;           // the best single candidate; -1: none admissible
        double single_total = 0;
        int32_t single_covered = 0;
        double base_total = 0;         // zx120 and the fixed sensors alone
        int32_t base_covered = 0;
        int32_t n_fixed = 0;
        int32_t total_cells = 0;
        std::vector<SimplifiedDualLidarOptimizer::LidarPosition> placed;   // the n_selected chosen
        SimplifiedDualLidarOptimizer::LidarPosition pair_pos[2], single_pos;   // where they exist
        std::string log;
    };
    // min_separation is params()'s; num_mobile_lidars plays no part.  greedy (nullable): a
    // place() result for the same tick, whose first two sensors the log compares the pair with
    PairResult place_pair(Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
                          const SimplifiedDualLidarOptimizer::Params &vl,
                          const std::vector<int64_t> &fixed = {}, const Result *greedy = nullptr);

    // The exact best triple (pcp_place_triple): every triple of the tick's candidates evaluated
    // beside zx120 and the `fixed` candidates, with the best pair, the best single and the base it
    // is compared with.
    struct TripleResult : PairResult {   // n_selected 3: the triple beats the pair, the single
                                         // and the base; 2, 1, 0: as PairResult
        int64_t triple[3] = {-1, -1, -1};   // candidate indices, a < b < c; -1: no admissible triple
        double triple_total = 0;
        int32_t triple_covered = 0;
        SimplifiedDualLidarOptimizer::LidarPosition triple_pos[3];   // where it exists
    };
    // min_separation is params()'s; num_mobile_lidars plays no part.  greedy (nullable): a
    // place() result for the same tick, whose first three sensors the log compares the triple with
    TripleResult place_triple(Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
                              const SimplifiedDualLidarOptimizer::Params &vl,
                              const std::vector<int64_t> &fixed = {},
                              const Result *greedy = nullptr);

    // 1-exchange refinement (pcp_place_refine): the set `start` of the tick's candidates -- a
    // place() answer, or a deployment as it stands -- improved by moving one sensor at a time to
    // the candidate that raises the total most, until no single move raises it.
    struct Move {
        int32_t slot = -1;             // which sensor of the set moved
        int64_t from = -1, to = -1;    // candidate indices
        SimplifiedDualLidarOptimizer::LidarPosition from_pos, to_pos;
        double total = 0;              // the set's total after the move
        double gain = 0;               // total - the total before it
        int32_t covered = 0;
    };
    struct RefineResult {
        bool ran = false;              // false: the tick did not run, or the call failed
        bool converged = false;        // no single move raises the total (1-exchange optimal);
                                       // false: max_moves ran out first
        std::vector<int64_t> start, selected;   // candidate indices by slot
        int32_t n_locked = 0;
        double start_total = 0, total = 0;
        int32_t start_covered = 0, covered = 0;
        int32_t total_cells = 0;
        std::vector<Move> moves;
        std::vector<SimplifiedDualLidarOptimizer::LidarPosition> placed;   // the refined set by
                                                                            // slot, total_score = total
        std::string log;
    };
    // min_separation is params()'s and is tested for the incoming candidate of a move only;
    // slots 0 .. n_locked - 1 never move; num_mobile_lidars plays no part
    RefineResult refine(Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
                        const SimplifiedDualLidarOptimizer::Params &vl,
                        const std::vector<int64_t> &start, int n_locked = 0,
                        int max_moves = PCP_REFINE_MAX_MOVES);

    // Sensors with a limited field of view (pcp_place_aimed): every candidate of the tick is
    // searched with every aim of a table, greedily as place(), beside zx120 and the `fixed`
    // aimed sensors.  The answer says where to stand and which way to look.
    struct Aim {
        double yaw_offset = 0;         // radians, added to the candidate's yaw
        double pitch = 0;              // radians, -pi / 2 .. pi / 2
    };
    struct AimedParams {
        double h_fov = 0, v_fov = 0;   // full angles, radians (h_fov >= 2 pi: no horizontal test)
        std::vector<Aim> aims;         // 1 .. PCP_AIM_MAX
    };
    struct FixedAimed {
        int64_t candidate = -1;
        int32_t aim = -1;
    };
    struct AimedRound : Round {
        int32_t aim = -1;              // index into AimedParams::aims
    };
    struct AimedResult {
        bool ran = false;              // false: the tick did not run, or the call failed
        std::vector<SimplifiedDualLidarOptimizer::LidarPosition> placed;   // in placement order:
                                       // yaw = the candidate's + the aim's offset, pitch = the
                                       // aim's, total_score = AimedRound::total
        std::vector<AimedRound> rounds;
        double base_total = 0;         // zx120 and the fixed sensors alone
        int32_t base_covered = 0;
        int32_t n_fixed = 0;
        int32_t total_cells = 0;
        double h_fov = 0, v_fov = 0;
        std::string log;
    };
    // num_mobile_lidars and min_separation are params()'s
    AimedResult place_aimed(Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
                            const SimplifiedDualLidarOptimizer::Params &vl, const AimedParams &ap,
                            const std::vector<FixedAimed> &fixed = {});
    const std::string &lastError() const { return err_; }

   private:
    Params p_;
    std::string err_;
};

// the placement's table: host arithmetic only
std::string placement_log(const MobileLidarPlacement::Result &r);
// the pair search's table in the same format: the base, the best single, the best pair with its
// gain over the single, and (greedy given, two sensors placed) its gain over greedy's two
std::string placement_pair_log(const MobileLidarPlacement::PairResult &r,
                               const MobileLidarPlacement::Result *greedy = nullptr);
// the triple search's table in the same format: the base, the best single, the best pair and the
// best triple with its gain over the pair, and (greedy given, three sensors placed) its gain over
// greedy's three
std::string placement_triple_log(const MobileLidarPlacement::TripleResult &r,
                                 const MobileLidarPlacement::Result *greedy = nullptr);
// the refinement's table in the same format: the start set, every move (slot, from and to with
// their positions, the gain), and either "1-exchange optimal" or "stopped after N moves"
std::string placement_refine_log(const MobileLidarPlacement::RefineResult &r);
// the aimed placement's table in the same format: the field of view, the base, and per sensor its
// position, heading and pitch with the candidate and the aim they come from
std::string placement_aimed_log(const MobileLidarPlacement::AimedResult &r);

}  // namespace pcp
