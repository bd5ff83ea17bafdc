// pcp_placement.cpp -- MobileLidarPlacement: see pcp_placement.hpp
#include "pcp_placement.hpp"

#include <cstdarg>
#include <cstdio>

namespace pcp {
namespace {

using Opt = SimplifiedDualLidarOptimizer;
using MLP = MobileLidarPlacement;
using Position = Opt::LidarPosition;

// ---- marshalling: what the five calls share -------------------------------------------------

// what every placement call takes from the tick: the zx120 pose, the scoring parameters and the
// candidates as flat poses
struct TickArgs {
    double zx[5];
    pcp_vl_params params;
    uint64_t n;
    std::vector<double> poses;
    TickArgs(const Opt::Result &tick, const Opt::Params &vl)
        : zx{tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch, tick.zx120.yaw},
          params{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                 vl.num_candidates,  vl.vertical_layers},
          n(tick.candidates.size()),
          poses(5 * tick.candidates.size()) {
        for (size_t i = 0; i < n; ++i) {
            const auto &c = tick.candidates[i];
            poses[5 * i] = c.x;
            poses[5 * i + 1] = c.y;
            poses[5 * i + 2] = c.z;
            poses[5 * i + 3] = c.pitch;
            poses[5 * i + 4] = c.yaw;
        }
    }
};

// the pair and the triple search's parameters; fixed.size() <= PCP_PLACE_MAX
pcp_pair_params pair_params(const std::vector<int64_t> &fixed, double min_separation) {
    pcp_pair_params pp{};
    pp.n_fixed = (int32_t)fixed.size();
    pp.min_separation = min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) pp.fixed[i] = fixed[i];
    return pp;
}

// candidate idx of the tick with the total it was chosen at
Position position(const Opt::Result &tick, int64_t idx, double total) {
    Position p = tick.candidates[(size_t)idx];
    p.total_score = total;
    return p;
}

// greedy rounds (place, place_aimed): a round's gain is over the total before it, `before` at first
template <class R>
void greedy_rounds(const Opt::Result &tick, const int64_t *sel, const double *tot,
                   const int32_t *cov, int32_t ns, double before, int32_t total_cells,
                   std::vector<R> &rounds, std::vector<Position> &placed) {
    for (int32_t i = 0; i < ns; ++i) {
        R q;
        q.candidate = sel[i];
        q.total = tot[i];
        q.gain = tot[i] - before;
        q.covered = cov[i];
        q.coverage_ratio = total_cells > 0 ? (double)cov[i] / total_cells : 0.0;
        before = tot[i];
        rounds.push_back(q);
        const Position p = position(tick, sel[i], tot[i]);
        placed.push_back(p);
    }
}

// an exact search's answer (its indices and totals are in r): the positions where they exist, and
// the n_selected chosen ones; triple_pos: the triple search's, filled by the caller
void finish_exact(MLP::PairResult &r, const Opt::Result &tick, int32_t n_fixed,
                  const Position *triple_pos = nullptr) {
    r.ran = true;
    r.n_fixed = n_fixed;
    r.total_cells = tick.report.total_cells;
    if (r.single >= 0) r.single_pos = position(tick, r.single, r.single_total);
    for (int i = 0; i < 2 && r.pair[0] >= 0; ++i)
        r.pair_pos[i] = position(tick, r.pair[i], r.pair_total);
    const Position *chosen = r.n_selected == 1   ? &r.single_pos
                             : r.n_selected == 2 ? r.pair_pos
                             : r.n_selected == 3 ? triple_pos
                                                 : nullptr;
    if (chosen) r.placed.assign(chosen, chosen + r.n_selected);
}

// ---- the logs' writer: the lines and the blocks the five tables are made of ------------------
class Log {
   public:
    explicit Log(int32_t total_cells) : tc_(total_cells) {}
    __attribute__((format(printf, 2, 3))) void line(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vline(fmt, ap);
        va_end(ap);
    }
    void rule() { line("%s", "========================================"); }
    void thin() { line("%s", "----------------------------------------"); }
    // a rule and the table's heading; the caller closes it with rule()
    __attribute__((format(printf, 2, 3))) void title(const char *fmt, ...) {
        rule();
        va_list ap;
        va_start(ap, fmt);
        vline(fmt, ap);
        va_end(ap);
    }
    void covered(int v) {
        line("  Covered cells: %d of %d (%.1f%%)", v, tc_, tc_ > 0 ? (double)v / tc_ * 100.0 : 0.0);
    }
    // what the search starts from
    void base(const char *of, double total, int covered_cells) {
        line("Total Score (%s): %.2f", of, total);
        covered(covered_cells);
    }
    // over: "" or what the gain is over (" over single")
    void score(double total, const char *over, double gain, int covered_cells) {
        line("  Total Score: %.2f (gain%s %.2f)", total, over, gain);
        covered(covered_cells);
    }
    // from: after the candidate, inside the brackets (", aim 3"); suffix: after them
    void mobile(size_t i, const Position &p, int64_t candidate, const char *from = "",
                const char *suffix = "") {
        line("Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld%s]%s", i + 1, p.x, p.y,
             p.z, (long long)candidate, from, suffix);
    }
    void best_single(const MLP::PairResult &r) {
        if (r.single < 0) return line("Best Single Position: none admissible");
        const auto &p = r.single_pos;
        line("Best Single Position: (%.2f, %.2f, %.2f)  [candidate %lld]", p.x, p.y, p.z,
             (long long)r.single);
        score(r.single_total, "", r.single_total - r.base_total, r.single_covered);
    }
    void best_pair(const MLP::PairResult &r) {
        if (r.pair[0] < 0) return line("Best Pair: no admissible pair");
        for (int i = 0; i < 2; ++i) {
            const auto &p = r.pair_pos[i];
            line("Best Pair LiDAR %d Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, p.x,
                 p.y, p.z, (long long)r.pair[i]);
        }
        score(r.pair_total, " over single", r.pair_total - r.single_total, r.pair_covered);
    }
    // the heading of an exact search, its base, the best single and the best pair
    void exact_head(const char *what, const MLP::PairResult &r) {
        title("Exact %s Placement (ZX120 + %d Fixed + %d Mobile)", what, r.n_fixed, r.n_selected);
        rule();
        base(zx120_with(r.n_fixed), r.base_total, r.base_covered);
        thin();
        best_single(r);
        thin();
        best_pair(r);
    }
    static const char *zx120_with(int32_t n_fixed) { return n_fixed ? "ZX120 + fixed" : "ZX120 only"; }
    std::string take() { return std::move(s_); }

   private:
    void vline(const char *fmt, va_list ap) {
        char buf[512];
        vsnprintf(buf, sizeof(buf), fmt, ap);
        s_ += buf;
        s_ += '\n';
    }
    std::string s_;
    int32_t tc_;
};

}  // namespace

std::string placement_log(const MobileLidarPlacement::Result &r) {
    Log log(r.total_cells);
    log.title("Multi LiDAR Placement (ZX120 + %zu Mobile)", r.placed.size());
    log.rule();
    log.base("ZX120 only", r.zx120_total, r.zx120_covered);
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        log.thin();
        log.mobile(i, r.placed[i], q.candidate);
        log.score(q.total, "", q.gain, q.covered);
    }
    log.rule();
    return log.take();
}

MobileLidarPlacement::Result MobileLidarPlacement::place(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl) {
    Result r;
    err_.clear();
    if (!tick.ran) return r;
    const TickArgs a(tick, vl);
    const pcp_place_params pp{p_.num_mobile_lidars, 0, p_.min_separation};
    int64_t sel[PCP_PLACE_MAX];
    double tot[PCP_PLACE_MAX];
    int32_t cov[PCP_PLACE_MAX], ns = 0;
    if (pcp_place_sensors(dev.ctx(), a.poses.data(), a.n, a.zx, &a.params, &pp, sel, tot, cov, nullptr,
                          nullptr, nullptr, &r.zx120_total, &r.zx120_covered, &ns) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.total_cells = tick.report.total_cells;
    greedy_rounds(tick, sel, tot, cov, ns, r.zx120_total, r.total_cells, r.rounds, r.placed);
    r.log = placement_log(r);
    return r;
}

std::string placement_pair_log(const MobileLidarPlacement::PairResult &r,
                               const MobileLidarPlacement::Result *greedy) {
    Log log(r.total_cells);
    log.exact_head("Pair", r);
    if (r.pair[0] >= 0 && greedy && greedy->ran && greedy->rounds.size() >= 2)
        log.line("  Greedy pair [candidates %lld, %lld]: %.2f (exact pair gains %.2f)",
                 (long long)greedy->rounds[0].candidate, (long long)greedy->rounds[1].candidate,
                 greedy->rounds[1].total, r.pair_total - greedy->rounds[1].total);
    log.rule();
    return log.take();
}

MobileLidarPlacement::PairResult MobileLidarPlacement::place_pair(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl, const std::vector<int64_t> &fixed,
    const Result *greedy) {
    PairResult r;
    err_.clear();
    if (!tick.ran) return r;
    if (fixed.size() > PCP_PLACE_MAX) {
        err_ = "place_pair: more fixed sensors than PCP_PLACE_MAX";
        return r;
    }
    const TickArgs a(tick, vl);
    const pcp_pair_params pp = pair_params(fixed, p_.min_separation);
    if (pcp_place_pair(dev.ctx(), a.poses.data(), a.n, a.zx, &a.params, &pp, r.pair, &r.pair_total,
                       &r.pair_covered, &r.single, &r.single_total, &r.single_covered,
                       &r.base_total, &r.base_covered, nullptr, nullptr, nullptr, nullptr,
                       &r.n_selected) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    finish_exact(r, tick, pp.n_fixed);
    r.log = placement_pair_log(r, greedy);
    return r;
}

std::string placement_triple_log(const MobileLidarPlacement::TripleResult &r,
                                 const MobileLidarPlacement::Result *greedy) {
    Log log(r.total_cells);
    log.exact_head("Triple", r);
    log.thin();
    if (r.triple[0] >= 0) {
        for (int i = 0; i < 3; ++i) {
            const auto &p = r.triple_pos[i];
            log.line("Best Triple LiDAR %d Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1,
                     p.x, p.y, p.z, (long long)r.triple[i]);
        }
        log.score(r.triple_total, " over pair", r.triple_total - r.pair_total, r.triple_covered);
        if (greedy && greedy->ran && greedy->rounds.size() >= 3)
            log.line("  Greedy triple [candidates %lld, %lld, %lld]: %.2f (exact triple gains %.2f)",
                     (long long)greedy->rounds[0].candidate, (long long)greedy->rounds[1].candidate,
                     (long long)greedy->rounds[2].candidate, greedy->rounds[2].total,
                     r.triple_total - greedy->rounds[2].total);
    } else {
        log.line("Best Triple: no admissible triple");
    }
    log.rule();
    return log.take();
}

MobileLidarPlacement::TripleResult MobileLidarPlacement::place_triple(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl, const std::vector<int64_t> &fixed,
    const Result *greedy) {
    TripleResult r;
    err_.clear();
    if (!tick.ran) return r;
    if (fixed.size() > PCP_PLACE_MAX) {
        err_ = "place_triple: more fixed sensors than PCP_PLACE_MAX";
        return r;
    }
    const TickArgs a(tick, vl);
    const pcp_pair_params pp = pair_params(fixed, p_.min_separation);
    if (pcp_place_triple(dev.ctx(), a.poses.data(), a.n, a.zx, &a.params, &pp, r.triple,
                         &r.triple_total, &r.triple_covered, r.pair, &r.pair_total, &r.pair_covered,
                         &r.single, &r.single_total, &r.single_covered, &r.base_total,
                         &r.base_covered, nullptr, nullptr, nullptr, nullptr, nullptr,
                         &r.n_selected) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    for (int i = 0; i < 3 && r.triple[0] >= 0; ++i)
        r.triple_pos[i] = position(tick, r.triple[i], r.triple_total);
    finish_exact(r, tick, pp.n_fixed, r.triple_pos);
    r.log = placement_triple_log(r, greedy);
    return r;
}

std::string placement_refine_log(const MobileLidarPlacement::RefineResult &r) {
    Log log(r.total_cells);
    log.title("Exchange Refinement (ZX120 + %zu Mobile, %d Locked)", r.selected.size(), r.n_locked);
    log.rule();
    log.base("start set", r.start_total, r.start_covered);
    for (size_t i = 0; i < r.moves.size(); ++i) {
        const auto &m = r.moves[i];
        log.thin();
        log.line("Move %zu: LiDAR %d from (%.2f, %.2f, %.2f) [candidate %lld] to "
                 "(%.2f, %.2f, %.2f) [candidate %lld]",
                 i + 1, m.slot + 1, m.from_pos.x, m.from_pos.y, m.from_pos.z, (long long)m.from,
                 m.to_pos.x, m.to_pos.y, m.to_pos.z, (long long)m.to);
        log.score(m.total, "", m.gain, m.covered);
    }
    log.thin();
    if (r.converged)
        log.line("1-exchange optimal after %zu moves: no single move raises the total",
                 r.moves.size());
    else
        log.line("stopped after %zu moves: a better single move remains", r.moves.size());
    log.score(r.total, " over start", r.total - r.start_total, r.covered);
    for (size_t i = 0; i < r.placed.size(); ++i)
        log.mobile(i, r.placed[i], r.selected[i], "", (int)i < r.n_locked ? "  (locked)" : "");
    log.rule();
    return log.take();
}

MobileLidarPlacement::RefineResult MobileLidarPlacement::refine(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl, const std::vector<int64_t> &start,
    int n_locked, int max_moves) {
    RefineResult r;
    err_.clear();
    if (!tick.ran) return r;
    if (start.empty() || start.size() > PCP_PLACE_MAX) {
        err_ = "refine: the start set holds no sensor or more than PCP_PLACE_MAX";
        return r;
    }
    const TickArgs a(tick, vl);
    pcp_refine_params rp{};
    rp.k = (int32_t)start.size();
    rp.n_locked = n_locked;
    rp.max_moves = max_moves;
    rp.min_separation = p_.min_separation;
    for (size_t i = 0; i < start.size(); ++i) rp.start[i] = start[i];
    int64_t sel[PCP_PLACE_MAX], from[PCP_REFINE_MAX_MOVES], to[PCP_REFINE_MAX_MOVES];
    int32_t slot[PCP_REFINE_MAX_MOVES], cov[PCP_REFINE_MAX_MOVES], nm = 0, conv = 0;
    double tot[PCP_REFINE_MAX_MOVES];
    if (pcp_place_refine(dev.ctx(), a.poses.data(), a.n, a.zx, &a.params, &rp, sel, &r.total,
                         &r.covered, &r.start_total, &r.start_covered, slot, from, to, tot, cov,
                         nullptr, nullptr, nullptr, &nm, &conv) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.converged = conv != 0;
    r.start = start;
    r.n_locked = n_locked;
    r.total_cells = tick.report.total_cells;
    double before = r.start_total;
    for (int32_t m = 0; m < nm; ++m) {
        Move q;
        q.slot = slot[m];
        q.from = from[m];
        q.to = to[m];
        q.from_pos = tick.candidates[(size_t)from[m]];
        q.to_pos = tick.candidates[(size_t)to[m]];
        q.total = tot[m];
        q.gain = tot[m] - before;
        q.covered = cov[m];
        before = tot[m];
        r.moves.push_back(q);
    }
    for (size_t i = 0; i < start.size(); ++i) {
        const Position p = position(tick, sel[i], r.total);
        r.selected.push_back(sel[i]);
        r.placed.push_back(p);
    }
    r.log = placement_refine_log(r);
    return r;
}

std::string placement_aimed_log(const MobileLidarPlacement::AimedResult &r) {
    const double deg = 180.0 / 3.14159265358979323846;
    Log log(r.total_cells);
    log.title("Aimed LiDAR Placement (ZX120 + %d Fixed + %zu Mobile)", r.n_fixed, r.placed.size());
    log.line("Field of view: %.1f x %.1f deg", r.h_fov * deg, r.v_fov * deg);
    log.rule();
    log.base(Log::zx120_with(r.n_fixed), r.base_total, r.base_covered);
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const auto &p = r.placed[i];
        char aim[24];
        std::snprintf(aim, sizeof(aim), ", aim %d", (int)q.aim);
        log.thin();
        log.mobile(i, p, q.candidate, aim);
        log.line("  Heading: yaw %.1f deg, pitch %.1f deg", p.yaw * deg, p.pitch * deg);
        log.score(q.total, "", q.gain, q.covered);
    }
    log.rule();
    return log.take();
}

MobileLidarPlacement::AimedResult MobileLidarPlacement::place_aimed(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl, const AimedParams &ap,
    const std::vector<FixedAimed> &fixed) {
    AimedResult r;
    err_.clear();
    if (!tick.ran) return r;
    if (fixed.size() > PCP_PLACE_MAX || ap.aims.size() > PCP_AIM_MAX) {
        err_ = "place_aimed: more than PCP_PLACE_MAX fixed sensors or PCP_AIM_MAX aims";
        return r;
    }
    const TickArgs a(tick, vl);
    pcp_aim_params pp{};
    pp.k_max = p_.num_mobile_lidars;
    pp.n_aims = (int32_t)ap.aims.size();
    pp.n_fixed = (int32_t)fixed.size();
    pp.h_fov = ap.h_fov;
    pp.v_fov = ap.v_fov;
    pp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) {
        pp.fixed_pose[i] = fixed[i].candidate;
        pp.fixed_aim[i] = fixed[i].aim;
    }
    std::vector<double> aims(2 * ap.aims.size());
    for (size_t i = 0; i < ap.aims.size(); ++i) {
        aims[2 * i] = ap.aims[i].yaw_offset;
        aims[2 * i + 1] = ap.aims[i].pitch;
    }
    int64_t sel[PCP_PLACE_MAX];
    int32_t sel_aim[PCP_PLACE_MAX], cov[PCP_PLACE_MAX], ns = 0;
    double tot[PCP_PLACE_MAX];
    if (pcp_place_aimed(dev.ctx(), a.poses.data(), a.n, a.zx, &a.params, &pp, aims.data(), sel, sel_aim,
                        tot, cov, nullptr, nullptr, nullptr, &r.base_total, &r.base_covered,
                        &ns) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.total_cells = tick.report.total_cells;
    r.n_fixed = pp.n_fixed;
    r.h_fov = ap.h_fov;
    r.v_fov = ap.v_fov;
    greedy_rounds(tick, sel, tot, cov, ns, r.base_total, r.total_cells, r.rounds, r.placed);
    for (int32_t i = 0; i < ns; ++i) {   // which way each looks
        const Aim &aim = ap.aims[(size_t)sel_aim[i]];
        r.rounds[i].aim = sel_aim[i];
        r.placed[i].yaw += aim.yaw_offset;
        r.placed[i].pitch = aim.pitch;
    }
    r.log = placement_aimed_log(r);
    return r;
}

}  // namespace pcp
