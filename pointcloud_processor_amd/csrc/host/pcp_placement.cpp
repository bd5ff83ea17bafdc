// pcp_placement.cpp -- MobileLidarPlacement: see pcp_placement.hpp
#include "pcp_placement.hpp"

#include <cstdarg>
#include <cstdio>

namespace pcp {

static void appendf(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void appendf(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
    s += '\n';
}

std::string placement_log(const MobileLidarPlacement::Result &r) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Multi LiDAR Placement (ZX120 + %zu Mobile)", r.placed.size());
    appendf(log, "%s", rule);
    appendf(log, "Total Score (ZX120 only): %.2f", r.zx120_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.zx120_covered, tc, pct(r.zx120_covered));
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const auto &p = r.placed[i];
        appendf(log, "%s", thin);
        appendf(log, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1, p.x,
                p.y, p.z, (long long)q.candidate);
        appendf(log, "  Total Score: %.2f (gain %.2f)", q.total, q.gain);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", q.covered, tc, pct(q.covered));
    }
    appendf(log, "%s", rule);
    return log;
}

MobileLidarPlacement::Result MobileLidarPlacement::place(
    Device &dev, const SimplifiedDualLidarOptimizer::Result &tick,
    const SimplifiedDualLidarOptimizer::Params &vl) {
    Result r;
    err_.clear();
    if (!tick.ran) return r;
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
    const pcp_place_params pp{p_.num_mobile_lidars, 0, p_.min_separation};
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    int64_t sel[PCP_PLACE_MAX];
    double tot[PCP_PLACE_MAX];
    int32_t cov[PCP_PLACE_MAX], ns = 0;
    if (pcp_place_sensors(dev.ctx(), poses.data(), n, zx, &p, &pp, sel, tot, cov, nullptr, nullptr,
                          nullptr, &r.zx120_total, &r.zx120_covered, &ns) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.total_cells = tick.report.total_cells;
    double before = r.zx120_total;
    for (int32_t i = 0; i < ns; ++i) {
        Round q;
        q.candidate = sel[i];
        q.total = tot[i];
        q.gain = tot[i] - before;
        q.covered = cov[i];
        q.coverage_ratio = r.total_cells > 0 ? (double)cov[i] / r.total_cells : 0.0;
        before = tot[i];
        r.rounds.push_back(q);
        r.placed.push_back(tick.candidates[(size_t)sel[i]]);
        r.placed.back().total_score = tot[i];
    }
    r.log = placement_log(r);
    return r;
}

std::string placement_pair_log(const MobileLidarPlacement::PairResult &r,
                               const MobileLidarPlacement::Result *greedy) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Exact Pair Placement (ZX120 + %d Fixed + %d Mobile)", r.n_fixed, r.n_selected);
    appendf(log, "%s", rule);
    appendf(log, "Total Score (ZX120%s): %.2f", r.n_fixed ? " + fixed" : " only", r.base_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.base_covered, tc, pct(r.base_covered));
    appendf(log, "%s", thin);
    if (r.single >= 0) {
        const auto &p = r.single_pos;
        appendf(log, "Best Single Position: (%.2f, %.2f, %.2f)  [candidate %lld]", p.x, p.y, p.z,
                (long long)r.single);
        appendf(log, "  Total Score: %.2f (gain %.2f)", r.single_total,
                r.single_total - r.base_total);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.single_covered, tc,
                pct(r.single_covered));
    } else {
        appendf(log, "Best Single Position: none admissible");
    }
    appendf(log, "%s", thin);
    if (r.pair[0] >= 0) {
        for (int i = 0; i < 2; ++i) {
            const auto &p = r.pair_pos[i];
            appendf(log, "Best Pair LiDAR %d Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1,
                    p.x, p.y, p.z, (long long)r.pair[i]);
        }
        appendf(log, "  Total Score: %.2f (gain over single %.2f)", r.pair_total,
                r.pair_total - r.single_total);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.pair_covered, tc,
                pct(r.pair_covered));
        if (greedy && greedy->ran && greedy->rounds.size() >= 2)
            appendf(log, "  Greedy pair [candidates %lld, %lld]: %.2f (exact pair gains %.2f)",
                    (long long)greedy->rounds[0].candidate, (long long)greedy->rounds[1].candidate,
                    greedy->rounds[1].total, r.pair_total - greedy->rounds[1].total);
    } else {
        appendf(log, "Best Pair: no admissible pair");
    }
    appendf(log, "%s", rule);
    return log;
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
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
    pcp_pair_params pp{};
    pp.n_fixed = (int32_t)fixed.size();
    pp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) pp.fixed[i] = fixed[i];
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    if (pcp_place_pair(dev.ctx(), poses.data(), n, zx, &p, &pp, r.pair, &r.pair_total,
                       &r.pair_covered, &r.single, &r.single_total, &r.single_covered,
                       &r.base_total, &r.base_covered, nullptr, nullptr, nullptr, nullptr,
                       &r.n_selected) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.n_fixed = pp.n_fixed;
    r.total_cells = tick.report.total_cells;
    if (r.single >= 0) {
        r.single_pos = tick.candidates[(size_t)r.single];
        r.single_pos.total_score = r.single_total;
    }
    for (int i = 0; i < 2 && r.pair[0] >= 0; ++i) {
        r.pair_pos[i] = tick.candidates[(size_t)r.pair[i]];
        r.pair_pos[i].total_score = r.pair_total;
    }
    if (r.n_selected == 2) r.placed = {r.pair_pos[0], r.pair_pos[1]};
    if (r.n_selected == 1) r.placed = {r.single_pos};
    r.log = placement_pair_log(r, greedy);
    return r;
}

std::string placement_triple_log(const MobileLidarPlacement::TripleResult &r,
                                 const MobileLidarPlacement::Result *greedy) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Exact Triple Placement (ZX120 + %d Fixed + %d Mobile)", r.n_fixed, r.n_selected);
    appendf(log, "%s", rule);
    appendf(log, "Total Score (ZX120%s): %.2f", r.n_fixed ? " + fixed" : " only", r.base_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.base_covered, tc, pct(r.base_covered));
    appendf(log, "%s", thin);
    if (r.single >= 0) {
        const auto &p = r.single_pos;
        appendf(log, "Best Single Position: (%.2f, %.2f, %.2f)  [candidate %lld]", p.x, p.y, p.z,
                (long long)r.single);
        appendf(log, "  Total Score: %.2f (gain %.2f)", r.single_total,
                r.single_total - r.base_total);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.single_covered, tc,
                pct(r.single_covered));
    } else {
        appendf(log, "Best Single Position: none admissible");
    }
    appendf(log, "%s", thin);
    if (r.pair[0] >= 0) {
        for (int i = 0; i < 2; ++i) {
            const auto &p = r.pair_pos[i];
            appendf(log, "Best Pair LiDAR %d Position: (%.2f, %.2f, %.2f)  [candidate %lld]", i + 1,
                    p.x, p.y, p.z, (long long)r.pair[i]);
        }
        appendf(log, "  Total Score: %.2f (gain over single %.2f)", r.pair_total,
                r.pair_total - r.single_total);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.pair_covered, tc,
                pct(r.pair_covered));
    } else {
        appendf(log, "Best Pair: no admissible pair");
    }
    appendf(log, "%s", thin);
    if (r.triple[0] >= 0) {
        for (int i = 0; i < 3; ++i) {
            const auto &p = r.triple_pos[i];
            appendf(log, "Best Triple LiDAR %d Position: (%.2f, %.2f, %.2f)  [candidate %lld]",
                    i + 1, p.x, p.y, p.z, (long long)r.triple[i]);
        }
        appendf(log, "  Total Score: %.2f (gain over pair %.2f)", r.triple_total,
                r.triple_total - r.pair_total);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.triple_covered, tc,
                pct(r.triple_covered));
        if (greedy && greedy->ran && greedy->rounds.size() >= 3)
            appendf(log,
                    "  Greedy triple [candidates %lld, %lld, %lld]: %.2f (exact triple gains %.2f)",
                    (long long)greedy->rounds[0].candidate, (long long)greedy->rounds[1].candidate,
                    (long long)greedy->rounds[2].candidate, greedy->rounds[2].total,
                    r.triple_total - greedy->rounds[2].total);
    } else {
        appendf(log, "Best Triple: no admissible triple");
    }
    appendf(log, "%s", rule);
    return log;
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
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
    pcp_pair_params pp{};
    pp.n_fixed = (int32_t)fixed.size();
    pp.min_separation = p_.min_separation;
    for (size_t i = 0; i < fixed.size(); ++i) pp.fixed[i] = fixed[i];
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    if (pcp_place_triple(dev.ctx(), poses.data(), n, zx, &p, &pp, r.triple, &r.triple_total,
                         &r.triple_covered, r.pair, &r.pair_total, &r.pair_covered, &r.single,
                         &r.single_total, &r.single_covered, &r.base_total, &r.base_covered,
                         nullptr, nullptr, nullptr, nullptr, nullptr, &r.n_selected) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.n_fixed = pp.n_fixed;
    r.total_cells = tick.report.total_cells;
    if (r.single >= 0) {
        r.single_pos = tick.candidates[(size_t)r.single];
        r.single_pos.total_score = r.single_total;
    }
    for (int i = 0; i < 2 && r.pair[0] >= 0; ++i) {
        r.pair_pos[i] = tick.candidates[(size_t)r.pair[i]];
        r.pair_pos[i].total_score = r.pair_total;
    }
    for (int i = 0; i < 3 && r.triple[0] >= 0; ++i) {
        r.triple_pos[i] = tick.candidates[(size_t)r.triple[i]];
        r.triple_pos[i].total_score = r.triple_total;
    }
    if (r.n_selected == 3) r.placed = {r.triple_pos[0], r.triple_pos[1], r.triple_pos[2]};
    if (r.n_selected == 2) r.placed = {r.pair_pos[0], r.pair_pos[1]};
    if (r.n_selected == 1) r.placed = {r.single_pos};
    r.log = placement_triple_log(r, greedy);
    return r;
}

std::string placement_refine_log(const MobileLidarPlacement::RefineResult &r) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Exchange Refinement (ZX120 + %zu Mobile, %d Locked)", r.selected.size(),
            r.n_locked);
    appendf(log, "%s", rule);
    appendf(log, "Total Score (start set): %.2f", r.start_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.start_covered, tc, pct(r.start_covered));
    for (size_t i = 0; i < r.moves.size(); ++i) {
        const auto &m = r.moves[i];
        appendf(log, "%s", thin);
        appendf(log, "Move %zu: LiDAR %d from (%.2f, %.2f, %.2f) [candidate %lld] to "
                     "(%.2f, %.2f, %.2f) [candidate %lld]",
                i + 1, m.slot + 1, m.from_pos.x, m.from_pos.y, m.from_pos.z, (long long)m.from,
                m.to_pos.x, m.to_pos.y, m.to_pos.z, (long long)m.to);
        appendf(log, "  Total Score: %.2f (gain %.2f)", m.total, m.gain);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", m.covered, tc, pct(m.covered));
    }
    appendf(log, "%s", thin);
    if (r.converged)
        appendf(log, "1-exchange optimal after %zu moves: no single move raises the total",
                r.moves.size());
    else
        appendf(log, "stopped after %zu moves: a better single move remains", r.moves.size());
    appendf(log, "  Total Score: %.2f (gain over start %.2f)", r.total, r.total - r.start_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.covered, tc, pct(r.covered));
    for (size_t i = 0; i < r.placed.size(); ++i) {
        const auto &p = r.placed[i];
        appendf(log, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld]%s", i + 1,
                p.x, p.y, p.z, (long long)r.selected[i], (int)i < r.n_locked ? "  (locked)" : "");
    }
    appendf(log, "%s", rule);
    return log;
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
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
    pcp_refine_params rp{};
    rp.k = (int32_t)start.size();
    rp.n_locked = n_locked;
    rp.max_moves = max_moves;
    rp.min_separation = p_.min_separation;
    for (size_t i = 0; i < start.size(); ++i) rp.start[i] = start[i];
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    int64_t sel[PCP_PLACE_MAX], from[PCP_REFINE_MAX_MOVES], to[PCP_REFINE_MAX_MOVES];
    int32_t slot[PCP_REFINE_MAX_MOVES], cov[PCP_REFINE_MAX_MOVES], nm = 0, conv = 0;
    double tot[PCP_REFINE_MAX_MOVES];
    if (pcp_place_refine(dev.ctx(), poses.data(), n, zx, &p, &rp, sel, &r.total, &r.covered,
                         &r.start_total, &r.start_covered, slot, from, to, tot, cov, nullptr,
                         nullptr, nullptr, &nm, &conv) != PCP_OK) {
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
        r.selected.push_back(sel[i]);
        r.placed.push_back(tick.candidates[(size_t)sel[i]]);
        r.placed.back().total_score = r.total;
    }
    r.log = placement_refine_log(r);
    return r;
}

std::string placement_aimed_log(const MobileLidarPlacement::AimedResult &r) {
    std::string log;
    const int tc = r.total_cells;
    auto pct = [tc](int v) { return tc > 0 ? (double)v / tc * 100.0 : 0.0; };
    const double deg = 180.0 / 3.14159265358979323846;
    const char *rule = "========================================";
    const char *thin = "----------------------------------------";
    appendf(log, "%s", rule);
    appendf(log, "Aimed LiDAR Placement (ZX120 + %d Fixed + %zu Mobile)", r.n_fixed,
            r.placed.size());
    appendf(log, "Field of view: %.1f x %.1f deg", r.h_fov * deg, r.v_fov * deg);
    appendf(log, "%s", rule);
    appendf(log, "Total Score (ZX120%s): %.2f", r.n_fixed ? " + fixed" : " only", r.base_total);
    appendf(log, "  Covered cells: %d of %d (%.1f%%)", r.base_covered, tc, pct(r.base_covered));
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        const auto &q = r.rounds[i];
        const auto &p = r.placed[i];
        appendf(log, "%s", thin);
        appendf(log, "Mobile LiDAR %zu Position: (%.2f, %.2f, %.2f)  [candidate %lld, aim %d]",
                i + 1, p.x, p.y, p.z, (long long)q.candidate, (int)q.aim);
        appendf(log, "  Heading: yaw %.1f deg, pitch %.1f deg", p.yaw * deg, p.pitch * deg);
        appendf(log, "  Total Score: %.2f (gain %.2f)", q.total, q.gain);
        appendf(log, "  Covered cells: %d of %d (%.1f%%)", q.covered, tc, pct(q.covered));
    }
    appendf(log, "%s", rule);
    return log;
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
    const double zx[5] = {tick.zx120.x, tick.zx120.y, tick.zx120.z, tick.zx120.pitch,
                          tick.zx120.yaw};
    const pcp_vl_params p{vl.grid_resolution, vl.sensor_height, vl.search_radius, vl.max_distance,
                          vl.num_candidates,  vl.vertical_layers};
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
    for (size_t a = 0; a < ap.aims.size(); ++a) {
        aims[2 * a] = ap.aims[a].yaw_offset;
        aims[2 * a + 1] = ap.aims[a].pitch;
    }
    const size_t n = tick.candidates.size();
    std::vector<double> poses(5 * n);
    for (size_t i = 0; i < n; ++i) {
        const auto &c = tick.candidates[i];
        poses[5 * i] = c.x;
        poses[5 * i + 1] = c.y;
        poses[5 * i + 2] = c.z;
        poses[5 * i + 3] = c.pitch;
        poses[5 * i + 4] = c.yaw;
    }
    int64_t sel[PCP_PLACE_MAX];
    int32_t sel_aim[PCP_PLACE_MAX], cov[PCP_PLACE_MAX], ns = 0;
    double tot[PCP_PLACE_MAX];
    if (pcp_place_aimed(dev.ctx(), poses.data(), n, zx, &p, &pp, aims.data(), sel, sel_aim, tot, cov,
                        nullptr, nullptr, nullptr, &r.base_total, &r.base_covered,
                        &ns) != PCP_OK) {
        err_ = dev.error();
        return r;
    }
    r.ran = true;
    r.total_cells = tick.report.total_cells;
    r.n_fixed = pp.n_fixed;
    r.h_fov = ap.h_fov;
    r.v_fov = ap.v_fov;
    double before = r.base_total;
    for (int32_t i = 0; i < ns; ++i) {
        AimedRound q;
        q.candidate = sel[i];
        q.aim = sel_aim[i];
        q.total = tot[i];
        q.gain = tot[i] - before;
        q.covered = cov[i];
        q.coverage_ratio = r.total_cells > 0 ? (double)cov[i] / r.total_cells : 0.0;
        before = tot[i];
        r.rounds.push_back(q);
        r.placed.push_back(tick.candidates[(size_t)sel[i]]);
        r.placed.back().yaw += ap.aims[(size_t)sel_aim[i]].yaw_offset;
        r.placed.back().pitch = ap.aims[(size_t)sel_aim[i]].pitch;
        r.placed.back().total_score = tot[i];
    }
    r.log = placement_aimed_log(r);
    return r;
}

}  // namespace pcp
