// placement_host_selftest.cpp -- what MobileLidarPlacement (pcp_placement.hpp) hands to the C ABI
// and makes of its answers, on the CPU.  Linked from pcp_nodes.cpp, pcp_placement.cpp, the shell
// tests' mock_pcp.cpp and the five pcp_place_* entry points below, which print what they were
// given and return the answers a case has set.  The program prints every call's arguments, every
// field of the result, lastError() and the log; tests/test_placement_host.py compares its output
// with tests/golden/placement_host.txt byte for byte.  Only the public surface of
// pcp_placement.hpp is used.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pcp_placement.hpp"

using namespace pcp;
using Opt = SimplifiedDualLidarOptimizer;
using MLP = MobileLidarPlacement;

// ---- the canned answers and the call record -------------------------------------------------
struct Canned {
    int rc = PCP_OK;
    // pcp_place_sensors / pcp_place_aimed
    int32_t ns = 0;
    int64_t sel[PCP_PLACE_MAX] = {};
    int32_t sel_aim[PCP_PLACE_MAX] = {};
    double tot[PCP_PLACE_MAX] = {};
    int32_t cov[PCP_PLACE_MAX] = {};
    double base_total = 0;
    int32_t base_covered = 0;
    // pcp_place_pair / pcp_place_triple
    int32_t n_selected = 0;
    int64_t triple[3] = {-1, -1, -1}, pair[2] = {-1, -1}, single = -1;
    double triple_total = -INFINITY, pair_total = -INFINITY, single_total = -INFINITY;
    int32_t triple_covered = 0, pair_covered = 0, single_covered = 0;
    // pcp_place_refine
    int64_t rsel[PCP_PLACE_MAX] = {};
    double total = 0, start_total = 0;
    int32_t covered = 0, start_covered = 0, nm = 0, conv = 0;
    int32_t slot[PCP_REFINE_MAX_MOVES] = {};
    int64_t from[PCP_REFINE_MAX_MOVES] = {}, to[PCP_REFINE_MAX_MOVES] = {};
    double mtot[PCP_REFINE_MAX_MOVES] = {};
    int32_t mcov[PCP_REFINE_MAX_MOVES] = {};
};
static Canned g;
static pcp_ctx *g_ctx = nullptr;
static int g_calls = 0;

static void arr_d(const char *k, const double *v, size_t n) {
    std::printf("    %s=", k);
    for (size_t i = 0; i < n; ++i) std::printf("%s%a", i ? " " : "", v[i]);
    std::printf("\n");
}
static void arr_i64(const char *k, const int64_t *v, size_t n) {
    std::printf("    %s=", k);
    for (size_t i = 0; i < n; ++i) std::printf("%s%lld", i ? " " : "", (long long)v[i]);
    std::printf("\n");
}
static void arr_i32(const char *k, const int32_t *v, size_t n) {
    std::printf("    %s=", k);
    for (size_t i = 0; i < n; ++i) std::printf("%s%d", i ? " " : "", (int)v[i]);
    std::printf("\n");
}

// the arguments every placement call shares; an error is left in the context by a call of the
// test double that always fails
static int common(const char *fn, pcp_ctx *ctx, const double *poses5, uint64_t n,
                  const double *zx, const pcp_vl_params *p) {
    ++g_calls;
    std::printf("  call %s: ctx_ok=%d n=%llu rc=%d\n", fn, ctx == g_ctx ? 1 : 0,
                (unsigned long long)n, g.rc);
    arr_d("poses5", poses5, 5 * n);
    arr_d("zx120_pose5", zx, 5);
    std::printf("    vl: grid_resolution=%a sensor_height=%a search_radius=%a max_distance=%a "
                "num_candidates=%d vertical_layers=%d\n",
                p->grid_resolution, p->sensor_height, p->search_radius, p->max_distance,
                (int)p->num_candidates, (int)p->vertical_layers);
    if (g.rc != PCP_OK) pcp_crop_voxel(ctx, nullptr, nullptr, 0.f, nullptr, 0, nullptr, nullptr);
    return g.rc;
}
static void nulls(std::initializer_list<std::pair<const char *, const void *>> ptrs) {
    std::printf("    null:");
    for (const auto &q : ptrs) std::printf(" %s=%d", q.first, q.second == nullptr ? 1 : 0);
    std::printf("\n");
}
static void pair_params(const pcp_pair_params *pp) {
    std::printf("    pp: n_fixed=%d reserved=%d min_separation=%a\n", (int)pp->n_fixed,
                (int)pp->reserved, pp->min_separation);
    arr_i64("pp.fixed", pp->fixed, PCP_PLACE_MAX);
}

extern "C" {

int pcp_place_sensors(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                      const pcp_vl_params *p, const pcp_place_params *pp, int64_t *selected,
                      double *total_after, int32_t *covered_after, double *round_totals,
                      double *cell_score, int32_t *cell_owner, double *zx120_total,
                      int32_t *zx120_covered, int32_t *n_selected) {
    const int rc = common("pcp_place_sensors", ctx, poses5, n, zx, p);
    std::printf("    pp: k_max=%d reserved=%d min_separation=%a\n", (int)pp->k_max,
                (int)pp->reserved, pp->min_separation);
    nulls({{"round_totals", round_totals}, {"cell_score", cell_score}, {"cell_owner", cell_owner},
           {"zx120_total", zx120_total}, {"zx120_covered", zx120_covered}});
    if (rc != PCP_OK) return rc;
    for (int32_t i = 0; i < g.ns; ++i) {
        selected[i] = g.sel[i];
        total_after[i] = g.tot[i];
        covered_after[i] = g.cov[i];
    }
    if (zx120_total) *zx120_total = g.base_total;
    if (zx120_covered) *zx120_covered = g.base_covered;
    *n_selected = g.ns;
    return PCP_OK;
}

int pcp_place_pair(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                   const pcp_vl_params *p, const pcp_pair_params *pp, int64_t best_pair[2],
                   double *pair_total, int32_t *pair_covered, int64_t *best_single,
                   double *single_total, int32_t *single_covered, double *base_total,
                   int32_t *base_covered, double *pair_totals, double *single_totals,
                   double *cell_score, int32_t *cell_owner, int32_t *n_selected) {
    const int rc = common("pcp_place_pair", ctx, poses5, n, zx, p);
    pair_params(pp);
    nulls({{"pair_totals", pair_totals}, {"single_totals", single_totals},
           {"cell_score", cell_score}, {"cell_owner", cell_owner}});
    if (rc != PCP_OK) return rc;
    best_pair[0] = g.pair[0];
    best_pair[1] = g.pair[1];
    *pair_total = g.pair_total;
    *pair_covered = g.pair_covered;
    *best_single = g.single;
    *single_total = g.single_total;
    *single_covered = g.single_covered;
    *base_total = g.base_total;
    *base_covered = g.base_covered;
    *n_selected = g.n_selected;
    return PCP_OK;
}

int pcp_place_triple(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                     const pcp_vl_params *p, const pcp_pair_params *pp, int64_t best_triple[3],
                     double *triple_total, int32_t *triple_covered, int64_t best_pair[2],
                     double *pair_total, int32_t *pair_covered, int64_t *best_single,
                     double *single_total, int32_t *single_covered, double *base_total,
                     int32_t *base_covered, double *first_totals, int64_t *first_partners,
                     double *triple_totals, double *cell_score, int32_t *cell_owner,
                     int32_t *n_selected) {
    const int rc = common("pcp_place_triple", ctx, poses5, n, zx, p);
    pair_params(pp);
    nulls({{"first_totals", first_totals}, {"first_partners", first_partners},
           {"triple_totals", triple_totals}, {"cell_score", cell_score},
           {"cell_owner", cell_owner}});
    if (rc != PCP_OK) return rc;
    for (int i = 0; i < 3; ++i) best_triple[i] = g.triple[i];
    *triple_total = g.triple_total;
    *triple_covered = g.triple_covered;
    best_pair[0] = g.pair[0];
    best_pair[1] = g.pair[1];
    *pair_total = g.pair_total;
    *pair_covered = g.pair_covered;
    *best_single = g.single;
    *single_total = g.single_total;
    *single_covered = g.single_covered;
    *base_total = g.base_total;
    *base_covered = g.base_covered;
    *n_selected = g.n_selected;
    return PCP_OK;
}

int pcp_place_refine(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                     const pcp_vl_params *p, const pcp_refine_params *rp, int64_t *selected,
                     double *total, int32_t *covered, double *start_total,
                     int32_t *start_covered, int32_t *move_slot, int64_t *move_from,
                     int64_t *move_to, double *move_total, int32_t *move_covered,
                     double *swap_totals, double *cell_score, int32_t *cell_owner,
                     int32_t *n_moves, int32_t *converged) {
    const int rc = common("pcp_place_refine", ctx, poses5, n, zx, p);
    std::printf("    rp: k=%d n_locked=%d max_moves=%d reserved=%d min_separation=%a\n",
                (int)rp->k, (int)rp->n_locked, (int)rp->max_moves, (int)rp->reserved,
                rp->min_separation);
    arr_i64("rp.start", rp->start, PCP_PLACE_MAX);
    nulls({{"swap_totals", swap_totals}, {"cell_score", cell_score}, {"cell_owner", cell_owner}});
    if (rc != PCP_OK) return rc;
    for (int32_t i = 0; i < rp->k; ++i) selected[i] = g.rsel[i];
    *total = g.total;
    *covered = g.covered;
    *start_total = g.start_total;
    *start_covered = g.start_covered;
    for (int32_t m = 0; m < g.nm; ++m) {
        move_slot[m] = g.slot[m];
        move_from[m] = g.from[m];
        move_to[m] = g.to[m];
        move_total[m] = g.mtot[m];
        move_covered[m] = g.mcov[m];
    }
    *n_moves = g.nm;
    *converged = g.conv;
    return PCP_OK;
}

int pcp_place_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                    const pcp_vl_params *p, const pcp_aim_params *ap, const double *aims,
                    int64_t *selected, int32_t *selected_aim, double *total_after,
                    int32_t *covered_after, double *round_totals, double *cell_score,
                    int32_t *cell_owner, double *base_total, int32_t *base_covered,
                    int32_t *n_selected) {
    const int rc = common("pcp_place_aimed", ctx, poses5, n, zx, p);
    std::printf("    ap: k_max=%d n_aims=%d n_fixed=%d reserved=%d h_fov=%a v_fov=%a "
                "min_separation=%a\n",
                (int)ap->k_max, (int)ap->n_aims, (int)ap->n_fixed, (int)ap->reserved, ap->h_fov,
                ap->v_fov, ap->min_separation);
    arr_i64("ap.fixed_pose", ap->fixed_pose, PCP_PLACE_MAX);
    arr_i32("ap.fixed_aim", ap->fixed_aim, PCP_PLACE_MAX);
    arr_d("aims", aims, 2 * (size_t)ap->n_aims);
    nulls({{"round_totals", round_totals}, {"cell_score", cell_score}, {"cell_owner", cell_owner}});
    if (rc != PCP_OK) return rc;
    for (int32_t i = 0; i < g.ns; ++i) {
        selected[i] = g.sel[i];
        selected_aim[i] = g.sel_aim[i];
        total_after[i] = g.tot[i];
        covered_after[i] = g.cov[i];
    }
    *base_total = g.base_total;
    *base_covered = g.base_covered;
    *n_selected = g.ns;
    return PCP_OK;
}

}  // extern "C"

// ---- printing the results -------------------------------------------------------------------
static void pos(const char *k, const Opt::LidarPosition &p) {
    std::printf("    %s=(%a %a %a %a %a %a)\n", k, p.x, p.y, p.z, p.pitch, p.yaw, p.total_score);
}
static void positions(const char *k, const std::vector<Opt::LidarPosition> &v) {
    std::printf("    %s.size=%zu\n", k, v.size());
    for (size_t i = 0; i < v.size(); ++i) pos((std::string(k) + "[" + std::to_string(i) + "]").c_str(), v[i]);
}
static void text(const char *k, const std::string &s) {
    std::printf("    %s (%zu bytes):\n%s    --\n", k, s.size(), s.c_str());
}

static void dump(const MLP::Result &r) {
    std::printf("  Result: ran=%d zx120_total=%a zx120_covered=%d total_cells=%d rounds=%zu\n",
                r.ran ? 1 : 0, r.zx120_total, (int)r.zx120_covered, (int)r.total_cells,
                r.rounds.size());
    for (const auto &q : r.rounds)
        std::printf("    round: candidate=%lld total=%a gain=%a covered=%d coverage_ratio=%a\n",
                    (long long)q.candidate, q.total, q.gain, (int)q.covered, q.coverage_ratio);
    positions("placed", r.placed);
    text("log", r.log);
}
static void dump(const MLP::PairResult &r) {
    std::printf("  PairResult: ran=%d n_selected=%d pair=[%lld %lld] pair_total=%a pair_covered=%d "
                "single=%lld single_total=%a single_covered=%d base_total=%a base_covered=%d "
                "n_fixed=%d total_cells=%d\n",
                r.ran ? 1 : 0, (int)r.n_selected, (long long)r.pair[0], (long long)r.pair[1],
                r.pair_total, (int)r.pair_covered, (long long)r.single, r.single_total,
                (int)r.single_covered, r.base_total, (int)r.base_covered, (int)r.n_fixed,
                (int)r.total_cells);
    positions("placed", r.placed);
    pos("pair_pos[0]", r.pair_pos[0]);
    pos("pair_pos[1]", r.pair_pos[1]);
    pos("single_pos", r.single_pos);
    text("log", r.log);
}
static void dump(const MLP::TripleResult &r) {
    std::printf("  TripleResult: ran=%d n_selected=%d triple=[%lld %lld %lld] triple_total=%a "
                "triple_covered=%d pair=[%lld %lld] pair_total=%a pair_covered=%d single=%lld "
                "single_total=%a single_covered=%d base_total=%a base_covered=%d n_fixed=%d "
                "total_cells=%d\n",
                r.ran ? 1 : 0, (int)r.n_selected, (long long)r.triple[0], (long long)r.triple[1],
                (long long)r.triple[2], r.triple_total, (int)r.triple_covered, (long long)r.pair[0],
                (long long)r.pair[1], r.pair_total, (int)r.pair_covered, (long long)r.single,
                r.single_total, (int)r.single_covered, r.base_total, (int)r.base_covered,
                (int)r.n_fixed, (int)r.total_cells);
    positions("placed", r.placed);
    for (int i = 0; i < 3; ++i) pos(("triple_pos[" + std::to_string(i) + "]").c_str(), r.triple_pos[i]);
    pos("pair_pos[0]", r.pair_pos[0]);
    pos("pair_pos[1]", r.pair_pos[1]);
    pos("single_pos", r.single_pos);
    text("log", r.log);
}
static void dump(const MLP::RefineResult &r) {
    std::printf("  RefineResult: ran=%d converged=%d n_locked=%d start_total=%a total=%a "
                "start_covered=%d covered=%d total_cells=%d moves=%zu\n",
                r.ran ? 1 : 0, r.converged ? 1 : 0, (int)r.n_locked, r.start_total, r.total,
                (int)r.start_covered, (int)r.covered, (int)r.total_cells, r.moves.size());
    arr_i64("start", r.start.data(), r.start.size());
    arr_i64("selected", r.selected.data(), r.selected.size());
    for (const auto &m : r.moves) {
        std::printf("    move: slot=%d from=%lld to=%lld total=%a gain=%a covered=%d\n", (int)m.slot,
                    (long long)m.from, (long long)m.to, m.total, m.gain, (int)m.covered);
        pos("from_pos", m.from_pos);
        pos("to_pos", m.to_pos);
    }
    positions("placed", r.placed);
    text("log", r.log);
}
static void dump(const MLP::AimedResult &r) {
    std::printf("  AimedResult: ran=%d base_total=%a base_covered=%d n_fixed=%d total_cells=%d "
                "h_fov=%a v_fov=%a rounds=%zu\n",
                r.ran ? 1 : 0, r.base_total, (int)r.base_covered, (int)r.n_fixed,
                (int)r.total_cells, r.h_fov, r.v_fov, r.rounds.size());
    for (const auto &q : r.rounds)
        std::printf("    round: candidate=%lld aim=%d total=%a gain=%a covered=%d "
                    "coverage_ratio=%a\n",
                    (long long)q.candidate, (int)q.aim, q.total, q.gain, (int)q.covered,
                    q.coverage_ratio);
    positions("placed", r.placed);
    text("log", r.log);
}

// ---- the cases ------------------------------------------------------------------------------
static void begin(const char *name) {
    std::printf("== %s\n", name);
    g = Canned{};
    g_calls = 0;
}
template <class R>
static void end(const MLP &pl, const R &r) {
    dump(r);
    std::printf("  calls=%d lastError=\"%s\"\n", g_calls, pl.lastError().c_str());
}

// 7 candidates, every x, y, z, pitch and yaw a value of its own
static Opt::Result make_tick(int total_cells) {
    Opt::Result t;
    t.ran = true;
    t.zx120.x = 0.55;
    t.zx120.y = -0.4;
    t.zx120.z = 3.5;
    t.zx120.pitch = -0.31;
    t.zx120.yaw = 0.77;
    for (int i = 0; i < 7; ++i) {
        Opt::LidarPosition c;
        c.x = 1.25 + 0.7 * i;
        c.y = -3.5 + 1.1 * i * i;
        c.z = 2.05 + 0.13 * i;
        c.pitch = -1.2 + 0.09 * i;
        c.yaw = -2.9 + 0.83 * i;
        c.total_score = 10.5 + i;
        t.candidates.push_back(c);
    }
    t.report.total_cells = total_cells;
    return t;
}

static void greedy_answer(int ns) {
    static const int64_t sel[3] = {4, 1, 6};
    static const double tot[3] = {31.25, 38.5, 39.125};
    static const int32_t cov[3] = {22, 29, 31};
    g.base_total = 17.75;
    g.base_covered = 13;
    g.ns = ns;
    for (int i = 0; i < ns; ++i) {
        g.sel[i] = sel[i];
        g.tot[i] = tot[i];
        g.cov[i] = cov[i];
    }
}

// n_selected 3, 2, 1, 0: what the exact searches return when that many sensors are worth placing;
// have_triple / have_pair: whether an admissible one exists at all
static void exact_answer(int n_selected, bool have_single, bool have_pair, bool have_triple) {
    g.base_total = 17.75;
    g.base_covered = 13;
    g.n_selected = n_selected;
    if (have_single) {
        g.single = 4;
        g.single_total = 31.25;
        g.single_covered = 22;
    }
    if (have_pair) {
        g.pair[0] = 2;
        g.pair[1] = 5;
        g.pair_total = n_selected >= 2 ? 39.75 : 30.5;
        g.pair_covered = 30;
    }
    if (have_triple) {
        g.triple[0] = 0;
        g.triple[1] = 3;
        g.triple[2] = 5;
        g.triple_total = n_selected >= 3 ? 41.0625 : 29.5;
        g.triple_covered = 33;
    }
}

int main() {
    Device dev(0);
    g_ctx = dev.ctx();
    const Opt::Result tick = make_tick(40), tick0 = make_tick(0), no_tick{};
    Opt::Params vl;
    vl.grid_resolution = 0.125;
    vl.sensor_height = 1.35;
    vl.search_radius = 2.75;
    vl.max_distance = 12.5;
    vl.num_candidates = 7;
    vl.vertical_layers = 9;
    MLP::Params mp;
    mp.num_mobile_lidars = 3;
    mp.min_separation = 1.75;
    MLP pl(mp);
    const std::vector<int64_t> fixed2 = {6, 1};
    const std::vector<int64_t> too_many(PCP_PLACE_MAX + 1, 0);

    // ---- place
    begin("place: 0 rounds");
    greedy_answer(0);
    end(pl, pl.place(dev, tick, vl));
    begin("place: 3 rounds");
    greedy_answer(3);
    const MLP::Result greedy3 = pl.place(dev, tick, vl);
    end(pl, greedy3);
    std::printf("  placement_log(r) == r.log: %d\n", placement_log(greedy3) == greedy3.log ? 1 : 0);
    begin("place: 2 rounds");
    greedy_answer(2);
    const MLP::Result greedy2 = pl.place(dev, tick, vl);
    end(pl, greedy2);
    begin("place: 1 round");
    greedy_answer(1);
    const MLP::Result greedy1 = pl.place(dev, tick, vl);
    end(pl, greedy1);
    begin("place: total_cells = 0");
    greedy_answer(2);
    end(pl, pl.place(dev, tick0, vl));
    begin("place: the call fails");
    g.rc = PCP_E_INVALID;
    end(pl, pl.place(dev, tick, vl));
    begin("place: tick not run (after a failure: the error is cleared)");
    end(pl, pl.place(dev, no_tick, vl));
    MLP::Result greedy_not_ran = greedy3;   // (the log's own test of greedy->ran)
    greedy_not_ran.ran = false;

    // ---- place_pair
    begin("place_pair: n_selected 2, greedy of 3 rounds, no fixed");
    exact_answer(2, true, true, false);
    end(pl, pl.place_pair(dev, tick, vl, {}, &greedy3));
    begin("place_pair: n_selected 2, greedy of 1 round, 2 fixed");
    exact_answer(2, true, true, false);
    end(pl, pl.place_pair(dev, tick, vl, fixed2, &greedy1));
    begin("place_pair: n_selected 2, greedy that did not run");
    exact_answer(2, true, true, false);
    end(pl, pl.place_pair(dev, tick, vl, {}, &greedy_not_ran));
    begin("place_pair: n_selected 2, no greedy (the defaults)");
    exact_answer(2, true, true, false);
    {
        const MLP::PairResult r = pl.place_pair(dev, tick, vl);
        end(pl, r);
        std::printf("  placement_pair_log(r) == r.log: %d\n", placement_pair_log(r) == r.log ? 1 : 0);
    }
    begin("place_pair: n_selected 1, the pair loses to the single");
    exact_answer(1, true, true, false);
    end(pl, pl.place_pair(dev, tick, vl, fixed2, &greedy3));
    begin("place_pair: n_selected 1, no admissible pair");
    exact_answer(1, true, false, false);
    end(pl, pl.place_pair(dev, tick, vl, fixed2, nullptr));
    begin("place_pair: n_selected 0, no admissible single");
    exact_answer(0, false, false, false);
    end(pl, pl.place_pair(dev, tick, vl, {}, &greedy3));
    begin("place_pair: total_cells = 0");
    exact_answer(2, true, true, false);
    end(pl, pl.place_pair(dev, tick0, vl, {}, &greedy3));
    begin("place_pair: PCP_PLACE_MAX + 1 fixed");
    end(pl, pl.place_pair(dev, tick, vl, too_many));
    begin("place_pair: the call fails");
    g.rc = PCP_E_INVALID;
    end(pl, pl.place_pair(dev, tick, vl, fixed2));
    begin("place_pair: tick not run");
    end(pl, pl.place_pair(dev, no_tick, vl, fixed2));

    // ---- place_triple
    begin("place_triple: n_selected 3, greedy of 3 rounds, no fixed");
    exact_answer(3, true, true, true);
    end(pl, pl.place_triple(dev, tick, vl, {}, &greedy3));
    begin("place_triple: n_selected 3, greedy of 2 rounds, 2 fixed");
    exact_answer(3, true, true, true);
    end(pl, pl.place_triple(dev, tick, vl, fixed2, &greedy2));
    begin("place_triple: n_selected 3, greedy that did not run");
    exact_answer(3, true, true, true);
    end(pl, pl.place_triple(dev, tick, vl, {}, &greedy_not_ran));
    begin("place_triple: n_selected 3, no greedy (the defaults)");
    exact_answer(3, true, true, true);
    {
        const MLP::TripleResult r = pl.place_triple(dev, tick, vl);
        end(pl, r);
        std::printf("  placement_triple_log(r) == r.log: %d\n",
                    placement_triple_log(r) == r.log ? 1 : 0);
    }
    begin("place_triple: n_selected 2, the triple loses to the pair");
    exact_answer(2, true, true, true);
    end(pl, pl.place_triple(dev, tick, vl, {}, &greedy3));
    begin("place_triple: n_selected 2, no admissible triple while a pair exists");
    exact_answer(2, true, true, false);
    end(pl, pl.place_triple(dev, tick, vl, fixed2, &greedy3));
    begin("place_triple: n_selected 1, no admissible pair");
    exact_answer(1, true, false, false);
    end(pl, pl.place_triple(dev, tick, vl, fixed2, nullptr));
    begin("place_triple: n_selected 0, no admissible single");
    exact_answer(0, false, false, false);
    end(pl, pl.place_triple(dev, tick, vl, {}, &greedy3));
    begin("place_triple: total_cells = 0");
    exact_answer(3, true, true, true);
    end(pl, pl.place_triple(dev, tick0, vl, {}, &greedy3));
    begin("place_triple: PCP_PLACE_MAX + 1 fixed");
    end(pl, pl.place_triple(dev, tick, vl, too_many));
    begin("place_triple: the call fails");
    g.rc = PCP_E_INVALID;
    end(pl, pl.place_triple(dev, tick, vl, fixed2));
    begin("place_triple: tick not run");
    end(pl, pl.place_triple(dev, no_tick, vl, fixed2));

    // ---- refine
    const std::vector<int64_t> start3 = {4, 1, 6};
    auto refine_answer = [&](int nm, int conv) {
        g.start_total = 39.125;
        g.start_covered = 31;
        g.rsel[0] = 4;
        g.rsel[1] = nm >= 1 ? 2 : 1;
        g.rsel[2] = nm >= 2 ? 0 : 6;
        g.nm = nm;
        g.conv = conv;
        const int32_t slot[2] = {1, 2};
        const int64_t from[2] = {1, 6}, to[2] = {2, 0};
        const double mtot[2] = {40.5, 40.8125};
        const int32_t mcov[2] = {32, 34};
        for (int m = 0; m < nm; ++m) {
            g.slot[m] = slot[m];
            g.from[m] = from[m];
            g.to[m] = to[m];
            g.mtot[m] = mtot[m];
            g.mcov[m] = mcov[m];
        }
        g.total = nm ? mtot[nm - 1] : g.start_total;
        g.covered = nm ? mcov[nm - 1] : g.start_covered;
    };
    begin("refine: 0 moves, converged (the defaults)");
    refine_answer(0, 1);
    {
        const MLP::RefineResult r = pl.refine(dev, tick, vl, start3);
        end(pl, r);
        std::printf("  placement_refine_log(r) == r.log: %d\n",
                    placement_refine_log(r) == r.log ? 1 : 0);
    }
    begin("refine: 2 moves, not converged, n_locked 1, max_moves 2");
    refine_answer(2, 0);
    end(pl, pl.refine(dev, tick, vl, start3, 1, 2));
    begin("refine: 1 move, converged, total_cells = 0");
    refine_answer(1, 1);
    end(pl, pl.refine(dev, tick0, vl, start3, 0, 5));
    begin("refine: an empty start");
    end(pl, pl.refine(dev, tick, vl, {}));
    begin("refine: PCP_PLACE_MAX + 1 start entries");
    end(pl, pl.refine(dev, tick, vl, too_many));
    begin("refine: the call fails");
    g.rc = PCP_E_INVALID;
    end(pl, pl.refine(dev, tick, vl, start3, 1, 2));
    begin("refine: tick not run");
    end(pl, pl.refine(dev, no_tick, vl, start3));

    // ---- place_aimed
    MLP::AimedParams ap;
    ap.h_fov = 1.5;
    ap.v_fov = 0.625;
    ap.aims.resize(3);
    ap.aims[0].yaw_offset = -0.75;
    ap.aims[0].pitch = -0.4;
    ap.aims[1].yaw_offset = 0.35;
    ap.aims[1].pitch = 0.2;
    ap.aims[2].yaw_offset = 2.1;
    ap.aims[2].pitch = -1.1;
    MLP::FixedAimed fa;
    fa.candidate = 5;
    fa.aim = 2;
    auto aimed_answer = [&](int ns) {
        greedy_answer(ns);
        g.sel_aim[0] = 1;
        g.sel_aim[1] = 2;
        g.sel_aim[2] = 0;
    };
    begin("place_aimed: 0 rounds (the defaults)");
    aimed_answer(0);
    {
        const MLP::AimedResult r = pl.place_aimed(dev, tick, vl, ap);
        end(pl, r);
        std::printf("  placement_aimed_log(r) == r.log: %d\n",
                    placement_aimed_log(r) == r.log ? 1 : 0);
    }
    begin("place_aimed: 2 rounds, 1 fixed aimed sensor");
    aimed_answer(2);
    end(pl, pl.place_aimed(dev, tick, vl, ap, {fa}));
    begin("place_aimed: 3 rounds, total_cells = 0");
    aimed_answer(3);
    end(pl, pl.place_aimed(dev, tick0, vl, ap));
    {
        MLP::AimedParams many = ap;
        many.aims.resize(PCP_AIM_MAX + 1);
        begin("place_aimed: PCP_AIM_MAX + 1 aims");
        end(pl, pl.place_aimed(dev, tick, vl, many));
    }
    begin("place_aimed: PCP_PLACE_MAX + 1 fixed");
    end(pl, pl.place_aimed(dev, tick, vl, ap, std::vector<MLP::FixedAimed>(PCP_PLACE_MAX + 1, fa)));
    begin("place_aimed: the call fails");
    g.rc = PCP_E_INVALID;
    end(pl, pl.place_aimed(dev, tick, vl, ap, {fa}));
    begin("place_aimed: tick not run");
    end(pl, pl.place_aimed(dev, no_tick, vl, ap, {fa}));

    // another instance's parameters reach the calls (k_max, min_separation)
    MLP other;
    other.params().num_mobile_lidars = 5;
    other.params().min_separation = 0.0;
    begin("place: another instance's parameters");
    greedy_answer(1);
    end(other, other.place(dev, tick, vl));
    begin("place_aimed: another instance's parameters");
    aimed_answer(1);
    end(other, other.place_aimed(dev, tick, vl, ap));
    std::printf("ok\n");
    return 0;
}
