// pcp_nodes_cli.cpp -- drives the C++ node cores (pcp_nodes.hpp) from files, for the parity
// tests, and runs the streaming replay benchmark (BASELINE configs[4] on one GPU).
//
//   pcp_nodes_cli filter  IN.f32 N STEP LEAF FRONT SIDE HEIGHT OUT.f32
//   pcp_nodes_cli merge   ROBOT.f32 RN ZX.f32 ZN TR(7) TZ(7) OUT.f32        (t xyz, q xyzw)
//   pcp_nodes_cli vlidar  TERRAIN.f32 TN AUX.f32 AN CELLS.f64 NORMALS.f32 CN BBOX(6) ZXT(3) NUMC
//                         MAXD OUT_TOTALS.f64 OUT_FLAGS.u8 OUT_REPORT.txt [TICKS]
//   pcp_nodes_cli place   TERRAIN.f32 TN AUX.f32 AN CELLS.f64 NORMALS.f32 CN BBOX(6) ZXT(3) NUMC
//                         MAXD KMAX MINSEP OUT_SELECTED.i64 OUT_TOTALS.f64 OUT_REPORT.txt
//   pcp_nodes_cli place_pair  (place's arguments; KMAX: the greedy placement it is compared with)
//                         OUT_SELECTED: the exact answer; OUT_TOTALS: base, single, pair
//   pcp_nodes_cli place_triple  (place's arguments; KMAX as for place_pair)
//                         OUT_SELECTED: the exact answer; OUT_TOTALS: base, single, pair, triple
//   pcp_nodes_cli place_refine  (place's arguments) [N_LOCKED [MAX_MOVES]]: KMAX sensors placed
//                         greedily, then refined by single-sensor exchanges; OUT_SELECTED: the
//                         refined set; OUT_TOTALS: start, final, then the total after each move
//   pcp_nodes_cli place_aimed  (place's arguments) H_FOV V_FOV AIMS.f64 [FIXED]: KMAX sensors of
//                         H_FOV x V_FOV radians placed greedily, every candidate searched with
//                         every aim of AIMS.f64 ([A][2] doubles: yaw offset, pitch) beside the
//                         aimed sensors already placed (FIXED: candidate,aim,candidate,aim,..);
//                         OUT_SELECTED: (candidate, aim) pairs; OUT_TOTALS: the total after each
//   pcp_nodes_cli scan    TERRAIN.f32 TN POSES(5 per sensor) NAZ NEL MAXD OUT_SCANS.bin
//   pcp_nodes_cli scan_mounted TERRAIN.f32 TN POSES(6 per sensor: x,y,z,roll,pitch,yaw) NAZ NEL
//                         MAXD ELTABLE|- OUT_SCANS.bin ... (scan's outputs; ELTABLE: NEL radians)
//                         OUT_OFFSETS.u64 OUT_BLIND.f32 OUT_MASK.u64
//   pcp_nodes_cli cover   TERRAIN.f32 TN POSES(5 per candidate, or a .f64 file of them) NAZ NEL MAXD
//                         KMAX MINSEP ROI.u8|- OUT_SELECTED.i64 OUT_OWNER.i32 OUT_BLIND.f32 [FIXED]:
//                         KMAX sensors placed by the terrain points their scans reach, within the
//                         region ROI.u8 (TN bytes, non-zero counts; -: every point), beside the
//                         candidates FIXED (c,c,..); OUT_SELECTED: candidate, gain, covered per round
//   pcp_nodes_cli cover_pair TERRAIN.f32 TN POSES NAZ NEL MAXD MINSEP ROI.u8|- OUT_SELECTED.i64
//                         OUT_OWNER.i32 OUT_BLIND.f32 [FIXED]: cover's arguments less KMAX; the
//                         exact best pair of the candidates (or the best single one where no pair
//                         adds more), the JSON line with best_pair, pair_gain, best_single, single_gain
//   pcp_nodes_cli cover_aimed TERRAIN.f32 TN POSES NAZ NEL MAXD KMAX MINSEP ROI.u8|- WAZ WEL AIMS
//                         OUT_SELECTED.i64 OUT_OWNER.i32 OUT_BLIND.f32 [FIXED]: cover with a limited
//                         field of view -- a window of WAZ columns x WEL rings of the fan at every
//                         aim of AIMS (az0,el0,az0,el0,..) of every candidate; FIXED (c,a,c,a,..):
//                         candidate and aim pairs already placed; OUT_SELECTED: candidate, aim,
//                         gain, covered per round
//   pcp_nodes_cli cover_weighted TERRAIN.f32 TN POSES NAZ NEL MAXD KMAX MINSEP WEIGHTS OUT_SELECTED.i64
//                         OUT_OWNER.i32 OUT_BLIND.f32 [FIXED]: cover by the WEIGHT of the points
//                         reached -- WEIGHTS a .u8 file (TN bytes, 0 .. 255 each, 0: outside the
//                         region) or BASE[/x0,x1,y0,y1,z0,z1,W]..: a base weight and boxes in map
//                         coordinates with theirs, a later box overriding an earlier one;
//                         OUT_SELECTED: candidate, weight gained, points gained, covered weight
//                         per round; the JSON line adds roi_weight, base_points, blind_weight
//   pcp_nodes_cli cover_refine cover's arguments [--start c,c,..] [--locked M] [--max-moves M]:
//                         the set START improved by single-sensor exchanges, its first LOCKED
//                         slots held; without --start greedy's answer of `cover` is refined in
//                         the same process (FIXED in front of it, locked); OUT_SELECTED: candidate,
//                         owned points, covered per slot; the JSON line adds n_locked,
//                         start_covered, moves [slot, from, to, covered] and converged
//   pcp_nodes_cli drivable IN.f32 N STEP TF(7) R1(2) R2(2) OUT.i8
//   pcp_nodes_cli replay  TERRAIN.f32 TN CELLS.f64 NORMALS.f32 CN BBOX(6) FRAMES POINTS
//
// Tuples are comma-separated doubles.  .f32 clouds are PointXYZRGB-like records of STEP bytes
// (terrain/aux: 32 B, x/y/z at 0/4/8).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <malloc.h>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "pcp_cover_aim_node.hpp"
#include "pcp_cover_node.hpp"
#include "pcp_cover_weight_node.hpp"
#include "pcp_nodes.hpp"
#include "pcp_placement.hpp"
#include "pcp_scan_node.hpp"

using namespace pcp;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> b;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    b.resize((size_t)n);
    if (n && std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) std::exit(2);
    std::fclose(f);
    return b;
}

static void write_file(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || (n && std::fwrite(p, 1, n, f) != n)) {
        std::fprintf(stderr, "cannot write %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

static std::vector<double> tuple(const char *s) {
    std::vector<double> v;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) v.push_back(std::strtod(tok.c_str(), nullptr));
    return v;
}

static PointCloud2 cloud_from(const std::vector<uint8_t> &raw, size_t n, uint32_t step,
                              const std::string &frame) {
    PointCloud2 m;
    m.frame_id = frame;
    m.width = (uint32_t)n;
    m.point_step = step;
    m.row_step = step * (uint32_t)n;
    m.fields = {{"x", 0}, {"y", 4}, {"z", 8}};
    m.data.assign(raw.begin(), raw.begin() + std::min(raw.size(), n * step));
    return m;
}

static Transform tf_from(const std::vector<double> &v) {
    Transform t;
    for (int i = 0; i < 3; ++i) t.t[i] = v[i];
    for (int i = 0; i < 4; ++i) t.q[i] = v[3 + i];
    return t;
}

static int cmd_filter(Device &dev, char **a) {
    const auto raw = read_file(a[0]);
    const size_t n = std::strtoull(a[1], nullptr, 10);
    SimplifiedScanMatcher::Params p;
    p.voxel_leaf_size = std::strtod(a[3], nullptr);
    p.robot_front_range = std::strtod(a[4], nullptr);
    p.robot_side_range = std::strtod(a[5], nullptr);
    p.robot_height_range = std::strtod(a[6], nullptr);
    SimplifiedScanMatcher node(dev, p);
    PointCloud2 in = cloud_from(raw, n, (uint32_t)std::strtoul(a[2], nullptr, 10), "velodyne_link");
    in.stamp = 12.5;
    PointCloud2 out = node.robotCloudCallback(in);
    if (!node.lastError().empty()) {
        std::fprintf(stderr, "filter: %s\n", node.lastError().c_str());
        return 1;
    }
    if (out.frame_id != in.frame_id || out.stamp != in.stamp || out.point_step != 16) return 3;
    write_file(a[7], out.data.data(), out.data.size());
    std::printf("{\"n_out\": %zu, \"n_cropped\": %zu}\n", out.size(), node.lastCroppedSize());
    return 0;
}

static int cmd_merge(Device &dev, char **a) {
    const auto r = read_file(a[0]), z = read_file(a[2]);
    const size_t rn = std::strtoull(a[1], nullptr, 10), zn = std::strtoull(a[3], nullptr, 10);
    GnssGicpMatcher node(dev);
    node.robotCloudCallback(make_xyz_cloud(reinterpret_cast<const float *>(r.data()), rn, "four_wheel_robot/velodyne_link"));
    node.backhoeCloudCallback(make_xyz_cloud(reinterpret_cast<const float *>(z.data()), zn, "zx120/velodyne_link"));
    const Transform tr = tf_from(tuple(a[4])), tz = tf_from(tuple(a[5]));
    auto o = node.processPointClouds(true, &tr, &tz);
    if (!node.lastError().empty()) {
        std::fprintf(stderr, "merge: %s\n", node.lastError().c_str());
        return 1;
    }
    if (o.merged.size() != o.robot_colored.size() + o.backhoe_colored.size()) return 3;
    auto none = node.processPointClouds(false, &tr, &tz);   // origin not set: nothing (:309)
    if (!none.merged.empty()) return 4;
    auto only_robot = node.processPointClouds(true, &tr, nullptr);   // zx120 TF failed
    if (only_robot.merged.size() != o.robot_colored.size()) return 5;
    write_file(a[6], o.merged.data.data(), o.merged.data.size());
    std::printf("{\"n_out\": %zu, \"robot\": %zu, \"backhoe\": %zu}\n", o.merged.size(),
                o.robot_colored.size(), o.backhoe_colored.size());
    return 0;
}

// PCP_DEVICES=d0,d1,...: the virtual-LiDAR node shards its poses over these devices (pcp_multi)
static std::unique_ptr<MultiDevice> multi_from_env() {
    const char *e = std::getenv("PCP_DEVICES");
    if (!e || !*e) return nullptr;
    std::vector<int> d;
    for (const char *p = e; *p;) {
        d.push_back(std::atoi(p));
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
    }
    return std::unique_ptr<MultiDevice>(new MultiDevice(d));
}

static int cmd_vlidar(Device &dev, char **a, int argc) {
    const auto t = read_file(a[0]), ax = read_file(a[2]), c = read_file(a[4]),
               nr = read_file(a[5]);
    const size_t tn = std::strtoull(a[1], nullptr, 10), an = std::strtoull(a[3], nullptr, 10),
                 cn = std::strtoull(a[6], nullptr, 10);
    const auto bbox = tuple(a[7]), zxt = tuple(a[8]);
    SimplifiedDualLidarOptimizer::Params p;
    p.num_candidates = std::atoi(a[9]);
    p.max_distance = std::strtod(a[10], nullptr);
    std::unique_ptr<MultiDevice> md = multi_from_env();
    std::unique_ptr<SimplifiedDualLidarOptimizer> nodep(
        md ? new SimplifiedDualLidarOptimizer(*md, p) : new SimplifiedDualLidarOptimizer(dev, p));
    SimplifiedDualLidarOptimizer &node = *nodep;
    Transform zx;
    zx.t[0] = zxt[0];
    zx.t[1] = zxt[1];
    zx.t[2] = zxt[2];
    // before any data: the early return of :455
    if (node.runOptimization(&zx).ran) return 3;
    node.terrainCallback(cloud_from(t, tn, 32, "map"));
    node.zx120PointsCallback(cloud_from(ax, an, 32, "velodyne_link"));
    std::vector<double> xyz(cn * 3);
    std::vector<float> nrm(cn * 3);
    std::memcpy(xyz.data(), c.data(), xyz.size() * 8);
    std::memcpy(nrm.data(), nr.data(), nrm.size() * 4);
    node.setExcavationGrid(xyz, nrm, bbox.data());
    if (node.runOptimization(nullptr).ran) return 4;   // TF missing
    const int ticks = argc > 14 ? std::atoi(a[14]) : 1;
    SimplifiedDualLidarOptimizer::Result r;
    for (int i = 0; i < ticks; ++i) r = node.runOptimization(&zx);   // flags carry over
    if (!r.ran) {
        std::fprintf(stderr, "vlidar: %s\n", node.lastError().c_str());
        return 1;
    }
    std::vector<double> tot(r.candidates.size());
    for (size_t i = 0; i < tot.size(); ++i) tot[i] = r.candidates[i].total_score;
    write_file(a[11], tot.data(), tot.size() * 8);
    write_file(a[12], node.cellFlags().data(), node.cellFlags().size());
    write_file(a[13], r.log.data(), r.log.size());
    std::printf("{\"n_candidates\": %zu, \"best_idx\": %lld, \"best\": [%.17g, %.17g, %.17g], "
                "\"devices\": %d, \"rccl\": %d}\n",
                r.candidates.size(), (long long)r.report.best_idx, r.best.x, r.best.y, r.best.z,
                md ? md->size() : 1, md && md->usesRccl() ? 1 : 0);
    return 0;
}

// ---- the placement commands: a tick of the virtual-LiDAR node, a search among its candidates ----
struct PlaceFront {
    SimplifiedDualLidarOptimizer::Params p;
    SimplifiedDualLidarOptimizer::Result tick;
    MobileLidarPlacement placement;   // with KMAX and MINSEP
    int failed(const char *cmd) const {   // a search that did not run
        std::fprintf(stderr, "%s: %s\n", cmd, placement.lastError().c_str());
        return 1;
    }
};
static const SimplifiedDualLidarOptimizer::Result kNoTick{};   // (every call must refuse it: 3)

// the shared arguments (vlidar's inputs, KMAX, MINSEP) and the tick; 0, or the failure's status
static int place_front(Device &dev, char **a, PlaceFront &f) {
    const auto t = read_file(a[0]), ax = read_file(a[2]), c = read_file(a[4]),
               nr = read_file(a[5]);
    const size_t tn = std::strtoull(a[1], nullptr, 10), an = std::strtoull(a[3], nullptr, 10),
                 cn = std::strtoull(a[6], nullptr, 10);
    const auto bbox = tuple(a[7]), zxt = tuple(a[8]);
    f.p.num_candidates = std::atoi(a[9]);
    f.p.max_distance = std::strtod(a[10], nullptr);
    f.placement.params().num_mobile_lidars = std::atoi(a[11]);
    f.placement.params().min_separation = std::strtod(a[12], nullptr);
    SimplifiedDualLidarOptimizer node(dev, f.p);
    Transform zx;
    for (int i = 0; i < 3; ++i) zx.t[i] = zxt[i];
    node.terrainCallback(cloud_from(t, tn, 32, "map"));
    node.zx120PointsCallback(cloud_from(ax, an, 32, "velodyne_link"));
    std::vector<double> xyz(cn * 3);
    std::vector<float> nrm(cn * 3);
    std::memcpy(xyz.data(), c.data(), xyz.size() * 8);
    std::memcpy(nrm.data(), nr.data(), nrm.size() * 4);
    node.setExcavationGrid(xyz, nrm, bbox.data());
    f.tick = node.runOptimization(&zx);
    if (!f.tick.ran) {
        std::fprintf(stderr, "place: %s\n", node.lastError().c_str());
        return 1;
    }
    return 0;
}

// OUT_SELECTED, OUT_TOTALS, OUT_REPORT
static void write_placement(char **a, const std::vector<int64_t> &sel,
                            const std::vector<double> &tot, const std::string &log) {
    write_file(a[13], sel.data(), sel.size() * 8);
    write_file(a[14], tot.data(), tot.size() * 8);
    write_file(a[15], log.data(), log.size());
}

// an exact search's answer as candidate indices (triple: null for the pair search)
static std::vector<int64_t> exact_selection(const MobileLidarPlacement::PairResult &r,
                                            const int64_t *triple = nullptr) {
    if (r.n_selected == 3 && triple) return {triple[0], triple[1], triple[2]};
    if (r.n_selected == 2) return {r.pair[0], r.pair[1]};
    if (r.n_selected == 1) return {r.single};
    return {};
}

// place: KMAX mobile sensors placed greedily; the selected candidates and the totals after each
static int cmd_place(Device &dev, char **a, int) {
    PlaceFront f;
    if (const int rc = place_front(dev, a, f)) return rc;
    if (f.placement.place(dev, kNoTick, f.p).ran) return 3;
    const auto r = f.placement.place(dev, f.tick, f.p);
    if (!r.ran) return f.failed("place");
    std::vector<int64_t> sel;
    std::vector<double> tot;
    for (const auto &q : r.rounds) sel.push_back(q.candidate);
    for (const auto &q : r.rounds) tot.push_back(q.total);
    write_placement(a, sel, tot, r.log);
    std::printf("{\"n_candidates\": %zu, \"n_selected\": %zu, \"zx120_total\": %.17g, "
                "\"zx120_covered\": %d, \"total_cells\": %d}\n",
                f.tick.candidates.size(), r.rounds.size(), r.zx120_total, r.zx120_covered,
                r.total_cells);
    return 0;
}

// place_pair: the exact best pair, compared with the first two of KMAX sensors placed greedily
static int cmd_place_pair(Device &dev, char **a, int) {
    PlaceFront f;
    if (const int rc = place_front(dev, a, f)) return rc;
    if (f.placement.place_pair(dev, kNoTick, f.p).ran) return 3;
    const auto greedy = f.placement.place(dev, f.tick, f.p);
    const auto r = f.placement.place_pair(dev, f.tick, f.p, {}, greedy.ran ? &greedy : nullptr);
    if (!r.ran) return f.failed("place_pair");
    write_placement(a, exact_selection(r), {r.base_total, r.single_total, r.pair_total}, r.log);
    std::printf("{\"n_candidates\": %zu, \"n_selected\": %d, \"best_pair\": [%lld, %lld], "
                "\"pair_covered\": %d, \"best_single\": %lld, \"single_covered\": %d, "
                "\"base_covered\": %d, \"total_cells\": %d}\n",
                f.tick.candidates.size(), r.n_selected, (long long)r.pair[0], (long long)r.pair[1],
                r.pair_covered, (long long)r.single, r.single_covered, r.base_covered,
                r.total_cells);
    return 0;
}

// place_triple: the exact best triple, compared with the first three of KMAX placed greedily
static int cmd_place_triple(Device &dev, char **a, int) {
    PlaceFront f;
    if (const int rc = place_front(dev, a, f)) return rc;
    if (f.placement.place_triple(dev, kNoTick, f.p).ran) return 3;
    const auto greedy = f.placement.place(dev, f.tick, f.p);
    const auto r = f.placement.place_triple(dev, f.tick, f.p, {}, greedy.ran ? &greedy : nullptr);
    if (!r.ran) return f.failed("place_triple");
    write_placement(a, exact_selection(r, r.triple),
                    {r.base_total, r.single_total, r.pair_total, r.triple_total}, r.log);
    std::printf("{\"n_candidates\": %zu, \"n_selected\": %d, \"best_triple\": [%lld, %lld, "
                "%lld], \"triple_covered\": %d, \"best_pair\": [%lld, %lld], "
                "\"pair_covered\": %d, \"best_single\": %lld, \"single_covered\": %d, "
                "\"base_covered\": %d, \"total_cells\": %d}\n",
                f.tick.candidates.size(), r.n_selected, (long long)r.triple[0],
                (long long)r.triple[1], (long long)r.triple[2], r.triple_covered,
                (long long)r.pair[0], (long long)r.pair[1], r.pair_covered, (long long)r.single,
                r.single_covered, r.base_covered, r.total_cells);
    return 0;
}

// place_refine: the greedy placement, then single-sensor exchanges from it
static int cmd_place_refine(Device &dev, char **a, int argc) {
    PlaceFront f;
    if (const int rc = place_front(dev, a, f)) return rc;
    if (f.placement.refine(dev, kNoTick, f.p, {0}).ran) return 3;
    const auto greedy = f.placement.place(dev, f.tick, f.p);
    if (!greedy.ran) return f.failed("place_refine");
    if (greedy.rounds.empty()) {
        std::fprintf(stderr, "place_refine: greedy placed nothing\n");
        return 1;
    }
    std::vector<int64_t> start;
    for (const auto &q : greedy.rounds) start.push_back(q.candidate);
    const int n_locked = argc > 16 ? std::atoi(a[16]) : 0;
    const int max_moves = argc > 17 ? std::atoi(a[17]) : PCP_REFINE_MAX_MOVES;
    const auto r = f.placement.refine(dev, f.tick, f.p, start, n_locked, max_moves);
    if (!r.ran) return f.failed("place_refine");
    std::vector<double> tot = {r.start_total, r.total};
    std::string moves;
    for (const auto &m : r.moves) {
        tot.push_back(m.total);
        char buf[96];
        std::snprintf(buf, sizeof(buf), "%s[%d, %lld, %lld]", moves.empty() ? "" : ", ", m.slot,
                      (long long)m.from, (long long)m.to);
        moves += buf;
    }
    std::string sel;
    for (size_t i = 0; i < r.selected.size(); ++i)
        sel += (i ? ", " : "") + std::to_string((long long)r.selected[i]);
    write_placement(a, r.selected, tot, r.log);
    std::printf("{\"n_candidates\": %zu, \"k\": %zu, \"n_locked\": %d, \"n_moves\": %zu, "
                "\"converged\": %d, \"selected\": [%s], \"moves\": [%s], "
                "\"start_covered\": %d, \"covered\": %d, \"total_cells\": %d}\n",
                f.tick.candidates.size(), r.selected.size(), r.n_locked, r.moves.size(),
                r.converged ? 1 : 0, sel.c_str(), moves.c_str(), r.start_covered, r.covered,
                r.total_cells);
    return 0;
}

// place_aimed: limited-field-of-view sensors, every candidate with every aim of the table
static int cmd_place_aimed(Device &dev, char **a, int argc) {
    PlaceFront f;
    if (const int rc = place_front(dev, a, f)) return rc;
    MobileLidarPlacement::AimedParams ap;
    ap.h_fov = std::strtod(a[16], nullptr);
    ap.v_fov = std::strtod(a[17], nullptr);
    const auto raw = read_file(a[18]);
    ap.aims.resize(raw.size() / 16);
    for (size_t i = 0; i < ap.aims.size(); ++i) {
        std::memcpy(&ap.aims[i].yaw_offset, raw.data() + 16 * i, 8);
        std::memcpy(&ap.aims[i].pitch, raw.data() + 16 * i + 8, 8);
    }
    if (f.placement.place_aimed(dev, kNoTick, f.p, ap).ran) return 3;
    std::vector<MobileLidarPlacement::FixedAimed> fixed;
    if (argc > 19) {
        const auto fx = tuple(a[19]);
        for (size_t i = 0; i + 1 < fx.size(); i += 2)
            fixed.push_back({(int64_t)fx[i], (int32_t)fx[i + 1]});
    }
    const auto r = f.placement.place_aimed(dev, f.tick, f.p, ap, fixed);
    if (!r.ran) return f.failed("place_aimed");
    std::vector<int64_t> sel;
    std::vector<double> tot;
    for (const auto &q : r.rounds) sel.insert(sel.end(), {q.candidate, (int64_t)q.aim});
    for (const auto &q : r.rounds) tot.push_back(q.total);
    write_placement(a, sel, tot, r.log);
    std::printf("{\"n_candidates\": %zu, \"n_aims\": %zu, \"n_fixed\": %d, "
                "\"n_selected\": %zu, \"base_total\": %.17g, \"base_covered\": %d, "
                "\"total_cells\": %d}\n",
                f.tick.candidates.size(), ap.aims.size(), r.n_fixed, r.rounds.size(),
                r.base_total, r.base_covered, r.total_cells);
    return 0;
}

// the simulated scans of the given sensor poses against a terrain: every sensor's returns (24-byte
// records, the sensors' segments one after the other), the segments' offsets, the terrain's
// blind-spot records and the per-point sensor mask
// mounted: scan_mounted -- six numbers per sensor and the beam table (or "-") before the outputs
static int cmd_scan(Device &dev, char **a, bool mounted = false) {
    const auto t = read_file(a[0]);
    const size_t tn = std::strtoull(a[1], nullptr, 10);
    const auto pv = tuple(a[2]);
    const size_t per = mounted ? 6 : 5;
    if (pv.size() % per != 0) {
        std::fprintf(stderr, "scan: POSES holds %zu numbers, not %zu per sensor\n", pv.size(), per);
        return 2;
    }
    VirtualScan::Params sp;
    sp.n_az = std::atoi(a[3]);
    sp.n_el = std::atoi(a[4]);
    sp.max_distance = std::strtod(a[5], nullptr);
    SimplifiedDualLidarOptimizer node(dev, SimplifiedDualLidarOptimizer::Params{});
    const PointCloud2 terrain = cloud_from(t, tn, 32, "map");
    node.terrainCallback(terrain);
    if (mounted && std::strcmp(a[6], "-") != 0) {
        sp.el_table = tuple(a[6]);
        if (sp.el_table.size() != (size_t)sp.n_el) {
            std::fprintf(stderr, "scan_mounted: ELTABLE holds %zu numbers, not NEL\n",
                         sp.el_table.size());
            return 2;
        }
    }
    if (mounted) a += 1;   // (the outputs follow the table)
    std::vector<VirtualScan::SensorPose> mounts(mounted ? pv.size() / 6 : 0);
    for (size_t i = 0; i < mounts.size(); ++i)
        mounts[i] = VirtualScan::SensorPose{pv[6 * i],     pv[6 * i + 1], pv[6 * i + 2],
                                            pv[6 * i + 3], pv[6 * i + 4], pv[6 * i + 5]};
    std::vector<SimplifiedDualLidarOptimizer::LidarPosition> sensors(mounted ? 0 : pv.size() / 5);
    for (size_t i = 0; i < sensors.size(); ++i) {
        sensors[i].x = pv[5 * i];
        sensors[i].y = pv[5 * i + 1];
        sensors[i].z = pv[5 * i + 2];
        sensors[i].pitch = pv[5 * i + 3];
        sensors[i].yaw = pv[5 * i + 4];
    }
    VirtualScan vs(sp);
    const auto r = mounted ? vs.scan_mounted(dev, terrain, mounts) : vs.scan(dev, terrain, sensors);
    if (!r.ran) {
        std::fprintf(stderr, "scan: %s\n", vs.lastError().c_str());
        return 1;
    }
    std::vector<uint8_t> all;
    std::vector<uint64_t> off(1, 0);
    for (const auto &m : r.scans) {
        if (m.point_step != 24 || m.fields.size() != 6) return 3;
        all.insert(all.end(), m.data.begin(), m.data.end());
        off.push_back(off.back() + m.width);
    }
    write_file(a[6], all.data(), all.size());
    write_file(a[7], off.data(), off.size() * 8);
    write_file(a[8], r.blind_spots.data.data(), r.blind_spots.data.size());
    write_file(a[9], r.point_mask.data(), r.point_mask.size() * 8);
    std::printf("{\"n_sensors\": %zu, \"n_returns\": %llu, \"n_points\": %llu, "
                "\"n_seen_any\": %llu, \"n_blind\": %u}\n",
                r.scans.size(), (unsigned long long)off.back(), (unsigned long long)r.n_points,
                (unsigned long long)r.n_seen_any, r.blind_spots.width);
    return 0;
}

// the coverage placement of the given candidate poses against a terrain: the rounds' records, the
// per-point owners and the blind-spot records of the region.  pair: the exact pair search
// (cover_pair: cover's arguments less KMAX, the JSON line with the search's figures); refine: the
// exchanges from --start or from greedy's answer (cover_refine: the slots in order as the rounds)
enum class CoverCmd { Greedy, Pair, Refine };
static int cover_front(Device &dev, char **a, int argc, CoverCmd mode) {
    const bool pair = mode == CoverCmd::Pair, refine = mode == CoverCmd::Refine;
    const char *cmd = pair ? "cover_pair" : refine ? "cover_refine" : "cover";
    const int k = pair ? 0 : 1;   // the arguments behind MAXD: [KMAX] MINSEP ROI OUT x 3 [FIXED]
    // cover_refine's options behind the positional arguments
    std::vector<int64_t> start;
    bool have_start = false;
    int n_locked = -1, max_moves = 16;
    if (refine) {
        int pos = argc;
        for (int i = 12; i < argc; ++i)
            if (std::strncmp(a[i], "--", 2) == 0) {
                pos = std::min(pos, i);
                const std::string opt = a[i];
                if (i + 1 >= argc || (opt != "--start" && opt != "--locked" && opt != "--max-moves")) {
                    std::fprintf(stderr, "%s: bad option %s\n", cmd, a[i]);
                    return 2;
                }
                const char *val = a[++i];
                if (opt == "--start") {
                    have_start = true;
                    for (double f : tuple(val)) {
                        if (f != (double)(int64_t)f) {
                            std::fprintf(stderr, "%s: --start entry %g is no index\n", cmd, f);
                            return 2;
                        }
                        start.push_back((int64_t)f);
                    }
                } else {
                    char *end = nullptr;
                    const long v = std::strtol(val, &end, 10);
                    if (end == val || *end != '\0' || v < 0 || v > PCP_REFINE_MAX_MOVES) {
                        std::fprintf(stderr, "%s: bad value %s for %s\n", cmd, val, a[i - 1]);
                        return 2;
                    }
                    (opt == "--locked" ? n_locked : max_moves) = (int)v;
                }
            } else if (i > 12) {   // (a[12] alone may be FIXED)
                std::fprintf(stderr, "%s: unexpected argument %s\n", cmd, a[i]);
                return 2;
            }
        argc = std::min(pos, 13);   // (what is left: the positional arguments with FIXED)
        if (have_start && (argc > 12 || start.empty() || start.size() > PCP_PLACE_MAX)) {
            std::fprintf(stderr, "%s: --start holds 1 .. %d indices and takes no FIXED\n", cmd,
                         PCP_PLACE_MAX);
            return 2;
        }
    }
    const auto t = read_file(a[0]);
    const size_t tn = std::strtoull(a[1], nullptr, 10);
    std::vector<double> pv;
    const std::string ps = a[2];
    if (ps.size() > 4 && ps.compare(ps.size() - 4, 4, ".f64") == 0) {
        const auto raw = read_file(a[2]);
        pv.resize(raw.size() / 8);
        std::memcpy(pv.data(), raw.data(), pv.size() * 8);
        if (raw.size() % 8 != 0) pv.push_back(0.0);   // (refused below)
    } else {
        pv = tuple(a[2]);
    }
    if (pv.size() % 5 != 0) {
        std::fprintf(stderr, "%s: POSES holds %zu numbers, not 5 per candidate\n", cmd, pv.size());
        return 2;
    }
    VirtualScan::Params sp;
    sp.n_az = std::atoi(a[3]);
    sp.n_el = std::atoi(a[4]);
    sp.max_distance = std::strtod(a[5], nullptr);
    CoveragePlacement::Params cp;
    if (!pair) cp.num_mobile_lidars = std::atoi(a[6]);
    cp.min_separation = std::strtod(a[6 + k], nullptr);
    CoveragePlacement::Roi roi;
    if (std::strcmp(a[7 + k], "-") != 0) {
        roi = CoveragePlacement::Roi(read_file(a[7 + k]));
        if (roi.bytes.size() != tn) {
            std::fprintf(stderr, "%s: ROI holds %zu bytes, not TN\n", cmd, roi.bytes.size());
            return 2;
        }
    }
    std::vector<int64_t> fixed;
    if (argc > 11 + k)
        for (double f : tuple(a[11 + k])) {
            if (f != (double)(int64_t)f || f < 0 || f >= (double)(pv.size() / 5)) {
                std::fprintf(stderr, "%s: FIXED entry %g is no candidate\n", cmd, f);
                return 2;
            }
            fixed.push_back((int64_t)f);
        }
    if (fixed.size() > PCP_PLACE_MAX) {
        std::fprintf(stderr, "%s: more than %d FIXED candidates\n", cmd, PCP_PLACE_MAX);
        return 2;
    }
    SimplifiedDualLidarOptimizer node(dev, SimplifiedDualLidarOptimizer::Params{});
    const PointCloud2 terrain = cloud_from(t, tn, 32, "map");
    node.terrainCallback(terrain);
    std::vector<SimplifiedDualLidarOptimizer::LidarPosition> cand(pv.size() / 5);
    for (size_t i = 0; i < cand.size(); ++i) {
        cand[i].x = pv[5 * i];
        cand[i].y = pv[5 * i + 1];
        cand[i].z = pv[5 * i + 2];
        cand[i].pitch = pv[5 * i + 3];
        cand[i].yaw = pv[5 * i + 4];
    }
    CoveragePlacement place(cp);
    for (int64_t s : start)
        if (s < 0 || (size_t)s >= cand.size()) {
            std::fprintf(stderr, "%s: --start entry %lld is no candidate\n", cmd, (long long)s);
            return 2;
        }
    auto r = pair ? place.place_pair(dev, terrain, cand, sp, fixed, roi)
                  : refine && have_start ? CoveragePlacement::Result()
                                         : place.place(dev, terrain, cand, sp, fixed, roi);
    if (refine) {
        // without a start: greedy's answer, the FIXED candidates in front of it as locked slots
        if (!have_start) {
            if (!r.ran) {
                std::fprintf(stderr, "%s: %s\n", cmd, place.lastError().c_str());
                return 1;
            }
            start = fixed;
            for (const auto &q : r.rounds) start.push_back(q.candidate);
            if (start.empty() || start.size() > PCP_PLACE_MAX) {
                std::fprintf(stderr, "%s: greedy and FIXED give %zu sensors, not 1 .. %d\n", cmd,
                             start.size(), PCP_PLACE_MAX);
                return 1;
            }
            if (n_locked < 0) n_locked = (int)fixed.size();
        }
        r = place.refine(dev, terrain, cand, sp, start, std::max(n_locked, 0), max_moves, roi);
    }
    if (!r.ran) {
        std::fprintf(stderr, "%s: %s\n", cmd, place.lastError().c_str());
        return 1;
    }
    std::vector<int64_t> rec;
    for (const auto &q : r.rounds) {
        rec.push_back(q.candidate);
        rec.push_back((int64_t)q.gain);
        rec.push_back((int64_t)q.covered);
    }
    write_file(a[8 + k], rec.data(), rec.size() * 8);
    write_file(a[9 + k], r.point_owner.data(), r.point_owner.size() * 4);
    write_file(a[10 + k], r.blind_spots.data.data(), r.blind_spots.data.size());
    std::fputs(r.log.c_str(), stderr);
    const unsigned long long covered =
        (unsigned long long)(r.rounds.empty() ? r.base_covered : r.rounds.back().covered);
    if (pair) {
        std::printf("{\"n_candidates\": %zu, \"n_selected\": %zu, \"n_points\": %llu, "
                    "\"roi_points\": %llu, \"base_covered\": %llu, \"covered\": %llu, "
                    "\"n_blind\": %u, \"best_pair\": [%lld, %lld], \"pair_gain\": %llu, "
                    "\"best_single\": %lld, \"single_gain\": %llu}\n",
                    cand.size(), r.rounds.size(), (unsigned long long)r.n_points,
                    (unsigned long long)r.roi_points, (unsigned long long)r.base_covered, covered,
                    r.blind_spots.width, (long long)r.best_pair[0], (long long)r.best_pair[1],
                    (unsigned long long)r.pair_gain, (long long)r.best_single,
                    (unsigned long long)r.single_gain);
        return 0;
    }
    if (refine) {
        std::string moves;
        for (const auto &m : r.moves) {
            char buf[128];
            std::snprintf(buf, sizeof(buf), "%s[%d, %lld, %lld, %llu]", moves.empty() ? "" : ", ",
                          m.slot, (long long)m.from, (long long)m.to,
                          (unsigned long long)m.covered);
            moves += buf;
        }
        std::printf("{\"n_candidates\": %zu, \"n_selected\": %zu, \"n_points\": %llu, "
                    "\"roi_points\": %llu, \"base_covered\": %llu, \"covered\": %llu, "
                    "\"n_blind\": %u, \"n_locked\": %d, \"start_covered\": %llu, "
                    "\"moves\": [%s], \"converged\": %d}\n",
                    cand.size(), r.rounds.size(), (unsigned long long)r.n_points,
                    (unsigned long long)r.roi_points, (unsigned long long)r.base_covered, covered,
                    r.blind_spots.width, r.n_locked, (unsigned long long)r.start_covered,
                    moves.c_str(), r.converged ? 1 : 0);
        return 0;
    }
    std::printf("{\"n_candidates\": %zu, \"n_selected\": %zu, \"n_points\": %llu, "
                "\"roi_points\": %llu, \"base_covered\": %llu, \"covered\": %llu, "
                "\"n_blind\": %u}\n",
                cand.size(), r.rounds.size(), (unsigned long long)r.n_points,
                (unsigned long long)r.roi_points, (unsigned long long)r.base_covered,
                covered, r.blind_spots.width);
    return 0;
}
static int cmd_cover(Device &dev, char **a, int argc) {
    return cover_front(dev, a, argc, CoverCmd::Greedy);
}

// whole numbers of a tuple argument as int64 (false: an entry is none)
static bool whole_numbers(const char *arg, std::vector<int64_t> &out) {
    for (double f : tuple(arg)) {
        if (f != (double)(int64_t)f) return false;
        out.push_back((int64_t)f);
    }
    return true;
}

// cover with a limited field of view: every candidate searched with every aim of a table
// (AimedCoveragePlacement); the records hold the aim beside the candidate
static int cmd_cover_aimed(Device &dev, char **a, int argc) {
    const char *cmd = "cover_aimed";
    const auto t = read_file(a[0]);
    const size_t tn = std::strtoull(a[1], nullptr, 10);
    std::vector<double> pv;
    const std::string ps = a[2];
    if (ps.size() > 4 && ps.compare(ps.size() - 4, 4, ".f64") == 0) {
        const auto raw = read_file(a[2]);
        pv.resize(raw.size() / 8);
        std::memcpy(pv.data(), raw.data(), pv.size() * 8);
        if (raw.size() % 8 != 0) pv.push_back(0.0);   // (refused below)
    } else {
        pv = tuple(a[2]);
    }
    if (pv.size() % 5 != 0) {
        std::fprintf(stderr, "%s: POSES holds %zu numbers, not 5 per candidate\n", cmd, pv.size());
        return 2;
    }
    VirtualScan::Params sp;
    sp.n_az = std::atoi(a[3]);
    sp.n_el = std::atoi(a[4]);
    sp.max_distance = std::strtod(a[5], nullptr);
    AimedCoveragePlacement::Params cp;
    cp.num_mobile_lidars = std::atoi(a[6]);
    cp.min_separation = std::strtod(a[7], nullptr);
    cp.w_az = std::atoi(a[9]);
    cp.w_el = std::atoi(a[10]);
    if (cp.w_az < 1 || cp.w_az > sp.n_az || cp.w_el < 1 || cp.w_el > sp.n_el) {
        std::fprintf(stderr, "%s: the window %d x %d does not fit the fan\n", cmd, cp.w_az, cp.w_el);
        return 2;
    }
    std::vector<int64_t> av;
    if (!whole_numbers(a[11], av) || av.empty() || av.size() % 2 != 0 ||
        av.size() / 2 > PCP_COVER_AIM_MAX) {
        std::fprintf(stderr, "%s: AIMS holds 1 .. %d pairs az0,el0 of whole numbers\n", cmd,
                     PCP_COVER_AIM_MAX);
        return 2;
    }
    for (size_t i = 0; i < av.size(); i += 2) {
        if (av[i] < 0 || av[i] >= sp.n_az || av[i + 1] < 0 || av[i + 1] > sp.n_el - cp.w_el) {
            std::fprintf(stderr, "%s: aim (%lld, %lld) lies outside the fan\n", cmd,
                         (long long)av[i], (long long)av[i + 1]);
            return 2;
        }
        AimedCoveragePlacement::Aim aim;
        aim.az0 = (int32_t)av[i];
        aim.el0 = (int32_t)av[i + 1];
        cp.aims.push_back(aim);
    }
    CoveragePlacement::Roi roi;
    if (std::strcmp(a[8], "-") != 0) {
        roi = CoveragePlacement::Roi(read_file(a[8]));
        if (roi.bytes.size() != tn) {
            std::fprintf(stderr, "%s: ROI holds %zu bytes, not TN\n", cmd, roi.bytes.size());
            return 2;
        }
    }
    std::vector<AimedCoveragePlacement::Fixed> fixed;
    if (argc > 15) {
        std::vector<int64_t> fv;
        if (!whole_numbers(a[15], fv) || fv.size() % 2 != 0 || fv.size() / 2 > PCP_PLACE_MAX) {
            std::fprintf(stderr, "%s: FIXED holds at most %d pairs candidate,aim\n", cmd,
                         PCP_PLACE_MAX);
            return 2;
        }
        for (size_t i = 0; i < fv.size(); i += 2) {
            if (fv[i] < 0 || fv[i] >= (int64_t)(pv.size() / 5) || fv[i + 1] < 0 ||
                fv[i + 1] >= (int64_t)cp.aims.size()) {
                std::fprintf(stderr, "%s: FIXED entry (%lld, %lld) is no candidate and aim\n", cmd,
                             (long long)fv[i], (long long)fv[i + 1]);
                return 2;
            }
            AimedCoveragePlacement::Fixed f;
            f.candidate = fv[i];
            f.aim = (int32_t)fv[i + 1];
            fixed.push_back(f);
        }
    }
    SimplifiedDualLidarOptimizer node(dev, SimplifiedDualLidarOptimizer::Params{});
    const PointCloud2 terrain = cloud_from(t, tn, 32, "map");
    node.terrainCallback(terrain);
    std::vector<SimplifiedDualLidarOptimizer::LidarPosition> cand(pv.size() / 5);
    for (size_t i = 0; i < cand.size(); ++i) {
        cand[i].x = pv[5 * i];
        cand[i].y = pv[5 * i + 1];
        cand[i].z = pv[5 * i + 2];
        cand[i].pitch = pv[5 * i + 3];
        cand[i].yaw = pv[5 * i + 4];
    }
    AimedCoveragePlacement place(cp);
    const auto r = place.place(dev, terrain, cand, sp, fixed, roi);
    if (!r.ran) {
        std::fprintf(stderr, "%s: %s\n", cmd, place.lastError().c_str());
        return 1;
    }
    std::vector<int64_t> rec;
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        rec.push_back(r.rounds[i].candidate);
        rec.push_back((int64_t)r.aim[i]);
        rec.push_back((int64_t)r.rounds[i].gain);
        rec.push_back((int64_t)r.rounds[i].covered);
    }
    write_file(a[12], rec.data(), rec.size() * 8);
    write_file(a[13], r.point_owner.data(), r.point_owner.size() * 4);
    write_file(a[14], r.blind_spots.data.data(), r.blind_spots.data.size());
    std::fputs(r.log.c_str(), stderr);
    const unsigned long long covered =
        (unsigned long long)(r.rounds.empty() ? r.base_covered : r.rounds.back().covered);
    std::printf("{\"n_candidates\": %zu, \"n_aims\": %zu, \"n_selected\": %zu, "
                "\"n_points\": %llu, \"roi_points\": %llu, \"base_covered\": %llu, "
                "\"covered\": %llu, \"n_blind\": %u}\n",
                cand.size(), cp.aims.size(), r.rounds.size(), (unsigned long long)r.n_points,
                (unsigned long long)r.roi_points, (unsigned long long)r.base_covered, covered,
                r.blind_spots.width);
    return 0;
}
// cover by weight: the candidates placed by the weight of the terrain points their scans reach
// (WeightedCoveragePlacement); the records hold the weight and the points gained
static int cmd_cover_weighted(Device &dev, char **a, int argc) {
    const char *cmd = "cover_weighted";
    const auto t = read_file(a[0]);
    const size_t tn = std::strtoull(a[1], nullptr, 10);
    std::vector<double> pv;
    const std::string ps = a[2];
    if (ps.size() > 4 && ps.compare(ps.size() - 4, 4, ".f64") == 0) {
        const auto raw = read_file(a[2]);
        pv.resize(raw.size() / 8);
        std::memcpy(pv.data(), raw.data(), pv.size() * 8);
        if (raw.size() % 8 != 0) pv.push_back(0.0);   // (refused below)
    } else {
        pv = tuple(a[2]);
    }
    if (pv.size() % 5 != 0) {
        std::fprintf(stderr, "%s: POSES holds %zu numbers, not 5 per candidate\n", cmd, pv.size());
        return 2;
    }
    VirtualScan::Params sp;
    sp.n_az = std::atoi(a[3]);
    sp.n_el = std::atoi(a[4]);
    sp.max_distance = std::strtod(a[5], nullptr);
    WeightedCoveragePlacement::Params cp;
    cp.num_mobile_lidars = std::atoi(a[6]);
    cp.min_separation = std::strtod(a[7], nullptr);
    // WEIGHTS: a .u8 file, or BASE[/x0,x1,y0,y1,z0,z1,W]..
    auto byte_of = [](double f) { return f == (double)(int64_t)f && f >= 0 && f <= 255; };
    CoverageWeights weights;
    const std::string ws = a[8];
    if (ws.size() > 3 && ws.compare(ws.size() - 3, 3, ".u8") == 0) {
        weights = CoverageWeights(read_file(a[8]));
        if (weights.bytes.size() != tn) {
            std::fprintf(stderr, "%s: WEIGHTS holds %zu bytes, not TN\n", cmd,
                         weights.bytes.size());
            return 2;
        }
    } else {
        std::stringstream ss(ws);
        std::string part;
        bool first = true;
        while (std::getline(ss, part, '/')) {
            const auto v = tuple(part.c_str());
            if (first) {
                if (v.size() != 1 || !byte_of(v[0])) {
                    std::fprintf(stderr, "%s: WEIGHTS starts with a base weight 0 .. 255\n", cmd);
                    return 2;
                }
                weights.base = (uint8_t)v[0];
                first = false;
                continue;
            }
            if (v.size() != 7 || !byte_of(v[6])) {
                std::fprintf(stderr, "%s: a box of WEIGHTS is x0,x1,y0,y1,z0,z1,W with W 0 .. 255\n",
                             cmd);
                return 2;
            }
            CoverageWeightBox b;
            b.box = CoverageBox{v[0], v[1], v[2], v[3], v[4], v[5]};
            b.weight = (uint8_t)v[6];
            weights.boxes.push_back(b);
        }
        if (first) {
            std::fprintf(stderr, "%s: WEIGHTS is empty\n", cmd);
            return 2;
        }
    }
    std::vector<int64_t> fixed;
    if (argc > 12)
        for (double f : tuple(a[12])) {
            if (f != (double)(int64_t)f || f < 0 || f >= (double)(pv.size() / 5)) {
                std::fprintf(stderr, "%s: FIXED entry %g is no candidate\n", cmd, f);
                return 2;
            }
            fixed.push_back((int64_t)f);
        }
    if (fixed.size() > PCP_PLACE_MAX) {
        std::fprintf(stderr, "%s: more than %d FIXED candidates\n", cmd, PCP_PLACE_MAX);
        return 2;
    }
    SimplifiedDualLidarOptimizer node(dev, SimplifiedDualLidarOptimizer::Params{});
    const PointCloud2 terrain = cloud_from(t, tn, 32, "map");
    node.terrainCallback(terrain);
    std::vector<SimplifiedDualLidarOptimizer::LidarPosition> cand(pv.size() / 5);
    for (size_t i = 0; i < cand.size(); ++i) {
        cand[i].x = pv[5 * i];
        cand[i].y = pv[5 * i + 1];
        cand[i].z = pv[5 * i + 2];
        cand[i].pitch = pv[5 * i + 3];
        cand[i].yaw = pv[5 * i + 4];
    }
    WeightedCoveragePlacement place(cp);
    const auto r = place.place(dev, terrain, cand, sp, weights, fixed);
    if (!r.ran) {
        std::fprintf(stderr, "%s: %s\n", cmd, place.lastError().c_str());
        return 1;
    }
    std::vector<int64_t> rec;
    for (size_t i = 0; i < r.rounds.size(); ++i) {
        rec.push_back(r.rounds[i].candidate);
        rec.push_back((int64_t)r.rounds[i].gain);
        rec.push_back((int64_t)r.gain_points[i]);
        rec.push_back((int64_t)r.rounds[i].covered);
    }
    write_file(a[9], rec.data(), rec.size() * 8);
    write_file(a[10], r.point_owner.data(), r.point_owner.size() * 4);
    write_file(a[11], r.blind_spots.data.data(), r.blind_spots.data.size());
    std::fputs(r.log.c_str(), stderr);
    const unsigned long long covered =
        (unsigned long long)(r.rounds.empty() ? r.base_covered : r.rounds.back().covered);
    std::printf("{\"n_candidates\": %zu, \"n_selected\": %zu, \"n_points\": %llu, "
                "\"roi_points\": %llu, \"roi_weight\": %llu, \"base_covered\": %llu, "
                "\"base_points\": %llu, \"covered\": %llu, \"n_blind\": %u, "
                "\"blind_weight\": %llu}\n",
                cand.size(), r.rounds.size(), (unsigned long long)r.n_points,
                (unsigned long long)r.roi_points, (unsigned long long)r.roi_weight,
                (unsigned long long)r.base_covered, (unsigned long long)r.base_points, covered,
                r.blind_spots.width, (unsigned long long)r.blind_weight);
    return 0;
}
static int cmd_cover_pair(Device &dev, char **a, int argc) {
    return cover_front(dev, a, argc, CoverCmd::Pair);
}
static int cmd_cover_refine(Device &dev, char **a, int argc) {
    return cover_front(dev, a, argc, CoverCmd::Refine);
}

// HDL-64-like scan (64 rings, -24.9..+2 deg) of n points against a ground plane
static std::vector<float> synth_scan(size_t n, double h, std::mt19937_64 &rng) {
    std::uniform_real_distribution<double> ua(-M_PI, M_PI), ur(1.0, 40.0);
    std::uniform_int_distribution<int> ring(0, 63);
    std::vector<float> p(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const double el = (-24.9 + 26.9 * ring(rng) / 63.0) * M_PI / 180.0, az = ua(rng);
        double r = ur(rng);
        if (el < 0) r = std::min(r, h / std::sin(-el));
        p[4 * i] = (float)(r * std::cos(el) * std::cos(az));
        p[4 * i + 1] = (float)(r * std::cos(el) * std::sin(az));
        p[4 * i + 2] = (float)(r * std::sin(el));
        p[4 * i + 3] = 0.f;
    }
    return p;
}

static int cmd_replay(Device &dev, char **a) {
    const auto t = read_file(a[0]), c = read_file(a[2]), nr = read_file(a[3]);
    const size_t tn = std::strtoull(a[1], nullptr, 10), cn = std::strtoull(a[4], nullptr, 10);
    const auto bbox = tuple(a[5]);
    const int frames = std::atoi(a[6]);
    const size_t npts = std::strtoull(a[7], nullptr, 10);
    // chain = 1: the launch file's whole per-frame chain -- the merged cloud goes through
    // excavated_surface_generator, whose /excavated_terrain and /excavation_area feed
    // virtual_lidar every frame (terrain index, normals, cell grid rebuilt per frame)
    const bool chain = a[8] && std::atoi(a[8]) != 0;
    // DUMP_DIR (optional): the inputs and every node's outputs of frames 0, 1, 2 and the last
    // one, for the oracle check of the streamed chain (tests/test_nodes_cli.py)
    const std::string dump = (a[8] && a[9]) ? a[9] : "";
    SimplifiedScanMatcher filt(dev);
    GnssGicpMatcher merger(dev);
    ComposedFilterMerge front(dev);
    bool front_fused = true;
    if (const char *ff = std::getenv("PCP_FRONT_FUSED")) front_fused = std::atoi(ff) != 0;
    // the carve node and virtual_lidar's area + terrain callbacks composed (default)
    bool carve_fused = true;
    if (const char *cf = std::getenv("PCP_CARVE_FUSED")) carve_fused = std::atoi(cf) != 0;
    // the composed carve reads the merger's landed records in place (default) / the message
    bool carve_landed = true;
    if (const char *cl = std::getenv("PCP_CARVE_LANDED")) carve_landed = std::atoi(cl) != 0;
    // the zx120 cloud's callback composed into the carve call as well (PCP_CARVE_ZX=1): its
    // index is enqueued before the carve's messages are copied out of the landing.  Off by
    // default: no faster (p50 0.644-0.673 vs 0.637-0.648 ms, profiles/r05_c5_host_bbox_zx_ab.log)
    bool carve_zx = false;
    if (const char *cz = std::getenv("PCP_CARVE_ZX")) carve_zx = std::atoi(cz) != 0;
    ExcavationTerrainGenerator gen(dev);
    SimplifiedDualLidarOptimizer vl(dev);
    // the nodes composed in one process: the grid setup is enqueued by the area callback and
    // waited for once by the tick (PCP_AREA_ASYNC=0: settled in the area callback, as a ROS shell
    // that publishes the grid markers there)
    bool area_async = true;
    if (const char *ea = std::getenv("PCP_AREA_ASYNC")) area_async = std::atoi(ea) != 0;
    vl.setDeferredGrid(area_async);
    // the filter / merger messages copied out of their landing after the composed carve has
    // read the merged cloud in place (default; only where every composition applies), while the
    // device builds the grid.  PCP_FRONT_DEFER=0: copied by the front call
    bool front_defer = true;
    if (const char *fd = std::getenv("PCP_FRONT_DEFER")) front_defer = std::atoi(fd) != 0;
    front_defer = front_defer && front_fused && chain && carve_fused && carve_landed && area_async &&
                  !carve_zx;
    // PCP_REPLAY_NO_TF=k: frame k's map -> zx120/base_link lookup fails (the carve's fallback:
    // the merged cloud republished as the terrain, no area); the line reports that frame's
    // terrain message (a deferred merged message must not go out as its header)
    long no_tf_frame = -1;
    if (const char *nt = std::getenv("PCP_REPLAY_NO_TF")) no_tf_frame = std::atol(nt);
    size_t no_tf_points = 0, no_tf_bytes = 0, no_tf_merged = 0;
    vl.terrainCallback(cloud_from(t, tn, 32, "map"));
    std::vector<double> xyz(cn * 3);
    std::vector<float> nrm(cn * 3);
    std::memcpy(xyz.data(), c.data(), xyz.size() * 8);
    std::memcpy(nrm.data(), nr.data(), nrm.size() * 4);
    vl.setExcavationGrid(xyz, nrm, bbox.data());
    std::mt19937_64 rng(20260227);
    const Transform robot_tf{{8.0, -3.0, 2.0}, {0.0, 0.0, 0.2588190451025208, 0.9659258262890683}};
    const Transform zx_tf{{0.55, 0.4, 3.5}, {0.0, 0.21633, 0.0, 0.97632}};
    const Transform zx_base{{0.0, 0.0, 0.0}, {0, 0, 0, 1}};
    std::vector<double> lat;
    std::vector<double> lat_frame;   // in frame order (the sorted copy gives the percentiles)
    // per-callback wall time (ms): filter x2, merger, carve, area, terrain, zx120 cloud, tick
    constexpr int kStages = 7;
    static const char *kStageName[kStages] = {"filter", "merge", "carve", "area",
                                              "terrain", "zx120", "tick"};
    std::vector<double> stage[kStages], stage_frame[kStages];   // sorted later / frame order
    size_t merged_n = 0, best = 0, cells_n = cn;
    uint64_t realloc_after_warmup = 0, ra0 = 0;
    std::string dumped;
    const bool alloc_trace = std::getenv("PCP_ALLOC_TRACE") != nullptr;
    for (int f = 0; f < frames + 2; ++f) {
        if (alloc_trace) std::fprintf(stderr, "replay frame %d\n", f);
        if (f == 2) pcp_alloc_stats(&ra0, nullptr, nullptr);
        auto rs = synth_scan(npts, 2.0, rng), zs = synth_scan(npts, 3.5, rng);
        PointCloud2 rm = make_xyz_cloud(rs.data(), npts, "four_wheel_robot/velodyne_link");
        PointCloud2 zm = make_xyz_cloud(zs.data(), npts, "zx120/velodyne_link");
        const auto t0 = std::chrono::steady_clock::now();
        double st[kStages] = {};
        auto lap = [&st, last = t0](int k) mutable {
            const auto now = std::chrono::steady_clock::now();
            st[k] = std::chrono::duration<double, std::milli>(now - last).count();
            last = now;
        };
        // pointcloud_filter: both sensors; pointcloud_merger: 10 Hz tick; virtual_lidar: zx120
        // filtered cloud + the pose search.  Composed (PCP_FRONT_FUSED, default): the filter
        // and merger nodes in one call and one synchronisation (stage "filter" then holds both)
        PointCloud2 rf, zf;
        GnssGicpMatcher::Output o;
        pcp_cloud_view front_landed{};
        ComposedFilterMerge::Output fo;
        // the front's messages (when deferred: after the carve call)
        auto take_front = [&]() {
            front.messages(fo);
            rf = std::move(fo.robot_filtered);
            zf = std::move(fo.backhoe_filtered);
            o = std::move(fo.merge);
        };
        if (front_fused) {
            fo = front.frame(rm, zm, true, &robot_tf, &zx_tf, front_defer);
            if (!front.lastError().empty()) {
                std::fprintf(stderr, "replay: filter+merge failed: %s\n", front.lastError().c_str());
                return 1;
            }
            front_landed = fo.merged_landed;
            if (front_defer) o.merged = fo.merge.merged;   // (its header: the carve reads the landing)
            else take_front();
            lap(0);
            lap(1);
        } else {
            rf = filt.robotCloudCallback(rm);
            zf = filt.backhoeCloudCallback(zm);
            lap(0);
            merger.robotCloudCallback(rf);
            merger.backhoeCloudCallback(zf);
            o = merger.processPointClouds(true, &robot_tf, &zx_tf);
            lap(1);
        }
        ExcavationTerrainGenerator::Output e;
        const bool zx_in_carve = chain && carve_fused && carve_zx;
        const bool no_tf = (long)f == no_tf_frame;
        if (chain && carve_fused) {   // the carve + both callbacks (stage "carve" holds all three)
            e = vl.carveCallbacks(gen, o.merged, no_tf ? nullptr : &zx_base,
                                  front_fused && carve_landed ? &front_landed : nullptr,
                                  zx_in_carve ? &zf : nullptr);
            if (no_tf) {
                no_tf_points = e.excavated_terrain.size();
                no_tf_bytes = e.excavated_terrain.data.size();
                no_tf_merged = front_landed.n;
            } else if (!e.area_published) {
                std::fprintf(stderr, "replay: carve failed: %s\n", gen.lastError().c_str());
                return 1;
            }
            if (front_defer) take_front();
            lap(2);
            lap(3);
            lap(4);
        } else if (chain) {
            e = gen.matchedCloudCallback(o.merged, &zx_base);
            if (!e.area_published) {
                std::fprintf(stderr, "replay: carve failed: %s\n", gen.lastError().c_str());
                return 1;
            }
            lap(2);
            vl.excavationAreaCallback(e.excavation_area);
            lap(3);
            vl.terrainCallback(e.excavated_terrain);
            lap(4);
        }
        if (!zx_in_carve) vl.zx120PointsCallback(zf);   // (else made by carveCallbacks)
        lap(5);
        auto r = vl.runOptimization(&zx_base);
        lap(6);
        if (chain) cells_n = vl.lastCells();   // (settled by the tick)
        const auto t1 = std::chrono::steady_clock::now();
        if (f >= 2)
            for (int k = 0; k < kStages; ++k) {
                stage[k].push_back(st[k]);
                stage_frame[k].push_back(st[k]);
            }
        if (!r.ran) {
            std::fprintf(stderr, "replay: pose search did not run: %s\n", vl.lastError().c_str());
            return 1;
        }
        merged_n = o.merged.size();
        best = (size_t)r.report.best_idx;
        if (f >= 2) lat.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        if (f >= 2) lat_frame.push_back(lat.back());
        if (!dump.empty() && chain && (f < 3 || f == frames + 1)) {
            const std::string pre = dump + "/f" + std::to_string(f) + "_";
            write_file((pre + "rscan.f32").c_str(), rs.data(), rs.size() * 4);
            write_file((pre + "zscan.f32").c_str(), zs.data(), zs.size() * 4);
            write_file((pre + "rf.bin").c_str(), rf.data.data(), rf.data.size());
            write_file((pre + "zf.bin").c_str(), zf.data.data(), zf.data.size());
            write_file((pre + "merged.bin").c_str(), o.merged.data.data(), o.merged.data.size());
            // the carve's outputs, as published (they are the node inputs of this frame)
            write_file((pre + "terrain.bin").c_str(), e.excavated_terrain.data.data(),
                       e.excavated_terrain.data.size());
            write_file((pre + "area.bin").c_str(), e.excavation_area.data.data(),
                       e.excavation_area.data.size());
            uint64_t nc = 0;
            pcp_get_cells(dev.ctx(), nullptr, nullptr, 0, &nc);
            std::vector<double> cx(3 * nc);
            std::vector<float> cnr(3 * nc);
            if (nc) pcp_get_cells(dev.ctx(), cx.data(), cnr.data(), nc, &nc);
            write_file((pre + "cells.f64").c_str(), cx.data(), cx.size() * 8);
            write_file((pre + "cnrm.f32").c_str(), cnr.data(), cnr.size() * 4);
            std::vector<double> ps, tot;
            for (const auto &c : r.candidates) {
                ps.insert(ps.end(), {c.x, c.y, c.z, c.pitch, c.yaw});
                tot.push_back(c.total_score);
            }
            write_file((pre + "poses.f64").c_str(), ps.data(), ps.size() * 8);
            write_file((pre + "tot.f64").c_str(), tot.data(), tot.size() * 8);
            char buf[128];
            std::snprintf(buf, sizeof(buf), "%s{\"frame\": %d, \"best_idx\": %lld}",
                          dumped.empty() ? "" : ", ", f, (long long)r.report.best_idx);
            dumped += buf;
        }
    }
    {
        uint64_t ra1 = 0;
        pcp_alloc_stats(&ra1, nullptr, nullptr);
        realloc_after_warmup = ra1 - ra0;
    }
    std::string lat_s;
    for (size_t i = 0; i < lat_frame.size(); ++i) {
        char b[32];
        std::snprintf(b, sizeof(b), "%s%.4f", i ? ", " : "", lat_frame[i]);
        lat_s += b;
    }
    // the stage times of the slowest frames (what the tail is made of)
    std::string slow_s;
    {
        std::vector<size_t> ord(lat_frame.size());
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
        std::sort(ord.begin(), ord.end(),
                  [&lat_frame](size_t a, size_t b) { return lat_frame[a] > lat_frame[b]; });
        for (size_t r = 0; r < std::min<size_t>(4, ord.size()); ++r) {
            char b[96];
            std::snprintf(b, sizeof(b), "%s{\"frame\": %zu, \"ms\": %.4f", r ? ", " : "", ord[r],
                          lat_frame[ord[r]]);
            slow_s += b;
            for (int k = 0; k < kStages; ++k) {
                std::snprintf(b, sizeof(b), ", \"%s\": %.4f", kStageName[k], stage_frame[k][ord[r]]);
                slow_s += b;
            }
            slow_s += "}";
        }
    }
    std::sort(lat.begin(), lat.end());
    auto q = [&lat](double p) { return lat[std::min(lat.size() - 1, (size_t)(p * lat.size()))]; };
    std::string stage_s;
    for (int k = 0; k < kStages; ++k) {
        auto &v = stage[k];
        std::sort(v.begin(), v.end());
        char b[64];
        std::snprintf(b, sizeof(b), "%s\"%s\": %.4f", k ? ", " : "", kStageName[k],
                      v.empty() ? 0.0 : v[v.size() / 2]);
        stage_s += b;
    }
    std::printf("{\"frames\": %zu, \"points_per_scan\": %zu, \"chain\": %d, \"p50_ms\": %.4f, "
                "\"p99_ms\": %.4f, \"max_ms\": %.4f, \"merged_points\": %zu, \"cells\": %zu, "
                "\"best_idx\": %zu, \"reallocs_after_warmup\": %llu, \"dumped\": [%s], "
                "\"stage_p50_ms\": {%s}, \"slowest\": [%s], \"lat_ms\": [%s], "
                "\"no_tf\": {\"frame\": %ld, \"terrain_points\": %zu, \"terrain_bytes\": %zu, "
                "\"merged_points\": %zu}}\n",
                lat.size(), npts, chain ? 1 : 0, q(0.5), q(0.99), lat.back(), merged_n, cells_n,
                best, (unsigned long long)realloc_after_warmup, dumped.c_str(), stage_s.c_str(),
                slow_s.c_str(), lat_s.c_str(), no_tf_frame, no_tf_points, no_tf_bytes,
                no_tf_merged);
    return 0;
}

// area AREA.f32 N_AREA TERRAIN.f32 N_TERRAIN ZX120_BASE(x,y,z) NUM_CANDIDATES MAX_DISTANCE
//      OUT_TOTAL.f64 OUT_CELLS.f64 OUT_NORMALS.f32
// the virtual_lidar node from its /excavation_area message: excavationAreaCallback (GPU normals
// + 3-D cell grid), terrainCallback, one runOptimization tick (no zx120 cloud)
static int cmd_area(Device &dev, char **a) {
    const auto ar = read_file(a[0]), t = read_file(a[2]);
    const size_t an = std::strtoull(a[1], nullptr, 10), tn = std::strtoull(a[3], nullptr, 10);
    const auto zxt = tuple(a[4]);
    SimplifiedDualLidarOptimizer::Params p;
    p.num_candidates = std::atoi(a[5]);
    p.max_distance = std::strtod(a[6], nullptr);
    SimplifiedDualLidarOptimizer node(dev, p);
    node.excavationAreaCallback(cloud_from(ar, an, 32, "map"));
    if (!node.lastError().empty()) {
        std::fprintf(stderr, "area: %s\n", node.lastError().c_str());
        return 1;
    }
    node.terrainCallback(cloud_from(t, tn, 32, "map"));
    Transform zx;
    zx.t[0] = zxt[0];
    zx.t[1] = zxt[1];
    zx.t[2] = zxt[2];
    const auto r = node.runOptimization(&zx);
    if (!r.ran) {
        std::fprintf(stderr, "area: %s\n", node.lastError().c_str());
        return 1;
    }
    std::vector<double> tot(r.candidates.size());
    for (size_t i = 0; i < tot.size(); ++i) tot[i] = r.candidates[i].total_score;
    write_file(a[7], tot.data(), tot.size() * 8);
    uint64_t nc = 0;
    pcp_get_cells(dev.ctx(), nullptr, nullptr, 0, &nc);
    std::vector<double> xyz(nc * 3);
    std::vector<float> nrm(nc * 3);
    if (pcp_get_cells(dev.ctx(), xyz.data(), nrm.data(), nc, &nc) != PCP_OK) return 1;
    write_file(a[8], xyz.data(), xyz.size() * 8);
    write_file(a[9], nrm.data(), nrm.size() * 4);
    std::printf("{\"n_cells\": %llu, \"n_candidates\": %zu, \"best_idx\": %lld}\n",
                (unsigned long long)nc, r.candidates.size(), (long long)r.report.best_idx);
    return 0;
}

// calc_drivable_area: two robotCloudCallback frames of the same cloud at robot positions R1, R2
// (the first one fixes the start-clear centre), plus the skipped cases (no TF, empty cloud)
static int cmd_drivable(Device &dev, char **a) {
    const auto raw = read_file(a[0]);
    const size_t n = std::strtoull(a[1], nullptr, 10);
    const uint32_t step = (uint32_t)std::strtoul(a[2], nullptr, 10);
    const Transform tf = tf_from(tuple(a[3]));
    const auto r1 = tuple(a[4]), r2 = tuple(a[5]);
    DrivableAreaMapper node(dev);
    const PointCloud2 msg = cloud_from(raw, n, step, "four_wheel_robot/velodyne_link");
    OccupancyGrid g1, g2, skip;
    Transform b1, b2;
    b1.t[0] = r1[0];
    b1.t[1] = r1[1];
    b2.t[0] = r2[0];
    b2.t[1] = r2[1];
    if (node.robotCloudCallback(msg, nullptr, &b1, skip) || node.startSet()) return 3;
    if (node.robotCloudCallback(msg, &tf, nullptr, skip) || node.startSet()) return 4;
    if (node.robotCloudCallback(cloud_from(raw, 0, step, msg.frame_id), &tf, &b1, skip) ||
        node.startSet())
        return 5;
    if (!node.robotCloudCallback(msg, &tf, &b1, g1) || !node.robotCloudCallback(msg, &tf, &b2, g2)) {
        std::fprintf(stderr, "drivable: %s\n", node.lastError().c_str());
        return 1;
    }
    std::vector<int8_t> both(g1.data);
    both.insert(both.end(), g2.data.begin(), g2.data.end());
    write_file(a[6], both.data(), both.size());
    std::printf("{\"width\": %u, \"height\": %u, \"resolution\": %.17g, "
                "\"origin1\": [%.17g, %.17g], \"origin2\": [%.17g, %.17g]}\n",
                g1.width, g1.height, g1.resolution, g1.origin_x, g1.origin_y, g2.origin_x,
                g2.origin_y);
    return 0;
}

int main(int argc, char **argv) {
    // the container keeps the heap it freed: every frame's messages (MBs of PointCloud2 data)
    // are allocated and freed again, and glibc's defaults would map and unmap them (or trim the
    // heap top), paying their page faults every frame (C5 p50 -17 us, p99 -30 us,
    // profiles/r05_c5_malloc_ab.log).  PCP_MALLOC_KEEP=0: glibc's defaults
    {
        const char *mk = std::getenv("PCP_MALLOC_KEEP");
        if (!mk || std::atoi(mk) != 0) {
            mallopt(M_MMAP_THRESHOLD, 256 << 20);
            mallopt(M_TRIM_THRESHOLD, 1 << 30);
        }
    }
    // waits poll the completion signals instead of sleeping on an interrupt (the container's
    // three waits per frame return ~5 us sooner; C5 p50 0.593-0.607 vs 0.600-0.616 ms,
    // profiles/r05_c5_wait_ab.log).  Before the first HIP call; PCP_HSA_POLL=0: the default
    {
        const char *hp = std::getenv("PCP_HSA_POLL");
        if (!hp || std::atoi(hp) != 0) setenv("HSA_ENABLE_INTERRUPT", "0", 0);
    }
    if (argc < 2) {
        std::fprintf(stderr, "usage: pcp_nodes_cli filter|merge|vlidar|place|place_pair|place_triple|place_refine|place_aimed|scan|scan_mounted|cover|cover_aimed|cover_pair|cover_refine|cover_weighted|area|drivable|replay ...\n");
        return 2;
    }
    // name, arguments required after it, the command (a: the arguments, argc: how many)
    struct Command {
        const char *name;
        int need;
        int (*run)(Device &dev, char **a, int argc);
    };
    static const Command commands[] = {
        {"filter", 8, [](Device &d, char **a, int) { return cmd_filter(d, a); }},
        {"merge", 7, [](Device &d, char **a, int) { return cmd_merge(d, a); }},
        {"vlidar", 14, cmd_vlidar},
        {"place", 16, cmd_place},
        {"place_pair", 16, cmd_place_pair},
        {"place_triple", 16, cmd_place_triple},
        {"place_refine", 16, cmd_place_refine},
        {"place_aimed", 19, cmd_place_aimed},
        {"scan", 10, [](Device &d, char **a, int) { return cmd_scan(d, a); }},
        {"scan_mounted", 11, [](Device &d, char **a, int) { return cmd_scan(d, a, /*mounted=*/true); }},
        {"cover", 12, cmd_cover},
        {"cover_aimed", 15, cmd_cover_aimed},
        {"cover_pair", 11, cmd_cover_pair},
        {"cover_refine", 12, cmd_cover_refine},
        {"cover_weighted", 12, cmd_cover_weighted},
        {"area", 10, [](Device &d, char **a, int) { return cmd_area(d, a); }},
        {"drivable", 7, [](Device &d, char **a, int) { return cmd_drivable(d, a); }},
        {"replay", 8, [](Device &d, char **a, int) { return cmd_replay(d, a); }},
    };
    const std::string cmd = argv[1];
    const Command *c = std::find_if(std::begin(commands), std::end(commands),
                                    [&cmd](const Command &k) { return cmd == k.name; });
    if (c == std::end(commands) || argc - 2 < c->need) {
        std::fprintf(stderr, "bad arguments for %s\n", cmd.c_str());
        return 2;
    }
    try {
        Device dev(0);
        return c->run(dev, argv + 2, argc - 2);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
