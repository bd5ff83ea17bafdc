// Stand-alone check of pcp_knobs.hpp (no GPU, no HIP): knobs_from_env() over fake environments.
// 1. An empty environment gives the defaults, listed literally below (the values pcp_create's
//    hand-written lines left in the context before the table replaced them).
// 2. Every plain flag with "0", "1" and "" (an empty value parses as 0), every plain integer.
// 3. Every odd row with values on each side of its rule.
// 4. PCP_SCORE_WIDE_G refuses "3", "8x" and "", names itself in the error, and leaves the rows
//    before it parsed and the rows after it at their defaults.
// Prints "var NAME" for every row of the table (tests/test_knobs_host.py looks each up in
// INTEGRATION.md), then "ok".
// Build: c++ -std=c++17 -ffp-contract=off -I pointcloud_processor_amd/csrc
//        tests/native/knobs_selftest.cpp   (add -fsanitize=undefined for a sanitizer run)
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "pcp_knobs.hpp"

using namespace pcp;

static std::map<std::string, std::string> g_env;
static const char *fake_get(const char *name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        ++g_checks;                                                           \
        if (!(cond)) {                                                        \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);               \
            ++g_fail;                                                         \
        }                                                                     \
    } while (0)

// the knobs of one environment; the parse must succeed
static Knobs parse(std::map<std::string, std::string> env) {
    g_env = std::move(env);
    Knobs k;
    std::string err = "untouched";
    CHECK(knobs_from_env(k, fake_get, &err) == 0);
    CHECK(err == "untouched");
    return k;
}

static void check_defaults(const Knobs &k) {
    CHECK(k.fan_batch == 0);
    CHECK(k.fan_npw == 8);
    CHECK(k.fan_cull == true);
    CHECK(k.fan_clear == true);
    CHECK(k.fan_pivot == true);
    CHECK(k.fan_band == true);
    CHECK(k.fan_clip_e == 1.0f / 64.0f);
    CHECK(k.fan_horizon_first == true);
    CHECK(k.fan_host_out == true);
    CHECK(k.normals_exact == true);
    CHECK(k.score_wide == true);
    CHECK(k.score_wide_rays == -1);
    CHECK(k.score_wide_g == 0);
    CHECK(k.cells_all_ordered == false);
    CHECK(k.nb_blocks == 0);
    CHECK(k.scan_onepass == true);
    CHECK(k.index_pair == true);
    CHECK(k.area_side == true);
    CHECK(k.nb_small == true);
    CHECK(k.nb_region_pct == 75);
    CHECK(k.nb_guess_max == 67108864ull);
    CHECK(k.copy_threads == 3);
    CHECK(k.fm_host_out == true);
    CHECK(k.fm_fast == 2);
    CHECK(k.bk_gt == 0);
    CHECK(k.scan_pair == true);
    CHECK(k.carve_fuse_copy == true);
    CHECK(k.bk_pts == 512);
    CHECK(k.zc_in == true);
    CHECK(k.copy_kernel == true);
    CHECK(k.terrain_blocks == 1);
    CHECK(k.terrain_fine == 2);
    CHECK(k.fine_tile == 2);
    CHECK(k.fine_skip == 2);
    CHECK(k.fine_pack == true);
    CHECK(k.use_graphs == true);
    CHECK(k.host_bbox_scalar == false);
}

int main() {
    check_defaults(parse({}));
    CHECK(kClipSlack == 1.0f / 64.0f && kClipSlackWhole == 1.0f);

    // plain flags: atoi(v) != 0
    struct { const char *name; bool Knobs::*f; } flags[] = {
        {"PCP_FAN_CULL", &Knobs::fan_cull},           {"PCP_FAN_CLEAR", &Knobs::fan_clear},
        {"PCP_FAN_PIVOT", &Knobs::fan_pivot},         {"PCP_FAN_BAND", &Knobs::fan_band},
        {"PCP_FAN_ORDER", &Knobs::fan_horizon_first}, {"PCP_FAN_HOST_OUT", &Knobs::fan_host_out},
        {"PCP_NORMALS_EXACT", &Knobs::normals_exact}, {"PCP_SCORE_WIDE", &Knobs::score_wide},
        {"PCP_SCAN_ONEPASS", &Knobs::scan_onepass},   {"PCP_INDEX_PAIR", &Knobs::index_pair},
        {"PCP_AREA_STREAM", &Knobs::area_side},       {"PCP_NB_SMALL", &Knobs::nb_small},
        {"PCP_FM_HOST_OUT", &Knobs::fm_host_out},     {"PCP_SCAN_PAIR", &Knobs::scan_pair},
        {"PCP_CARVE_FUSE_COPY", &Knobs::carve_fuse_copy}, {"PCP_ZC_IN", &Knobs::zc_in},
        {"PCP_COPY_KERNEL", &Knobs::copy_kernel},     {"PCP_FINE_PACK", &Knobs::fine_pack},
    };
    for (const auto &f : flags) {
        CHECK(parse({{f.name, "0"}}).*f.f == false);
        CHECK(parse({{f.name, "1"}}).*f.f == true);
        CHECK(parse({{f.name, ""}}).*f.f == false);
        CHECK(parse({{f.name, "7"}}).*f.f == true);
        CHECK(parse({{f.name, "x"}}).*f.f == false);
    }
    // the inverted flags: true when the value parses to 0
    struct { const char *name; bool Knobs::*f; } inverted[] = {
        {"PCP_CELLS_ORDER_FREE", &Knobs::cells_all_ordered}, {"PCP_NO_GRAPHS", &Knobs::use_graphs}};
    for (const auto &f : inverted) {
        CHECK(parse({{f.name, "0"}}).*f.f == true);
        CHECK(parse({{f.name, "1"}}).*f.f == false);
        CHECK(parse({{f.name, ""}}).*f.f == true);
    }
    // plain integers: atoi
    struct { const char *name; int Knobs::*f; } ints[] = {
        {"PCP_FAN_BATCH", &Knobs::fan_batch},   {"PCP_NB_BLOCKS", &Knobs::nb_blocks},
        {"PCP_COPY_THREADS", &Knobs::copy_threads}, {"PCP_BK_GT", &Knobs::bk_gt},
        {"PCP_BK_PTS", &Knobs::bk_pts},         {"PCP_TERRAIN_BLOCKS", &Knobs::terrain_blocks},
        {"PCP_TERRAIN_FINE", &Knobs::terrain_fine}, {"PCP_FINE_TILE", &Knobs::fine_tile},
    };
    for (const auto &f : ints) {
        CHECK(parse({{f.name, "0"}}).*f.f == 0);
        CHECK(parse({{f.name, "5"}}).*f.f == 5);
        CHECK(parse({{f.name, "-3"}}).*f.f == -3);
        CHECK(parse({{f.name, ""}}).*f.f == 0);
        CHECK(parse({{f.name, "12abc"}}).*f.f == 12);
    }

    // the odd rows
    for (int w : {2, 4, 8, 16, 32})
        CHECK(parse({{"PCP_FAN_NPW", std::to_string(w)}}).fan_npw == w);
    for (const char *v : {"0", "1", "3", "6", "64", "-8", "", "x"})
        CHECK(parse({{"PCP_FAN_NPW", v}}).fan_npw == 1);
    CHECK(parse({{"PCP_FAN_CLIP", "1"}}).fan_clip_e == kClipSlack);
    CHECK(parse({{"PCP_FAN_CLIP", "-2"}}).fan_clip_e == kClipSlack);
    CHECK(parse({{"PCP_FAN_CLIP", "0"}}).fan_clip_e == kClipSlackWhole);
    CHECK(parse({{"PCP_FAN_CLIP", ""}}).fan_clip_e == kClipSlackWhole);
    CHECK(parse({{"PCP_SCORE_WIDE_RAYS", "0"}}).score_wide_rays == 0);
    CHECK(parse({{"PCP_SCORE_WIDE_RAYS", "5000000000"}}).score_wide_rays == 5000000000ll);
    CHECK(parse({{"PCP_SCORE_WIDE_RAYS", "-7"}}).score_wide_rays == -7);
    CHECK(parse({{"PCP_SCORE_WIDE_RAYS", ""}}).score_wide_rays == 0);
    for (int g : {2, 4, 8, 16})
        CHECK(parse({{"PCP_SCORE_WIDE_G", std::to_string(g)}}).score_wide_g == g);
    CHECK(parse({{"PCP_NB_REGION_PCT", "0"}}).nb_region_pct == 1);
    CHECK(parse({{"PCP_NB_REGION_PCT", "-5"}}).nb_region_pct == 1);
    CHECK(parse({{"PCP_NB_REGION_PCT", ""}}).nb_region_pct == 1);
    CHECK(parse({{"PCP_NB_REGION_PCT", "1"}}).nb_region_pct == 1);
    CHECK(parse({{"PCP_NB_REGION_PCT", "40"}}).nb_region_pct == 40);
    CHECK(parse({{"PCP_NB_REGION_PCT", "100"}}).nb_region_pct == 100);
    CHECK(parse({{"PCP_NB_REGION_PCT", "101"}}).nb_region_pct == 100);
    CHECK(parse({{"PCP_NB_GUESS_WORDS", "0"}}).nb_guess_max == 1);
    CHECK(parse({{"PCP_NB_GUESS_WORDS", ""}}).nb_guess_max == 1);
    CHECK(parse({{"PCP_NB_GUESS_WORDS", "1"}}).nb_guess_max == 1);
    CHECK(parse({{"PCP_NB_GUESS_WORDS", "4096"}}).nb_guess_max == 4096);
    CHECK(parse({{"PCP_NB_GUESS_WORDS", "8589934592"}}).nb_guess_max == 8589934592ull);
    CHECK(parse({{"PCP_FM_FAST", "0"}}).fm_fast == 0);
    CHECK(parse({{"PCP_FM_FAST", "1"}}).fm_fast == 1);
    CHECK(parse({{"PCP_FM_FAST", "2"}}).fm_fast == 2);
    CHECK(parse({{"PCP_FM_FAST", "3"}}).fm_fast == 2);
    CHECK(parse({{"PCP_FM_FAST", "-1"}}).fm_fast == 2);
    CHECK(parse({{"PCP_FM_FAST", ""}}).fm_fast == 0);
    CHECK(parse({{"PCP_FINE_SKIP", "2"}}).fine_skip == 2);
    CHECK(parse({{"PCP_FINE_SKIP", "1"}}).fine_skip == 1);
    CHECK(parse({{"PCP_FINE_SKIP", "0"}}).fine_skip == 1);
    CHECK(parse({{"PCP_FINE_SKIP", "3"}}).fine_skip == 1);
    CHECK(parse({{"PCP_FINE_SKIP", ""}}).fine_skip == 1);
    CHECK(parse({{"PCP_FINE_PACK", "5"}}).fine_pack == true);
    for (const char *v : {"1", "0", ""})   // presence alone
        CHECK(parse({{"PCP_HOST_BBOX_SCALAR", v}}).host_bbox_scalar == true);

    // a variable the table does not hold changes nothing
    check_defaults(parse({{"PCP_ALLOC_TRACE", "1"}, {"PCP_NO_SUCH_KNOB", "1"}}));

    // the one refusal: the error names the variable; PCP_FAN_NPW (a row before it) is parsed,
    // PCP_FM_FAST and PCP_NO_GRAPHS (rows after it) and the refused field keep their defaults
    for (const char *v : {"3", "8x", "", "0", "32", "-4", "8 "}) {
        g_env = {{"PCP_FAN_NPW", "4"}, {"PCP_SCORE_WIDE_G", v}, {"PCP_FM_FAST", "0"},
                 {"PCP_NO_GRAPHS", "1"}};
        Knobs k;
        std::string err;
        CHECK(knobs_from_env(k, fake_get, &err) != 0);
        CHECK(err.find("PCP_SCORE_WIDE_G") != std::string::npos);
        CHECK(err.find(std::string("\"") + v + "\"") != std::string::npos);
        CHECK(k.fan_npw == 4 && k.score_wide_g == 0 && k.fm_fast == 2 && k.use_graphs == true);
        CHECK(knobs_from_env(k, fake_get, nullptr) != 0);   // the message is optional
    }

    // every row once, by name: no name twice
    const std::vector<KnobRow> &rows = knob_rows();
    const size_t n = rows.size();
    for (size_t i = 0; i < n; ++i) {
        std::printf("var %s\n", rows[i].name);
        for (size_t j = 0; j < i; ++j) CHECK(std::strcmp(rows[i].name, rows[j].name) != 0);
    }
    CHECK(n == sizeof(flags) / sizeof(flags[0]) + sizeof(inverted) / sizeof(inverted[0]) +
                   sizeof(ints) / sizeof(ints[0]) + 9);   // + the nine odd rows above
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
