// pcp_aim.hpp on the host: the aims' table (the infinite bounds, h_fov >= 2 pi), the predicate at
// its edges, the argument check and the plan of the call's blocks.  Stand-alone: prints "ok" and
// returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pcp_abi.h"
#include "pcp_aim.hpp"

using namespace pcp;

static int fails = 0;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            ++fails;                  \
        }                             \
    } while (0)

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void check_tables() {
    const double d = kAimPi / 180.0;
    // pitch -45 with v_fov 90: lo = -90 exactly -> -inf; pitch 45: hi = 90 -> +inf
    const double aims[] = {0.0, -45 * d, 0.5, 45 * d, -1.25, 0.0, 3.0, -kAimPi2, 3.0, kAimPi2};
    AimRow r[5];
    double ch = 0;
    const double v = 90 * d;
    CHECK(aim_rows(aims, 5, 90 * d, v, r, &ch) == 0, "90 degrees has a horizontal test");
    CHECK(same(ch, std::cos(90 * d * 0.5)), "ch");
    for (int a = 0; a < 5; ++a) {
        CHECK(same(r[a].ca, std::cos(aims[2 * a])) && same(r[a].sa, std::sin(aims[2 * a])),
              "aim %d: cos / sin of the offset", a);
        const double lo = aims[2 * a + 1] - v * 0.5, hi = aims[2 * a + 1] + v * 0.5;
        CHECK(same(r[a].tlo, lo <= -kAimPi2 ? -INFINITY : std::tan(lo)), "aim %d: tlo", a);
        CHECK(same(r[a].thi, hi >= kAimPi2 ? INFINITY : std::tan(hi)), "aim %d: thi", a);
    }
    CHECK(r[0].tlo == -INFINITY && std::isfinite(r[0].thi), "aim 0: lo reaches -90");
    CHECK(r[1].thi == INFINITY && std::isfinite(r[1].tlo), "aim 1: hi reaches 90");
    CHECK(std::isfinite(r[2].tlo) && std::isfinite(r[2].thi) && r[2].tlo < 0 && r[2].thi > 0,
          "aim 2: both bounds finite");
    CHECK(r[3].tlo == -INFINITY && r[4].thi == INFINITY, "aims at the vertical");
    // a bound just inside the vertical stays finite (tan of it is large, not infinite)
    const double near[] = {0.0, -45 * d + 1e-12};
    AimRow q;
    aim_rows(near, 1, 1.0, v, &q, &ch);
    CHECK(near[1] - v * 0.5 > -kAimPi2 && std::isfinite(q.tlo) && q.tlo < -1e11,
          "lo just above -90: %g", q.tlo);
    const double in[] = {0.0, 0.0};
    // h_fov at and around 2 pi; pi as the whole band
    CHECK(aim_rows(in, 1, 2.0 * kAimPi, kAimPi, &q, &ch) == 1, "2 pi: no horizontal test");
    CHECK(q.tlo == -INFINITY && q.thi == INFINITY, "v_fov = pi about pitch 0");
    CHECK(aim_rows(in, 1, 7.0, 1.0, &q, &ch) == 1, "past 2 pi");
    CHECK(aim_rows(in, 1, std::nextafter(2.0 * kAimPi, 0.0), 1.0, &q, &ch) == 0, "just under 2 pi");
    const double poses[] = {1, 2, 3, 0.25, 0.75, 4, 5, 6, 0.0, NAN};
    double cs[4];
    aim_pose_rows(poses, 2, cs);
    CHECK(same(cs[0], std::cos(0.75)) && same(cs[1], std::sin(0.75)), "pose 0: cos / sin of yaw");
    CHECK(std::isnan(cs[2]) && std::isnan(cs[3]), "a NaN yaw gives NaN rows");
}

static void check_predicate() {
    const double d = kAimPi / 180.0;
    const double aims[] = {0.0, -45 * d, 0.0, 0.0, 0.0, 45 * d};
    AimRow r[3];
    double ch;
    aim_rows(aims, 3, 90 * d, 90 * d, r, &ch);
    double Cy, Sy;
    aim_heading(1.0, 0.0, r[0].ca, r[0].sa, Cy, Sy);   // yaw 0, offset 0: looks along +x
    CHECK(Cy == 1.0 && Sy == 0.0, "heading");
    // straight below: hyp = 0, -inf * 0 = NaN counts as inside for aim 0 only
    AimGeo g = aim_geo(0, 0, -2, 0, 0, 0, ch);
    CHECK(g.hyp == 0 && aim_sees(g, Cy, Sy, r[0].tlo, r[0].thi, false), "straight below, lo = -90");
    CHECK(!aim_sees(g, Cy, Sy, r[1].tlo, r[1].thi, false), "straight below, lo = -45");
    // straight above: only the aim whose upper bound reaches 90
    g = aim_geo(0, 0, 2, 0, 0, 0, ch);
    CHECK(aim_sees(g, Cy, Sy, r[2].tlo, r[2].thi, false), "straight above, hi = 90");
    CHECK(!aim_sees(g, Cy, Sy, r[1].tlo, r[1].thi, false), "straight above, hi = 45");
    // ahead, behind, and behind without a horizontal test
    g = aim_geo(3, 0.5, 0, 0, 0, 0, ch);
    CHECK(aim_sees(g, Cy, Sy, r[1].tlo, r[1].thi, false), "ahead");
    g = aim_geo(-3, 0, 0, 0, 0, 0, ch);
    CHECK(!aim_sees(g, Cy, Sy, r[1].tlo, r[1].thi, false), "behind");
    CHECK(aim_sees(g, Cy, Sy, r[1].tlo, r[1].thi, true), "behind, h_fov >= 2 pi");
    // a NaN heading sees nothing under a horizontal test
    g = aim_geo(3, 0, 0, 0, 0, 0, ch);
    CHECK(!aim_sees(g, NAN, NAN, r[1].tlo, r[1].thi, false), "NaN yaw");
    // the rotation's sense: offset +90 degrees looks along +y
    const double left[] = {90 * d, 0.0};
    aim_rows(left, 1, 90 * d, 90 * d, r, &ch);
    aim_heading(1.0, 0.0, r[0].ca, r[0].sa, Cy, Sy);
    g = aim_geo(0, 3, 0, 0, 0, 0, ch);
    CHECK(aim_sees(g, Cy, Sy, r[0].tlo, r[0].thi, false), "offset +90 sees +y");
    g = aim_geo(0, -3, 0, 0, 0, 0, ch);
    CHECK(!aim_sees(g, Cy, Sy, r[0].tlo, r[0].thi, false), "offset +90 does not see -y");
}

static pcp_aim_params good() {
    pcp_aim_params ap;
    std::memset(&ap, 0, sizeof ap);
    ap.k_max = 3;
    ap.n_aims = 2;
    ap.h_fov = 1.5;
    ap.v_fov = 1.0;
    return ap;
}

static void check_args() {
    const double aims[] = {0.0, 0.0, 1.0, -0.5};
    int bad = -1;
    pcp_aim_params ap = good();
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimOk, "a valid call refused");
    CHECK(aim_check(&ap, aims, 0, &bad) == kAimOk, "no poses refused");
    ap.k_max = 0;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimKmax, "k_max 0");
    ap.k_max = PCP_PLACE_MAX + 1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimKmax, "k_max past the limit");
    ap = good();
    ap.n_aims = 0;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimCount, "n_aims 0");
    ap.n_aims = PCP_AIM_MAX + 1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimCount, "n_aims past the limit");
    ap = good();
    ap.n_fixed = -1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimFixedCount, "n_fixed -1");
    ap.n_fixed = PCP_PLACE_MAX + 1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimFixedCount, "n_fixed past the limit");
    ap = good();
    ap.reserved = 1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimReserved, "reserved");
    for (double h : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
        ap = good();
        ap.h_fov = h;
        CHECK(aim_check(&ap, aims, 10, &bad) == kAimHfov, "h_fov %g", h);
    }
    for (double v : {0.0, -1.0, std::nextafter(kAimPi, 4.0), (double)INFINITY, (double)NAN}) {
        ap = good();
        ap.v_fov = v;
        CHECK(aim_check(&ap, aims, 10, &bad) == kAimVfov, "v_fov %g", v);
    }
    ap = good();
    ap.v_fov = kAimPi;
    ap.h_fov = 100.0;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimOk, "v_fov = pi, h_fov = 100 refused");
    ap = good();
    const double nan_aim[] = {0.0, 0.0, NAN, 0.0}, steep[] = {0.0, std::nextafter(kAimPi2, 2.0)},
                 inf_aim[] = {0.0, 0.0, 0.0, -INFINITY}, edge[] = {0.0, kAimPi2, 9.0, -kAimPi2};
    CHECK(aim_check(&ap, nan_aim, 10, &bad) == kAimAim && bad == 1, "NaN offset: aim %d", bad);
    CHECK(aim_check(&ap, steep, 10, &bad) == kAimAim && bad == 0, "pitch past 90: aim %d", bad);
    CHECK(aim_check(&ap, inf_aim, 10, &bad) == kAimAim && bad == 1, "infinite pitch: aim %d", bad);
    CHECK(aim_check(&ap, edge, 10, &bad) == kAimOk, "pitches of +-90 refused");
    CHECK(aim_check(&ap, aims, PCP_PAIR_MAX_POSES, &bad) == kAimOk, "the most poses refused");
    CHECK(aim_check(&ap, aims, PCP_PAIR_MAX_POSES + 1, &bad) == kAimPoses, "too many poses");
    std::vector<double> many(2 * PCP_AIM_MAX, 0.0);
    ap.n_aims = PCP_AIM_MAX;
    CHECK(aim_check(&ap, many.data(), PCP_AIM_MAX_ROWS / PCP_AIM_MAX, &bad) == kAimOk,
          "the most rows refused");
    CHECK(aim_check(&ap, many.data(), PCP_AIM_MAX_ROWS / PCP_AIM_MAX + 1, &bad) == kAimRows,
          "too many rows");
    ap = good();
    ap.n_fixed = 3;
    ap.fixed_pose[0] = 4, ap.fixed_pose[1] = 0, ap.fixed_pose[2] = 9;
    ap.fixed_aim[0] = 1, ap.fixed_aim[1] = 0, ap.fixed_aim[2] = 1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimOk, "a valid fixed list refused");
    CHECK(aim_check(&ap, aims, 9, &bad) == kAimFixedPose && bad == 2, "fixed pose == n: %d", bad);
    ap.fixed_pose[2] = 4;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimFixedTwice && bad == 2, "fixed twice: %d", bad);
    ap.fixed_pose[2] = 9;
    ap.fixed_aim[1] = 2;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimFixedAim && bad == 1, "fixed aim == A: %d", bad);
    ap.fixed_aim[1] = -1;
    CHECK(aim_check(&ap, aims, 10, &bad) == kAimFixedAim && bad == 1, "fixed aim -1: %d", bad);
}

static void check_plan() {
    for (int C : {1, 63, 64, 65, 3704})
        for (int P : {0, 1, 17, 91})
            for (int A : {1, 2, 45, 64})
                for (int K : {1, 3, 16}) {
                    const AimPlan s = aim_plan(352, C, P, A, K);
                    const size_t rows = (size_t)P * A;
                    CHECK(s.rows() == rows, "rows");
                    CHECK(s.cb.score_off >= 352 && s.rt_off == s.cb.rest_off, "the cells' front");
                    CHECK(s.rt_off % 16 == 0 && s.rc_off % 16 == 0 && s.al_off % 16 == 0 &&
                              s.bytes % 16 == 0 && s.ta_off % 16 == 0,
                          "C %d P %d A %d K %d: alignment", C, P, A, K);
                    CHECK(s.rc_off >= s.rt_off + K * rows * sizeof(double) &&
                              s.al_off >= s.rc_off + K * rows * sizeof(int32_t) &&
                              s.bytes >= s.al_off + P * sizeof(uint32_t),
                          "C %d P %d A %d K %d: the parts overlap", C, P, A, K);
                    CHECK(s.ta_off >= (size_t)P * 2 * sizeof(double) &&
                              s.tab_bytes == s.ta_off + A * sizeof(AimRow),
                          "the tables");
                    // the download is a prefix: the state alone, + the cells, + the round totals
                    CHECK(s.down(false, false) == s.cb.score_off && s.down(false, true) == s.rt_off &&
                              s.down(true, false) == s.rc_off && s.down(true, true) == s.rc_off,
                          "the download's span");
                    CHECK(s.down(true, true) <= s.bytes, "the download leaves the block");
                }
}

int main() {
    check_tables();
    check_predicate();
    check_args();
    check_plan();
    if (fails)
        std::printf("FAILED (%d)\n", fails);
    else
        std::printf("ok\n");
    return fails ? 1 : 0;
}
