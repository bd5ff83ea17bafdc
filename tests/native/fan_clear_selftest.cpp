// Stand-alone check of pcp_fan_clear.hpp (DESIGN.md §5 Skip 5) with the host compiler: the
// clearance codes of a small fine grid against brute force, and the march's jump against
// every point of the set.  No GPU call.  Prints "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pcp_fan_clear.hpp"

using namespace pcp;

namespace {

constexpr int FN = 32, RZ = 6;                       // 32 x 32 fine cells, 6 record levels
constexpr double C = 0.12, CF = 0.06, R = 0.056, M = 1e-3, RM = R + M;
constexpr double OX = 10.0, OY = -7.0, OZ = -0.5;

int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++fails < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

struct Set {
    std::vector<double> xyz;
    size_t n() const { return xyz.size() / 3; }
    void add(double x, double y, double z) {
        xyz.push_back(x);
        xyz.push_back(y);
        xyz.push_back(z);
    }
};

// a top sheet with holes inside an empty border, and a buried layer under part of it
Set make_set(std::mt19937 &rng) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    Set s;
    const int border = (int)(U(rng) * 8.0);           // empty border, in fine cells
    const double keep = 0.15 + 0.85 * U(rng);         // top-sheet density
    const double ztop = OZ + 0.35 + 0.3 * U(rng), zlow = OZ + 0.05 + 0.15 * U(rng);
    const double split = U(rng);                      // the buried layer lies at x below split
    const bool buried = U(rng) < 0.7;
    for (int y = border; y < FN - border; ++y)
        for (int x = border; x < FN - border; ++x) {
            const double px = OX + (x + U(rng)) * CF, py = OY + (y + U(rng)) * CF;
            const bool top = U(rng) < keep;
            if (top) s.add(px, py, ztop + 0.01 * (U(rng) - 0.5));
            if (buried && x < split * FN && U(rng) < 0.5)   // two-layer columns where top holds
                s.add(OX + (x + U(rng)) * CF, OY + (y + U(rng)) * CF, zlow + 0.01 * (U(rng) - 0.5));
        }
    return s;
}

bool any_within(const Set &s, double qx, double qy, double qz) {
    for (size_t i = 0; i < s.n(); ++i) {
        const double dx = s.xyz[3 * i] - qx, dy = s.xyz[3 * i + 1] - qy, dz = s.xyz[3 * i + 2] - qz;
        if (dx * dx + dy * dy + dz * dz <= R * R) return true;
    }
    return false;
}

}  // namespace

int main() {
    std::mt19937 rng(20260227u);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double zabs = std::fmax(std::fabs(OZ), std::fabs(OZ + (RZ + 1) * C));
    const ClearGeo cg = fan_clear_geo(OZ, C, RM, zabs);
    const float rb = std::nextafter((float)(RM + 1e-6 * 10.0), INFINITY), cf = (float)CF;
    long skipped = 0, jumps = 0, rays = 0;

    // levels: the smallest iz with z <= Zt(iz)
    for (int q = 0; q < 2000; ++q) {
        const double z = OZ - 0.3 + 1.5 * U(rng);
        const int l = fan_clear_level(cg, z, RZ);
        CHECK(l >= 0 && l <= RZ);
        CHECK(l == RZ || z <= fan_clear_ztop(cg, l));
        CHECK(l == 0 || z > fan_clear_ztop(cg, l - 1));
    }

    for (int trial = 0; trial < 10; ++trial) {
        const Set s = make_set(rng);
        // the build's passes over the cells' lowest levels
        std::vector<uint32_t> lev((size_t)FN * FN, 0xFFFFFFFFu);
        for (size_t i = 0; i < s.n(); ++i) {
            const int cx = std::min(std::max((int)std::floor((s.xyz[3 * i] - OX) / CF), 0), FN - 1);
            const int cy = std::min(std::max((int)std::floor((s.xyz[3 * i + 1] - OY) / CF), 0), FN - 1);
            const uint32_t l = (uint32_t)fan_clear_level(cg, s.xyz[3 * i + 2], RZ);
            lev[(size_t)cy * FN + cx] = std::min(lev[(size_t)cy * FN + cx], l);
        }
        std::vector<uint8_t> grid;
        fan_clear_grid(lev, FN, FN, RZ, grid);
        // the reference: the code's meaning from the point list; the passes never promise more
        std::vector<uint8_t> ref((size_t)FN * FN * RZ);
        long informative = 0;
        for (int iz = 0; iz < RZ; ++iz)
            for (int y = 0; y < FN; ++y)
                for (int x = 0; x < FN; ++x) {
                    const size_t r = ((size_t)iz * FN + y) * FN + x;
                    ref[r] = (uint8_t)fan_clear_ref(s.xyz.data(), s.n(), OX, OY, CF, x, y, cg, iz);
                    CHECK(grid[r] <= ref[r]);
                    if (fan_clear_border(x, y, iz, FN, FN, RZ)) CHECK(grid[r] == 0);
                    else CHECK(ref[r] == grid[r]);   // (the passes are exact inside the border)
                    informative += grid[r] > 0;
                }
        if (s.n() > 0 && s.n() < (size_t)FN * FN / 2) CHECK(informative > 0);

        // descending rays through the grid, production step and a short one (more samples)
        for (int q = 0; q < 150; ++q) {
            const float step = (q & 1) ? 0.3f : 0.05f;
            const double az = 6.283185307179586 * U(rng), el = -(0.02 + 1.5 * U(rng));
            const double dx = std::cos(el) * std::cos(az), dy = std::cos(el) * std::sin(az),
                         dz = std::sin(el);
            // aimed at a random spot of the grid's mid-height plane, started 0.5 + a bit before
            const double tx = OX + FN * CF * U(rng), ty = OY + FN * CF * U(rng),
                         tz = OZ + RZ * C * U(rng), back = 0.5 + 2.0 * U(rng);
            const double px = tx - dx * back, py = ty - dy * back, pz = tz - dz * back;
            const ClearRay cr = fan_clear_ray((float)dx, (float)dy, (float)dz, step, cf, rb, true);
            CHECK(cr.a > 0.0f && cr.b > 0.0f);
            ++rays;
            for (int pass = 0; pass < 2; ++pass) {
                const std::vector<uint8_t> &code = pass ? grid : ref;
                for (int k = 0; k < 200; ++k) {
                    const double sk = 0.5 + (double)step * k;
                    const double qx = px + dx * sk, qy = py + dy * sk, qz = pz + dz * sk;
                    // the probe's cell mapping (fine x, y; coarse corner z), in float
                    const float fx = (float)((qx - OX) / CF), fy = (float)((qy - OY) / CF),
                                fz = (float)((qz - OZ - RM) / C);
                    // clamped as the march clamps: a sample outside the grid reads a border record
                    const int ix = std::min((int)std::fmax(fx, 0.0f), FN - 1),
                              iy = std::min((int)std::fmax(fy, 0.0f), FN - 1),
                              iz = std::min((int)std::fmax(fz, 0.0f), RZ - 1);
                    const bool outside = !(fx >= 0.0f && fx < FN && fy >= 0.0f && fy < FN &&
                                           fz >= 0.0f && fz < RZ);
                    const size_t r = ((size_t)iz * FN + iy) * FN + ix;
                    if (outside) CHECK(grid[r] == 0);
                    if (outside && !pass) continue;   // (the meaning alone says nothing there)
                    const int n = fan_clear_skip((float)code[r], cr);
                    CHECK(n >= 0 && (!outside || n == 0));
                    if (n > 0) ++jumps;
                    for (int j = k + 1; j <= k + n && j < 200; ++j) {
                        const double sj = 0.5 + (double)step * j;
                        ++skipped;
                        CHECK(!any_within(s, px + dx * sj, py + dy * sj, pz + dz * sj));
                    }
                }
            }
        }
    }
    CHECK(rays > 0 && jumps > 1000 && skipped > jumps);

    // saturation: 255 = "at least 255 cells", never further; an empty set saturates
    CHECK(fan_clear_code(0) == 0 && fan_clear_code(1) == 0 && fan_clear_code(2) == 1);
    CHECK(fan_clear_code(256) == 255 && fan_clear_code(300) == 255 && fan_clear_code(100000) == 255);
    CHECK(fan_clear_ref(nullptr, 0, OX, OY, CF, 3, 4, cg, 2) == 255);
    for (int q = 0; q < 20000; ++q) {
        const double el = -(1e-4 + 1.5706 * U(rng)), az = 6.283185307179586 * U(rng);
        const float dx = (float)(std::cos(el) * std::cos(az)), dy = (float)(std::cos(el) * std::sin(az)),
                    dz = (float)std::sin(el);
        const ClearRay cr = fan_clear_ray(dx, dy, dz, 0.3f, cf, rb, true);
        const double hs = 0.3 * std::sqrt((double)dx * dx + (double)dy * dy);
        for (uint32_t e : {1u, 2u, 7u, 100u, 255u}) {
            const int n = fan_clear_skip((float)e, cr);
            if (hs > 1e-5) CHECK((double)n * hs <= (double)e * CF - (double)rb);   // (uncapped 1 / hs)
            if (hs > 1e-5) CHECK((double)n * hs <= 255.0 * CF);
        }
    }
    // a vertical ray: the capped reciprocal, a large finite jump
    {
        const ClearRay cr = fan_clear_ray(0.0f, 0.0f, -1.0f, 0.3f, cf, rb, true);
        CHECK(cr.a > 0.0f && cr.a < 1e5f && cr.b > 0.0f);
        CHECK(fan_clear_skip(0.0f, cr) == 0);
        const int n = fan_clear_skip(255.0f, cr);
        CHECK(n > 4096 && n < (1 << 24));
    }
    // nothing is skipped: a ray that does not descend, the knob off, no information
    for (uint32_t e = 0; e <= 255; ++e) {
        CHECK(fan_clear_skip((float)e, fan_clear_ray(0.6f, 0.0f, 0.8f, 0.3f, cf, rb, true)) == 0);
        CHECK(fan_clear_skip((float)e, fan_clear_ray(1.0f, 0.0f, 0.0f, 0.3f, cf, rb, true)) == 0);
        CHECK(fan_clear_skip((float)e, fan_clear_ray(0.6f, 0.0f, -0.8f, 0.3f, cf, rb, false)) == 0);
        CHECK(fan_clear_skip((float)e, fan_clear_ray(0.6f, 0.0f, NAN, 0.3f, cf, rb, true)) == 0);
    }
    for (float el : {-0.01f, -0.5f, -1.2f, -1.5707f})
        CHECK(fan_clear_skip(0.0f, fan_clear_ray(std::cos(el), 0.0f, std::sin(el), 0.3f, cf, rb, true)) == 0);
    // the border: the outermost cells and levels, and only they
    CHECK(fan_clear_border(0, 5, 2, 32, 32, 6) && fan_clear_border(31, 5, 2, 32, 32, 6));
    CHECK(fan_clear_border(5, 0, 2, 32, 32, 6) && fan_clear_border(5, 31, 2, 32, 32, 6));
    CHECK(fan_clear_border(5, 5, 0, 32, 32, 6) && fan_clear_border(5, 5, 5, 32, 32, 6));
    CHECK(!fan_clear_border(1, 1, 1, 32, 32, 6) && !fan_clear_border(30, 30, 4, 32, 32, 6));

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("rays %ld jumps %ld skipped samples %ld\nok\n", rays, jumps, skipped);
    return 0;
}
