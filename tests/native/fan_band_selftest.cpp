// Stand-alone check of pcp_fan_band.hpp (DESIGN.md §5 Skip 7) with the host compiler: brute force
// over random small clouds and the samples of random rays.  Each sample is aimed at a position in
// a fine cell, on its edges, or within the probe's error of them, about r from a point of the
// cloud; the clouds lie up to 100 m out in xy and 1 km up or down in z, on grids a few cells or
// 1 km tall.  Whenever any point passes FLANN's float predicate for the sample's exact float
// position, the march's probe -- restated here in the same float operations -- must call the
// sample a candidate under the tight thresholds of the record it reads, and those must be no
// looser than the specified ones (zband_code + T).  No GPU call.  Prints "ok" on success.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pcp_fan_band.hpp"

using namespace pcp;

namespace {

int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++fails < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

struct P3 {
    float x, y, z;
};

constexpr double kC = 0.12, kR = 0.056, kM = 1e-3, kStepLen = 0.3;
constexpr float kZq = 2.0f / 250.0f;
constexpr int kF = 2;

// zband_code (pcp_grid.hpp) with the build's T folded in (pcp_fine.hip, k_frec)
uint32_t spec_word(float zmax, float zmin, double zb, uint32_t tsteps) {
    const double step = (double)kZq * kC;
    const double h = std::ceil(((double)zmax - zb) / step) + 1.0;
    const double l = std::floor(((double)zmin - zb) / step) - 1.0;
    const uint32_t hi = h >= 255.0 ? 255u : (uint32_t)std::fmax(h, 1.0);
    const uint32_t lo = l <= 0.0 ? 0u : (uint32_t)std::fmin(l, 254.0);
    const uint32_t lo2 = (lo == 0u || lo <= tsteps) ? 0u : lo - tsteps;
    const uint32_t hi2 = hi == 255u ? 255u : std::min(hi + tsteps, 255u);
    return lo2 | (hi2 << 8);
}

// FLANN's float predicate as the walk evaluates it
bool within(float qx, float qy, float qz, const P3 &p, float r2) {
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    return (dx * dx + dy * dy) + dz * dz < r2;
}

}  // namespace

int main() {
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double R = kR + kM, rho = kR + kBandMu, cf = kC / kF, step = (double)kZq * kC;
    const uint32_t tsteps = (uint32_t)std::ceil((kR + 2e-3) / kC / (double)kZq);
    const float r2 = (float)(kR * kR);
    long hits = 0, hits_near_edge = 0, hits_tightened = 0, samples = 0, tighter = 0, records = 0;
    for (int trial = 0; trial < 300; ++trial) {
        // the cloud: a patch of 0.6 m, level, sloped or two-storeyed, somewhere within 100 m in
        // xy and 1 km in z; every third cloud has an outlier 1 km away in z (a tall grid: large
        // cell coordinates in the probe)
        const double X0 = (trial & 1) ? (U(rng) - 0.5) * 200.0 : U(rng), Y0 = (trial & 2) ? (U(rng) - 0.5) * 200.0 : -U(rng);
        const double Z0 = (trial & 4) ? (U(rng) - 0.5) * 2000.0 : U(rng);
        const int kind = trial % 3;
        std::vector<P3> pts;
        const int n = 40 + (int)(U(rng) * 80.0);
        for (int i = 0; i < n; ++i) {
            const double x = 0.6 * U(rng), y = 0.6 * U(rng);
            const double z = kind == 0 ? 0.01 * U(rng) : kind == 1 ? x + 0.01 * U(rng)
                                                                   : (U(rng) < 0.5 ? 0.0 : 0.17) + 0.01 * U(rng);
            pts.push_back(P3{(float)(X0 + x), (float)(Y0 + y), (float)(Z0 + z)});
        }
        if (trial % 3 == 2) pts.push_back(P3{(float)(X0 + 0.3), (float)(Y0 + 0.3), (float)(Z0 + ((trial & 8) ? 1000.0 : -1000.0))});
        // the grid as the index lays it (GridIndex::view): one padding cell around the points
        double bmin[3] = {1e300, 1e300, 1e300}, bmax[3] = {-1e300, -1e300, -1e300};
        for (const P3 &p : pts) {
            const double v[3] = {p.x, p.y, p.z};
            for (int a = 0; a < 3; ++a) {
                bmin[a] = std::fmin(bmin[a], v[a]);
                bmax[a] = std::fmax(bmax[a], v[a]);
            }
        }
        const double ox = bmin[0] - kC, oy = bmin[1] - kC, oz = bmin[2] - kC, inv_c = 1.0 / kC;
        int nc[3];
        for (int a = 0; a < 3; ++a) nc[a] = (int)std::floor((bmax[a] - bmin[a]) / kC) + 3;
        const int fnx = kF * nc[0], fny = kF * nc[1], rz = nc[2] - 1;
        const float flo_x = (float)(ox + R), flo_y = (float)(oy + R), flo_z = (float)(oz + R);
        const float finv_c = (float)inv_c, fzoff = (float)(R * inv_c);
        const float fus_off = (float)(R * inv_c / (double)kZq);
        for (int s = 0; s < 400; ++s) {
            // the aim: about r from a point of the patch, its xy in a cell, on an edge or a
            // corner of one, or a probe's error (1e-5 m, and ulps of the coordinate) beside one
            const P3 &a = pts[(size_t)(U(rng) * n) % (size_t)n];
            const double len = kR * (0.7 + 0.4 * U(rng)), ph = 2.0 * M_PI * U(rng), ct = 2.0 * U(rng) - 1.0;
            const double st = std::sqrt(1.0 - ct * ct);
            double t[3] = {a.x + len * st * std::cos(ph), a.y + len * st * std::sin(ph), a.z + len * ct};
            const int mode = s % 4;
            if (mode) {
                const double ex = ox + std::round((t[0] - ox) / cf) * cf, ey = oy + std::round((t[1] - oy) / cf) * cf;
                const double off = mode == 3 ? (U(rng) - 0.5) * 2e-5 : 0.0;
                if (mode != 2 || U(rng) < 0.5) t[0] = ex + off;
                if (mode == 2 || U(rng) < 0.3) t[1] = ey + off;
            }
            // the ray: any direction, grazing ones among them, the sample k of it at the aim
            const double dph = 2.0 * M_PI * U(rng), el = (s & 8) ? -0.07 * U(rng) : M_PI * (U(rng) - 0.5);
            const double d[3] = {std::cos(el) * std::cos(dph), std::cos(el) * std::sin(dph), std::sin(el)};
            const int k = (s & 16) ? (int)(U(rng) * 400.0) : (int)(U(rng) * 49.0);
            double sk = 0.5;
            for (int i = 0; i < k; ++i) sk += kStepLen;   // the step table's additions
            const double p[3] = {t[0] - d[0] * sk, t[1] - d[1] * sk, t[2] - d[2] * sk};
            // the exact sample, as the march computes it for a candidate
            const float qx = (float)(p[0] + d[0] * sk), qy = (float)(p[1] + d[1] * sk), qz = (float)(p[2] + d[2] * sk);
            bool hit = false;
            for (const P3 &q : pts) hit |= within(qx, qy, qz, q, r2);
            // the probe (march, FN 8), operation by operation in float
            const float fdx = (float)d[0], fdy = (float)d[1], fdz = (float)d[2];
            const float sc = (float)kStepLen * finv_c, h = 0.5f * finv_c;
            const float Dx = fdx * sc, Dy = fdy * sc, Dz = fdz * sc;
            const float Ax = ((float)p[0] - flo_x) * finv_c + fdx * h;
            const float Ay = ((float)p[1] - flo_y) * finv_c + fdy * h;
            const float Az = ((float)p[2] - flo_z) * finv_c + fdz * h;
            const float F = (float)kF;
            const float D2x = F * Dx, D2y = F * Dy, A2x = F * (Ax + fzoff), A2y = F * (Ay + fzoff);
            const float kf = (float)k;
            const float fx = std::fmaf(D2x, kf, A2x), fy = std::fmaf(D2y, kf, A2y), fz = std::fmaf(Dz, kf, Az);
            const uint32_t ix = std::min((uint32_t)std::fmax(fx, 0.0f), (uint32_t)fnx - 1u);
            const uint32_t iy = std::min((uint32_t)std::fmax(fy, 0.0f), (uint32_t)fny - 1u);
            const uint32_t iz = std::min((uint32_t)std::fmax(fz, 0.0f), (uint32_t)rz - 1u);
            const float us = std::fmaf(fz - (float)iz, 1.0f / kZq, fus_off);
            // record (W, iz): the window's entries in coarse z cells iz, iz + 1, both rules
            BandAcc acc = fan_band_begin();
            float zmax = -INFINITY, zmin = INFINITY;
            for (const P3 &q : pts) {
                const double dd = fan_band_dist(ox, oy, cf, (int)ix, (int)iy, (double)q.x, (double)q.y);
                if (!(dd * dd <= R * R)) continue;
                const int cz = std::min(std::max((int)std::floor(((double)q.z - oz) * inv_c), 0), nc[2] - 1);
                if (cz < (int)iz || cz > (int)iz + 1) continue;
                zmax = std::fmax(zmax, q.z);
                zmin = std::fmin(zmin, q.z);
                fan_band_add(acc, (double)q.z, dd, kM, rho);
            }
            ++samples;
            if (zmax == -INFINITY) {   // an empty record: no candidate, so no point may be within r
                CHECK(!hit);
                continue;
            }
            const double zb = oz + (double)iz * kC;
            const uint32_t spec = spec_word(zmax, zmin, zb, tsteps);
            const uint32_t word = fan_band_word(acc, zb, step, spec);
            const uint32_t lo = word & 255u, hi = word >> 8, slo = spec & 255u, shi = spec >> 8;
            ++records;
            CHECK(acc.any);   // an entry of the window lies within r + m of the cell: it takes part
            CHECK(lo >= slo && hi <= shi && lo <= 254u);
            tighter += (lo > slo) + (hi < shi);
            const bool cand = (us < (float)hi) & (us > (float)lo);
            const bool cand_spec = (us < (float)shi) & (us > (float)slo);
            if (hit) {
                CHECK(cand_spec);
                CHECK(cand);
                if (!cand && fails < 20)
                    std::printf("  trial %d sample %d: us %.4f lo %u hi %u (specified %u %u)\n", trial, s,
                                (double)us, lo, hi, slo, shi);
                ++hits;
                hits_tightened += (lo > slo) || (hi < shi);
                hits_near_edge += (us > (float)hi - 8.0f) || (us < (float)lo + 8.0f);
            }
        }
    }
    std::printf("samples %ld records %ld tightened thresholds %ld hits %ld (in tightened records %ld, "
                "within 8 steps of a threshold %ld)\n",
                samples, records, tighter, hits, hits_tightened, hits_near_edge);
    // the run is not vacuous
    CHECK(hits > 20000 && hits_tightened > 5000 && hits_near_edge > 100 && tighter > records / 4);
    // no entry takes part: thresholds no sample satisfies, and not the empty mark
    {
        BandAcc a = fan_band_begin();
        fan_band_add(a, 1.0, rho + kM, kM, rho);
        const uint32_t w = fan_band_word(a, 0.0, step, 0xFF00u);
        CHECK(!a.any && (w & 255u) == 254u && (w >> 8) == 0u);
    }
    if (fails) {
        std::printf("%d failures\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
