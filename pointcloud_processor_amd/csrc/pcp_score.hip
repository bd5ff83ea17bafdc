// pcp_score.hip -- virtual_lidar.cpp's scoring on gfx950: candidate generation, per (pose,
// cell) visibility scoring over the shared march (pcp_march.hpp), the ordered row sums and cell
// flags, and the score keys of the pose-sharded search.  The dense ray fan is pcp_fan.hip.
//
// Numerics: compiled with -ffp-contract=off (no FMA) so every double/float operation
// rounds exactly as the reference's SSE2 build.  The radius predicate restates FLANN's
// L2_Simple<float> (x, y, z accumulated in order, strict '<' against float(r*r)).
// Build knobs of this file: PCP_SCORE_ULP, PCP_SCORE_OCML, PCP_CELL_EXP, PCP_SCORE_WAVES,
// PCP_SUM_ROWS / PCP_SUM_LPT / PCP_SUM_BATCH, PCP_ROW_SUM_LANES.
#pragma clang fp contract(off)

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "pcp_crmath.h"
#include "pcp_internal.hpp"
#include "pcp_march.hpp"

namespace pcp {

// ---------------------------------------------------------------------------------------
// cell scoring (evaluateCellScore, virtual_lidar.cpp:656-714)
// ---------------------------------------------------------------------------------------
struct VisEnv {
    GridView terrain;
    GridView aux;
    int terrain_present;   // terrain_kdtree_ non-null
    int aux_present;       // zx120 tree non-null and cloud non-empty
    double max_distance;
    const double *steps;
    int K;
    float r2_ray, r2_relaxed;
    float rexit_ray;       // exit_dist(r2_ray)
};

// evaluateCellScore's score of a visible cell (:689-700): the cosine d = |dot| clamped to
// [0, 1] gives sin(pi / 2 - acos(d)) (score_sin_part), then + 1 / L and the clamp at 0
// (score_finish).  glibc's acos and sin, which the reference calls, round correctly but for
// rare near ties: ocml's first results, then the midpoint tests / one rounding of pcp_crmath.h
// (ocml alone left 9 % of the cell scores off by 1-8 ulps, test_parity_bar_per_cell)
__device__ __forceinline__ double score_sin_part(double ad) {
#ifdef PCP_SCORE_OCML   // A/B build only (tools/r6_cr_ab.sh): ocml's acos / sin as they come
    return sin(kPi / 2 - acos(ad));
#else
    return pcp_score_sin_part(ad, acos(ad), nullptr);   // (two phases, pcp_crmath.h)
#endif
}

__device__ __forceinline__ double score_finish(double sin_part, double L, int cell) {
    const double score = 1.0 * sin_part + 1.0 * (1.0 / L);
#if PCP_SCORE_ULP   // parity-bar check builds only: the score of every PCP_SCORE_ULP-th cell
                    // one ulp up (make perturb: every cell; make perturb8: every 8th)
    if (cell % PCP_SCORE_ULP == 0) return fmax(0.0, nextafter(score, INFINITY));
#else
    (void)cell;
#endif
    return fmax(0.0, score);
}

// result bits: 1 = in_range, 2 = in_fov (valid if in_range), 4 = visible (valid if both)
// G > 1: the G lanes of an aligned lane group evaluate the same (pose, cell), each marching the
// samples koff (mod G) (march's koff / kstr); every lane returns the same result
// STATS (pcp_score_poses_stats): the march's probes / walk starts / point tests into cnt[0..2]
template <int G = 1, bool STATS = false>
__device__ __forceinline__ double eval_cell(const VisEnv &E, double px, double py, double pz,
                                            double pitch, double cx, double cy, double cz,
                                            float nx, float ny, float nz, bool is_zx120,
                                            uint32_t &bits, const double *steps,
                                            uint32_t *cnt = nullptr, int cell = 0) {
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double L = sqrt(dx * dx + dy * dy + dz * dz);
    bits = 0;
    const bool in_range = (L >= kMinDistance && L <= E.max_distance);
    if (!in_range) return 0.0;
    bits |= 1u;
    const double fov_local = 180.0 * kPi / 180.0;
    // the FOV decision, exactly the reference's double one: a float atan2 (error < 1e-6 rad
    // including the rounding of its arguments) decides every case farther than 1e-5 rad from
    // the boundary; the double atan2 only the rest
    const double h2 = dx * dx + dy * dy;
    const double dfast = (double)atan2f((float)dz, sqrtf((float)h2)) - pitch;
    if (fabs(dfast) > fov_local / 2.0 + 1e-5) return 0.0;
    if (!(fabs(dfast) < fov_local / 2.0 - 1e-5)) {
        const double elevation = atan2(dz, sqrt(h2));
        const double elevation_diff = elevation - pitch;
        if (!(fabs(elevation_diff) <= fov_local / 2.0)) return 0.0;
    }
    bits |= 2u;
    bool visible;
    const double ndx = dx / L, ndy = dy / L, ndz = dz / L;
    const double end = L - kVisRadius;
    if (is_zx120 && E.aux_present &&
        stencil_any(E.aux, (float)cx, (float)cy, (float)cz, E.r2_relaxed)) {
        visible = true;   // checkVisibilityWithPointCloudRelaxed (:745-747)
    } else if (!E.terrain_present) {
        visible = true;   // (:721, :727, :750)
    } else {
#if defined(PCP_CELL_EXP) && PCP_CELL_EXP == 1   // A/B timing only: no march
        visible = end > 1e300;
#elif defined(PCP_CELL_EXP) && PCP_CELL_EXP == 2  // A/B timing only: probes, a candidate = hit
        visible = march<false, true, PCP_CELL_PROBES>(E.terrain, px, py, pz, ndx, ndy, ndz,
                                                      steps, E.K, end, 1e30f, 1e15f) < 0;
#else
        const int lane = threadIdx.x & 63;
        const bool clear = march<STATS, true, PCP_CELL_PROBES, 2>(
                               E.terrain, px, py, pz, ndx, ndy, ndz, steps, E.K, end, E.r2_ray,
                               E.rexit_ray, cnt, G > 1 ? lane % G : 0, G) < 0;
        if (G > 1) {   // the group's lanes all reach here (same inputs, same branches)
            const uint64_t blocked = __ballot(!clear);
            visible = ((blocked >> (lane & ~(G - 1))) & ((1ull << G) - 1)) == 0;
        } else {
            visible = clear;
        }
#endif
    }
    if (!visible) return 0.0;
    bits |= 4u;
    const double dot = ndx * (double)nx + ndy * (double)ny + ndz * (double)nz;
    const double ad = fmax(0.0, fmin(1.0, fabs(dot)));
    return score_finish(score_sin_part(ad), L, cell);
}

// one thread per (cell c, row r): rows r < P are the candidate poses (evaluatePosition's
// score_mobile, written [p][c], coalesced), row P is the pose-invariant zx120 evaluation
// (score_zx120 and its result bits) -- one launch, so the zx120 row does not run alone on a
// handful of CUs.  std::max(score_zx120, score_mobile) is applied by k_row_sum.
#ifndef PCP_SCORE_WAVES
#define PCP_SCORE_WAVES 6   // waves per SIMD of k_score_cells (build knob)
#endif
// SL: the step table in LDS (K <= kStepLds, checked by the launcher).  (Several rows per
// thread, the cell loaded once, spilled ~120 dwords: the loop hoists both GridViews' kernel
// arguments into registers.)
template <bool SL>
__global__ void __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(PCP_SCORE_WAVES, 8)))
k_score_cells(VisEnv E, const double *__restrict__ cxyz, const float *__restrict__ cn, int C,
              const double *__restrict__ poses5, int P, const double *__restrict__ zx5,
              double *__restrict__ sm_out, uint8_t *__restrict__ mbits,
              double *__restrict__ score_z, uint8_t *__restrict__ zbits,
              int32_t *__restrict__ stats, const uint32_t *__restrict__ P_dev,
              const uint32_t *__restrict__ C_dev) {
    const int c = blockIdx.x * kT + threadIdx.x;
    // the colour-statistics slots k_cell_flags accumulates into (it runs after this kernel)
    if (stats && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) stats[threadIdx.x] = 0;
    __shared__ double s_steps[SL ? kStepLds : 1];
    if (SL) {
        for (int q = threadIdx.x; q < E.K; q += kT) s_steps[q] = E.steps[q];
        __syncthreads();
    }
    const double *steps = SL ? s_steps : E.steps;
    // C_dev: the cells' count is the device's (a setup still in flight, C = its capacity and the
    // rows' stride)
    if (c >= (C_dev ? (int)*C_dev : C)) return;
    const int p = blockIdx.y;
    const bool zrow = p == P;   // the last row (P = the rows' capacity with P_dev)
    // P_dev: the pose count is the device's (candidates generated in the same stream)
    if (P_dev && !zrow && p >= (int)*P_dev) return;
    const double *Q = zrow ? zx5 : poses5 + 5 * (size_t)p;
    uint32_t bits;
    const double s = eval_cell(E, Q[0], Q[1], Q[2], Q[3], cxyz[3 * c], cxyz[3 * c + 1],
                               cxyz[3 * c + 2], cn[3 * c], cn[3 * c + 1], cn[3 * c + 2], zrow, bits,
                               steps, nullptr, c);
    if (zrow) {
        score_z[c] = s;
        zbits[c] = (uint8_t)bits;
    } else {
        sm_out[(size_t)p * C + c] = s;
        mbits[(size_t)p * C + c] = (uint8_t)bits;
    }
}

// Diagnostic twin of k_score_cells (pcp_score_poses_stats; never timed): the same rows and the
// same march, counting per launch the gather lane-loads its visibility rays issue -- z-band
// probes (2-byte thresholds), candidates' walk starts (4 bytes), point records (12 bytes) --
// into stats[0..2] (u64, one atomic per wave and counter).  No scores are written.
template <bool SL>
__global__ void __launch_bounds__(kT)
k_score_cells_stats(VisEnv E, const double *__restrict__ cxyz, const float *__restrict__ cn,
                    int C, const double *__restrict__ poses5, int P,
                    const double *__restrict__ zx5, unsigned long long *__restrict__ stats) {
    const int c = blockIdx.x * kT + threadIdx.x;
    __shared__ double s_steps[SL ? kStepLds : 1];
    if (SL) {
        for (int q = threadIdx.x; q < E.K; q += kT) s_steps[q] = E.steps[q];
        __syncthreads();
    }
    const double *steps = SL ? s_steps : E.steps;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};
    if (c < C) {
        const int p = blockIdx.y;
        const double *Q = p == P ? zx5 : poses5 + 5 * (size_t)p;
        uint32_t bits;
        (void)eval_cell<1, true>(E, Q[0], Q[1], Q[2], Q[3], cxyz[3 * c], cxyz[3 * c + 1],
                                 cxyz[3 * c + 2], cn[3 * c], cn[3 * c + 1], cn[3 * c + 2], p == P,
                                 bits, steps, cnt, c);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        unsigned long long v = cnt[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[i], v);
    }
}

// The same rows with G lanes per (cell, row): for launches with few rays (one candidate pose,
// C1 / C5), where one lane per ray leaves the GPU nearly empty and each ray's march is a long
// chain of dependent probes.  The G lanes split the ray's samples (march koff / kstr) and AND
// their verdicts; lane 0 of the group writes.
template <bool SL, int G>
__global__ void __launch_bounds__(kT)
k_score_cells_wide(VisEnv E, const double *__restrict__ cxyz, const float *__restrict__ cn,
                   int C, const double *__restrict__ poses5, int P,
                   const double *__restrict__ zx5, double *__restrict__ sm_out,
                   uint8_t *__restrict__ mbits, double *__restrict__ score_z,
                   uint8_t *__restrict__ zbits, int32_t *__restrict__ stats,
                   const uint32_t *__restrict__ P_dev, const uint32_t *__restrict__ C_dev) {
    static_assert(G > 1 && G <= 64 && (G & (G - 1)) == 0, "lane groups within a wave");
    const int c = (int)((blockIdx.x * kT + threadIdx.x) / G);
    if (stats && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) stats[threadIdx.x] = 0;
    __shared__ double s_steps[SL ? kStepLds : 1];
    if (SL) {
        for (int q = threadIdx.x; q < E.K; q += kT) s_steps[q] = E.steps[q];
        __syncthreads();
    }
    const double *steps = SL ? s_steps : E.steps;
    if (c >= (C_dev ? (int)*C_dev : C)) return;   // (whole groups: C * G threads, groups aligned)
    const int p = blockIdx.y;
    const bool zrow = p == P;
    if (P_dev && !zrow && p >= (int)*P_dev) return;
    const double *Q = zrow ? zx5 : poses5 + 5 * (size_t)p;
    uint32_t bits;
    const double s = eval_cell<G>(E, Q[0], Q[1], Q[2], Q[3], cxyz[3 * c], cxyz[3 * c + 1],
                                  cxyz[3 * c + 2], cn[3 * c], cn[3 * c + 1], cn[3 * c + 2], zrow,
                                  bits, steps, nullptr, c);
    if ((threadIdx.x & (G - 1)) != 0) return;
    if (zrow) {
        score_z[c] = s;
        zbits[c] = (uint8_t)bits;
    } else {
        sm_out[(size_t)p * C + c] = s;
        mbits[(size_t)p * C + c] = (uint8_t)bits;
    }
}
constexpr int kWideG = 16;               // lanes per ray of k_score_cells_wide
constexpr int kWideMaxRays = 1 << 15;    // (rows x cells) up to which the wide kernel runs

// ordered sequential sum per row (evaluatePosition :634-645): total_score += s for s > 0 in cell
// order, s = std::max(score_zx120, score_mobile) = (sz < sm) ? sm : sz for a pose row, sz for
// the zx120 row (r == P).  One wave per row: each lane holds 8 of the next 512 values in
// registers (the following 512 already loading), and the wave walks them in cell order with
// v_readlane into scalar registers, every lane carrying the same running sum -- no LDS round
// trip in the chain, which is the dependent adds alone.
constexpr int kSumChunk = 512;
__device__ __forceinline__ double readlane_f64(double x, int l) {
    const uint64_t b = __double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ void row_sum_body(const double *__restrict__ sm,
                                             const double *__restrict__ score_z, int C, int P,
                                             double *__restrict__ total,
                                             int32_t *__restrict__ covered, int r) {
    const int lane = threadIdx.x & 63;
    const double *row = sm + (size_t)r * C;
    constexpr int kPer = kSumChunk / 64;
    double v[kPer], wz[kPer], wm[kPer];
    int32_t cov = 0;   // order-free: each lane counts its own positive values
    // raw loads only: the values they feed are formed after the chain that overlaps them
    auto load = [&](int base) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int c = base + q * 64 + lane;
            wz[q] = c < C ? score_z[c] : 0.0;
            wm[q] = (c < C && r < P) ? row[c] : 0.0;
        }
    };
    // x > 0 ? x : +0.0 -- adding +0.0 to the (non-negative) running sum leaves it bit-identical,
    // so the unconditional adds are the reference's `if (x > 0) total += x`
    auto form = [&]() {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const double sz = wz[q], m = wm[q];
            const double x = r < P ? ((sz < m) ? m : sz) : sz;
            const bool pos = x > 0;
            cov += pos ? 1 : 0;
            v[q] = pos ? x : 0.0;
        }
    };
    double acc = 0.0;
    load(0);
    form();
    for (int base = 0; base < C; base += kSumChunk) {
        const bool more = base + kSumChunk < C;
        if (more) load(base + kSumChunk);   // in flight during the chain
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            if (base + q * 64 >= C) break;   // wave-uniform; the tail's zero lanes add +0.0
#pragma unroll
            for (int l = 0; l < 64; l += 8) {   // 8 readlanes ahead of their adds
                double t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t[i] = readlane_f64(v[q], l + i);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc += t[i];
            }
        }
        if (more) form();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cov += __shfl_xor(cov, o, 64);
    if (lane == 0) {
        total[r] = acc;
        covered[r] = cov;
    }
}

// The same sums, one ROW PER LANE: a block of kT threads owns kSumRows rows.  Waves 1..3 load
// chunks of kSumCh cells of those rows (coalesced, one row per pass, kSumLpt cells per thread),
// form the values (the max with score_z, x > 0 ? x : +0.0, the covered counts) and stage them
// in LDS [row][cell]; lane r of wave 0 then walks row r of the chunk in cell order -- its
// chain is the dependent v_add_f64s alone (~6 clocks each on gfx950, tools/mb/chain.hip), the
// LDS reads of the next two groups of 32 values in flight under the adds of the current group,
// with no readlane traffic in front of each add (the one-wave-per-row chain above: 2 readlanes
// per add, ~19 clocks).  Three LDS buffers: the loaders fill chunk k + 2 while the chain walks
// chunk k, one barrier per chunk; their global loads run two chunks further ahead.
// k_sum_flags at 256 poses x 3,704 cells (tools/ab_libs.sh): 29.6 us one wave per row; lane
// per row with 16 / 8 / 4 / 2 rows per block 33 / 27 / 25.5 / 25.5 us (a block's loads are
// latency x concurrency bound on its CU, so few rows per block), the ring walk 20.5 us.
#ifndef PCP_SUM_ROWS
#define PCP_SUM_ROWS 4   // rows per block: few, so the loads of the rows spread over many CUs
#endif
#ifndef PCP_SUM_LPT
#define PCP_SUM_LPT 2    // cells per loader thread per chunk (chunk = 192 x this)
#endif
#ifndef PCP_SUM_BATCH
#define PCP_SUM_BATCH 16 // ds_read_b128 per group of the walk
#endif
constexpr int kSumRows = PCP_SUM_ROWS, kSumLpt = PCP_SUM_LPT, kSumCh = (kT - 64) * kSumLpt;
constexpr int kSumLd = kSumCh + 2;   // +2: b128 reads of lanes r, r + 1 four banks apart
// C: the rows' stride; Ca: the cells summed (C, or the device's count of a setup in flight)
__device__ __forceinline__ void row_group_body(const double *__restrict__ sm,
                                               const double *__restrict__ score_z, int C, int Ca,
                                               int P, double *__restrict__ total,
                                               int32_t *__restrict__ covered, int g) {
    __shared__ double s_v[3][kSumRows][kSumLd];
    __shared__ int32_t s_cov[kSumRows];
    const int tid = threadIdx.x, r0 = g * kSumRows;
    if (Ca <= 0) {   // no cells (uniform): every total is the +0.0 it starts from
        if (tid < kSumRows && r0 + tid <= P) {
            total[r0 + tid] = 0.0;
            covered[r0 + tid] = 0;
        }
        return;
    }
    const int nch = (Ca + kSumCh - 1) / kSumCh;
    if (tid < kSumRows) s_cov[tid] = 0;
    const int lt = tid - 64;   // loader thread (waves 1..3): cells lt + (kT - 64) i of a chunk
    int32_t cov[kSumRows];
#pragma unroll
    for (int q = 0; q < kSumRows; ++q) cov[q] = 0;
    // raw loads into registers, unconditional (row and cell clamped into the buffer; the
    // formation masks them), in two register sets for chunks of even / odd index: the loads
    // of chunk k + 4 go out while chunk k + 2 is formed, two chain chunks ahead of their use
    double mA[kSumLpt][kSumRows], szA[kSumLpt], mB[kSumLpt][kSumRows], szB[kSumLpt];
    auto load = [&](int k, double (&m)[kSumLpt][kSumRows], double (&sz)[kSumLpt]) {
#pragma unroll
        for (int i = 0; i < kSumLpt; ++i) {
            const int c = min(k * kSumCh + lt + (kT - 64) * i, Ca - 1);
            sz[i] = score_z[c];
#pragma unroll
            for (int q = 0; q < kSumRows; ++q)
                m[i][q] = sm[(size_t)max(min(r0 + q, P - 1), 0) * C + c];
        }
    };
    auto form = [&](int k, const double (&m)[kSumLpt][kSumRows], const double (&sz)[kSumLpt]) {
        double(*dst)[kSumLd] = s_v[k % 3];
#pragma unroll
        for (int i = 0; i < kSumLpt; ++i) {
            const int cl = lt + (kT - 64) * i;
            const bool in = k * kSumCh + cl < Ca;
#pragma unroll
            for (int q = 0; q < kSumRows; ++q) {
                const double x = r0 + q < P ? ((sz[i] < m[i][q]) ? m[i][q] : sz[i]) : sz[i];
                const bool pos = in && x > 0;   // (cells past C add +0.0)
                cov[q] += pos ? 1 : 0;
                dst[q][cl] = pos ? x : 0.0;
            }
        }
    };
    double acc = 0.0;
    auto walk = [&](int k) {
        // software-pipelined walk over a ring of three groups of kG b128 reads: the adds of
        // group i run while groups i + 1 and i + 2 are in flight.  lgkmcnt counts at most 15
        // outstanding LDS operations, so a wait for group i also waits for the head of group
        // i + 1 -- issued a whole group of adds earlier, so already in -- but never for group
        // i + 2, issued just before.  The scheduling barriers keep each group's reads ahead of
        // the adds before it (the scheduler otherwise sinks them next to their use, exposing
        // the LDS latency).  tools/ab_libs.sh: two batches of 4 / 6 / 16 reads 24.1 / 23.2 /
        // 21.0 us per k_sum_flags, the ring of 8 / 16 21.1 / 20.5 us.
        const double2 *v = reinterpret_cast<const double2 *>(s_v[k % 3][tid]);
        constexpr int kG = PCP_SUM_BATCH, kN = kSumCh / 2;
        static_assert(kN % (3 * kG) == 0, "whole group triples per chunk");
        double2 g0[kG], g1[kG], g2[kG];
        auto rd = [&](double2 *g, int j) {
#pragma unroll
            for (int i = 0; i < kG; ++i) g[i] = v[j + i];
        };
        auto add = [&](const double2 *g) {
#pragma unroll
            for (int i = 0; i < kG; ++i) {
                acc += g[i].x;
                acc += g[i].y;
            }
        };
        rd(g0, 0);
        rd(g1, kG);
#pragma unroll
        for (int j = 0; j < kN; j += 3 * kG) {
            if (j + 2 * kG < kN) rd(g2, j + 2 * kG);
            __builtin_amdgcn_sched_barrier(0);
            add(g0);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 3 * kG < kN) rd(g0, j + 3 * kG);
            __builtin_amdgcn_sched_barrier(0);
            add(g1);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 4 * kG < kN) rd(g1, j + 4 * kG);
            __builtin_amdgcn_sched_barrier(0);
            add(g2);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // one chunk: the loaders form chunk k + 2 (and load k + 4) while the chain walks chunk k
    auto step = [&](int k, double (&m)[kSumLpt][kSumRows], double (&sz)[kSumLpt]) {
        if (tid >= 64) {
            if (k + 2 < nch) {
                form(k + 2, m, sz);
                if (k + 4 < nch) load(k + 4, m, sz);
            }
        } else if (tid < kSumRows) {
            walk(k);
        }
        __syncthreads();
    };
    if (tid >= 64) {
        load(0, mA, szA);
        if (nch > 1) load(1, mB, szB);
        form(0, mA, szA);
        if (nch > 2) load(2, mA, szA);
        if (nch > 1) form(1, mB, szB);
        if (nch > 3) load(3, mB, szB);
    }
    __syncthreads();
    for (int k = 0; k < nch; k += 2) {
        step(k, mA, szA);
        if (k + 1 < nch) step(k + 1, mB, szB);
    }
    if (tid >= 64) {
#pragma unroll
        for (int q = 0; q < kSumRows; ++q) {
            int32_t x = cov[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
            if ((tid & 63) == 0) atomicAdd(&s_cov[q], x);
        }
    }
    __syncthreads();
    if (tid < kSumRows && r0 + tid <= P) {
        total[r0 + tid] = acc;
        covered[r0 + tid] = s_cov[tid];
    }
}
__host__ __device__ constexpr int sum_groups(int P) { return (P + 1 + kSumRows - 1) / kSumRows; }

#ifndef PCP_ROW_SUM_LANES
#define PCP_ROW_SUM_LANES 1   // 0: the readlane chain (one wave per row) above
#endif

__global__ void __launch_bounds__(64)
k_row_sum(const double *__restrict__ sm, const double *__restrict__ score_z, int C, int P,
          double *__restrict__ total, int32_t *__restrict__ covered) {
    row_sum_body(sm, score_z, C, P, total, covered, blockIdx.x);
}
__global__ void __launch_bounds__(kT)
k_row_sum_lanes(const double *__restrict__ sm, const double *__restrict__ score_z, int C, int P,
                double *__restrict__ total, int32_t *__restrict__ covered) {
    row_group_body(sm, score_z, C, C, P, total, covered, blockIdx.x);
}

// stats slots
enum {
    S_TOTAL = 0, S_ZR, S_ZF, S_ZV, S_ZG, S_ZRED, S_ZB, S_ZY, S_G, S_RED, S_B, S_Y, S_N
};

// stale-flag resolution (virtual_lidar.cpp:487-501 read flags written by the LAST
// evaluation that reached each assignment, :662-687) + colour statistics
// stats_host (nullable): the last of the nblk flag blocks to finish copies the finished
// statistics there (ticket in stats[63], zeroed with the rest by k_score_cells)
__device__ __forceinline__ void cell_flags_body(const uint8_t *__restrict__ zbits,
                                                const uint8_t *__restrict__ mbits, int C, int Ca,
                                                int P, uint8_t *__restrict__ flags,
                                                int32_t *__restrict__ stats, int blk,
                                                int32_t *__restrict__ stats_host = nullptr,
                                                int nblk = 0) {
    const int c = blk * kT + threadIdx.x;
    __shared__ int32_t bst[S_N];
    if (threadIdx.x < S_N) bst[threadIdx.x] = 0;
    __syncthreads();
    if (c < Ca) {   // (C: mbits' row stride)
        uint32_t f = flags[c];
        const uint32_t z = zbits[c];
        f = (z & 1u) ? (f | PCP_F_RANGE_Z) : (f & ~PCP_F_RANGE_Z);
        if (z & 1u) f = (z & 2u) ? (f | PCP_F_FOV_Z) : (f & ~PCP_F_FOV_Z);
        if ((z & 3u) == 3u) f = (z & 4u) ? (f | PCP_F_VIS_Z) : (f & ~PCP_F_VIS_Z);
        // evaluateZX120Only statistics use the zx120 flags right after its evaluation (:377-397)
        const bool zr = f & PCP_F_RANGE_Z, zf = f & PCP_F_FOV_Z, zv = f & PCP_F_VIS_Z;
        if (P > 0) {
            // the last pose that reached each assignment, newest first, 16 poses per round of
            // independent loads (coalesced over the cells of the block)
            const uint32_t lastb = mbits[(size_t)(P - 1) * C + c];
            f = (lastb & 1u) ? (f | PCP_F_RANGE_M) : (f & ~PCP_F_RANGE_M);
            int fov_from = -1, vis_from = -1;   // pose whose bits set the flag
            for (int p0 = P - 1; p0 >= 0 && (fov_from < 0 || vis_from < 0); p0 -= 16) {
                uint32_t b[16];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    b[q] = (p0 - q >= 0) ? mbits[(size_t)(p0 - q) * C + c] : 0u;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (fov_from < 0 && (b[q] & 1u)) fov_from = p0 - q, f = (b[q] & 2u) ? (f | PCP_F_FOV_M) : (f & ~PCP_F_FOV_M);
                    if (vis_from < 0 && (b[q] & 3u) == 3u) vis_from = p0 - q, f = (b[q] & 4u) ? (f | PCP_F_VIS_M) : (f & ~PCP_F_VIS_M);
                }
                if (p0 - 15 <= 0) break;
            }
        }
        flags[c] = (uint8_t)f;
        atomicAdd(&bst[S_TOTAL], 1);
        if (zr) atomicAdd(&bst[S_ZR], 1);
        if (zf) atomicAdd(&bst[S_ZF], 1);
        if (zv) atomicAdd(&bst[S_ZV], 1);
        if (!zr) atomicAdd(&bst[S_ZB], 1);
        else if (!zf) atomicAdd(&bst[S_ZY], 1);
        else if (!zv) atomicAdd(&bst[S_ZRED], 1);
        else atomicAdd(&bst[S_ZG], 1);
        const bool mr = f & PCP_F_RANGE_M, mf = f & PCP_F_FOV_M, mv = f & PCP_F_VIS_M;
        const bool zr2 = f & PCP_F_RANGE_Z, zf2 = f & PCP_F_FOV_Z, zv2 = f & PCP_F_VIS_Z;
        if (!zr2 && !mr) atomicAdd(&bst[S_B], 1);
        else if (!zf2 && !mf) atomicAdd(&bst[S_Y], 1);
        else if (!zv2 && !mv) atomicAdd(&bst[S_RED], 1);
        else atomicAdd(&bst[S_G], 1);
    }
    __syncthreads();
    if (threadIdx.x < S_N && bst[threadIdx.x]) atomicAdd(&stats[threadIdx.x], bst[threadIdx.x]);
    if (!stats_host) return;
    __threadfence();   // this block's statistics adds before its ticket
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) last = atomicAdd(&stats[63], 1) == nblk - 1;
    __syncthreads();
    if (last && threadIdx.x < S_N) stats_host[threadIdx.x] = atomicAdd(&stats[threadIdx.x], 0);
}

__global__ void __launch_bounds__(kT)
k_cell_flags(const uint8_t *__restrict__ zbits, const uint8_t *__restrict__ mbits, int C, int P,
             uint8_t *__restrict__ flags, int32_t *__restrict__ stats) {
    cell_flags_body(zbits, mbits, C, C, P, flags, stats, blockIdx.x);
}

// the two independent tails of a score query in ONE launch: the first blocks are the ordered
// row sums (row_group_body, kSumRows rows per block; a 3,704-add chain per row, ~20 us), the
// blocks after them the stale-flag resolution (~7 us), which so runs beside the chains
// instead of after them
__global__ void __launch_bounds__(kT)
k_sum_flags(const double *__restrict__ sm, const double *__restrict__ score_z, int C, int P,
            double *__restrict__ total, int32_t *__restrict__ covered,
            const uint8_t *__restrict__ zbits, const uint8_t *__restrict__ mbits,
            uint8_t *__restrict__ flags, int32_t *__restrict__ stats,
            int32_t *__restrict__ stats_host, const uint32_t *__restrict__ P_dev,
            const uint32_t *__restrict__ C_dev) {
    // P: the rows the grid was sized for; Pa: the poses (the device's count with P_dev, the
    // row blocks past it idle); C: the rows' stride and the cells the grid was sized for, Ca
    // the cells (the device's count with C_dev)
    const int Pa = P_dev ? (int)*P_dev : P;
    const int Ca = C_dev ? (int)*C_dev : C;
#if PCP_ROW_SUM_LANES
    const int nr = sum_groups(P);
    if ((int)blockIdx.x < nr) {
        if ((int)blockIdx.x < sum_groups(Pa))
            row_group_body(sm, score_z, C, Ca, Pa, total, covered, blockIdx.x);
        return;
    }
#else
    const int nr = P + 1;
    if ((int)blockIdx.x < nr) {
        if (threadIdx.x < 64 && (int)blockIdx.x <= Pa)
            row_sum_body(sm, score_z, C, Pa, total, covered, blockIdx.x);   // (C_dev: lanes path only)
        return;
    }
#endif
    cell_flags_body(zbits, mbits, C, Ca, Pa, flags, stats, (int)blockIdx.x - nr, stats_host,
                    (int)gridDim.x - nr);
}
__host__ __device__ constexpr int sum_flag_row_blocks(int P) {
    return PCP_ROW_SUM_LANES ? sum_groups(P) : P + 1;
}

// ---------------------------------------------------------------------------------------
// pose-sharded search across GPUs (pcp_multi.hip): per-rank key vectors, reduced by ONE
// collective, then finalized on one rank.  The fan's keys: pcp_fan.hip
// ---------------------------------------------------------------------------------------
// reference mode: v = [P totals | P covered | C range | C fov | C vis], all-reduce(MAX).
// Totals are >= +0.0 (sums of positive scores from +0.0), so their IEEE bits order like the
// values; 0 = +0.0 marks other ranks' poses.  A covered key carries kScoreWritten beside the
// count, so a pose no rank scored reduces to 0 and is reported, not read as a zero total (as the
// fan's UINT64_MAX key).  Per cell, the newest pose of this rank that
// reached each stale-flag assignment (:662-687) as ((global index + 1) << 1) | bit, 0 = none:
// the maximum over the ranks is the newest pose overall, which is what k_cell_flags resolves.
__global__ void __launch_bounds__(kT)
k_score_keys(const double *__restrict__ tot, const int32_t *__restrict__ cov,
             const uint8_t *__restrict__ mbits, int C, int Pl, int lo, int P,
             unsigned long long *__restrict__ v) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < P) {
        const bool mine = i >= lo && i - lo < Pl;
        v[i] = mine ? (unsigned long long)__double_as_longlong(tot[i - lo]) : 0ull;
        v[P + i] = mine ? (kScoreWritten | (unsigned long long)(uint32_t)cov[i - lo]) : 0ull;
    }
    if (i < C) {
        unsigned long long kr = 0, kf = 0, kv = 0;
        if (Pl > 0) {
            const uint32_t lb = mbits[(size_t)(Pl - 1) * C + i];
            kr = ((unsigned long long)(lo + Pl) << 1) | (lb & 1u);
            for (int q = Pl - 1; q >= 0 && (!kf || !kv); --q) {
                const uint32_t b = mbits[(size_t)q * C + i];
                const unsigned long long g1 = (unsigned long long)(lo + q + 1) << 1;
                if (!kf && (b & 1u)) kf = g1 | ((b >> 1) & 1u);
                if (!kv && (b & 3u) == 3u) kv = g1 | ((b >> 2) & 1u);
            }
        }
        v[2 * (size_t)P + i] = kr;
        v[2 * (size_t)P + C + i] = kf;
        v[2 * (size_t)P + 2 * (size_t)C + i] = kv;
    }
}

// colour statistics of one cell's final flags (evaluateZX120Only :377-397 and :487-501)
__device__ __forceinline__ void count_flags(uint32_t f, int32_t *bst) {
    const bool zr = f & PCP_F_RANGE_Z, zf = f & PCP_F_FOV_Z, zv = f & PCP_F_VIS_Z;
    atomicAdd(&bst[S_TOTAL], 1);
    if (zr) atomicAdd(&bst[S_ZR], 1);
    if (zf) atomicAdd(&bst[S_ZF], 1);
    if (zv) atomicAdd(&bst[S_ZV], 1);
    if (!zr) atomicAdd(&bst[S_ZB], 1);
    else if (!zf) atomicAdd(&bst[S_ZY], 1);
    else if (!zv) atomicAdd(&bst[S_ZRED], 1);
    else atomicAdd(&bst[S_ZG], 1);
    const bool mr = f & PCP_F_RANGE_M, mf = f & PCP_F_FOV_M, mv = f & PCP_F_VIS_M;
    if (!zr && !mr) atomicAdd(&bst[S_B], 1);
    else if (!zf && !mf) atomicAdd(&bst[S_Y], 1);
    else if (!zv && !mv) atomicAdd(&bst[S_RED], 1);
    else atomicAdd(&bst[S_G], 1);
}

// the reduced keys -> cell flags + colour statistics (the k_cell_flags result)
__global__ void __launch_bounds__(kT)
k_flags_from_keys(const unsigned long long *__restrict__ v, const uint8_t *__restrict__ zbits,
                  int C, int P, uint8_t *__restrict__ flags, int32_t *__restrict__ stats) {
    const int c = blockIdx.x * kT + threadIdx.x;
    __shared__ int32_t bst[S_N];
    if (threadIdx.x < S_N) bst[threadIdx.x] = 0;
    __syncthreads();
    if (c < C) {
        uint32_t f = flags[c];
        const uint32_t z = zbits[c];
        f = (z & 1u) ? (f | PCP_F_RANGE_Z) : (f & ~PCP_F_RANGE_Z);
        if (z & 1u) f = (z & 2u) ? (f | PCP_F_FOV_Z) : (f & ~PCP_F_FOV_Z);
        if ((z & 3u) == 3u) f = (z & 4u) ? (f | PCP_F_VIS_Z) : (f & ~PCP_F_VIS_Z);
        const unsigned long long kr = v[2 * (size_t)P + c], kf = v[2 * (size_t)P + C + c],
                                 kv = v[2 * (size_t)P + 2 * (size_t)C + c];
        if (kr) f = (kr & 1ull) ? (f | PCP_F_RANGE_M) : (f & ~PCP_F_RANGE_M);
        if (kf) f = (kf & 1ull) ? (f | PCP_F_FOV_M) : (f & ~PCP_F_FOV_M);
        if (kv) f = (kv & 1ull) ? (f | PCP_F_VIS_M) : (f & ~PCP_F_VIS_M);
        flags[c] = (uint8_t)f;
        count_flags(f, bst);
    }
    __syncthreads();
    if (threadIdx.x < S_N && bst[threadIdx.x]) atomicAdd(&stats[threadIdx.x], bst[threadIdx.x]);
}

// element-wise min / max of two key vectors (ranks sharing one device, no RCCL)
__global__ void __launch_bounds__(kT)
k_keys_combine(unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b,
               size_t n, int is_max) {
    const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    a[i] = is_max ? (a[i] > b[i] ? a[i] : b[i]) : (a[i] < b[i] ? a[i] : b[i]);
}

void launch_score_keys(hipStream_t st, const ScoreEnq &o, int lo, int P,
                       unsigned long long *v) {
    const int n = std::max(P, o.C);
    hipLaunchKernelGGL(k_score_keys, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, st,
                       (const double *)o.tot_d, (const int32_t *)o.cov_d,
                       (const uint8_t *)o.mbits, o.C, o.P, lo, P, v);
}
void launch_flags_from_keys(hipStream_t st, const unsigned long long *v, const uint8_t *zbits,
                            int C, int P, uint8_t *flags, int32_t *stats) {
    if (C)
        hipLaunchKernelGGL(k_flags_from_keys, dim3((unsigned)((C + kT - 1) / kT)), dim3(kT), 0, st,
                           v, zbits, C, P, flags, stats);
}
// the one-collective scoring's results into the caller's pinned block in one launch (instead of
// five D2H copies): [2P reduced keys | the zx120 total | the health word | C flags | 64 stats]
__global__ void __launch_bounds__(kT)
k_score_land(const unsigned long long *__restrict__ v, int P, size_t hw,
             const double *__restrict__ zx_total, const uint8_t *__restrict__ flags, int C,
             const int32_t *__restrict__ stats, unsigned char *__restrict__ pin, size_t fl_off,
             size_t st_off) {
    const size_t t = (size_t)blockIdx.x * kT + threadIdx.x, nt = (size_t)gridDim.x * kT;
    unsigned long long *ph = reinterpret_cast<unsigned long long *>(pin);
    for (size_t i = t; i < 2 * (size_t)P; i += nt) ph[i] = v[i];
    if (t == 0) {
        ph[2 * (size_t)P] = (unsigned long long)__double_as_longlong(*zx_total);
        ph[2 * (size_t)P + 1] = v[hw];
    }
    for (size_t i = t; i < (size_t)C; i += nt) pin[fl_off + i] = flags[i];
    if (t < 64) reinterpret_cast<int32_t *>(pin + st_off)[t] = stats[t];
}
void launch_score_land(hipStream_t st, const unsigned long long *v, int P, size_t hw,
                       const double *zx_total, const uint8_t *flags, int C, const int32_t *stats,
                       void *pin, size_t fl_off, size_t st_off) {
    const size_t work = std::max<size_t>(std::max<size_t>(2 * (size_t)P, (size_t)C), 64);
    const unsigned g = (unsigned)std::min<size_t>((work + kT - 1) / kT, 64);
    hipLaunchKernelGGL(k_score_land, dim3(g), dim3(kT), 0, st, v, P, hw, zx_total, flags, C,
                       stats, static_cast<unsigned char *>(pin), fl_off, st_off);
}
void launch_keys_combine(hipStream_t st, unsigned long long *a, const unsigned long long *b,
                         size_t n, bool is_max) {
    if (n)
        hipLaunchKernelGGL(k_keys_combine, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, st,
                           a, b, n, is_max ? 1 : 0);
}

// ---------------------------------------------------------------------------------------
// candidates (generateCandidatePositions :550-598, getGroundHeight :600-625)
// ---------------------------------------------------------------------------------------
struct CandArgs {
    GridView g;
    int ground_enabled;    // terrain cloud non-empty (:601)
    int gs;
    double exminx, exminy, xs, ys;
    double gminx, gmaxx, gminy, gmaxy;
    double cx, cy, cz;
    double zxx, zxy;
    double sensor_height;
    double *lat;           // gs*gs x 6: valid, x, y, z, pitch, yaw
};

// 1,024 threads per lattice point: the ground query's rows of cells (~600 for a 0.12 m terrain
// grid) one per thread, so a block's latency is one row walk, not three
constexpr int kCandT = 1024;
__global__ void __launch_bounds__(kCandT) k_candidates(CandArgs a) {
    const int l = blockIdx.x;
    const int i = l / a.gs, j = l - i * a.gs;
    const double x = a.exminx + i * a.xs;
    const double y = a.exminy + j * a.ys;
    double *out = a.lat + 6 * (size_t)l;
    const double ddx = x - a.zxx, ddy = y - a.zxy;
    if (sqrt(ddx * ddx + ddy * ddy) < 0.5 ||
        (x >= a.gminx && x <= a.gmaxx && y >= a.gminy && y <= a.gmaxy)) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    // getGroundHeight: radiusSearch((float)x,(float)y,0; r=2) then 2-D distance < 1.0
    double mz = -DBL_MAX;
    if (a.ground_enabled && a.g.n_pts > 0) {
        const GridView &g = a.g;
        const float qx = (float)x, qy = (float)y, qz = 0.0f;
        const float r2 = (float)(2.0 * 2.0);
        const double m = kQueryMargin;
        auto rng = [&](double lo, double hi, double o, int n, int &i0, int &i1) {
            i0 = (int)fmax(floor((lo - o) * g.inv_c), 0.0);
            i1 = (int)fmin(floor((hi - o) * g.inv_c), (double)(n - 1));
        };
        int x0, x1, y0, y1, z0, z1;
        rng(x - 1.0 - m, x + 1.0 + m, g.ox, g.nx, x0, x1);
        rng(y - 1.0 - m, y + 1.0 + m, g.oy, g.ny, y0, y1);
        rng(-2.0 - m, 2.0 + m, g.oz, g.nz, z0, z1);
        if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
            const int ny_r = y1 - y0 + 1, rows = ny_r * (z1 - z0 + 1);
            for (int r = threadIdx.x; r < rows; r += kCandT) {
                const int iy = y0 + r % ny_r, iz = z0 + r / ny_r;
                const size_t row = (size_t)g.nx * ((size_t)iy + (size_t)g.ny * iz);
                const uint32_t s = g.start[row + x0], e = g.start[row + x1 + 1];
                // four independent loads per step: a row's walk is a chain of load latencies,
                // and the maximum does not depend on the order the points come in
                for (uint32_t k0 = s; k0 < e; k0 += 4) {
                    float4 p4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) p4[u] = g.pts[min(k0 + (uint32_t)u, e - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float4 p = p4[u];
                        if (k0 + (uint32_t)u >= e || !flann_within(qx, qy, qz, p, r2)) continue;
                        const double dx = (double)p.x - x, dy = (double)p.y - y;
                        if (sqrt(dx * dx + dy * dy) < 1.0) mz = fmax(mz, (double)p.z);
                    }
                }
            }
        }
    }
    // block max
    __shared__ double red[kCandT / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mz = fmax(mz, __shfl_xor(mz, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mz;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kCandT / 64; ++w) mz = fmax(mz, red[w]);
    const double ground = (mz != -DBL_MAX) ? mz : 0.0;
    const double z = ground + a.sensor_height;
    const double dx = a.cx - x, dy = a.cy - y, dz = a.cz - z;
    const double hd = sqrt(dx * dx + dy * dy);
    if (hd < 0.1) {
        out[0] = 0.0;
        return;
    }
    // glibc's atan2 (the reference's) rounds correctly but for rare near-ties; ocml's is up to
    // 1.45 ulps off: pcp_cr_atan2_fix rounds it correctly (pcp_crmath.h, tests/test_crmath.py,
    // tests/test_device_math_gpu.py)
    const double elev = pcp_cr_atan2_fix(-dz, hd, atan2(-dz, hd));
    if (elev >= kMinElevation && elev <= kMaxElevation) {
        out[0] = 1.0;
        out[1] = x;
        out[2] = y;
        out[3] = z;
        out[4] = -kPi / 2 + elev;
        out[5] = pcp_cr_atan2_fix(dy, dx, atan2(dy, dx));
    } else {
        out[0] = 0.0;
    }
}

// order-preserving compaction of the lattice (single block)
__global__ void __launch_bounds__(1024)
k_cand_compact(const double *__restrict__ lat, int L, double *__restrict__ out, uint32_t *n_out,
               double *__restrict__ out_h = nullptr, uint32_t *__restrict__ n_h = nullptr) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t base_s;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int chunk = 0; chunk < L; chunk += 1024) {
        const int l = chunk + threadIdx.x;
        const bool v = l < L && lat[6 * (size_t)l] != 0.0;
        const uint64_t bal = __ballot(v);
        const uint32_t pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        uint32_t off = base_s;
        uint32_t tot = 0;
        for (int k = 0; k < 16; ++k) {
            if (k < w) off += wsum[k];
            tot += wsum[k];
        }
        if (v) {
            const uint32_t d = off + pre;
            for (int q = 0; q < 5; ++q) {
                const double x = lat[6 * (size_t)l + 1 + q];
                out[5 * (size_t)d + q] = x;
                if (out_h) out_h[5 * (size_t)d + q] = x;   // the host's copy (pinned)
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *n_out = base_s;
        if (n_h) *n_h = base_s;
    }
}

static VisEnv make_env(pcp_ctx *ctx, const pcp_vl_params *p, const double *steps_d, int K) {
    VisEnv E{};
    E.terrain_present = ctx->terrain.present ? 1 : 0;
    if (E.terrain_present) E.terrain = ctx->terrain.view(ctx->knob);
    E.aux_present = (ctx->aux.present && ctx->aux_cloud_n > 0) ? 1 : 0;
    if (E.aux_present) E.aux = ctx->aux.view();
    E.max_distance = p->max_distance;
    E.steps = steps_d;
    E.K = K;
    E.r2_ray = (float)(kRayRadius * kRayRadius);
    E.r2_relaxed = (float)(kRelaxedRadius * kRelaxedRadius);
    E.rexit_ray = exit_dist(E.r2_ray);
    return E;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int pcp_set_cells(pcp_ctx *ctx, const double *xyz, const float *normals, uint64_t n) {
    if (!ctx) return PCP_E_INVALID;
    if (n && (!xyz || !normals)) return set_err(ctx, PCP_E_INVALID, "pcp_set_cells: null input");
    if (n > (1u << 30)) return set_err(ctx, PCP_E_INVALID, "pcp_set_cells: too many cells");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = area_finish(ctx)) return rc;   // (a setup in flight writes the same buffers)
    PCP_HIP(ctx, ctx->cells_xyz.ensure(n * 3 * sizeof(double) + 16));
    PCP_HIP(ctx, ctx->cells_nrm.ensure(n * 3 * sizeof(float) + 16));
    if (n) {   // through the pinned ring: no wait on the stream, the caller may reuse its arrays
        if (int rc = upload_async(ctx, ctx->cells_xyz.p, xyz, n * 3 * sizeof(double), ctx->stream))
            return rc;
        if (int rc = upload_async(ctx, ctx->cells_nrm.p, normals, n * 3 * sizeof(float), ctx->stream))
            return rc;
    }
    ctx->n_cells = n;
    return PCP_OK;
}

}  // extern "C"

namespace pcp {
// generateCandidatePositions' kernel arguments (:357-415)
static CandArgs cand_args(pcp_ctx *ctx, const double bb[6], const pcp_vl_params *p,
                          const double zx[5], int gs) {
    CandArgs a{};
    a.ground_enabled = (ctx->terrain_cloud_n > 0 && ctx->terrain.present) ? 1 : 0;
    if (a.ground_enabled) a.g = ctx->terrain.view(ctx->knob);
    a.gs = gs;
    const double exminx = bb[0] - p->search_radius, exmaxx = bb[1] + p->search_radius;
    const double exminy = bb[2] - p->search_radius, exmaxy = bb[3] + p->search_radius;
    a.exminx = exminx;
    a.exminy = exminy;
    a.xs = (exmaxx - exminx) / (gs - 1);
    a.ys = (exmaxy - exminy) / (gs - 1);
    a.gminx = bb[0];
    a.gmaxx = bb[1];
    a.gminy = bb[2];
    a.gmaxy = bb[3];
    a.cx = (bb[0] + bb[1]) / 2.0;
    a.cy = (bb[2] + bb[3]) / 2.0;
    a.cz = (bb[4] + bb[5]) / 2.0;
    a.zxx = zx[0];
    a.zxy = zx[1];
    a.sensor_height = p->sensor_height;
    return a;
}

// the lattice a.lat of L points, then its valid poses and their count to out / n_d (and, when
// given, to the pinned out_h / n_h as well) in lattice order
static int cand_enqueue(pcp_ctx *ctx, const CandArgs &a, int L, double *out, uint32_t *n_d,
                        double *out_h = nullptr, uint32_t *n_h = nullptr) {
    ProfScope ps(ctx, PCP_K_CANDIDATES);
    hipLaunchKernelGGL(k_candidates, dim3((unsigned)L), dim3(kCandT), 0, ctx->stream, a);
    PCP_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_cand_compact, dim3(1), dim3(1024), 0, ctx->stream,
                       (const double *)a.lat, L, out, n_d, out_h, n_h);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

}  // namespace pcp

extern "C" {

int pcp_generate_candidates(pcp_ctx *ctx, const double bb[6], const pcp_vl_params *p,
                            const double zx[5], double *poses5, uint64_t cap, uint64_t *n_out) {
    if (!ctx) return PCP_E_INVALID;
    if (!bb || !p || !zx || !n_out || (cap && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_generate_candidates: null argument");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    const int gs = (int)std::ceil(std::sqrt((double)p->num_candidates));
    if (gs <= 0) return PCP_OK;
    if ((int64_t)gs * gs > (1 << 24))
        return set_err(ctx, PCP_E_INVALID, "pcp_generate_candidates: num_candidates too large");
    CandArgs a = cand_args(ctx, bb, p, zx, gs);
    const int L = gs * gs;
    PCP_HIP(ctx, ctx->out_a.ensure((size_t)L * 6 * sizeof(double)));
    a.lat = ctx->out_a.as<double>();
    // the poses and their count are adjacent: k_cand_compact stores them straight into pinned
    // memory (one synchronisation, no copy); huge lattices go through a device buffer, the
    // count first, then the poses
    const size_t span = (size_t)L * 5 * sizeof(double) + sizeof(uint32_t);
    const bool land = span <= (4u << 20);
    double *outp;
    if (land) {
        PCP_HIP(ctx, ctx->cand_host.ensure(span));
        outp = ctx->cand_host.as<double>();
    } else {
        PCP_HIP(ctx, ctx->out_b.ensure((size_t)L * 5 * sizeof(double) + 64));
        outp = ctx->out_b.as<double>();
    }
    uint32_t *n_d = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(outp) +
                                                 (size_t)L * 5 * sizeof(double));
    if (int rc = cand_enqueue(ctx, a, L, outp, n_d)) return rc;
    if (!land) {
        uint32_t nh = 0;
        if (int rc0 = read_small(ctx, &nh, n_d, 4, ctx->stream)) return rc0;
        *n_out = nh;
        prof_resolve(ctx);
        if (nh > cap)
            return set_err(ctx, PCP_E_CAPACITY, "pcp_generate_candidates: need %u poses, cap %llu",
                           nh, (unsigned long long)cap);
        if (nh)
            PCP_HIP(ctx, hipMemcpyAsync(poses5, outp, (size_t)nh * 5 * sizeof(double),
                                        hipMemcpyDeviceToHost, ctx->stream));
        PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return PCP_OK;
    }
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t nh = 0;
    std::memcpy(&nh, n_d, sizeof(nh));
    *n_out = nh;
    prof_resolve(ctx);
    if (nh > cap)
        return set_err(ctx, PCP_E_CAPACITY, "pcp_generate_candidates: need %u poses, cap %llu", nh,
                       (unsigned long long)cap);
    if (nh) std::memcpy(poses5, outp, (size_t)nh * 5 * sizeof(double));
    return PCP_OK;
}

}  // extern "C"

namespace pcp {
// the production k_score_cells launch of a query (one lane per ray, or kWideG lanes per ray for
// the few-ray queries of C1 / C5); score_enqueue and pcp_score_poses_burst
static void launch_score_cells(hipStream_t st, pcp_ctx *ctx, const VisEnv &E, int C, int P,
                               const double *poses_k, const double *zx_k, const ScoreEnq &o,
                               double *score_z, const uint32_t *P_dev, const uint32_t *C_dev) {
    const unsigned cb = (unsigned)((C + kT - 1) / kT);
    const dim3 g(cb, (unsigned)(P + 1));
    const uint64_t wide_rays = ctx->knob.score_wide_rays >= 0 ? (uint64_t)ctx->knob.score_wide_rays
                                                         : (uint64_t)kWideMaxRays;
    const bool wide = (uint64_t)(P + 1) * (uint64_t)C <= wide_rays && ctx->knob.score_wide;
    // the lanes per ray of the kernel that IS launched size its grid: PCP_SCORE_WIDE_G (2 / 4 /
    // 8 / 16, validated by pcp_create) with the step table in LDS, the default width past it
    // (the only instantiation there)
    const int Gq = ctx->knob.score_wide_g;
    const int G = (E.K <= kStepLds && (Gq == 2 || Gq == 4 || Gq == 8)) ? Gq : kWideG;
    const dim3 gw((unsigned)(((uint64_t)C * G + kT - 1) / kT), (unsigned)(P + 1));
    const double *cx = ctx->cells_xyz.as<const double>();
    const float *cn = ctx->cells_nrm.as<const float>();
    // k_score_cells_wide by [SL][G 2 / 4 / 8 / 16] (a step table past LDS: the default width
    // only), k_score_cells by [SL]
    using ScoreKernel = decltype(&k_score_cells<true>);
    static constexpr ScoreKernel kWide[2][4] = {
        {nullptr, nullptr, nullptr, k_score_cells_wide<false, kWideG>},
        {k_score_cells_wide<true, 2>, k_score_cells_wide<true, 4>, k_score_cells_wide<true, 8>,
         k_score_cells_wide<true, kWideG>}};
    static constexpr ScoreKernel kNarrow[2] = {k_score_cells<false>, k_score_cells<true>};
    const bool sl = E.K <= kStepLds;
    const ScoreKernel f = wide ? kWide[sl][__builtin_ctz((unsigned)G) - 1] : kNarrow[sl];
    hipLaunchKernelGGL(f, wide ? gw : g, dim3(kT), 0, st, E, cx, cn, C, poses_k, P, zx_k, o.comb,
                       o.mbits, score_z, o.zbits, o.stats, P_dev, C_dev);
}

// runOptimization's scoring up to the per-pose sums, enqueued on ctx->stream: poses + the
// zx120 pose uploaded through the pinned block, k_score_cells (rows 0..P-1 = poses, row P =
// zx120), k_row_sum.  On return the device holds comb/mbits [P][C], zbits [C], tot_d/cov_d
// [P+1] (row P = zx120); the caller synchronizes.  Validation is the caller's.
int score_enqueue(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                  const pcp_vl_params *p, ScoreEnq &o, const uint8_t *cell_flags,
                  bool fuse_tail, bool zc, const uint32_t *P_dev, const double *poses_dev) {
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // a setup in flight (pcp_set_excavation_area_async): its lattice capacity is the rows'
    // stride and the grids' size, the device's count the cells (only pcp_generate_and_score
    // queries it that way: every other caller settled it first)
    const bool pend = ctx->area_pending;
    area_join(ctx);   // (a setup's side stream: the cells, their normals and count)
    const int C = pend ? (int)ctx->cells_cap : (int)ctx->n_cells, P = (int)n;
    const uint32_t *C_dev = pend ? ctx->cells_n_d.as<const uint32_t>() : nullptr;
    o.C_dev = C_dev;
    int K = 0;
    int rc = ensure_steps(ctx, p->max_distance - kVisRadius, &K);
    if (rc) return rc;
    if ((rc = terrain_blocks_before_query(ctx))) return rc;
    VisEnv E = make_env(ctx, p, ctx->steps_d.as<const double>(), K);
    // buffers.  One device block mirrors the pinned one, so a query is ONE upload and ONE
    // download: [poses + zx120 (P + 1) x 5 f64 | cell flags C | totals f64 (P + 1) | covered
    // i32 (P + 1) | stats 64 i32] -- upload [poses .. flags], download [flags .. stats]
    const size_t pc = (size_t)P * (size_t)C;
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    o.fl_off = a16((size_t)(P + 1) * 5 * sizeof(double));
    const size_t to_off = a16(o.fl_off + (size_t)C);
    o.tc_bytes = (size_t)(P + 1) * (sizeof(double) + sizeof(int32_t));
    o.st_off = a16(to_off + o.tc_bytes);
    o.blk_bytes = o.st_off + 64 * sizeof(int32_t);
    PCP_HIP(ctx, ctx->poses_d.ensure(o.blk_bytes + 64));
    PCP_HIP(ctx, ctx->out_a.ensure(pc * sizeof(double) + (size_t)C * sizeof(double) + 64));
    PCP_HIP(ctx, ctx->out_b.ensure(pc + (size_t)C * 2 + 64));
    char *blk = ctx->poses_d.as<char>();
    o.P = P;
    o.C = C;
    o.comb = ctx->out_a.as<double>();
    double *score_z = o.comb + pc;
    o.mbits = ctx->out_b.as<uint8_t>();
    o.zbits = o.mbits + pc;
    o.flags_d = reinterpret_cast<uint8_t *>(blk + o.fl_off);
    o.tot_d = reinterpret_cast<double *>(blk + to_off);
    o.cov_d = reinterpret_cast<int32_t *>(o.tot_d + (P + 1));
    o.stats = reinterpret_cast<int32_t *>(blk + o.st_off);
    PCP_HIP(ctx, ctx->res_host.ensure(o.blk_bytes + 64));
    char *pin = ctx->res_host.as<char>();
    // the candidates, then the zx120 pose behind them (row P of k_score_cells), then the
    // caller's cell flags: one upload -- or none (zc: the kernels read the pinned block)
    if (P && poses5) std::memcpy(pin, poses5, (size_t)P * 5 * sizeof(double));
    o.P_dev = P_dev;
    std::memcpy(pin + (size_t)P * 5 * sizeof(double), zx, 5 * sizeof(double));
    size_t up = (size_t)(P + 1) * 5 * sizeof(double);
    if (pend && C) {   // fresh GridCells (:259): the setup's cells start with every flag clear
        std::memset(pin + o.fl_off, 0, C);
        up = o.fl_off + C;
    } else if (cell_flags && C) {
        std::memcpy(pin + o.fl_off, cell_flags, C);
        up = o.fl_off + C;
    }
    o.zc = zc && fuse_tail && C > 0;
    const char *pose_blk = blk;
    if (o.zc) {
        pose_blk = pin;
        o.flags_d = reinterpret_cast<uint8_t *>(pin + o.fl_off);
        o.tot_d = reinterpret_cast<double *>(pin + to_off);
        o.cov_d = reinterpret_cast<int32_t *>(o.tot_d + (P + 1));
        o.stats_host = reinterpret_cast<int32_t *>(pin + o.st_off);
    } else {
        PCP_HIP(ctx, hipMemcpyAsync(blk, pin, up, hipMemcpyHostToDevice, st));
    }
    const double *poses_k = reinterpret_cast<const double *>(pose_blk);
    const double *zx_k = poses_k + 5 * (size_t)P;
    if (poses_dev) poses_k = poses_dev;   // (the zx120 pose stays in the block)
    o.poses_k = poses_k;
    o.zx_k = zx_k;
    if (C) {
        {
            ProfScope ps(ctx, PCP_K_SCORE_CELLS);
            launch_score_cells(st, ctx, E, C, P, poses_k, zx_k, o, score_z, P_dev, C_dev);
            PCP_CHECK_LAUNCH(ctx);
        }
        o.score_z = score_z;
        if (!fuse_tail) {   // (fused: k_sum_flags, launched by the caller)
            ProfScope ps(ctx, PCP_K_POSE_SUM);
            if (PCP_ROW_SUM_LANES)
                hipLaunchKernelGGL(k_row_sum_lanes, dim3((unsigned)sum_groups(P)), dim3(kT), 0, st,
                                   (const double *)o.comb, (const double *)score_z, C, P, o.tot_d,
                                   o.cov_d);
            else
                hipLaunchKernelGGL(k_row_sum, dim3(P + 1), dim3(64), 0, st, (const double *)o.comb,
                                   (const double *)score_z, C, P, o.tot_d, o.cov_d);
            PCP_CHECK_LAUNCH(ctx);
        }
    } else {
        PCP_HIP(ctx, hipMemsetAsync(o.tot_d, 0, (size_t)(P + 1) * sizeof(double), st));
        PCP_HIP(ctx, hipMemsetAsync(o.cov_d, 0, (size_t)(P + 1) * sizeof(int32_t), st));
        PCP_HIP(ctx, hipMemsetAsync(o.stats, 0, 64 * sizeof(int32_t), st));
    }
    return PCP_OK;
}

void fill_report(const int32_t *st_h, double zx_total, int64_t best_idx, double best,
                 pcp_vl_report *rep) {
    std::memset(rep, 0, sizeof(*rep));
    rep->best_idx = best_idx;
    rep->best_score = best;
    rep->zx120_total_score = zx_total;
    rep->total_cells = st_h[S_TOTAL];
    rep->zx120_range_ok = st_h[S_ZR];
    rep->zx120_fov_ok = st_h[S_ZF];
    rep->zx120_visible_ok = st_h[S_ZV];
    rep->zx120_green = st_h[S_ZG];
    rep->zx120_red = st_h[S_ZRED];
    rep->zx120_blue = st_h[S_ZB];
    rep->zx120_yellow = st_h[S_ZY];
    rep->green = st_h[S_G];
    rep->red = st_h[S_RED];
    rep->blue = st_h[S_B];
    rep->yellow = st_h[S_Y];
}

// The tail of a query whose score_enqueue left the row sums to it (fuse_tail), in two steps: a
// setup in flight is settled between them (pcp_generate_and_score).
// 1. the ordered row sums and the stale-flag resolution side by side (k_sum_flags), then flags,
// totals, covered counts and statistics, one span of the block, in one download (zc: the kernels
// stored them in the pinned block), and the wait for the stream
static int score_tail_sync(pcp_ctx *ctx, const ScoreEnq &o) {
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P;
    if (C) {
        ProfScope ps(ctx, PCP_K_POSE_SUM);
        hipLaunchKernelGGL(k_sum_flags,
                           dim3((unsigned)(sum_flag_row_blocks(P) + (C + kT - 1) / kT)), dim3(kT),
                           0, st, (const double *)o.comb, (const double *)o.score_z, C, P, o.tot_d,
                           o.cov_d, (const uint8_t *)o.zbits, (const uint8_t *)o.mbits, o.flags_d,
                           o.stats, o.stats_host, o.P_dev, o.C_dev);
        PCP_CHECK_LAUNCH(ctx);
    }
    if (!o.zc)   // (no cells: the zeroed totals and statistics)
        PCP_HIP(ctx, hipMemcpyAsync(ctx->res_host.as<char>() + o.fl_off,
                                    reinterpret_cast<const char *>(o.flags_d),
                                    o.blk_bytes - o.fl_off, hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipStreamSynchronize(st));
    return PCP_OK;
}
// 2. the landed block into the caller's arrays and the report.  The totals were laid out for o.P
// rows; n of them are reported (the device's count: pcp_generate_and_score), the zx120 row
// behind them; Cn cells' flags are copied
static void score_tail_report(pcp_ctx *ctx, const ScoreEnq &o, uint32_t n, int Cn,
                              uint8_t *cell_flags, double *total_score, int32_t *covered,
                              pcp_vl_report *rep) {
    const char *pin = ctx->res_host.as<const char>();
    const double *tot_h = o.zc ? o.tot_d
                               : reinterpret_cast<const double *>(
                                     pin + (reinterpret_cast<const char *>(o.tot_d) -
                                            ctx->poses_d.as<const char>()));
    const int32_t *cov_h = reinterpret_cast<const int32_t *>(tot_h + (o.P + 1));
    const int32_t *st_h = reinterpret_cast<const int32_t *>(pin + o.st_off);
    if (Cn) std::memcpy(cell_flags, pin + o.fl_off, Cn);
    // runOptimization candidate loop (:464-475): strict '>' keeps the first maximum
    double best = -INFINITY;
    int64_t best_idx = -1;
    for (uint32_t k = 0; k < n; ++k) {
        if (total_score) total_score[k] = tot_h[k];
        if (covered) covered[k] = cov_h[k];
        if (tot_h[k] > best) {
            best = tot_h[k];
            best_idx = k;
        }
    }
    fill_report(st_h, tot_h[n], best_idx, best, rep);
}
}  // namespace pcp

extern "C" {

int pcp_score_poses(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                    const pcp_vl_params *p, uint8_t *cell_flags, double *total_score,
                    int32_t *covered, pcp_vl_report *rep) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;   // (the host's flags need the settled count)
    if (!zx || !p || !rep || (n && !poses5) || (ctx->n_cells && !cell_flags))
        return set_err(ctx, PCP_E_INVALID, "pcp_score_poses: null argument");
    if (n > 65535) return set_err(ctx, PCP_E_INVALID, "pcp_score_poses: at most 65535 poses per call");
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o, cell_flags, true, ctx->knob.zc_in))
        return rc;
    if (int rc = score_tail_sync(ctx, o)) return rc;
    prof_resolve(ctx);
    score_tail_report(ctx, o, (uint32_t)o.P, o.C, cell_flags, total_score, covered, rep);
    return PCP_OK;
}

// the roofline's inputs for the reference's own ray march (k_score_cells): the query's
// production launch set up by score_enqueue, then either its lane-loads counted by the STATS
// twin or the production launch `reps` times back-to-back between two events
static int score_diag(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                      const pcp_vl_params *p, uint64_t *stats, int reps, double *ms) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_score_poses_stats/burst: null argument");
    if (n > 65535) return set_err(ctx, PCP_E_INVALID, "pcp_score_poses_stats/burst: too many poses");
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P;
    int K = 0;
    if (int rc = ensure_steps(ctx, p->max_distance - kVisRadius, &K)) return rc;
    const VisEnv E = make_env(ctx, p, ctx->steps_d.as<const double>(), K);
    if (stats) {
        PCP_HIP(ctx, ctx->stats_d.ensure(4 * sizeof(unsigned long long) + 64));
        unsigned long long *sd = ctx->stats_d.as<unsigned long long>();
        PCP_HIP(ctx, hipMemsetAsync(sd, 0, 4 * sizeof(unsigned long long), st));
        if (C) {
            const dim3 g((unsigned)((C + kT - 1) / kT), (unsigned)(P + 1));
            if (E.K <= kStepLds)
                hipLaunchKernelGGL(k_score_cells_stats<true>, g, dim3(kT), 0, st, E,
                                   ctx->cells_xyz.as<const double>(),
                                   ctx->cells_nrm.as<const float>(), C, o.poses_k, P, o.zx_k, sd);
            else
                hipLaunchKernelGGL(k_score_cells_stats<false>, g, dim3(kT), 0, st, E,
                                   ctx->cells_xyz.as<const double>(),
                                   ctx->cells_nrm.as<const float>(), C, o.poses_k, P, o.zx_k, sd);
            PCP_CHECK_LAUNCH(ctx);
        }
        unsigned long long h[4] = {0, 0, 0, 0};
        PCP_HIP(ctx, hipMemcpyAsync(h, sd, sizeof(h), hipMemcpyDeviceToHost, st));
        PCP_HIP(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < 4; ++i) stats[i] = h[i];
    }
    if (ms) {
        *ms = 0.0;
        const char *what = "pcp_score_poses_burst";
        auto launch = [&]() -> int {   // (no cells: the empty interval)
            if (!C) return PCP_OK;
            launch_score_cells(st, ctx, E, C, P, o.poses_k, o.zx_k, o, o.score_z, nullptr, nullptr);
            const hipError_t e = hipGetLastError();
            return e == hipSuccess ? PCP_OK : hip_fail(ctx, e, what, __FILE__, __LINE__);
        };
        // (no warm-up: score_enqueue's own launch ran already)
        if (int rc = time_reps(ctx, what, st, reps, [] { return PCP_OK; }, launch, ms)) return rc;
    }
    PCP_HIP(ctx, hipStreamSynchronize(st));
    prof_resolve(ctx);
    return PCP_OK;
}

int pcp_score_matrix(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                     const pcp_vl_params *p, double *score_mobile, double *score_zx120) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || (n && !poses5) || (ctx->n_cells && (!score_zx120 || (n && !score_mobile))))
        return set_err(ctx, PCP_E_INVALID, "pcp_score_matrix: null argument");
    if (n > 65535) return set_err(ctx, PCP_E_INVALID, "pcp_score_matrix: too many poses");
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const size_t C = (size_t)o.C, P = (size_t)o.P;
    if (C) {
        if (P)
            PCP_HIP(ctx, hipMemcpyAsync(score_mobile, o.comb, P * C * sizeof(double),
                                        hipMemcpyDeviceToHost, st));
        PCP_HIP(ctx, hipMemcpyAsync(score_zx120, o.score_z, C * sizeof(double),
                                    hipMemcpyDeviceToHost, st));
    }
    PCP_HIP(ctx, hipStreamSynchronize(st));
    prof_resolve(ctx);
    return PCP_OK;
}

int pcp_score_poses_stats(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                          const pcp_vl_params *p, uint64_t stats[4]) {
    if (!ctx || !stats) return PCP_E_INVALID;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    return score_diag(ctx, poses5, n, zx, p, stats, 0, nullptr);
}

int pcp_score_poses_burst(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                          const pcp_vl_params *p, int reps, double *ms_per_launch) {
    if (!ctx || !ms_per_launch || reps <= 0) return PCP_E_INVALID;
    return score_diag(ctx, poses5, n, zx, p, nullptr, reps, ms_per_launch);
}

int pcp_generate_and_score(pcp_ctx *ctx, const double bb[6], const pcp_vl_params *p,
                           const double zx[5], double *poses5, uint64_t cap, uint64_t *n_out,
                           uint8_t *cell_flags, double *total_score, int32_t *covered,
                           pcp_vl_report *rep) {
    if (!ctx) return PCP_E_INVALID;
    const bool pend = ctx->area_pending;
    if (!bb || !p || !zx || !n_out || !rep || (cap && !poses5) ||
        ((pend ? ctx->cells_cap : ctx->n_cells) && !cell_flags))
        return set_err(ctx, PCP_E_INVALID, "pcp_generate_and_score: null argument");
    // (before the candidates are launched: the scoring behind them would refuse the table)
    if (int rc = steps_within_bound(ctx, p->max_distance - kVisRadius)) return rc;
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    const int gs = (int)std::ceil(std::sqrt((double)p->num_candidates));
    const int64_t L = gs > 0 ? (int64_t)gs * gs : 0;
    if (pend && (L == 0 || L > 65535 || !ctx->knob.zc_in || !PCP_ROW_SUM_LANES)) {
        // the two-call path needs the count on the host: settle the setup (fresh flags, :259)
        if (int rc = area_finish(ctx)) return rc;
        if (ctx->n_cells) std::memset(cell_flags, 0, ctx->n_cells);
        return pcp_generate_and_score(ctx, bb, p, zx, poses5, cap, n_out, cell_flags, total_score,
                                      covered, rep);
    }
    if (L == 0 || L > 65535 || !ctx->knob.zc_in) {   // the two calls (one synchronisation each)
        uint64_t n = 0;
        if (int rc = pcp_generate_candidates(ctx, bb, p, zx, poses5, cap, &n)) return rc;
        *n_out = n;
        return pcp_score_poses(ctx, poses5, n, zx, p, cell_flags, total_score, covered, rep);
    }
    // candidates -> device poses + their count (and the host's pinned copies), scoring sized
    // for the whole lattice with the count read on the device: one synchronisation
    CandArgs a = cand_args(ctx, bb, p, zx, gs);
    PCP_HIP(ctx, ctx->out_a.ensure((size_t)L * 6 * sizeof(double)));
    a.lat = ctx->out_a.as<double>();
    PCP_HIP(ctx, ctx->out_d.ensure((size_t)L * 5 * sizeof(double) + 64));
    double *poses_d = ctx->out_d.as<double>();
    uint32_t *n_d = reinterpret_cast<uint32_t *>(poses_d + 5 * (size_t)L);
    const size_t span = (size_t)L * 5 * sizeof(double) + sizeof(uint32_t);
    PCP_HIP(ctx, ctx->cand_host.ensure(span));
    double *poses_h = ctx->cand_host.as<double>();
    uint32_t *n_h = reinterpret_cast<uint32_t *>(poses_h + 5 * (size_t)L);
    if (int rc = cand_enqueue(ctx, a, (int)L, poses_d, n_d, poses_h, n_h)) return rc;
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, nullptr, (uint64_t)L, zx, p, o, cell_flags, true, true, n_d,
                               poses_d))
        return rc;
    if (int rc = score_tail_sync(ctx, o)) return rc;
    if (pend) {
        // the setup ran in front of this tick on the stream: an overflow of its neighbour lists
        // left the cells' normals incomplete -- settle it (regrow, rerun) and tick again from
        // fresh flags; otherwise its count is final (area_finish returns at once)
        const bool over = area_overflowed(ctx);
        if (int rc = area_finish(ctx, true)) return rc;   // (joined by score_enqueue, synced)
        if (over) {
            if (ctx->n_cells) std::memset(cell_flags, 0, ctx->n_cells);
            return pcp_generate_and_score(ctx, bb, p, zx, poses5, cap, n_out, cell_flags,
                                          total_score, covered, rep);
        }
    }
    const int Cn = pend ? (int)ctx->n_cells : o.C;   // the cells (o.C: the grids' size)
    const uint32_t P = *n_h;
    *n_out = P;
    prof_resolve(ctx);
    if (P > cap)
        return set_err(ctx, PCP_E_CAPACITY, "pcp_generate_and_score: need %u poses, cap %llu", P,
                       (unsigned long long)cap);
    if (P) std::memcpy(poses5, poses_h, (size_t)P * 5 * sizeof(double));
    score_tail_report(ctx, o, P, Cn, cell_flags, total_score, covered, rep);
    return PCP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// pcp_debug_math's double ops: one thread per element through the functions above -- the
// scoring's composite as eval_cell calls it, ocml's first results, the candidate generator's
// angle expression -- and the bare double operations the exactness arguments rest on
// ---------------------------------------------------------------------------------------
namespace pcp {

__global__ void __launch_bounds__(256)
k_debug_math_f64(int op, const double *__restrict__ a, const double *__restrict__ b, uint64_t n,
                 void *__restrict__ out, int32_t *__restrict__ aux) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    double *o = static_cast<double *>(out);
    switch (op) {
    case PCP_MATH_SCORE_SIN_PART: {
        o[i] = score_sin_part(x);
        int ph = 0;   // the phase: the same call with the phase asked for
        (void)pcp_score_sin_part(x, acos(x), &ph);
        aux[i] = ph;
        break;
    }
    case PCP_MATH_ACOS_RAW: o[i] = acos(x); break;
    case PCP_MATH_ATAN2_RAW: o[i] = atan2(x, b[i]); break;
    case PCP_MATH_ATAN2_CR: o[i] = pcp_cr_atan2_fix(x, b[i], atan2(x, b[i])); break;
    case PCP_MATH_F64_DIV: o[i] = x / b[i]; break;
    case PCP_MATH_F64_SQRT: o[i] = sqrt(x); break;
    case PCP_MATH_F64_TO_F32: static_cast<float *>(out)[i] = (float)x; break;
    case PCP_MATH_F64_FMA: o[i] = fma(x, b[2 * i], b[2 * i + 1]); break;
    case PCP_MATH_F64_NEXTAFTER: o[i] = nextafter(x, b[i]); break;
    case PCP_MATH_F64_NEARBYINT: o[i] = nearbyint(x); break;
    default: break;
    }
}

int debug_math_f64(pcp_ctx *ctx, int op, const double *a, const double *b, uint64_t n, void *out,
                   int32_t *aux) {
    hipLaunchKernelGGL(k_debug_math_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, op, a, b, n, out, aux);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

}  // namespace pcp
