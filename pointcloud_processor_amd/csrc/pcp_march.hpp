// pcp_march.hpp -- the ray march over the terrain index and its stencil scans, as the cell
// scoring (pcp_score.hip) and the dense ray fan (pcp_fan.hip) share them: templates and
// __forceinline__ device functions only, so each source compiles its own kernels around them.
// Both sources include it under #pragma clang fp contract(off) (no FMA, see their headers).
// Build knobs of the march: PCP_CELL_PROBES, PCP_BLK_STEP, PCP_NO_VGPR_PIN, PCP_WALK_CENSUS,
// PCP_CLAMP_INT, PCP_FAN_NO_PAIR, PCP_WALK_CENSUS_PAIR.
#pragma once

#include <cfloat>

#include "pcp_fan_clear.hpp"
#include "pcp_fan_clip.hpp"
#include "pcp_fan_row.hpp"
#include "pcp_internal.hpp"
#include "pcp_stencil.hpp"
#include "pcp_walk_pair.hpp"

namespace pcp {

constexpr int kT = 256;   // block size of both sources' kernels that state no other
#ifndef PCP_CELL_PROBES
// z-band probes issued per round in the cell-scoring march (build knob; 4 measured 130 vs 132
// us per 256-pose k_score_cells: that march is not probe-latency bound)
#define PCP_CELL_PROBES 1
#endif

// Lower-corner cell of the 2x2x2 stencil of a query (q - r - margin), as one linear index.
// False when the corner falls outside [0, n-2]^3: then the stencil holds only padding /
// outside cells and no point can be within r (exact skip, see DESIGN.md "Terrain index").
__device__ __forceinline__ bool stencil_cell(const GridView &g, float qx, float qy, float qz,
                                             uint32_t &lin) {
    uint32_t ix, iy, iz;
    const bool ok = stencil_cell3_fb(g, qx, qy, qz, ix, iy, iz);
    lin = ix + (uint32_t)g.nx * (iy + (uint32_t)g.ny * iz);
    return ok;
}

// Exact point tests of an occupied stencil: 2 x 2 rows (y, z) x 2 cells (x) = 8 runs.  Points
// of a cell are sorted by descending z, so a run ends at the first point with dz = qz - pz >= 0
// and fl(dz*dz) >= r2: FLANN's accumulator ((0 + dx^2) + dy^2) + dz^2 is >= fl(dz^2) (adding
// non-negative floats never decreases), and every later point of the run has a larger dz, so
// none of them can be within r (exact).
// Latency shape: round 1 = the 4 rows' directory entries (one 12-byte load per row: cells c,
// c+1 and the end of c+1); round 2 = the first point of all 8 runs (independent loads; an empty
// run reads point 0, one line shared by every such lane); only runs that continue are walked,
// 2 points per step.  Loads use 32-bit offsets from the kernel-argument bases.
template <bool STATS>
__device__ __forceinline__ bool scan_stencil(const GridView &g, uint32_t lin, float qx, float qy,
                                             float qz, float r2, uint32_t *cnt) {
    const uint32_t nx = (uint32_t)g.nx, nxy = nx * (uint32_t)g.ny;
    uint32_t b[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const U3 u = ld_u3o(g.start, lin + (r & 1) * nx + (r >> 1) * nxy);
        b[r][0] = u.a;
        b[r][1] = u.b;
        b[r][2] = u.c;
    }
    P3 f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t k = b[i >> 1][i & 1];
        f[i] = ld_p3o(g.pts, k < b[i >> 1][(i & 1) + 1] ? k : 0u);
    }
    uint32_t live = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t k = b[i >> 1][i & 1], e = b[i >> 1][(i & 1) + 1];
        if (k < e) {
            if (STATS) cnt[2] += 1;
            if (flann_within(qx, qy, qz, f[i], r2)) return true;
            const float dz = qz - f[i].z;
            if (!(dz >= 0.0f && dz * dz >= r2) && k + 1 < e) live |= 1u << i;
        }
    }
    if (!live) return false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (!(live & (1u << i))) continue;
        const uint32_t e = b[i >> 1][(i & 1) + 1];
        for (uint32_t k = b[i >> 1][i & 1] + 1; k < e; k += 2) {
            const P3 p0 = ld_p3o(g.pts, k);
            const P3 p1 = ld_p3o(g.pts, min(k + 1, e - 1));
            if (STATS) cnt[2] += 1;
            if (flann_within(qx, qy, qz, p0, r2)) return true;
            float dz = qz - p0.z;
            if (dz >= 0.0f && dz * dz >= r2) break;
            if (k + 1 >= e) break;
            if (STATS) cnt[2] += 1;
            if (flann_within(qx, qy, qz, p1, r2)) return true;
            dz = qz - p1.z;
            if (dz >= 0.0f && dz * dz >= r2) break;
        }
    }
    return false;
}

// The same test over the block-major copy: the block's points are one run in descending z,
// so one directory load, then one point per step until a point lies r below q (exact: every
// later point is lower still) -- a single early exit instead of one per cell.  (2, 3 or 4
// independent loads per step measured 1-2 % slower: the loads past the exit are wasted on the
// bound vector-memory path.)
#ifndef PCP_BLK_STEP
#define PCP_BLK_STEP 1   // block-walk points per step (build knob)
#endif
// a * b + c for a, b < 2^24 as one full-rate v_mad_u32_u24 (the compiler otherwise picks the
// 64-bit multi-pass v_mad_u64_u32 -- also for masked operands and for __umul24 plus an add; the
// operands are VGPRs, so a loop that multiplies by a scalar pins its copy first, vgpr_pin)
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// A wave-uniform value as a VGPR the compiler keeps: ahead of a loop whose instructions need it
// in a VGPR (mad_u24's operands, v_fmamk_f32's addend), instead of one v_mov_b32 per trip
template <class T>
__device__ __forceinline__ T vgpr_pin(T x) {
#ifndef PCP_NO_VGPR_PIN   // (A/B build knob)
    asm("" : "+v"(x));
#endif
    return x;
}

// entries per trip of the packed walk under march's SP (PCP_FAN_NO_PAIR: an A/B build that keeps
// the one-entry walk everywhere)
#ifdef PCP_FAN_NO_PAIR
template <bool SP> constexpr int kWalkSp = 1;
#else
template <bool SP> constexpr int kWalkSp = SP ? 2 : 1;
#endif

// a z-descending run pts[k0 .. e): the walk of one block (or one fine window)
template <bool STATS>
__device__ __forceinline__ bool scan_run(const float4 *pts, uint32_t k0, uint32_t e, float qx,
                                         float qy, float qz, float r2, uint32_t *cnt) {
    for (uint32_t k = k0; k < e; k += PCP_BLK_STEP) {
        P3 p[PCP_BLK_STEP];   // independent loads (the tail repeats the last entry)
#pragma unroll
        for (int i = 0; i < PCP_BLK_STEP; ++i) p[i] = ld_p3o(pts, min(k + i, e - 1));
#pragma unroll
        for (int i = 0; i < PCP_BLK_STEP; ++i) {
            if (i > 0 && k + i >= e) return false;
            if (STATS) cnt[2] += 1;
            if (flann_within(qx, qy, qz, p[i], r2)) return true;
            const float dz = qz - p[i].z;
            if (dz >= 0.0f && dz * dz >= r2) return false;
        }
    }
    return false;
}

// the packed (12-byte) entries' walk: the same test on x, y, z at k * 12
// WS 2 (the production fan kernels, march's SP): two entries per trip, pcp_walk_pair.hpp -- the
// same answer and the same tests from half the dependent round trips through vector memory.
// Both entries' loads are in flight before the first wait: left to itself the compiler sinks
// the second entry's load behind the first entry's test, so its floats are pinned right after
// the loads.
template <bool STATS, int WS = 1>
__device__ __forceinline__ bool scan_window3(const float *pts, uint32_t k, float qx, float qy,
                                             float qz, float r2, float rexit, uint32_t *cnt) {
    bool within, stop;
    if (WS == 2) {
        do {
            const float *f = walk_entry(pts, k);
            const float ax = f[0], ay = f[1], az = f[2];
            float bx = f[3], by = f[4], bz = f[5];
            asm volatile("" : "+v"(bx), "+v"(by), "+v"(bz));
            k += 2;
            uint32_t t;
            stop = walk_pair_step(ax, ay, az, bx, by, bz, qx, qy, qz, r2, rexit, within, t);
            if (STATS) cnt[2] += t;
        } while (!stop);
        return within;
    }
    const uint32_t k0 = k;
    (void)k0;
    do {
        const float *f = reinterpret_cast<const float *>(reinterpret_cast<const char *>(pts) +
                                                         ((k << 3) + (k << 2)));
        const P3 p = P3{f[0], f[1], f[2]};
        ++k;
        if (STATS) cnt[2] += 1;
#if defined(PCP_WALK_CENSUS) && !defined(PCP_WALK_CENSUS_PAIR)
        if (STATS && p.z - qz >= rexit) cnt[3] += 1;   // an entry r above q: a later start skips it
#endif
        within = flann_within(qx, qy, qz, p, r2);
        stop = within | (qz - p.z >= rexit);
    } while (!stop);
#if defined(PCP_WALK_CENSUS) && defined(PCP_WALK_CENSUS_PAIR)
    // (make census EXTRA=-DPCP_WALK_CENSUS_PAIR) a walk of an odd number of tests: the paired
    // walk's last trip loads an entry it does not test
    if (STATS && ((k - k0) & 1u)) cnt[3] += 1;
#endif
    return within;
}

// a fine window's walk from k: z-descending, ended by the window's sentinel (never within r,
// always r below), so no end index; dz >= rexit is FLANN's "fl(dz^2) >= r2" as one compare
template <bool STATS>
__device__ __forceinline__ bool scan_window(const float4 *pts, uint32_t k, float qx, float qy,
                                            float qz, float r2, float rexit, uint32_t *cnt) {
    bool within, stop;
    do {   // one exit condition: simple exec-mask bookkeeping per step
        const P3 p = ld_p3o(pts, k++);
        if (STATS) cnt[2] += 1;
#ifdef PCP_WALK_CENSUS
        if (STATS && p.z - qz >= rexit) cnt[3] += 1;
#endif
        within = flann_within(qx, qy, qz, p, r2);
        stop = within | (qz - p.z >= rexit);
    } while (!stop);
    return within;
}

template <bool STATS>
__device__ __forceinline__ bool scan_block(const GridView &g, uint32_t lin, float qx, float qy,
                                           float qz, float r2, uint32_t *cnt) {
    const uint2 se = ld_u2o(g.bstart, lin);
    return scan_run<STATS>(g.bpts, se.x, se.y, qx, qy, qz, r2, cnt);
}

template <bool STATS>
__device__ __forceinline__ bool scan_corner(const GridView &g, uint32_t lin, float qx, float qy,
                                            float qz, float r2, uint32_t *cnt) {
    if (g.bpts) return scan_block<STATS>(g, lin, qx, qy, qz, r2, cnt);
    return scan_stencil<STATS>(g, lin, qx, qy, qz, r2, cnt);
}

// KdTreeFLANN::radiusSearch(q, r) > 0 for r <= the index's stencil radius.
__device__ __forceinline__ bool stencil_any(const GridView &g, float qx, float qy, float qz,
                                            float r2) {
    uint32_t lin;
    if (!stencil_cell(g, qx, qy, qz, lin)) return false;
    if (!((ld_u32o(g.occ2, lin >> 5) >> (lin & 31)) & 1u)) return false;
    return scan_stencil<false>(g, lin, qx, qy, qz, r2, nullptr);
}

// clip_k in float (approximate reciprocal), pcp_fan_clip.hpp: the samples it drops lie outside
// the clip box shrunk by fan_clip_delta (< 1 mm of the margin beside the box's own 1e-6 |coord|),
// i.e. further than r from every point (the box is the point bbox inflated by r + m +
// 1e-6 |coord|): empty.  g.fclip_e samples of slack each side (2^-6; PCP_FAN_CLIP=0: 1).
__device__ __forceinline__ void clip_kf(const GridView &g, double px, double py, double pz,
                                        double dx, double dy, double dz, int K, int &klo,
                                        int &khi) {
    const float p[3] = {(float)px, (float)py, (float)pz};
    const float inv[3] = {__builtin_amdgcn_rcpf((float)dx), __builtin_amdgcn_rcpf((float)dy),
                          __builtin_amdgcn_rcpf((float)dz)};
    fan_clip(g.fb, p, inv, (float)(1.0 / kRayStep), g.fclip_e, K, klo, khi);
}
// the same from a pose row's six face differences (pcp_fan_row.hpp: fb[i] - (float)p, the
// subtractions fan_clip_slabs would do)
__device__ __forceinline__ void clip_kf_row(const GridView &g, const float *rel, double dx,
                                            double dy, double dz, int K, int &klo, int &khi) {
    const float inv[3] = {__builtin_amdgcn_rcpf((float)dx), __builtin_amdgcn_rcpf((float)dy),
                          __builtin_amdgcn_rcpf((float)dz)};
    fan_clip_rel(rel, inv, (float)(1.0 / kRayStep), g.fclip_e, K, klo, khi);
}

// checkVisibilityWithRaycasting's march (virtual_lidar.cpp:765-797) from pos along unit dir:
// the samples s_k < end in order, returns the first blocked k or -1.
//  * Samples outside the clip box have no point within r (clip_kf, exact skip).
//  * Probe: sample k's stencil-corner coordinates (cell units) are A + D k, one fma per axis,
//    instead of the double query point q_k = float(p + d s_k).  Their error against the exact
//    corner arithmetic is ~1e-5 m, far inside the 1 mm query margin that already absorbs the
//    float corner: a block found empty from the approximate corner holds no point
//    within r of q_k.
//  * ZB (the z-sorted terrain index): the probe reads the corner block's z band (GridView.occz)
//    and skips q_k when it lies >= r + 2 mm above the block's highest point or below its lowest
//    -- then dz alone exceeds r for every point of the block, so FLANN's float sum does too.
//    Without ZB the probe reads the block's occupancy bit.
//  * A surviving sample computes q_k exactly (s_k is the step table entry: the table was built
//    by the same repeated additions the reference performs) and scans the block of its exact
//    corner, so every point test is the reference's test.
// STATS counts probes, scanned stencils and point tests into cnt[0..2] (FN 8: probes, walk starts
// loaded, exact point tests with the pivot tests among them: the gather lane-loads by kind).
//  * FN (the fine-window copy, g.frec): the probe reads the record of the sample's fine corner
//    -- its window's z band and run -- and a candidate walks that run with the exact q_k.  The
//    approximate corner's window holds every point within r of q_k (the same margin argument as
//    the block's), so no exact corner and no directory load are needed.  FN = 2 decides at run
//    time (g.frec null or not).
//  * koff, kstr: a lane of a group of kstr lanes marching one ray takes the samples
//    k = klo + koff (mod kstr) (NB-sample rounds: the rounds koff (mod kstr)); the ray is blocked
//    iff some lane finds a blocked sample -- the group's answer to "march < 0" is the same
//  * CLR (the fan kernels): Skip 5, the jump over empty ground, below.  Cell scoring's march
//    leaves it out: its rays end at their cell, few of them run on underground, and the jump's
//    instructions cost it 1.7 %.
//  * PIV (the fan kernels, FN 8): Skip 6, a candidate tests its window's pivot first, below.
//    Cell scoring, the scan and the placement leave it out: their rays end at a visible cell, so
//    few of their candidates are hits.
//  * ROW (the level fan kernels): rowf is the float block of the pose's row (pcp_fan_row.hpp) --
//    the clip's face differences and the probe origin's pose part, formed once per pose on the
//    host with the expressions below, bit for bit; the other callers form them here.
//  * SP (the production fan kernel): the layout facts of the default build as compile-time
//    facts -- packed walk entries (g.wpack), two skip thresholds (g.fskip == 2), a pivot table
//    (g.fpiv) and clearance codes (g.fclear).  fan_launch picks an SP kernel only over a view that
//    has all four; the flags and the pointers they guard are then not held across the pose loop.
template <bool STATS, bool ZB = true, int NB = 1, int FN = 0, bool CLR = false, bool PIV = false,
          bool ROW = false, bool SP = false>
__device__ __forceinline__ int march(const GridView &g, double px, double py, double pz,
                                     double dx, double dy, double dz,
                                     const double *__restrict__ steps, int K, double end,
                                     float r2, float rexit, uint32_t *cnt = nullptr,
                                     int koff = 0, int kstr = 1, const float *rowf = nullptr) {
    static_assert(!SP || FN == 8, "the layout facts are the split records'");
    if (FN == 2) {
        if (g.frec && g.ftile == 2)
            return march<STATS, ZB, NB, 8, CLR, PIV, ROW>(g, px, py, pz, dx, dy, dz, steps, K,
                                                          end, r2, rexit, cnt, koff, kstr, rowf);
        if (g.frec && g.ftile)
            return march<STATS, ZB, NB, 4, CLR, PIV, ROW>(g, px, py, pz, dx, dy, dz, steps, K,
                                                          end, r2, rexit, cnt, koff, kstr, rowf);
        if (g.frec)
            return march<STATS, ZB, NB, 1, CLR, PIV, ROW>(g, px, py, pz, dx, dy, dz, steps, K,
                                                          end, r2, rexit, cnt, koff, kstr, rowf);
        return march<STATS, ZB, NB, 0, CLR, PIV, ROW>(g, px, py, pz, dx, dy, dz, steps, K, end,
                                                      r2, rexit, cnt, koff, kstr, rowf);
    }
    int klo, khi;
    if (ROW) clip_kf_row(g, rowf + FRF_CLIP, dx, dy, dz, K, klo, khi);
    else clip_kf(g, px, py, pz, dx, dy, dz, K, klo, khi);
    if (end < 1e299) {   // s_k < end: k <= (end - 0.5) / 0.3, with one sample of slack
        const double ke = floor((end - 0.5) / kRayStep) + 1.0;
        khi = (int)fmin((double)khi, fmax(ke, -1.0));
    }
    if (klo > khi) return -1;
    const float fdx = (float)dx, fdy = (float)dy, fdz = (float)dz;
    const float sc = (float)kRayStep * g.finv_c, h = 0.5f * g.finv_c;   // s_k = 0.5 + 0.3 k
    const float Dx = fdx * sc, Dy = fdy * sc, Dz = fdz * sc;
    const float Ax = (ROW ? rowf[FRF_BASE] : ((float)px - g.flo_x) * g.finv_c) + fdx * h;
    const float Ay = (ROW ? rowf[FRF_BASE + 1] : ((float)py - g.flo_y) * g.finv_c) + fdy * h;
    const float Az = (ROW ? rowf[FRF_BASE + 2] : ((float)pz - g.flo_z) * g.finv_c) + fdz * h;
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny;
    if (FN == 1 || FN == 4 || FN == 8) {
        // fine units for x, y (the fine cell of the sample, (q - o) / c_f = F (f + fzoff)),
        // coarse stencil-corner units for z; out-of-range cells are clamped: a sample outside
        // the grid has no point within r, and a clamped record can only cost a walk whose exact
        // tests all fail.  The float cell is within ~1e-5 m of the exact one, inside the margin
        // m of the window's radius r + m (pcp_fine.hip).
        const float F = g.ffine;
        const float D2x = F * Dx, D2y = F * Dy, A2x = F * (Ax + g.fzoff), A2y = F * (Ay + g.fzoff);
        const uint32_t mx = g.frx - 1, my = g.fry - 1, mz = g.frz - 1;
        const float fmx = (float)mx, fmy = (float)my, fmz = (float)mz;
        (void)mx, (void)my, (void)mz, (void)fmx, (void)fmy, (void)fmz;
        const uint32_t rxs = FN == 4 ? (g.frx + 3) >> 2 : FN == 8 ? (g.frx + 7) >> 3 : g.frx;
        const uint32_t rys = FN == 4 ? (g.fry + 3) >> 2 : FN == 8 ? (g.fry + 7) >> 3 : g.fry;
        // (FN 8, the fan's layout: the tile counts and the probe's height offset pinned in
        // VGPRs for the loop -- three v_mov_b32 per probe fewer)
        const uint32_t rx = FN == 8 ? vgpr_pin(rxs) : rxs, ry = FN == 8 ? vgpr_pin(rys) : rys;
        const float fus_off = FN == 8 ? vgpr_pin(g.fus_off) : g.fus_off;
        // Skip 5 (FN 8 with CLR, pcp_fan_clear.hpp): a descending ray whose sample reads an
        // empty record with clearance code e jumps its next floor((e c_f - rb) / hs) samples.
        // They are lower than q_k and horizontally within e c_f - rb of it, q_k lies in the
        // record's cell up to the probe's error (inside m), and no point at or below the record's
        // Zt lies within e c_f of that cell: none of them has a point within r.  A clamped probe
        // reads a border record, whose code is 0; a ray that does not descend (or the knob off)
        // has a = b = 0.
        const ClearRay cr = FN == 8 && CLR ? fan_clear_ray(fdx, fdy, fdz, (float)kRayStep, g.fclr_cf,
                                                    g.fclr_rb, SP || g.fclear != 0)
                                    : ClearRay{0.0f, 0.0f};
        // jump: the samples skipped after sample k; the lane goes on at its next own sample
        // past k + jump (a group's lanes keep their residue)
        for (int k = klo + koff, jump = 0; k <= khi; k += kstr * (1 + jump / kstr)) {
            const float kf = (float)k;
            const float fx = __builtin_fmaf(D2x, kf, A2x);
            const float fy = __builtin_fmaf(D2y, kf, A2y);
            const float fz = __builtin_fmaf(Dz, kf, Az);
            // the clamp to [0, m] in float, one v_med3_f32 before the conversion: m < 2^24 is a
            // float, a value in (m, m + 1) converts to m either way, and a NaN gives
            // min(NaN, 0, m) = 0 as fmaxf(NaN, 0) did -- the same cell for every input
#ifdef PCP_CLAMP_INT   // A/B build only: the former three instructions per axis
            const uint32_t ix = min((uint32_t)fmaxf(fx, 0.0f), mx);
            const uint32_t iy = min((uint32_t)fmaxf(fy, 0.0f), my);
            const uint32_t iz = min((uint32_t)fmaxf(fz, 0.0f), mz);
#else
            const uint32_t ix = (uint32_t)__builtin_amdgcn_fmed3f(fx, 0.0f, fmx);
            const uint32_t iy = (uint32_t)__builtin_amdgcn_fmed3f(fy, 0.0f, fmy);
            const uint32_t iz = (uint32_t)__builtin_amdgcn_fmed3f(fz, 0.0f, fmz);
#endif
            // 24-bit multiply-adds (full rate): build_fine caps frx, fry * frz below 2^24.
            // FN 4: records in 4 x 4 xy tiles, one 128-byte line each (a wave's arc of probes
            // touches fewer lines whatever its direction); rx, ry are then the tile counts.
            // FN 8: the split records in 8 x 8 tiles, the probe reads only the 2-byte thresholds
            // (64 per 128-byte line: a quarter of FN 4's bytes through the texture path) and a
            // candidate then its 4-byte walk start
            const uint32_t ri = FN == 8 ? (mad_u24(rx, mad_u24(ry, iz, iy >> 3), ix >> 3) << 6) |
                                              ((iy & 7u) << 3) | (ix & 7u)
                              : FN == 4 ? (mad_u24(rx, mad_u24(ry, iz, iy >> 2), ix >> 2) << 4) |
                                              ((iy & 3u) << 2) | (ix & 3u)
                                        : mad_u24(rx, mad_u24(ry, iz, iy), ix);
            uint2 R = make_uint2(0u, 0u);   // FN 8: only the thresholds (.y) come with the probe
            if (FN == 8) R.y = ld_u16o(g.fband, ri);
            else R = ld_rec(g.frec, ri);
            // height above the block floor in kZq steps against the record's thresholds
            const float us = __builtin_fmaf(fz - (float)iz, 1.0f / kZq, fus_off);
            const float lo = (float)(R.y & 255u);   // 255: an empty record
            const bool cand = (us < (float)((R.y >> 8) & 255u)) & (us > lo);
            // Skip 5: the samples to jump after this one (0 unless the record is empty)
            // (the empty asm keeps these few instructions here, ahead of the candidate branch:
            // sunk below it they become a masked block of their own at the loop's end)
            jump = (FN == 8 && CLR && lo == 255.0f) ? fan_clear_skip((float)(R.y >> 8), cr)
                                                    : 0;
            if (FN == 8 && CLR) asm volatile("" : "+v"(jump));
            if (STATS) cnt[0] += 1;
            if (cand) {
                const double s = steps[k];
                if (!(s < end)) return -1;
                const float qx = (float)(px + dx * s);
                const float qy = (float)(py + dy * s);
                const float qz = (float)(pz + dz * s);
                // Skip 6 (FN 8 with PIV, pcp_fan_pivot.hpp): the window's point nearest its
                // cell's centre, tested first with the walk's own predicate.  Within r: a
                // terrain point within r of q_k, which is all radiusSearch(q, r) > 0 asks -- no
                // walk start, no entry.  Otherwise nothing is concluded and the walk runs as it
                // did.  The table's tiles are the band records' (rx = g.fptx; ri's low 6 bits
                // are the cell's place in its tile); an empty window's sentinel is never within r.
                if (FN == 8 && PIV && (SP || g.fpiv)) {
                    const uint32_t pi = (mad_u24(rx, iy >> 3, ix >> 3) << 6) | (ri & 63u);
                    const float *pf = reinterpret_cast<const float *>(
                        reinterpret_cast<const char *>(g.fpiv) + ((pi << 3) + (pi << 2)));
                    const P3 pv = P3{pf[0], pf[1], pf[2]};
                    if (STATS) cnt[2] += 1;
                    if (flann_within(qx, qy, qz, pv, r2)) return k;
                }
                if (STATS) cnt[1] += 1;
                uint32_t w0 = R.x;
                if (FN == 8) {   // skip the run's entries > r above q (pcp_fine.hip, k_frec)
                    const uint32_t ws = ld_u32o(g.fstart, ri);
                    // the thresholds are the record's double heights rounded through fzo, fzc
                    // and the fma (a few ulps of the larger magnitude): the margin grows with
                    // them, so far from the origin (|z| of km) the skip stays exact
                    if (SP || g.fskip == 2) {
                        const float ha = __builtin_fmaf((float)iz + 1.375f, g.fzc, g.fzo);
                        const float hb = __builtin_fmaf((float)iz + 1.6875f, g.fzc, g.fzo);
                        const float marg = 1e-4f + 4.0f * FLT_EPSILON *
                                                       (fmaxf(fabsf(ha), fabsf(hb)) +
                                                        fabsf(g.fzo) + fabsf(qz));
                        const float v = qz + (rexit + marg);
                        w0 = (ws & 0x01FFFFFFu) +
                             (v < ha ? (ws >> 25) & 15u : v < hb ? ws >> 29 : 0u);
                    } else {
                        const float h2 = __builtin_fmaf((float)iz + 1.5f, g.fzc, g.fzo);
                        const float marg =
                            1e-4f + 4.0f * FLT_EPSILON * (fabsf(h2) + fabsf(g.fzo) + fabsf(qz));
                        w0 = (ws & 0x0FFFFFFFu) + (qz + (rexit + marg) < h2 ? ws >> 28 : 0u);
                    }
                }
                const bool packed = SP || g.wpack;
                if (packed ? scan_window3<STATS, kWalkSp<SP>>(
                                 reinterpret_cast<const float *>(g.wpts), w0, qx, qy, qz, r2, rexit,
                                 cnt)
                           : scan_window<STATS>(g.wpts, w0, qx, qy, qz, r2, rexit, cnt))
                    return k;
            }
        }
        return -1;
    }
    if (NB > 1 && ZB) {
        // latency-bound callers (few rays in flight): NB probes per round as independent loads,
        // then taken in sample order -- the same samples, candidates and scans as below
        for (int k0 = klo + NB * koff; k0 <= khi; k0 += NB * kstr) {
            uint32_t zz[NB], izs[NB];
            float fzs[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float kf = (float)(k0 + b);
                const float fx = __builtin_fmaf(Dx, kf, Ax);
                const float fy = __builtin_fmaf(Dy, kf, Ay);
                const float fz = __builtin_fmaf(Dz, kf, Az);
                const bool ok = (k0 + b <= khi) & (fx >= 0.0f) & (fx < g.fnx1) & (fy >= 0.0f) &
                                (fy < g.fny1) & (fz >= 0.0f) & (fz < g.fnz1);
                const uint32_t izc = ok ? (uint32_t)fz : 0u;
                const uint32_t lin = ok ? (uint32_t)fx + nx * ((uint32_t)fy + ny * izc) : 0u;
                zz[b] = ok ? ld_u16o(g.occz, lin) : 0x00FFu;
                izs[b] = izc;
                fzs[b] = fz;
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int k = k0 + b;
                const uint32_t lo = zz[b] & 255u, hi = zz[b] >> 8;
                const float u = fzs[b] - (float)izs[b] + g.fzoff;
                const bool cand = (lo <= hi) & ((hi == 255u) | (u - (float)hi * kZq < g.fzt)) &
                                  ((lo == 0u) | ((float)lo * kZq - u < g.fzt));
                if (STATS && k <= khi) cnt[0] += 1;
                if (cand) {
                    const double s = steps[k];
                    if (!(s < end)) return -1;
                    if (STATS) cnt[1] += 1;
                    const float qx = (float)(px + dx * s);
                    const float qy = (float)(py + dy * s);
                    const float qz = (float)(pz + dz * s);
                    uint32_t l2;
                    if (stencil_cell(g, qx, qy, qz, l2) && scan_corner<STATS>(g, l2, qx, qy, qz, r2, cnt))
                        return k;
                }
            }
        }
        return -1;
    }
    for (int k = klo + koff; k <= khi; k += kstr) {
        const float kf = (float)k;
        const float fx = __builtin_fmaf(Dx, kf, Ax);
        const float fy = __builtin_fmaf(Dy, kf, Ay);
        const float fz = __builtin_fmaf(Dz, kf, Az);
        const bool ok = (fx >= 0.0f) & (fx < g.fnx1) & (fy >= 0.0f) & (fy < g.fny1) &
                        (fz >= 0.0f) & (fz < g.fnz1);
        const uint32_t izc = ok ? (uint32_t)fz : 0u;
        const uint32_t lin = ok ? (uint32_t)fx + nx * ((uint32_t)fy + ny * izc) : 0u;
        bool cand;
        if (ZB) {
            const uint32_t zz = ok ? ld_u16o(g.occz, lin) : 0x00FFu;
            const uint32_t lo = zz & 255u, hi = zz >> 8;
            const float u = fz - (float)izc + g.fzoff;          // (q_z - block floor) / c
            cand = (lo <= hi) & ((hi == 255u) | (u - (float)hi * kZq < g.fzt)) &
                   ((lo == 0u) | ((float)lo * kZq - u < g.fzt));
        } else {
            const uint32_t word = ok ? ld_u32o(g.occ2, lin >> 5) : 0u;
            cand = (word >> (lin & 31u)) & 1u;
        }
        if (STATS) cnt[0] += 1;
        if (cand) {
            const double s = steps[k];
            if (!(s < end)) return -1;       // every later sample is beyond end too
            if (STATS) cnt[1] += 1;
            const float qx = (float)(px + dx * s);
            const float qy = (float)(py + dy * s);
            const float qz = (float)(pz + dz * s);
            uint32_t l2;
            if (stencil_cell(g, qx, qy, qz, l2) && scan_corner<STATS>(g, l2, qx, qy, qz, r2, cnt))
                return k;
        }
    }
    return -1;
}

}  // namespace pcp
