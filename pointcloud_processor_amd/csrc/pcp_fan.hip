// pcp_fan.hip -- the dense ray-fan occlusion march on gfx950: every fan kernel over the shared
// march (pcp_march.hpp), their tables and the one launch, the per-pose sums, and the
// pcp_raycast_fan* entries.  The reference's cell scoring is pcp_score.hip.
//
// Numerics: compiled with -ffp-contract=off (no FMA) so every double/float operation
// rounds exactly as the reference's SSE2 build.  The radius predicate restates FLANN's
// L2_Simple<float> (x, y, z accumulated in order, strict '<' against float(r*r)).
// Build knobs of this file: PCP_FAN_NO_ROW, PCP_FAN_NO_SP, PCP_FAN_NO_PRO1.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_ext.h>

#include "pcp_fan_cull.hpp"
#include "pcp_fan_dir.hpp"
#include "pcp_internal.hpp"
#include "pcp_march.hpp"

namespace pcp {

// ---------------------------------------------------------------------------------------
// dense ray fan (BASELINE configs[1])
// ---------------------------------------------------------------------------------------
struct FanArgs {
    GridView g;
    const double *ca, *sa, *ce, *se;
    const double *pose;    // P x kFanRow, the rows of pcp_fan_row.hpp: the pose, cos / sin of its
                           // yaw, its live rings [j0, j1) (pcp_fan_cull.hpp) and the preamble's
                           // pose-uniform floats; the mounted kernels: P x kFanDirRow, the rows
                           // of pcp_fan_dir.hpp
    const double *steps;
    int K;
    int n_az;
    int uniform_el;        // every wave lies in one elevation ring
    uint32_t rays;
    uint32_t waves;        // waves per pose = ceil(rays / 64)
    float r2, rexit;
    int present;
    int16_t *first_hit;
    // the launch covers the waves [w0, w0 + lw) of each pose: the others hold only rays of rings
    // that reach the terrain from no pose of the call (Skip 4; w0 = 0, lw = waves: no culling).
    // rev: ray block b of the launch is wave w0 + lw - 1 - b, not w0 + b
    uint32_t w0, lw;
    int rev;
    // per-wave partials {blocked, units}, one 8-byte store per wave (no atomics), pose-major:
    // slot = p * lw + w - w0.  Every wave of a pose runs on one XCD (the XCD-chunk kernels: XCD
    // p / (P / 8); the interleaved ones: XCD p % 8), so that XCD's L2 fills the pose's lines,
    // and k_fan_reduce reads each pose's partials as one contiguous run
    uint2 *wave_part;
    uint32_t P;
    unsigned long long *stats;     // MODE 1: probes, scanned stencils, point tests
                                   // MODE 2: per-wave s_memtime stamps [P*waves][4]
};

enum { FAN_PLAIN = (int)FanMode::Plain, FAN_STATS = (int)FanMode::Stats,
       FAN_STAMPS = (int)FanMode::Stamps };

// sum over the 64 lanes (all active): rotate-adds inside each 16-lane row (DPP row_ror 8, 4,
// 2, 1), then the four row sums by readlane -- no LDS crossbar round trips
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// one lane = one ray; 64 consecutive azimuths of one elevation ring per wave (coherent
// termination on near-flat terrain).  Each wave writes its blocked-ray count and its
// sample-query count to its own slot: the per-pose sums are formed by k_fan_reduce in a fixed
// order (deterministic, no same-address atomics).
// MT: the mounted form (pcp_raycast_fan_mounted, Plain only).  The pose rows are pcp_fan_dir.hpp's
// and the direction is its fan_dir() -- roll, pitch and yaw per pose on the wave's shared local
// direction; a tilted ring has no one dz, so there is no ring liveness (Skip 4) and the launch
// covers the full grid.
// SP: march's layout facts (the production kernel; fan_launch).
template <int MODE, int BS, bool ZB = true, int FN = 0, bool UE = false, int NPW = 1,
          bool SL = false, bool MT = false, bool SP = false>
__device__ __forceinline__ void fan_body(const FanArgs &a, uint32_t p0, uint32_t rblock) {
    static_assert(!MT || MODE == FAN_PLAIN, "the mounted march has no diagnostic modes");
    static_assert(!SP || !MT, "the mounted kernels keep the run-time layout tests");
    constexpr int PR = MT ? kFanDirRow : kFanRow;   // doubles per pose row
    static_assert(PR * 32 * sizeof(double) + kStepLds * sizeof(double) <= 160 * 1024 / 8,
                  "at the widest NPW at least 8 one-wave workgroups per CU keep their LDS");
    const uint32_t ray = rblock * BS + threadIdx.x;
    const uint32_t wid = ray >> 6;
    const bool active = ray < a.rays;
    // the ray's direction in the pose frame, loaded once for the wave's NPW poses (poses
    // p0 .. p0 + NPW - 1 share the fan: the table loads are a quarter of the launch's
    // vector-memory bytes at NPW 1)
    double lx = 0.0, ly = 0.0, lz = 0.0;
    // SL: the step table in LDS (the launcher guarantees K <= kStepLds): one load per 64
    // entries per workgroup, then a candidate's step is an LDS read instead of a gather through
    // the texture path
    // and the wave's NPW pose rows (contiguous: one coalesced load) behind the same barrier: a
    // pose's values and its live rings are then LDS broadcasts, not a round trip through
    // vector memory at the top of every pose
    __shared__ double s_steps[SL ? kStepLds : 1];
    // (whole trips of BS lanes: the staging below stores every lane's value unguarded)
    __shared__ double s_pose[SL ? (PR * NPW + BS - 1) / BS * BS : 1];
#ifdef PCP_FAN_NO_PRO1   // A/B build only: each staging loop and each table load waits by itself
    constexpr bool PRO1 = false;
#else
    constexpr bool PRO1 = SL;
#endif
    if (PRO1) {
        // every address of the prologue is known at the wave's start: the step table's entries,
        // the rows and the four direction-table values are all loaded before the first wait --
        // one round trip through vector memory, not one per staging trip and table
        constexpr int NS = kStepLds / BS, NR = (PR * NPW + BS - 1) / BS;
        static_assert(kStepLds % BS == 0, "whole trips over the step table");
        double sv[NS], rv[NR], cej = 0.0, cai = 0.0, sai = 0.0, sej = 0.0;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int q = (int)threadIdx.x + t * BS;
            sv[t] = q < a.K ? a.steps[q] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < NR; ++t) {
            const int q = (int)threadIdx.x + t * BS;
            rv[t] = q < PR * NPW ? a.pose[PR * (size_t)p0 + q] : 0.0;
        }
        if (active && a.present) {
            const uint32_t j = UE ? (rblock * BS + (threadIdx.x & ~63u)) / (uint32_t)a.n_az
                                  : ray / (uint32_t)a.n_az;
            const uint32_t i = ray - j * (uint32_t)a.n_az;
            cej = a.ce[j];
            cai = a.ca[i];
            sai = a.sa[i];
            sej = a.se[j];
        }
        // (both arrays hold whole trips: an entry past K or past the rows is a zero nobody
        // reads, and the stores need no guard -- one block, one wait)
#pragma unroll
        for (int t = 0; t < NS; ++t) s_steps[threadIdx.x + t * BS] = sv[t];
#pragma unroll
        for (int t = 0; t < NR; ++t) s_pose[threadIdx.x + t * BS] = rv[t];
        __syncthreads();
        if (active && a.present) {
            lx = cej * cai;
            ly = cej * sai;
            lz = sej;
        }
    } else if (SL) {
        for (int q = threadIdx.x; q < a.K; q += BS) s_steps[q] = a.steps[q];
        for (int q = threadIdx.x; q < PR * NPW; q += BS) s_pose[q] = a.pose[PR * (size_t)p0 + q];
        __syncthreads();
    }
    const double *steps = SL ? s_steps : a.steps;
    // UE: the wave's ring as a scalar, tested against each pose's live rings below
    uint32_t ju = 0;
    if (UE)
        ju = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)((rblock * BS + (threadIdx.x & ~63u)) / (uint32_t)a.n_az));
    if (!PRO1 && active && a.present) {
        // UE (n_az % 64 == 0): the wave's ring is uniform, a scalar division of its first ray
        const uint32_t j = UE ? (rblock * BS + (threadIdx.x & ~63u)) / (uint32_t)a.n_az
                              : ray / (uint32_t)a.n_az;
        const uint32_t i = ray - j * (uint32_t)a.n_az;
        const double cej = a.ce[j];
        lx = cej * a.ca[i];
        ly = cej * a.sa[i];
        lz = a.se[j];
    }
#pragma unroll 1
    for (int q = 0; q < NPW; ++q) {
    const uint32_t p = p0 + (uint32_t)q;
    const uint32_t wslot = p * a.waves + wid;
    unsigned long long t0 = 0, t1 = 0, t2 = 0;
    if (MODE == FAN_STAMPS) t0 = __builtin_amdgcn_s_memtime();
    int hit = -1;
    uint32_t cnt[4] = {0, 0, 0, 0};   // [3]: PCP_WALK_CENSUS builds only
    // Skip 4, per pose: a ring outside the pose's live interval has every sample of every ray
    // outside the clip box -- no rotation, no clip, no reductions (a uniform test: the ring
    // and the pose's interval are scalars)
    const double *P = SL ? s_pose + PR * q : a.pose + PR * (size_t)p;
    bool dead = false;
    FanDir md{0.0, 0.0, 0.0};
    // (a per-wave early-out -- every lane's two end heights against the clip box with the ring
    // test's arithmetic, the march skipped on a full ballot -- measured no gain over the clip's
    // own immediate return: 0.0557 vs 0.0555 ms at zero tilt, profiles/mount_early_out_ab.json)
    if (MT) md = fan_dir(P, lx, ly, lz);
    if (UE && !MT) {
        const uint2 lr = *reinterpret_cast<const uint2 *>(P + FR_LIVE);
        const uint32_t j0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lr.x);
        const uint32_t j1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lr.y);
        dead = ju < j0 || ju >= j1;
        if (MODE == FAN_STAMPS && dead) t1 = t0;
    }
    if (!dead && active && a.present) {
        const double cy = MT ? 0.0 : P[FR_CY], sy = MT ? 0.0 : P[FR_SY];
        const double dx = MT ? md.x : cy * lx - sy * ly;
        const double dy = MT ? md.y : sy * lx + cy * ly;
        const double dz = MT ? md.z : lz;
        if (MODE == FAN_STAMPS) {
            asm volatile("" ::"v"(dx), "v"(dy));
            t1 = __builtin_amdgcn_s_memtime();
        }
        // (the level rows carry the preamble's pose-uniform floats; a mounted row does not)
#ifdef PCP_FAN_NO_ROW   // A/B build only: the row's floats unused, the preamble derives them
        constexpr bool ROW = false;
#else
        constexpr bool ROW = !MT;
#endif
        hit = march<MODE == FAN_STATS, ZB, 1, FN, true, true, ROW, SP>(
            a.g, P[0], P[1], P[2], dx, dy, dz, steps, a.K, 1e300, a.r2, a.rexit, cnt, 0, 1,
            MT ? nullptr : fan_row_floats(P));
    }
    if (MODE == FAN_STAMPS) {
        asm volatile("" ::"v"(hit));
        t2 = __builtin_amdgcn_s_memtime();
    }
    if (active && a.first_hit) a.first_hit[(size_t)p * a.rays + ray] = (int16_t)hit;
    uint2 part;
    if (UE && !MT && dead) {   // (UE: every wave is full)
        part = make_uint2(0u, 64u * (uint32_t)a.K);
    } else {
        const uint64_t bal = __ballot(active && hit >= 0);
        uint32_t u = active ? (hit >= 0 ? (uint32_t)hit + 1u : (uint32_t)a.K) : 0u;
        part = make_uint2((uint32_t)__popcll(bal), wave_sum_u32(u));
    }
    if ((threadIdx.x & 63) == 0 && wid < a.waves) {
        a.wave_part[(size_t)p * a.lw + (wid - a.w0)] = part;
    }
    if (MODE == FAN_STATS) {   // per-wave slots [4][P * waves], summed by k_sum_u64
        const size_t nw = (size_t)a.P * a.waves;
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // [3] directory loads: one per scan (none: FN, the
                                        // probe's record is the directory)
            // (a PCP_WALK_CENSUS build: FN's [3] = the walks' tests of entries r above q)
            unsigned long long v = c < 3 ? cnt[c] : (FN ? cnt[3] : cnt[1]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((threadIdx.x & 63) == 0 && wid < a.waves) a.stats[c * nw + wslot] = v;
        }
    }
    if (MODE == FAN_STAMPS && (threadIdx.x & 63) == 0 && wid < a.waves) {
        const unsigned long long t3 = __builtin_amdgcn_s_memtime();
        unsigned long long *o = a.stats + 4 * (size_t)wslot;
        o[0] = t0;
        o[1] = t1;
        o[2] = t2;
        o[3] = t3;
    }
    }   // poses of the wave
}

// The fan kernel: one wave per workgroup (a finished wave's slot refills without waiting for
// the rest of a workgroup), 1-D grid interleaving the poses (block b = ray block b / P of pose
// b % P: the waves in flight at any time march the same ring of many poses), capped at 7 waves
// per SIMD (94 SGPRs; the compiler's own choice, 106, admits only 6).
template <int MODE, int BS = 64, bool ZB = true, int W = 7, int FN = 0, bool UE = false,
          bool MT = false>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(W, W)))
k_raycast_fan(FanArgs a, uint32_t P) {
    fan_body<MODE, BS, ZB, FN, UE, 1, false, MT>(a, blockIdx.x % P, a.w0 + blockIdx.x / P);
}

// A/B: XCD-chunked placement (P % 8 == 0): workgroup b runs on XCD b % 8, which takes the
// contiguous pose chunk [x P/8, (x + 1) P/8) -- neighbouring candidate poses, overlapping fans
// -- interleaved inside the XCD as above
// NPW > 1: each wave marches its rays for NPW consecutive poses of the chunk (one direction-
// table load for all of them); P % (8 NPW) == 0, grid = lw * P / NPW (the live waves, Skip 4).
// a.rev: the launch's last wave first.  Workgroups are dispatched in index order and the rings
// just below the horizon march 2-3 times as long as the steep ones: dispatched last they would
// be the launch's tail
template <int MODE, int BS = 64, bool ZB = true, int W = 8, int FN = 1, bool UE = true, int NPW = 1,
          bool MT = false, bool SP = false>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(W, W)))
k_raycast_fan_xcd(FanArgs a, uint32_t P) {
    const uint32_t pc = P >> 3, gpc = pc / NPW, j = blockIdx.x >> 3;
    const uint32_t b = j / gpc;
    fan_body<MODE, BS, ZB, FN, UE, NPW, true, MT, SP>(a, (blockIdx.x & 7u) * pc + (j % gpc) * NPW,
                                                      a.w0 + (a.rev ? a.lw - 1u - b : b));
}

// A/B: pose-major 2-D grid (blockIdx.y = pose), BS-thread workgroups (P: unused, fan_launch's)
template <int BS, bool ZB>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(7, 7)))
k_raycast_fan_pm(FanArgs a, uint32_t) {
    fan_body<FAN_PLAIN, BS, ZB>(a, blockIdx.y, blockIdx.x);
}

// out[q] = sum of in[q * n .. (q + 1) * n) (one block per q)
__global__ void __launch_bounds__(1024)
k_sum_u64(const unsigned long long *__restrict__ in, size_t n, unsigned long long *__restrict__ out) {
    const unsigned long long *row = in + (size_t)blockIdx.x * n;
    unsigned long long v = 0;
    for (size_t k = threadIdx.x; k < n; k += 1024) v += row[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __shared__ unsigned long long sw[16];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += sw[w];
        out[blockIdx.x] = t;
    }
}

// per-pose sums of the per-wave partials: one block per pose, fixed order (integer sums:
// exact and deterministic).  waves: the live waves the launch covered (0: none was launched);
// the culled rays' share (Skip 4) is closed-form: none blocked, K units each = units_culled per
// pose.  fh (nullable): their first hits, rays [0, r_lo) and [r_hi, rays) of the pose, are -1.
__global__ void __launch_bounds__(kT)
k_fan_reduce(const uint2 *__restrict__ part, uint32_t waves,
             uint32_t *__restrict__ blocked, unsigned long long *__restrict__ units,
             unsigned long long *__restrict__ keys, uint32_t lo, uint32_t Pall,
             unsigned long long units_culled, int16_t *__restrict__ fh, uint32_t rays,
             uint32_t r_lo, uint32_t r_hi) {
    const uint32_t p = blockIdx.x;
    if (fh) {
        int16_t *row = fh + (size_t)p * rays;
        for (uint32_t r = threadIdx.x; r < r_lo; r += kT) row[r] = (int16_t)-1;
        for (uint32_t r = r_hi + threadIdx.x; r < rays; r += kT) row[r] = (int16_t)-1;
    }
    if (keys)   // (FanEnq.keys) the other ranks' slots and the health word: the MIN identity
        for (uint32_t i = p * kT + threadIdx.x; i <= Pall; i += gridDim.x * kT)
            if (i < lo || i - lo >= gridDim.x) keys[i] = ~0ull;
    const uint2 *row = part + (size_t)p * waves;   // the pose's partials, contiguous
    uint32_t b = 0;
    unsigned long long u = 0;
    for (uint32_t w = threadIdx.x; w < waves; w += kT) {
        const uint2 v = row[w];
        b += v.x;
        u += v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        b += __shfl_xor(b, o, 64);
        u += __shfl_xor(u, o, 64);
    }
    __shared__ uint32_t sb[kT / 64];
    __shared__ unsigned long long su[kT / 64];
    if ((threadIdx.x & 63) == 0) {
        sb[threadIdx.x >> 6] = b;
        su[threadIdx.x >> 6] = u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t bs = sb[0] + sb[1] + sb[2] + sb[3];
        const unsigned long long us = su[0] + su[1] + su[2] + su[3] + units_culled;
        blocked[p] = bs;
        units[p] = us;
        if (keys) {
            keys[lo + p] = ((unsigned long long)bs << 32) | (unsigned long long)(lo + p);
            keys[(size_t)Pall + 1 + p] = us;
        }
        // the outputs may be pinned host memory (fan_host_out): the caller reads them after
        // hipStreamSynchronize, whose completion signal carries the kernel's system-scope
        // release.  A __threadfence_system() per block here measured 11.7 vs 5.8 us per launch
        // (profiles/r02_fan_ab_fence.log) for nothing the synchronisation does not give.
    }
}

// the pose-sharded search across GPUs (pcp_multi.hip), one rank's key vector:
// keys[i] = (blocked << 32) | i for this rank's poses [lo, lo + cnt), UINT64_MAX elsewhere;
// all-reduce(MIN) leaves every pose's key on every rank and the minimum key is the reference
// argmin with ties to the lowest index
__global__ void __launch_bounds__(kT)
k_fan_keys(const uint32_t *__restrict__ blocked, uint32_t lo, uint32_t cnt, uint32_t P,
           unsigned long long *__restrict__ keys, unsigned long long identity) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= P) return;
    keys[i] = (i >= lo && i - lo < cnt)
                  ? (((unsigned long long)blocked[i - lo] << 32) | (unsigned long long)i)
                  : identity;
}
void launch_fan_keys(hipStream_t st, const uint32_t *blocked_d, uint32_t lo, uint32_t cnt,
                     uint32_t P, unsigned long long *keys, unsigned long long identity) {
    hipLaunchKernelGGL(k_fan_keys, dim3((P + kT - 1) / kT), dim3(kT), 0, st, blocked_d, lo, cnt,
                       P, keys, identity);
}

// Every instantiated fan kernel, by what fan_pick() (pcp_fan_pick.hpp) answers (the fine-window
// kernels: DESIGN.md §5, 28 VGPRs, 8 waves per SIMD; the coarse layouts' kernel has no UE form)
using FanKernel = void (*)(FanArgs, uint32_t);
template <int M, int FN, bool UE>
constexpr FanKernel kFine = k_raycast_fan<M, 64, true, 8, FN, UE>;
struct FanRows { FanKernel k[4][2]; };
template <int M>
constexpr FanRows kRows = {{{k_raycast_fan<M>}, {kFine<M, 1, false>, kFine<M, 1, true>},
                            {kFine<M, 4, false>, kFine<M, 4, true>},
                            {kFine<M, 8, false>, kFine<M, 8, true>}}};
// k_raycast_fan by [MODE].k[FN 0 / 1 / 4 / 8][UE]
constexpr FanRows kFanInterleaved[3] = {kRows<FAN_PLAIN>, kRows<FAN_STATS>, kRows<FAN_STAMPS>};
// k_raycast_fan_xcd by [FN 1 / 4 / 8][log2 NPW]: several poses per wave over the tiled copies
template <int FN, int NPW>
constexpr FanKernel kXcd = k_raycast_fan_xcd<FAN_PLAIN, 64, true, 8, FN, true, NPW>;
constexpr FanKernel kFanXcd[3][6] = {
    {kXcd<1, 1>},   // (the untiled copy: one pose per wave only)
    {kXcd<4, 1>, kXcd<4, 2>, kXcd<4, 4>, kXcd<4, 8>, kXcd<4, 16>, kXcd<4, 32>},
    {kXcd<8, 1>, kXcd<8, 2>, kXcd<8, 4>, kXcd<8, 8>, kXcd<8, 16>, kXcd<8, 32>}};
// the split records' kernels with the default build's layout as compile-time facts (march, SP)
template <int NPW>
constexpr FanKernel kXcdSp = k_raycast_fan_xcd<FAN_PLAIN, 64, true, 8, 8, true, NPW, false, true>;
constexpr FanKernel kFanXcdSp[6] = {kXcdSp<1>, kXcdSp<2>,  kXcdSp<4>,
                                    kXcdSp<8>, kXcdSp<16>, kXcdSp<32>};
// the mounted forms (Plain only): the same two tables
template <int FN, bool UE>
constexpr FanKernel kFineMt = k_raycast_fan<FAN_PLAIN, 64, true, 8, FN, UE, true>;
constexpr FanRows kFanInterleavedMt = {{{k_raycast_fan<FAN_PLAIN, 64, true, 7, 0, false, true>},
                                        {kFineMt<1, false>, kFineMt<1, true>},
                                        {kFineMt<4, false>, kFineMt<4, true>},
                                        {kFineMt<8, false>, kFineMt<8, true>}}};
template <int FN, int NPW>
constexpr FanKernel kXcdMt = k_raycast_fan_xcd<FAN_PLAIN, 64, true, 8, FN, true, NPW, true>;
constexpr FanKernel kFanXcdMt[3][6] = {
    {kXcdMt<1, 1>},
    {kXcdMt<4, 1>, kXcdMt<4, 2>, kXcdMt<4, 4>, kXcdMt<4, 8>, kXcdMt<4, 16>, kXcdMt<4, 32>},
    {kXcdMt<8, 1>, kXcdMt<8, 2>, kXcdMt<8, 4>, kXcdMt<8, 8>, kXcdMt<8, 16>, kXcdMt<8, 32>}};

// The one fan launch, and its error.  ev0 / ev1: hipExtLaunchKernelGGL's start / stop events
// (null: none).  A pick without an instantiated kernel is an error.
static hipError_t fan_launch(const FanPick &k, FanGrid g, hipStream_t st, hipEvent_t ev0,
                             hipEvent_t ev1, const FanArgs &a, uint32_t P) {
    const int fn = k.FN == 8 ? 3 : k.FN == 4 ? 2 : k.FN;   // 0 / 1 / 4 / 8 -> 0 .. 3
    FanKernel f = nullptr;
    switch (k.family) {
    case FanFamily::Coarse:
    case FanFamily::Fine:
        if (k.mounted)
            f = k.mode == FanMode::Plain ? kFanInterleavedMt.k[fn][k.UE ? 1 : 0] : nullptr;
        else
            f = kFanInterleaved[(int)k.mode].k[fn][k.UE ? 1 : 0];
        break;
    case FanFamily::Xcd:   // (FAN_PLAIN only, over a fine copy)
        f = fn > 0 && k.mode == FanMode::Plain
                ? (k.mounted ? kFanXcdMt : kFanXcd)[fn - 1][__builtin_ctz(k.NPW)]
                : nullptr;
        // the default build's layout (PCP_FINE_PACK, PCP_FINE_SKIP=2, the pivot table, the
        // clearance codes): the kernel that knows it at compile time; any knob off keeps the
        // kernel that tests at run time (PCP_FAN_NO_SP: an A/B build that never picks it)
#ifndef PCP_FAN_NO_SP
        if (f && fn == 3 && !k.mounted && a.g.wpack && a.g.fskip == 2 && a.g.fpiv && a.g.fclear)
            f = kFanXcdSp[__builtin_ctz(k.NPW)];
#endif
        break;
    case FanFamily::PoseMajor: f = k.mounted ? nullptr : k_raycast_fan_pm<128, true>; break;
    case FanFamily::OccBit: f = k.mounted ? nullptr : k_raycast_fan<FAN_PLAIN, 64, false>; break;
    }
    if (!f) return hipErrorInvalidDeviceFunction;
    hipExtLaunchKernelGGL(f, dim3(g.x, g.y), dim3((uint32_t)k.block), 0, st, ev0, ev1, 0, a, P);
    return hipGetLastError();
}

// a mounted query's beam table: every entry finite (fan: checked non-null by the caller)
int fan_el_table_check(pcp_ctx *ctx, const char *what, const pcp_fan_params *fan,
                       const double *el_table) {
    if (!el_table) return PCP_OK;
    for (int32_t j = 0; j < fan->n_el; ++j)
        if (!std::isfinite(el_table[j]))
            return set_err(ctx, PCP_E_INVALID, "%s: el_table[%d] is not finite", what, (int)j);
    return PCP_OK;
}

// Everything of a fan query up to the per-pose sums, enqueued on ctx->stream (no host sync
// unless the fan tables or the step table change): poses uploaded through the pinned block,
// the march, k_fan_reduce.  On return o.blocked_d / o.units_d (and o.fh_d when opt.want_fh) are
// device results in flight; the caller synchronizes.  n > 0.
int fan_enqueue(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                FanEnq &o, FanMode mode, const FanOpts &opt) {
    if (fan->n_az <= 0 || fan->n_el <= 0 || (int64_t)fan->n_az * fan->n_el > (1ll << 30))
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: bad fan size %d x %d", fan->n_az,
                       fan->n_el);
    if (n > 65535) return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: at most 65535 poses per call");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int P = (int)n;
    const uint32_t rays = (uint32_t)fan->n_az * (uint32_t)fan->n_el;
    // direction tables (host libm, identical to the oracle), cached per fan shape
    const size_t tab_doubles = 2 * (size_t)fan->n_az + 2 * (size_t)fan->n_el;
    // (a beam table is part of the key: the cache holds the table it was built from, or none, so
    // a level call after a mounted one of the same shape rebuilds the uniform rings, and another
    // table its own)
    const double *elt = opt.mounted ? opt.el_table : nullptr;
    const bool same_rings =
        elt ? ctx->fan_el_h.size() == (size_t)fan->n_el &&
                  std::memcmp(ctx->fan_el_h.data(), elt, (size_t)fan->n_el * sizeof(double)) == 0
            : ctx->fan_el_h.empty() && ctx->fan_elmin == fan->el_min &&
                  ctx->fan_elmax == fan->el_max;
    if (ctx->fan_naz != fan->n_az || ctx->fan_nel != fan->n_el || !same_rings) {
        std::vector<double> t(tab_doubles);
        fan_tables(fan->n_az, fan->n_el, fan->el_min, fan->el_max, t.data(), t.data() + fan->n_az,
                   t.data() + 2 * fan->n_az, t.data() + 2 * fan->n_az + fan->n_el);
        if (elt)
            for (int32_t j = 0; j < fan->n_el; ++j) {
                t[2 * (size_t)fan->n_az + j] = std::cos(elt[j]);
                t[2 * (size_t)fan->n_az + fan->n_el + j] = std::sin(elt[j]);
            }
        ctx->fan_naz = -1;   // (no valid key while the upload can still fail)
        if (elt) ctx->fan_el_h.assign(elt, elt + fan->n_el);
        else ctx->fan_el_h.clear();
        PCP_HIP(ctx, ctx->fan_tab.ensure(tab_doubles * sizeof(double)));
        PCP_HIP(ctx, hipMemcpyAsync(ctx->fan_tab.p, t.data(), tab_doubles * sizeof(double),
                                    hipMemcpyHostToDevice, st));
        PCP_HIP(ctx, hipStreamSynchronize(st));
        ctx->fan_se_h.assign(t.begin() + 2 * (size_t)fan->n_az + fan->n_el, t.end());
        ctx->fan_naz = fan->n_az;
        ctx->fan_nel = fan->n_el;
        ctx->fan_elmin = fan->el_min;
        ctx->fan_elmax = fan->el_max;
    }
    int K = 0;
    int rc = ensure_steps(ctx, fan->max_distance - kVisRadius, &K);
    if (rc) return rc;
    // a keys query handed to a wait_stream may not have uploaded its poses yet: its copy reads
    // the pinned staging below, so that copy must be done before the staging is rewritten (or
    // regrown) by this query, whichever entry point enqueues it
    if (ctx->keys_pending) PCP_HIP(ctx, hipEventSynchronize(ctx->keys_ev));
    ctx->keys_pending = false;
    // pinned staging: poses in (P x kFanRow doubles; a mounted query: P x kFanDirRow), then {units
    // u64[P], blocked u32[P]} out
    const size_t row = opt.mounted ? (size_t)kFanDirRow : (size_t)kFanRow;
    PCP_HIP(ctx, ctx->fan_host.ensure((size_t)P * (row * sizeof(double) + 12) + 64));
    double *pose8 = ctx->fan_host.as<double>();
    for (int k = 0; k < P && opt.mounted; ++k)   // (poses6 rows)
        fan_dir_row(poses5 + 6 * (size_t)k, pose8 + row * (size_t)k);
    PCP_HIP(ctx, ctx->poses_d.ensure((size_t)P * row * sizeof(double)));
    const uint32_t waves = (rays + 63) / 64;
    if ((uint64_t)waves * (uint64_t)P >= (1ull << 31))
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: %d poses x %u rays exceed one launch",
                       P, rays);
    if (int rcb = terrain_blocks_before_query(ctx)) return rcb;
    FanArgs a{};
    a.present = ctx->terrain.present ? 1 : 0;
    if (a.present) {
        a.g = ctx->terrain.view(ctx->knob);
        if (!a.g.occz) return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: terrain index has no z bands");
        if (ctx->knob.fan_batch == 2 && !a.g.occ2)
            return set_err(ctx, PCP_E_STATE, "pcp_raycast_fan: variant 2 needs a terrain set with PCP_FAN_BATCH=2");
    }
    // the level rows (pcp_fan_row.hpp): the pose and, against this query's view, the march
    // preamble's pose-uniform floats (no terrain: a zero view, the march does not run)
    if (!opt.mounted) {
        const FanRowGrid rg{{a.g.fb[0], a.g.fb[1], a.g.fb[2], a.g.fb[3], a.g.fb[4], a.g.fb[5]},
                            {a.g.flo_x, a.g.flo_y, a.g.flo_z},
                            a.g.finv_c};
        for (int k = 0; k < P; ++k)
            fan_row_fill(poses5 + 5 * (size_t)k, rg, pose8 + row * (size_t)k);
    }
    a.uniform_el = (fan->n_az % 64 == 0) ? 1 : 0;
    // the kernel and whether it runs on the full grid: asked once, here (pcp_fan_pick.hpp)
    const FanPick pick = fan_pick(mode, ctx->knob.fan_batch, a.g.frec != nullptr, a.g.ftile,
                                  a.uniform_el != 0, P, K, ctx->knob.fan_npw, opt.burst > 0,
                                  opt.mounted);
    if (opt.mounted && mode != FanMode::Plain)
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan_mounted: no diagnostic modes");
    // Skip 4: each pose's live rings [j0, j1) into its eighth slot (the UE
    // kernels leave a pose's dead rings at once), and the waves that hold a live ring of some
    // pose: only those are launched, unless the pick needs the full grid.
    uint32_t w0 = 0, lw = waves;
    if (!opt.mounted) {   // (a mounted row has no live-ring slot: its kernels cover every ring)
        uint32_t *lr = reinterpret_cast<uint32_t *>(pose8) + kFanRowLiveU32;
        const bool rule = ctx->knob.fan_cull && ctx->terrain.present && K > 0;
        if (rule) {
            const FanLive L = fan_live_rings((double)a.g.fb[4], (double)a.g.fb[5], pose8 + FR_Z,
                                             (uint64_t)P, kFanRow, ctx->fan_se_h.data(), fan->n_el,
                                             ctx->steps_first, ctx->steps_last, lr,
                                             kFanRowStrideU32);
            if (!pick.full_grid) {
                const FanWaves W = fan_live_waves(L, fan->n_az, fan->n_el);
                w0 = W.w0;
                lw = W.w1 - W.w0;
            }
        } else {
            for (int k = 0; k < P; ++k) {
                lr[kFanRowStrideU32 * (size_t)k] = 0u;
                lr[kFanRowStrideU32 * (size_t)k + 1] = (uint32_t)fan->n_el;
            }
        }
    }
    PCP_HIP(ctx, ctx->out_c.ensure((size_t)P * (sizeof(uint32_t) + sizeof(uint64_t)) + 64));
    PCP_HIP(ctx, ctx->out_b.ensure(((size_t)P * waves + 8) * sizeof(uint2)));
    // stamps: 4 per wave; stats: 3 per wave + the 3 sums
    const size_t stats_bytes =
        mode == FanMode::Stamps  ? (size_t)P * waves * 4 * sizeof(uint64_t)
        : mode == FanMode::Stats ? ((size_t)P * waves * 4 + 4) * sizeof(uint64_t)
                                 : 64 * sizeof(uint64_t);
    PCP_HIP(ctx, ctx->stats_d.ensure(stats_bytes));
    if (int rc0 = copy_pinned_async(ctx, ctx->poses_d.p, pose8, (size_t)P * row * sizeof(double), st))
        return rc0;
    // results land in device memory, or (host_out) straight in the pinned block behind the
    // staged poses: one copy and its dispatch fewer per query
    unsigned long long *units_d =
        opt.host_out ? reinterpret_cast<unsigned long long *>(pose8 + row * (size_t)P)
                     : ctx->out_c.as<unsigned long long>();
    uint32_t *blocked_d = reinterpret_cast<uint32_t *>(units_d + P);
    int16_t *fh_d = nullptr;
    if (opt.want_fh) {
        PCP_HIP(ctx, ctx->out_d.ensure((size_t)P * rays * sizeof(int16_t)));
        fh_d = ctx->out_d.as<int16_t>();
    }
    const double *tab = ctx->fan_tab.as<const double>();
    a.ca = tab;
    a.sa = tab + fan->n_az;
    a.ce = tab + 2 * fan->n_az;
    a.se = tab + 2 * fan->n_az + fan->n_el;
    a.pose = ctx->poses_d.as<const double>();
    a.steps = ctx->steps_d.as<const double>();
    a.K = K;
    a.n_az = fan->n_az;
    a.rays = rays;
    a.waves = waves;
    a.w0 = w0;
    a.lw = lw;
    // the live rings nearest the horizon first: they are the far end of the interval when the
    // near end is the steeper one
    a.rev = (ctx->knob.fan_horizon_first && lw > 0 && lw < waves &&
             std::fabs(ctx->fan_se_h[std::min<size_t>((size_t)(w0 + lw - 1) * 64 / (size_t)fan->n_az,
                                                      (size_t)fan->n_el - 1)]) <
                 std::fabs(ctx->fan_se_h[(size_t)w0 * 64 / (size_t)fan->n_az]))
                ? 1 : 0;
    a.P = (uint32_t)P;
    a.r2 = (float)(kRayRadius * kRayRadius);
    a.rexit = exit_dist(a.r2);
    a.first_hit = fh_d;
    a.wave_part = ctx->out_b.as<uint2>();
    a.stats = ctx->stats_d.as<unsigned long long>();
    const FanGrid grid = fan_grid(lw, (uint32_t)P, rays, pick);
    if (mode != FanMode::Plain) {   // (the full grid: never empty)
        PCP_HIP(ctx, fan_launch(pick, grid, st, nullptr, nullptr, a, (uint32_t)P));
        const size_t nw = (size_t)P * waves;
        o.stats_d = mode == FanMode::Stats ? a.stats + 4 * nw : a.stats;
        if (mode == FanMode::Stats) {
            hipLaunchKernelGGL(k_sum_u64, dim3(4), dim3(1024), 0, st,
                               (const unsigned long long *)a.stats, nw, a.stats + 4 * nw);
            PCP_CHECK_LAUNCH(ctx);
        }
    } else if (grid.x == 0) {
        // every ring is dead for every pose: no march (a zero-sized grid is not submitted);
        // k_fan_reduce below gives the closed-form result
        if (opt.burst_ms) *opt.burst_ms = 0.0;
    } else if (opt.burst > 0) {
        // the production kernel `burst` times back-to-back between two events: the queue never
        // idles between the events, so the interval is the launches themselves (the per-call
        // events of a synchronous query also hold the queue's wake-up before the kernel)
        auto launch = [&]() -> int {
            PCP_HIP(ctx, fan_launch(pick, grid, st, nullptr, nullptr, a, (uint32_t)P));
            return PCP_OK;
        };
        double ms = 0.0;   // (an empty warm-up: the burst's launches are the query's only ones)
        if (int rcb = time_reps(ctx, "pcp_raycast_fan_burst", st, opt.burst,
                                [] { return PCP_OK; }, launch, &ms))
            return rcb;
        if (opt.burst_ms) *opt.burst_ms = ms;
    } else {
        KernelTimer kt(ctx, PCP_K_RAYCAST_FAN);   // events around the kernel itself
        PCP_HIP(ctx, fan_launch(pick, grid, st, kt.a, kt.b, a, (uint32_t)P));
    }
    // the rays the launch covered: [r_lo, r_hi) of each pose
    const uint32_t r_lo = w0 * 64u, r_hi = std::min<uint64_t>((uint64_t)(w0 + lw) * 64u, rays);
    hipLaunchKernelGGL(k_fan_reduce, dim3(P), dim3(kT), 0, st,
                       (const uint2 *)a.wave_part, lw, blocked_d,
                       units_d, o.keys, o.keys_lo, o.keys_P,
                       (unsigned long long)(rays - (r_hi - r_lo)) * (unsigned long long)K, fh_d,
                       rays, r_lo, r_hi);
    PCP_CHECK_LAUNCH(ctx);
    o.blocked_d = opt.host_out ? nullptr : blocked_d;
    o.units_d = opt.host_out ? nullptr : units_d;
    o.fh_d = fh_d;
    o.rays = rays;
    o.stats_bytes = stats_bytes;
    o.wave_part = a.wave_part;
    o.waves = waves;
    o.wave0 = w0;
    o.live_waves = lw;
    o.K = K;
    o.pose_row = (uint32_t)row;
    o.mounted = opt.mounted;
    return PCP_OK;
}
}  // namespace pcp

using namespace pcp;

extern "C" {

static int raycast_fan_impl(pcp_ctx *ctx, const double *poses5, uint64_t n,
                            const pcp_fan_params *fan, uint32_t *blocked, uint64_t *units,
                            int16_t *first_hit, int64_t *best_idx,
                            FanMode mode = FanMode::Plain, uint64_t *diag = nullptr,
                            int burst = 0, double *burst_ms = nullptr, bool mounted = false,
                            const double *el_table = nullptr) {
    if (!ctx) return PCP_E_INVALID;
    if (!fan || (n && (!poses5 || !blocked)))
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: null argument");
    if (int rc = fan_el_table_check(ctx, "pcp_raycast_fan_mounted", fan, el_table)) return rc;
    if (best_idx) *best_idx = -1;
    if (n == 0) {
        if (fan->n_az <= 0 || fan->n_el <= 0 || (int64_t)fan->n_az * fan->n_el > (1ll << 30))
            return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan: bad fan size %d x %d",
                           fan->n_az, fan->n_el);
        return PCP_OK;
    }
    FanEnq o;   // (the kernel and its poses per wave: pcp_fan_pick.hpp, mirrored by bench._fan_npw)
    const bool host_out = ctx->knob.fan_host_out;
    if (int rc = fan_enqueue(ctx, poses5, n, fan, o, mode,
                             FanOpts{first_hit != nullptr, burst, burst_ms, host_out, mounted,
                                     el_table}))
        return rc;
    hipStream_t st = ctx->stream;
    const int P = (int)n;
    const uint32_t rays = o.rays;
    if (diag)   // the four sums, or every wave's stamps
        PCP_HIP(ctx, hipMemcpyAsync(diag, o.stats_d,
                                    mode == FanMode::Stats ? 4 * sizeof(uint64_t) : o.stats_bytes,
                                    hipMemcpyDeviceToHost, st));
    // units and blocked are adjacent on the device: one copy into the pinned block
    double *pose8 = ctx->fan_host.as<double>();
    uint64_t *u_h = reinterpret_cast<uint64_t *>(pose8 + (size_t)o.pose_row * (size_t)P);
    const uint32_t *b_h = reinterpret_cast<const uint32_t *>(u_h + P);
    if (!host_out)   // else k_fan_reduce stored them into u_h / b_h itself
        PCP_HIP(ctx, hipMemcpyAsync(u_h, o.units_d, (size_t)P * 12, hipMemcpyDeviceToHost, st));
    if (first_hit)
        PCP_HIP(ctx, hipMemcpyAsync(first_hit, o.fh_d, (size_t)P * rays * sizeof(int16_t),
                                    hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipStreamSynchronize(st));
    prof_resolve(ctx);
    std::memcpy(blocked, b_h, (size_t)P * sizeof(uint32_t));
    if (units)
        for (int k = 0; k < P; ++k) units[k] = u_h[k];
    if (best_idx) {
        int64_t b = 0;
        for (int k = 1; k < P; ++k)
            if (blocked[k] < blocked[b]) b = k;
        *best_idx = b;
    }
    return PCP_OK;
}

int pcp_raycast_fan(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                    uint32_t *blocked, uint64_t *units, int16_t *first_hit, int64_t *best_idx) {
    return raycast_fan_impl(ctx, poses5, n, fan, blocked, units, first_hit, best_idx);
}

int pcp_raycast_fan_stats(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const pcp_fan_params *fan, uint64_t stats[4]) {
    if (!ctx || !stats) return PCP_E_INVALID;
    std::vector<uint32_t> blocked(n ? n : 1);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    return raycast_fan_impl(ctx, poses5, n, fan, blocked.data(), nullptr, nullptr, nullptr,
                            FanMode::Stats, stats);
}

int pcp_raycast_fan_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const pcp_fan_params *fan, int reps, double *ms_per_launch) {
    if (!ctx || !ms_per_launch || reps <= 0) return PCP_E_INVALID;
    std::vector<uint32_t> blocked(n ? n : 1);
    *ms_per_launch = 0.0;
    return raycast_fan_impl(ctx, poses5, n, fan, blocked.data(), nullptr, nullptr, nullptr,
                            FanMode::Plain, nullptr, reps, ms_per_launch);
}

int pcp_raycast_fan_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                            const pcp_fan_params *fan, const double *el_table, uint32_t *blocked,
                            uint64_t *units, int16_t *first_hit, int64_t *best_idx) {
    return raycast_fan_impl(ctx, poses6, n, fan, blocked, units, first_hit, best_idx,
                            FanMode::Plain, nullptr, 0, nullptr, true, el_table);
}

int pcp_raycast_fan_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                  const pcp_fan_params *fan, const double *el_table, int reps,
                                  double *ms_per_launch) {
    if (!ctx || !ms_per_launch || reps <= 0) return PCP_E_INVALID;
    std::vector<uint32_t> blocked(n ? n : 1);
    *ms_per_launch = 0.0;
    return raycast_fan_impl(ctx, poses6, n, fan, blocked.data(), nullptr, nullptr, nullptr,
                            FanMode::Plain, nullptr, reps, ms_per_launch, true, el_table);
}

int pcp_raycast_fan_stamps(pcp_ctx *ctx, const double *poses5, uint64_t n,
                           const pcp_fan_params *fan, uint64_t *stamps) {
    if (!ctx || !stamps) return PCP_E_INVALID;
    std::vector<uint32_t> blocked(n ? n : 1);
    return raycast_fan_impl(ctx, poses5, n, fan, blocked.data(), nullptr, nullptr, nullptr,
                            FanMode::Stamps, stamps);
}

// one rank's shard of a pose-sharded fan query whose collective the caller runs (one process
// per GPU, torch.distributed over RCCL): keys stay on the device, in the caller's buffer
int pcp_raycast_fan_keys(pcp_ctx *ctx, const double *poses5, uint64_t n,
                         const pcp_fan_params *fan, uint64_t lo, uint64_t p_total,
                         int64_t *keys_dev, uint64_t *units_dev, void *wait_stream) {
    if (!ctx) return PCP_E_INVALID;
    if (!fan || !keys_dev || (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan_keys: null argument");
    if (lo + n > p_total || p_total > 65535u * 64u)
        return set_err(ctx, PCP_E_INVALID, "pcp_raycast_fan_keys: shard [%llu, %llu) of %llu poses",
                       (unsigned long long)lo, (unsigned long long)(lo + n),
                       (unsigned long long)p_total);
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // (fan_enqueue waits for a previous keys query's pose upload before it rewrites the
    // pinned staging; an n == 0 shard touches no staging)
    const uint32_t *blocked_d = nullptr;
    if (n) {
        FanEnq o;
        if (int rc = fan_enqueue(ctx, poses5, n, fan, o)) return rc;
        blocked_d = o.blocked_d;
        if (units_dev)
            PCP_HIP(ctx, hipMemcpyAsync(units_dev, o.units_d, n * sizeof(uint64_t),
                                        hipMemcpyDeviceToDevice, st));
    }
    launch_fan_keys(st, blocked_d, (uint32_t)lo, (uint32_t)n, (uint32_t)p_total,
                    reinterpret_cast<unsigned long long *>(keys_dev), 0x7fffffffffffffffull);
    PCP_CHECK_LAUNCH(ctx);
    if (!ctx->keys_ev) PCP_HIP(ctx, hipEventCreateWithFlags(&ctx->keys_ev, hipEventDisableTiming));
    PCP_HIP(ctx, hipEventRecord(ctx->keys_ev, st));
    if (wait_stream) {
        PCP_HIP(ctx, hipStreamWaitEvent(static_cast<hipStream_t>(wait_stream), ctx->keys_ev, 0));
        ctx->keys_pending = true;
    } else {
        PCP_HIP(ctx, hipEventSynchronize(ctx->keys_ev));
    }
    return PCP_OK;
}

}  // extern "C"
