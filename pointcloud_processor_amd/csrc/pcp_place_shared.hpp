// What the placement calls share (pcp_place_sensors, pcp_place_pair, pcp_place_refine,
// pcp_place_triple: pcp_place.hip, pcp_pairs.hip, pcp_refine.hip, pcp_triples.hip; DESIGN.md
// §6h/§6i/§6k): the first-maximum order, the
// ordered walk of a staged chunk, the last-block ticket, the one-lane ordered total, the fold with
// owners, the separation test and the front of the calls' blocks (the timing entries' scaffold,
// time_reps, is pcp_internal.hpp's: the scoring and the fan time their bursts with it too).
// The first part is plain C++ (no HIP dependency): tests/native/place_shared_selftest.cpp builds
// it with the host compiler.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PCP_PS_HD __host__ __device__
#else
#define PCP_PS_HD
#endif

namespace pcp {

// a candidate of a first-maximum search in row-major order: total t of row (a, b); a < 0: none
struct RowBest {
    double t;
    int32_t a, b;
};
static_assert(sizeof(RowBest) == 16, "two 8-byte words");

// (t2, a2, b2) ahead of (t1, a1, b1): a larger total, or the same and earlier in row-major order
PCP_PS_HD inline bool best_ahead(double t2, int a2, int b2, double t1, int a1, int b1) {
    return a2 >= 0 && (a1 < 0 || t2 > t1 || (t2 == t1 && (a2 < a1 || (a2 == a1 && b2 < b1))));
}

// the ordered walk (walk_chunk): the pair tiles and the exchange evaluation stage chunks of kWalkC
// cells per row in LDS, rows kWalkLd apart
constexpr int kWalkC = 64;           // cells per staged chunk
constexpr int kWalkLd = kWalkC + 2;  // a staged row: 16 rows of b128 reads fall on 16 x 4 banks
constexpr int kWalkG = 4;            // b128 reads per row per register group
static_assert((kWalkC / 2) % (2 * kWalkG) == 0 && kWalkLd % 2 == 0, "whole group pairs per chunk");

PCP_PS_HD inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
PCP_PS_HD inline double sep2_of(double sep) { return sep > 0 ? sep * sep : 0.0; }

// the front of a call's block, device and pinned alike: [state | cell_score f64 C | cell_owner
// i32 C | rest ..], every part on a 16-byte boundary
struct CellBlock {
    size_t score_off, owner_off, rest_off;
};
inline CellBlock cell_block(size_t state_bytes, int C) {
    CellBlock b;
    b.score_off = a16(state_bytes);
    b.owner_off = a16(b.score_off + (size_t)C * sizeof(double));
    b.rest_off = a16(b.owner_off + (size_t)C * sizeof(int32_t));
    return b;
}
inline void copy_cells(const char *pin, const CellBlock &b, int C, double *cell_score,
                       int32_t *cell_owner) {
    if (cell_score) std::memcpy(cell_score, pin + b.score_off, (size_t)C * sizeof(double));
    if (cell_owner) std::memcpy(cell_owner, pin + b.owner_off, (size_t)C * sizeof(int32_t));
}

// a list of `count` distinct poses of n: 0, or what is wrong with entry *bad (the first such)
enum { kListOk = 0, kListRange = 1, kListTwice = 2 };
inline int check_index_list(const int64_t *list, int count, uint64_t n, int *bad) {
    for (int i = 0; i < count; ++i) {
        *bad = i;
        if (list[i] < 0 || (uint64_t)list[i] >= n) return kListRange;
        for (int j = 0; j < i; ++j)
            if (list[j] == list[i]) return kListTwice;
    }
    return kListOk;
}

}  // namespace pcp

#if defined(__HIPCC__)
#include "pcp_internal.hpp"

namespace pcp {

// the larger of two values that are finite, not NaN and never -0.0 (the clamped rows'): one
// instruction, and for equal values their common bits -- the reference's std::max on these inputs
__device__ __forceinline__ double max_pos(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// One chunk of a lane's chain: acc += max(va[c], vb[c]) over the kWalkC cells of its two staged
// rows in ascending order.  Two register groups of kWalkG b128 reads per row: the adds of one
// group run while the other's reads are in flight (one wave per SIMD: nothing else hides the LDS
// latency; the scheduling barriers keep each group's reads ahead of the adds before it).
// k_refine_eval calls it; k_pair_tiles holds the same text in place (the reason stands there).
__device__ __forceinline__ void walk_chunk(const double2 *va, const double2 *vb, double &acc) {
    double2 a0[kWalkG], b0[kWalkG], a1[kWalkG], b1[kWalkG];
    auto rd = [&](double2 *a, double2 *b, int j) {
#pragma unroll
        for (int i = 0; i < kWalkG; ++i) {
            a[i] = va[j + i];
            b[i] = vb[j + i];
        }
    };
    auto add = [&](const double2 *a, const double2 *b) {
#pragma unroll
        for (int i = 0; i < kWalkG; ++i) {
            acc += max_pos(a[i].x, b[i].x);
            acc += max_pos(a[i].y, b[i].y);
        }
    };
    rd(a0, b0, 0);
#pragma unroll
    for (int j = 0; j < kWalkC / 2; j += 2 * kWalkG) {
        rd(a1, b1, j + kWalkG);
        __builtin_amdgcn_sched_barrier(0);
        add(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (j + 2 * kWalkG < kWalkC / 2) rd(a0, b0, j + 2 * kWalkG);
        __builtin_amdgcn_sched_barrier(0);
        add(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the first maximum of a block of W waves: (t, a, b) becomes the earlier of itself and (t2, a2, b2)
__device__ __forceinline__ void take_ahead(double &t, int &a, int &b, double t2, int a2, int b2) {
    if (best_ahead(t2, a2, b2, t, a, b)) {
        t = t2;
        a = a2;
        b = b2;
    }
}
// a wave's candidates by shuffles, the waves' through s_best[W]: the block's best in thread 0
template <int W>
__device__ __forceinline__ void block_first_max(RowBest *s_best, double &t, int &a, int &b) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        take_ahead(t, a, b, __shfl_xor(t, o, 64), __shfl_xor(a, o, 64), __shfl_xor(b, o, 64));
    if ((tid & 63) == 0) s_best[tid >> 6] = RowBest{t, a, b};
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < W; ++w) take_ahead(t, a, b, s_best[w].t, s_best[w].a, s_best[w].b);
}
// the same with the block's best in every thread; s_best may have readers of an earlier use
template <int W>
__device__ __forceinline__ void block_first_max_all(RowBest *s_best, double &t, int &a, int &b) {
    __syncthreads();
    block_first_max<1>(s_best, t, a, b);
    t = s_best[0].t;
    a = s_best[0].a;
    b = s_best[0].b;
    for (int w = 1; w < W; ++w) take_ahead(t, a, b, s_best[w].t, s_best[w].a, s_best[w].b);
}

// The last-block ticket.  Every block of a launch calls this after its last store of what the
// launch's last block reads: those stores are released to the device before the draw, and the
// block that draws the last ticket (true in all its threads) acquires the others' after it.  That
// block resets *ticket before it ends; the next launch draws from zero.
__device__ __forceinline__ bool last_block(uint32_t *ticket, int &s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t =
            __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_flag = t == gridDim.x - 1;
        if (s_flag) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return s_flag != 0;
}

// One block of T threads: the ordered sum of the positive value_of_cell(c), c = 0 .. C - 1, as one
// chain of thread 0 (returned there; the other threads stage and count, +0.0 is bit-neutral), and
// the number of positive cells in s_cnt.
template <int T, class F>
__device__ __forceinline__ double ordered_total(F value_of_cell, int C, double *s_b,
                                                int32_t &s_cnt) {
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;
    double acc = 0.0;
    int32_t cnt = 0;
    for (int c0 = 0; c0 < C; c0 += T) {
        __syncthreads();
        const double b = c0 + tid < C ? value_of_cell(c0 + tid) : 0.0;
        const bool pos = b > 0;
        cnt += pos ? 1 : 0;
        s_b[tid] = pos ? b : 0.0;
        __syncthreads();
        if (tid == 0) {
#pragma unroll 16
            for (int i = 0; i < T; ++i) acc += s_b[i];
        }
    }
    __syncthreads();
    atomicAdd(&s_cnt, cnt);
    __syncthreads();
    return acc;
}

// std::max(b, v) with the owner: sensor i takes the cell when it raises it; ties keep the earlier
__device__ __forceinline__ bool fold_owner(double &b, int32_t &own, double v, int32_t i) {
    if (!(b < v)) return false;
    b = v;
    own = i;
    return true;
}
// a cell's fold from zx120's score z
__device__ __forceinline__ int32_t owner_of_zx(double z) {
    return z > 0 ? PCP_OWNER_ZX120 : PCP_OWNER_NONE;
}

// poses a and b are closer than the separation in XY; a loop over b loads (ax, ay) once
__device__ __forceinline__ bool closer_than(double ax, double ay,
                                            const double *__restrict__ poses5, int b, double sep2) {
    const double dx = ax - poses5[5 * (size_t)b], dy = ay - poses5[5 * (size_t)b + 1];
    return dx * dx + dy * dy < sep2;
}
__device__ __forceinline__ bool closer_than(const double *__restrict__ poses5, int a, int b,
                                            double sep2) {
    return closer_than(poses5[5 * (size_t)a], poses5[5 * (size_t)a + 1], poses5, b, sep2);
}

// ---- host ---------------------------------------------------------------------------------

// the end of a call's work on the stream
inline int stream_done(pcp_ctx *ctx) {
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return PCP_OK;
}

// at most PCP_PAIR_MAX_POSES poses, and `list` (the caller's `name`, "pose f is `twice` twice")
// holds `count` distinct ones: into idx as the kernels take them
inline int check_pose_list(pcp_ctx *ctx, const char *what, const char *name, const char *twice,
                           const int64_t *list, int count, uint64_t n, int32_t *idx) {
    if (n > PCP_PAIR_MAX_POSES)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses, at most %d per call", what,
                       (unsigned long long)n, PCP_PAIR_MAX_POSES);
    int i = 0;
    const int bad = check_index_list(list, count, n, &i);
    if (bad == kListRange)
        return set_err(ctx, PCP_E_INVALID, "%s: %s[%d] = %lld is no pose of %llu", what, name, i,
                       (long long)list[i], (unsigned long long)n);
    if (bad == kListTwice)
        return set_err(ctx, PCP_E_INVALID, "%s: pose %lld is %s twice", what, (long long)list[i],
                       twice);
    for (i = 0; i < count; ++i) idx[i] = (int32_t)list[i];
    return PCP_OK;
}

}  // namespace pcp
#endif
