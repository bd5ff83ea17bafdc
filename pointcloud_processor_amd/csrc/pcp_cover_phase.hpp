// The build phase of the coverage placements: the call's plan and argument
// checks, k_cover_clear, k_cover_need, k_cover_resolve, k_cover_count and k_cover_commit with their
// enqueue functions, as pcp_cover.hip held them.  pcp_place_coverage (pcp_cover.hip) runs its greedy
// rounds behind it in ctx->cover_d; pcp_place_coverage_pair (pcp_cover_pair.hip) runs its mask, tile
// and selection passes behind it in a block of its own, and pcp_place_coverage_refine
// (pcp_cover_refine.hip) its preparations and evaluations in a third.  The unnamed
// namespace gives each of the translation units its own copy of the kernels.
#pragma once

#include <algorithm>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_place_shared.hpp"
#include "pcp_scan_hit.hpp"

namespace pcp {
namespace {

constexpr int kCT = 256;             // threads per block: four waves
constexpr int kCW = kCT / 64;
constexpr uint32_t kCntBlock = kCT * 2 * 4;    // words per block of the row counts

// the call's device state: control words of the rounds and the selection record (downloaded)
struct CoverState {
    int32_t n_sel;              // rounds recorded
    int32_t done;               // a round stopped: the later launches return at once
    uint32_t ticket;            // blocks of the current round that have finished
    uint32_t pad;
    unsigned long long roi_points;     // |R|
    unsigned long long base_covered;   // points of R the fixed sensors reach
    int64_t sel[PCP_PLACE_MAX];
    unsigned long long gain[PCP_PLACE_MAX];
    unsigned long long cov_after[PCP_PLACE_MAX];
};
static_assert(sizeof(CoverState) % 16 == 0, "the counts follow on a 16-byte boundary");

struct CoverFixed {
    int32_t n;
    int32_t idx[PCP_PLACE_MAX];
};

// pose a is closer than the separation to pose b in XY: pcp_place_sensors' expression
// (closer_than, pcp_place_shared.hpp) on columns 0 and 1 of the staged pose rows
__device__ __forceinline__ bool cover_closer(const double *__restrict__ pose, uint32_t row, int a,
                                             int b, double sep2) {
    const double dx = pose[(size_t)row * a] - pose[(size_t)row * b];
    const double dy = pose[(size_t)row * a + 1] - pose[(size_t)row * b + 1];
    return dx * dx + dy * dy < sep2;
}

// The call's first launch: the bitsets, the gains table and the counts cleared, the state reset,
// and every pose alive unless it is fixed or closer than the separation to a fixed pose.
__global__ void __launch_bounds__(kCT)
k_cover_clear(ulonglong2 *__restrict__ seen2, unsigned long long n_seen2,
              long long *__restrict__ rg, unsigned long long n_rg,
              uint32_t *__restrict__ seen_pts, uint32_t *__restrict__ alive, int n,
              CoverState *__restrict__ s, const double *__restrict__ pose, uint32_t row,
              CoverFixed fx, double sep2) {
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kCT + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kCT;
    for (unsigned long long i = t0; i < n_seen2; i += stride) seen2[i] = make_ulonglong2(0ull, 0ull);
    for (unsigned long long i = t0; i < n_rg; i += stride) rg[i] = 0ll;
    for (unsigned long long i = t0; i < (unsigned long long)n; i += stride) {
        const int p = (int)i;
        bool a = true;
        for (int f = 0; f < fx.n; ++f)
            if (p == fx.idx[f] || (sep2 > 0 && cover_closer(pose, row, p, fx.idx[f], sep2))) a = false;
        alive[p] = a ? 1u : 0u;
        seen_pts[p] = 0u;
    }
    if (t0 == 0) {
        s->n_sel = 0;
        s->done = 0;
        s->ticket = 0u;
        s->pad = 0u;
        s->roi_points = 0ull;
        s->base_covered = 0ull;
    }
}

// need = R as bits, one wave per word by ballot (roi null: every point below N), |R| counted, and
// every owner PCP_OWNER_NONE.  The words past ceil(N / 64) (the padding to an even count) are zero.
__global__ void __launch_bounds__(kCT)
k_cover_need(const uint8_t *__restrict__ roi, unsigned long long N, uint32_t W2,
             unsigned long long *__restrict__ need, int32_t *__restrict__ owner,
             CoverState *__restrict__ s) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    const unsigned long long i = (unsigned long long)gw * 64u + lane;
    const bool in = gw < W2 && i < N;
    const bool bit = in && (roi ? roi[i] != 0 : true);
    const uint64_t bal = __ballot(bit);
    if (in && owner) owner[i] = PCP_OWNER_NONE;
    if (lane == 0 && gw < W2) {
        need[gw] = bal;
        if (bal) atomicAdd(&s_cnt, (uint32_t)__popcll(bal));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&s->roi_points, (unsigned long long)s_cnt);
}

// One lane per ray in the fan's wave-to-ray mapping, over the live waves [w0, w0 + lw) of every
// pose only (a culled wave has no blocked ray).  A blocked lane finds its hit point by the scan's
// search and ORs one bit into its pose's bitset, with k_scan_resolve's neighbour-lane suppression:
// of a run of neighbouring lanes on one point only the first issues the atomic.
// MT: a mounted query (pcp_fan_dir.hpp's rows and direction).
template <bool MT>
__global__ void __launch_bounds__(kCT)
k_cover_resolve(ScanHitQuery q, const int16_t *__restrict__ first_hit, uint32_t rays, uint32_t w0,
                uint32_t lw, uint32_t P, unsigned long long *__restrict__ seen, uint32_t W2,
                unsigned long long N) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    if (gw >= P * lw) return;   // (whole waves)
    const uint32_t p = gw / lw, w = w0 + (gw - p * lw);
    const uint32_t ray = w * 64u + lane;
    const bool active = ray < rays;
    const int k = active ? (int)first_hit[(size_t)p * rays + ray] : -1;
    const bool hit = k >= 0;
    const uint64_t bal = __ballot(hit);
    if (!hit) return;
    const ScanHit h = scan_hit<MT>(q, p, ray, k);
    const uint32_t bidx = h.idx;
    const uint32_t prev = (uint32_t)__shfl_up((int)bidx, 1, 64);
    const bool dup = lane > 0 && ((bal >> (lane - 1)) & 1ull) && prev == bidx;
    // (bidx < N <= 64 W2: inside the pose's row; ~0, no point within r, sets nothing)
    if (!dup && (unsigned long long)bidx < N)
        atomicOr(&seen[(size_t)p * W2 + (bidx >> 6)], 1ull << (bidx & 63u));
}

// seen_points[p] = |seen(p)|: blockIdx.y = the pose, blockIdx.x = a chunk of kCntBlock words
__global__ void __launch_bounds__(kCT)
k_cover_count(const unsigned long long *__restrict__ seen, uint32_t W2,
              uint32_t *__restrict__ seen_pts) {
    const uint32_t p = blockIdx.y;
    const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(seen + (size_t)p * W2);
    const uint32_t n2 = W2 / 2;
    const uint32_t lo = blockIdx.x * (kCntBlock / 2);
    const uint32_t hi = min(n2, lo + kCntBlock / 2);
    uint32_t cnt = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kCT) {
        const ulonglong2 v = row[i];
        cnt += (uint32_t)(__popcll(v.x) + __popcll(v.y));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&seen_pts[p], cnt);
}

// The commit of one sensor: the points of seen(b) still in need get the owner and leave need.  One
// wave per word (the only writer of that word and of its 64 owners), lane i = bit i.
// b_fixed >= 0: a fixed sensor, its points counted into base_covered; otherwise round r's record,
// and a return at once when that round recorded nothing.
__global__ void __launch_bounds__(kCT)
k_cover_commit(const unsigned long long *__restrict__ seen, unsigned long long *need, uint32_t W2,
               int32_t *__restrict__ owner, CoverState *s, int b_fixed, int32_t owner_id, int r) {
    __shared__ uint32_t s_cnt;
    const int b = b_fixed >= 0 ? b_fixed : (s->n_sel > r ? (int)s->sel[r] : -1);
    if (b < 0) return;   // (uniform)
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    if (gw < W2) {
        const unsigned long long nd = need[gw];
        const unsigned long long m = seen[(size_t)b * W2 + gw] & nd;
        if (m) {   // (wave-uniform)
            if (owner && ((m >> lane) & 1ull)) owner[(size_t)gw * 64u + lane] = owner_id;
            if (lane == 0) {
                need[gw] = nd & ~m;
                if (b_fixed >= 0) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
            }
        }
    }
    if (b_fixed < 0) return;
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&s->base_covered, (unsigned long long)s_cnt);
}

// the call's device block: [state | seen_points u32 n | gains i64 K x n | alive u32 n | need u64 W2
// | seen u64 n x W2 | owner i32 N | roi bytes N]; the download is [state .. gains) or [.. alive)
struct CoverPlan {
    int n = 0, K = 0;
    uint64_t N = 0;
    uint32_t W2 = 0;
    bool owner = false, roi = false;
    size_t sp_off = 0, rg_off = 0, al_off = 0, need_off = 0, seen_off = 0, own_off = 0, roi_off = 0,
           bytes = 0;
};

CoverPlan make_plan(int n, int K, uint64_t N, bool owner, bool roi) {
    CoverPlan c;
    c.n = n;
    c.K = K;
    c.N = N;
    c.W2 = (uint32_t)(((N + 63) / 64 + 1) & ~(uint64_t)1);
    c.owner = owner;
    c.roi = roi;
    c.sp_off = a16(sizeof(CoverState));
    c.rg_off = a16(c.sp_off + (size_t)n * sizeof(uint32_t));
    c.al_off = a16(c.rg_off + (size_t)K * n * sizeof(int64_t));
    c.need_off = a16(c.al_off + (size_t)n * sizeof(uint32_t));
    c.seen_off = c.need_off + (size_t)c.W2 * sizeof(uint64_t);
    c.own_off = a16(c.seen_off + (size_t)n * c.W2 * sizeof(uint64_t));
    c.roi_off = a16(c.own_off + (owner ? (size_t)N * sizeof(int32_t) : 0));
    c.bytes = c.roi_off + (roi ? (size_t)N : 0) + 64;
    return c;
}

struct CoverDev {
    CoverState *s;
    uint32_t *seen_pts, *alive;
    long long *rg;
    unsigned long long *need, *seen;
    int32_t *owner;
    uint8_t *roi;
};

// the parts of the plan in the call's device block blk
CoverDev dev_of(char *blk, const CoverPlan &c) {
    CoverDev d;
    d.s = reinterpret_cast<CoverState *>(blk);
    d.seen_pts = reinterpret_cast<uint32_t *>(blk + c.sp_off);
    d.rg = reinterpret_cast<long long *>(blk + c.rg_off);
    d.alive = reinterpret_cast<uint32_t *>(blk + c.al_off);
    d.need = reinterpret_cast<unsigned long long *>(blk + c.need_off);
    d.seen = reinterpret_cast<unsigned long long *>(blk + c.seen_off);
    d.owner = c.owner ? reinterpret_cast<int32_t *>(blk + c.own_off) : nullptr;
    d.roi = c.roi ? reinterpret_cast<uint8_t *>(blk + c.roi_off) : nullptr;
    return d;
}

// the bitsets' phase on ctx->stream, behind the fan: clear, need, resolve, counts
int build_enqueue(pcp_ctx *ctx, const CoverPlan &c, const CoverDev &d, const pcp_fan_params *fan,
                  const FanEnq &o, const CoverFixed &fx, double sep2) {
    hipStream_t st = ctx->stream;
    const double *pose = ctx->poses_d.as<const double>();
    {
        const unsigned long long n2 = (unsigned long long)c.n * c.W2 / 2;
        const unsigned g = (unsigned)std::min<uint64_t>((n2 + kCT - 1) / kCT + 1, 4096);
        hipLaunchKernelGGL(k_cover_clear, dim3(g), dim3(kCT), 0, st,
                           reinterpret_cast<ulonglong2 *>(d.seen), n2, d.rg,
                           (unsigned long long)c.K * c.n, d.seen_pts, d.alive, c.n, d.s, pose,
                           o.pose_row, fx, sep2);
        PCP_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(k_cover_need, dim3((c.W2 + kCW - 1) / kCW), dim3(kCT), 0, st,
                       (const uint8_t *)d.roi, (unsigned long long)c.N, c.W2, d.need, d.owner, d.s);
    PCP_CHECK_LAUNCH(ctx);
    const uint32_t nW = (uint32_t)c.n * o.live_waves;
    if (nW) {
        const ScanHitQuery q = scan_hit_query(ctx, fan);
        hipLaunchKernelGGL(o.mounted ? k_cover_resolve<true> : k_cover_resolve<false>,
                           dim3((nW + kCW - 1) / kCW), dim3(kCT), 0, st, q,
                           (const int16_t *)o.fh_d, o.rays, o.wave0, o.live_waves, (uint32_t)c.n,
                           d.seen, c.W2, (unsigned long long)c.N);
        PCP_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_cover_count, dim3((c.W2 + kCntBlock - 1) / kCntBlock, (unsigned)c.n),
                           dim3(kCT), 0, st, (const unsigned long long *)d.seen, c.W2, d.seen_pts);
        PCP_CHECK_LAUNCH(ctx);
    }
    return PCP_OK;
}

int commit_enqueue(pcp_ctx *ctx, const CoverPlan &c, const CoverDev &d, int b_fixed, int owner_id,
                   int r) {
    hipLaunchKernelGGL(k_cover_commit, dim3((c.W2 + kCW - 1) / kCW), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, d.need, c.W2, d.owner, d.s, b_fixed,
                       (int32_t)owner_id, r);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what is refused before any launch (ctx non-null); *N_out = N
int check_args(pcp_ctx *ctx, const char *what, const double *poses, uint64_t n,
               const pcp_fan_params *fan, bool mounted, const double *el_table,
               const pcp_cover_params *cp, const uint8_t *roi, uint64_t roi_n, CoverFixed &fx,
               uint64_t *N_out) {
    if (!fan || !cp || (n && !poses)) return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    if (fan->n_az <= 0 || fan->n_el <= 0 || (int64_t)fan->n_az * fan->n_el > (1ll << 30))
        return set_err(ctx, PCP_E_INVALID, "%s: bad fan size %d x %d", what, fan->n_az, fan->n_el);
    if (int rc = steps_within_bound(ctx, fan->max_distance - kVisRadius)) return rc;
    if (mounted)
        if (int rc = fan_el_table_check(ctx, what, fan, el_table)) return rc;
    if (n > PCP_COVER_MAX_POSES)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses, at most %d per call", what,
                       (unsigned long long)n, PCP_COVER_MAX_POSES);
    if (n * (uint64_t)fan->n_az * (uint64_t)fan->n_el > (1ull << 31))
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses x %d x %d rays exceed 2^31", what,
                       (unsigned long long)n, fan->n_az, fan->n_el);
    if (cp->k_max < 1 || cp->k_max > PCP_PLACE_MAX || cp->n_fixed < 0 ||
        cp->n_fixed > PCP_PLACE_MAX || cp->reserved[0] != 0 || cp->reserved[1] != 0)
        return set_err(ctx, PCP_E_INVALID,
                       "%s: k_max %d outside 1..%d, n_fixed %d outside 0..%d or reserved != 0",
                       what, (int)cp->k_max, PCP_PLACE_MAX, (int)cp->n_fixed, PCP_PLACE_MAX);
    int i = 0;
    const int bad = check_index_list(cp->fixed, cp->n_fixed, n, &i);
    if (bad == kListRange)
        return set_err(ctx, PCP_E_INVALID, "%s: fixed[%d] = %lld is no pose of %llu", what, i,
                       (long long)cp->fixed[i], (unsigned long long)n);
    if (bad == kListTwice)
        return set_err(ctx, PCP_E_INVALID, "%s: pose %lld is fixed twice", what,
                       (long long)cp->fixed[i]);
    fx.n = cp->n_fixed;
    for (i = 0; i < PCP_PLACE_MAX; ++i) fx.idx[i] = i < cp->n_fixed ? (int32_t)cp->fixed[i] : 0;
    const uint64_t N = ctx->terrain.present ? ctx->terrain_index_n : 0;
    if (roi && roi_n != N)
        return set_err(ctx, PCP_E_INVALID, "%s: roi of %llu entries for %llu terrain points", what,
                       (unsigned long long)roi_n, (unsigned long long)N);
    *N_out = N;
    return PCP_OK;
}

}  // namespace
}  // namespace pcp
