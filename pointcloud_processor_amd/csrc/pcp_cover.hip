// pcp_cover.hip -- pcp_place_coverage on gfx950: greedy maximum coverage over simulated scans
// (DESIGN.md §6m).  The production fan launch runs unchanged for every candidate pose and leaves
// its first hits on the device; k_cover_resolve finds each blocked ray's terrain point by the
// scan's own hit search (pcp_scan_hit.hpp) and sets one bit of the pose's bitset.  The bitsets are
// pose-major -- seen[p] = W2 64-bit words, bit i % 64 of word i / 64 = terrain point i -- so any
// number of poses fits and a placement round is a streaming AND + population count of every alive
// pose's row against `need`, the points of the region of interest nobody reaches yet.
//
// One gain launch per round in the shape of pcp_place.hip: the blocks add their partial counts
// into the round's row of the gains table, and the LAST block of the round to finish takes the
// first maximum, appends the record and updates `alive`.  A second small launch per round, the
// commit, reads that record from device memory, clears the placed pose's points out of `need` and
// writes their owners: each word of `need` has one writer there, while the gain launch's blocks
// (word chunks x pose groups) share the words they read.  Rounds are ordered by the stream alone;
// no block ever waits for another.  All results are integers and order-free: exact, deterministic.
#pragma clang fp contract(off)

#include <algorithm>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_place_shared.hpp"
#include "pcp_scan_hit.hpp"

namespace pcp {
namespace {

constexpr int kCT = 256;             // threads per block: four waves
constexpr int kCW = kCT / 64;
constexpr int kRP = 8;               // poses per block of a round
constexpr int kRL = 2;               // 16-byte loads per lane and row: four words per lane
constexpr uint32_t kRWave = 64 * 2 * kRL;      // words of `need` a wave holds
constexpr uint32_t kRBlock = kRWave * kCW;     // words per block chunk
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

// One placement round.  Block = (word chunk, pose group): blockIdx.x = group * nchunks + chunk.  A
// wave loads its kRWave words of need once (16-byte loads), streams the rows of its group's alive
// poses through AND + population count, reduces across the wave and adds one integer per (wave,
// pose) into the round's row of the gains table (cleared up front; dead poses are skipped
// wave-uniformly, and so is a wave whose words of need are all zero).
//
// The last block to draw the round's ticket takes the first maximum over the alive poses (ties to
// the lowest index), marks the dead poses' gains -1, tests the best gain against 0, appends the
// record and updates alive: every block of the round has read alive before its draw, and the next
// launch starts after this one has ended.  commit false (the timing entry): the selection is
// made and nothing is written.
__global__ void __launch_bounds__(kCT)
k_cover_round(const unsigned long long *__restrict__ seen,
              const unsigned long long *__restrict__ need, uint32_t W2, int n, uint32_t *alive,
              long long *rg, CoverState *s, const double *__restrict__ pose, uint32_t row,
              double sep2, int r, uint32_t nchunks, int commit) {
    __shared__ RowBest s_best[kCW];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = s->done;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier round stopped the search
    const uint32_t lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % nchunks, grp = blockIdx.x / nchunks;
    const uint32_t wb = chunk * kRBlock + (uint32_t)(tid >> 6) * kRWave + lane * 2u;
    const ulonglong2 *need2 = reinterpret_cast<const ulonglong2 *>(need);
    ulonglong2 nd[kRL];
    bool some = false;
#pragma unroll
    for (int j = 0; j < kRL; ++j) {
        const uint32_t wi = wb + (uint32_t)j * 128u;   // (W2 is even: a pair is inside or outside)
        nd[j] = wi < W2 ? need2[wi >> 1] : make_ulonglong2(0ull, 0ull);
        some |= (nd[j].x | nd[j].y) != 0ull;
    }
    if (__ballot(some)) {   // (wave-uniform)
        uint32_t cnt[kRP];
#pragma unroll
        for (int q = 0; q < kRP; ++q) {
            const int p = (int)grp * kRP + q;
            cnt[q] = 0u;
            if (p < n && alive[p] != 0u) {   // (wave-uniform)
                const ulonglong2 *row2 =
                    reinterpret_cast<const ulonglong2 *>(seen + (size_t)p * W2);
#pragma unroll
                for (int j = 0; j < kRL; ++j) {
                    const uint32_t wi = wb + (uint32_t)j * 128u;
                    if (wi < W2) {
                        const ulonglong2 v = row2[wi >> 1];
                        cnt[q] += (uint32_t)(__popcll(v.x & nd[j].x) + __popcll(v.y & nd[j].y));
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kRP; ++q) {
            uint32_t c = cnt[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c)
                atomicAdd(reinterpret_cast<unsigned long long *>(&rg[(int)grp * kRP + q]),
                          (unsigned long long)c);
        }
    }
    // the round's ticket: this block's sums added before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the round ------------------------------------------------------
    // (a gain is at most 2^32: exact as a double, so the shared first-maximum reduction serves)
    double tb = -1.0;
    int b = -1, none = 0;
    for (int p = tid; p < n; p += kCT) {
        if (alive[p] == 0u) {
            if (commit) rg[p] = -1ll;
            continue;
        }
        const double t =
            (double)__hip_atomic_load(&rg[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t > tb) {
            tb = t;
            b = p;
        }
    }
    block_first_max_all<kCW>(s_best, tb, b, none);
    // no pose alive, or the best reaches nothing new
    if (tid == 0) {
        s->ticket = 0u;   // (the next launch draws from zero)
        s_flag = b >= 0 && tb > 0.0;
        if (!s_flag && commit) s->done = 1;
    }
    __syncthreads();
    if (!s_flag || !commit) return;
    if (tid == 0) {
        const unsigned long long g = (unsigned long long)tb;
        s->sel[r] = b;
        s->gain[r] = g;
        s->cov_after[r] = (r == 0 ? s->base_covered : s->cov_after[r - 1]) + g;
        s->n_sel = r + 1;
    }
    // the placed pose and, with a separation, every pose closer than it in XY leave the search
    for (int p = tid; p < n; p += kCT)
        if (p == b || (sep2 > 0 && cover_closer(pose, row, p, b, sep2))) alive[p] = 0u;
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

CoverDev dev_of(pcp_ctx *ctx, const CoverPlan &c) {
    char *blk = ctx->cover_d.as<char>();
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

int round_enqueue(pcp_ctx *ctx, const CoverPlan &c, const CoverDev &d, const FanEnq &o,
                  double sep2, int r, bool commit) {
    const uint32_t nchunks = (c.W2 + kRBlock - 1) / kRBlock;
    const uint32_t groups = ((uint32_t)c.n + kRP - 1) / kRP;
    hipLaunchKernelGGL(k_cover_round, dim3(nchunks * groups), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, (const unsigned long long *)d.need,
                       c.W2, c.n, d.alive, d.rg + (size_t)r * c.n, d.s,
                       ctx->poses_d.as<const double>(), o.pose_row, sep2, r, nchunks,
                       commit ? 1 : 0);
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

using namespace pcp;

// pcp_place_coverage and, mounted (poses: poses6 rows, el_table nullable), its mounted twin
static int place_coverage_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                               const pcp_fan_params *fan, bool mounted, const double *el_table,
                               const pcp_cover_params *cp, const uint8_t *roi, uint64_t roi_n,
                               int64_t *selected, uint64_t *gain, uint64_t *covered_after,
                               int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                               uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                               uint64_t *base_covered, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_mounted" : "pcp_place_coverage";
    if (!selected || !gain || !covered_after || !n_points || !roi_points || !base_covered ||
        !n_selected)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    CoverFixed fx{};
    uint64_t N = 0;
    if (int rc = check_args(ctx, what, poses, n, fan, mounted, el_table, cp, roi, roi_n, fx, &N))
        return rc;
    if (point_owner && owner_cap < N) {
        *n_points = N;
        return set_err(ctx, PCP_E_CAPACITY, "%s: owners of %llu points, cap %llu", what,
                       (unsigned long long)N, (unsigned long long)owner_cap);
    }
    *n_points = N;
    *n_selected = 0;
    *base_covered = 0;
    if (n == 0 || N == 0) {   // nothing to place or nothing to cover
        uint64_t R = roi ? 0 : N;
        for (uint64_t i = 0; roi && i < N; ++i) R += roi[i] != 0;
        *roi_points = R;
        for (uint64_t i = 0; point_owner && i < N; ++i) point_owner[i] = PCP_OWNER_NONE;
        for (uint64_t p = 0; seen_points && p < n; ++p) seen_points[p] = 0u;
        return PCP_OK;
    }
    // the production fan query: first hits and the live waves stay on the device
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const int K = cp->k_max;
    const CoverPlan c = make_plan((int)n, K, N, point_owner != nullptr, roi != nullptr);
    const size_t down = round_gains ? c.al_off : c.rg_off;
    const size_t pin_own = a16(down);
    PCP_HIP(ctx, ctx->cover_d.ensure(c.bytes));
    PCP_HIP(ctx, ctx->cover_host.ensure(pin_own + (c.owner ? (size_t)N * sizeof(int32_t) : 0) + 64));
    const CoverDev d = dev_of(ctx, c);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(cp->min_separation);
    if (int rc = build_enqueue(ctx, c, d, fan, o, fx, sep2)) return rc;
    // the fixed sensors, in list order, by the rounds' own commit
    for (int i = 0; i < fx.n; ++i)
        if (int rc = commit_enqueue(ctx, c, d, fx.idx[i], i, 0)) return rc;
    for (int r = 0; r < K; ++r) {
        ProfScope ps(ctx, PCP_K_PLACE);
        if (int rc = round_enqueue(ctx, c, d, o, sep2, r, true)) return rc;
        if (int rc = commit_enqueue(ctx, c, d, -1, fx.n + r, r)) return rc;
    }
    // downloads: the state, the counts and the gains in one span, the owners when asked for
    char *blk = ctx->cover_d.as<char>();
    char *pin = ctx->cover_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, down, hipMemcpyDeviceToHost, st));
    if (c.owner)
        if (int rc = copy_to_pinned_async(ctx, pin + pin_own, blk + c.own_off,
                                          (size_t)N * sizeof(int32_t), st))
            return rc;
    if (int rc = stream_done(ctx)) return rc;
    const CoverState *h = reinterpret_cast<const CoverState *>(pin);
    const int ns = h->n_sel;
    for (int r = 0; r < ns; ++r) {
        selected[r] = h->sel[r];
        gain[r] = h->gain[r];
        covered_after[r] = h->cov_after[r];
    }
    if (round_gains && ns)
        std::memcpy(round_gains, pin + c.rg_off, (size_t)ns * n * sizeof(int64_t));
    if (seen_points) std::memcpy(seen_points, pin + c.sp_off, (size_t)n * sizeof(uint32_t));
    if (point_owner) host_copy(ctx, point_owner, pin + pin_own, (size_t)N * sizeof(int32_t));
    *roi_points = h->roi_points;
    *base_covered = h->base_covered;
    *n_selected = ns;
    return PCP_OK;
}

extern "C" int pcp_place_coverage(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                  const pcp_fan_params *fan, const pcp_cover_params *cp,
                                  const uint8_t *roi, uint64_t roi_n, int64_t *selected,
                                  uint64_t *gain, uint64_t *covered_after, int64_t *round_gains,
                                  uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap,
                                  uint64_t *n_points, uint64_t *roi_points,
                                  uint64_t *base_covered, int32_t *n_selected) {
    return place_coverage_impl(ctx, poses5, n, fan, false, nullptr, cp, roi, roi_n, selected, gain,
                               covered_after, round_gains, seen_points, point_owner, owner_cap,
                               n_points, roi_points, base_covered, n_selected);
}

extern "C" int pcp_place_coverage_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                          const pcp_fan_params *fan, const double *el_table,
                                          const pcp_cover_params *cp, const uint8_t *roi,
                                          uint64_t roi_n, int64_t *selected, uint64_t *gain,
                                          uint64_t *covered_after, int64_t *round_gains,
                                          uint32_t *seen_points, int32_t *point_owner,
                                          uint64_t owner_cap, uint64_t *n_points,
                                          uint64_t *roi_points, uint64_t *base_covered,
                                          int32_t *n_selected) {
    return place_coverage_impl(ctx, poses6, n, fan, true, el_table, cp, roi, roi_n, selected, gain,
                               covered_after, round_gains, seen_points, point_owner, owner_cap,
                               n_points, roi_points, base_covered, n_selected);
}

static int place_coverage_burst_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                     const pcp_fan_params *fan, bool mounted,
                                     const double *el_table, const pcp_cover_params *cp,
                                     const uint8_t *roi, uint64_t roi_n, int reps, double ms[3]) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_mounted_burst" : "pcp_place_coverage_burst";
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument or nothing to time", what);
    CoverFixed fx{};
    uint64_t N = 0;
    if (int rc = check_args(ctx, what, poses, n, fan, mounted, el_table, cp, roi, roi_n, fx, &N))
        return rc;
    if (N == 0) return set_err(ctx, PCP_E_INVALID, "%s: no terrain index, nothing to time", what);
    ms[0] = ms[1] = ms[2] = 0.0;
    FanEnq o;
    FanOpts fo{/*want_fh=*/true, /*burst=*/reps, /*burst_ms=*/&ms[0]};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const CoverPlan c = make_plan((int)n, cp->k_max, N, false, roi != nullptr);
    PCP_HIP(ctx, ctx->cover_d.ensure(c.bytes));
    const CoverDev d = dev_of(ctx, c);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(cp->min_separation);
    auto build = [&] { return build_enqueue(ctx, c, d, fan, o, fx, sep2); };
    if (int rc = time_reps(ctx, what, st, reps, build, build, &ms[1])) return rc;
    for (int i = 0; i < fx.n; ++i)
        if (int rc = commit_enqueue(ctx, c, d, fx.idx[i], i, 0)) return rc;
    // round 0's launch with the selection, nothing committed (the row's sums add up over the
    // repetitions: the selection is the same)
    auto round0 = [&] { return round_enqueue(ctx, c, d, o, sep2, 0, false); };
    return time_reps(ctx, what, st, reps, round0, round0, &ms[2]);
}

extern "C" int pcp_place_coverage_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                        const pcp_fan_params *fan, const pcp_cover_params *cp,
                                        const uint8_t *roi, uint64_t roi_n, int reps,
                                        double ms[3]) {
    return place_coverage_burst_impl(ctx, poses5, n, fan, false, nullptr, cp, roi, roi_n, reps, ms);
}

extern "C" int pcp_place_coverage_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                                const pcp_fan_params *fan, const double *el_table,
                                                const pcp_cover_params *cp, const uint8_t *roi,
                                                uint64_t roi_n, int reps, double ms[3]) {
    return place_coverage_burst_impl(ctx, poses6, n, fan, true, el_table, cp, roi, roi_n, reps, ms);
}
