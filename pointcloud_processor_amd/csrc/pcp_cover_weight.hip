// pcp_cover_weight.hip -- pcp_place_coverage_weighted on gfx950: pcp_place_coverage's greedy with a
// weight of 0 .. 255 per terrain point.  The fan launch, k_cover_clear,
// k_cover_resolve and k_cover_count are pcp_cover_phase.hpp's, unchanged; the objective is new.
//
// Bit planes: weight[i] = sum over b of 2^b bit_b(i), so
//     w(seen(p) & need) = sum over b of 2^b popcount(seen[p] & need & plane_b)
// with plane_b the W2-word bitset of the points whose weight has bit b set.  A round stays a
// streaming AND + population count of the alive rows, against up to eight register-resident words
// per position instead of one, and no weight is gathered anywhere.  The host ORs the weight bytes
// and passes the used bits: planes of unused bits are neither built nor read, so a 0/1 weighting is
// one plane and costs what pcp_place_coverage's round costs.
//
// The call keeps one `need` (the commit's single writer per word, as the parent's); a wave of the
// round loads its words of need and of the B planes once and holds need & plane_b in registers.
// PCP_COVER_WEIGHT_ROWS builds the other choice §6q measured against it -- the commit keeps the
// rows need & plane_b themselves, so the round loads B words per position and no need -- and
// PCP_COVER_WEIGHT_WL / _WP the other words per lane and poses per block (the timing tool's
// builds: make wvariants).
#pragma clang fp contract(off)

#include "pcp_cover_phase.hpp"

namespace pcp {
namespace {

#ifndef PCP_COVER_WEIGHT_WP
#define PCP_COVER_WEIGHT_WP 8
#endif
#ifndef PCP_COVER_WEIGHT_WL
#define PCP_COVER_WEIGHT_WL 2
#endif
#ifdef PCP_COVER_WEIGHT_ROWS
constexpr bool kWRows = true;
#else
constexpr bool kWRows = false;
#endif
constexpr int kWP = PCP_COVER_WEIGHT_WP;   // poses per block of a round
constexpr int kWL = PCP_COVER_WEIGHT_WL;   // 16-byte loads per lane and row: four words per lane
constexpr uint32_t kWWave = 64 * 2 * kWL;      // words of `need` a wave holds
constexpr uint32_t kWBlock = kWWave * kCW;     // words per block chunk

// the weighted counts, in front of the parent's block: CoverState's base_covered, gain and
// cov_after are in weight here, and its roi_points stays |R|
struct CoverWExtra {
    unsigned long long roi_weight;     // w(R)
    unsigned long long base_points;    // points of R the fixed sensors reach
    unsigned long long gain_points[PCP_PLACE_MAX];
};
static_assert(sizeof(CoverWExtra) % 16 == 0, "the state follows on a 16-byte boundary");

// the used bits of the weights, lowest first: plane j holds bit (sh >> 4 j) & 7
struct WeightBits {
    int nb = 0;
    uint32_t sh = 0;
};

WeightBits bits_of(uint32_t used) {
    WeightBits w;
    if (!used) used = 1u;   // (every weight zero: one empty plane, R is empty)
    for (uint32_t b = 0; b < 8; ++b)
        if ((used >> b) & 1u) w.sh |= b << (4 * w.nb++);
    return w;
}

// need = {weight != 0} as bits and one plane per used bit, one wave per word, one ballot each;
// |R| and w(R) by a wave reduction and one 64-bit atomic per block; every owner PCP_OWNER_NONE.
// The words past ceil(N / 64) (the padding to an even count) are zero in need and in every plane.
__global__ void __launch_bounds__(kCT)
k_cover_wneed(const uint8_t *__restrict__ weight, unsigned long long N, uint32_t W2,
              unsigned long long *__restrict__ need, unsigned long long *__restrict__ plane,
              int nb, uint32_t sh, int32_t *__restrict__ owner, CoverState *__restrict__ s,
              CoverWExtra *__restrict__ x) {
    __shared__ uint32_t s_cnt, s_w;
    if (threadIdx.x == 0) {
        s_cnt = 0u;
        s_w = 0u;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    const unsigned long long i = (unsigned long long)gw * 64u + lane;
    const bool in = gw < W2 && i < N;
    const uint32_t w = in ? (uint32_t)weight[i] : 0u;
    const uint64_t bal = __ballot(w != 0u);
    if (in && owner) owner[i] = PCP_OWNER_NONE;
    for (int j = 0; j < nb; ++j) {   // (uniform)
        const uint64_t pb = __ballot(((w >> ((sh >> (4 * j)) & 7u)) & 1u) != 0u);
        if (lane == 0 && gw < W2) plane[(size_t)j * W2 + gw] = pb;
    }
    uint32_t ws = w;   // (a wave's weights: at most 64 x 255)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
    if (lane == 0 && gw < W2) {
        need[gw] = bal;
        if (bal) {
            atomicAdd(&s_cnt, (uint32_t)__popcll(bal));
            atomicAdd(&s_w, ws);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) {
        atomicAdd(&s->roi_points, (unsigned long long)s_cnt);
        atomicAdd(&x->roi_weight, (unsigned long long)s_w);
    }
}

// One placement round in the shape of k_cover_round: block = (word chunk, pose group),
// blockIdx.x = group * nchunks + chunk.  A wave loads its kWWave words of need and of the B planes
// once and keeps need & plane_b; each row word of an alive pose then costs B ANDs, B population
// counts and B shift-adds.  One 64-bit atomic per (wave, pose) into the round's row of the gains
// table; the last block to draw the round's ticket takes the first maximum, as k_cover_round's.
template <int B>
__global__ void __launch_bounds__(kCT)
k_cover_wround(const unsigned long long *__restrict__ seen,
               const unsigned long long *__restrict__ need,
               const unsigned long long *__restrict__ plane, uint32_t sh, uint32_t W2, int n,
               uint32_t *alive, long long *rg, CoverState *s, const double *__restrict__ pose,
               uint32_t row, double sep2, int r, uint32_t nchunks, int commit) {
    __shared__ RowBest s_best[kCW];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = s->done;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier round stopped the search
    const uint32_t lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % nchunks, grp = blockIdx.x / nchunks;
    const uint32_t wb = chunk * kWBlock + (uint32_t)(tid >> 6) * kWWave + lane * 2u;
    const ulonglong2 *need2 = reinterpret_cast<const ulonglong2 *>(need);
    ulonglong2 np[B][kWL];   // need & plane_b
    bool some = false;
#pragma unroll
    for (int j = 0; j < kWL; ++j) {
        const uint32_t wi = wb + (uint32_t)j * 128u;   // (W2 is even: a pair is inside or outside)
        const bool in = wi < W2;
        // (kWRows: the planes are kept as need & plane_b, need itself is not read)
        const ulonglong2 nd = kWRows ? make_ulonglong2(~0ull, ~0ull)
                              : in   ? need2[wi >> 1]
                                     : make_ulonglong2(0ull, 0ull);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            // One plane: every weight is 0 or one power of two, so the plane is R and need, a
            // subset of it, is need & plane already -- the plane is not read and the round loads
            // what k_cover_round loads.  (b * W2 is even: a plane's pairs are 16-byte aligned)
            const ulonglong2 pl =
                B == 1 && !kWRows ? nd
                : in ? reinterpret_cast<const ulonglong2 *>(plane + (size_t)b * W2)[wi >> 1]
                     : make_ulonglong2(0ull, 0ull);
            np[b][j] = make_ulonglong2(nd.x & pl.x, nd.y & pl.y);
            if (kWRows) some |= (pl.x | pl.y) != 0ull;
        }
        // (a point of need has a weight >= 1, so some plane holds it: need alone says whether
        // the wave has anything to count)
        if (!kWRows) some |= (nd.x | nd.y) != 0ull;
    }
    if (__ballot(some)) {   // (wave-uniform)
        // a lane's partial is at most 4 words x 64 bits x 255 < 2^16 and a wave's 256 words x 64
        // bits x 255 < 2^23: 32 bits hold both
        uint32_t cnt[kWP];
#pragma unroll
        for (int q = 0; q < kWP; ++q) {
            const int p = (int)grp * kWP + q;
            cnt[q] = 0u;
            if (p < n && alive[p] != 0u) {   // (wave-uniform)
                const ulonglong2 *row2 =
                    reinterpret_cast<const ulonglong2 *>(seen + (size_t)p * W2);
#pragma unroll
                for (int j = 0; j < kWL; ++j) {
                    const uint32_t wi = wb + (uint32_t)j * 128u;
                    if (wi < W2) {
                        const ulonglong2 v = row2[wi >> 1];
#pragma unroll
                        for (int b = 0; b < B; ++b)
                            cnt[q] += (uint32_t)(__popcll(v.x & np[b][j].x) +
                                                 __popcll(v.y & np[b][j].y))
                                      << ((sh >> (4 * b)) & 7u);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kWP; ++q) {
            uint32_t c = cnt[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c)
                atomicAdd(reinterpret_cast<unsigned long long *>(&rg[(int)grp * kWP + q]),
                          (unsigned long long)c);
        }
    }
    // the round's ticket: this block's sums added before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the round ------------------------------------------------------
    // (a gain is at most 255 N < 2^40: exact as a double, so the shared first-maximum reduction
    // serves)
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

// k_cover_commit with the weight and the point count of the committed points added into the
// record: a fixed sensor (b_fixed >= 0) adds to base_covered (weight) and base_points, round r's
// commit to gain_points[r] (its weight is the round's own gain).  One wave per word, the only
// writer of that word of need and of its 64 owners; the planes are read only (kWRows: the same
// wave clears the committed points out of its word of every plane too).
__global__ void __launch_bounds__(kCT)
k_cover_wcommit(const unsigned long long *__restrict__ seen, unsigned long long *need,
                unsigned long long *plane, int nb, uint32_t sh, uint32_t W2,
                int32_t *__restrict__ owner, CoverState *s, CoverWExtra *x, int b_fixed,
                int32_t owner_id, int r) {
    __shared__ uint32_t s_cnt, s_w;
    const int b = b_fixed >= 0 ? b_fixed : (s->n_sel > r ? (int)s->sel[r] : -1);
    if (b < 0) return;   // (uniform)
    if (threadIdx.x == 0) {
        s_cnt = 0u;
        s_w = 0u;
    }
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
                atomicAdd(&s_cnt, (uint32_t)__popcll(m));
                if (b_fixed >= 0 || kWRows) {
                    uint32_t w = 0u;   // (a word's weight: at most 64 x 255)
                    for (int j = 0; j < nb; ++j) {
                        const unsigned long long pw = plane[(size_t)j * W2 + gw];
                        w += (uint32_t)__popcll(m & pw) << ((sh >> (4 * j)) & 7u);
                        if (kWRows) plane[(size_t)j * W2 + gw] = pw & ~m;
                    }
                    atomicAdd(&s_w, w);   // (a block's: at most 4 x 64 x 255)
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0 || !s_cnt) return;
    if (b_fixed >= 0) {
        atomicAdd(&s->base_covered, (unsigned long long)s_w);
        atomicAdd(&x->base_points, (unsigned long long)s_cnt);
    } else {
        atomicAdd(&x->gain_points[r], (unsigned long long)s_cnt);
    }
}

// the call's device block: [CoverWExtra | the parent's block (its staged bytes = the weights) |
// planes u64 nb x W2]; the download is [extra .. gains) or [.. alive)
struct WeightPlan {
    CoverPlan c;
    WeightBits wb;
    size_t pre = 0, plane_off = 0, bytes = 0;
};

WeightPlan make_wplan(int n, int K, uint64_t N, bool owner, WeightBits wb) {
    WeightPlan p;
    p.c = make_plan(n, K, N, owner, /*roi=*/true);
    p.wb = wb;
    p.pre = a16(sizeof(CoverWExtra));
    p.plane_off = p.pre + a16(p.c.bytes);
    p.bytes = p.plane_off + (size_t)wb.nb * p.c.W2 * sizeof(uint64_t) + 64;
    return p;
}

struct WeightDev {
    CoverDev d;
    CoverWExtra *x;
    unsigned long long *plane;
};

WeightDev wdev_of(char *blk, const WeightPlan &p) {
    WeightDev w;
    w.d = dev_of(blk + p.pre, p.c);
    w.x = reinterpret_cast<CoverWExtra *>(blk);
    w.plane = reinterpret_cast<unsigned long long *>(blk + p.plane_off);
    return w;
}

// build_enqueue with k_cover_wneed in k_cover_need's place: clear, need and planes, resolve, counts
int wbuild_enqueue(pcp_ctx *ctx, const WeightPlan &p, const WeightDev &w,
                   const pcp_fan_params *fan, const FanEnq &o, const CoverFixed &fx, double sep2) {
    hipStream_t st = ctx->stream;
    const CoverPlan &c = p.c;
    const CoverDev &d = w.d;
    const double *pose = ctx->poses_d.as<const double>();
    PCP_HIP(ctx, hipMemsetAsync(w.x, 0, sizeof(CoverWExtra), st));
    {
        const unsigned long long n2 = (unsigned long long)c.n * c.W2 / 2;
        const unsigned g = (unsigned)std::min<uint64_t>((n2 + kCT - 1) / kCT + 1, 4096);
        hipLaunchKernelGGL(k_cover_clear, dim3(g), dim3(kCT), 0, st,
                           reinterpret_cast<ulonglong2 *>(d.seen), n2, d.rg,
                           (unsigned long long)c.K * c.n, d.seen_pts, d.alive, c.n, d.s, pose,
                           o.pose_row, fx, sep2);
        PCP_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(k_cover_wneed, dim3((c.W2 + kCW - 1) / kCW), dim3(kCT), 0, st,
                       (const uint8_t *)d.roi, (unsigned long long)c.N, c.W2, d.need, w.plane,
                       p.wb.nb, p.wb.sh, d.owner, d.s, w.x);
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

int wcommit_enqueue(pcp_ctx *ctx, const WeightPlan &p, const WeightDev &w, int b_fixed,
                    int owner_id, int r) {
    hipLaunchKernelGGL(k_cover_wcommit, dim3((p.c.W2 + kCW - 1) / kCW), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)w.d.seen, w.d.need, w.plane, p.wb.nb, p.wb.sh,
                       p.c.W2, w.d.owner,
                       w.d.s, w.x, b_fixed, (int32_t)owner_id, r);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

template <int B>
void wround_launch(pcp_ctx *ctx, const WeightPlan &p, const WeightDev &w, const FanEnq &o,
                   double sep2, int r, bool commit, uint32_t nchunks, uint32_t groups) {
    hipLaunchKernelGGL(k_cover_wround<B>, dim3(nchunks * groups), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)w.d.seen, (const unsigned long long *)w.d.need,
                       (const unsigned long long *)w.plane, p.wb.sh, p.c.W2, p.c.n, w.d.alive,
                       w.d.rg + (size_t)r * p.c.n, w.d.s, ctx->poses_d.as<const double>(),
                       o.pose_row, sep2, r, nchunks, commit ? 1 : 0);
}

int wround_enqueue(pcp_ctx *ctx, const WeightPlan &p, const WeightDev &w, const FanEnq &o,
                   double sep2, int r, bool commit) {
    const uint32_t nchunks = (p.c.W2 + kWBlock - 1) / kWBlock;
    const uint32_t groups = ((uint32_t)p.c.n + kWP - 1) / kWP;
    switch (p.wb.nb) {   // the plane count is a compile-time constant of the round: registers
    case 1: wround_launch<1>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 2: wround_launch<2>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 3: wround_launch<3>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 4: wround_launch<4>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 5: wround_launch<5>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 6: wround_launch<6>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    case 7: wround_launch<7>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    default: wround_launch<8>(ctx, p, w, o, sep2, r, commit, nchunks, groups); break;
    }
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what pcp_place_coverage refuses, then the weights; *N_out = N, *used = the OR of the bytes
int wcheck_args(pcp_ctx *ctx, const char *what, const double *poses, uint64_t n,
                const pcp_fan_params *fan, bool mounted, const double *el_table,
                const pcp_cover_params *cp, const uint8_t *weight, uint64_t weight_n,
                CoverFixed &fx, uint64_t *N_out, uint32_t *used) {
    if (int rc = check_args(ctx, what, poses, n, fan, mounted, el_table, cp, nullptr, 0, fx, N_out))
        return rc;
    if (!weight) return set_err(ctx, PCP_E_INVALID, "%s: null weight", what);
    if (weight_n != *N_out)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu weights for %llu terrain points", what,
                       (unsigned long long)weight_n, (unsigned long long)*N_out);
    // the used bits, eight bytes at a time
    const uint64_t N = *N_out;
    uint64_t acc = 0;
    uint64_t i = 0;
    for (; i + 8 <= N; i += 8) {
        uint64_t v;
        std::memcpy(&v, weight + i, 8);
        acc |= v;
    }
    for (; i < N; ++i) acc |= weight[i];
    acc |= acc >> 32;
    acc |= acc >> 16;
    acc |= acc >> 8;
    *used = (uint32_t)(acc & 0xffu);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

// pcp_place_coverage_weighted and, mounted (poses: poses6 rows, el_table nullable), its twin
static int place_weighted_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                               const pcp_fan_params *fan, bool mounted, const double *el_table,
                               const pcp_cover_params *cp, const uint8_t *weight,
                               uint64_t weight_n, int64_t *selected, uint64_t *gain,
                               uint64_t *covered_after, uint64_t *gain_points,
                               int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                               uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                               uint64_t *roi_weight, uint64_t *base_covered,
                               uint64_t *base_points, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    const char *what =
        mounted ? "pcp_place_coverage_weighted_mounted" : "pcp_place_coverage_weighted";
    if (!selected || !gain || !covered_after || !n_points || !roi_points || !roi_weight ||
        !base_covered || !base_points || !n_selected)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    CoverFixed fx{};
    uint64_t N = 0;
    uint32_t used = 0;
    if (int rc = wcheck_args(ctx, what, poses, n, fan, mounted, el_table, cp, weight, weight_n, fx,
                             &N, &used))
        return rc;
    if (point_owner && owner_cap < N) {
        *n_points = N;
        return set_err(ctx, PCP_E_CAPACITY, "%s: owners of %llu points, cap %llu", what,
                       (unsigned long long)N, (unsigned long long)owner_cap);
    }
    *n_points = N;
    *n_selected = 0;
    *base_covered = 0;
    *base_points = 0;
    if (n == 0 || N == 0) {   // nothing to place or nothing to cover
        uint64_t R = 0, wR = 0;
        for (uint64_t i = 0; i < N; ++i) {
            R += weight[i] != 0;
            wR += weight[i];
        }
        *roi_points = R;
        *roi_weight = wR;
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
    const WeightPlan p = make_wplan((int)n, K, N, point_owner != nullptr, bits_of(used));
    const CoverPlan &c = p.c;
    const size_t down = p.pre + (round_gains ? c.al_off : c.rg_off);
    const size_t pin_own = a16(down);
    PCP_HIP(ctx, ctx->cweight_d.ensure(p.bytes));
    PCP_HIP(ctx,
            ctx->cweight_host.ensure(pin_own + (c.owner ? (size_t)N * sizeof(int32_t) : 0) + 64));
    char *blk = ctx->cweight_d.as<char>();
    const WeightDev w = wdev_of(blk, p);
    if (int rc = upload_async(ctx, w.d.roi, weight, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(cp->min_separation);
    if (int rc = wbuild_enqueue(ctx, p, w, fan, o, fx, sep2)) return rc;
    // the fixed sensors, in list order, by the rounds' own commit
    for (int i = 0; i < fx.n; ++i)
        if (int rc = wcommit_enqueue(ctx, p, w, fx.idx[i], i, 0)) return rc;
    for (int r = 0; r < K; ++r) {
        ProfScope ps(ctx, PCP_K_PLACE);
        if (int rc = wround_enqueue(ctx, p, w, o, sep2, r, true)) return rc;
        if (int rc = wcommit_enqueue(ctx, p, w, -1, fx.n + r, r)) return rc;
    }
    // downloads: the counts, the state and the gains in one span, the owners when asked for
    char *pin = ctx->cweight_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, down, hipMemcpyDeviceToHost, st));
    if (c.owner)
        if (int rc = copy_to_pinned_async(ctx, pin + pin_own, blk + p.pre + c.own_off,
                                          (size_t)N * sizeof(int32_t), st))
            return rc;
    if (int rc = stream_done(ctx)) return rc;
    const CoverWExtra *x = reinterpret_cast<const CoverWExtra *>(pin);
    const char *par = pin + p.pre;
    const CoverState *h = reinterpret_cast<const CoverState *>(par);
    const int ns = h->n_sel;
    for (int r = 0; r < ns; ++r) {
        selected[r] = h->sel[r];
        gain[r] = h->gain[r];
        covered_after[r] = h->cov_after[r];
        if (gain_points) gain_points[r] = x->gain_points[r];
    }
    if (round_gains && ns)
        std::memcpy(round_gains, par + c.rg_off, (size_t)ns * n * sizeof(int64_t));
    if (seen_points) std::memcpy(seen_points, par + c.sp_off, (size_t)n * sizeof(uint32_t));
    if (point_owner) host_copy(ctx, point_owner, pin + pin_own, (size_t)N * sizeof(int32_t));
    *roi_points = h->roi_points;
    *roi_weight = x->roi_weight;
    *base_covered = h->base_covered;
    *base_points = x->base_points;
    *n_selected = ns;
    return PCP_OK;
}

extern "C" int pcp_place_coverage_weighted(
    pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
    const pcp_cover_params *cp, const uint8_t *weight, uint64_t weight_n, int64_t *selected,
    uint64_t *gain, uint64_t *covered_after, uint64_t *gain_points, int64_t *round_gains,
    uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
    uint64_t *roi_points, uint64_t *roi_weight, uint64_t *base_covered, uint64_t *base_points,
    int32_t *n_selected) {
    return place_weighted_impl(ctx, poses5, n, fan, false, nullptr, cp, weight, weight_n, selected,
                               gain, covered_after, gain_points, round_gains, seen_points,
                               point_owner, owner_cap, n_points, roi_points, roi_weight,
                               base_covered, base_points, n_selected);
}

extern "C" int pcp_place_coverage_weighted_mounted(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_cover_params *cp, const uint8_t *weight, uint64_t weight_n,
    int64_t *selected, uint64_t *gain, uint64_t *covered_after, uint64_t *gain_points,
    int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap,
    uint64_t *n_points, uint64_t *roi_points, uint64_t *roi_weight, uint64_t *base_covered,
    uint64_t *base_points, int32_t *n_selected) {
    return place_weighted_impl(ctx, poses6, n, fan, true, el_table, cp, weight, weight_n, selected,
                               gain, covered_after, gain_points, round_gains, seen_points,
                               point_owner, owner_cap, n_points, roi_points, roi_weight,
                               base_covered, base_points, n_selected);
}

static int place_weighted_burst_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                     const pcp_fan_params *fan, bool mounted,
                                     const double *el_table, const pcp_cover_params *cp,
                                     const uint8_t *weight, uint64_t weight_n, int reps,
                                     double ms[3]) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_weighted_mounted_burst"
                               : "pcp_place_coverage_weighted_burst";
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument or nothing to time", what);
    CoverFixed fx{};
    uint64_t N = 0;
    uint32_t used = 0;
    if (int rc = wcheck_args(ctx, what, poses, n, fan, mounted, el_table, cp, weight, weight_n, fx,
                             &N, &used))
        return rc;
    if (N == 0) return set_err(ctx, PCP_E_INVALID, "%s: no terrain index, nothing to time", what);
    ms[0] = ms[1] = ms[2] = 0.0;
    FanEnq o;
    FanOpts fo{/*want_fh=*/true, /*burst=*/reps, /*burst_ms=*/&ms[0]};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const WeightPlan p = make_wplan((int)n, cp->k_max, N, false, bits_of(used));
    PCP_HIP(ctx, ctx->cweight_d.ensure(p.bytes));
    const WeightDev w = wdev_of(ctx->cweight_d.as<char>(), p);
    if (int rc = upload_async(ctx, w.d.roi, weight, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(cp->min_separation);
    auto build = [&] { return wbuild_enqueue(ctx, p, w, fan, o, fx, sep2); };
    if (int rc = time_reps(ctx, what, st, reps, build, build, &ms[1])) return rc;
    for (int i = 0; i < fx.n; ++i)
        if (int rc = wcommit_enqueue(ctx, p, w, fx.idx[i], i, 0)) return rc;
    // round 0's launch with the selection, nothing committed (the row's sums add up over the
    // repetitions: the selection is the same)
    auto round0 = [&] { return wround_enqueue(ctx, p, w, o, sep2, 0, false); };
    return time_reps(ctx, what, st, reps, round0, round0, &ms[2]);
}

extern "C" int pcp_place_coverage_weighted_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                                 const pcp_fan_params *fan,
                                                 const pcp_cover_params *cp,
                                                 const uint8_t *weight, uint64_t weight_n,
                                                 int reps, double ms[3]) {
    return place_weighted_burst_impl(ctx, poses5, n, fan, false, nullptr, cp, weight, weight_n,
                                     reps, ms);
}

extern "C" int pcp_place_coverage_weighted_mounted_burst(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_cover_params *cp, const uint8_t *weight, uint64_t weight_n,
    int reps, double ms[3]) {
    return place_weighted_burst_impl(ctx, poses6, n, fan, true, el_table, cp, weight, weight_n,
                                     reps, ms);
}
