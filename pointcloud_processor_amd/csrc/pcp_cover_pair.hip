// pcp_cover_pair.hip -- pcp_place_coverage_pair on gfx950: the exact best pair of mobile sensors by
// the terrain their scans reach.  The bitsets, the need words and the fixed
// sensors' commits are pcp_place_coverage's own (pcp_cover_phase.hpp), in a block of this call's.
// Behind them, with need0 = the region less what the fixed sensors reach:
//   k_cpair_mask    M[p] = seen[p] & need0 in place (seen_points is counted before it) and
//                   g[p] = |M[p]| into the plan's one row of gains;
//   k_cpair_tiles   x[a][b] = sum over the words of popcount(M[a] & M[b]) for the upper triangle:
//                   an AND-popcount "GEMM" over the rows, partial sums by integer atomics;
//   k_cpair_select  u[a][b] = g[a] + g[b] - x[a][b] under the admissibility and separation masks,
//                   each row's first maximum, the optional dense table, and in the launch's last
//                   block the best pair, the best single and the answer's record;
// then the answer's one or two poses are folded by k_cover_commit.  The launches are ordered by
// the stream alone; no block ever waits for another.  Every count is an integer below 2^32 (a
// count of terrain points, N < 2^32), so 32-bit accumulators hold it and the order of the atomic
// additions cannot matter: exact, deterministic.
#pragma clang fp contract(off)

#include "pcp_cover_phase.hpp"

namespace pcp {
namespace {

constexpr int kPT = 64;              // poses per tile side
constexpr int kPM = 4;               // a lane's micro-tile: kPM x kPM pairs, rows 16 apart
constexpr int kPC = 32;              // words per staged chunk of a row
constexpr int kPLd = kPC / 2 + 1;    // a staged row in 16-byte slots: 68 dwords, so the 16 rows a
                                     // 16-lane group of a b128 read touches fall on 16 x 4 banks
constexpr int kPLoads = 2 * kPT * (kPC / 2) / kCT;   // b128 loads per thread per chunk
static_assert(kPT == 16 * kPM && kCT == 256, "16 x 16 lanes of micro-tiles");
static_assert(2 * kPT * (kPC / 2) % kCT == 0, "whole b128 loads per thread");
constexpr uint32_t kPBlocks = 1024;  // blocks a launch aims at: four per CU (LDS: 34 KiB each)

// the call's result record (downloaded), the singles and the rows' partners behind it
struct CPairOut {
    int64_t pair[2];
    unsigned long long pair_gain;
    int64_t single;
    unsigned long long single_gain;
    int64_t pad[3];
};
static_assert(sizeof(CPairOut) == 64, "the singles follow on a 16-byte boundary");

// M[p] = seen[p] & need0 in place and g[p] += |M[p]|: blockIdx.y = the pose, blockIdx.x = a chunk
// of kCntBlock words (k_cover_count's shape).  g is the plan's row of gains, zero before
__global__ void __launch_bounds__(kCT)
k_cpair_mask(unsigned long long *__restrict__ seen, const unsigned long long *__restrict__ need,
             uint32_t W2, long long *g) {
    const uint32_t p = blockIdx.y;
    ulonglong2 *row = reinterpret_cast<ulonglong2 *>(seen + (size_t)p * W2);
    const ulonglong2 *need2 = reinterpret_cast<const ulonglong2 *>(need);
    const uint32_t n2 = W2 / 2;
    const uint32_t lo = blockIdx.x * (kCntBlock / 2);
    const uint32_t hi = min(n2, lo + kCntBlock / 2);
    uint32_t cnt = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kCT) {
        const ulonglong2 v = row[i], nd = need2[i];
        const ulonglong2 m = make_ulonglong2(v.x & nd.x, v.y & nd.y);
        if (m.x != v.x || m.y != v.y) row[i] = m;
        cnt += (uint32_t)(__popcll(m.x) + __popcll(m.y));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt)
        atomicAdd(reinterpret_cast<unsigned long long *>(&g[p]), (unsigned long long)cnt);
}

// The pair tiles.  Block (slice, ta, tb), ta <= tb: the pairs of poses ta kPT .. x tb kPT .. over
// the chunks [slice per_slice, + per_slice) of the word axis.  A chunk's 2 kPT rows of kPC words
// are staged in LDS; lane (i, j) of the 16 x 16 owns the pairs (i + 16 r, j + 16 c), r, c < kPM,
// and walks the chunk with b128 reads: of a wave's reads the A rows are four addresses
// (broadcast) and the B rows sixteen, 68 dwords apart -- no bank is met twice in a 16-lane group.
// Per 64-bit word and pair: two ANDs and two accumulating bit counts, no cross-lane reduction.
// A chunk whose need0 words are all zero holds only zero rows and is skipped (the same decision in
// every wave of the block).  The partial sums go into x by atomics.
__global__ void __launch_bounds__(kCT)
k_cpair_tiles(const unsigned long long *__restrict__ M, const unsigned long long *__restrict__ need,
              uint32_t W2, int n, uint32_t *x, uint32_t nchunks, uint32_t per_slice) {
    __shared__ ulonglong2 s_rows[2 * kPT][kPLd];
    const uint32_t ta = blockIdx.y, tb = blockIdx.z;
    if (ta > tb) return;   // (uniform) the lower triangle of the tiles
    const int tid = threadIdx.x;
    const int i = tid >> 4, j = tid & 15;
    const uint32_t c0 = blockIdx.x * per_slice, c1 = min(nchunks, c0 + per_slice);
    uint32_t acc[kPM][kPM];
#pragma unroll
    for (int r = 0; r < kPM; ++r)
#pragma unroll
        for (int c = 0; c < kPM; ++c) acc[r][c] = 0u;
    for (uint32_t ch = c0; ch < c1; ++ch) {
        const uint32_t w0 = ch * kPC;
        const uint32_t wn = w0 + ((uint32_t)tid & (kPC - 1));
        if (!__ballot(wn < W2 && need[wn] != 0ull)) continue;   // (block-uniform)
        __syncthreads();   // the chunk before has been walked
#pragma unroll
        for (int l = 0; l < kPLoads; ++l) {
            const int idx = tid + kCT * l;
            const int r = idx / (kPC / 2), q = idx % (kPC / 2);
            const uint32_t p = r < kPT ? ta * kPT + (uint32_t)r : tb * kPT + (uint32_t)(r - kPT);
            const uint32_t wq = w0 + 2u * (uint32_t)q;   // (W2 is even: a slot is inside or outside)
            ulonglong2 v = make_ulonglong2(0ull, 0ull);
            if (p < (uint32_t)n && wq < W2)
                v = reinterpret_cast<const ulonglong2 *>(M)[((size_t)p * W2 + wq) >> 1];
            s_rows[r][q] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kPC / 2; ++k) {
            ulonglong2 a[kPM], b[kPM];
#pragma unroll
            for (int r = 0; r < kPM; ++r) a[r] = s_rows[i + 16 * r][k];
#pragma unroll
            for (int c = 0; c < kPM; ++c) b[c] = s_rows[kPT + j + 16 * c][k];
#pragma unroll
            for (int r = 0; r < kPM; ++r)
#pragma unroll
                for (int c = 0; c < kPM; ++c)
                    acc[r][c] += (uint32_t)(__popcll(a[r].x & b[c].x) + __popcll(a[r].y & b[c].y));
        }
    }
#pragma unroll
    for (int r = 0; r < kPM; ++r)
#pragma unroll
        for (int c = 0; c < kPM; ++c) {
            const uint32_t pa = ta * kPT + (uint32_t)(i + 16 * r);
            const uint32_t pb = tb * kPT + (uint32_t)(j + 16 * c);
            if (pa < pb && pb < (uint32_t)n && acc[r][c]) atomicAdd(&x[(size_t)pa * n + pb], acc[r][c]);
        }
}

// The selection.  Block a = row a of the pairs: u[a][b] for the admissible b > a not closer to a
// than the separation, the row's first maximum into partner / pgain, the row of the dense table
// (-1 elsewhere) when asked for, and single_gains[a].  The last block to draw the ticket takes
// the first maxima over the rows and over the singles (a gain is below 2^32: exact as a double, so
// the shared first-maximum reduction serves), writes the result record and, commit set, the
// answer's poses as rounds 0 and 1 of the state for k_cover_commit.
__global__ void __launch_bounds__(kCT)
k_cpair_select(const long long *g, const uint32_t *__restrict__ x,
               const uint32_t *__restrict__ adm, int n, const double *__restrict__ pose,
               uint32_t row, double sep2, int64_t *sg, int64_t *partner, int64_t *pgain,
               int64_t *__restrict__ table, CoverState *s, CPairOut *out, int commit) {
    __shared__ RowBest s_best[kCW];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    const int a = blockIdx.x;
    const bool adm_a = adm[a] != 0u;
    const long long ga = g[a];
    double t = -1.0;
    int ba = -1, bb = -1;
    for (int b = tid; b < n; b += kCT) {
        long long u = -1ll;
        if (adm_a && b > a && adm[b] != 0u && !(sep2 > 0 && cover_closer(pose, row, a, b, sep2))) {
            u = ga + g[b] - (long long)x[(size_t)a * n + b];
            if ((double)u > t) {
                t = (double)u;
                ba = a;
                bb = b;
            }
        }
        if (table) table[(size_t)a * n + b] = u;
    }
    block_first_max<kCW>(s_best, t, ba, bb);
    if (tid == 0) {
        partner[a] = bb;
        pgain[a] = bb >= 0 ? (int64_t)t : -1ll;
        sg[a] = adm_a ? ga : -1ll;
    }
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block ---------------------------------------------------------------------
    t = -1.0;
    ba = bb = -1;
    double ts = -1.0;
    int sa = -1, sb = -1;
    for (int p = tid; p < n; p += kCT) {
        const long long pg = __hip_atomic_load(&pgain[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pg >= 0 && (double)pg > t) {
            t = (double)pg;
            ba = p;
            bb = (int)__hip_atomic_load(&partner[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const long long s1 = __hip_atomic_load(&sg[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s1 >= 0 && (double)s1 > ts) {
            ts = (double)s1;
            sa = p;
            sb = 0;
        }
    }
    block_first_max_all<kCW>(s_best, t, ba, bb);
    block_first_max_all<kCW>(s_best, ts, sa, sb);
    if (tid != 0) return;
    s->ticket = 0u;   // (the next launch draws from zero)
    const unsigned long long pg = ba >= 0 ? (unsigned long long)t : 0ull;
    const unsigned long long s1 = sa >= 0 ? (unsigned long long)ts : 0ull;
    out->pair[0] = ba;
    out->pair[1] = ba >= 0 ? bb : -1;
    out->pair_gain = pg;
    out->single = sa;
    out->single_gain = s1;
    if (!commit) return;
    const int ns = ba >= 0 && pg > s1 ? 2 : (sa >= 0 && s1 > 0ull ? 1 : 0);
    s->sel[0] = ns == 2 ? ba : sa;
    s->sel[1] = bb;
    s->n_sel = ns;
}

// the call's device block: the plan's block with one row of gains (g), then [result | singles i64
// n | partner i64 n | partner gains i64 n | x u32 n x n | dense table i64 n x n]; the downloads are
// [state .. gains), [result .. x) and, when asked for, the table and the owners
struct CPairPlan {
    CoverPlan c;
    bool table = false;
    size_t out_off = 0, sg_off = 0, pt_off = 0, pg_off = 0, x_off = 0, tab_off = 0, bytes = 0;
    // the pinned landing: [state .. gains) | [result .. x) | table | owners
    size_t pin_out = 0, pin_tab = 0, pin_own = 0, pin_bytes = 0;
};

CPairPlan make_pair_plan(int n, uint64_t N, bool owner, bool roi, bool table) {
    CPairPlan q;
    q.c = make_plan(n, 1, N, owner, roi);
    q.table = table;
    const size_t row = (size_t)n * sizeof(int64_t);
    q.out_off = a16(q.c.bytes);
    q.sg_off = q.out_off + sizeof(CPairOut);
    q.pt_off = a16(q.sg_off + row);
    q.pg_off = a16(q.pt_off + row);
    q.x_off = a16(q.pg_off + row);
    q.tab_off = a16(q.x_off + (size_t)n * n * sizeof(uint32_t));
    q.bytes = q.tab_off + (table ? (size_t)n * n * sizeof(int64_t) : 0) + 64;
    q.pin_out = a16(q.c.rg_off);
    q.pin_tab = a16(q.pin_out + (q.x_off - q.out_off));
    q.pin_own = a16(q.pin_tab + (table ? (size_t)n * n * sizeof(int64_t) : 0));
    q.pin_bytes = q.pin_own + (owner ? (size_t)N * sizeof(int32_t) : 0) + 64;
    return q;
}

struct CPairDev {
    CPairOut *out;
    int64_t *sg, *partner, *pgain, *table;
    uint32_t *x;
};

CPairDev pair_dev_of(char *blk, const CPairPlan &q) {
    CPairDev e;
    e.out = reinterpret_cast<CPairOut *>(blk + q.out_off);
    e.sg = reinterpret_cast<int64_t *>(blk + q.sg_off);
    e.partner = reinterpret_cast<int64_t *>(blk + q.pt_off);
    e.pgain = reinterpret_cast<int64_t *>(blk + q.pg_off);
    e.x = reinterpret_cast<uint32_t *>(blk + q.x_off);
    e.table = q.table ? reinterpret_cast<int64_t *>(blk + q.tab_off) : nullptr;
    return e;
}

// the mask pass with the singles; clear_g: the row of gains is zeroed first (a repetition of the
// timing entry: the call's own row comes zero out of k_cover_clear)
int mask_enqueue(pcp_ctx *ctx, const CoverPlan &c, const CoverDev &d, bool clear_g) {
    if (clear_g)
        PCP_HIP(ctx, hipMemsetAsync(d.rg, 0, (size_t)c.n * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(k_cpair_mask, dim3((c.W2 + kCntBlock - 1) / kCntBlock, (unsigned)c.n),
                       dim3(kCT), 0, ctx->stream, d.seen, (const unsigned long long *)d.need, c.W2,
                       d.rg);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// x cleared, the tiles and the selection
int pairs_enqueue(pcp_ctx *ctx, const CPairPlan &q, const CoverDev &d, const CPairDev &e,
                  const FanEnq &o, double sep2, bool table, bool commit) {
    const CoverPlan &c = q.c;
    hipStream_t st = ctx->stream;
    PCP_HIP(ctx, hipMemsetAsync(e.x, 0, (size_t)c.n * c.n * sizeof(uint32_t), st));
    const uint32_t nt = ((uint32_t)c.n + kPT - 1) / kPT;
    const uint32_t nchunks = (c.W2 + kPC - 1) / kPC;
    const uint32_t tiles = nt * (nt + 1) / 2;
    const uint32_t slices = std::min(nchunks, std::max(1u, (kPBlocks + tiles - 1) / tiles));
    const uint32_t per_slice = (nchunks + slices - 1) / slices;
    hipLaunchKernelGGL(k_cpair_tiles, dim3((nchunks + per_slice - 1) / per_slice, nt, nt), dim3(kCT),
                       0, st, (const unsigned long long *)d.seen,
                       (const unsigned long long *)d.need, c.W2, c.n, e.x, nchunks, per_slice);
    PCP_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_cpair_select, dim3((unsigned)c.n), dim3(kCT), 0, st,
                       (const long long *)d.rg, (const uint32_t *)e.x, (const uint32_t *)d.alive,
                       c.n, ctx->poses_d.as<const double>(), o.pose_row, sep2, e.sg, e.partner,
                       e.pgain, table ? e.table : nullptr, d.s, e.out, commit ? 1 : 0);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// pcp_place_coverage's checks on the pair call's struct; cp: the same arguments as that call's
int check_pair_args(pcp_ctx *ctx, const char *what, const double *poses, uint64_t n,
                    const pcp_fan_params *fan, bool mounted, const double *el_table,
                    const pcp_pair_params *pp, const uint8_t *roi, uint64_t roi_n, CoverFixed &fx,
                    uint64_t *N_out) {
    if (!pp) return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    if (pp->reserved != 0) return set_err(ctx, PCP_E_INVALID, "%s: reserved != 0", what);
    pcp_cover_params cp{};
    cp.k_max = 1;
    cp.n_fixed = pp->n_fixed;
    cp.min_separation = pp->min_separation;
    std::memcpy(cp.fixed, pp->fixed, sizeof cp.fixed);
    return check_args(ctx, what, poses, n, fan, mounted, el_table, &cp, roi, roi_n, fx, N_out);
}

}  // namespace
}  // namespace pcp

using namespace pcp;

// pcp_place_coverage_pair and, mounted (poses: poses6 rows, el_table nullable), its mounted twin
static int place_coverage_pair_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                    const pcp_fan_params *fan, bool mounted,
                                    const double *el_table, const pcp_pair_params *pp,
                                    const uint8_t *roi, uint64_t roi_n, int64_t best_pair[2],
                                    uint64_t *pair_gain, int64_t *best_single,
                                    uint64_t *single_gain, int64_t *single_gains,
                                    int64_t *pair_gains, int64_t *partner, int64_t *partner_gain,
                                    uint32_t *seen_points, int32_t *point_owner,
                                    uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                                    uint64_t *base_covered, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_pair_mounted" : "pcp_place_coverage_pair";
    if (!best_pair || !pair_gain || !best_single || !single_gain || !n_points || !roi_points ||
        !base_covered || !n_selected)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    CoverFixed fx{};
    uint64_t N = 0;
    if (int rc = check_pair_args(ctx, what, poses, n, fan, mounted, el_table, pp, roi, roi_n, fx, &N))
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
        best_pair[0] = best_pair[1] = *best_single = -1;
        *pair_gain = *single_gain = 0;
        for (uint64_t i = 0; point_owner && i < N; ++i) point_owner[i] = PCP_OWNER_NONE;
        for (uint64_t p = 0; p < n; ++p) {
            if (seen_points) seen_points[p] = 0u;
            if (single_gains) single_gains[p] = -1;
            if (partner) partner[p] = -1;
            if (partner_gain) partner_gain[p] = -1;
        }
        for (uint64_t i = 0; pair_gains && i < n * n; ++i) pair_gains[i] = -1;
        return PCP_OK;
    }
    // the production fan query: first hits and the live waves stay on the device
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const CPairPlan q =
        make_pair_plan((int)n, N, point_owner != nullptr, roi != nullptr, pair_gains != nullptr);
    const CoverPlan &c = q.c;
    PCP_HIP(ctx, ctx->cpair_d.ensure(q.bytes));
    PCP_HIP(ctx, ctx->cpair_host.ensure(q.pin_bytes));
    char *blk = ctx->cpair_d.as<char>();
    char *pin = ctx->cpair_host.as<char>();
    const CoverDev d = dev_of(blk, c);
    const CPairDev e = pair_dev_of(blk, q);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(pp->min_separation);
    if (int rc = build_enqueue(ctx, c, d, fan, o, fx, sep2)) return rc;
    // the fixed sensors, in list order: need becomes need0
    for (int i = 0; i < fx.n; ++i)
        if (int rc = commit_enqueue(ctx, c, d, fx.idx[i], i, 0)) return rc;
    {
        ProfScope ps(ctx, PCP_K_PLACE);
        if (int rc = mask_enqueue(ctx, c, d, false)) return rc;
        if (int rc = pairs_enqueue(ctx, q, d, e, o, sep2, pair_gains != nullptr, true)) return rc;
    }
    // the answer's poses, a and then b, by the rounds' own commit
    for (int r = 0; r < 2; ++r)
        if (int rc = commit_enqueue(ctx, c, d, -1, fx.n + r, r)) return rc;
    // downloads: the state and the counts, the result with the singles and the partners, the
    // table and the owners when asked for
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, c.rg_off, hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipMemcpyAsync(pin + q.pin_out, blk + q.out_off, q.x_off - q.out_off,
                                hipMemcpyDeviceToHost, st));
    if (q.table)
        if (int rc = copy_to_pinned_async(ctx, pin + q.pin_tab, blk + q.tab_off,
                                          (size_t)n * n * sizeof(int64_t), st))
            return rc;
    if (c.owner)
        if (int rc = copy_to_pinned_async(ctx, pin + q.pin_own, blk + c.own_off,
                                          (size_t)N * sizeof(int32_t), st))
            return rc;
    if (int rc = stream_done(ctx)) return rc;
    const CoverState *h = reinterpret_cast<const CoverState *>(pin);
    const CPairOut *po = reinterpret_cast<const CPairOut *>(pin + q.pin_out);
    const size_t row = (size_t)n * sizeof(int64_t);
    best_pair[0] = po->pair[0];
    best_pair[1] = po->pair[1];
    *pair_gain = po->pair_gain;
    *best_single = po->single;
    *single_gain = po->single_gain;
    if (single_gains) std::memcpy(single_gains, pin + q.pin_out + (q.sg_off - q.out_off), row);
    if (partner) std::memcpy(partner, pin + q.pin_out + (q.pt_off - q.out_off), row);
    if (partner_gain) std::memcpy(partner_gain, pin + q.pin_out + (q.pg_off - q.out_off), row);
    if (pair_gains) host_copy(ctx, pair_gains, pin + q.pin_tab, (size_t)n * n * sizeof(int64_t));
    if (seen_points) std::memcpy(seen_points, pin + c.sp_off, (size_t)n * sizeof(uint32_t));
    if (point_owner) host_copy(ctx, point_owner, pin + q.pin_own, (size_t)N * sizeof(int32_t));
    *roi_points = h->roi_points;
    *base_covered = h->base_covered;
    *n_selected = h->n_sel;
    return PCP_OK;
}

extern "C" int pcp_place_coverage_pair(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                       const pcp_fan_params *fan, const pcp_pair_params *pp,
                                       const uint8_t *roi, uint64_t roi_n, int64_t best_pair[2],
                                       uint64_t *pair_gain, int64_t *best_single,
                                       uint64_t *single_gain, int64_t *single_gains,
                                       int64_t *pair_gains, int64_t *partner,
                                       int64_t *partner_gain, uint32_t *seen_points,
                                       int32_t *point_owner, uint64_t owner_cap,
                                       uint64_t *n_points, uint64_t *roi_points,
                                       uint64_t *base_covered, int32_t *n_selected) {
    return place_coverage_pair_impl(ctx, poses5, n, fan, false, nullptr, pp, roi, roi_n, best_pair,
                                    pair_gain, best_single, single_gain, single_gains, pair_gains,
                                    partner, partner_gain, seen_points, point_owner, owner_cap,
                                    n_points, roi_points, base_covered, n_selected);
}

extern "C" int pcp_place_coverage_pair_mounted(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_pair_params *pp, const uint8_t *roi, uint64_t roi_n,
    int64_t best_pair[2], uint64_t *pair_gain, int64_t *best_single, uint64_t *single_gain,
    int64_t *single_gains, int64_t *pair_gains, int64_t *partner, int64_t *partner_gain,
    uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
    uint64_t *roi_points, uint64_t *base_covered, int32_t *n_selected) {
    return place_coverage_pair_impl(ctx, poses6, n, fan, true, el_table, pp, roi, roi_n, best_pair,
                                    pair_gain, best_single, single_gain, single_gains, pair_gains,
                                    partner, partner_gain, seen_points, point_owner, owner_cap,
                                    n_points, roi_points, base_covered, n_selected);
}

static int place_coverage_pair_burst_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                          const pcp_fan_params *fan, bool mounted,
                                          const double *el_table, const pcp_pair_params *pp,
                                          const uint8_t *roi, uint64_t roi_n, int reps,
                                          double ms[2]) {
    if (!ctx) return PCP_E_INVALID;
    const char *what =
        mounted ? "pcp_place_coverage_pair_mounted_burst" : "pcp_place_coverage_pair_burst";
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument or nothing to time", what);
    CoverFixed fx{};
    uint64_t N = 0;
    if (int rc = check_pair_args(ctx, what, poses, n, fan, mounted, el_table, pp, roi, roi_n, fx, &N))
        return rc;
    if (N == 0) return set_err(ctx, PCP_E_INVALID, "%s: no terrain index, nothing to time", what);
    ms[0] = ms[1] = 0.0;
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const CPairPlan q = make_pair_plan((int)n, N, false, roi != nullptr, false);
    const CoverPlan &c = q.c;
    PCP_HIP(ctx, ctx->cpair_d.ensure(q.bytes));
    char *blk = ctx->cpair_d.as<char>();
    const CoverDev d = dev_of(blk, c);
    const CPairDev e = pair_dev_of(blk, q);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(pp->min_separation);
    if (int rc = build_enqueue(ctx, c, d, fan, o, fx, sep2)) return rc;
    for (int i = 0; i < fx.n; ++i)
        if (int rc = commit_enqueue(ctx, c, d, fx.idx[i], i, 0)) return rc;
    // (the mask is idempotent: a repetition finds the rows masked and counts them again)
    auto mask = [&] { return mask_enqueue(ctx, c, d, true); };
    if (int rc = time_reps(ctx, what, st, reps, mask, mask, &ms[0])) return rc;
    auto pairs = [&] { return pairs_enqueue(ctx, q, d, e, o, sep2, false, false); };
    return time_reps(ctx, what, st, reps, pairs, pairs, &ms[1]);
}

extern "C" int pcp_place_coverage_pair_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                             const pcp_fan_params *fan, const pcp_pair_params *pp,
                                             const uint8_t *roi, uint64_t roi_n, int reps,
                                             double ms[2]) {
    return place_coverage_pair_burst_impl(ctx, poses5, n, fan, false, nullptr, pp, roi, roi_n, reps,
                                          ms);
}

extern "C" int pcp_place_coverage_pair_mounted_burst(pcp_ctx *ctx, const double *poses6,
                                                     uint64_t n, const pcp_fan_params *fan,
                                                     const double *el_table,
                                                     const pcp_pair_params *pp, const uint8_t *roi,
                                                     uint64_t roi_n, int reps, double ms[2]) {
    return place_coverage_pair_burst_impl(ctx, poses6, n, fan, true, el_table, pp, roi, roi_n, reps,
                                          ms);
}
