// pcp_cover_refine.hip -- pcp_place_coverage_refine on gfx950: a set of mobile sensors improved by
// single-sensor exchanges, scored by the terrain their scans reach.  The bitsets
// are pcp_place_coverage's own (pcp_cover_phase.hpp), in a block of this call's.  Behind them one
// evaluation is two launches.  With s the set, any = the union of its rows, multi = the points two
// slots or more reach:
//   k_crefine_prep   the k + 1 class rows Z = R & ~any and E_i = R & seen[s_i] & ~multi (the points
//                    of R only slot i reaches), their counts |E_i| and T = |R & any|;
//   k_crefine_eval   z[p] = |seen(p) & Z| and e[i][p] = |seen(p) & E_i| for every pose: a wave
//                    keeps eight poses' words in registers and streams the class rows past them,
//                    so a pose's row is read once per evaluation, not once per slot.  The
//                    launch's last block forms u[i][p] = T - |E_i| + z[p] + e[i][p] (Z and the E_i
//                    are pairwise disjoint: the identity is exact) under the admissibility and
//                    separation masks, takes the first maximum in row-major order, and appends
//                    the move and updates s on the device, or stops the search.
// max_moves + 1 such pairs are enqueued up front and ordered by the stream alone; behind the stop
// each returns at once.  No block ever waits for another.  Every count is an integer below 2^32:
// exact, deterministic whatever the order of the atomic additions.
#pragma clang fp contract(off)

#include "pcp_cover_phase.hpp"

namespace pcp {
namespace {

constexpr int kEP = 8;               // poses per block of an evaluation (k_cover_round's shape)
constexpr int kEL = 2;               // 16-byte loads per lane and row: four words per lane
constexpr uint32_t kEWave = 64 * 2 * kEL;      // words a wave holds of each of its poses
constexpr uint32_t kEBlock = kEWave * kCW;     // words per block chunk
constexpr int kAcc = PCP_PLACE_MAX + 2;        // |E_i|, T and a pad: a whole number of 16 bytes

// the call's state (downloaded); acc = the preparation's counts |E_0| .. |E_k-1| and, at [k], T
struct CRefState {
    int32_t n_moves, done, converged, k;
    uint32_t ticket, pad[3];
    unsigned long long T, start_T;
    int64_t set[PCP_PLACE_MAX];
    unsigned long long uniq[PCP_PLACE_MAX];
    unsigned long long acc[kAcc];
    int32_t move_slot[PCP_REFINE_MAX_MOVES];
    int64_t move_from[PCP_REFINE_MAX_MOVES], move_to[PCP_REFINE_MAX_MOVES];
    unsigned long long move_cov[PCP_REFINE_MAX_MOVES];
};
static_assert(sizeof(CRefState) % 16 == 0, "the tables follow on a 16-byte boundary");

struct CRefStart {
    int32_t k;
    int32_t idx[PCP_PLACE_MAX];
};

// the state reset, s = start, the counts and the evaluation's sums zero
__global__ void __launch_bounds__(kCT)
k_crefine_init(CRefState *__restrict__ s, CRefStart st, uint32_t *__restrict__ tab,
               unsigned long long n_tab) {
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kCT + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kCT;
    for (unsigned long long i = t0; i < n_tab; i += stride) tab[i] = 0u;
    if (t0 >= (unsigned long long)kAcc) return;
    s->acc[t0] = 0ull;
    if (t0 < PCP_PLACE_MAX) {
        s->set[t0] = (int)t0 < st.k ? st.idx[t0] : -1;
        s->uniq[t0] = 0ull;
    }
    if (t0 == 0) {
        s->n_moves = 0;
        s->done = 0;
        s->converged = 0;
        s->k = st.k;
        s->ticket = 0u;
        s->T = s->start_T = 0ull;
    }
}

// The preparation.  One lane per word: R's word and the k rows seen[s_j] (s from device memory),
// any |= row, multi |= any & row; Z and every E_i written (each word of each class row has this
// one writer), |E_i| and T added with one atomic per wave.  Returns at once behind the stop.
__global__ void __launch_bounds__(kCT)
k_crefine_prep(const unsigned long long *__restrict__ seen,
               const unsigned long long *__restrict__ need, uint32_t W2, int k, CRefState *s,
               unsigned long long *__restrict__ cls) {
    if (s->done) return;   // (uniform)
    const uint32_t gw = blockIdx.x * kCT + threadIdx.x;
    const bool in = gw < W2;
    const unsigned long long R = in ? need[gw] : 0ull;
    unsigned long long any = 0ull, multi = 0ull;
    for (int j = 0; j < k; ++j) {
        const unsigned long long row = in ? seen[(size_t)s->set[j] * W2 + gw] : 0ull;
        multi |= any & row;
        any |= row;
    }
    if (in) cls[gw] = R & ~any;
    const uint32_t lane = threadIdx.x & 63u;
    for (int j = 0; j <= k; ++j) {
        unsigned long long e = R & any;   // (j == k: the covered points)
        if (j < k) {
            e = in ? R & seen[(size_t)s->set[j] * W2 + gw] & ~multi : 0ull;
            if (in) cls[(size_t)(1 + j) * W2 + gw] = e;
        }
        uint32_t c = (uint32_t)__popcll(e);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0 && c) atomicAdd(&s->acc[j], (unsigned long long)c);
    }
}

// a wave's sums of eight values per lane, transposed as they fold: three exchanges halve the
// values a lane carries, three more finish the one left.  Lane L with L % 8 == 0 returns the
// wave's sum of v[L / 8]; the other lanes' returns mean nothing.
__device__ __forceinline__ uint32_t wave_sum8(const uint32_t (&v)[kEP], uint32_t lane) {
    uint32_t a[4], b[2];
    const bool h5 = (lane & 32u) != 0u, h4 = (lane & 16u) != 0u, h3 = (lane & 8u) != 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        a[j] = (h5 ? v[j + 4] : v[j]) + __shfl_xor(h5 ? v[j] : v[j + 4], 32, 64);
#pragma unroll
    for (int j = 0; j < 2; ++j)
        b[j] = (h4 ? a[j + 2] : a[j]) + __shfl_xor(h4 ? a[j] : a[j + 2], 16, 64);
    uint32_t c = (h3 ? b[1] : b[0]) + __shfl_xor(h3 ? b[0] : b[1], 8, 64);
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}
static_assert(kEP == 8, "wave_sum8 folds eight poses");

// One evaluation.  Block = (word chunk, pose group): blockIdx.x = group * nchunks + chunk.  A wave
// holds its kEWave words of its group's kEP poses in registers (kEP x four words per lane) and
// streams Z and the rows E_i of the slots that may move past them: AND + population count, one
// transposed wave reduction per class row, one integer atomic per (wave, class, pose) with a
// non-zero sum into tab [k + 1][n].  A class row whose words are zero across the wave is skipped
// (wave-uniform).
//
// The last block to draw the ticket does the rest: u under the masks (slot i locked; p in s; with
// a separation p closer than it to some s_j, j != i), the evaluation's table when asked for, the
// first maximum in row-major order against T, and the move or the stop.  It leaves tab zero for
// the next evaluation.  commit false (the timing entry): the selection is made, nothing recorded.
__global__ void __launch_bounds__(kCT)
k_crefine_eval(const unsigned long long *__restrict__ seen,
               const unsigned long long *__restrict__ cls, uint32_t W2, int n, int k, int n_locked,
               int max_moves, uint32_t *tab, CRefState *s, CoverState *cs,
               const double *__restrict__ pose, uint32_t row, double sep2, int e,
               uint32_t nchunks, int64_t *__restrict__ table, int commit) {
    __shared__ RowBest s_best[kCW];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = s->done;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier evaluation stopped the search
    const uint32_t lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % nchunks, grp = blockIdx.x / nchunks;
    const uint32_t wb = chunk * kEBlock + (uint32_t)(tid >> 6) * kEWave + lane * 2u;
    ulonglong2 pw[kEP][kEL];
    bool some = false;
#pragma unroll
    for (int q = 0; q < kEP; ++q) {
        const uint32_t p = grp * kEP + (uint32_t)q;
        const ulonglong2 *row2 = reinterpret_cast<const ulonglong2 *>(seen + (size_t)p * W2);
#pragma unroll
        for (int j = 0; j < kEL; ++j) {
            const uint32_t wi = wb + (uint32_t)j * 128u;   // (W2 is even: a pair is inside or outside)
            pw[q][j] = p < (uint32_t)n && wi < W2 ? row2[wi >> 1] : make_ulonglong2(0ull, 0ull);
            some |= (pw[q][j].x | pw[q][j].y) != 0ull;
        }
    }
    if (__ballot(some)) {   // (wave-uniform) poses that reach nothing here add nothing
        for (int c = 0; c <= k; c = c ? c + 1 : 1 + n_locked) {
            const ulonglong2 *c2 = reinterpret_cast<const ulonglong2 *>(cls + (size_t)c * W2);
            ulonglong2 cw[kEL];
            bool live = false;
#pragma unroll
            for (int j = 0; j < kEL; ++j) {
                const uint32_t wi = wb + (uint32_t)j * 128u;
                cw[j] = wi < W2 ? c2[wi >> 1] : make_ulonglong2(0ull, 0ull);
                live |= (cw[j].x | cw[j].y) != 0ull;
            }
            if (!__ballot(live)) continue;   // (wave-uniform)
            uint32_t cnt[kEP];
#pragma unroll
            for (int q = 0; q < kEP; ++q) {
                cnt[q] = 0u;
#pragma unroll
                for (int j = 0; j < kEL; ++j)
                    cnt[q] += (uint32_t)(__popcll(pw[q][j].x & cw[j].x) +
                                         __popcll(pw[q][j].y & cw[j].y));
            }
            const uint32_t sum = wave_sum8(cnt, lane);
            const uint32_t p = grp * kEP + (lane >> 3);
            if ((lane & 7u) == 0u && sum && p < (uint32_t)n) atomicAdd(&tab[(size_t)c * n + p], sum);
        }
    }
    // the evaluation's ticket: this block's sums added before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the evaluation ---------------------------------------------------
    // (a count is below 2^32: exact as a double, so the shared first-maximum reduction serves)
    const unsigned long long T = s->acc[k];
    double t = -1.0;
    int ba = -1, bb = -1;
    for (int p = tid; p < n; p += kCT) {
        uint32_t close = 0u;
        bool in_s = false;
        for (int j = 0; j < k; ++j) {
            const int sj = (int)s->set[j];
            in_s |= sj == p;
            if (sep2 > 0 && cover_closer(pose, row, p, sj, sep2)) close |= 1u << j;
        }
        const long long z =
            (long long)__hip_atomic_load(&tab[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tab[p] = 0u;
        for (int i = 0; i < k; ++i) {
            long long u = -1ll;
            if (i >= n_locked) {
                uint32_t *cell = &tab[(size_t)(1 + i) * n + p];
                const long long ei =
                    (long long)__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *cell = 0u;
                if (!in_s && (close & ~(1u << i)) == 0u) {
                    u = (long long)T - (long long)s->acc[i] + z + ei;
                    take_ahead(t, ba, bb, (double)u, i, p);
                }
            }
            if (table) table[((size_t)e * k + i) * n + p] = u;
        }
    }
    block_first_max_all<kCW>(s_best, t, ba, bb);
    if (tid != 0) return;
    s->ticket = 0u;   // (the next launch draws from zero)
    if (!commit) return;
    if (e == 0) s->start_T = T;
    s->T = T;
    for (int i = 0; i < k; ++i) s->uniq[i] = s->acc[i];
    for (int i = 0; i <= k; ++i) s->acc[i] = 0ull;   // (the next preparation adds from zero)
    const int nm = s->n_moves;
    const bool better = ba >= 0 && t > (double)T;
    if (better && nm < max_moves) {
        s->move_slot[nm] = ba;
        s->move_from[nm] = s->set[ba];
        s->move_to[nm] = bb;
        s->move_cov[nm] = (unsigned long long)t;
        s->set[ba] = bb;
        s->T = (unsigned long long)t;
        s->n_moves = nm + 1;
        return;
    }
    // the stop: the set stands as the last preparation saw it (uniq is the answer's), and the
    // owners' commits read it as k recorded rounds
    s->converged = better ? 0 : 1;
    s->done = 1;
    for (int i = 0; i < k; ++i) cs->sel[i] = s->set[i];
    cs->n_sel = k;
}

// the call's device block: the plan's block (one row of gains, not used), then [state | tab u32
// (k + 1) x n | class rows u64 (k + 1) x W2 | dense tables i64 (max_moves + 1) x k x n]
struct CRefPlan {
    CoverPlan c;
    int k = 0, n_locked = 0, max_moves = 0;
    bool table = false;
    size_t st_off = 0, tab_off = 0, cls_off = 0, den_off = 0, den_bytes = 0, bytes = 0;
    // the pinned landing: [cover state .. gains) | state | dense tables | owners
    size_t pin_st = 0, pin_den = 0, pin_own = 0, pin_bytes = 0;
};

CRefPlan make_refine_plan(int n, uint64_t N, const pcp_refine_params *rp, bool owner, bool roi,
                          bool table) {
    CRefPlan q;
    q.c = make_plan(n, 1, N, owner, roi);
    q.k = rp->k;
    q.n_locked = rp->n_locked;
    q.max_moves = rp->max_moves;
    q.table = table;
    q.st_off = a16(q.c.bytes);
    q.tab_off = a16(q.st_off + sizeof(CRefState));
    q.cls_off = a16(q.tab_off + (size_t)(q.k + 1) * n * sizeof(uint32_t));
    q.den_off = a16(q.cls_off + (size_t)(q.k + 1) * q.c.W2 * sizeof(uint64_t));
    q.den_bytes = table ? (size_t)(q.max_moves + 1) * q.k * n * sizeof(int64_t) : 0;
    q.bytes = q.den_off + q.den_bytes + 64;
    q.pin_st = a16(q.c.rg_off);
    q.pin_den = a16(q.pin_st + sizeof(CRefState));
    q.pin_own = a16(q.pin_den + q.den_bytes);
    q.pin_bytes = q.pin_own + (owner ? (size_t)N * sizeof(int32_t) : 0) + 64;
    return q;
}

struct CRefDev {
    CRefState *s;
    uint32_t *tab;
    unsigned long long *cls;
    int64_t *table;
};

CRefDev refine_dev_of(char *blk, const CRefPlan &q) {
    CRefDev e;
    e.s = reinterpret_cast<CRefState *>(blk + q.st_off);
    e.tab = reinterpret_cast<uint32_t *>(blk + q.tab_off);
    e.cls = reinterpret_cast<unsigned long long *>(blk + q.cls_off);
    e.table = q.table ? reinterpret_cast<int64_t *>(blk + q.den_off) : nullptr;
    return e;
}

int init_enqueue(pcp_ctx *ctx, const CRefPlan &q, const CRefDev &e, const CRefStart &start) {
    const unsigned long long n_tab = (unsigned long long)(q.k + 1) * q.c.n;
    hipLaunchKernelGGL(k_crefine_init, dim3((unsigned)((n_tab + kCT - 1) / kCT)), dim3(kCT), 0,
                       ctx->stream, e.s, start, e.tab, n_tab);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// clear_acc: the counts are zeroed first (a repetition of the timing entry: within the call the
// evaluation before leaves them zero)
int prep_enqueue(pcp_ctx *ctx, const CRefPlan &q, const CoverDev &d, const CRefDev &e,
                 bool clear_acc) {
    if (clear_acc)
        PCP_HIP(ctx, hipMemsetAsync(e.s->acc, 0, sizeof(e.s->acc), ctx->stream));
    hipLaunchKernelGGL(k_crefine_prep, dim3((q.c.W2 + kCT - 1) / kCT), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, (const unsigned long long *)d.need,
                       q.c.W2, q.k, e.s, e.cls);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

int eval_enqueue(pcp_ctx *ctx, const CRefPlan &q, const CoverDev &d, const CRefDev &e,
                 const FanEnq &o, double sep2, int ev, bool commit) {
    const uint32_t nchunks = (q.c.W2 + kEBlock - 1) / kEBlock;
    const uint32_t groups = ((uint32_t)q.c.n + kEP - 1) / kEP;
    hipLaunchKernelGGL(k_crefine_eval, dim3(nchunks * groups), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, (const unsigned long long *)e.cls,
                       q.c.W2, q.c.n, q.k, q.n_locked, q.max_moves, e.tab, e.s, d.s,
                       ctx->poses_d.as<const double>(), o.pose_row, sep2, ev, nchunks,
                       commit ? e.table : nullptr, commit ? 1 : 0);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what both entries refuse before any launch (ctx non-null): pcp_place_coverage's checks of the
// fan, the poses and the region, pcp_place_refine's of rp; start = the set as the kernels take it
int check_refine_args(pcp_ctx *ctx, const char *what, const double *poses, uint64_t n,
                      const pcp_fan_params *fan, bool mounted, const double *el_table,
                      const pcp_refine_params *rp, const uint8_t *roi, uint64_t roi_n,
                      CRefStart &start, uint64_t *N_out) {
    if (!rp) return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    pcp_cover_params cp{};
    cp.k_max = 1;
    CoverFixed fx{};
    if (int rc = check_args(ctx, what, poses, n, fan, mounted, el_table, &cp, roi, roi_n, fx, N_out))
        return rc;
    if (rp->k < 1 || rp->k > PCP_PLACE_MAX || rp->n_locked < 0 || rp->n_locked > rp->k ||
        rp->max_moves < 0 || rp->max_moves > PCP_REFINE_MAX_MOVES || rp->reserved != 0)
        return set_err(ctx, PCP_E_INVALID,
                       "%s: k %d outside 1..%d, n_locked %d outside 0..k, max_moves %d outside "
                       "0..%d or reserved %d != 0",
                       what, (int)rp->k, PCP_PLACE_MAX, (int)rp->n_locked, (int)rp->max_moves,
                       PCP_REFINE_MAX_MOVES, (int)rp->reserved);
    int i = 0;
    const int bad = check_index_list(rp->start, rp->k, n, &i);
    if (bad == kListRange)
        return set_err(ctx, PCP_E_INVALID, "%s: start[%d] = %lld is no pose of %llu", what, i,
                       (long long)rp->start[i], (unsigned long long)n);
    if (bad == kListTwice)
        return set_err(ctx, PCP_E_INVALID, "%s: pose %lld is in the set twice", what,
                       (long long)rp->start[i]);
    start.k = rp->k;
    for (i = 0; i < PCP_PLACE_MAX; ++i) start.idx[i] = i < rp->k ? (int32_t)rp->start[i] : 0;
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

// pcp_place_coverage_refine and, mounted (poses: poses6 rows, el_table nullable), its mounted twin
static int place_coverage_refine_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                      const pcp_fan_params *fan, bool mounted,
                                      const double *el_table, const pcp_refine_params *rp,
                                      const uint8_t *roi, uint64_t roi_n, int64_t *selected,
                                      uint64_t *covered, uint64_t *start_covered,
                                      int32_t *move_slot, int64_t *move_from, int64_t *move_to,
                                      uint64_t *move_covered, int64_t *swap_covered,
                                      uint64_t *slot_unique, uint32_t *seen_points,
                                      int32_t *point_owner, uint64_t owner_cap,
                                      uint64_t *n_points, uint64_t *roi_points, int32_t *n_moves,
                                      int32_t *converged) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_refine_mounted" : "pcp_place_coverage_refine";
    if (!selected || !covered || !start_covered || !n_points || !roi_points || !n_moves ||
        !converged)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    CRefStart start{};
    uint64_t N = 0;
    if (int rc = check_refine_args(ctx, what, poses, n, fan, mounted, el_table, rp, roi, roi_n,
                                   start, &N))
        return rc;
    if (rp->max_moves > 0 && (!move_slot || !move_from || !move_to || !move_covered))
        return set_err(ctx, PCP_E_INVALID, "%s: null move array", what);
    if (point_owner && owner_cap < N) {
        *n_points = N;
        return set_err(ctx, PCP_E_CAPACITY, "%s: owners of %llu points, cap %llu", what,
                       (unsigned long long)N, (unsigned long long)owner_cap);
    }
    const int K = rp->k;
    *n_points = N;
    if (N == 0) {   // nothing to cover, nothing to gain
        for (int i = 0; i < K; ++i) selected[i] = rp->start[i];
        for (int i = 0; slot_unique && i < K; ++i) slot_unique[i] = 0;
        for (uint64_t p = 0; seen_points && p < n; ++p) seen_points[p] = 0u;
        *covered = *start_covered = *roi_points = 0;
        *n_moves = 0;
        *converged = 1;
        return PCP_OK;
    }
    // the production fan query: first hits and the live waves stay on the device
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const CRefPlan q = make_refine_plan((int)n, N, rp, point_owner != nullptr, roi != nullptr,
                                        swap_covered != nullptr);
    const CoverPlan &c = q.c;
    PCP_HIP(ctx, ctx->crefine_d.ensure(q.bytes));
    PCP_HIP(ctx, ctx->crefine_host.ensure(q.pin_bytes));
    char *blk = ctx->crefine_d.as<char>();
    char *pin = ctx->crefine_host.as<char>();
    const CoverDev d = dev_of(blk, c);
    const CRefDev e = refine_dev_of(blk, q);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(rp->min_separation);
    const CoverFixed none{};
    if (int rc = build_enqueue(ctx, c, d, fan, o, none, sep2)) return rc;
    {
        ProfScope ps(ctx, PCP_K_PLACE);
        if (int rc = init_enqueue(ctx, q, e, start)) return rc;
        // every evaluation the moves allow, back to back: those behind the stop return at once
        for (int ev = 0; ev <= q.max_moves; ++ev) {
            if (int rc = prep_enqueue(ctx, q, d, e, false)) return rc;
            if (int rc = eval_enqueue(ctx, q, d, e, o, sep2, ev, true)) return rc;
        }
    }
    // the owners: the final set's slots in order by the rounds' own commit (need is R until here)
    for (int i = 0; c.owner && i < K; ++i)
        if (int rc = commit_enqueue(ctx, c, d, -1, i, i)) return rc;
    // downloads: the counts, the state, the tables and the owners when asked for
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, c.rg_off, hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipMemcpyAsync(pin + q.pin_st, blk + q.st_off, sizeof(CRefState),
                                hipMemcpyDeviceToHost, st));
    if (q.table)
        if (int rc = copy_to_pinned_async(ctx, pin + q.pin_den, blk + q.den_off, q.den_bytes, st))
            return rc;
    if (c.owner)
        if (int rc = copy_to_pinned_async(ctx, pin + q.pin_own, blk + c.own_off,
                                          (size_t)N * sizeof(int32_t), st))
            return rc;
    if (int rc = stream_done(ctx)) return rc;
    const CoverState *hc = reinterpret_cast<const CoverState *>(pin);
    const CRefState *h = reinterpret_cast<const CRefState *>(pin + q.pin_st);
    const int nm = h->n_moves;
    for (int i = 0; i < K; ++i) selected[i] = h->set[i];
    *covered = h->T;
    *start_covered = h->start_T;
    for (int m = 0; m < nm; ++m) {
        move_slot[m] = h->move_slot[m];
        move_from[m] = h->move_from[m];
        move_to[m] = h->move_to[m];
        move_covered[m] = h->move_cov[m];
    }
    if (swap_covered)
        host_copy(ctx, swap_covered, pin + q.pin_den, (size_t)(nm + 1) * K * n * sizeof(int64_t));
    for (int i = 0; slot_unique && i < K; ++i) slot_unique[i] = h->uniq[i];
    if (seen_points) std::memcpy(seen_points, pin + c.sp_off, (size_t)n * sizeof(uint32_t));
    if (point_owner) host_copy(ctx, point_owner, pin + q.pin_own, (size_t)N * sizeof(int32_t));
    *roi_points = hc->roi_points;
    *n_moves = nm;
    *converged = h->converged;
    return PCP_OK;
}

extern "C" int pcp_place_coverage_refine(
    pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
    const pcp_refine_params *rp, const uint8_t *roi, uint64_t roi_n, int64_t *selected,
    uint64_t *covered, uint64_t *start_covered, int32_t *move_slot, int64_t *move_from,
    int64_t *move_to, uint64_t *move_covered, int64_t *swap_covered, uint64_t *slot_unique,
    uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
    uint64_t *roi_points, int32_t *n_moves, int32_t *converged) {
    return place_coverage_refine_impl(ctx, poses5, n, fan, false, nullptr, rp, roi, roi_n, selected,
                                      covered, start_covered, move_slot, move_from, move_to,
                                      move_covered, swap_covered, slot_unique, seen_points,
                                      point_owner, owner_cap, n_points, roi_points, n_moves,
                                      converged);
}

extern "C" int pcp_place_coverage_refine_mounted(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_refine_params *rp, const uint8_t *roi, uint64_t roi_n,
    int64_t *selected, uint64_t *covered, uint64_t *start_covered, int32_t *move_slot,
    int64_t *move_from, int64_t *move_to, uint64_t *move_covered, int64_t *swap_covered,
    uint64_t *slot_unique, uint32_t *seen_points, int32_t *point_owner, uint64_t owner_cap,
    uint64_t *n_points, uint64_t *roi_points, int32_t *n_moves, int32_t *converged) {
    return place_coverage_refine_impl(ctx, poses6, n, fan, true, el_table, rp, roi, roi_n, selected,
                                      covered, start_covered, move_slot, move_from, move_to,
                                      move_covered, swap_covered, slot_unique, seen_points,
                                      point_owner, owner_cap, n_points, roi_points, n_moves,
                                      converged);
}

static int place_coverage_refine_burst_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                            const pcp_fan_params *fan, bool mounted,
                                            const double *el_table, const pcp_refine_params *rp,
                                            const uint8_t *roi, uint64_t roi_n, int reps,
                                            double ms[2]) {
    if (!ctx) return PCP_E_INVALID;
    const char *what =
        mounted ? "pcp_place_coverage_refine_mounted_burst" : "pcp_place_coverage_refine_burst";
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument or nothing to time", what);
    CRefStart start{};
    uint64_t N = 0;
    if (int rc = check_refine_args(ctx, what, poses, n, fan, mounted, el_table, rp, roi, roi_n,
                                   start, &N))
        return rc;
    if (N == 0) return set_err(ctx, PCP_E_INVALID, "%s: no terrain index, nothing to time", what);
    ms[0] = ms[1] = 0.0;
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const CRefPlan q = make_refine_plan((int)n, N, rp, false, roi != nullptr, false);
    const CoverPlan &c = q.c;
    PCP_HIP(ctx, ctx->crefine_d.ensure(q.bytes));
    char *blk = ctx->crefine_d.as<char>();
    const CoverDev d = dev_of(blk, c);
    const CRefDev e = refine_dev_of(blk, q);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    const double sep2 = sep2_of(rp->min_separation);
    const CoverFixed none{};
    if (int rc = build_enqueue(ctx, c, d, fan, o, none, sep2)) return rc;
    if (int rc = init_enqueue(ctx, q, e, start)) return rc;
    // the start set's preparation, its counts cleared before each repetition; then its evaluation:
    // nothing is committed and the last block leaves the sums zero, so every repetition does the
    // whole work of a live evaluation on the counts the last preparation left
    auto prep = [&] { return prep_enqueue(ctx, q, d, e, true); };
    if (int rc = time_reps(ctx, what, st, reps, prep, prep, &ms[0])) return rc;
    auto eval = [&] { return eval_enqueue(ctx, q, d, e, o, sep2, 0, false); };
    return time_reps(ctx, what, st, reps, eval, eval, &ms[1]);
}

extern "C" int pcp_place_coverage_refine_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                               const pcp_fan_params *fan,
                                               const pcp_refine_params *rp, const uint8_t *roi,
                                               uint64_t roi_n, int reps, double ms[2]) {
    return place_coverage_refine_burst_impl(ctx, poses5, n, fan, false, nullptr, rp, roi, roi_n,
                                            reps, ms);
}

extern "C" int pcp_place_coverage_refine_mounted_burst(pcp_ctx *ctx, const double *poses6,
                                                       uint64_t n, const pcp_fan_params *fan,
                                                       const double *el_table,
                                                       const pcp_refine_params *rp,
                                                       const uint8_t *roi, uint64_t roi_n, int reps,
                                                       double ms[2]) {
    return place_coverage_refine_burst_impl(ctx, poses6, n, fan, true, el_table, rp, roi, roi_n,
                                            reps, ms);
}
