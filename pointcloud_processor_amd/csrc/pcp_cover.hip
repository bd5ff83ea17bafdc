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
// The bitsets' phase and the commit are pcp_cover_phase.hpp's, shared with pcp_cover_pair.hip.
#pragma clang fp contract(off)

#include "pcp_cover_phase.hpp"

namespace pcp {
namespace {

constexpr int kRP = 8;               // poses per block of a round
constexpr int kRL = 2;               // 16-byte loads per lane and row: four words per lane
constexpr uint32_t kRWave = 64 * 2 * kRL;      // words of `need` a wave holds
constexpr uint32_t kRBlock = kRWave * kCW;     // words per block chunk

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
    const CoverDev d = dev_of(ctx->cover_d.as<char>(), c);
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
    const CoverDev d = dev_of(ctx->cover_d.as<char>(), c);
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
