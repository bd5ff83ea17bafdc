// pcp_place.hip -- greedy multi-sensor pose selection (pcp_place_sensors): runOptimization's
// "best of one" (virtual_lidar.cpp:460-475 over evaluatePosition :627-654) generalised to K
// sensors.  A cell's combined score is the max over zx120 and every placed sensor; a pose's
// total is the ordered sum of the positive combined scores; each round places the pose with the
// highest total (first maximum) while that adds anything.
//
// The scoring (k_score_cells) leaves comb [P][C] and score_z [C] on the device.  One launch per
// round then sums every alive pose's row against `base` (the combined score of what is placed
// so far) in the reference's order, and the LAST block of the round to finish selects the pose
// and folds its row into `base` for the next launch.  Rounds are ordered by the stream alone:
// no block ever waits for another.  The ticket, the first-maximum reduction, the fold and the
// separation test are pcp_place_shared.hpp's.
#include <cmath>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_place_shared.hpp"

namespace pcp {
namespace {

constexpr int kPT = 256;        // threads per block: wave 0 walks, waves 1..3 load
constexpr int kPRows = 4;       // rows (poses) per block, as the scoring's row sums
constexpr int kPLpt = 2;        // cells per loader thread per chunk
constexpr int kPCh = (kPT - 64) * kPLpt;   // 384 cells per chunk
constexpr int kPLd = kPCh + 2;  // +2: b128 reads of lanes r, r + 1 four banks apart
constexpr int kPG = 16;         // ds_read_b128 per group of the walk

// the call's device state: control words of the rounds and the selection record (downloaded)
struct PlaceState {
    int32_t n_sel;              // rounds recorded
    int32_t done;               // a round stopped: the later launches return at once
    uint32_t ticket;            // blocks of the current round that have finished
    int32_t zx_cov;             // #{Z > 0}
    double T;                   // the total of what is placed so far
    double zx_total;            // osum(Z)
    int64_t sel[PCP_PLACE_MAX];
    double total_after[PCP_PLACE_MAX];
    int32_t cov_after[PCP_PLACE_MAX];
};
static_assert(sizeof(PlaceState) % 16 == 0, "the cells' block follows on a 16-byte boundary");

// base = Z, the owners of Z's cells, every pose alive, the state from the zx120 row of the
// scoring's sums (row P of tot / cov: osum(Z) and #{Z > 0}, as pcp_score_poses reports them)
__global__ void __launch_bounds__(kPT)
k_place_init(const double *__restrict__ score_z, int C, int P, const double *__restrict__ tot,
             const int32_t *__restrict__ cov, double *__restrict__ base,
             int32_t *__restrict__ owner, uint32_t *__restrict__ alive,
             PlaceState *__restrict__ s) {
    const int i = blockIdx.x * kPT + threadIdx.x;
    if (i < C) {
        const double z = score_z[i];
        base[i] = z;
        owner[i] = owner_of_zx(z);
    }
    if (i < P) alive[i] = 1u;
    if (i == 0) {
        s->n_sel = 0;
        s->done = 0;
        s->ticket = 0u;
        s->zx_cov = cov[P];
        s->T = tot[P];
        s->zx_total = tot[P];
    }
}

// One placement round.  Blocks of kPRows rows laid out as the scoring's row sums
// (row_group_body, pcp_score.hip): waves 1..3 load chunks of kPCh cells of the block's rows and
// of base (coalesced, two register sets two chunks ahead), form max(base, S) with the
// reference's std::max, x > 0 ? x : +0.0 and the covered counts, and stage the values in a ring
// of three LDS buffers; lane r of wave 0 walks row r of each chunk in cell order, one dependent
// f64 chain per row with the next two groups of LDS reads in flight under the adds.  Adding
// +0.0 to the non-negative running sum leaves it bit-identical, so the unconditional adds are
// the reference's `if (x > 0) total += x`.  Rows of dead poses get -inf; a block whose rows are
// all dead loads nothing.
//
// The last block to draw the round's ticket (its totals released to the device before the
// draw, the others' acquired after it) scans the totals for the first maximum, tests the gain
// against T, appends the record and updates base / owner / alive in place: every block of the
// round has consumed its loads of them before its draw, and the next launch starts after this
// one has ended.
__global__ void __launch_bounds__(kPT)
k_place_round(const double *__restrict__ S, double *base, int C, int P, uint32_t *alive,
              double *rt, int32_t *rc, PlaceState *s, int32_t *owner,
              const double *__restrict__ poses5, double sep2, int r) {
    __shared__ double s_v[3][kPRows][kPLd];
    __shared__ int32_t s_cov[kPRows];
    __shared__ int s_flag;
    const int tid = threadIdx.x, r0 = blockIdx.x * kPRows;
    if (tid == 0) s_flag = s->done;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier round stopped the search
    bool live = false;    // uniform: any alive row in this block
#pragma unroll
    for (int q = 0; q < kPRows; ++q) live |= r0 + q < P && alive[r0 + q] != 0u;
    double acc = 0.0;
    if (live) {
        const int nch = (C + kPCh - 1) / kPCh;
        if (tid < kPRows) s_cov[tid] = 0;
        const int lt = tid - 64;   // loader thread: cells lt + (kPT - 64) i of a chunk
        int32_t cov[kPRows];
#pragma unroll
        for (int q = 0; q < kPRows; ++q) cov[q] = 0;
        // raw loads, unconditional (row and cell clamped into the buffers; the formation masks
        // the cells past C, rows past P are never stored)
        double mA[kPLpt][kPRows], bA[kPLpt], mB[kPLpt][kPRows], bB[kPLpt];
        auto load = [&](int k, double (&m)[kPLpt][kPRows], double (&b)[kPLpt]) {
#pragma unroll
            for (int i = 0; i < kPLpt; ++i) {
                const int c = min(k * kPCh + lt + (kPT - 64) * i, C - 1);
                b[i] = base[c];
#pragma unroll
                for (int q = 0; q < kPRows; ++q) m[i][q] = S[(size_t)min(r0 + q, P - 1) * C + c];
            }
        };
        auto form = [&](int k, const double (&m)[kPLpt][kPRows], const double (&b)[kPLpt]) {
            double(*dst)[kPLd] = s_v[k % 3];
#pragma unroll
            for (int i = 0; i < kPLpt; ++i) {
                const int cl = lt + (kPT - 64) * i;
                const bool in = k * kPCh + cl < C;
#pragma unroll
                for (int q = 0; q < kPRows; ++q) {
                    const double x = (b[i] < m[i][q]) ? m[i][q] : b[i];   // std::max(base, S)
                    const bool pos = in && x > 0;
                    cov[q] += pos ? 1 : 0;
                    dst[q][cl] = pos ? x : 0.0;
                }
            }
        };
        auto walk = [&](int k) {
            // a ring of three groups of kPG b128 reads: the adds of group i run while groups
            // i + 1 and i + 2 are in flight; the scheduling barriers keep each group's reads
            // ahead of the adds before it
            const double2 *v = reinterpret_cast<const double2 *>(s_v[k % 3][tid]);
            constexpr int kN = kPCh / 2;
            static_assert(kN % (3 * kPG) == 0, "whole group triples per chunk");
            double2 g0[kPG], g1[kPG], g2[kPG];
            auto rd = [&](double2 *g, int j) {
#pragma unroll
                for (int i = 0; i < kPG; ++i) g[i] = v[j + i];
            };
            auto add = [&](const double2 *g) {
#pragma unroll
                for (int i = 0; i < kPG; ++i) {
                    acc += g[i].x;
                    acc += g[i].y;
                }
            };
            rd(g0, 0);
            rd(g1, kPG);
#pragma unroll
            for (int j = 0; j < kN; j += 3 * kPG) {
                if (j + 2 * kPG < kN) rd(g2, j + 2 * kPG);
                __builtin_amdgcn_sched_barrier(0);
                add(g0);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 3 * kPG < kN) rd(g0, j + 3 * kPG);
                __builtin_amdgcn_sched_barrier(0);
                add(g1);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 4 * kPG < kN) rd(g1, j + 4 * kPG);
                __builtin_amdgcn_sched_barrier(0);
                add(g2);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // one chunk: the loaders form chunk k + 2 (and load k + 4) while the chain walks chunk k
        auto step = [&](int k, double (&m)[kPLpt][kPRows], double (&b)[kPLpt]) {
            if (tid >= 64) {
                if (k + 2 < nch) {
                    form(k + 2, m, b);
                    if (k + 4 < nch) load(k + 4, m, b);
                }
            } else if (tid < kPRows) {
                walk(k);
            }
            __syncthreads();
        };
        if (tid >= 64) {
            load(0, mA, bA);
            if (nch > 1) load(1, mB, bB);
            form(0, mA, bA);
            if (nch > 2) load(2, mA, bA);
            if (nch > 1) form(1, mB, bB);
            if (nch > 3) load(3, mB, bB);
        }
        __syncthreads();
        for (int k = 0; k < nch; k += 2) {
            step(k, mA, bA);
            if (k + 1 < nch) step(k + 1, mB, bB);
        }
        if (tid >= 64) {
#pragma unroll
            for (int q = 0; q < kPRows; ++q) {
                int32_t x = cov[q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                if ((tid & 63) == 0) atomicAdd(&s_cov[q], x);
            }
        }
        __syncthreads();
    }
    if (tid < kPRows && r0 + tid < P) {
        const bool a = live && alive[r0 + tid] != 0u;
        rt[r0 + tid] = a ? acc : -INFINITY;
        rc[r0 + tid] = a ? s_cov[tid] : 0;
    }
    // the round's ticket: this block's totals written back before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the round ------------------------------------------------------
    // first maximum over the alive poses (strict '>' from -inf, :471-474): each thread scans
    // its poses in ascending order, the threads' bests are combined with ties to the lower index
    RowBest *s_best = reinterpret_cast<RowBest *>(&s_v[0][0][0]);   // [kPT / 64]
    double tb = -INFINITY;
    int b = -1, none = 0;   // (a row is a pose here: RowBest's second index stays 0)
    for (int p = tid; p < P; p += kPT) {
        if (alive[p] == 0u) continue;
        const double t = __hip_atomic_load(&rt[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t > tb) {
            tb = t;
            b = p;
        }
    }
    block_first_max_all<kPT / 64>(s_best, tb, b, none);
    // no pose alive, or the best adds nothing (fl-addition is monotone: t >= T always)
    if (tid == 0) {
        s->ticket = 0u;   // (the next launch draws from zero)
        s_flag = b >= 0 && tb > s->T;
        if (!s_flag) s->done = 1;
    }
    __syncthreads();
    if (!s_flag) return;
    if (tid == 0) {
        s->sel[r] = b;
        s->total_after[r] = tb;
        s->cov_after[r] =
            __hip_atomic_load(&rc[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s->T = tb;
        s->n_sel = r + 1;
    }
    // the placed pose's row into base; ties keep the earlier owner
    const double *row = S + (size_t)b * C;
    for (int c = tid; c < C; c += kPT) {
        double x = base[c];
        int32_t own;
        if (fold_owner(x, own, row[c], r)) {
            base[c] = x;
            owner[c] = own;
        }
    }
    // the placed pose and, with a separation, every pose closer than it in XY leave the search
    for (int p = tid; p < P; p += kPT)
        if (p == b || (sep2 > 0 && closer_than(poses5, p, b, sep2))) alive[p] = 0u;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" int pcp_place_sensors(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                 const double zx[5], const pcp_vl_params *p,
                                 const pcp_place_params *pp, int64_t *selected,
                                 double *total_after, int32_t *covered_after,
                                 double *round_totals, double *cell_score, int32_t *cell_owner,
                                 double *zx120_total, int32_t *zx120_covered,
                                 int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !pp || !selected || !total_after || !covered_after || !n_selected ||
        (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_place_sensors: null argument");
    if (pp->k_max < 1 || pp->k_max > PCP_PLACE_MAX || pp->reserved != 0)
        return set_err(ctx, PCP_E_INVALID,
                       "pcp_place_sensors: k_max %d outside 1..%d or reserved %d != 0",
                       (int)pp->k_max, PCP_PLACE_MAX, (int)pp->reserved);
    if (n > 65535)
        return set_err(ctx, PCP_E_INVALID, "pcp_place_sensors: at most 65535 poses per call");
    // the scoring, no flags and no fused tail: comb [P][C], score_z [C] and the row sums (row P:
    // zx120) on the device; a step table past PCP_MAX_STEPS is refused in there, before any launch
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P, K = pp->k_max;
    *n_selected = 0;
    if (!C) {   // no cells: nothing to cover
        if (int rc = stream_done(ctx)) return rc;
        if (zx120_total) *zx120_total = 0.0;
        if (zx120_covered) *zx120_covered = 0;
        return PCP_OK;
    }
    // the call's block, device and pinned alike: [state | base f64 C | owner i32 C | round
    // totals f64 K x P | round covered i32 K x P | alive u32 P]; the download is the span the
    // caller asked for, in one copy
    const CellBlock cb = cell_block(sizeof(PlaceState), C);
    const size_t rt_off = cb.rest_off;
    const size_t rc_off = a16(rt_off + (size_t)K * P * sizeof(double));
    const size_t al_off = a16(rc_off + (size_t)K * P * sizeof(int32_t));
    const size_t bytes = al_off + (size_t)P * sizeof(uint32_t);
    const bool cells_out = cell_score || cell_owner;
    const size_t down = round_totals ? rc_off : cells_out ? rt_off : cb.score_off;
    PCP_HIP(ctx, ctx->place_d.ensure(bytes + 64));
    PCP_HIP(ctx, ctx->place_host.ensure(down + 64));
    char *blk = ctx->place_d.as<char>();
    PlaceState *s = reinterpret_cast<PlaceState *>(blk);
    double *base = reinterpret_cast<double *>(blk + cb.score_off);
    int32_t *owner = reinterpret_cast<int32_t *>(blk + cb.owner_off);
    double *rt = reinterpret_cast<double *>(blk + rt_off);
    int32_t *rcov = reinterpret_cast<int32_t *>(blk + rc_off);
    uint32_t *alive = reinterpret_cast<uint32_t *>(blk + al_off);
    const double sep2 = sep2_of(pp->min_separation);
    hipLaunchKernelGGL(k_place_init, dim3((unsigned)((std::max(C, P) + kPT - 1) / kPT)), dim3(kPT),
                       0, st, (const double *)o.score_z, C, P, (const double *)o.tot_d,
                       (const int32_t *)o.cov_d, base, owner, alive, s);
    PCP_CHECK_LAUNCH(ctx);
    for (int r = 0; r < K && P > 0; ++r) {
        ProfScope ps(ctx, PCP_K_PLACE);
        hipLaunchKernelGGL(k_place_round, dim3((unsigned)((P + kPRows - 1) / kPRows)), dim3(kPT), 0,
                           st, (const double *)o.comb, base, C, P, alive, rt + (size_t)r * P,
                           rcov + (size_t)r * P, s, owner, o.poses_k, sep2, r);
        PCP_CHECK_LAUNCH(ctx);
    }
    char *pin = ctx->place_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, down, hipMemcpyDeviceToHost, st));
    if (int rc = stream_done(ctx)) return rc;
    const PlaceState *h = reinterpret_cast<const PlaceState *>(pin);
    const int ns = h->n_sel;
    for (int r = 0; r < ns; ++r) {
        selected[r] = h->sel[r];
        total_after[r] = h->total_after[r];
        covered_after[r] = h->cov_after[r];
    }
    if (round_totals && ns)
        std::memcpy(round_totals, pin + rt_off, (size_t)ns * P * sizeof(double));
    copy_cells(pin, cb, C, cell_score, cell_owner);
    if (zx120_total) *zx120_total = h->zx_total;
    if (zx120_covered) *zx120_covered = h->zx_cov;
    *n_selected = ns;
    return PCP_OK;
}
