// pcp_aim.hip -- greedy placement of mobile sensors with a limited field of view
// (pcp_place_aimed): pcp_place_sensors' rounds over (pose, aim) rows.  A row's cell counts for the
// pose's score S[p][c] where the cell lies inside the aimed sector and elevation band, for +0.0
// elsewhere (include/pcp_abi.h has the definition, DESIGN.md §6l the kernels and their timing).
//
// The scoring runs unchanged on a pitch-zeroed host copy of the poses and leaves comb [P][C] and
// score_z [C] on the device.  The predicate's tables (pcp_aim.hpp: host cos / sin / tan) are
// uploaded in one copy.  k_aim_init folds the fixed sensors into the base, k_aim_base sums it, then
// one launch per round: block p holds pose p, lane a of wave 0 walks row (p, a) as one f64 chain
// in cell order, waves 1..7 stage chunks of kWalkC cells one chunk ahead: every staging wave forms
// the geometry of its lanes' cells and, for its share of the aims, the in-view bits of the chunk's
// cells as one ballot word; the first of them also stores b = clamp(base), m = clamp(max(base, S))
// and their positive bits.  So the walking lanes only select and add.  The rows of a pose share the staged cells (broadcast
// reads).  The round's last block selects the first maximum over all rows and folds the chosen
// row into the base; rounds are ordered by the stream alone, no block ever waits for another.
// The ticket, the first-maximum reduction, the fold and the separation test are
// pcp_place_shared.hpp's.
#include <cmath>
#include <cstring>
#include <vector>

#include "pcp_aim.hpp"
#include "pcp_internal.hpp"
#include "pcp_place_shared.hpp"

namespace pcp {
namespace {

constexpr int kAT = 256;   // threads per block of the preparation kernels
constexpr int kAR = 512;   // threads per block of a round: wave 0 walks, waves 1..7 stage (two
                           // staging waves per SIMD hide each other's LDS and f64 latencies)
constexpr int kALoad = (kAR - 64) / 64;   // staging waves: aim a is formed by wave a % kALoad
constexpr int kAG = 8;     // cells (b128 reads) per register group of the walk
static_assert(kWalkC % (2 * kAG) == 0, "whole group pairs per chunk");
static_assert(PCP_AIM_MAX <= 64, "one lane of the walking wave per aim");
static_assert(kWalkC == 64, "a chunk's in-view bits are one ballot word");

// the call's device state: control words of the rounds and the selection record (downloaded)
struct AimState {
    int32_t n_sel;              // rounds recorded
    int32_t done;               // a round stopped: the later launches return at once
    uint32_t ticket;            // blocks of the current round that have finished
    int32_t base_cov;           // #{base > 0} before the rounds
    double T;                   // the total of what is placed so far
    double base_total;          // osum(base) before the rounds
    int32_t sel[PCP_PLACE_MAX], sel_aim[PCP_PLACE_MAX];
    double total_after[PCP_PLACE_MAX];
    int32_t cov_after[PCP_PLACE_MAX];
};
static_assert(sizeof(AimState) % 16 == 0, "the cells' block follows on a 16-byte boundary");

// what the kernels read of the call: the cells, the poses the scoring read, the tables
struct AimEnv {
    const double *cxyz;     // [C][3]
    const double *poses5;   // [P][5] (pitch zeroed)
    const double *tp;       // [P][2] cos, sin of the yaws
    const AimRow *ta;       // [A]
    double ch;
    int32_t no_h;
    int32_t C, P, A;
};

// W[p][a][c] is S[p][c] (true) or +0.0
__device__ __forceinline__ bool sees(const AimEnv &E, int p, int a, int c) {
    const double *q = E.poses5 + 5 * (size_t)p;
    const AimGeo g =
        aim_geo(E.cxyz[3 * (size_t)c], E.cxyz[3 * (size_t)c + 1], E.cxyz[3 * (size_t)c + 2], q[0],
                q[1], q[2], E.ch);
    const AimRow r = E.ta[a];
    double Cy, Sy;
    aim_heading(E.tp[2 * (size_t)p], E.tp[2 * (size_t)p + 1], r.ca, r.sa, Cy, Sy);
    return aim_sees(g, Cy, Sy, r.tlo, r.thi, E.no_h != 0);
}

// base = Z with the fixed sensors' rows folded in list order, the owners, the poses in the search
__global__ void __launch_bounds__(kAT)
k_aim_init(AimEnv E, const double *__restrict__ S, const double *__restrict__ score_z,
           AimFixed fx, double sep2, double *__restrict__ base, int32_t *__restrict__ owner,
           uint32_t *__restrict__ alive) {
    const int i = blockIdx.x * kAT + threadIdx.x;
    if (i < E.C) {
        double x = score_z[i];
        int32_t own = owner_of_zx(x);
        for (int f = 0; f < fx.n; ++f) {
            const double v = sees(E, fx.pose[f], fx.aim[f], i) ? S[(size_t)fx.pose[f] * E.C + i] : 0.0;
            (void)fold_owner(x, own, v, f);
        }
        base[i] = x;
        owner[i] = own;
    }
    if (i < E.P) {
        bool a = true;
        for (int f = 0; f < fx.n; ++f)
            a = a && i != fx.pose[f] && !(sep2 > 0 && closer_than(E.poses5, i, fx.pose[f], sep2));
        alive[i] = a ? 1u : 0u;
    }
}

// the base's ordered total and count, the state of the rounds (one block)
__global__ void __launch_bounds__(kAT)
k_aim_base(const double *__restrict__ base, int C, AimState *__restrict__ s) {
    __shared__ double s_b[kAT];
    __shared__ int32_t s_cnt;
    const double t = ordered_total<kAT>([&](int c) { return base[c]; }, C, s_b, s_cnt);
    if (threadIdx.x == 0) {
        s->n_sel = 0;
        s->done = 0;
        s->ticket = 0u;
        s->base_cov = s_cnt;
        s->T = t;
        s->base_total = t;
    }
}

// One round.  Block p: the staging waves load chunk k + 2's base, S[p] and cell coordinates while
// they form chunk k + 1 and the walking wave adds chunk k (two LDS buffers, one barrier per
// chunk).  Lane l of a staging wave owns cell l of the chunk: the geometry of (pose, cell), then
// per aim of its wave (a mod kALoad) the predicate and a ballot; staging wave 0 alone also stores
// the clamped pair (b, m) and the two words of positive bits.  Lane a of wave 0
// adds, cell by cell, m where its aim's bit is set and b where not: adding +0.0 to the
// non-negative running sum leaves it bit-identical, so the unconditional adds are osum's.  The
// covered count is a popcount of the same words.  A dead pose's rows get -inf.
// commit 0 (the timing entry): the last block selects and leaves everything as it was.
__global__ void __launch_bounds__(kAR)
k_aim_round(AimEnv E, const double *__restrict__ S, double *base, uint32_t *alive, double *rt,
            int32_t *rc, AimState *s, int32_t *owner, double sep2, int n_fixed, int r,
            int commit) {
    __shared__ double2 s_bm[2][kWalkC];       // (b, m) per cell
    __shared__ uint64_t s_mask[2][64];        // per aim: the chunk's in-view bits
    __shared__ uint64_t s_pos[2][2];          // the chunk's b > 0 and m > 0 bits
    __shared__ AimRow s_aim[64];              // per aim: (Cy, Sy, tlo, thi) of this pose
    __shared__ RowBest s_best[kAR / 64];
    __shared__ int s_flag;
    const int tid = threadIdx.x, p = blockIdx.x;
    const int C = E.C, A = E.A;
    if (tid == 0) s_flag = s->done;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier round stopped the search
    const bool live = alive[p] != 0u;   // uniform
    double acc = 0.0;
    int32_t cnt = 0;
    if (live) {
        if (tid < 64) {
            if (tid < A) {
                const AimRow t = E.ta[tid];
                AimRow h;
                aim_heading(E.tp[2 * (size_t)p], E.tp[2 * (size_t)p + 1], t.ca, t.sa, h.ca, h.sa);
                h.tlo = t.tlo;
                h.thi = t.thi;
                s_aim[tid] = h;
            }
            s_mask[0][tid] = 0ull;   // (the lanes past A walk b alone; their sums are dropped)
            s_mask[1][tid] = 0ull;
        }
        __syncthreads();
        const int nch = (C + kWalkC - 1) / kWalkC;
        const int lw = (tid >> 6) - 1, ll = tid & 63;   // staging wave, its lane's cell
        const double px = E.poses5[5 * (size_t)p], py = E.poses5[5 * (size_t)p + 1],
                     pz = E.poses5[5 * (size_t)p + 2];
        const bool no_h = E.no_h != 0;
        struct Raw {
            double b, v, x, y, z;
        };
        // raw loads, unconditional (the cell clamped into the buffers; form masks the cells past C)
        auto load = [&](int k) {
            const size_t c = (size_t)min(k * kWalkC + ll, C - 1);
            Raw w;
            w.b = base[c];
            w.v = S[(size_t)p * C + c];
            w.x = E.cxyz[3 * c];
            w.y = E.cxyz[3 * c + 1];
            w.z = E.cxyz[3 * c + 2];
            return w;
        };
        auto form = [&](int k, const Raw &w) {
            const int buf = k & 1;
            const bool in = k * kWalkC + ll < C;
            const double x = (w.b < w.v) ? w.v : w.b;   // std::max(base, S)
            const bool pb = in && w.b > 0, pm = in && x > 0;
            const AimGeo g = aim_geo(w.x, w.y, w.z, px, py, pz, E.ch);
            if (lw == 0) {
                s_bm[buf][ll] = make_double2(pb ? w.b : 0.0, pm ? x : 0.0);
                const uint64_t wb = __ballot(pb), wm = __ballot(pm);
                if (ll == 0) {
                    s_pos[buf][0] = wb;
                    s_pos[buf][1] = wm;
                }
            }
            for (int a = lw; a < A; a += kALoad) {
                const AimRow h = s_aim[a];
                const uint64_t bits = __ballot(in && aim_sees(g, h.ca, h.sa, h.tlo, h.thi, no_h));
                if (ll == 0) s_mask[buf][a] = bits;
            }
        };
        auto walk = [&](int k) {
            const int buf = k & 1;
            const uint64_t mk = s_mask[buf][tid];
            cnt += __popcll((mk & s_pos[buf][1]) | (~mk & s_pos[buf][0]));
            const uint32_t lo = (uint32_t)mk, hi = (uint32_t)(mk >> 32);
            // two register groups of kAG b128 reads (one cell each): the selects and adds of one
            // group run while the other's reads are in flight (one wave per SIMD: nothing else
            // hides the LDS latency; the scheduling barriers keep each group's reads ahead of the
            // adds before it, as walk_chunk's)
            const double2 *v = s_bm[buf];
            double2 g0[kAG], g1[kAG];
            auto rd = [&](double2 *g, int j) {
#pragma unroll
                for (int i = 0; i < kAG; ++i) g[i] = v[j + i];
            };
            auto add = [&](const double2 *g, int j) {
#pragma unroll
                for (int i = 0; i < kAG; ++i) {
                    const int c = j + i;
                    const bool in = (((c < 32 ? lo : hi) >> (c & 31)) & 1u) != 0u;
                    acc += in ? g[i].y : g[i].x;
                }
            };
            rd(g0, 0);
#pragma unroll
            for (int j = 0; j < kWalkC; j += 2 * kAG) {
                rd(g1, j + kAG);
                __builtin_amdgcn_sched_barrier(0);
                add(g0, j);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 2 * kAG < kWalkC) rd(g0, j + 2 * kAG);
                __builtin_amdgcn_sched_barrier(0);
                add(g1, j + kAG);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        Raw cur{}, nxt{};
        if (tid >= 64) {
            cur = load(0);
            if (nch > 1) nxt = load(1);
            form(0, cur);
        }
        __syncthreads();
        for (int k = 0; k < nch; ++k) {
            if (tid >= 64) {
                if (k + 1 < nch) {
                    cur = nxt;
                    if (k + 2 < nch) nxt = load(k + 2);
                    form(k + 1, cur);
                }
            } else {
                walk(k);
            }
            __syncthreads();
        }
    }
    if (tid < A) {
        rt[(size_t)p * A + tid] = live ? acc : -INFINITY;
        rc[(size_t)p * A + tid] = live ? cnt : 0;
    }
    // the round's ticket: this block's totals written back before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the round ------------------------------------------------------
    // first maximum over the rows in row-major order (strict '>' from -inf; a dead pose's rows
    // hold -inf): each thread scans its rows in ascending order, the threads' bests are combined
    // with ties to the earlier row
    double tb = -INFINITY;
    int bp = -1, ba = -1;
    const int rows = E.P * A;
    for (int i = tid; i < rows; i += kAR) {
        const double t = __hip_atomic_load(&rt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t > tb) {
            tb = t;
            bp = i / A;
            ba = i - bp * A;
        }
    }
    block_first_max_all<kAR / 64>(s_best, tb, bp, ba);
    // no pose alive, or the best adds nothing (fl-addition is monotone: t >= T always)
    if (tid == 0) {
        s->ticket = 0u;   // (the next launch draws from zero)
        s_flag = commit && bp >= 0 && tb > s->T;
        if (commit && !s_flag) s->done = 1;
    }
    __syncthreads();
    if (!s_flag) return;
    if (tid == 0) {
        s->sel[r] = bp;
        s->sel_aim[r] = ba;
        s->total_after[r] = tb;
        s->cov_after[r] = __hip_atomic_load(&rc[(size_t)bp * A + ba], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        s->T = tb;
        s->n_sel = r + 1;
    }
    // the placed row into base; ties keep the earlier owner
    const double *row = S + (size_t)bp * C;
    for (int c = tid; c < C; c += kAR) {
        double x = base[c];
        int32_t own;
        if (fold_owner(x, own, sees(E, bp, ba, c) ? row[c] : 0.0, n_fixed + r)) {
            base[c] = x;
            owner[c] = own;
        }
    }
    // the placed pose and, with a separation, every pose closer than it in XY leave the search
    for (int q = tid; q < E.P; q += kAR)
        if (q == bp || (sep2 > 0 && closer_than(E.poses5, q, bp, sep2))) alive[q] = 0u;
}

// the checks of both entries: PCP_E_INVALID with the reason, before anything is launched
int check_args(pcp_ctx *ctx, const char *what, uint64_t n, const pcp_vl_params *p,
               const pcp_aim_params *ap, const double *aims, AimFixed &fx) {
    int bad = 0;
    switch (aim_check(ap, aims, n, &bad)) {
    case kAimOk: break;
    case kAimKmax:
        return set_err(ctx, PCP_E_INVALID, "%s: k_max %d outside 1..%d", what, (int)ap->k_max,
                       PCP_PLACE_MAX);
    case kAimCount:
        return set_err(ctx, PCP_E_INVALID, "%s: n_aims %d outside 1..%d", what, (int)ap->n_aims,
                       PCP_AIM_MAX);
    case kAimFixedCount:
        return set_err(ctx, PCP_E_INVALID, "%s: n_fixed %d outside 0..%d", what, (int)ap->n_fixed,
                       PCP_PLACE_MAX);
    case kAimReserved:
        return set_err(ctx, PCP_E_INVALID, "%s: reserved %d != 0", what, (int)ap->reserved);
    case kAimHfov:
        return set_err(ctx, PCP_E_INVALID, "%s: h_fov %.17g is not a positive finite angle", what,
                       ap->h_fov);
    case kAimVfov:
        return set_err(ctx, PCP_E_INVALID, "%s: v_fov %.17g outside (0, pi]", what, ap->v_fov);
    case kAimAim:
        return set_err(ctx, PCP_E_INVALID,
                       "%s: aim %d (%.17g, %.17g) is not finite or its pitch is outside "
                       "[-pi/2, pi/2]", what, bad, aims[2 * bad], aims[2 * bad + 1]);
    case kAimPoses:
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses, at most %d per call", what,
                       (unsigned long long)n, PCP_PAIR_MAX_POSES);
    case kAimRows:
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses x %d aims, at most %d rows per call",
                       what, (unsigned long long)n, (int)ap->n_aims, PCP_AIM_MAX_ROWS);
    case kAimFixedPose:
        return set_err(ctx, PCP_E_INVALID, "%s: fixed_pose[%d] = %lld is no pose of %llu", what,
                       bad, (long long)ap->fixed_pose[bad], (unsigned long long)n);
    case kAimFixedTwice:
        return set_err(ctx, PCP_E_INVALID, "%s: pose %lld is fixed twice", what,
                       (long long)ap->fixed_pose[bad]);
    default:
        return set_err(ctx, PCP_E_INVALID, "%s: fixed_aim[%d] = %d is no aim of %d", what, bad,
                       (int)ap->fixed_aim[bad], (int)ap->n_aims);
    }
    fx.n = ap->n_fixed;
    for (int i = 0; i < ap->n_fixed; ++i) {
        fx.pose[i] = (int32_t)ap->fixed_pose[i];
        fx.aim[i] = ap->fixed_aim[i];
    }
    return steps_within_bound(ctx, p->max_distance - kVisRadius);
}

// the pointers of a call's device block
struct AimDev {
    AimState *s;
    double *base, *rt;
    int32_t *owner, *rc;
    uint32_t *alive;
    AimEnv E;
};

// The front of both entries behind the checks: the scoring on the pitch-zeroed poses, the buffers,
// the tables' upload, the base.  Device results in flight on return; o.C == 0: nothing enqueued
// past the scoring.  K = the rounds the block has tables for.
int aim_enqueue(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                const pcp_vl_params *p, const pcp_aim_params *ap, const double *aims,
                const AimFixed &fx, int K, ScoreEnq &o, AimPlan &s, AimDev &d) {
    std::vector<double> flat(poses5, poses5 + 5 * n);
    for (uint64_t q = 0; q < n; ++q) flat[5 * q + 3] = 0.0;
    if (int rc = score_enqueue(ctx, flat.data(), n, zx, p, o)) return rc;
    if (!o.C) return PCP_OK;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P, A = ap->n_aims;
    s = aim_plan(sizeof(AimState), C, P, A, K);
    // pinned: [tables | the download's landing, sized for its largest span, the round totals']
    const size_t land = a16(s.tab_bytes);
    PCP_HIP(ctx, ctx->aim_d.ensure(s.bytes + 64));
    PCP_HIP(ctx, ctx->aim_m.ensure(s.tab_bytes + 64));
    PCP_HIP(ctx, ctx->aim_host.ensure(land + s.rc_off + 64));
    char *pin = ctx->aim_host.as<char>();
    double ch = 0.0;
    aim_pose_rows(poses5, n, reinterpret_cast<double *>(pin + s.tp_off));
    const int no_h =
        aim_rows(aims, A, ap->h_fov, ap->v_fov, reinterpret_cast<AimRow *>(pin + s.ta_off), &ch);
    char *tab = ctx->aim_m.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(tab, pin, s.tab_bytes, hipMemcpyHostToDevice, st));
    char *blk = ctx->aim_d.as<char>();
    d.s = reinterpret_cast<AimState *>(blk);
    d.base = reinterpret_cast<double *>(blk + s.cb.score_off);
    d.owner = reinterpret_cast<int32_t *>(blk + s.cb.owner_off);
    d.rt = reinterpret_cast<double *>(blk + s.rt_off);
    d.rc = reinterpret_cast<int32_t *>(blk + s.rc_off);
    d.alive = reinterpret_cast<uint32_t *>(blk + s.al_off);
    d.E.cxyz = ctx->cells_xyz.as<const double>();
    d.E.poses5 = o.poses_k;
    d.E.tp = reinterpret_cast<const double *>(tab + s.tp_off);
    d.E.ta = reinterpret_cast<const AimRow *>(tab + s.ta_off);
    d.E.ch = ch;
    d.E.no_h = no_h;
    d.E.C = C;
    d.E.P = P;
    d.E.A = A;
    hipLaunchKernelGGL(k_aim_init, dim3((unsigned)((std::max(C, P) + kAT - 1) / kAT)), dim3(kAT), 0,
                       st, d.E, (const double *)o.comb, (const double *)o.score_z, fx,
                       sep2_of(ap->min_separation), d.base, d.owner, d.alive);
    PCP_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_aim_base, dim3(1), dim3(kAT), 0, st, (const double *)d.base, C, d.s);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

int round_launch(pcp_ctx *ctx, const ScoreEnq &o, const AimPlan &s, const AimDev &d, double sep2,
                 int n_fixed, int r, int commit) {
    ProfScope ps(ctx, PCP_K_PLACE);
    hipLaunchKernelGGL(k_aim_round, dim3((unsigned)s.P), dim3(kAR), 0, ctx->stream, d.E,
                       (const double *)o.comb, d.base, d.alive, d.rt + (size_t)r * s.rows(),
                       d.rc + (size_t)r * s.rows(), d.s, d.owner, sep2, n_fixed, r, commit);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" int pcp_place_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                               const pcp_vl_params *p, const pcp_aim_params *ap,
                               const double *aims, int64_t *selected, int32_t *selected_aim,
                               double *total_after, int32_t *covered_after, double *round_totals,
                               double *cell_score, int32_t *cell_owner, double *base_total,
                               int32_t *base_covered, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !ap || !aims || !selected || !selected_aim || !total_after ||
        !covered_after || !base_total || !base_covered || !n_selected || (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_place_aimed: null argument");
    AimFixed fx{};
    if (int rc = check_args(ctx, "pcp_place_aimed", n, p, ap, aims, fx)) return rc;
    const bool cells_out = cell_score || cell_owner;
    ScoreEnq o;
    AimPlan s{};
    AimDev d{};
    if (int rc = aim_enqueue(ctx, poses5, n, zx, p, ap, aims, fx, ap->k_max, o, s, d)) return rc;
    *n_selected = 0;
    if (!o.C) {   // no cells: nothing to cover
        if (int rc = stream_done(ctx)) return rc;
        *base_total = 0.0;
        *base_covered = 0;
        return PCP_OK;
    }
    hipStream_t st = ctx->stream;
    const double sep2 = sep2_of(ap->min_separation);
    for (int r = 0; r < s.K && s.P > 0; ++r)
        if (int rc = round_launch(ctx, o, s, d, sep2, fx.n, r, 1)) return rc;
    const size_t down = s.down(round_totals != nullptr, cells_out);
    char *pin = ctx->aim_host.as<char>() + a16(s.tab_bytes);
    PCP_HIP(ctx, hipMemcpyAsync(pin, ctx->aim_d.as<char>(), down, hipMemcpyDeviceToHost, st));
    if (int rc = stream_done(ctx)) return rc;
    const AimState *h = reinterpret_cast<const AimState *>(pin);
    const int ns = h->n_sel;
    for (int r = 0; r < ns; ++r) {
        selected[r] = h->sel[r];
        selected_aim[r] = h->sel_aim[r];
        total_after[r] = h->total_after[r];
        covered_after[r] = h->cov_after[r];
    }
    if (round_totals && ns)
        host_copy(ctx, round_totals, pin + s.rt_off, (size_t)ns * s.rows() * sizeof(double));
    copy_cells(pin, s.cb, s.C, cell_score, cell_owner);
    *base_total = h->base_total;
    *base_covered = h->base_cov;
    *n_selected = ns;
    return PCP_OK;
}

extern "C" int pcp_place_aimed_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                     const double zx[5], const pcp_vl_params *p,
                                     const pcp_aim_params *ap, const double *aims, int reps,
                                     double *ms_per_round) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !ap || !aims || !ms_per_round || !poses5 || n == 0 || reps <= 0)
        return set_err(ctx, PCP_E_INVALID,
                       "pcp_place_aimed_burst: null argument or nothing to time");
    AimFixed fx{};
    if (int rc = check_args(ctx, "pcp_place_aimed_burst", n, p, ap, aims, fx)) return rc;
    *ms_per_round = 0.0;
    ScoreEnq o;
    AimPlan s{};
    AimDev d{};
    if (int rc = aim_enqueue(ctx, poses5, n, zx, p, ap, aims, fx, 1, o, s, d)) return rc;
    if (!o.C) {
        if (int rc = stream_done(ctx)) return rc;
        return set_err(ctx, PCP_E_INVALID, "pcp_place_aimed_burst: no cells, nothing to time");
    }
    const double sep2 = sep2_of(ap->min_separation);
    auto once = [&] { return round_launch(ctx, o, s, d, sep2, fx.n, 0, 0); };
    return time_reps(ctx, "pcp_place_aimed_burst", ctx->stream, reps, once, once, ms_per_round);
}
