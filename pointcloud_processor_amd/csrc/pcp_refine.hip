// pcp_refine.hip -- 1-exchange refinement of a multi-sensor placement (pcp_place_refine): every
// unlocked sensor of the set is tried at every other pose with the rest of the set held, the best
// such exchange is taken while it raises the total, and the evaluation repeats (include/pcp_abi.h
// has the definition; DESIGN.md §6i the kernels and their timing).
//
// The scoring (k_score_cells) leaves comb [P][C] and score_z [C] on the device.  One launch
// (k_refine_init) clamps the rows once, Sc[p][c] = S > 0 ? S : +0.0, padded to whole tiles and
// whole chunks with +0.0.  Each evaluation is then two launches, ordered by the stream alone (no
// block ever waits for another):
//   k_refine_prep  per cell the largest and second-largest of {Z, the set's rows} and the slot of
//                  the largest, hence the clamped leave-one-out rows Lc[j][c] of the unlocked slots
//                  j + n_locked (max never rounds and scores are never NaN or -0.0: eval_cell ends
//                  in fmax(0.0, .)), so that a row's term is max(Lc[j][c], Sc[p][c]); in the first
//                  evaluation also the start total
//   k_refine_eval  one block per tile of kRTile poses x all unlocked slots, one wave per four
//                  slots; the LAST block of the launch picks the first maximum, tests it against
//                  T, records the move and updates the set; the evaluations enqueued behind a stop
//                  return at once
// and k_refine_final folds the final set into cell_score / cell_owner.  The walk, the ticket, the
// first-maximum reduction, the ordered total, the fold and the separation test are
// pcp_place_shared.hpp's.
#include <cmath>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_place_shared.hpp"

namespace pcp {
namespace {

constexpr int kRT = 256;          // threads per block of the preparation, cells per block
constexpr int kRTile = 16;        // poses per block of an evaluation
constexpr int kRSl = 64 / kRTile; // slots per wave: lane (j, q) is slot row j against pose q
constexpr int kRD = 4;            // chunks a thread's loads run ahead of the walk
static_assert(kRD == 4, "k_refine_eval names its four register sets");
static_assert(kRTile == PCP_PLACE_MAX, "four waves of kRSl slot rows are the whole set");
static_assert(kRT % kWalkC == 0, "whole chunks per preparation block");

// the call's state: control words of the evaluations and the result record (downloaded)
struct RefineState {
    int32_t n_moves;            // moves recorded
    int32_t done;               // an evaluation stopped: the later launches return at once
    int32_t converged;          // it stopped because no exchange raises the total
    int32_t start_cov;
    uint32_t ticket;            // blocks of the current evaluation that have finished
    int32_t pad[3];
    double T;                   // the total of the current set
    double start_total;
    int32_t set[PCP_PLACE_MAX];
    int32_t move_slot[PCP_REFINE_MAX_MOVES], move_from[PCP_REFINE_MAX_MOVES];
    int32_t move_to[PCP_REFINE_MAX_MOVES], move_cov[PCP_REFINE_MAX_MOVES];
    double move_total[PCP_REFINE_MAX_MOVES];
};
static_assert(sizeof(RefineState) % 16 == 0, "the cells' block follows on a 16-byte boundary");

struct RefineSet {
    int32_t idx[PCP_PLACE_MAX];
};

// a staged pair of cells in registers (a native vector: the register sets stay in VGPRs)
typedef double v2d __attribute__((ext_vector_type(2)));

// Once per call: the clamped rows Sc [Pp][Cs] (+0.0 in the rows past P and the cells past C), the
// slot rows Lc [kRTile][Cs] zeroed (the preparation stores the unlocked slots' cells below C
// only), and the state with the start set.
__global__ void __launch_bounds__(kRT)
k_refine_init(const double *__restrict__ S, int C, int P, int Pp, int Cs, RefineSet start, int K,
              double *__restrict__ Sc, double *__restrict__ Lc, RefineState *__restrict__ s) {
    const size_t i = (size_t)blockIdx.x * kRT + threadIdx.x;
    if (i < (size_t)Pp * Cs) {
        const int p = (int)(i / Cs), c = (int)(i % Cs);
        double x = 0.0;
        if (p < P && c < C) {
            const double v = S[(size_t)p * C + c];
            x = v > 0 ? v : 0.0;
        }
        Sc[i] = x;
    }
    if (i < (size_t)kRTile * Cs) Lc[i] = 0.0;
    if (i == 0) {
        s->n_moves = 0;
        s->done = 0;
        s->converged = 0;
        s->start_cov = 0;
        s->ticket = 0u;
        s->T = 0.0;
        s->start_total = 0.0;
    }
    if (i < PCP_PLACE_MAX) s->set[i] = (int)i < K ? start.idx[i] : -1;
}

// One evaluation's leave-one-out rows.  Block b of the first ncb: cells b kRT ..; per cell the
// largest (first) and second-largest of {Z, S[set[0]], .., S[set[K - 1]]} as a multiset and the
// slot that holds the largest (-1: Z), so that fold(set without slot i)[c] = arg == i ? second :
// first; its clamp goes to Lc[i - n_locked][c] for the unlocked slots.  In the first evaluation
// one more block (ncb) computes the start total: an ordered chain over the clamped `first` (one
// lane; the other threads stage and count).
__global__ void __launch_bounds__(kRT)
k_refine_prep(const double *__restrict__ S, const double *__restrict__ Z, int C, int Cs, int ncb,
              int K, int n_locked, RefineState *s, double *__restrict__ Lc) {
    __shared__ double s_b[kRT];
    __shared__ int s_set[PCP_PLACE_MAX];
    __shared__ int s_flag;
    __shared__ int32_t s_cnt;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = s->done;
    if (tid < PCP_PLACE_MAX) s_set[tid] = s->set[tid];
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier evaluation stopped the refinement
    auto top2 = [&](int c, double &second, int &arg) {
        double first = Z[c];
        second = -INFINITY;
        arg = -1;
        for (int j = 0; j < K; ++j) {
            const double v = S[(size_t)s_set[j] * C + c];
            if (first < v) {
                second = first;
                first = v;
                arg = j;
            } else if (second < v) {
                second = v;
            }
        }
        return first;
    };
    if ((int)blockIdx.x == ncb) {   // ---- the start total (the first evaluation only)
        const double acc = ordered_total<kRT>(
            [&](int c) {
                double second;
                int arg;
                return top2(c, second, arg);
            },
            C, s_b, s_cnt);
        if (tid == 0) {
            s->start_total = acc;
            s->T = acc;
            s->start_cov = s_cnt;
        }
        return;
    }
    const int c = blockIdx.x * kRT + tid;
    if (c >= C) return;
    double second;
    int arg;
    const double first = top2(c, second, arg);
    for (int i = n_locked; i < K; ++i) {
        const double x = arg == i ? second : first;
        Lc[(size_t)(i - n_locked) * Cs + c] = x > 0 ? x : 0.0;
    }
}

// One evaluation.  Block t of W waves owns the poses t kRTile ..; lane (j, q) owns slot row j
// (slot j + n_locked) against pose q: one f64 chain, adding its cells in ascending order from
// +0.0, one rounded add per cell (+0.0 for the cells that are not positive and for the padding
// past C: bit-neutral).  W = 1, 2 or 4 waves for up to 4, 8 or 16 unlocked slots: a small set
// neither stages nor walks sixteen slot rows (four waves take 18 % longer than one or two).  The
// block stages chunks of kWalkC cells of its kRSl W slot rows and its kRTile pose rows -- coalesced
// b128 loads, kRD chunks ahead in registers, stored to LDS as they lie, rows kWalkLd apart -- and
// every lane reads two cells of its slot row and of its pose row per ds_read_b128 (walk_chunk, as
// k_pair_tiles: a pose's loads are shared by every slot).
//
// The last block to draw the evaluation's ticket (its best released to the device before the
// draw, the others' acquired after it) takes the first maximum of the blocks' bests in row-major
// order, tests the gain against T, appends the move and updates the set in place: every block of
// the evaluation has copied the set to LDS before its draw, and the next launch starts after
// this one has ended.  commit == 0 (the timing entry): the record is written at the current
// index, but the set, T, the count and the stop words stay.
template <int W>
__global__ void __launch_bounds__(64 * W)
k_refine_eval(const double *__restrict__ Lc, const double *__restrict__ Sc, int Cs, int C, int P,
              int K, int n_locked, const double *__restrict__ poses5, double sep2,
              RowBest *slots, double *__restrict__ table, RefineState *s, int max_moves,
              int commit) {
    constexpr int kT = 64 * W;                    // threads
    constexpr int kA = kRSl * W;                  // staged slot rows
    constexpr int kRows = kA + kRTile;            // and the pose rows behind them
    constexpr int kStep = kT / (kWalkC / 2);         // rows one b128 load of every thread covers
    constexpr int kNL = kRows / kStep;            // b128 loads per thread per chunk
    static_assert(kRows % kStep == 0 && kA % kStep == 0, "whole loads; a load is of one kind");
    __shared__ double2 s_m[2][kRows * kWalkLd / 2];
    __shared__ RowBest s_best[W];
    __shared__ int s_set[PCP_PLACE_MAX];
    __shared__ int s_flag;
    __shared__ int32_t s_cnt;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = s->done;
    if (tid < PCP_PLACE_MAX) s_set[tid] = s->set[tid];
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier evaluation stopped the refinement
    const int tb = blockIdx.x;
    double acc = 0.0;
    {
        const int nch = Cs / kWalkC;
        const int ia = tid / kRTile, jb = kA + tid % kRTile;
        // a thread's b128 loads per chunk: double2 `col` of the rows r0 + kStep i, slot rows
        // first (32 threads per row: 512 contiguous bytes)
        const int r0 = tid / (kWalkC / 2), col = tid % (kWalkC / 2);
        const v2d *srcA = reinterpret_cast<const v2d *>(Lc + (size_t)r0 * Cs) + col;
        const v2d *srcB = reinterpret_cast<const v2d *>(Sc + (size_t)(tb * kRTile + r0) * Cs) + col;
        const size_t step = (size_t)kStep * Cs / 2;          // kStep rows in double2
        const int dst = r0 * (kWalkLd / 2) + col;
        v2d g0[kNL], g1[kNL], g2[kNL], g3[kNL];
        auto load = [&](int k, v2d (&r)[kNL]) __attribute__((always_inline)) {
            // (past the end: the last chunk once more)
            const size_t o = (size_t)min(k, nch - 1) * (kWalkC / 2);
#pragma unroll
            for (int i = 0; i < kNL; ++i)
                r[i] = i < kA / kStep ? srcA[o + i * step] : srcB[o + (i - kA / kStep) * step];
        };
        auto store = [&](int buf, const v2d (&r)[kNL]) __attribute__((always_inline)) {
            v2d *d = reinterpret_cast<v2d *>(s_m[buf]) + dst;
#pragma unroll
            for (int i = 0; i < kNL; ++i) d[i * kStep * (kWalkLd / 2)] = r[i];
        };
        // kRD chunks in flight in registers: a chunk's walk is a fraction of a load's latency, so
        // the loads run that many chunks ahead of the walk.  While chunk k is walked, g[(k + 1)
        // % kRD] .. g[k % kRD] hold the chunks k + 1 .. k + kRD; after the walk chunk k + 1
        // goes to the other LDS buffer and its registers take chunk k + 1 + kRD (the stores past
        // the last chunk go to the buffer no one reads again: straight-line code keeps the
        // prefetch in registers)
        auto chunk = [&](int k, int buf, v2d (&next)[kNL]) __attribute__((always_inline)) {
            if (k < nch) {   // (uniform)
                walk_chunk(s_m[buf] + ia * (kWalkLd / 2), s_m[buf] + jb * (kWalkLd / 2), acc);
                store(buf ^ 1, next);
                load(k + 1 + kRD, next);
                __syncthreads();
            }
        };
        load(0, g0);
        load(1, g1);
        load(2, g2);
        load(3, g3);
        store(0, g0);
        load(kRD, g0);
        __syncthreads();
        for (int k = 0; k < nch; k += kRD) {
            chunk(k, 0, g1);
            chunk(k + 1, 1, g2);
            chunk(k + 2, 0, g3);
            chunk(k + 3, 1, g0);
        }
    }
    // the row's admissibility: an unlocked slot, a pose outside the set, and with a separation
    // not closer than it to any other sensor of the set
    const int slot = n_locked + tid / kRTile, p = tb * kRTile + tid % kRTile;
    bool ok = slot < K && p < P;
    if (ok) {
        const double px = poses5[5 * (size_t)p], py = poses5[5 * (size_t)p + 1];
        for (int j = 0; j < K; ++j) {
            const int q = s_set[j];
            ok &= q != p;
            if (sep2 > 0 && j != slot) ok &= !closer_than(px, py, poses5, q, sep2);
        }
    }
    double bt = ok ? acc : -INFINITY;
    if (table && p < P) {
        if (slot < K) table[(size_t)slot * P + p] = bt;
        if (tid < kRTile)   // the locked slots' rows
            for (int i = 0; i < n_locked; ++i) table[(size_t)i * P + p] = -INFINITY;
    }
    // the block's first maximum in row-major order
    int ba = ok ? slot : -1, bb = ok ? p : -1;
    block_first_max<W>(s_best, bt, ba, bb);
    if (tid == 0) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(&slots[blockIdx.x]);
        w[0] = (unsigned long long)__double_as_longlong(bt);
        w[1] = (unsigned long long)(uint32_t)ba | ((unsigned long long)(uint32_t)bb << 32);
    }
    // the evaluation's ticket: this block's best written back before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the evaluation ---------------------------------------------------
    bt = -INFINITY;
    ba = bb = -1;
    for (int i = tid; i < (int)gridDim.x; i += kT) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(&slots[i]);
        const unsigned long long w0 =
            __hip_atomic_load(&w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long w1 =
            __hip_atomic_load(&w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        take_ahead(bt, ba, bb, __longlong_as_double((long long)w0), (int)(uint32_t)w1,
                   (int)(uint32_t)(w1 >> 32));
    }
    __syncthreads();   // (s_best's readers of the block's own reduction are done)
    block_first_max<W>(s_best, bt, ba, bb);
    if (tid == 0) {
        s_best[0] = RowBest{bt, ba, bb};
        s_cnt = 0;
        s->ticket = 0u;   // (the next launch draws from zero)
        // no admissible row, or the best exchange adds nothing; or it does and no move is left
        const bool gain = ba >= 0 && bt > s->T;
        const bool room = s->n_moves < max_moves;
        if (commit) {
            if (!gain) s->converged = 1;
            if (!gain || !room) s->done = 1;
        }
        s_flag = gain && room;
    }
    __syncthreads();
    if (!s_flag) return;
    bt = s_best[0].t;
    ba = s_best[0].a;
    bb = s_best[0].b;
    // the covered cells of the set after the move
    const double *la = Lc + (size_t)(ba - n_locked) * Cs, *sb = Sc + (size_t)bb * Cs;
    int32_t cnt = 0;
    for (int c = tid; c < C; c += kT) cnt += (la[c] > 0 || sb[c] > 0) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) {
        const int m = s->n_moves;
        s->move_slot[m] = ba;
        s->move_from[m] = s_set[ba];
        s->move_to[m] = bb;
        s->move_total[m] = bt;
        s->move_cov[m] = s_cnt;
        if (commit) {
            s->set[ba] = bb;
            s->T = bt;
            s->n_moves = m + 1;
        }
    }
}

// The final set folded in slot order: cell_score = fold(set), cell_owner the slot whose fold
// raised the cell last (ties keep the earlier owner).
__global__ void __launch_bounds__(kRT)
k_refine_final(const double *__restrict__ S, const double *__restrict__ Z, int C, int K,
               const RefineState *__restrict__ s, double *__restrict__ cs,
               int32_t *__restrict__ owner) {
    const int c = blockIdx.x * kRT + threadIdx.x;
    if (c >= C) return;
    double b = Z[c];
    int32_t own = owner_of_zx(b);
    for (int i = 0; i < K; ++i) fold_owner(b, own, S[(size_t)s->set[i] * C + c], i);
    cs[c] = b;
    owner[c] = own;
}

// the call's block on the device (refine_d) and, up to `down`, in the pinned landing:
// [state | cell_score f64 C | cell_owner i32 C | swap totals f64 E x K x P (only when asked for)];
// the scratch (refine_m): [Sc f64 Pp x Cs | Lc f64 kRTile x Cs | block bests]
struct RefinePlan {
    int C, P, Pp, Cs, nblk, ncb, K, n_locked, max_moves;
    CellBlock cb;   // tab_off = cb.rest_off
    size_t tab_off, bytes, lc_off, slot_off, m_bytes;
    bool dense;
};

RefinePlan make_plan(int C, int P, const pcp_refine_params *rp, bool dense) {
    RefinePlan s{};
    s.C = C;
    s.P = P;
    s.K = rp->k;
    s.n_locked = rp->n_locked;
    s.max_moves = rp->max_moves;
    s.nblk = (P + kRTile - 1) / kRTile;
    s.Pp = s.nblk * kRTile;
    s.Cs = (C + kWalkC - 1) / kWalkC * kWalkC;
    s.ncb = (C + kRT - 1) / kRT;
    s.dense = dense;
    s.cb = cell_block(sizeof(RefineState), C);
    s.tab_off = s.cb.rest_off;
    s.bytes = s.tab_off +
              (dense ? (size_t)(s.max_moves + 1) * s.K * P * sizeof(double) : 0);
    s.lc_off = (size_t)s.Pp * s.Cs * sizeof(double);
    s.slot_off = s.lc_off + (size_t)kRTile * s.Cs * sizeof(double);
    s.m_bytes = s.slot_off + (size_t)s.nblk * sizeof(RowBest);
    return s;
}

struct RefinePtrs {
    RefineState *state;
    double *cs, *table, *Sc, *Lc;
    int32_t *owner;
    RowBest *slots;
};

RefinePtrs pointers(pcp_ctx *ctx, const RefinePlan &s) {
    char *blk = ctx->refine_d.as<char>(), *m = ctx->refine_m.as<char>();
    RefinePtrs q;
    q.state = reinterpret_cast<RefineState *>(blk);
    q.cs = reinterpret_cast<double *>(blk + s.cb.score_off);
    q.owner = reinterpret_cast<int32_t *>(blk + s.cb.owner_off);
    q.table = s.dense ? reinterpret_cast<double *>(blk + s.tab_off) : nullptr;
    q.Sc = reinterpret_cast<double *>(m);
    q.Lc = reinterpret_cast<double *>(m + s.lc_off);
    q.slots = reinterpret_cast<RowBest *>(m + s.slot_off);
    return q;
}

int init_enqueue(pcp_ctx *ctx, const RefinePlan &s, const ScoreEnq &o, const RefineSet &start) {
    const RefinePtrs q = pointers(ctx, s);
    const size_t cells = (size_t)s.Pp * s.Cs;
    hipLaunchKernelGGL(k_refine_init, dim3((unsigned)((cells + kRT - 1) / kRT)), dim3(kRT), 0,
                       ctx->stream, (const double *)o.comb, s.C, s.P, s.Pp, s.Cs, start, s.K, q.Sc,
                       q.Lc, q.state);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// evaluation e's two launches on ctx->stream (C > 0; the buffers are large enough)
int eval_enqueue(pcp_ctx *ctx, const RefinePlan &s, const ScoreEnq &o, double sep2, int e,
                 bool first, bool commit) {
    const RefinePtrs q = pointers(ctx, s);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_refine_prep, dim3((unsigned)(s.ncb + (first ? 1 : 0))), dim3(kRT), 0, st,
                       (const double *)o.comb, (const double *)o.score_z, s.C, s.Cs, s.ncb, s.K,
                       s.n_locked, q.state, q.Lc);
    PCP_CHECK_LAUNCH(ctx);
    double *tab = q.table ? q.table + (size_t)e * s.K * s.P : nullptr;
    const int live = s.K - s.n_locked;   // a wave per kRSl unlocked slots: 1, 2 or 4
    auto launch = [&](auto kernel, int waves) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)s.nblk), dim3(64 * waves), 0, st,
                           (const double *)q.Lc, (const double *)q.Sc, s.Cs, s.C, s.P, s.K,
                           s.n_locked, o.poses_k, sep2, q.slots, tab, q.state, s.max_moves,
                           commit ? 1 : 0);
    };
    if (live <= kRSl)
        launch(k_refine_eval<1>, 1);
    else if (live <= 2 * kRSl)
        launch(k_refine_eval<2>, 2);
    else
        launch(k_refine_eval<4>, 4);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what both entries refuse before any launch; start = the set as the kernels take it
int check_args(pcp_ctx *ctx, const char *what, uint64_t n, const pcp_refine_params *rp,
               RefineSet &start) {
    if (rp->k < 1 || rp->k > PCP_PLACE_MAX || rp->n_locked < 0 || rp->n_locked > rp->k ||
        rp->max_moves < 0 || rp->max_moves > PCP_REFINE_MAX_MOVES || rp->reserved != 0)
        return set_err(ctx, PCP_E_INVALID,
                       "%s: k %d outside 1..%d, n_locked %d outside 0..k, max_moves %d outside "
                       "0..%d or reserved %d != 0",
                       what, (int)rp->k, PCP_PLACE_MAX, (int)rp->n_locked, (int)rp->max_moves,
                       PCP_REFINE_MAX_MOVES, (int)rp->reserved);
    return check_pose_list(ctx, what, "start", "in the set", rp->start, rp->k, n, start.idx);
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" int pcp_place_refine(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                                const pcp_vl_params *p, const pcp_refine_params *rp,
                                int64_t *selected, double *total, int32_t *covered,
                                double *start_total, int32_t *start_covered, int32_t *move_slot,
                                int64_t *move_from, int64_t *move_to, double *move_total,
                                int32_t *move_covered, double *swap_totals, double *cell_score,
                                int32_t *cell_owner, int32_t *n_moves, int32_t *converged) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !rp || !selected || !total || !covered || !start_total || !start_covered ||
        !n_moves || !converged || !poses5)
        return set_err(ctx, PCP_E_INVALID, "pcp_place_refine: null argument");
    RefineSet start{};
    if (int rc = check_args(ctx, "pcp_place_refine", n, rp, start)) return rc;
    if (rp->max_moves > 0 && (!move_slot || !move_from || !move_to || !move_total || !move_covered))
        return set_err(ctx, PCP_E_INVALID, "pcp_place_refine: null move array");
    // the scoring, no flags and no fused tail, as pcp_place_sensors runs it: comb [P][C], score_z
    // [C] on the device; a step table past PCP_MAX_STEPS is refused in there, before any launch
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P, K = rp->k;
    if (!C) {   // no cells: nothing to cover, nothing to gain
        if (int rc = stream_done(ctx)) return rc;
        for (int i = 0; i < K; ++i) selected[i] = rp->start[i];
        *total = *start_total = 0.0;
        *covered = *start_covered = 0;
        *n_moves = 0;
        *converged = 1;
        return PCP_OK;
    }
    const RefinePlan s = make_plan(C, P, rp, swap_totals != nullptr);
    const bool cells_out = cell_score || cell_owner;
    const size_t down = s.dense ? s.bytes : cells_out ? s.tab_off : s.cb.score_off;
    PCP_HIP(ctx, ctx->refine_d.ensure(s.bytes + 64));
    PCP_HIP(ctx, ctx->refine_m.ensure(s.m_bytes + 64));
    PCP_HIP(ctx, ctx->refine_host.ensure(down + 64));
    const double sep2 = sep2_of(rp->min_separation);
    if (int rc = init_enqueue(ctx, s, o, start)) return rc;
    // every evaluation the moves allow, back to back: those behind the stop return at once
    for (int e = 0; e <= s.max_moves; ++e)
        if (int rc = eval_enqueue(ctx, s, o, sep2, e, e == 0, true)) return rc;
    const RefinePtrs q = pointers(ctx, s);
    if (cells_out) {
        hipLaunchKernelGGL(k_refine_final, dim3((unsigned)s.ncb), dim3(kRT), 0, st,
                           (const double *)o.comb, (const double *)o.score_z, C, K,
                           (const RefineState *)q.state, q.cs, q.owner);
        PCP_CHECK_LAUNCH(ctx);
    }
    char *pin = ctx->refine_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, ctx->refine_d.as<char>(), down, hipMemcpyDeviceToHost, st));
    if (int rc = stream_done(ctx)) return rc;
    const RefineState *h = reinterpret_cast<const RefineState *>(pin);
    const int nm = h->n_moves;
    for (int i = 0; i < K; ++i) selected[i] = h->set[i];
    *start_total = h->start_total;
    *start_covered = h->start_cov;
    *total = h->T;
    *covered = nm ? h->move_cov[nm - 1] : h->start_cov;
    for (int m = 0; m < nm; ++m) {
        move_slot[m] = h->move_slot[m];
        move_from[m] = h->move_from[m];
        move_to[m] = h->move_to[m];
        move_total[m] = h->move_total[m];
        move_covered[m] = h->move_cov[m];
    }
    *n_moves = nm;
    *converged = h->converged;
    if (swap_totals)
        host_copy(ctx, swap_totals, pin + s.tab_off, (size_t)(nm + 1) * K * P * sizeof(double));
    copy_cells(pin, s.cb, C, cell_score, cell_owner);
    return PCP_OK;
}

extern "C" int pcp_place_refine_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                      const double zx[5], const pcp_vl_params *p,
                                      const pcp_refine_params *rp, int reps, double *ms_per_eval) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !rp || !ms_per_eval || !poses5 || n == 0 || reps <= 0)
        return set_err(ctx, PCP_E_INVALID,
                       "pcp_place_refine_burst: null argument or nothing to time");
    RefineSet start{};
    if (int rc = check_args(ctx, "pcp_place_refine_burst", n, rp, start)) return rc;
    *ms_per_eval = 0.0;
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    if (!o.C) {
        if (int rc = stream_done(ctx)) return rc;
        return set_err(ctx, PCP_E_INVALID, "pcp_place_refine_burst: no cells, nothing to time");
    }
    const RefinePlan s = make_plan(o.C, o.P, rp, false);
    PCP_HIP(ctx, ctx->refine_d.ensure(s.bytes + 64));
    PCP_HIP(ctx, ctx->refine_m.ensure(s.m_bytes + 64));
    const double sep2 = sep2_of(rp->min_separation);
    // the start set's evaluation, over and over: nothing is committed, so every repetition does
    // the whole work of a live evaluation.  Once untimed: the start total and the first touches
    auto warm = [&] {
        const int rc = init_enqueue(ctx, s, o, start);
        return rc ? rc : eval_enqueue(ctx, s, o, sep2, 0, true, false);
    };
    auto body = [&] { return eval_enqueue(ctx, s, o, sep2, 0, false, false); };
    return time_reps(ctx, "pcp_place_refine_burst", ctx->stream, reps, warm, body, ms_per_eval);
}
