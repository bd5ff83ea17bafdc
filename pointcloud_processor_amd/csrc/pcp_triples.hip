// pcp_triples.hip -- the exact best triple of mobile sensors (pcp_place_triple): every triple
// a < b < c of the admissible poses gets t[a][b][c] = osum(max(max(max(base, S[a]), S[b]), S[c])),
// and the first maximum wins (include/pcp_abi.h has the definition; DESIGN.md §6k the kernels and
// their timing).  The base, the singles and the pairs are the pair phase's (pcp_pair_phase.hpp),
// run inside the call; it also leaves the clamped rows M [Pp][Cs] and the admissible mask that
// the triples read.  A triple's term is max(max(M[b][c], M[c'][c]), M[a][c]): max selects one of
// its operands, so the order of a, b, c in the fold changes no bit; the adds of a chain run in
// ascending cell order from +0.0, one rounded add per cell.
//
// After the pair phase, ordered by the stream alone (no block ever waits for another):
//   k_triple_clear   the dense table's -inf background (only when the table is asked for)
//   k_triple_tiles   kTripleSub blocks per tile triple ta <= tb <= tc (pcp_triple_tiles.hpp)
//   k_triple_rows    one wave per pose a: the first maximum over (b, c) of its blocks' bests
//   k_triple_select  the best triple, its covered count, the answer's size (step 6) and the
//                    answer folded into cell_score / cell_owner
#include <cmath>
#include <cstring>

#include "pcp_pair_phase.hpp"
#include "pcp_triple_tiles.hpp"

namespace pcp {
namespace {

constexpr int kTS = 1024;                                   // threads of the selection's one block
constexpr int kTRows = 2 * kTripleTile + kTripleA;          // staged rows: B, C, then the A group
constexpr int kTLd2 = kWalkLd / 2;                          // a staged row in double2
constexpr int kTCol2 = kWalkC / 2;                          // a chunk of a row in double2
constexpr int kTALoads = (kTripleA * kTCol2 + kTripleLanes - 1) / kTripleLanes;
static_assert(kTripleLanes / kTCol2 == kTripleTile / 2, "a thread loads two rows of B and of C");

// the call's result record (downloaded)
struct TripleState {
    int64_t triple[3];
    double triple_total;
    int64_t pair[2];
    double pair_total;
    int64_t single;
    double single_total;
    double base_total;
    int32_t triple_cov, pair_cov, single_cov, base_cov, n_sel, pad[3];
};
static_assert(sizeof(TripleState) == 112, "the cells' block follows on a 16-byte boundary");

__global__ void __launch_bounds__(256) k_triple_clear(double *__restrict__ table, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256)
        table[i] = -INFINITY;
}

// One A group of a tile triple per block of four waves.  Lane (jb, jc) owns the poses b and c of
// the B and C tiles and runs kTripleA chains, one per pose a of the group: per cell it forms
// m = max(M[b], M[c]) once and adds max(m, M[a]) to chain a.  The block stages chunks of kWalkC
// cells of its 16 B rows, 16 C rows and kTripleA A rows as k_pair_tiles does (coalesced b128 loads
// of M, one chunk ahead in registers, rows kWalkLd apart in LDS); a lane reads two cells of its B
// row and of its C row per ds_read_b128 and the A rows by broadcast.  A tile triple with no
// admissible row in one of its three parts loads nothing.  Each chain's first maximum over the
// block's (b, c) goes to slots[block][chain].
__global__ void __launch_bounds__(kTripleLanes)
k_triple_tiles(const double *__restrict__ M, int Cs, int n, int nt,
               const uint32_t *__restrict__ adm, const double *__restrict__ poses5, double sep2,
               RowBest *__restrict__ slots, double *__restrict__ table) {
    __shared__ double2 s_m[2][kTRows * kTLd2];
    __shared__ int s_live[3];
    __shared__ RowBest s_best[kTripleA][kTripleLanes / 64];
    const int tid = threadIdx.x;
    const int sub = (int)blockIdx.x % kTripleSub;
    const TripleTile tile = triple_tile_of(nt, (int)blockIdx.x / kTripleSub);
    const int rowB = tile.tb * kTripleTile, rowC = tile.tc * kTripleTile,
              rowA = tile.ta * kTripleTile + sub * kTripleA;   // (all below nt kTripleTile rows)
    if (tid < 3) s_live[tid] = 0;
    __syncthreads();
    if (tid < kTRows) {
        const int part = tid < kTripleTile ? 0 : tid < 2 * kTripleTile ? 1 : 2;
        const int row = part == 0   ? rowB + tid
                        : part == 1 ? rowC + tid - kTripleTile
                                    : rowA + tid - 2 * kTripleTile;
        if (adm[row] != 0u) s_live[part] = 1;   // (benign race: every writer stores 1)
    }
    __syncthreads();
    const bool live = s_live[0] != 0 && s_live[1] != 0 && s_live[2] != 0;
    double acc[kTripleA];
#pragma unroll
    for (int s = 0; s < kTripleA; ++s) acc[s] = 0.0;
    if (live) {   // (uniform)
        const int nch = Cs / kWalkC;
        const int jb = tid / kTripleTile, jc = kTripleTile + tid % kTripleTile;
        // a thread's b128 loads per chunk: double2 `col` of the rows r0 and r0 + 8 of B and of C,
        // and of the A group's rows r0, r0 + 8 .. below kTripleA
        const int r0 = tid / kTCol2, col = tid % kTCol2;
        const size_t half = (size_t)(kTripleTile / 2) * Cs / 2;   // 8 rows of M in double2
        const double2 *srcB = reinterpret_cast<const double2 *>(M + (size_t)(rowB + r0) * Cs) + col;
        const double2 *srcC = reinterpret_cast<const double2 *>(M + (size_t)(rowC + r0) * Cs) + col;
        const double2 *srcA = reinterpret_cast<const double2 *>(M + (size_t)(rowA + r0) * Cs) + col;
        const int dst = r0 * kTLd2 + col;
        constexpr int kHalf = (kTripleTile / 2) * kTLd2;   // 8 staged rows in double2
        double2 rB0, rB1, rC0, rC1, rA[kTALoads];
        auto load = [&](int k) {
            const size_t o = (size_t)k * kTCol2;
            rB0 = srcB[o];
            rB1 = srcB[o + half];
            rC0 = srcC[o];
            rC1 = srcC[o + half];
#pragma unroll
            for (int i = 0; i < kTALoads; ++i)
                if (r0 + 8 * i < kTripleA) rA[i] = srcA[o + i * half];
        };
        auto store = [&](int buf) {
            double2 *d = s_m[buf] + dst;
            d[0] = rB0;
            d[kHalf] = rB1;
            d[2 * kHalf] = rC0;
            d[3 * kHalf] = rC1;
#pragma unroll
            for (int i = 0; i < kTALoads; ++i)
                if (r0 + 8 * i < kTripleA) d[(4 + i) * kHalf] = rA[i];
        };
        load(0);
        store(0);
        __syncthreads();
        for (int k = 0; k < nch; ++k) {
            // (unconditional, as in k_pair_tiles: the last chunk is loaded and stored once more,
            // into the buffer no one reads again)
            load(min(k + 1, nch - 1));
            const double2 *vb = s_m[k & 1] + jb * kTLd2, *vc = s_m[k & 1] + jc * kTLd2,
                          *va = s_m[k & 1] + 2 * kTripleTile * kTLd2;
            // two register groups of 2 + kTripleA b128 reads, as walk_chunk's: one group's reads
            // are in flight under the other's maxima and adds (a block may be alone on its CU,
            // one wave per SIMD: nothing else hides the LDS latency)
            struct Grp {
                double2 b, c, a[kTripleA];
            };
            auto rd = [&](Grp &g, int j) {
                g.b = vb[j];
                g.c = vc[j];
#pragma unroll
                for (int s = 0; s < kTripleA; ++s) g.a[s] = va[s * kTLd2 + j];
            };
            auto run = [&](const Grp &g) {
                const double mx = max_pos(g.b.x, g.c.x), my = max_pos(g.b.y, g.c.y);
#pragma unroll
                for (int s = 0; s < kTripleA; ++s) {
                    acc[s] += max_pos(mx, g.a[s].x);
                    acc[s] += max_pos(my, g.a[s].y);
                }
            };
            Grp g0, g1;
            rd(g0, 0);
            // (not unrolled: unrolled, the compiler lifts later groups' reads to the front -- with
            // 8 chains per lane 228 VGPRs at two iterations, spills at all sixteen)
#pragma unroll 1
            for (int j = 0; j < kTCol2; j += 2) {
                rd(g1, j + 1);
                __builtin_amdgcn_sched_barrier(0);
                run(g0);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 2 < kTCol2) rd(g0, j + 2);
                __builtin_amdgcn_sched_barrier(0);
                run(g1);
                __builtin_amdgcn_sched_barrier(0);
            }
            store((k + 1) & 1);
            __syncthreads();
        }
    }
    const TripleSlot l0 = triple_slot(tile, sub, tid, 0);
    bool bc_ok = l0.b < l0.c && l0.c < n && adm[l0.b] != 0u && adm[l0.c] != 0u;
    if (bc_ok && sep2 > 0) bc_ok = !closer_than(poses5, l0.b, l0.c, sep2);
#pragma unroll
    for (int s = 0; s < kTripleA; ++s) {
        const TripleSlot ts = triple_slot(tile, sub, tid, s);
        bool ok = bc_ok && triple_is_triple(ts, n) && adm[ts.a] != 0u;
        if (ok && sep2 > 0)
            ok = !closer_than(poses5, ts.a, ts.b, sep2) && !closer_than(poses5, ts.a, ts.c, sep2);
        double bt = ok ? acc[s] : -INFINITY;
        if (table && ok) table[((size_t)ts.a * n + ts.b) * n + ts.c] = bt;
        // the chain's first maximum over the block's (b, c) in row-major order
        int bb = ok ? ts.b : -1, bc = ok ? ts.c : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            take_ahead(bt, bb, bc, __shfl_xor(bt, o, 64), __shfl_xor(bb, o, 64),
                       __shfl_xor(bc, o, 64));
        if ((tid & 63) == 0) s_best[s][tid >> 6] = RowBest{bt, bb, bc};
    }
    __syncthreads();
    if (tid < kTripleA) {
        RowBest r = s_best[tid][0];
        for (int w = 1; w < kTripleLanes / 64; ++w)
            take_ahead(r.t, r.a, r.b, s_best[tid][w].t, s_best[tid][w].a, s_best[tid][w].b);
        slots[(size_t)blockIdx.x * kTripleA + tid] = r;
    }
}

// One wave per pose a: the first maximum over (b, c) of the bests its blocks left (ties to the
// lexicographically smaller (b, c): row-major order); -inf and (-1, -1) where a starts no triple.
__global__ void __launch_bounds__(64)
k_triple_rows(const RowBest *__restrict__ slots, int nt, double *__restrict__ first_totals,
              int32_t *__restrict__ first_partners) {
    const int a = blockIdx.x, tid = threadIdx.x;
    const int ta = a / kTripleTile, sub = a % kTripleTile / kTripleA, s = a % kTripleA;
    const int start = triple_row_start(nt, ta), cnt = triple_row_count(nt, ta);
    double t = -INFINITY;
    int b = -1, c = -1;
    for (int j = tid; j < cnt; j += 64) {
        const RowBest v = slots[((size_t)(start + j) * kTripleSub + sub) * kTripleA + s];
        take_ahead(t, b, c, v.t, v.a, v.b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        take_ahead(t, b, c, __shfl_xor(t, o, 64), __shfl_xor(b, o, 64), __shfl_xor(c, o, 64));
    if (tid == 0) {
        first_totals[a] = b >= 0 ? t : -INFINITY;
        first_partners[2 * a] = b;
        first_partners[2 * a + 1] = c;
    }
}

// Selection, one block: the first maximum over a of first_totals (ties to the lower a: with the
// rows' order, the lexicographically first maximal triple), its covered count from M's rows, the
// answer's size by step 6 from the pair phase's record, and the answer folded into cell_score /
// cell_owner from the base (recomputed here: the pair phase folds its own answer into its copy).
__global__ void __launch_bounds__(kTS)
k_triple_select(const double *__restrict__ first_totals, const int32_t *__restrict__ first_partners,
                int P, int Cs, const double *__restrict__ M, const double *__restrict__ S,
                const double *__restrict__ Z, int C, PairFixed fx,
                const PairState *__restrict__ ps, double *__restrict__ cs,
                int32_t *__restrict__ owner, TripleState *__restrict__ st) {
    __shared__ RowBest s_best[kTS / 64];
    __shared__ int32_t s_tc;
    const int tid = threadIdx.x;
    double bt = -INFINITY;
    int ba = -1, bz = 0;
    for (int a = tid; a < P; a += kTS)
        if (first_partners[2 * a] >= 0) take_ahead(bt, ba, bz, first_totals[a], a, 0);
    block_first_max_all<kTS / 64>(s_best, bt, ba, bz);
    if (tid == 0) s_tc = 0;
    __syncthreads();
    const int tb = ba >= 0 ? first_partners[2 * ba] : -1, tc = ba >= 0 ? first_partners[2 * ba + 1] : -1;
    const PairState q = *ps;   // (the pair phase's, earlier launches)
    int n_sel = 0;
    double T = q.base_total;
    if (q.single >= 0 && q.single_total > T) {
        n_sel = 1;
        T = q.single_total;
    }
    if (q.pair[0] >= 0 && q.pair_total > T) {
        n_sel = 2;
        T = q.pair_total;
    }
    if (ba >= 0 && bt > T) n_sel = 3;
    // the chosen poses in ascending index order
    int ch[3] = {-1, -1, -1};
    if (n_sel == 1) ch[0] = (int)q.single;
    if (n_sel == 2) {
        ch[0] = (int)q.pair[0];
        ch[1] = (int)q.pair[1];
    }
    if (n_sel == 3) {
        ch[0] = ba;
        ch[1] = tb;
        ch[2] = tc;
    }
    int32_t cov = 0;
    for (int c = tid; c < C; c += kTS) {
        if (ba >= 0)
            cov += (M[(size_t)ba * Cs + c] > 0 || M[(size_t)tb * Cs + c] > 0 ||
                    M[(size_t)tc * Cs + c] > 0)
                       ? 1
                       : 0;
        double x = Z[c];
        int32_t own = owner_of_zx(x);
        for (int i = 0; i < fx.n; ++i) fold_owner(x, own, S[(size_t)fx.idx[i] * C + c], i);
        for (int i = 0; i < n_sel; ++i) fold_owner(x, own, S[(size_t)ch[i] * C + c], fx.n + i);
        cs[c] = x;
        owner[c] = own;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cov += __shfl_xor(cov, o, 64);
    if ((tid & 63) == 0 && cov) atomicAdd(&s_tc, cov);
    __syncthreads();
    if (tid == 0) {
        st->triple[0] = ba;
        st->triple[1] = tb;
        st->triple[2] = tc;
        st->triple_total = bt;
        st->pair[0] = q.pair[0];
        st->pair[1] = q.pair[1];
        st->pair_total = q.pair_total;
        st->single = q.single;
        st->single_total = q.single_total;
        st->base_total = q.base_total;
        st->triple_cov = s_tc;
        st->pair_cov = q.pair_cov;
        st->single_cov = q.single_cov;
        st->base_cov = q.base_cov;
        st->n_sel = n_sel;
    }
}

// the call's block on the device (triple_d) and, up to `down`, in the pinned landing:
// [state | cell_score f64 C | cell_owner i32 C | first_totals f64 P | first partners i32 P x 2 |
//  block bests | triple table f64 P x P x P (only when asked for)]
struct TriplePlan {
    PairPlan pair;   // the pair phase, no dense pair table
    int nblk;
    CellBlock cb;    // ft_off = cb.rest_off
    size_t ft_off, fp_off, slot_off, tab_off, tab_count, bytes;
    bool dense;
};

TriplePlan make_triple_plan(int C, int P, bool dense) {
    TriplePlan t{};
    t.pair = make_plan(C, P, false);
    t.nblk = triple_blocks(t.pair.nt);
    t.dense = dense;
    t.cb = cell_block(sizeof(TripleState), C);
    t.ft_off = t.cb.rest_off;
    t.fp_off = a16(t.ft_off + (size_t)P * sizeof(double));
    t.slot_off = a16(t.fp_off + (size_t)P * 2 * sizeof(int32_t));
    t.tab_off = a16(t.slot_off + (size_t)t.nblk * kTripleA * sizeof(RowBest));
    t.tab_count = dense ? (size_t)P * P * P : 0;
    t.bytes = t.tab_off + t.tab_count * sizeof(double);
    return t;
}

// the pair phase, then the triples' launches on ctx->stream (C > 0; the buffers are large enough)
int triple_enqueue(pcp_ctx *ctx, const TriplePlan &t, const ScoreEnq &o, const PairFixed &fx,
                   double sep2) {
    if (int rc = pair_enqueue(ctx, t.pair, o, fx, sep2)) return rc;
    hipStream_t st = ctx->stream;
    const PairPlan &s = t.pair;
    char *pblk = ctx->pair_d.as<char>();
    const PairState *pstate = reinterpret_cast<const PairState *>(pblk);
    const uint32_t *adm = reinterpret_cast<const uint32_t *>(pblk + s.adm_off);
    const double *M = ctx->pair_m.as<double>();
    char *blk = ctx->triple_d.as<char>();
    TripleState *state = reinterpret_cast<TripleState *>(blk);
    double *cs = reinterpret_cast<double *>(blk + t.cb.score_off);
    int32_t *owner = reinterpret_cast<int32_t *>(blk + t.cb.owner_off);
    double *ft = reinterpret_cast<double *>(blk + t.ft_off);
    int32_t *fp = reinterpret_cast<int32_t *>(blk + t.fp_off);
    RowBest *slots = reinterpret_cast<RowBest *>(blk + t.slot_off);
    double *table = t.dense ? reinterpret_cast<double *>(blk + t.tab_off) : nullptr;
    if (t.nblk) {
        if (table) {
            const unsigned g = (unsigned)std::min<size_t>((t.tab_count + 255) / 256, 4096);
            hipLaunchKernelGGL(k_triple_clear, dim3(g), dim3(256), 0, st, table, t.tab_count);
            PCP_CHECK_LAUNCH(ctx);
        }
        hipLaunchKernelGGL(k_triple_tiles, dim3((unsigned)t.nblk), dim3(kTripleLanes), 0, st, M,
                           s.Cs, s.P, s.nt, adm, o.poses_k, sep2, slots, table);
        PCP_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_triple_rows, dim3((unsigned)s.P), dim3(64), 0, st,
                           (const RowBest *)slots, s.nt, ft, fp);
        PCP_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(k_triple_select, dim3(1), dim3(kTS), 0, st, (const double *)ft,
                       (const int32_t *)fp, s.P, s.Cs, M, (const double *)o.comb,
                       (const double *)o.score_z, s.C, fx, pstate, cs, owner, state);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what both entries refuse before any launch, beyond the pair call's own list
int check_triple_args(pcp_ctx *ctx, const char *what, uint64_t n, const pcp_pair_params *pp,
                      bool table, PairFixed &fx) {
    if (n > PCP_TRIPLE_MAX_POSES)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses, at most %d per call", what,
                       (unsigned long long)n, PCP_TRIPLE_MAX_POSES);
    if (table && n > PCP_TRIPLE_TABLE_MAX_POSES)
        return set_err(ctx, PCP_E_INVALID, "%s: triple_totals with %llu poses, at most %d", what,
                       (unsigned long long)n, PCP_TRIPLE_TABLE_MAX_POSES);
    return check_args(ctx, what, n, pp, fx);
}

}  // namespace
}  // namespace pcp

using namespace pcp;

extern "C" int pcp_place_triple(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx[5],
                                const pcp_vl_params *p, const pcp_pair_params *pp,
                                int64_t best_triple[3], double *triple_total,
                                int32_t *triple_covered, int64_t best_pair[2], double *pair_total,
                                int32_t *pair_covered, int64_t *best_single, double *single_total,
                                int32_t *single_covered, double *base_total,
                                int32_t *base_covered, double *first_totals,
                                int64_t *first_partners, double *triple_totals,
                                double *cell_score, int32_t *cell_owner, int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !pp || !best_triple || !triple_total || !triple_covered || !best_pair ||
        !pair_total || !pair_covered || !best_single || !single_total || !single_covered ||
        !base_total || !base_covered || !n_selected || (n && !poses5))
        return set_err(ctx, PCP_E_INVALID, "pcp_place_triple: null argument");
    PairFixed fx{};
    if (int rc = check_triple_args(ctx, "pcp_place_triple", n, pp, triple_totals != nullptr, fx))
        return rc;
    // the scoring as pcp_place_pair runs it; a step table past PCP_MAX_STEPS is refused in there,
    // before any launch
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    hipStream_t st = ctx->stream;
    const int C = o.C, P = o.P;
    auto nothing = [&] {
        best_triple[0] = best_triple[1] = best_triple[2] = -1;
        *triple_total = -INFINITY;
        *triple_covered = 0;
        best_pair[0] = best_pair[1] = -1;
        *pair_total = -INFINITY;
        *pair_covered = 0;
        *best_single = -1;
        *single_total = -INFINITY;
        *single_covered = 0;
        *n_selected = 0;
    };
    auto no_rows = [&] {   // the tables of a call without triples
        for (int a = 0; a < P; ++a) {
            if (first_totals) first_totals[a] = -INFINITY;
            if (first_partners) first_partners[2 * a] = first_partners[2 * a + 1] = -1;
        }
        if (triple_totals)
            for (size_t i = 0; i < (size_t)P * P * P; ++i) triple_totals[i] = -INFINITY;
    };
    if (!C) {   // no cells: nothing to cover
        if (int rc = stream_done(ctx)) return rc;
        nothing();
        no_rows();
        *base_total = 0.0;
        *base_covered = 0;
        return PCP_OK;
    }
    const TriplePlan t = make_triple_plan(C, P, triple_totals != nullptr);
    const bool cells_out = cell_score || cell_owner;
    const size_t down = t.dense                           ? t.bytes
                        : (first_totals || first_partners) ? t.slot_off
                        : cells_out                        ? t.ft_off
                                                           : t.cb.score_off;
    PCP_HIP(ctx, ctx->pair_d.ensure(t.pair.bytes + 64));
    PCP_HIP(ctx, ctx->pair_m.ensure(t.pair.m_bytes + 64));
    PCP_HIP(ctx, ctx->triple_d.ensure(t.bytes + 64));
    PCP_HIP(ctx, ctx->triple_host.ensure(down + 64));
    if (int rc = triple_enqueue(ctx, t, o, fx, sep2_of(pp->min_separation))) return rc;
    char *pin = ctx->triple_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, ctx->triple_d.as<char>(), down, hipMemcpyDeviceToHost, st));
    if (int rc = stream_done(ctx)) return rc;
    const TripleState *h = reinterpret_cast<const TripleState *>(pin);
    nothing();
    if (P && h->triple[0] >= 0) {
        for (int i = 0; i < 3; ++i) best_triple[i] = h->triple[i];
        *triple_total = h->triple_total;
        *triple_covered = h->triple_cov;
    }
    best_pair[0] = h->pair[0];
    best_pair[1] = h->pair[1];
    if (h->pair[0] >= 0) {
        *pair_total = h->pair_total;
        *pair_covered = h->pair_cov;
    }
    *best_single = h->single;
    if (h->single >= 0) {
        *single_total = h->single_total;
        *single_covered = h->single_cov;
    }
    *base_total = h->base_total;
    *base_covered = h->base_cov;
    *n_selected = h->n_sel;
    if (P) {
        if (first_totals) std::memcpy(first_totals, pin + t.ft_off, (size_t)P * sizeof(double));
        if (first_partners) {
            const int32_t *fp = reinterpret_cast<const int32_t *>(pin + t.fp_off);
            for (int i = 0; i < 2 * P; ++i) first_partners[i] = fp[i];
        }
        if (triple_totals)
            host_copy(ctx, triple_totals, pin + t.tab_off, t.tab_count * sizeof(double));
    }
    copy_cells(pin, t.cb, C, cell_score, cell_owner);
    return PCP_OK;
}

extern "C" int pcp_place_triple_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                      const double zx[5], const pcp_vl_params *p,
                                      const pcp_pair_params *pp, int reps, double *ms_per_rep) {
    if (!ctx) return PCP_E_INVALID;
    if (int rc = area_finish(ctx)) return rc;
    if (!zx || !p || !pp || !ms_per_rep || !poses5 || n < 3 || reps <= 0)
        return set_err(ctx, PCP_E_INVALID,
                       "pcp_place_triple_burst: null argument or nothing to time");
    PairFixed fx{};
    if (int rc = check_triple_args(ctx, "pcp_place_triple_burst", n, pp, false, fx)) return rc;
    *ms_per_rep = 0.0;
    ScoreEnq o;
    if (int rc = score_enqueue(ctx, poses5, n, zx, p, o)) return rc;
    if (!o.C) {
        if (int rc = stream_done(ctx)) return rc;
        return set_err(ctx, PCP_E_INVALID, "pcp_place_triple_burst: no cells, nothing to time");
    }
    const TriplePlan t = make_triple_plan(o.C, o.P, false);
    PCP_HIP(ctx, ctx->pair_d.ensure(t.pair.bytes + 64));
    PCP_HIP(ctx, ctx->pair_m.ensure(t.pair.m_bytes + 64));
    PCP_HIP(ctx, ctx->triple_d.ensure(t.bytes + 64));
    const double sep2 = sep2_of(pp->min_separation);
    auto once = [&] { return triple_enqueue(ctx, t, o, fx, sep2); };
    return time_reps(ctx, "pcp_place_triple_burst", ctx->stream, reps, once, once, ms_per_rep);
}
