// The pair phase of the placement searches: k_pair_prep, k_pair_tiles, k_pair_select,
// their plan and pair_enqueue, as pcp_pairs.hip held them.  pcp_place_pair (pcp_pairs.hip) runs it
// as its whole search; pcp_place_triple (pcp_triples.hip) runs it for its steps 1-4 and reads the
// clamped rows M, the admissible mask and the PairState it leaves in ctx->pair_d / ctx->pair_m.
// The unnamed namespace gives each of the two translation units its own copy of the kernels.
#pragma once

#include <cmath>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_pair_tiles.hpp"
#include "pcp_place_shared.hpp"

namespace pcp {
namespace {

constexpr int kQT = 256;        // threads per block of the preparation
constexpr int kQS = 1024;       // threads of the selection's one block
constexpr int kQRows = 2 * kPairTile;                      // a tile pair's A rows and B rows
constexpr int kQLoads = kQRows * (kWalkC / 2) / kPairLanes;    // b128 loads per thread per chunk
static_assert(kPairSub == 1 && kPairLanes == 256, "k_pair_tiles: one pair per lane, four waves");
static_assert(kQRows * (kWalkC / 2) % kPairLanes == 0, "whole b128 loads per thread");

// the call's result record (downloaded)
struct PairState {
    int64_t pair[2];
    double pair_total;
    int64_t single;
    double single_total;
    double base_total;
    int32_t pair_cov, single_cov, base_cov, n_sel;
};
static_assert(sizeof(PairState) == 64, "the cells' block follows on a 16-byte boundary");

struct PairFixed {
    int32_t n;
    int32_t idx[PCP_PLACE_MAX];
};

// Preparation.  Block (cc, g) of the first ncc * npg: cells cc kWalkC .., poses g kPairTile ..: the
// base of its cells from Z and the fixed rows (every block its own: no block waits for
// another), then its poses' clamped rows into M [Pp][Cs] (+0.0 in the rows past P and the cells
// past C).  The blocks with g == 0 store base / owner, those with cc == 0 the admissible mask.
// The last block computes the base total: with no fixed sensor it is the scoring's zx120 row
// sum, otherwise an ordered chain over the clamped base (one lane; the other threads stage and
// count).
__global__ void __launch_bounds__(kQT)
k_pair_prep(const double *__restrict__ S, const double *__restrict__ Z, int C, int P, int Pp,
            int Cs, int ncc, int npg, PairFixed fx, const double *__restrict__ poses5,
            double sep2, const double *__restrict__ tot, const int32_t *__restrict__ cov,
            double *__restrict__ base, int32_t *__restrict__ owner, uint32_t *__restrict__ adm,
            double *__restrict__ M, PairState *__restrict__ st) {
    __shared__ double s_b[kQT];
    __shared__ int32_t s_cnt;
    const int tid = threadIdx.x;
    auto base_of = [&](int c, int32_t &own) {
        double b = Z[c];
        own = owner_of_zx(b);
        for (int i = 0; i < fx.n; ++i) fold_owner(b, own, S[(size_t)fx.idx[i] * C + c], i);
        return b;
    };
    if ((int)blockIdx.x == ncc * npg) {   // ---- the base total
        if (fx.n == 0) {
            if (tid == 0) {
                st->base_total = tot[P];
                st->base_cov = cov[P];
            }
            return;
        }
        const double acc = ordered_total<kQT>(
            [&](int c) {
                int32_t own;
                return base_of(c, own);
            },
            C, s_b, s_cnt);
        if (tid == 0) {
            st->base_total = acc;
            st->base_cov = s_cnt;
        }
        return;
    }
    const int cc = blockIdx.x % ncc, g = blockIdx.x / ncc;
    if (tid < kWalkC) {
        const int c = cc * kWalkC + tid;
        if (c < C) {
            int32_t own;
            const double b = base_of(c, own);
            s_b[tid] = b;
            if (g == 0) {
                base[c] = b;
                owner[c] = own;
            }
        }
    }
    if (cc == 0 && tid < kPairTile && Pp) {
        const int p = g * kPairTile + tid;
        bool ok = p < P;
        if (ok) {
            const double px = poses5[5 * (size_t)p], py = poses5[5 * (size_t)p + 1];
            for (int i = 0; i < fx.n; ++i) {
                const int f = fx.idx[i];
                ok &= f != p;
                if (sep2 > 0) ok &= !closer_than(px, py, poses5, f, sep2);
            }
        }
        adm[p] = ok ? 1u : 0u;
    }
    if (!Pp) return;   // (uniform) no poses: the base alone
    __syncthreads();
    const int cl = tid & (kWalkC - 1), c = cc * kWalkC + cl;   // (c < Cs: Cs is whole chunks)
#pragma unroll
    for (int k = 0; k < kPairTile * kWalkC / kQT; ++k) {
        const int p = g * kPairTile + (tid >> 6) + (kQT / kWalkC) * k;
        double x = 0.0;   // rows past P and cells past C: +0.0
        if (p < P && c < C) {
            const double v = S[(size_t)p * C + c], b = s_b[cl];
            x = (b < v) ? v : b;
            x = x > 0 ? x : 0.0;
        }
        M[(size_t)p * Cs + c] = x;
    }
}

// One tile pair (ta <= tb) per block of four waves; lane (ia, jb) owns the pair of A row ia and
// B row jb: one f64 chain, adding its cells in ascending order from +0.0, one rounded add per
// cell (+0.0 for the cells that are not positive and for the padding past C: bit-neutral).  The
// block stages chunks of kWalkC cells of its 16 A rows and 16 B rows -- coalesced b128 loads of M,
// one chunk ahead in registers, stored to LDS as they lie, rows kWalkLd apart -- and every lane
// reads two cells of its A row and of its B row per ds_read_b128: a group of 16 lanes reads at
// most 16 B rows, 4 banks apart each, and its A rows by broadcast.  A tile with no admissible A
// row or B row loads nothing.
__global__ void __launch_bounds__(kPairLanes)
k_pair_tiles(const double *__restrict__ M, int Cs, int n, int nt,
             const uint32_t *__restrict__ adm, const double *__restrict__ poses5, double sep2,
             double *__restrict__ singles, RowBest *__restrict__ slots,
             double *__restrict__ table) {
    __shared__ double2 s_m[2][kQRows * kWalkLd / 2];
    __shared__ int s_live[2];
    __shared__ RowBest s_best[kPairLanes / 64];
    const int tid = threadIdx.x;
    const PairTile tile = pair_tile_of(nt, (int)blockIdx.x);
    const int ta = tile.ta, tb = tile.tb;
    if (tid < 2) s_live[tid] = 0;
    __syncthreads();
    if (tid < kQRows && adm[(tid < kPairTile ? ta : tb) * kPairTile + (tid & (kPairTile - 1))] != 0u)
        s_live[tid / kPairTile] = 1;   // (benign race: every writer stores 1)
    __syncthreads();
    const bool live = s_live[0] != 0 && s_live[1] != 0;
    double acc = 0.0;
    if (live) {   // (uniform)
        const int nch = Cs / kWalkC;
        const int ia = tid / kPairSide, jb = kPairTile + tid % kPairSide;
        // a thread's four b128 loads per chunk: double2 `col` of the rows r0 and r0 + 8 of A and
        // of B (32 threads per row: 512 contiguous bytes)
        static_assert(kQLoads == 4 && kPairLanes / (kWalkC / 2) == kPairTile / 2,
                      "two rows of each");
        const int r0 = tid / (kWalkC / 2), col = tid % (kWalkC / 2);
        const size_t half = (size_t)(kPairTile / 2) * Cs / 2;   // 8 rows of M in double2
        const double2 *srcA =
            reinterpret_cast<const double2 *>(M + (size_t)(ta * kPairTile + r0) * Cs) + col;
        const double2 *srcB =
            reinterpret_cast<const double2 *>(M + (size_t)(tb * kPairTile + r0) * Cs) + col;
        const int dst = r0 * (kWalkLd / 2) + col;
        constexpr int kHalf = (kPairTile / 2) * (kWalkLd / 2);     // 8 staged rows in double2
        double2 rA0, rA1, rB0, rB1;
        auto load = [&](int k) {
            const size_t o = (size_t)k * (kWalkC / 2);
            rA0 = srcA[o];
            rA1 = srcA[o + half];
            rB0 = srcB[o];
            rB1 = srcB[o + half];
        };
        auto store = [&](int buf) {
            double2 *d = s_m[buf] + dst;
            d[0] = rA0;
            d[kHalf] = rA1;
            d[2 * kHalf] = rB0;
            d[3 * kHalf] = rB1;
        };
        load(0);
        store(0);
        __syncthreads();
        for (int k = 0; k < nch; ++k) {
            // (unconditional: the last chunk is loaded and stored once more, into the buffer no
            // one reads again -- straight-line code keeps the prefetch in registers)
            load(min(k + 1, nch - 1));
            // walk_chunk's text in place: called from here, the compiler keeps the last two
            // groups' adds behind their maxima one by one where it otherwise gathers the maxima
            // first, and the pair phase takes 0.3 us longer (profiles/place_shared_timing.json)
            const double2 *va = s_m[k & 1] + ia * (kWalkLd / 2),
                          *vb = s_m[k & 1] + jb * (kWalkLd / 2);
            double2 a0[kWalkG], b0[kWalkG], a1[kWalkG], b1[kWalkG];
            auto rd = [&](double2 *a, double2 *b, int j) {
#pragma unroll
                for (int i = 0; i < kWalkG; ++i) {
                    a[i] = va[j + i];
                    b[i] = vb[j + i];
                }
            };
            auto add = [&](const double2 *a, const double2 *b) {
#pragma unroll
                for (int i = 0; i < kWalkG; ++i) {
                    acc += max_pos(a[i].x, b[i].x);
                    acc += max_pos(a[i].y, b[i].y);
                }
            };
            rd(a0, b0, 0);
#pragma unroll
            for (int j = 0; j < kWalkC / 2; j += 2 * kWalkG) {
                rd(a1, b1, j + kWalkG);
                __builtin_amdgcn_sched_barrier(0);
                add(a0, b0);
                __builtin_amdgcn_sched_barrier(0);
                if (j + 2 * kWalkG < kWalkC / 2) rd(a0, b0, j + 2 * kWalkG);
                __builtin_amdgcn_sched_barrier(0);
                add(a1, b1);
                __builtin_amdgcn_sched_barrier(0);
            }
            store((k + 1) & 1);
            __syncthreads();
        }
    }
    const PairSlot ps = pair_slot(ta, tb, tid, 0);
    bool ok = pair_is_pair(ps, n) && adm[ps.a] != 0u && adm[ps.b] != 0u;
    if (ok && sep2 > 0) ok = !closer_than(poses5, ps.a, ps.b, sep2);
    double bt = ok ? acc : -INFINITY;
    if (table && ps.a < n && ps.b < n) {
        table[(size_t)ps.a * n + ps.b] = bt;
        if (ta != tb) table[(size_t)ps.b * n + ps.a] = -INFINITY;   // the mirror tile
    }
    if (pair_is_single(ps, n)) singles[ps.a] = adm[ps.a] != 0u ? acc : -INFINITY;
    // the block's first maximum in row-major order
    int ba = ok ? ps.a : -1, bb = ok ? ps.b : -1;
    block_first_max<kPairLanes / 64>(s_best, bt, ba, bb);
    if (tid == 0) slots[blockIdx.x] = RowBest{bt, ba, bb};
}

// Selection, one block: the first maximum of the tile bests (ties to the lexicographically
// smaller pair: row-major order) and of the singles (ties to the lower index), the answer's size,
// the covered counts of both from M's rows, and the answer folded into cell_score / cell_owner
// (base and the owners of the fixed sensors are there from the preparation).
__global__ void __launch_bounds__(kQS)
k_pair_select(const RowBest *__restrict__ slots, int nblk, const double *__restrict__ singles,
              int P, int Cs, const double *__restrict__ M, const double *__restrict__ S, int C,
              int n_fixed, double *__restrict__ cs, int32_t *__restrict__ owner,
              PairState *__restrict__ st) {
    __shared__ RowBest s_best[kQS / 64];
    __shared__ int32_t s_pc, s_sc;
    const int tid = threadIdx.x;
    double bt = -INFINITY;
    int ba = -1, bb = -1;
    for (int i = tid; i < nblk; i += kQS) {
        const RowBest v = slots[i];
        take_ahead(bt, ba, bb, v.t, v.a, v.b);
    }
    block_first_max_all<kQS / 64>(s_best, bt, ba, bb);
    // the singles: inadmissible poses hold -inf and are never taken (strict '>' from -inf)
    double sv = -INFINITY;
    int si = -1, sz = 0;
    for (int p = tid; p < P; p += kQS) {
        const double t = singles[p];
        if (t > sv) {
            sv = t;
            si = p;
        }
    }
    block_first_max_all<kQS / 64>(s_best, sv, si, sz);
    if (tid == 0) {
        s_pc = 0;
        s_sc = 0;
    }
    __syncthreads();
    const double base_total = st->base_total;   // (the preparation's, an earlier launch)
    const int n_sel = (ba >= 0 && bt > sv) ? 2 : (si >= 0 && sv > base_total) ? 1 : 0;
    int32_t pc = 0, sc = 0;
    for (int c = tid; c < C; c += kQS) {
        if (ba >= 0)
            pc += (M[(size_t)ba * Cs + c] > 0 || M[(size_t)bb * Cs + c] > 0) ? 1 : 0;
        if (si >= 0) sc += M[(size_t)si * Cs + c] > 0 ? 1 : 0;
        if (n_sel) {
            double x = cs[c];
            int32_t own = owner[c];
            fold_owner(x, own, S[(size_t)(n_sel == 2 ? ba : si) * C + c], n_fixed);
            if (n_sel == 2) fold_owner(x, own, S[(size_t)bb * C + c], n_fixed + 1);
            cs[c] = x;
            owner[c] = own;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pc += __shfl_xor(pc, o, 64);
        sc += __shfl_xor(sc, o, 64);
    }
    if ((tid & 63) == 0) {
        if (pc) atomicAdd(&s_pc, pc);
        if (sc) atomicAdd(&s_sc, sc);
    }
    __syncthreads();
    if (tid == 0) {
        st->pair[0] = ba;
        st->pair[1] = bb;
        st->pair_total = bt;
        st->single = si;
        st->single_total = sv;
        st->pair_cov = s_pc;
        st->single_cov = s_sc;
        st->n_sel = n_sel;
    }
}

// the call's block on the device (pair_d) and, up to `down`, in the pinned landing:
// [state | cell_score f64 C | cell_owner i32 C | singles f64 P | admissible u32 Pp | tile bests |
//  pair table f64 P x P (only when asked for)]
struct PairPlan {
    int C, P, Pp, Cs, nt, nblk, ncc, npg;
    CellBlock cb;   // sg_off = cb.rest_off
    size_t sg_off, adm_off, slot_off, tab_off, bytes, m_bytes;
    bool dense;
};

PairPlan make_plan(int C, int P, bool dense) {
    PairPlan s{};
    s.C = C;
    s.P = P;
    s.nt = pair_tiles(P);
    s.Pp = s.nt * kPairTile;
    s.nblk = pair_blocks(s.nt);
    s.ncc = (C + kWalkC - 1) / kWalkC;
    s.Cs = s.ncc * kWalkC;
    s.npg = std::max(1, s.nt);
    s.dense = dense;
    s.cb = cell_block(sizeof(PairState), C);
    s.sg_off = s.cb.rest_off;
    s.adm_off = a16(s.sg_off + (size_t)P * sizeof(double));
    s.slot_off = a16(s.adm_off + (size_t)s.Pp * sizeof(uint32_t));
    s.tab_off = a16(s.slot_off + (size_t)s.nblk * sizeof(RowBest));
    s.bytes = s.tab_off + (dense ? (size_t)P * P * sizeof(double) : 0);
    s.m_bytes = (size_t)s.Cs * s.Pp * sizeof(double);
    return s;
}

// preparation, tiles, selection on ctx->stream (C > 0; the buffers are large enough)
int pair_enqueue(pcp_ctx *ctx, const PairPlan &s, const ScoreEnq &o, const PairFixed &fx,
                 double sep2) {
    hipStream_t st = ctx->stream;
    char *blk = ctx->pair_d.as<char>();
    PairState *state = reinterpret_cast<PairState *>(blk);
    double *cs = reinterpret_cast<double *>(blk + s.cb.score_off);
    int32_t *owner = reinterpret_cast<int32_t *>(blk + s.cb.owner_off);
    double *singles = reinterpret_cast<double *>(blk + s.sg_off);
    uint32_t *adm = reinterpret_cast<uint32_t *>(blk + s.adm_off);
    RowBest *slots = reinterpret_cast<RowBest *>(blk + s.slot_off);
    double *table = s.dense ? reinterpret_cast<double *>(blk + s.tab_off) : nullptr;
    double *M = ctx->pair_m.as<double>();
    hipLaunchKernelGGL(k_pair_prep, dim3((unsigned)(s.ncc * s.npg + 1)), dim3(kQT), 0, st,
                       (const double *)o.comb, (const double *)o.score_z, s.C, s.P, s.Pp, s.Cs,
                       s.ncc, s.npg, fx, o.poses_k, sep2, (const double *)o.tot_d,
                       (const int32_t *)o.cov_d, cs, owner, adm, M, state);
    PCP_CHECK_LAUNCH(ctx);
    if (s.nblk) {
        hipLaunchKernelGGL(k_pair_tiles, dim3((unsigned)s.nblk), dim3(kPairLanes), 0, st,
                           (const double *)M, s.Cs, s.P, s.nt, (const uint32_t *)adm, o.poses_k,
                           sep2, singles, slots, table);
        PCP_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(k_pair_select, dim3(1), dim3(kQS), 0, st, (const RowBest *)slots, s.nblk,
                       (const double *)singles, s.P, s.Cs, (const double *)M,
                       (const double *)o.comb, s.C, (int)fx.n, cs, owner, state);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what both entries refuse before any launch; fx = the fixed list as the kernels take it
int check_args(pcp_ctx *ctx, const char *what, uint64_t n, const pcp_pair_params *pp,
               PairFixed &fx) {
    if (pp->n_fixed < 0 || pp->n_fixed > PCP_PLACE_MAX || pp->reserved != 0)
        return set_err(ctx, PCP_E_INVALID, "%s: n_fixed %d outside 0..%d or reserved %d != 0", what,
                       (int)pp->n_fixed, PCP_PLACE_MAX, (int)pp->reserved);
    fx.n = pp->n_fixed;
    return check_pose_list(ctx, what, "fixed", "fixed", pp->fixed, pp->n_fixed, n, fx.idx);
}

}  // namespace
}  // namespace pcp
