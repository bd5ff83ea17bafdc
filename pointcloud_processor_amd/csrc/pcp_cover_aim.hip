// pcp_cover_aim.hip -- pcp_place_coverage_aimed on gfx950: greedy coverage placement of sensors
// with a limited field of view, every pose searched with every aim of a table.
// An aim is a window of the pose's own fan, so the fan is marched and resolved once per pose
// whatever the aim: fan_enqueue and pcp_cover_phase.hpp's build_enqueue run unchanged and leave the
// poses' bitsets seen[p].  Behind them this file gives every (pose, seen point) a slot and a 64-bit
// aim mask -- bit a set when a ray of Window(a) resolved to the point:
//   k_caim_rank   base[p][w] = the exclusive prefix of popc(seen[p][.]) along row p; the slot of
//                 point i of pose p is p * cap + base[p][i / 64] + popc(seen[p][i / 64] below bit
//                 i % 64), cap = min(live rays per pose, N) -- a pose's seen points are at most
//                 that many, so the storage is bounded without a synchronisation and no per-pose
//                 offset has to be prefixed;
//   k_caim_zero   the used slots of every pose cleared;
//   k_caim_masks  a second resolve pass over the live waves: a blocked ray finds its point by
//                 scan_hit, as k_cover_resolve does, and ORs colmask[i] & ringmask[j] into the
//                 point's slot (OR is order-free: deterministic).
// A round (k_caim_round) is a positional population count: per word m = seen[p][w] & need[w], the
// masks of m's bits gathered and added into bit-sliced carry-save planes per lane, the planes
// reduced to one count per aim across the wave and added into round_gains[r][p][.]; the last block
// takes the first maximum over [n][n_aims].  The commit (k_caim_commit) is k_cover_commit with one
// more condition: a lane leaves need iff its point's mask has the chosen aim's bit.
// No [n][n_aims] bitset exists anywhere; all results are integers and order-free.
#pragma clang fp contract(off)

#include <vector>

#include "pcp_cover_phase.hpp"

namespace pcp {
namespace {

constexpr int kAP = 2;                          // poses per block of a round
constexpr int kASub = 4;                        // 64-word runs per wave: one word per lane and run
constexpr uint32_t kAWave = 64u * kASub;        // words of `need` a wave holds
constexpr uint32_t kABlock = kAWave * kCW;      // words per block chunk
constexpr int kAPl = 9;                         // planes: a lane adds at most 64 kASub = 2^8 masks
static_assert(64 * kASub < (1 << kAPl), "a lane's per-aim count fits the planes");

// the aims of the rounds' records (behind the base plan's CoverState)
struct AimState {
    int32_t sel_aim[PCP_PLACE_MAX];
};
static_assert(sizeof(AimState) % 16 == 0, "the tables follow on a 16-byte boundary");

struct AimFixed {
    int32_t aim[PCP_PLACE_MAX];
};

// the call's device block: pcp_cover_phase.hpp's plan, then [aim record | aim counts i64 n x A |
// gains i64 K x n x A | column masks u64 n_az | ring masks u64 n_el | ranks u32 n x W2 | masks u64
// n x cap]; the second download is [aim record .. gains) or [.. ring masks)
struct AimPlan {
    CoverPlan c;
    int A = 0, n_az = 0, n_el = 0;
    uint64_t cap = 0;
    size_t as_off = 0, ap_off = 0, rga_off = 0, tab_off = 0, base_off = 0, mask_off = 0, bytes = 0;
};

AimPlan make_aim_plan(int n, int K, uint64_t N, bool owner, bool roi, int A, int n_az, int n_el,
                      uint32_t live_waves) {
    AimPlan a;
    a.c = make_plan(n, K, N, owner, roi);
    a.A = A;
    a.n_az = n_az;
    a.n_el = n_el;
    a.cap = std::min<uint64_t>((uint64_t)live_waves * 64u, N);
    a.as_off = a16(a.c.bytes);
    a.ap_off = a16(a.as_off + sizeof(AimState));
    a.rga_off = a16(a.ap_off + (size_t)n * A * sizeof(int64_t));
    a.tab_off = a16(a.rga_off + (size_t)K * n * A * sizeof(int64_t));
    a.base_off = a16(a.tab_off + (size_t)(n_az + n_el) * sizeof(uint64_t));
    a.mask_off = a16(a.base_off + (size_t)n * a.c.W2 * sizeof(uint32_t));
    a.bytes = a.mask_off + (size_t)n * a.cap * sizeof(uint64_t) + 64;
    return a;
}

struct AimDev {
    AimState *as;
    long long *ap, *rga;
    unsigned long long *col, *ring, *mask;
    uint32_t *base;
};

AimDev aim_dev_of(char *blk, const AimPlan &a) {
    AimDev d;
    d.as = reinterpret_cast<AimState *>(blk + a.as_off);
    d.ap = reinterpret_cast<long long *>(blk + a.ap_off);
    d.rga = reinterpret_cast<long long *>(blk + a.rga_off);
    d.col = reinterpret_cast<unsigned long long *>(blk + a.tab_off);
    d.ring = d.col + a.n_az;
    d.base = reinterpret_cast<uint32_t *>(blk + a.base_off);
    d.mask = reinterpret_cast<unsigned long long *>(blk + a.mask_off);
    return d;
}

// the aim record, the aim counts and the gains cleared ([aim record .. column masks) as words)
__global__ void __launch_bounds__(kCT)
k_caim_clear(unsigned long long *__restrict__ w, unsigned long long n_w) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kCT;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kCT + threadIdx.x; i < n_w;
         i += stride)
        w[i] = 0ull;
}

// base[p][w] = popc(seen[p][0]) + .. + popc(seen[p][w - 1]): one block per pose, two words per
// thread and step, the wave's scan by shuffles and the block's through LDS
__global__ void __launch_bounds__(kCT)
k_caim_rank(const unsigned long long *__restrict__ seen, uint32_t W2, uint32_t *__restrict__ base) {
    __shared__ uint32_t s_w[kCW];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const ulonglong2 *row2 = reinterpret_cast<const ulonglong2 *>(seen + (size_t)p * W2);
    uint2 *out2 = reinterpret_cast<uint2 *>(base + (size_t)p * W2);
    uint32_t carry = 0u;
    for (uint32_t w0 = 0; w0 < W2; w0 += 2u * kCT) {   // (uniform)
        const uint32_t wi = w0 + 2u * tid;             // (W2 is even: a pair is inside or outside)
        const ulonglong2 v = wi < W2 ? row2[wi >> 1] : make_ulonglong2(0ull, 0ull);
        const uint32_t c0 = (uint32_t)__popcll(v.x), c = c0 + (uint32_t)__popcll(v.y);
        uint32_t x = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63u) s_w[wv] = x;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int k = 0; k < kCW; ++k) {
            const uint32_t t = s_w[k];
            before += (uint32_t)k < wv ? t : 0u;
            total += t;
        }
        const uint32_t excl = carry + before + x - c;
        if (wi < W2) out2[wi >> 1] = make_uint2(excl, excl + c0);
        carry += total;
        __syncthreads();
    }
}

// mask[p][0 .. seen_pts[p]) = 0: blockIdx.y = the pose (seen_pts[p] <= cap)
__global__ void __launch_bounds__(kCT)
k_caim_zero(const uint32_t *__restrict__ seen_pts, unsigned long long *__restrict__ mask,
            unsigned long long cap) {
    const uint32_t p = blockIdx.y;
    const unsigned long long cnt = min((unsigned long long)seen_pts[p], cap);
    const unsigned long long stride = (unsigned long long)gridDim.x * kCT;
    unsigned long long *m = mask + (size_t)p * cap;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kCT + threadIdx.x; i < cnt;
         i += stride)
        m[i] = 0ull;
}

// the slot of bit `bit` of a row's word v whose rank base is bw
__device__ __forceinline__ uint32_t caim_slot(uint32_t bw, unsigned long long v, uint32_t bit) {
    return bw + (uint32_t)__popcll(v & ((1ull << bit) - 1ull));
}

// k_cover_resolve's pass once more, behind the ranks: a blocked lane finds its point and ORs the
// aims holding its ray into the point's slot.  The point's bit is set in seen[p] (k_cover_resolve
// set it from the same search), so its slot lies below seen_pts[p] <= cap.  ~0, no point within r,
// has no slot: its rank is never computed.
template <bool MT>
__global__ void __launch_bounds__(kCT)
k_caim_masks(ScanHitQuery q, const int16_t *__restrict__ first_hit, uint32_t rays, uint32_t w0,
             uint32_t lw, uint32_t P, const unsigned long long *__restrict__ seen,
             const uint32_t *__restrict__ base, uint32_t W2, unsigned long long N,
             const unsigned long long *__restrict__ col, const unsigned long long *__restrict__ ring,
             unsigned long long *__restrict__ mask, unsigned long long cap) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    if (gw >= P * lw) return;   // (whole waves)
    const uint32_t p = gw / lw, w = w0 + (gw - p * lw);
    const uint32_t ray = w * 64u + lane;
    const bool active = ray < rays;
    const int k = active ? (int)first_hit[(size_t)p * rays + ray] : -1;
    if (k < 0) return;
    const ScanHit h = scan_hit<MT>(q, p, ray, k);
    const uint32_t bidx = h.idx;
    if ((unsigned long long)bidx >= N) return;
    const uint32_t j = ray / (uint32_t)q.n_az, i = ray - j * (uint32_t)q.n_az;
    const unsigned long long am = col[i] & ring[j];
    if (am == 0ull) return;   // no window holds this ray
    const size_t wi = (size_t)p * W2 + (bidx >> 6);
    const unsigned long long v = seen[wi];
    const uint32_t slot = caim_slot(base[wi], v, bidx & 63u);
    // (the bit is set and the slot inside the pose's span: anything else is a broken build phase,
    // and then nothing is written)
    if (((v >> (bidx & 63u)) & 1ull) && (unsigned long long)slot < cap)
        atomicOr(&mask[(size_t)p * cap + slot], am);
}

// One placement round over every aim.  Block = (word chunk, pose group), blockIdx.x = group *
// nchunks + chunk.  A wave holds kAWave words of need, one word per lane and run.  For each alive
// pose of the group (dead poses and all-zero need are skipped wave-uniformly) a lane walks the set
// bits of m = seen[p][w] & need[w] of its words, gathers each point's mask (a lane's slots ascend,
// the wave's lanes hold neighbouring words) and adds it into kAPl bit-sliced planes: bit a of plane
// k = bit k of the lane's count for aim a, one carry-save ripple per mask.  The planes are then
// reduced per aim across the wave by ballots, lane a keeps aim a's count, the block's waves add
// theirs up in LDS and the block adds one integer atomic per (pose, aim) into the round's [n][A]
// table.
// ALL: need is all ones, every pose counts and there is no selection: aim_points.
// Otherwise the last block to draw the round's ticket takes the first maximum over [n][A] in
// row-major order, writes the -1 rows, appends the record and updates alive, as k_cover_round.
template <bool ALL>
__global__ void __launch_bounds__(kCT)
k_caim_round(const unsigned long long *__restrict__ seen,
             const unsigned long long *__restrict__ need, const uint32_t *__restrict__ base,
             const unsigned long long *__restrict__ mask, unsigned long long cap, uint32_t W2,
             int n, int A, uint32_t *alive, long long *rg, CoverState *s, AimState *as,
             const double *__restrict__ pose, uint32_t row, double sep2, int r, uint32_t nchunks,
             int commit) {
    __shared__ RowBest s_best[kCW];
    __shared__ uint32_t s_cnt[kAP][64];   // the block's counts per (pose of the group, aim)
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = ALL ? 0 : s->done;
    if (tid < kAP * 64) s_cnt[tid >> 6][tid & 63] = 0u;
    __syncthreads();
    if (s_flag) return;   // (uniform) an earlier round stopped the search
    const uint32_t lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % nchunks, grp = blockIdx.x / nchunks;
    const uint32_t wb = chunk * kABlock + (uint32_t)(tid >> 6) * kAWave + lane;
    unsigned long long nd[kASub];
    bool some = false;
#pragma unroll
    for (int j = 0; j < kASub; ++j) {
        const uint32_t wi = wb + (uint32_t)j * 64u;
        nd[j] = wi < W2 ? (ALL ? ~0ull : need[wi]) : 0ull;
        some |= nd[j] != 0ull;
    }
    if (__ballot(some)) {   // (wave-uniform)
        for (int q = 0; q < kAP; ++q) {
            const int p = (int)grp * kAP + q;
            if (p >= n || (!ALL && alive[p] == 0u)) continue;   // (wave-uniform)
            const unsigned long long *srow = seen + (size_t)p * W2;
            const uint32_t *brow = base + (size_t)p * W2;
            const unsigned long long *mrow = mask + (size_t)p * cap;
            unsigned long long pl[kAPl];
#pragma unroll
            for (int k = 0; k < kAPl; ++k) pl[k] = 0ull;
            auto add = [&](unsigned long long c) {
#pragma unroll
                for (int k = 0; k < kAPl; ++k) {
                    const unsigned long long t = pl[k] & c;
                    pl[k] ^= c;
                    c = t;
                }
            };
            // the lane's kASub words of the row at once, then one gather per word and step: kASub
            // loads in flight before any is added (the walk is bound by the gathers' latency)
            unsigned long long v[kASub], m[kASub];
            uint32_t bw[kASub];
            bool left = false;
#pragma unroll
            for (int j = 0; j < kASub; ++j) {
                const uint32_t wi = wb + (uint32_t)j * 64u;
                v[j] = nd[j] != 0ull ? srow[wi] : 0ull;   // (nd != 0: wi < W2)
                m[j] = v[j] & nd[j];
                bw[j] = m[j] ? brow[wi] : 0u;
                left |= m[j] != 0ull;
            }
            while (__ballot(left)) {   // (wave-uniform)
                unsigned long long c[kASub];
                left = false;
#pragma unroll
                for (int j = 0; j < kASub; ++j) {
                    c[j] = 0ull;
                    if (m[j]) {
                        const uint32_t u = (uint32_t)__builtin_ctzll(m[j]);
                        m[j] &= m[j] - 1ull;
                        c[j] = mrow[caim_slot(bw[j], v[j], u)];
                        left |= m[j] != 0ull;
                    }
                }
#pragma unroll
                for (int j = 0; j < kASub; ++j) add(c[j]);
            }
            // the planes across the wave: aim a's count = sum over k of 2^k * #{lanes with bit a
            // of plane k}; planes no lane reached are skipped
            uint32_t live = 0u;
#pragma unroll
            for (int k = 0; k < kAPl; ++k)
                if (__ballot(pl[k] != 0ull)) live |= 1u << k;   // (wave-uniform)
            if (live) {
                uint32_t cnt = 0u;
                for (int a = 0; a < A; ++a) {   // (uniform)
                    uint32_t tot = 0u;
#pragma unroll
                    for (int k = 0; k < kAPl; ++k)
                        if (live & (1u << k))
                            tot += (uint32_t)__popcll(__ballot((pl[k] >> a) & 1ull)) << k;
                    if (lane == (uint32_t)a) cnt = tot;
                }
                if (cnt) atomicAdd(&s_cnt[q][lane], cnt);   // (LDS: a lane per address)
            }
        }
    }
    // the block's four waves as one: an integer atomic per (pose, aim) the block counted
    __syncthreads();
    if (tid < kAP * 64) {
        const int p = (int)grp * kAP + (tid >> 6);
        const uint32_t cnt = s_cnt[tid >> 6][tid & 63];
        if (cnt)   // (then p < n and lane < A: the masks hold no bit from A on)
            atomicAdd(reinterpret_cast<unsigned long long *>(&rg[(size_t)p * A + (tid & 63)]),
                      (unsigned long long)cnt);
    }
    if (ALL) return;
    // the round's ticket: this block's sums added before the draw
    if (!last_block(&s->ticket, s_flag)) return;

    // ---- the last block of the round ------------------------------------------------------
    // (a gain is at most 2^32: exact as a double, so the shared first-maximum reduction serves;
    // a thread's entries ascend in row-major order, so strict '>' keeps its first maximum)
    double tb = -1.0;
    int b = -1, ab = 0;
    const int rows = n * A;
    for (int e0 = tid; e0 < rows; e0 += 4 * kCT) {   // (four loads in flight per step)
        long long t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * kCT;
            t4[u] = e < rows ? __hip_atomic_load(&rg[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                             : 0ll;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * kCT;
            if (e >= rows) continue;
            const int p = e / A;
            if (alive[p] == 0u) {
                if (commit) rg[e] = -1ll;
                continue;
            }
            const double t = (double)t4[u];
            if (t > tb) {
                tb = t;
                b = p;
                ab = e - p * A;
            }
        }
    }
    block_first_max_all<kCW>(s_best, tb, b, ab);
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
        as->sel_aim[r] = ab;
        s->gain[r] = g;
        s->cov_after[r] = (r == 0 ? s->base_covered : s->cov_after[r - 1]) + g;
        s->n_sel = r + 1;
    }
    // the placed pose with all its aims and, with a separation, every pose closer than it in XY
    // leave the search
    for (int p = tid; p < n; p += kCT)
        if (p == b || (sep2 > 0 && cover_closer(pose, row, p, b, sep2))) alive[p] = 0u;
}

// The commit of one aimed sensor: the points of seen(b, ab) still in need get the owner and leave
// need.  One wave per word (its only writer, and of its 64 owners), lane i = bit i; a lane leaves
// iff its point's mask has bit ab.  b_fixed >= 0: a fixed sensor with aim a_fixed, its points
// counted into base_covered; otherwise round r's record, and a return at once when that round
// recorded nothing.
__global__ void __launch_bounds__(kCT)
k_caim_commit(const unsigned long long *__restrict__ seen, unsigned long long *need,
              const uint32_t *__restrict__ base, const unsigned long long *__restrict__ mask,
              unsigned long long cap, uint32_t W2, int32_t *__restrict__ owner, CoverState *s,
              const AimState *as, int b_fixed, int a_fixed, int32_t owner_id, int r) {
    __shared__ uint32_t s_cnt;
    const int b = b_fixed >= 0 ? b_fixed : (s->n_sel > r ? (int)s->sel[r] : -1);
    if (b < 0) return;   // (uniform)
    const int ab = b_fixed >= 0 ? a_fixed : as->sel_aim[r];
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kCW + (threadIdx.x >> 6);
    if (gw < W2) {
        const unsigned long long nd = need[gw];
        const unsigned long long v = seen[(size_t)b * W2 + gw];
        const unsigned long long m = v & nd;
        if (m) {   // (wave-uniform)
            bool take = false;
            if ((m >> lane) & 1ull) {
                const uint32_t slot = caim_slot(base[(size_t)b * W2 + gw], v, lane);
                take = (mask[(size_t)b * cap + slot] >> ab) & 1ull;
            }
            const unsigned long long t = __ballot(take);
            if (t) {   // (wave-uniform)
                if (owner && take) owner[(size_t)gw * 64u + lane] = owner_id;
                if (lane == 0) {
                    need[gw] = nd & ~t;
                    if (b_fixed >= 0) atomicAdd(&s_cnt, (uint32_t)__popcll(t));
                }
            }
        }
    }
    if (b_fixed < 0) return;
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&s->base_covered, (unsigned long long)s_cnt);
}

// the ranks and the masks on ctx->stream, behind build_enqueue
int masks_enqueue(pcp_ctx *ctx, const AimPlan &a, const CoverDev &d, const AimDev &ad,
                  const pcp_fan_params *fan, const FanEnq &o) {
    hipStream_t st = ctx->stream;
    const CoverPlan &c = a.c;
    {
        const unsigned long long n_w = (a.tab_off - a.as_off) / sizeof(unsigned long long);
        const unsigned g = (unsigned)std::min<uint64_t>((n_w + kCT - 1) / kCT, 4096);
        hipLaunchKernelGGL(k_caim_clear, dim3(g), dim3(kCT), 0, st,
                           reinterpret_cast<unsigned long long *>(ad.as), n_w);
        PCP_CHECK_LAUNCH(ctx);
    }
    const uint32_t nW = (uint32_t)c.n * o.live_waves;
    if (!nW || !a.cap) return PCP_OK;   // no blocked ray: every bitset is empty
    hipLaunchKernelGGL(k_caim_rank, dim3((unsigned)c.n), dim3(kCT), 0, st,
                       (const unsigned long long *)d.seen, c.W2, ad.base);
    PCP_CHECK_LAUNCH(ctx);
    {
        const unsigned g = (unsigned)std::min<uint64_t>((a.cap + 4 * kCT - 1) / (4 * kCT), 256);
        hipLaunchKernelGGL(k_caim_zero, dim3(g, (unsigned)c.n), dim3(kCT), 0, st,
                           (const uint32_t *)d.seen_pts, ad.mask, (unsigned long long)a.cap);
        PCP_CHECK_LAUNCH(ctx);
    }
    const ScanHitQuery q = scan_hit_query(ctx, fan);
    hipLaunchKernelGGL(o.mounted ? k_caim_masks<true> : k_caim_masks<false>,
                       dim3((nW + kCW - 1) / kCW), dim3(kCT), 0, st, q, (const int16_t *)o.fh_d,
                       o.rays, o.wave0, o.live_waves, (uint32_t)c.n,
                       (const unsigned long long *)d.seen, (const uint32_t *)ad.base, c.W2,
                       (unsigned long long)c.N, (const unsigned long long *)ad.col,
                       (const unsigned long long *)ad.ring, ad.mask, (unsigned long long)a.cap);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

template <bool ALL>
int aim_round_enqueue(pcp_ctx *ctx, const AimPlan &a, const CoverDev &d, const AimDev &ad,
                      const FanEnq &o, double sep2, int r, bool commit) {
    const CoverPlan &c = a.c;
    const uint32_t nchunks = (c.W2 + kABlock - 1) / kABlock;
    const uint32_t groups = ((uint32_t)c.n + kAP - 1) / kAP;
    long long *rg = ALL ? ad.ap : ad.rga + (size_t)r * c.n * a.A;
    hipLaunchKernelGGL(k_caim_round<ALL>, dim3(nchunks * groups), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, (const unsigned long long *)d.need,
                       (const uint32_t *)ad.base, (const unsigned long long *)ad.mask,
                       (unsigned long long)a.cap, c.W2, c.n, a.A, d.alive, rg, d.s, ad.as,
                       ctx->poses_d.as<const double>(), o.pose_row, sep2, r, nchunks,
                       commit ? 1 : 0);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

int aim_commit_enqueue(pcp_ctx *ctx, const AimPlan &a, const CoverDev &d, const AimDev &ad,
                       int b_fixed, int a_fixed, int owner_id, int r) {
    const CoverPlan &c = a.c;
    hipLaunchKernelGGL(k_caim_commit, dim3((c.W2 + kCW - 1) / kCW), dim3(kCT), 0, ctx->stream,
                       (const unsigned long long *)d.seen, d.need, (const uint32_t *)ad.base,
                       (const unsigned long long *)ad.mask, (unsigned long long)a.cap, c.W2,
                       d.owner, d.s, (const AimState *)ad.as, b_fixed, a_fixed,
                       (int32_t)owner_id, r);
    PCP_CHECK_LAUNCH(ctx);
    return PCP_OK;
}

// what is refused before any launch beyond check_args (ctx non-null); cp: the coverage call's
// struct of the same search, tab: the column masks [n_az] and behind them the ring masks [n_el]
int check_aim_args(pcp_ctx *ctx, const char *what, const double *poses, uint64_t n,
                   const pcp_fan_params *fan, bool mounted, const double *el_table,
                   const pcp_cover_aim_params *ap, const int32_t *aims, const uint8_t *roi,
                   uint64_t roi_n, pcp_cover_params &cp, CoverFixed &fx, AimFixed &fa,
                   std::vector<unsigned long long> &tab, uint64_t *N_out) {
    if (!fan || !ap || !aims || (n && !poses))
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    cp = pcp_cover_params{};
    cp.k_max = ap->k_max;
    cp.n_fixed = ap->n_fixed;
    cp.reserved[0] = ap->reserved[0];
    cp.reserved[1] = ap->reserved[1] | ap->reserved[2];
    cp.min_separation = ap->min_separation;
    for (int i = 0; i < PCP_PLACE_MAX; ++i) cp.fixed[i] = ap->fixed_pose[i];
    if (int rc = check_args(ctx, what, poses, n, fan, mounted, el_table, &cp, roi, roi_n, fx, N_out))
        return rc;
    if (ap->n_aims < 1 || ap->n_aims > PCP_COVER_AIM_MAX)
        return set_err(ctx, PCP_E_INVALID, "%s: n_aims %d outside 1..%d", what, (int)ap->n_aims,
                       PCP_COVER_AIM_MAX);
    if (n * (uint64_t)ap->n_aims > PCP_AIM_MAX_ROWS)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses x %d aims, at most %d rows", what,
                       (unsigned long long)n, (int)ap->n_aims, PCP_AIM_MAX_ROWS);
    if (ap->w_az < 1 || ap->w_az > fan->n_az || ap->w_el < 1 || ap->w_el > fan->n_el)
        return set_err(ctx, PCP_E_INVALID, "%s: window %d x %d outside 1..%d x 1..%d", what,
                       (int)ap->w_az, (int)ap->w_el, fan->n_az, fan->n_el);
    for (int a = 0; a < ap->n_aims; ++a)
        if (aims[2 * a] < 0 || aims[2 * a] >= fan->n_az || aims[2 * a + 1] < 0 ||
            aims[2 * a + 1] > fan->n_el - ap->w_el)
            return set_err(ctx, PCP_E_INVALID, "%s: aims[%d] = (%d, %d) outside 0..%d x 0..%d",
                           what, a, (int)aims[2 * a], (int)aims[2 * a + 1], fan->n_az - 1,
                           fan->n_el - ap->w_el);
    for (int i = 0; i < PCP_PLACE_MAX; ++i) fa.aim[i] = 0;
    for (int i = 0; i < ap->n_fixed; ++i) {
        if (ap->fixed_aim[i] < 0 || ap->fixed_aim[i] >= ap->n_aims)
            return set_err(ctx, PCP_E_INVALID, "%s: fixed_aim[%d] = %d is no aim of %d", what, i,
                           (int)ap->fixed_aim[i], (int)ap->n_aims);
        fa.aim[i] = ap->fixed_aim[i];
    }
    // the aims holding each column and each ring
    tab.assign((size_t)fan->n_az + fan->n_el, 0ull);
    for (int a = 0; a < ap->n_aims; ++a) {
        for (int k = 0; k < ap->w_az; ++k)
            tab[(size_t)((aims[2 * a] + k) % fan->n_az)] |= 1ull << a;
        for (int k = 0; k < ap->w_el; ++k)
            tab[(size_t)fan->n_az + aims[2 * a + 1] + k] |= 1ull << a;
    }
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

// pcp_place_coverage_aimed and, mounted (poses: poses6 rows, el_table nullable), its mounted twin
static int place_coverage_aimed_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                     const pcp_fan_params *fan, bool mounted,
                                     const double *el_table, const pcp_cover_aim_params *ap,
                                     const int32_t *aims, const uint8_t *roi, uint64_t roi_n,
                                     int64_t *selected, int32_t *selected_aim, uint64_t *gain,
                                     uint64_t *covered_after, int64_t *round_gains,
                                     uint32_t *seen_points, uint32_t *aim_points,
                                     int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                                     uint64_t *roi_points, uint64_t *base_covered,
                                     int32_t *n_selected) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_aimed_mounted" : "pcp_place_coverage_aimed";
    if (!selected || !selected_aim || !gain || !covered_after || !n_points || !roi_points ||
        !base_covered || !n_selected)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    pcp_cover_params cp;
    CoverFixed fx{};
    AimFixed fa{};
    std::vector<unsigned long long> tab;
    uint64_t N = 0;
    if (int rc = check_aim_args(ctx, what, poses, n, fan, mounted, el_table, ap, aims, roi, roi_n,
                                cp, fx, fa, tab, &N))
        return rc;
    if (point_owner && owner_cap < N) {
        *n_points = N;
        return set_err(ctx, PCP_E_CAPACITY, "%s: owners of %llu points, cap %llu", what,
                       (unsigned long long)N, (unsigned long long)owner_cap);
    }
    const int A = ap->n_aims;
    *n_points = N;
    *n_selected = 0;
    *base_covered = 0;
    if (n == 0 || N == 0) {   // nothing to place or nothing to cover
        uint64_t R = roi ? 0 : N;
        for (uint64_t i = 0; roi && i < N; ++i) R += roi[i] != 0;
        *roi_points = R;
        for (uint64_t i = 0; point_owner && i < N; ++i) point_owner[i] = PCP_OWNER_NONE;
        for (uint64_t p = 0; seen_points && p < n; ++p) seen_points[p] = 0u;
        for (uint64_t e = 0; aim_points && e < n * (uint64_t)A; ++e) aim_points[e] = 0u;
        return PCP_OK;
    }
    // the production fan query: first hits and the live waves stay on the device
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const int K = cp.k_max;
    const AimPlan a = make_aim_plan((int)n, K, N, point_owner != nullptr, roi != nullptr, A,
                                    fan->n_az, fan->n_el, o.live_waves);
    const CoverPlan &c = a.c;
    // the downloads: [state | counts], [aim record | aim counts | gains], the owners
    const size_t down0 = c.rg_off;
    const size_t down1 = (round_gains ? a.tab_off : a.rga_off) - a.as_off;
    const size_t pin1 = a16(down0), pin_own = a16(pin1 + down1);
    PCP_HIP(ctx, ctx->caim_d.ensure(a.bytes));
    PCP_HIP(ctx, ctx->caim_host.ensure(pin_own + (c.owner ? (size_t)N * sizeof(int32_t) : 0) + 64));
    char *blk = ctx->caim_d.as<char>();
    const CoverDev d = dev_of(blk, c);
    const AimDev ad = aim_dev_of(blk, a);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    if (int rc = upload_async(ctx, ad.col, tab.data(), tab.size() * sizeof(unsigned long long), st))
        return rc;
    const double sep2 = sep2_of(cp.min_separation);
    if (int rc = build_enqueue(ctx, c, d, fan, o, fx, sep2)) return rc;
    if (int rc = masks_enqueue(ctx, a, d, ad, fan, o)) return rc;
    if (aim_points)
        if (int rc = aim_round_enqueue<true>(ctx, a, d, ad, o, sep2, 0, false)) return rc;
    // the fixed sensors, in list order, by the rounds' own commit
    for (int i = 0; i < fx.n; ++i)
        if (int rc = aim_commit_enqueue(ctx, a, d, ad, fx.idx[i], fa.aim[i], i, 0)) return rc;
    for (int r = 0; r < K; ++r) {
        ProfScope ps(ctx, PCP_K_PLACE);
        if (int rc = aim_round_enqueue<false>(ctx, a, d, ad, o, sep2, r, true)) return rc;
        if (int rc = aim_commit_enqueue(ctx, a, d, ad, -1, 0, fx.n + r, r)) return rc;
    }
    char *pin = ctx->caim_host.as<char>();
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk, down0, hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipMemcpyAsync(pin + pin1, blk + a.as_off, down1, hipMemcpyDeviceToHost, st));
    if (c.owner)
        if (int rc = copy_to_pinned_async(ctx, pin + pin_own, blk + c.own_off,
                                          (size_t)N * sizeof(int32_t), st))
            return rc;
    if (int rc = stream_done(ctx)) return rc;
    const CoverState *h = reinterpret_cast<const CoverState *>(pin);
    const AimState *ha = reinterpret_cast<const AimState *>(pin + pin1);
    const int ns = h->n_sel;
    for (int r = 0; r < ns; ++r) {
        selected[r] = h->sel[r];
        selected_aim[r] = ha->sel_aim[r];
        gain[r] = h->gain[r];
        covered_after[r] = h->cov_after[r];
    }
    if (round_gains && ns)
        std::memcpy(round_gains, pin + pin1 + (a.rga_off - a.as_off),
                    (size_t)ns * n * A * sizeof(int64_t));
    if (seen_points) std::memcpy(seen_points, pin + c.sp_off, (size_t)n * sizeof(uint32_t));
    if (aim_points) {
        const int64_t *src = reinterpret_cast<const int64_t *>(pin + pin1 + (a.ap_off - a.as_off));
        for (uint64_t e = 0; e < n * (uint64_t)A; ++e) aim_points[e] = (uint32_t)src[e];
    }
    if (point_owner) host_copy(ctx, point_owner, pin + pin_own, (size_t)N * sizeof(int32_t));
    *roi_points = h->roi_points;
    *base_covered = h->base_covered;
    *n_selected = ns;
    return PCP_OK;
}

extern "C" int pcp_place_coverage_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                        const pcp_fan_params *fan, const pcp_cover_aim_params *ap,
                                        const int32_t *aims, const uint8_t *roi, uint64_t roi_n,
                                        int64_t *selected, int32_t *selected_aim, uint64_t *gain,
                                        uint64_t *covered_after, int64_t *round_gains,
                                        uint32_t *seen_points, uint32_t *aim_points,
                                        int32_t *point_owner, uint64_t owner_cap,
                                        uint64_t *n_points, uint64_t *roi_points,
                                        uint64_t *base_covered, int32_t *n_selected) {
    return place_coverage_aimed_impl(ctx, poses5, n, fan, false, nullptr, ap, aims, roi, roi_n,
                                     selected, selected_aim, gain, covered_after, round_gains,
                                     seen_points, aim_points, point_owner, owner_cap, n_points,
                                     roi_points, base_covered, n_selected);
}

extern "C" int pcp_place_coverage_aimed_mounted(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_cover_aim_params *ap, const int32_t *aims,
    const uint8_t *roi, uint64_t roi_n, int64_t *selected, int32_t *selected_aim, uint64_t *gain,
    uint64_t *covered_after, int64_t *round_gains, uint32_t *seen_points, uint32_t *aim_points,
    int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
    uint64_t *base_covered, int32_t *n_selected) {
    return place_coverage_aimed_impl(ctx, poses6, n, fan, true, el_table, ap, aims, roi, roi_n,
                                     selected, selected_aim, gain, covered_after, round_gains,
                                     seen_points, aim_points, point_owner, owner_cap, n_points,
                                     roi_points, base_covered, n_selected);
}

static int place_coverage_aimed_burst_impl(pcp_ctx *ctx, const double *poses, uint64_t n,
                                           const pcp_fan_params *fan, bool mounted,
                                           const double *el_table, const pcp_cover_aim_params *ap,
                                           const int32_t *aims, const uint8_t *roi,
                                           uint64_t roi_n, int reps, double ms[3]) {
    if (!ctx) return PCP_E_INVALID;
    const char *what = mounted ? "pcp_place_coverage_aimed_mounted_burst"
                               : "pcp_place_coverage_aimed_burst";
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "%s: null argument or nothing to time", what);
    pcp_cover_params cp;
    CoverFixed fx{};
    AimFixed fa{};
    std::vector<unsigned long long> tab;
    uint64_t N = 0;
    if (int rc = check_aim_args(ctx, what, poses, n, fan, mounted, el_table, ap, aims, roi, roi_n,
                                cp, fx, fa, tab, &N))
        return rc;
    if (N == 0) return set_err(ctx, PCP_E_INVALID, "%s: no terrain index, nothing to time", what);
    ms[0] = ms[1] = ms[2] = 0.0;
    FanEnq o;
    FanOpts fo{/*want_fh=*/true, /*burst=*/reps, /*burst_ms=*/&ms[0]};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const AimPlan a = make_aim_plan((int)n, cp.k_max, N, false, roi != nullptr, ap->n_aims,
                                    fan->n_az, fan->n_el, o.live_waves);
    PCP_HIP(ctx, ctx->caim_d.ensure(a.bytes));
    char *blk = ctx->caim_d.as<char>();
    const CoverDev d = dev_of(blk, a.c);
    const AimDev ad = aim_dev_of(blk, a);
    if (roi)
        if (int rc = upload_async(ctx, d.roi, roi, (size_t)N, st)) return rc;
    if (int rc = upload_async(ctx, ad.col, tab.data(), tab.size() * sizeof(unsigned long long), st))
        return rc;
    const double sep2 = sep2_of(cp.min_separation);
    auto build = [&] {
        if (int rc = build_enqueue(ctx, a.c, d, fan, o, fx, sep2)) return rc;
        return masks_enqueue(ctx, a, d, ad, fan, o);
    };
    if (int rc = time_reps(ctx, what, st, reps, build, build, &ms[1])) return rc;
    for (int i = 0; i < fx.n; ++i)
        if (int rc = aim_commit_enqueue(ctx, a, d, ad, fx.idx[i], fa.aim[i], i, 0)) return rc;
    // round 0's launch with the selection, nothing committed (the table's sums add up over the
    // repetitions: the selection is the same)
    auto round0 = [&] { return aim_round_enqueue<false>(ctx, a, d, ad, o, sep2, 0, false); };
    return time_reps(ctx, what, st, reps, round0, round0, &ms[2]);
}

extern "C" int pcp_place_coverage_aimed_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                              const pcp_fan_params *fan,
                                              const pcp_cover_aim_params *ap, const int32_t *aims,
                                              const uint8_t *roi, uint64_t roi_n, int reps,
                                              double ms[3]) {
    return place_coverage_aimed_burst_impl(ctx, poses5, n, fan, false, nullptr, ap, aims, roi,
                                           roi_n, reps, ms);
}

extern "C" int pcp_place_coverage_aimed_mounted_burst(
    pcp_ctx *ctx, const double *poses6, uint64_t n, const pcp_fan_params *fan,
    const double *el_table, const pcp_cover_aim_params *ap, const int32_t *aims,
    const uint8_t *roi, uint64_t roi_n, int reps, double ms[3]) {
    return place_coverage_aimed_burst_impl(ctx, poses6, n, fan, true, el_table, ap, aims, roi,
                                           roi_n, reps, ms);
}
