// pcp_scan.hip -- pcp_simulate_scan on gfx950: the dense ray fan's blocked rays resolved to the
// terrain points they hit.  The production fan launch runs unchanged and leaves
// its first hits and per-wave blocked counts on the device; an exclusive scan of those counts
// gives every wave its base in the compacted returns, k_scan_resolve finds each blocked ray's
// nearest point (FLANN's float accumulator, ties to the lowest input index) in the cell-major
// copy of the terrain index, and k_scan_mask_count counts the terrain points each pose reaches.
//
// Numerics: no contraction, as everywhere -- the query point is the march's own
// float(p + d * s_k) and the range is rounded operation by operation in double.
#pragma clang fp contract(off)

#include <algorithm>
#include <cstring>

#include "pcp_internal.hpp"
#include "pcp_scan_hit.hpp"

namespace pcp {
namespace {

constexpr int kST = 256;           // threads per block: four waves of 64 rays
constexpr int kSW = kST / 64;
// the mask counts' partial sums: kSlots slots of kSlotWords uint32 (512 bytes apart: the blocks'
// atomics spread over as many cache lines) -- [0, 64) points per pose bit, [64] points with any
// bit; block b adds into slot b % kSlots, the host adds the slots up (integers: exact, any order)
constexpr int kSlots = 32, kSlotWords = 128;

static_assert(sizeof(pcp_scan_return) == 24, "pcp_scan_return is a 24-byte record");

struct ResolveArgs {
    ScanHitQuery q;                      // the hit search's tables (pcp_scan_hit.hpp)
    uint32_t rays, waves, P;
    const int16_t *first_hit;            // [P][rays], the march's
    const uint32_t *wbase;               // exclusive scan of the waves' blocked counts (mod 2^32)
    const unsigned long long *offsets;   // [P + 1]
    pcp_scan_return *returns;            // records_cap records
    unsigned long long records_cap;
    int32_t *hit_point;                  // nullable [P][rays]
    float *range_img;                    // nullable [P][rays]
    unsigned long long *mask;            // nullable [n_mask]
    unsigned long long n_mask;
};

// The resolve phase's first launch: the waves' blocked counts as one uint32 array (the context's
// scan reads uint32), the point mask cleared, and by block 0 the head -- offsets[p] = blocked[0]
// + ... + blocked[p - 1] in 64 bits (P <= 64: one thread, fixed order), the mask counts' slots
// zeroed.  head = {offsets u64[P + 1], pad, slots u32[kSlots][kSlotWords]}
__global__ void __launch_bounds__(kST)
k_scan_prepare(const uint2 *__restrict__ part, uint32_t nW, uint32_t waves, uint32_t w0,
               uint32_t lw, uint32_t *__restrict__ cnt,
               unsigned long long *__restrict__ mask, unsigned long long n_mask,
               const uint32_t *__restrict__ blocked, uint32_t P,
               unsigned long long *__restrict__ head, uint32_t *__restrict__ slots) {
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kST + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kST;
    // part holds the live waves [w0, w0 + lw) of each pose's `waves`; a culled wave has no return
    for (unsigned long long i = t0; i < nW; i += stride) {
        const uint32_t p = (uint32_t)i / waves, w = (uint32_t)i - p * waves - w0;
        cnt[i] = w < lw ? part[(size_t)p * lw + w].x : 0u;
    }
    // (the mask starts 16-byte aligned: two entries per store, then the odd last one)
    ulonglong2 *m2 = reinterpret_cast<ulonglong2 *>(mask);
    const unsigned long long n2 = n_mask >> 1;
    for (unsigned long long i = t0; i < n2; i += stride) m2[i] = make_ulonglong2(0ull, 0ull);
    if (t0 == 0 && (n_mask & 1ull)) mask[n_mask - 1] = 0ull;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < kSlots * kSlotWords; i += kST) slots[i] = 0u;
        if (threadIdx.x == 0) {
            unsigned long long run = 0;
            for (uint32_t p = 0; p < P; ++p) {
                head[p] = run;
                run += blocked[p];
            }
            head[P] = run;
        }
    }
}

// One lane per ray in the fan's wave-to-ray mapping (wave w of pose p = rays 64 w .. 64 w + 63),
// so a wave's ballot of blocked lanes counts what the march's wave counted.  A blocked lane
// finds its hit point by pcp_scan_hit.hpp's search (the march's query point of its first blocked
// sample, the eight cell runs of its stencil, the (acc, input index) minimum within r).
// MT: a mounted query -- the direction is the mounted march's own fan_dir() (pcp_fan_dir.hpp).
template <bool MT>
__global__ void __launch_bounds__(kST) k_scan_resolve(ResolveArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * kSW + (threadIdx.x >> 6);
    if (gw >= a.P * a.waves) return;   // (whole waves)
    const uint32_t p = gw / a.waves, w = gw - p * a.waves;
    const uint32_t ray = w * 64u + lane;
    const bool active = ray < a.rays;
    const size_t cell = (size_t)p * a.rays + ray;
    const int k = active ? (int)a.first_hit[cell] : -1;
    const bool hit = k >= 0;
    const uint64_t bal = __ballot(hit);
    if (!hit) {
        if (active) {
            if (a.hit_point) a.hit_point[cell] = -1;
            if (a.range_img) a.range_img[cell] = -1.0f;
        }
        return;
    }
    const uint32_t pre = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    // the wave's base: the pose's offset plus the scan's distance from the pose's first wave
    // (a difference of two prefix sums mod 2^32: exact, a pose has at most 2^30 rays)
    const unsigned long long slot =
        a.offsets[p] + (unsigned long long)(uint32_t)(a.wbase[gw] - a.wbase[p * a.waves]) + pre;
    // the hit search (pcp_scan_hit.hpp): the march's q_k, the eight runs, the (acc, index) minimum
    const ScanHit h = scan_hit<MT>(a.q, p, ray, k);
    const uint32_t bidx = h.idx;
    const float bx = h.x, by = h.y, bz = h.z;
    const double px = h.px, py = h.py, pz = h.pz;
    // (bidx stays ~0 only if the blocking set were empty, which the march excludes: the record
    // is still written, so that the segment holds no unwritten row)
    float range = -1.0f;
    if (bidx != 0xFFFFFFFFu) {
        const double ex = (double)bx - px, ey = (double)by - py, ez = (double)bz - pz;
        range = (float)sqrt((ex * ex + ey * ey) + ez * ez);
    }
    if (slot < a.records_cap) {
        pcp_scan_return rec;
        rec.x = bx;
        rec.y = by;
        rec.z = bz;
        rec.range = range;
        rec.ray = ray;
        rec.point = bidx;
        a.returns[slot] = rec;
    }
    if (a.hit_point) a.hit_point[cell] = (int32_t)bidx;
    if (a.range_img) a.range_img[cell] = range;
    // neighbouring rays mostly end on the same point (a whole wave of them near the sensor), and
    // same-address atomics are served one after the other: of a run of neighbouring lanes on one
    // point only the first sets the bit (OR is idempotent: the mask is the same)
    const uint32_t prev = (uint32_t)__shfl_up((int)bidx, 1, 64);
    const bool dup = lane > 0 && ((bal >> (lane - 1)) & 1ull) && prev == bidx;
    if (a.mask && !dup && (unsigned long long)bidx < a.n_mask) atomicOr(&a.mask[bidx], 1ull << p);
}

// The mask counts: slot[p] += points with bit p set, slot[64] += points with any bit set, in the
// block's slot.  Lane p of every wave counts bit p through ballots (two mask entries per lane and
// round, one 16-byte load); integer sums in LDS, then one global atomic per block and count.
__global__ void __launch_bounds__(kST)
k_scan_mask_count(const unsigned long long *__restrict__ mask, unsigned long long n, uint32_t P,
                  uint32_t *__restrict__ slots) {
    __shared__ uint32_t s_cnt[65];
    if (threadIdx.x < 65) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const ulonglong2 *m2 = reinterpret_cast<const ulonglong2 *>(mask);
    const unsigned long long n2 = (n + 1) >> 1;
    uint32_t acc = 0, acc_any = 0;
    for (unsigned long long b = (unsigned long long)blockIdx.x * kST; b < n2;
         b += (unsigned long long)gridDim.x * kST) {
        const unsigned long long i = b + threadIdx.x;
        ulonglong2 m = make_ulonglong2(0ull, 0ull);
        if (2 * i + 1 < n) m = m2[i];
        else if (2 * i < n) m.x = mask[2 * i];
        const uint64_t nz0 = __ballot(m.x != 0ull), nz1 = __ballot(m.y != 0ull);
        if (!(nz0 | nz1)) continue;   // (wave-uniform)
        acc_any += (uint32_t)(__popcll(nz0) + __popcll(nz1));
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t c = (uint32_t)(__popcll(__ballot(((m.x >> p) & 1ull) != 0ull)) +
                                          __popcll(__ballot(((m.y >> p) & 1ull) != 0ull)));
            if (lane == p) acc += c;
        }
    }
    if (acc) atomicAdd(&s_cnt[lane], acc);
    if (lane == 0 && acc_any) atomicAdd(&s_cnt[64], acc_any);
    __syncthreads();
    uint32_t *slot = slots + (blockIdx.x % kSlots) * kSlotWords;
    if ((threadIdx.x < P || threadIdx.x == 64) && s_cnt[threadIdx.x])
        atomicAdd(&slot[threadIdx.x], s_cnt[threadIdx.x]);
}

// the first min(total, cap) records into the pinned landing (total is known to the device only)
__global__ void __launch_bounds__(kST)
k_scan_land(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
            const unsigned long long *__restrict__ total, unsigned long long cap) {
    const unsigned long long t = *total;
    const unsigned long long words = (t < cap ? t : cap) * (sizeof(pcp_scan_return) / 8);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kST + threadIdx.x; i < words;
         i += (unsigned long long)gridDim.x * kST)
        dst[i] = src[i];
}

size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

// the call's device block: [wave counts | wave bases | scan scratch | head | hit_point | range |
// mask | records]; head = {offsets u64[P + 1], pad, the mask counts' slots}, downloaded as one span
struct ScanPlan {
    uint32_t P = 0, rays = 0, waves = 0;
    uint64_t N = 0, rec_cap = 0;
    bool dense_hp = false, dense_rg = false, mask = false;
    size_t cnt_off = 0, wbase_off = 0, tmp_off = 0, head_off = 0, slot_off = 0, head_bytes = 0, hp_off = 0,
           rg_off = 0, mask_off = 0, rec_off = 0, bytes = 0;
    // pinned: [head | mask | records]
    size_t pin_mask_off = 0, pin_rec_off = 0, pin_bytes = 0;
};

ScanPlan make_plan(uint32_t P, uint32_t rays, uint32_t waves, uint64_t N, uint64_t rec_cap,
                   bool hp, bool rg, bool mask) {
    ScanPlan s;
    s.P = P;
    s.rays = rays;
    s.waves = waves;
    s.N = N;
    s.rec_cap = std::min<uint64_t>(rec_cap, (uint64_t)P * rays);
    s.dense_hp = hp;
    s.dense_rg = rg;
    s.mask = mask && N > 0;
    const size_t nW = (size_t)P * waves, cells = (size_t)P * rays;
    s.cnt_off = 0;
    s.wbase_off = a16(s.cnt_off + nW * sizeof(uint32_t));
    s.tmp_off = a16(s.wbase_off + (nW + 1) * sizeof(uint32_t));
    s.head_off = a16(s.tmp_off + scan_tmp_bytes(nW));
    s.head_off = (s.head_off + 511) & ~(size_t)511;
    s.slot_off = ((size_t)(P + 1) * sizeof(uint64_t) + 511) & ~(size_t)511;   // within the head
    s.head_bytes = s.slot_off + (size_t)kSlots * kSlotWords * sizeof(uint32_t);
    s.hp_off = s.head_off + s.head_bytes;
    s.rg_off = a16(s.hp_off + (hp ? cells * sizeof(int32_t) : 0));
    s.mask_off = a16(s.rg_off + (rg ? cells * sizeof(float) : 0));
    s.rec_off = a16(s.mask_off + (s.mask ? (size_t)N * sizeof(uint64_t) : 0));
    s.bytes = s.rec_off + (size_t)s.rec_cap * sizeof(pcp_scan_return) + 64;
    s.pin_mask_off = s.head_bytes;
    s.pin_rec_off = a16(s.pin_mask_off + (s.mask ? (size_t)N * sizeof(uint64_t) : 0));
    s.pin_bytes = s.pin_rec_off + (size_t)s.rec_cap * sizeof(pcp_scan_return) + 64;
    return s;
}

// the resolve phase on ctx->stream, after the fan: k_scan_prepare (wave counts, mask and counts
// cleared, offsets), the wave bases' scan, k_scan_resolve, the mask counts
int resolve_enqueue(pcp_ctx *ctx, const ScanPlan &s, const pcp_fan_params *fan, const FanEnq &o) {
    hipStream_t st = ctx->stream;
    char *blk = ctx->vscan_d.as<char>();
    const uint32_t nW = s.P * s.waves;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(blk + s.cnt_off);
    uint32_t *wbase = reinterpret_cast<uint32_t *>(blk + s.wbase_off);
    unsigned long long *offsets = reinterpret_cast<unsigned long long *>(blk + s.head_off);
    uint32_t *slots = reinterpret_cast<uint32_t *>(blk + s.head_off + s.slot_off);
    unsigned long long *mask =
        s.mask ? reinterpret_cast<unsigned long long *>(blk + s.mask_off) : nullptr;
    {
        const uint64_t work = std::max<uint64_t>(nW, mask ? s.N / 2 : 0);
        const unsigned g = (unsigned)std::min<uint64_t>((work + kST - 1) / kST + 1, 2048);
        hipLaunchKernelGGL(k_scan_prepare, dim3(g), dim3(kST), 0, st, o.wave_part, nW, s.waves,
                           o.wave0, o.live_waves, cnt, mask,
                           (unsigned long long)(mask ? s.N : 0), (const uint32_t *)o.blocked_d,
                           s.P, offsets, slots);
        PCP_CHECK_LAUNCH(ctx);
    }
    if (int rc = exclusive_scan_u32(ctx, cnt, wbase, nW, blk + s.tmp_off)) return rc;
    ResolveArgs a{};
    a.q = scan_hit_query(ctx, fan);
    a.rays = s.rays;
    a.waves = s.waves;
    a.P = s.P;
    a.first_hit = o.fh_d;
    a.wbase = wbase;
    a.offsets = offsets;
    a.returns = reinterpret_cast<pcp_scan_return *>(blk + s.rec_off);
    a.records_cap = s.rec_cap;
    a.hit_point = s.dense_hp ? reinterpret_cast<int32_t *>(blk + s.hp_off) : nullptr;
    a.range_img = s.dense_rg ? reinterpret_cast<float *>(blk + s.rg_off) : nullptr;
    a.mask = mask;
    a.n_mask = s.mask ? s.N : 0;
    hipLaunchKernelGGL(o.mounted ? k_scan_resolve<true> : k_scan_resolve<false>,
                       dim3((nW + kSW - 1) / kSW), dim3(kST), 0, st, a);
    PCP_CHECK_LAUNCH(ctx);
    if (mask) {
        const unsigned g = (unsigned)std::min<uint64_t>((s.N / 2 + kST) / kST, 1024);
        hipLaunchKernelGGL(k_scan_mask_count, dim3(g), dim3(kST), 0, st,
                           (const unsigned long long *)mask, (unsigned long long)s.N, s.P, slots);
        PCP_CHECK_LAUNCH(ctx);
    }
    return PCP_OK;
}

// what pcp_raycast_fan rejects before any launch, and the pose bound of the mask's 64 bits
int check_args(pcp_ctx *ctx, const char *what, const double *poses5, uint64_t n,
               const pcp_fan_params *fan) {
    if (!fan || (n && !poses5)) return set_err(ctx, PCP_E_INVALID, "%s: null argument", what);
    if (n > PCP_SCAN_MAX_POSES)
        return set_err(ctx, PCP_E_INVALID, "%s: %llu poses, at most %d per call", what,
                       (unsigned long long)n, PCP_SCAN_MAX_POSES);
    if (fan->n_az <= 0 || fan->n_el <= 0 || (int64_t)fan->n_az * fan->n_el > (1ll << 30))
        return set_err(ctx, PCP_E_INVALID, "%s: bad fan size %d x %d", what, fan->n_az, fan->n_el);
    return PCP_OK;
}

}  // namespace
}  // namespace pcp

using namespace pcp;

// pcp_simulate_scan and, mounted (poses5: poses6 rows, el_table nullable), its mounted twin
static int simulate_scan_impl(pcp_ctx *ctx, const double *poses5, uint64_t n,
                              const pcp_fan_params *fan, bool mounted, const double *el_table,
                              pcp_scan_return *returns,
                              uint64_t returns_cap, uint64_t *n_returns, uint64_t *offsets,
                              int32_t *hit_point, float *range_img, int16_t *first_hit,
                              uint64_t *point_mask, uint64_t mask_cap, uint64_t *n_points,
                              uint32_t *seen_points, uint64_t *n_seen_any) {
    if (!ctx) return PCP_E_INVALID;
    if (!n_returns || !offsets)
        return set_err(ctx, PCP_E_INVALID, "pcp_simulate_scan: null argument");
    if (int rc = check_args(ctx, "pcp_simulate_scan", poses5, n, fan)) return rc;
    if (int rc = fan_el_table_check(ctx, "pcp_simulate_scan_mounted", fan, el_table)) return rc;
    const uint64_t N = ctx->terrain.present ? ctx->terrain_index_n : 0;
    if (!returns) returns_cap = 0;
    if (n == 0) {
        *n_returns = 0;
        offsets[0] = 0;
        if (n_points) *n_points = N;
        if (n_seen_any) *n_seen_any = 0;
        if (point_mask) {
            if (mask_cap < N)
                return set_err(ctx, PCP_E_CAPACITY, "pcp_simulate_scan: mask of %llu points, cap %llu",
                               (unsigned long long)N, (unsigned long long)mask_cap);
            std::memset(point_mask, 0, (size_t)N * sizeof(uint64_t));
        }
        return PCP_OK;
    }
    // the production fan query: first hits, per-wave partials and per-pose blocked counts stay
    // on the device (a step table past PCP_MAX_STEPS is refused in there, before any launch)
    FanEnq o;
    FanOpts fo{/*want_fh=*/true};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses5, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t P = (uint32_t)n;
    const bool want_mask = point_mask || seen_points || n_seen_any;
    const ScanPlan s = make_plan(P, o.rays, o.waves, N, returns_cap, hit_point != nullptr,
                                 range_img != nullptr, want_mask);
    PCP_HIP(ctx, ctx->vscan_d.ensure(s.bytes));
    PCP_HIP(ctx, ctx->vscan_host.ensure(s.pin_bytes));
    if (int rc = resolve_enqueue(ctx, s, fan, o)) return rc;
    // downloads: the head and the mask through the pinned landing, the records by a copy kernel
    // that knows the total, the dense images straight into the caller's arrays
    char *blk = ctx->vscan_d.as<char>();
    char *pin = ctx->vscan_host.as<char>();
    const size_t cells = (size_t)P * o.rays;
    PCP_HIP(ctx, hipMemcpyAsync(pin, blk + s.head_off, s.head_bytes, hipMemcpyDeviceToHost, st));
    if (s.mask && point_mask && mask_cap >= N)
        if (int rc = copy_to_pinned_async(ctx, pin + s.pin_mask_off, blk + s.mask_off,
                                          (size_t)N * sizeof(uint64_t), st))
            return rc;
    if (s.rec_cap) {
        const uint64_t words = s.rec_cap * (sizeof(pcp_scan_return) / 8);
        const unsigned g = (unsigned)std::min<uint64_t>((words + kST - 1) / kST, 1024);
        hipLaunchKernelGGL(k_scan_land, dim3(g), dim3(kST), 0, st,
                           reinterpret_cast<const unsigned long long *>(blk + s.rec_off),
                           reinterpret_cast<unsigned long long *>(pin + s.pin_rec_off),
                           reinterpret_cast<const unsigned long long *>(blk + s.head_off) + P,
                           (unsigned long long)s.rec_cap);
        PCP_CHECK_LAUNCH(ctx);
    }
    if (hit_point)
        PCP_HIP(ctx, hipMemcpyAsync(hit_point, blk + s.hp_off, cells * sizeof(int32_t),
                                    hipMemcpyDeviceToHost, st));
    if (range_img)
        PCP_HIP(ctx, hipMemcpyAsync(range_img, blk + s.rg_off, cells * sizeof(float),
                                    hipMemcpyDeviceToHost, st));
    if (first_hit)
        PCP_HIP(ctx, hipMemcpyAsync(first_hit, o.fh_d, cells * sizeof(int16_t),
                                    hipMemcpyDeviceToHost, st));
    PCP_HIP(ctx, hipStreamSynchronize(st));
    prof_resolve(ctx);
    const uint64_t *off_h = reinterpret_cast<const uint64_t *>(pin);
    const uint64_t total = off_h[P];
    std::memcpy(offsets, off_h, (size_t)(P + 1) * sizeof(uint64_t));
    *n_returns = total;
    if (n_points) *n_points = N;
    const uint32_t *slot_h = reinterpret_cast<const uint32_t *>(pin + s.slot_off);
    uint64_t any = 0;
    for (int q = 0; q < kSlots; ++q) any += slot_h[q * kSlotWords + 64];
    if (n_seen_any) *n_seen_any = any;
    if (seen_points)
        for (uint32_t p = 0; p < P; ++p) {
            uint32_t v = 0;
            for (int q = 0; q < kSlots; ++q) v += slot_h[q * kSlotWords + p];
            seen_points[p] = v;
        }
    const uint64_t landed = std::min<uint64_t>(total, s.rec_cap);
    if (landed)
        host_copy(ctx, returns, pin + s.pin_rec_off, (size_t)landed * sizeof(pcp_scan_return));
    int rc = PCP_OK;
    if (point_mask) {
        if (mask_cap >= N) {
            if (N) host_copy(ctx, point_mask, pin + s.pin_mask_off, (size_t)N * sizeof(uint64_t));
        } else {
            rc = set_err(ctx, PCP_E_CAPACITY, "pcp_simulate_scan: mask of %llu points, cap %llu",
                         (unsigned long long)N, (unsigned long long)mask_cap);
        }
    }
    if (returns_cap < total)
        rc = set_err(ctx, PCP_E_CAPACITY, "pcp_simulate_scan: %llu returns, cap %llu",
                     (unsigned long long)total, (unsigned long long)returns_cap);
    return rc;
}

extern "C" int pcp_simulate_scan(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                 const pcp_fan_params *fan, pcp_scan_return *returns,
                                 uint64_t returns_cap, uint64_t *n_returns, uint64_t *offsets,
                                 int32_t *hit_point, float *range_img, int16_t *first_hit,
                                 uint64_t *point_mask, uint64_t mask_cap, uint64_t *n_points,
                                 uint32_t *seen_points, uint64_t *n_seen_any) {
    return simulate_scan_impl(ctx, poses5, n, fan, false, nullptr, returns, returns_cap, n_returns,
                              offsets, hit_point, range_img, first_hit, point_mask, mask_cap,
                              n_points, seen_points, n_seen_any);
}

extern "C" int pcp_simulate_scan_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                         const pcp_fan_params *fan, const double *el_table,
                                         pcp_scan_return *returns, uint64_t returns_cap,
                                         uint64_t *n_returns, uint64_t *offsets,
                                         int32_t *hit_point, float *range_img,
                                         int16_t *first_hit, uint64_t *point_mask,
                                         uint64_t mask_cap, uint64_t *n_points,
                                         uint32_t *seen_points, uint64_t *n_seen_any) {
    return simulate_scan_impl(ctx, poses6, n, fan, true, el_table, returns, returns_cap, n_returns,
                              offsets, hit_point, range_img, first_hit, point_mask, mask_cap,
                              n_points, seen_points, n_seen_any);
}

static int simulate_scan_burst_impl(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                    const pcp_fan_params *fan, bool mounted,
                                    const double *el_table, int reps, double ms[2]) {
    if (!ctx) return PCP_E_INVALID;
    if (!ms || reps <= 0 || n == 0)
        return set_err(ctx, PCP_E_INVALID, "pcp_simulate_scan_burst: null argument or nothing to time");
    if (int rc = check_args(ctx, "pcp_simulate_scan_burst", poses5, n, fan)) return rc;
    if (int rc = fan_el_table_check(ctx, "pcp_simulate_scan_mounted_burst", fan, el_table)) return rc;
    ms[0] = ms[1] = 0.0;
    // the fan kernel `reps` times between two events (first hits and partials written by each),
    // then the resolve phase `reps` times between two events
    FanEnq o;
    FanOpts fo{/*want_fh=*/true, /*burst=*/reps, /*burst_ms=*/&ms[0]};
    fo.mounted = mounted;
    fo.el_table = el_table;
    if (int rc = fan_enqueue(ctx, poses5, n, fan, o, FanMode::Plain, fo)) return rc;
    hipStream_t st = ctx->stream;
    const uint64_t N = ctx->terrain.present ? ctx->terrain_index_n : 0;
    const ScanPlan s = make_plan((uint32_t)n, o.rays, o.waves, N, (uint64_t)n * o.rays, false,
                                 false, true);
    PCP_HIP(ctx, ctx->vscan_d.ensure(s.bytes));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PCP_HIP(ctx, hipEventCreate(&e0));
    PCP_HIP(ctx, hipEventCreate(&e1));
    int rc = resolve_enqueue(ctx, s, fan, o);   // once untimed: the phase's first touches
    hipError_t e = rc ? hipSuccess : hipEventRecord(e0, st);
    for (int r = 0; r < reps && !rc && e == hipSuccess; ++r) rc = resolve_enqueue(ctx, s, fan, o);
    if (!rc && e == hipSuccess) e = hipEventRecord(e1, st);
    if (!rc && e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.0f;
    if (!rc && e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(ctx, e, "pcp_simulate_scan_burst", __FILE__, __LINE__);
    ms[1] = (double)t / reps;
    prof_resolve(ctx);
    return PCP_OK;
}

extern "C" int pcp_simulate_scan_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                       const pcp_fan_params *fan, int reps, double ms[2]) {
    return simulate_scan_burst_impl(ctx, poses5, n, fan, false, nullptr, reps, ms);
}

extern "C" int pcp_simulate_scan_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                               const pcp_fan_params *fan, const double *el_table,
                                               int reps, double ms[2]) {
    return simulate_scan_burst_impl(ctx, poses6, n, fan, true, el_table, reps, ms);
}
