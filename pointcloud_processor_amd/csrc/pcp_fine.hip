// pcp_fine.hip -- the fine-window copy of the terrain index, the layout the
// ray march walks once a terrain is queried repeatedly.
//
// The xy plane is cut into fine cells of c_f = c / F (F = PCP_TERRAIN_FINE, default 2: 0.06 m
// for the ray radius).  The WINDOW of fine cell W holds every point whose xy distance to W's
// rectangle is at most R = r + m: a rounded square that contains the radius-r disk around any
// query whose xy lies in W (or within float rounding of it) -- 0.027 m^2 at F = 2 against the
// 0.058 m^2 of the 2x2x2 block's square (F = 3: 0.021 m^2, fewer point tests but 2.25x the
// records for the probes to gather: measured slower).  Each window's points are
// one run in descending z (ties by original index, as k_cell_rank_z), ended by a sentinel
// (x, y NaN: never within r; z -inf: always r below).  One 8-byte record per (fine cell x, y,
// coarse z corner iz), in 4 x 4 xy tiles of one 128-byte line (PCP_FINE_TILE; 0: x-fastest):
// {first point of the window in coarse z cells <= iz + 1, probe thresholds}; the walk stops at
// the first point r below q, at the latest the first point below cell iz, or at the sentinel.
//
// Build (all on the device, O(pairs log)): global z order of the points (radix sort of
// (descending z, index) keys) -> per point, the windows that hold it, emitted in z order ->
// stable radix sort of the (window, z rank) pairs by window -> runs + sentinels -> records.
#pragma clang fp contract(off)

#include <cfloat>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

#include "pcp_fan_band.hpp"
#include "pcp_fan_clear.hpp"
#include "pcp_fan_pivot.hpp"
#include "pcp_grid.hpp"
#include "pcp_internal.hpp"
#include "pcp_walk_pair.hpp"

namespace pcp {

namespace {

constexpr int kThreads = 256;

struct FineGeo {
    double ox, oy;        // grid origin (x, y)
    double cf, inv_cf;    // fine cell edge and its inverse
    double R2;            // (r + m)^2
    int32_t fnx, fny;     // fine cells per axis (= windows per axis)
    int32_t reach;        // ceil(R / c_f): windows within this many cells can hold a point
};

// p's xy distance to window (wx, wy)'s rectangle is <= R (double arithmetic, the same in every
// kernel, so counts and emissions agree)
__device__ __forceinline__ bool in_window(const FineGeo &f, double px, double py, int wx, int wy) {
    const double x0 = f.ox + (double)wx * f.cf, y0 = f.oy + (double)wy * f.cf;
    const double dx = fmax(fmax(x0 - px, px - (x0 + f.cf)), 0.0);
    const double dy = fmax(fmax(y0 - py, py - (y0 + f.cf)), 0.0);
    return dx * dx + dy * dy <= f.R2;
}

__device__ __forceinline__ void fine_cell(const FineGeo &f, float x, float y, int &cx, int &cy) {
    cx = min(max((int)floor(((double)x - f.ox) * f.inv_cf), 0), f.fnx - 1);
    cy = min(max((int)floor(((double)y - f.oy) * f.inv_cf), 0), f.fny - 1);
}

// (descending z, ascending original index) as one ascending 64-bit key
__global__ void __launch_bounds__(kThreads)
k_zkeys(const float4 *__restrict__ pts, uint32_t n, unsigned long long *__restrict__ key,
        uint32_t *__restrict__ val) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    uint32_t u = __float_as_uint(p.z);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending in z
    key[i] = ((unsigned long long)(~u) << 32) | __float_as_uint(p.w);
    val[i] = i;
}

// windows holding each point (in z order): count per point
__global__ void __launch_bounds__(kThreads)
k_win_count(const float4 *__restrict__ pts, const uint32_t *__restrict__ zord, uint32_t n,
            FineGeo f, uint32_t *__restrict__ pcount) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[zord[i]];
    int cx, cy;
    fine_cell(f, p.x, p.y, cx, cy);
    uint32_t c = 0;
    for (int wy = max(cy - f.reach, 0); wy <= min(cy + f.reach, f.fny - 1); ++wy)
        for (int wx = max(cx - f.reach, 0); wx <= min(cx + f.reach, f.fnx - 1); ++wx)
            if (in_window(f, (double)p.x, (double)p.y, wx, wy)) ++c;
    pcount[i] = c;
}

__global__ void __launch_bounds__(kThreads)
k_win_emit(const float4 *__restrict__ pts, const uint32_t *__restrict__ zord, uint32_t n,
           FineGeo f, const uint32_t *__restrict__ poff, uint32_t *__restrict__ wkey,
           uint32_t *__restrict__ rank) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[zord[i]];
    int cx, cy;
    fine_cell(f, p.x, p.y, cx, cy);
    uint32_t o = poff[i];
    for (int wy = max(cy - f.reach, 0); wy <= min(cy + f.reach, f.fny - 1); ++wy)
        for (int wx = max(cx - f.reach, 0); wx <= min(cx + f.reach, f.fnx - 1); ++wx)
            if (in_window(f, (double)p.x, (double)p.y, wx, wy)) {
                wkey[o] = (uint32_t)wx + (uint32_t)f.fnx * (uint32_t)wy;
                rank[o] = i;
                ++o;
            }
}

// cstart[w] = first sorted pair of window w (lower bound in the sorted window keys), w <= nw
__global__ void __launch_bounds__(kThreads)
k_win_bounds(const uint32_t *__restrict__ wkey, uint32_t np, uint32_t nw,
             uint32_t *__restrict__ cstart) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    if (w > nw) return;
    uint32_t lo = 0, hi = np;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (wkey[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    cstart[w] = lo;
}

// sorted pair k of window W lands at k + W (one sentinel ends each earlier window)
__global__ void __launch_bounds__(kThreads)
k_win_place(const float4 *__restrict__ pts, const uint32_t *__restrict__ zord,
            const uint32_t *__restrict__ wkey, const uint32_t *__restrict__ rank, uint32_t np,
            float4 *__restrict__ wpts) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= np) return;
    wpts[k + wkey[k]] = pts[zord[rank[k]]];
}

// records of one window, one thread per window: for coarse z corner iz, the window's points in
// coarse z cells iz, iz + 1 start at the first point with cz <= iz + 1 of the z-descending run
// (cz is non-increasing along it); no end is stored (see the header).  The z band is stored as
// probe thresholds in steps of kZq cells above the block floor: lo - T, hi + T with
// T = ceil((r + 2 mm) / c / kZq) folded in (0 / 255 unbounded; empty: lo 255, hi 0), so the
// probe is two compares.  (One thread per record with two binary searches each
// measured 1.7x slower: 17 levels re-search the same short run.)
__global__ void __launch_bounds__(kThreads)
k_frec(float4 *__restrict__ wpts, const uint32_t *__restrict__ cstart, CellMap m, double c,
       uint32_t fnx, uint32_t fny, uint32_t rz, uint32_t tsteps, int tile,
       int skip2, uint2 *__restrict__ frec, uint16_t *__restrict__ fband,
       uint32_t *__restrict__ fstart) {
    const uint32_t nw = fnx * fny, w = blockIdx.x * kThreads + threadIdx.x;
    // tiles of T x T records: 4 x 4 8-byte records (tile 1) or 8 x 8 split records (tile 2),
    // 128 bytes of probe data each
    const uint32_t sh = tile == 2 ? 3u : 2u, T = 1u << sh, TS = T * T;
    const uint32_t tx = (fnx + T - 1) >> sh, ty = (fny + T - 1) >> sh;
    const size_t plane = tile ? (size_t)tx * ty * TS : (size_t)nw;
    auto put = [&](size_t r, uint32_t start, uint32_t band) {
        if (tile == 2) {
            fband[r] = (uint16_t)band;
            fstart[r] = start;
        } else {
            frec[r] = make_uint2(start, band);
        }
    };
    if (tile && w < tx * ty * TS) {   // padding records of the tiles (never windows)
        const uint32_t t = w >> (2 * sh), sub = w & (TS - 1);
        const uint32_t px = (t % tx) * T + (sub & (T - 1)), py = (t / tx) * T + (sub >> sh);
        if (px >= fnx || py >= fny)
            for (uint32_t iz = 0; iz < rz; ++iz) put((size_t)iz * plane + w, 0u, 0x00FFu);
    }
    if (w >= nw) return;
    // record index of (w, iz): x-fastest, or T x T xy tiles
    const uint32_t wx = w % fnx, wy = w / fnx;
    const size_t base = tile ? ((size_t)((wy >> sh) * tx + (wx >> sh)) << (2 * sh)) |
                                   ((wy & (T - 1)) << sh) | (wx & (T - 1))
                             : (size_t)w;
    const uint32_t s = cstart[w] + w, e = cstart[w + 1] + w;   // e: the sentinel
    wpts[e] = make_float4(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), -INFINITY,
                          __uint_as_float(0xFFFFFFFFu));
    // one pass down the run: jt / jb advance monotonically, each entry's z and coarse z cell
    // loaded once per pointer (the walk of every level reuses them)
    uint32_t jt = s, jb = s, j2 = s, j3 = s;
    float zt = wpts[s].z, zb = zt, zlast = zt, z2 = zt, z3 = zt;
    int ct = s < e ? cell_z(m, zt) : -1, cb = ct;
    for (int iz = (int)rz - 1; iz >= 0; --iz) {
        while (jt < e && ct > iz + 1) {
            ++jt;
            zt = wpts[jt].z;
            ct = jt < e ? cell_z(m, zt) : -1;
        }
        if (jb < jt) {
            jb = jt;
            zb = zt;
            cb = ct;
        }
        while (jb < e && cb >= iz) {
            zlast = zb;
            ++jb;
            zb = wpts[jb].z;
            cb = jb < e ? cell_z(m, zb) : -1;
        }
        uint32_t band = 0x00FFu;   // empty
        if (jb > jt) {
            const uint32_t code = zband_code(zt, zlast, m.oz + (double)iz * c, c);
            const uint32_t lo = code & 255u, hi = code >> 8;
            const uint32_t lo2 = (lo == 0u || lo <= tsteps) ? 0u : lo - tsteps;
            const uint32_t hi2 = (hi == 255u) ? 255u : min(hi + tsteps, 255u);
            band = lo2 | (hi2 << 8);
        }
        // split records: the entries from jt that lie at or above oz + (iz + 1.5) c (at most
        // 15 of them) can be skipped by a query more than r below that height (march, FN 8).
        // skip2: two thresholds, iz + 1.375 and iz + 1.6875 (exact in float), at most 15 and 7
        // entries, with a 25-bit start (build_fine: below 2^25 entries)
        uint32_t word = jt;
        if (tile == 2) {
            if (j2 < jt) {
                j2 = jt;
                z2 = zt;
            }
            const double h2 = m.oz + ((double)iz + (skip2 ? 1.375 : 1.5)) * c;
            while (j2 < e && (double)z2 >= h2) z2 = wpts[++j2].z;
            if (skip2) {
                if (j3 < jt) {
                    j3 = jt;
                    z3 = zt;
                }
                const double h3 = m.oz + ((double)iz + 1.6875) * c;
                while (j3 < e && (double)z3 >= h3) z3 = wpts[++j3].z;
                word = jt | (min(j2 - jt, 15u) << 25) | (min(j3 - jt, 7u) << 29);
            } else {
                word = jt | (min(j2 - jt, 15u) << 28);
            }
        }
        put((size_t)iz * plane + base, word, band);
    }
}

// Clearance codes of the empty split records (pcp_fan_clear.hpp, DESIGN.md §5 Skip 5), three
// passes.  lev[w]: the lowest level at which fine cell w's lowest point counts (preset to
// 0xFFFFFFFF: no point), one atomicMin per point.
__global__ void __launch_bounds__(kThreads)
k_clear_level(const float4 *__restrict__ pts, uint32_t n, FineGeo f, ClearGeo cg, int rz,
              uint32_t *__restrict__ lev) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    int cx, cy;
    fine_cell(f, p.x, p.y, cx, cy);
    atomicMin(&lev[(uint32_t)cx + (uint32_t)f.fnx * (uint32_t)cy],
              (uint32_t)fan_clear_level(cg, (double)p.z, rz));
}

// h[iz][w]: cells along y to the column's nearest cell occupied at level iz (lev <= iz), capped
// at 256.  One thread per cell for all its levels: the levels nest (a cell occupied at iz is
// occupied above it), so one walk outwards with the running minimum m of lev settles, at
// distance d, the levels [m, top) not settled nearer; it ends when level 0 is settled.
__global__ void __launch_bounds__(kThreads)
k_clear_col(const uint32_t *__restrict__ lev, int fnx, int fny, uint32_t nw, uint32_t rz,
            uint16_t *__restrict__ h) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= nw) return;
    const int x = (int)(w % (uint32_t)fnx), y = (int)(w / (uint32_t)fnx);
    uint32_t top = rz;   // the levels below top are not settled yet
    for (int d = 0; d <= kClearMax && top > 0u; ++d) {
        const int ya = y - d, yb = y + d;
        const uint32_t la = ya >= 0 ? lev[(size_t)ya * fnx + x] : 0xFFFFFFFFu;
        const uint32_t lb = yb < fny ? lev[(size_t)yb * fnx + x] : 0xFFFFFFFFu;
        const uint32_t m = min(la, lb);
        for (uint32_t iz = m; iz < top; ++iz) h[(size_t)iz * nw + w] = (uint16_t)d;
        top = min(top, m);
    }
    for (uint32_t iz = 0; iz < top; ++iz) h[(size_t)iz * nw + w] = (uint16_t)(kClearMax + 1);
}

// D = min over dx of max(h(x + dx), |dx|), the Chebyshev distance in cells to the nearest
// occupied cell, into the high byte of (w, iz)'s record when that record is empty.  The grid's
// outermost cells and levels keep 0 (fan_clear_border: what a clamped probe reads).
__global__ void __launch_bounds__(kThreads)
k_clear_code(const uint16_t *__restrict__ h, int fnx, int fny, uint32_t nw, uint32_t tx,
             size_t plane, uint16_t *__restrict__ fband) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x, iz = blockIdx.y;
    if (w >= nw) return;
    const uint32_t wx = w % (uint32_t)fnx, wy = w / (uint32_t)fnx;
    if (fan_clear_border(wx, wy, iz, (uint32_t)fnx, (uint32_t)fny, gridDim.y)) return;
    const size_t r = (size_t)iz * plane + (((size_t)((wy >> 3) * tx + (wx >> 3)) << 6) |
                                           ((wy & 7u) << 3) | (wx & 7u));
    if (fband[r] != 0x00FFu) return;
    const uint16_t *row = h + (size_t)iz * nw + (size_t)wy * fnx;
    int D = (int)row[wx];
    for (int d = 1; d < D; ++d) {
        const int xa = (int)wx - d, xb = (int)wx + d;
        if (xa >= 0) D = min(D, max((int)row[xa], d));
        if (xb < fnx) D = min(D, max((int)row[xb], d));
    }
    fband[r] = (uint16_t)(0x00FFu | (fan_clear_code((uint32_t)D) << 8));
}

// The tight twin of the split records' thresholds (pcp_fan_band.hpp, DESIGN.md §5 Skip 7), one
// thread per window after the clearance codes are in: `twin` starts as a copy of fband (empty
// records with their codes and padding records stay as they are), and every other record of the
// window is coded again from its entries -- k_frec's membership, the same two pointers down the
// run -- each entry widening the band by its reach over the cell.
__global__ void __launch_bounds__(kThreads)
k_band_tight(const float4 *__restrict__ wpts, const uint32_t *__restrict__ cstart, CellMap m,
             FineGeo f, double c, double qm, double rho, uint32_t rz, uint32_t tx, size_t plane,
             const uint16_t *__restrict__ fband, uint16_t *__restrict__ twin) {
    const uint32_t nw = (uint32_t)f.fnx * (uint32_t)f.fny, w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= nw) return;
    const uint32_t wx = w % (uint32_t)f.fnx, wy = w / (uint32_t)f.fnx;
    const size_t base = ((size_t)((wy >> 3) * tx + (wx >> 3)) << 6) | ((wy & 7u) << 3) | (wx & 7u);
    const uint32_t s = cstart[w] + w, e = cstart[w + 1] + w;   // e: the sentinel
    uint32_t jt = s, jb = s;
    int ct = s < e ? cell_z(m, wpts[s].z) : -1, cb = ct;
    const double step = (double)kZq * c;
    for (int iz = (int)rz - 1; iz >= 0; --iz) {
        while (jt < e && ct > iz + 1) {
            ++jt;
            ct = jt < e ? cell_z(m, wpts[jt].z) : -1;
        }
        if (jb < jt) {
            jb = jt;
            cb = ct;
        }
        while (jb < e && cb >= iz) {
            ++jb;
            cb = jb < e ? cell_z(m, wpts[jb].z) : -1;
        }
        const size_t r = (size_t)iz * plane + base;
        const uint32_t spec = fband[r];
        if (jb == jt || (spec & 255u) == 255u) continue;   // empty: the copy stands
        BandAcc a = fan_band_begin();
        for (uint32_t j = jt; j < jb; ++j) {
            const float4 p = wpts[j];
            fan_band_add(a, (double)p.z,
                         fan_band_dist(f.ox, f.oy, f.cf, (int)wx, (int)wy, (double)p.x, (double)p.y),
                         qm, rho);
        }
        twin[r] = (uint16_t)fan_band_word(a, m.oz + (double)iz * c, step, spec);
    }
}

// The pivot table (pcp_fan_pivot.hpp, DESIGN.md §5 Skip 6), one thread per slot of the padded
// 8 x 8 tile plane: the window's member nearest its cell's centre in xy, from the float4 entries
// (their w still carries the original index), or the sentinel for an empty window or a padding
// slot, as a 12-byte (x, y, z) record.
__global__ void __launch_bounds__(kThreads)
k_pivot(const float4 *__restrict__ wpts, const uint32_t *__restrict__ cstart, FineGeo f,
        uint32_t tx, uint32_t nslot, float *__restrict__ piv) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nslot) return;
    const uint32_t tile = t >> 6, sub = t & 63u;
    const uint32_t wx = (tile % tx) * 8u + (sub & 7u), wy = (tile / tx) * 8u + (sub >> 3);
    float3 best = make_float3(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), -INFINITY);
    if (wx < (uint32_t)f.fnx && wy < (uint32_t)f.fny) {
        const uint32_t w = wx + (uint32_t)f.fnx * wy;
        const uint32_t s = cstart[w] + w, e = cstart[w + 1] + w;
        PivotKey kb{};
        for (uint32_t j = s; j < e; ++j) {
            const float4 p = wpts[j];
            const PivotKey k{pivot_d2(f.ox, f.oy, f.cf, wx, wy, p.x, p.y), p.z,
                             __float_as_uint(p.w)};
            if (j == s || pivot_better(k, kb)) {
                kb = k;
                best = make_float3(p.x, p.y, p.z);
            }
        }
    }
    float *o = piv + 3 * (size_t)t;   // (t = pivot_index(tx, wx, wy))
    o[0] = best.x;
    o[1] = best.y;
    o[2] = best.z;
}

// the fine-window entries packed to 12 bytes (x, y, z): a quarter less working set for the walks
__global__ void __launch_bounds__(kThreads)
k_pack3(const float4 *__restrict__ src, uint32_t n, float *__restrict__ dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = src[i];
    dst[3 * (size_t)i] = p.x;
    dst[3 * (size_t)i + 1] = p.y;
    dst[3 * (size_t)i + 2] = p.z;
}

// Everything the build's kernels receive as a parameter, from the index and the knobs alone (the
// read-back, pcp_debug_fine_copy, reports the same values for a built copy).
struct FinePlan {
    CellMap m;
    FineGeo f;
    ClearGeo cg;
    int F, tile;
    uint64_t fnx, fny, rz, nw, nrec;
    uint64_t npiv;   // slots of the pivot table: the padded 8 x 8 tile plane (tile 2 only)
    size_t band_bytes, rec_bytes;
    uint32_t tsteps;
};

FinePlan fine_plan(const GridIndex &g, int F, int tile) {
    FinePlan p{};
    const GridView gv = g.view();
    p.m = CellMap{gv.ox, gv.oy, gv.oz, gv.inv_c, g.nx, g.ny, g.nz};
    p.F = F;
    p.tile = tile;
    p.fnx = (uint64_t)F * g.nx;
    p.fny = (uint64_t)F * g.ny;
    p.rz = (uint64_t)(g.nz > 1 ? g.nz - 1 : 0);
    const uint64_t T = tile == 2 ? 8 : 4;
    p.nrec = tile ? ((p.fnx + T - 1) / T) * ((p.fny + T - 1) / T) * T * T * p.rz
                  : p.fnx * p.fny * p.rz;
    p.nw = p.fnx * p.fny;   // windows (the runs)
    p.npiv = tile == 2 ? (uint64_t)pivot_tiles((uint32_t)p.fnx) * pivot_tiles((uint32_t)p.fny) * 64
                       : 0;
    p.band_bytes = ((size_t)p.nrec * 2 + 255) & ~(size_t)255;
    p.rec_bytes = tile == 2 ? p.band_bytes + (size_t)p.nrec * 4 : (size_t)p.nrec * sizeof(uint2);
    p.f.ox = gv.ox;
    p.f.oy = gv.oy;
    p.f.cf = g.c / F;
    p.f.inv_cf = F * gv.inv_c;
    const double R = g.r_q + kQueryMargin;
    p.f.R2 = R * R;
    p.f.fnx = (int32_t)p.fnx;
    p.f.fny = (int32_t)p.fny;
    p.f.reach = (int32_t)std::ceil(R / p.f.cf);
    p.tsteps = (uint32_t)std::ceil((g.r_q + 2e-3) / g.c / (double)kZq);
    const double zabs = std::fmax(std::fabs(gv.oz), std::fabs(gv.oz + (double)g.nz * g.c));
    p.cg = fan_clear_geo(gv.oz, g.c, R, zabs);
    return p;
}

}  // namespace

int build_fine(pcp_ctx *ctx, GridIndex &g) {
    if (g.fine_ok || g.fine_fail || !g.present || !g.occz_ok || g.n_pts == 0) return PCP_OK;
    hipStream_t st = ctx->stream;
    ProfScope prof(ctx, PCP_K_INDEX_BUILD);
    const FinePlan plan = fine_plan(g, std::max(2, std::min(ctx->knob.terrain_fine, 8)),
                                    ctx->knob.fine_tile == 2 ? 2 : ctx->knob.fine_tile ? 1 : 0);
    const CellMap m = plan.m;
    const FineGeo f = plan.f;
    const int F = plan.F, tile = plan.tile;
    const uint64_t fnx = plan.fnx, fny = plan.fny, rz = plan.rz, nrec = plan.nrec, nw = plan.nw;
    const size_t band_bytes = plan.band_bytes, rec_bytes = plan.rec_bytes;
    // caps: 32-bit record byte offsets (< 2^29 records), 24-bit probe multiplies, window keys
    if (rz == 0 || nrec >= (1ull << 29) || fnx >= (1ull << 24) || fny * rz >= (1ull << 24)) {
        g.fine_fail = true;
        return PCP_OK;
    }
    const uint32_t n = (uint32_t)g.n_pts;
    const unsigned gridn = (n + kThreads - 1) / kThreads;
    const float4 *pts = g.pts.as<const float4>();
    // 1. global z order
    size_t t1 = 0, t2 = 0;
    // rocPRIM's onesweep radix sort, called directly (no CUB-compatibility layer)
    (void)rocprim::radix_sort_pairs(nullptr, t1, (unsigned long long *)nullptr,
                                    (unsigned long long *)nullptr, (uint32_t *)nullptr,
                                    (uint32_t *)nullptr, n, 0u, 64u, st);
    PCP_HIP(ctx, ctx->scratch[2].ensure((size_t)n * 24 + 64));   // keys x2, vals x2
    unsigned long long *k0 = ctx->scratch[2].as<unsigned long long>(), *k1 = k0 + n;
    uint32_t *v0 = reinterpret_cast<uint32_t *>(k1 + n), *zord = v0 + n;
    hipLaunchKernelGGL(k_zkeys, dim3(gridn), dim3(kThreads), 0, st, pts, n, k0, v0);
    PCP_CHECK_LAUNCH(ctx);
    // 2. windows per point (pcount); points per window come from the sorted pairs (step 4)
    PCP_HIP(ctx, ctx->scratch[3].ensure((size_t)(n + 1) * 8 + (nw + 1) * 4 + 64));
    uint32_t *pcount = ctx->scratch[3].as<uint32_t>(), *poff = pcount + (n + 1);
    uint32_t *cstart = poff + (n + 1);
    // 3. scans
    const size_t tscan = scan_tmp_bytes(std::max<uint64_t>(n, nw)) +
                         (std::max<uint64_t>(n, nw) + 1) * sizeof(uint32_t);
    PCP_HIP(ctx, ctx->scratch[4].ensure(std::max(t1, tscan) + 256));
    if (rocprim::radix_sort_pairs(ctx->scratch[4].p, t1, k0, k1, v0, zord, n, 0u, 64u, st) !=
        hipSuccess)
        return set_err(ctx, PCP_E_HIP, "build_fine: z sort failed");
    hipLaunchKernelGGL(k_win_count, dim3(gridn), dim3(kThreads), 0, st, pts, zord, n, f, pcount);
    PCP_CHECK_LAUNCH(ctx);
    int rc = exclusive_scan_u32(ctx, pcount, poff, n, ctx->scratch[4].p);
    if (rc) return rc;
    uint32_t np = 0;
    if ((rc = read_small(ctx, &np, poff + n, 4, st))) return rc;
    // entries = pairs + one sentinel per window, addressed with 32-bit indices (<< 4 bytes)
    if (np == 0 || (uint64_t)np + nw >= (1ull << 28)) {
        g.fine_fail = true;
        return PCP_OK;
    }
    // 4. pairs (window, z rank), stable sort by window
    int wbits = 1;
    while ((1ull << wbits) < nw) ++wbits;
    (void)rocprim::radix_sort_pairs(nullptr, t2, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (uint32_t *)nullptr, np, 0u,
                                    (unsigned)wbits, st);
    PCP_HIP(ctx, ctx->scratch[5].ensure((size_t)np * 16 + 64));
    uint32_t *wk0 = ctx->scratch[5].as<uint32_t>(), *wk1 = wk0 + np, *rk0 = wk1 + np,
             *rk1 = rk0 + np;
    PCP_HIP(ctx, ctx->scratch[6].ensure(t2 + 256));
    hipLaunchKernelGGL(k_win_emit, dim3(gridn), dim3(kThreads), 0, st, pts, zord, n, f,
                       (const uint32_t *)poff, wk0, rk0);
    PCP_CHECK_LAUNCH(ctx);
    if (rocprim::radix_sort_pairs(ctx->scratch[6].p, t2, wk0, wk1, rk0, rk1, np, 0u,
                                  (unsigned)wbits, st) != hipSuccess)
        return set_err(ctx, PCP_E_HIP, "build_fine: window sort failed");
    hipLaunchKernelGGL(k_win_bounds, dim3((unsigned)((nw + kThreads) / kThreads)), dim3(kThreads),
                       0, st, (const uint32_t *)wk1, np, (uint32_t)nw, cstart);
    PCP_CHECK_LAUNCH(ctx);
    // the copy is an optional speed-up: an allocation failure keeps the other layouts
    const size_t nent = (size_t)np + nw;
    const bool pack = ctx->knob.fine_pack != 0;
    // the pivot table goes with the split records; its 12-byte records are addressed with
    // 32-bit byte offsets (a plane past 2^28 cells keeps the copy and goes without)
    const bool pivots = tile == 2 && plan.npiv < (1ull << 28);
    // packed: the float4 entries are built in scratch, then packed into wpts.  The packed array
    // keeps kWalkPairSlack bytes behind its last entry (the last window's sentinel): the paired
    // walk loads one entry behind the one it tests, 12 bytes of slack per extra entry loaded
    // (pcp_walk_pair.hpp)
    if ((pack && ctx->scratch[7].ensure(nent * sizeof(float4)) != hipSuccess) ||
        g.wpts.ensure(pack ? nent * kWalkEntryBytes + kWalkPairSlack
                           : nent * sizeof(float4)) != hipSuccess ||
        g.frec.ensure(rec_bytes) != hipSuccess ||
        (pivots && g.fpiv.ensure(plan.npiv * kPivotBytes + 16) != hipSuccess)) {
        (void)hipGetLastError();
        g.wpts.release();
        g.frec.release();
        g.fpiv.release();
        g.fine_fail = true;
        return PCP_OK;
    }
    float4 *went = pack ? ctx->scratch[7].as<float4>() : g.wpts.as<float4>();
    hipLaunchKernelGGL(k_win_place, dim3((np + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                       pts, (const uint32_t *)zord, (const uint32_t *)wk1, (const uint32_t *)rk1,
                       np, went);
    PCP_CHECK_LAUNCH(ctx);
    // 5. records (and the sentinels), one thread per window; two skip thresholds need a 25-bit
    // walk start
    const bool skip2 = tile == 2 && ctx->knob.fine_skip == 2 && nent < (1ull << 25);
    const uint32_t tsteps = plan.tsteps;
    const uint64_t nthr = std::max<uint64_t>(nw, tile ? nrec / rz : 0);
    hipLaunchKernelGGL(k_frec, dim3((unsigned)((nthr + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       st, went, (const uint32_t *)cstart, m, g.c, (uint32_t)fnx,
                       (uint32_t)fny, (uint32_t)rz, tsteps, tile, skip2 ? 1 : 0,
                       g.frec.as<uint2>(),
                       g.frec.as<uint16_t>(),
                       reinterpret_cast<uint32_t *>(g.frec.as<char>() + band_bytes));
    PCP_CHECK_LAUNCH(ctx);
    if (pivots) {
        // the pivots, while the entries still carry their original index (the packing drops it)
        hipLaunchKernelGGL(k_pivot, dim3((unsigned)((plan.npiv + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, (const float4 *)went, (const uint32_t *)cstart,
                           f, pivot_tiles((uint32_t)fnx), (uint32_t)plan.npiv,
                           g.fpiv.as<float>());
        PCP_CHECK_LAUNCH(ctx);
    }
    if (tile == 2) {
        // clearance codes into the empty records (their high byte; the table does not grow)
        const size_t lev_bytes = ((size_t)nw * 4 + 255) & ~(size_t)255;
        PCP_HIP(ctx, ctx->scratch[5].ensure(lev_bytes + (size_t)nw * rz * 2 + 64));
        uint32_t *lev = ctx->scratch[5].as<uint32_t>();
        uint16_t *hcol = reinterpret_cast<uint16_t *>(ctx->scratch[5].as<char>() + lev_bytes);
        const ClearGeo cg = plan.cg;
        PCP_HIP(ctx, hipMemsetAsync(lev, 0xFF, (size_t)nw * 4, st));
        hipLaunchKernelGGL(k_clear_level, dim3(gridn), dim3(kThreads), 0, st, pts, n, f, cg,
                           (int)rz, lev);
        PCP_CHECK_LAUNCH(ctx);
        const dim3 cgrid((unsigned)((nw + kThreads - 1) / kThreads), (unsigned)rz);
        hipLaunchKernelGGL(k_clear_col, dim3(cgrid.x), dim3(kThreads), 0, st,
                           (const uint32_t *)lev, (int)fnx, (int)fny, (uint32_t)nw, (uint32_t)rz,
                           hcol);
        PCP_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_clear_code, cgrid, dim3(kThreads), 0, st, (const uint16_t *)hcol,
                           (int)fnx, (int)fny, (uint32_t)nw, (uint32_t)((fnx + 7) / 8), (size_t)(nrec / rz),
                           g.frec.as<uint16_t>());
        PCP_CHECK_LAUNCH(ctx);
        // the tight twin of the thresholds (Skip 7); without its allocation the march reads the
        // specified ones
        g.fband_ok = false;
        if (g.fband2.ensure(band_bytes) == hipSuccess) {
            PCP_HIP(ctx, hipMemcpyAsync(g.fband2.p, g.frec.p, band_bytes, hipMemcpyDeviceToDevice,
                                        st));
            hipLaunchKernelGGL(k_band_tight, dim3(cgrid.x), dim3(kThreads), 0, st,
                               (const float4 *)went, (const uint32_t *)cstart, m, f, g.c,
                               kQueryMargin, g.r_q + kBandMu, (uint32_t)rz,
                               (uint32_t)((fnx + 7) / 8), (size_t)(nrec / rz),
                               g.frec.as<const uint16_t>(), g.fband2.as<uint16_t>());
            PCP_CHECK_LAUNCH(ctx);
            g.fband_ok = true;
        } else {
            (void)hipGetLastError();
            g.fband2.release();
        }
    }
    if (pack) {
        hipLaunchKernelGGL(k_pack3, dim3((unsigned)((nent + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, (const float4 *)went, (uint32_t)nent,
                           g.wpts.as<float>());
        PCP_CHECK_LAUNCH(ctx);
    }
    g.wpack = pack ? 1 : 0;
    g.frx = (uint32_t)fnx;
    g.fry = (uint32_t)fny;
    g.frz = (uint32_t)rz;
    g.ffine = (float)F;
    g.ftile = tile;
    g.fskip = skip2 ? 2 : 1;
    g.fstart_off = tile == 2 ? band_bytes : 0;
    g.fnent = nent;
    g.fpiv_ok = pivots;
    g.fine_ok = true;
    return PCP_OK;
}

}  // namespace pcp

// Test infrastructure (tests/test_fine_copy_gpu.py): the terrain's built fine copy as it lies on
// the device, with every parameter its build kernels received.  No launch and no build: the
// stream is drained, then plain copies.
extern "C" int pcp_debug_fine_copy(pcp_ctx *ctx, pcp_fine_geo *geo, void *frec,
                                   uint64_t frec_cap, void *wpts, uint64_t wpts_cap, void *pts,
                                   uint64_t pts_cap) {
    using namespace pcp;
    if (!ctx || !geo) return PCP_E_INVALID;
    const GridIndex &g = ctx->terrain;
    *geo = pcp_fine_geo{};
    if (!g.present || !g.fine_ok) return PCP_OK;   // built = 0
    const FinePlan p = fine_plan(g, (int)g.ffine, g.ftile);
    geo->built = 1;
    geo->tile = g.ftile;
    geo->skip = g.fskip;
    geo->packed = g.wpack;
    geo->nx = g.nx;
    geo->ny = g.ny;
    geo->nz = g.nz;
    geo->F = p.F;
    geo->reach = p.f.reach;
    geo->fnx = p.f.fnx;
    geo->fny = p.f.fny;
    geo->rz = (int32_t)p.rz;
    geo->tsteps = (int32_t)p.tsteps;
    geo->n_points = g.n_pts;
    geo->n_records = p.nrec;
    geo->n_entries = g.fnent;
    geo->start_off = g.fstart_off;
    geo->frec_bytes = p.rec_bytes;
    geo->wpts_bytes = g.fnent * (g.wpack ? 12u : 16u);
    geo->pts_bytes = g.n_pts * sizeof(float4);
    geo->ox = p.m.ox;
    geo->oy = p.m.oy;
    geo->oz = p.m.oz;
    geo->c = g.c;
    geo->inv_c = p.m.inv_c;
    geo->r_q = g.r_q;
    geo->cf = p.f.cf;
    geo->inv_cf = p.f.inv_cf;
    geo->R2 = p.f.R2;
    geo->zq = (double)kZq;
    geo->clear_zt0 = p.cg.zt0;
    geo->clear_c = p.cg.c;
    if (!frec && !wpts && !pts) return PCP_OK;     // the sizes only
    if ((frec && frec_cap < geo->frec_bytes) || (wpts && wpts_cap < geo->wpts_bytes) ||
        (pts && pts_cap < geo->pts_bytes))
        return set_err(ctx, PCP_E_CAPACITY, "pcp_debug_fine_copy: a buffer is too small");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (frec) PCP_HIP(ctx, hipMemcpy(frec, g.frec.p, geo->frec_bytes, hipMemcpyDeviceToHost));
    if (wpts) PCP_HIP(ctx, hipMemcpy(wpts, g.wpts.p, geo->wpts_bytes, hipMemcpyDeviceToHost));
    if (pts) PCP_HIP(ctx, hipMemcpy(pts, g.pts.p, geo->pts_bytes, hipMemcpyDeviceToHost));
    return PCP_OK;
}

// Test infrastructure (tests/test_fan_pivot.py): the pivot table as it lies on the device.
extern "C" int pcp_debug_fine_pivot(pcp_ctx *ctx, pcp_fine_pivot_geo *geo, void *piv,
                                    uint64_t piv_cap) {
    using namespace pcp;
    if (!ctx || !geo) return PCP_E_INVALID;
    const GridIndex &g = ctx->terrain;
    *geo = pcp_fine_pivot_geo{};
    if (!g.present || !g.fine_ok || !g.fpiv_ok) return PCP_OK;   // built = 0
    const FinePlan p = fine_plan(g, (int)g.ffine, g.ftile);
    geo->built = 1;
    geo->enabled = ctx->knob.fan_pivot ? 1 : 0;
    geo->fnx = p.f.fnx;
    geo->fny = p.f.fny;
    geo->tx = (int32_t)pivot_tiles((uint32_t)p.fnx);
    geo->ty = (int32_t)pivot_tiles((uint32_t)p.fny);
    geo->n_slots = p.npiv;
    geo->bytes = p.npiv * kPivotBytes;
    geo->ox = p.f.ox;
    geo->oy = p.f.oy;
    geo->cf = p.f.cf;
    if (!piv) return PCP_OK;   // the sizes only
    if (piv_cap < geo->bytes)
        return set_err(ctx, PCP_E_CAPACITY, "pcp_debug_fine_pivot: the buffer is too small");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCP_HIP(ctx, hipMemcpy(piv, g.fpiv.p, geo->bytes, hipMemcpyDeviceToHost));
    return PCP_OK;
}

// Test infrastructure (tests/test_fan_band.py): the thresholds' tight twin as it lies on the
// device, the bytes of the split records' threshold array (pcp_debug_fine_copy's geometry
// describes both).  *bytes: the array's size, 0 when no twin is built; *enabled: the march reads
// it (PCP_FAN_BAND).
extern "C" int pcp_debug_fine_band(pcp_ctx *ctx, uint64_t *bytes, int32_t *enabled, void *band,
                                   uint64_t band_cap) {
    using namespace pcp;
    if (!ctx || !bytes) return PCP_E_INVALID;
    const GridIndex &g = ctx->terrain;
    *bytes = 0;
    if (enabled) *enabled = ctx->knob.fan_band ? 1 : 0;
    if (!g.present || !g.fine_ok || !g.fband_ok) return PCP_OK;
    const FinePlan p = fine_plan(g, (int)g.ffine, g.ftile);
    *bytes = (uint64_t)p.nrec * 2;
    if (!band) return PCP_OK;   // the size only
    if (band_cap < *bytes)
        return set_err(ctx, PCP_E_CAPACITY, "pcp_debug_fine_band: the buffer is too small");
    PCP_HIP(ctx, hipSetDevice(ctx->device));
    PCP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PCP_HIP(ctx, hipMemcpy(band, g.fband2.p, *bytes, hipMemcpyDeviceToHost));
    return PCP_OK;
}
