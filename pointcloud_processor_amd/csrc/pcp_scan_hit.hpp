// The hit search of a blocked ray: what k_scan_resolve (pcp_scan.hip) and
// k_cover_resolve (pcp_cover.hip) share, so that the terrain point a placement counts is the point
// the simulated scan reports, bit for bit.  The march's query point of sample k, the stencil
// corner, the eight cell runs of the cell-major copy (descending z per run: a point r below q ends
// the run) and the (acc, input index) minimum over the points within r.
//
// Numerics: no contraction, as everywhere -- the query point is the march's own
// float(p + d * s_k); the including source sets `#pragma clang fp contract(off)`.
#pragma once

#include "pcp_fan_dir.hpp"
#include "pcp_fan_row.hpp"
#include "pcp_internal.hpp"
#include "pcp_stencil.hpp"

namespace pcp {

// the query's tables, as fan_enqueue left them on the device
struct ScanHitQuery {
    GridView g;
    const double *ca, *sa, *ce, *se;
    const double *pose;                  // P x kFanRow, pcp_fan_row.hpp's rows
                                         // (MT: P x kFanDirRow, pcp_fan_dir.hpp's rows)
    const double *steps;
    int n_az;
    float r2;
};

// idx ~0: no point within r (the march excludes it for a blocked sample)
struct ScanHit {
    uint32_t idx;
    float x, y, z;        // the hit point's own bits
    double px, py, pz;    // the pose's position
};

#if defined(__HIPCC__)
// the hit point of ray `ray` of pose p whose first blocked sample is k >= 0
// MT: a mounted query -- the direction is the mounted march's own fan_dir() (pcp_fan_dir.hpp).
template <bool MT>
__device__ __forceinline__ ScanHit scan_hit(const ScanHitQuery &a, uint32_t p, uint32_t ray,
                                            int k) {
    // the march's q_k (fan_body, march)
    const uint32_t j = ray / (uint32_t)a.n_az, i = ray - j * (uint32_t)a.n_az;
    const double cej = a.ce[j];
    const double lx = cej * a.ca[i], ly = cej * a.sa[i], lz = a.se[j];
    const double *Pq = a.pose + (MT ? kFanDirRow : kFanRow) * (size_t)p;
    const double px = Pq[0], py = Pq[1], pz = Pq[2];
    double dx, dy, dz;
    if (MT) {
        const FanDir d = fan_dir(Pq, lx, ly, lz);
        dx = d.x;
        dy = d.y;
        dz = d.z;
    } else {
        const double cy = Pq[FR_CY], sy = Pq[FR_SY];
        dx = cy * lx - sy * ly;
        dy = sy * lx + cy * ly;
        dz = lz;
    }
    const double s = a.steps[k];
    const float qx = (float)(px + dx * s);
    const float qy = (float)(py + dy * s);
    const float qz = (float)(pz + dz * s);
    float best = 0.0f;
    uint32_t bidx = 0xFFFFFFFFu;
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
    // one point against the running (acc, input index) minimum; true: the point lies r or more
    // below q, so every later point of its run does too
    auto take = [&](const float4 &v) {
        const float d0 = qx - v.x, d1 = qy - v.y, d2 = qz - v.z;
        float acc = 0.0f;
        acc = acc + d0 * d0;
        acc = acc + d1 * d1;
        acc = acc + d2 * d2;
        const uint32_t vi = __float_as_uint(v.w);
        if (acc < a.r2 && (bidx == 0xFFFFFFFFu || acc < best || (acc == best && vi < bidx))) {
            best = acc;
            bidx = vi;
            bx = v.x;
            by = v.y;
            bz = v.z;
        }
        return d2 >= 0.0f && d2 * d2 >= a.r2;
    };
    uint32_t ix, iy, iz;
    if (stencil_cell3_fb(a.g, qx, qy, qz, ix, iy, iz)) {
        const uint32_t nx = (uint32_t)a.g.nx, nxy = nx * (uint32_t)a.g.ny;
        const uint32_t lin = ix + nx * iy + nxy * iz;
        // (the rounds of independent loads the march's scan_stencil issues -- all eight first
        // points at once, or the eight runs in lockstep -- measured the same 133 us here: the
        // kernel is bound by the number of point gathers, not by their latency)
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            // cells c, c + 1 of one stencil row and the end of c + 1 in one directory load
            const U3 u = ld_u3o(a.g.start, lin + (uint32_t)(r & 1) * nx + (uint32_t)(r >> 1) * nxy);
            for (uint32_t t = u.a; t < u.b; ++t)
                if (take(a.g.pts[t])) break;
            for (uint32_t t = u.b; t < u.c; ++t)
                if (take(a.g.pts[t])) break;
        }
    }
    return ScanHit{bidx, bx, by, bz, px, py, pz};
}
#endif

// the query's tables on the host side: the context's cached fan tables, staged poses and step table
// (valid behind a fan_enqueue of the same fan on ctx->stream)
inline ScanHitQuery scan_hit_query(pcp_ctx *ctx, const pcp_fan_params *fan) {
    ScanHitQuery q{};
    if (ctx->terrain.present) q.g = ctx->terrain.view(ctx->knob);
    const double *tab = ctx->fan_tab.as<const double>();
    q.ca = tab;
    q.sa = tab + fan->n_az;
    q.ce = tab + 2 * fan->n_az;
    q.se = tab + 2 * fan->n_az + fan->n_el;
    q.pose = ctx->poses_d.as<const double>();
    q.steps = ctx->steps_d.as<const double>();
    q.n_az = fan->n_az;
    q.r2 = (float)(kRayRadius * kRayRadius);
    return q;
}

}  // namespace pcp
